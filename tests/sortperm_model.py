"""TEST INFRASTRUCTURE: the selection's sort as plain Python over an index list - klib's introsort (ksort.h:110-160) as hao_intro_sort
(hifiasm_amd/csrc/hao_chain.cuh) restates it: median of three, Hoare partition with the pivot parked at t, sub-ranges of at most 16 elements left
to ONE closing insertion sort, combsort once the depth budget of a sub-range is used up.  Besides the permutation it says which of the device
sorts' paths a key array exercises (tests/test_sortperm_cpu.py checks that tests/golden/sortperm.npz holds every kind)."""


def sort_keys(mode, xs, sc):
    """order-preserving integer keys: mode 0 = score descending (oreg_ss_lt), mode 1 = (x_pos_s << 32 | x_pos_e) ascending (oreg_xs_lt)"""
    return [-int(v) for v in sc] if mode == 0 else [int(v) for v in xs]


def _ins_sort(K, P, lo, hi):
    for i in range(lo + 1, hi):
        j = i
        while j > lo and K[j] < K[j - 1]:
            K[j], K[j - 1] = K[j - 1], K[j]; P[j], P[j - 1] = P[j - 1], P[j]
            j -= 1


def _comb_sort(K, P, lo, n):
    shrink = 1.2473309501039786540366528676643
    gap = n
    while True:
        if gap > 2:
            gap = int(gap / shrink)
            if gap == 9 or gap == 10:
                gap = 11
        swapped = False
        for i in range(lo, lo + n - gap):
            if K[i + gap] < K[i]:
                K[i], K[i + gap] = K[i + gap], K[i]; P[i], P[i + gap] = P[i + gap], P[i]
                swapped = True
        if not (swapped or gap > 2):
            break
    if gap != 1:
        _ins_sort(K, P, lo, lo + n)


def intro_sort(keys):
    """keys: integers, sorted ascending with klib's tie order.  Returns (perm, info): perm[i] = input index of the element at slot i;
    info = {"widest": most sub-ranges of more than 16 elements alive in one level of the recursion (the root counts as one),
            "comb": times combsort was entered, "far": the closing insertion sort moves an element by more than 16 slots}"""
    n = len(keys)
    K = list(keys); P = list(range(n))
    info = {"widest": 0, "comb": 0, "far": False}
    if n < 1:
        return P, info
    if n == 2:
        if K[1] < K[0]:
            K[0], K[1] = K[1], K[0]; P[0], P[1] = P[1], P[0]
        return P, info
    d = 2
    while (1 << d) < n:
        d += 1
    d <<= 1
    d0 = d
    width = {}
    stack = []
    s, t = 0, n - 1
    first = True
    while True:
        if s < t:
            if first or t - s + 1 > 16:      # (the root is listed whatever its size; every other range here has more than 16 elements)
                width[d0 - d] = width.get(d0 - d, 0) + 1
            first = False
            d -= 1
            if d == 0:
                info["comb"] += 1
                _comb_sort(K, P, s, t - s + 1)
                t = s
                continue
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if K[k] < K[i]:
                if K[k] < K[j]:
                    k = j
            else:
                k = i if K[j] < K[i] else j
            if k != t:
                K[k], K[t] = K[t], K[k]; P[k], P[t] = P[t], P[k]
            rp = K[t]
            while True:
                i += 1
                while K[i] < rp:
                    i += 1
                j -= 1
                while i <= j and rp < K[j]:
                    j -= 1
                if j <= i:
                    break
                K[i], K[j] = K[j], K[i]; P[i], P[j] = P[j], P[i]
            K[i], K[t] = K[t], K[i]; P[i], P[t] = P[t], P[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
        else:
            if not stack:
                break
            s, t, d = stack.pop()
    info["widest"] = max(width.values(), default=0)
    before = list(P)
    _ins_sort(K, P, 0, n)
    at = {p: i for i, p in enumerate(before)}
    info["far"] = any(abs(i - at[p]) > 16 for i, p in enumerate(P))
    return P, info

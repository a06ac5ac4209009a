"""The arena of a streamed batch (include/hao.h: hao_overlap_batch_async, hao_deliver_wait, hao_deliver_ed / _trace / _rescue / _wlist), as a caller sees it
through the views alone.  For reads [2, n - 1) of the small HiFi set and for one empty batch, in four combinations of parts:
  * `bytes` is the sum hao.h documents, computed here from the views' own counts and the sizes of the structures that travel - bytes copied, not padded regions;
  * the view pointers lie in the documented section order, each region starts 64-byte aligned where the previous one ends (so none overlaps the next), a
    region of no bytes takes no room;
  * a part the batch did not ask for has null pointers in the main view and no view of its own (HAO_EINVAL from its getter);
  * the empty batch has 0 bytes and null pointers everywhere, and the ED view of a batch that asked for ED still names its window."""
import ctypes as C

import numpy as np
import pytest

from helpers import scenario_reads

pytestmark = pytest.mark.gpu


# the records of include/hao.h that travel and that hifiasm_amd/api.py reads as plain arrays
class _Wire(C.Structure):      # hao_ovlp_wire_t
    _fields_ = [(k, C.c_uint32) for k in ("y", "x_pos_s", "x_pos_e", "y_pos_s", "y_pos_e")] + [("shared_seed", C.c_int32), ("non_homopolymer_errors", C.c_uint32), ("fc_len", C.c_uint32)]


class _Qmz(C.Structure):       # hao_qmz_t
    _fields_ = [("self_offset", C.c_uint32), ("cnt", C.c_uint32)]


class _Exc(C.Structure):       # hao_exc_t (its hit: hao_hit_t, four 32-bit words)
    _fields_ = [("index", C.c_uint64), ("q", C.c_uint32), ("pad", C.c_uint32), ("hit", C.c_uint32 * 4)]


class _EdOvlp(C.Structure):    # hao_ed_ovlp_t
    _fields_ = [(k, C.c_uint32) for k in ("n_win", "n_aligned", "aligned_bases", "err_sum")]


class _Win(C.Structure):       # hao_rescue_win_t, hao_wlist_win_t
    _fields_ = [("y_start", C.c_int32), ("y_end", C.c_int32), ("win", C.c_uint32), ("info", C.c_uint32)]


OL, CL, EXACT, ED, TRACE, RESCUE, WLIST = 1, 2, 4, 8, 16, 32, 64
CASES = {"ol": (OL, None), "ol_cl_exact": (OL | CL | EXACT, None), "diag_trace": (OL | CL | EXACT | ED | TRACE, ("diag", 375, 15)),
         "ref_wlist": (OL | CL | EXACT | ED | RESCUE | WLIST, ("ref", 775, 0.004))}


@pytest.fixture(scope="module")
def eng():
    from hifiasm_amd.api import Engine
    rs, okw = scenario_reads("hifi")
    e = Engine(0, **okw)
    e.set_readset(rs); e.ha_ft_gen(); e.ha_pt_gen()
    yield e, rs
    e.close()


def _sections(d, parts):
    """(name, pointer, bytes of the region, bytes copied) of every section of the batch's arena in the documented order, and the parts' counts that were checked"""
    from hifiasm_amd.api import ChainHdr, RESCUE_OVLP, _arr
    n, n_ol = int(d.n_reads), int(d.n_ol)
    S = []

    def put(name, ptr, region, copied=None):
        S.append((name, ptr or 0, int(region), int(region if copied is None else copied)))
    if parts & OL:
        put("ol_off", d.ol_off, (n + 1) * 8); put("ol", d.ol, n_ol * C.sizeof(_Wire))
        put("fc_off", d.fc_off, (n_ol + 1) * 8, n_ol * 8)                        # (the last word is the host's: room for it, no copy of it)
        put("fc", d.fc, int(d.n_fc) * 4)
    if parts & CL:
        n_mz = int(_arr(d.qm_off, n + 1, np.uint64)[n])
        nw = (int(d.n_pos) + 63) // 64
        for k in ("ch_off", "cl_off", "qm_off"):
            put(k, getattr(d, k), (n + 1) * 8)
        put("hdr", d.chains, int(d.n_chains) * C.sizeof(ChainHdr))
        if d.qmz_pos:
            assert not d.qmz and d.qmz_cnt
            put("qmz_pos", d.qmz_pos, n_mz * 2); put("qmz_cnt", d.qmz_cnt, n_mz * 2)
        else:
            assert d.qmz and not d.qmz_cnt
            put("qmz", d.qmz, n_mz * C.sizeof(_Qmz))
        put("bits", d.cl_bits, nw * 8); put("rank", d.cl_rank, (nw // 4 + 1) * 4); put("codes", d.cl_codes, int(d.n_codes)); put("exc", d.cl_exc, int(d.n_exc) * C.sizeof(_Exc))
    if parts & EXACT:
        put("exact", d.exact, n_ol)
    if parts & ED:
        e = d.ed; T = int(e.n_pairs)
        put("ed_off", e.ed_off, (n + 1) * 8); put("ed_err", e.err, T); put("ed_pe", e.pe, 2 * T)
        if e.placement:
            put("ed_sum", e.ovlp, n_ol * C.sizeof(_EdOvlp))
        else:
            assert not e.ovlp
    if parts & TRACE:
        t = d.tr; T = int(d.ed.n_pairs)
        put("tr_off", t.cg_off, (n + 1) * 8); put("tr_ps", t.ps, 2 * T); put("tr_ncig", t.n_cig, 2 * T); put("tr_cig", t.cigar, 2 * int(t.n_cigar))
    if parts & RESCUE:
        r = d.rs
        assert int(r.n_ol) == n_ol
        put("rs_ovlp", r.ovlp, n_ol * RESCUE_OVLP.itemsize); put("rs_off", r.win_off, (n_ol + 1) * 8); put("rs_wins", r.wins, int(r.n_wins) * C.sizeof(_Win))
    if parts & WLIST:
        w = d.wl; N = int(w.n_wins)
        assert int(w.n_ol) == n_ol
        put("wl_woff", w.win_off, (n_ol + 1) * 8); put("wl_wins", w.wins, N * C.sizeof(_Win)); put("wl_cigoff", w.cig_off, (N + 1) * 8); put("wl_cig", w.cigars, 2 * int(w.n_cigar))
    return S


MAIN_PTRS = {OL: ("ol_off", "ol", "fc_off", "fc"), CL: ("ch_off", "cl_off", "qm_off", "chains", "cl_bits", "cl_rank", "cl_codes", "qmz", "cl_exc", "qmz_pos", "qmz_cnt"), EXACT: ("exact",)}
PART_VIEW = {ED: ("ed", "deliver_ed", ("ed_off", "err", "pe", "ovlp")), TRACE: ("tr", "deliver_trace", ("cg_off", "ps", "n_cig", "cigar")),
             RESCUE: ("rs", "deliver_rescue", ("ovlp", "win_off", "wins")), WLIST: ("wl", "deliver_wlist", ("win_off", "wins", "cig_off", "cigars"))}


def _absent_parts_are_null(e, slot, d, parts):
    from hifiasm_amd.api import HaoError
    for bit, names in MAIN_PTRS.items():
        if not parts & bit:
            assert all(not getattr(d, k) for k in names), (bit, names)
    for bit, (attr, getter, _) in PART_VIEW.items():
        if not parts & bit:
            assert getattr(d, attr) is None
            with pytest.raises(HaoError, match=r"\(-2\)"):
                getattr(e, getter)(slot)


@pytest.mark.parametrize("case", list(CASES))
def test_bytes_and_layout(eng, case):
    e, rs = eng
    parts, cfg = CASES[case]
    if cfg:
        (e.deliver_ed_config if cfg[0] == "diag" else e.deliver_ed_config_ref)(cfg[1], cfg[2])
    lo, hi = 2, rs.n - 1
    slot = e.overlap_batch_async(lo, hi, parts=parts)
    d = e.deliver_wait(slot)
    assert (int(d.rid_lo), int(d.n_reads)) == (lo, hi - lo) and int(d.n_ol) > 100
    _absent_parts_are_null(e, slot, d, parts)
    if parts & ED:
        assert (int(d.ed.window), int(d.ed.placement)) == (cfg[1], int(cfg[0] == "ref")) and int(d.ed.n_pairs) > 100
    if parts & TRACE:
        assert int(d.tr.n_cigar) > 0
    if parts & WLIST:
        assert int(d.rs.n_wins) > 0 and int(d.wl.n_cigar) > int(d.wl.n_wins) > 0
    S = _sections(d, parts)
    copied = sum(s[3] for s in S)
    print(f"[layout] {case}: bytes {int(d.bytes)}, formula {copied}, {len(S)} sections, padded {sum((s[2] + 63) // 64 * 64 for s in S)}")
    assert int(d.bytes) == copied
    base = S[0][1]
    assert base, S[0]
    for (name, p, region, _), (name1, p1, _, _) in zip(S, S[1:] + [S[-1]]):
        assert p and (p - base) % 64 == 0, (name, p - base)
        if name1 != name or p1 != p:
            assert p1 >= p and p1 >= p + region, (name, name1, p - base, p1 - base, region)      # ascending, no overlap
            assert p1 == p + (region + 63) // 64 * 64, (name, name1, p - base, p1 - base, region)  # the next region starts where this one, padded, ends


@pytest.mark.parametrize("case", list(CASES))
def test_empty_batch(eng, case):
    e, rs = eng
    parts, cfg = CASES[case]
    if cfg:
        (e.deliver_ed_config if cfg[0] == "diag" else e.deliver_ed_config_ref)(cfg[1], cfg[2])
    k = rs.n // 2
    slot = e.overlap_batch_async(k, k, parts=parts)
    d = e.deliver_wait(slot)
    assert (int(d.rid_lo), int(d.n_reads), int(d.bytes)) == (k, 0, 0)
    assert all(int(getattr(d, c)) == 0 for c in ("n_ol", "n_fc", "n_chains", "n_cl", "n_exc", "n_codes", "n_pos"))
    assert all(not getattr(d, p) for names in MAIN_PTRS.values() for p in names)
    _absent_parts_are_null(e, slot, d, parts)
    for bit, (attr, _, ptrs) in PART_VIEW.items():
        if parts & bit:
            v = getattr(d, attr)
            assert v is not None and all(not getattr(v, p) for p in ptrs), (attr, ptrs)
    if parts & ED:                                                               # the view of a batch that asked for ED names its grid, pairs or not
        assert (int(d.ed.n_pairs), int(d.ed.window), int(d.ed.placement)) == (0, cfg[1], int(cfg[0] == "ref"))

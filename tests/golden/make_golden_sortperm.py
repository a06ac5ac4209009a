"""Golden permutations for the direct tests of the selection sorts, from the REAL reference: oracle/_ref/ref_harness --sort-keys fills overlap_region arrays
with the key arrays of helpers.sortperm_cases() and sorts them with the reference's own ks_introsort_or_ss / ks_introsort_or_xs (anchor.cpp:33, :36).
Run in the build container only:  python tests/golden/make_golden_sortperm.py  -> tests/golden/sortperm.npz (names, mode, off, xs, sc, perm as uint16; the
keys are stored too).  The archive is written with fixed time stamps: the same keys give the same bytes."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import sortperm_cases  # noqa: E402
import sortperm_model  # noqa: E402

cases = sortperm_cases()
d = tempfile.mkdtemp(prefix="hao_sortperm_")
with open(os.path.join(d, "keys.bin"), "wb") as f:
    for name, mode, xs, sc in cases:
        f.write(np.array([mode, len(xs)], dtype=np.uint32).tobytes()); f.write(xs.astype(np.uint64).tobytes()); f.write(sc.astype(np.int32).tobytes())
r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_harness"), "--dump", os.path.join(d, "s"), "--sort-keys", os.path.join(d, "keys.bin")], capture_output=True, text=True)
assert r.returncode == 0, r.stderr[-2000:]
perm = np.fromfile(os.path.join(d, "s.sortperm.u32"), dtype=np.uint32)
off = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])]).astype(np.uint32)
assert perm.size == off[-1] and perm.max() < 65536
for i, (name, mode, xs, sc) in enumerate(cases):
    p = perm[off[i]:off[i + 1]]
    assert (np.sort(p) == np.arange(len(xs))).all(), name
    info = sortperm_model.intro_sort(sortperm_model.sort_keys(mode, xs, sc))[1]
    print(f"{name:18s} widest level {info['widest']:4d}  combsort {info['comb']:3d}  far move {int(info['far'])}")
out = {"names": np.array([c[0] for c in cases]), "mode": np.array([c[1] for c in cases], dtype=np.uint8), "off": off,
       "xs": np.concatenate([c[2] for c in cases]).astype(np.uint64), "sc": np.concatenate([c[3] for c in cases]).astype(np.int32), "perm": perm.astype(np.uint16)}
with zipfile.ZipFile(os.path.join(HERE, "sortperm.npz"), "w") as z:
    for k, v in out.items():
        b = io.BytesIO(); np.lib.format.write_array(b, v, allow_pickle=False)
        zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)); zi.compress_type = zipfile.ZIP_DEFLATED; zi.external_attr = 0o644 << 16
        z.writestr(zi, b.getvalue())
print(len(cases), "cases,", int(off[-1]), "keys ->", os.path.getsize(os.path.join(HERE, "sortperm.npz")), "bytes")

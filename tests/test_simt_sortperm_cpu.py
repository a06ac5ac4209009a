from simt_suite import reexport, FULL
import test_gpu_sortperm as _g

# (default selection: the arrays of at most 129 keys and the large ones that keep every kind the fixture is for - test_gpu_sortperm.SMALL; HAO_SIMT_FULL=1: every array)
reexport(globals(), "test_gpu_sortperm")
if not FULL:
    test_sort_matches_reference.__defaults__ = (_g.SMALL,)

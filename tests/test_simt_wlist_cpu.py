from simt_suite import reexport, FULL

# (default selection: the small HiFi set at its own configuration, at the tight one that has forward and backward windows and at the one with untraced windows,
# the wide-window case, the case with re-placements that are taken, and the contracts; HAO_SIMT_FULL=1: every case)
# (the many-slice case: the small HiFi set at its own configuration in place of nn at 200-base windows, 18 763 swept windows in 74 slices)
reexport(globals(), "test_gpu_wlist", replace={} if FULL else {"case": [("hifi", 775, 0.04)]}, drop=lambda v: not FULL and isinstance(v, (tuple, list)) and not (v[0] in ("hifi", "nn") or v[1] == 1500 or (len(v) == 3 and isinstance(v[2], tuple) and v[2][0] == 1500)))

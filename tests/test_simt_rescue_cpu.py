from simt_suite import reexport, FULL

# (default selection: the small HiFi set at its own configuration and at the tight one that walks the rescue's branches, the wide-window case in which forward
# steps fail, the streamed path on the small HiFi set, and the contracts; HAO_SIMT_FULL=1: every case the emulator can take)
# (the many-slice case: the tight HiFi case in place of the ONT one, 1748 overlaps with a gap in 7 slices)
reexport(globals(), "test_gpu_rescue", replace={} if FULL else {"case": [("hifi", 775, 0.004)]}, drop=lambda v: not FULL and isinstance(v, (tuple, list)) and not ((v[0] == "hifi" and v[1] in (775, 64)) or v[1] == 1500))

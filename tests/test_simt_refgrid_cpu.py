from simt_suite import reexport, FULL

# (default selection: the blocking and the streamed path on the small HiFi set and the contract's edges; HAO_SIMT_FULL=1: every read set the emulator can take)
reexport(globals(), "test_gpu_refgrid", drop=lambda v: not FULL and isinstance(v, (tuple, list)) and (v[0] != "hifi" or (len(v) == 6 and v[3] != 0)))

from simt_suite import reexport, FULL

# (default selection: one one-word band on the small read set - the blocking path against the oracle and the host-fed path, and the streaming pass with the
# TRACE part, three batches, both slots, against the blocking path; HAO_SIMT_FULL=1: every case and the contract's edges)
# (the many-slice case: the small read set in place of the repeat-rich one, 38 063 traced pairs in 149 slices)
reexport(globals(), "test_gpu_trace_grid", replace={} if FULL else {"case": [("hifi", 375, 15)]},
         only=None if FULL else ("test_grid_pairs_traced_on_the_device", "test_grid_pairs_traced_in_many_slices", "test_streamed_batches_carry_their_traceback"),
         drop=lambda v: not FULL and isinstance(v, (tuple, list)) and tuple(v) not in (("hifi", 375, 15), ("hifi", 375, 15, "ol")))

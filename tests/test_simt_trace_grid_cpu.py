from simt_suite import reexport, FULL

# (default selection: one one-word band on the small read set - the blocking path against the oracle and the host-fed path, and the streaming pass with the
# TRACE part, three batches, both slots, against the blocking path; HAO_SIMT_FULL=1: every case and the contract's edges)
reexport(globals(), "test_gpu_trace_grid",
         only=None if FULL else ("test_grid_pairs_traced_on_the_device", "test_streamed_batches_carry_their_traceback"),
         drop=lambda v: not FULL and isinstance(v, (tuple, list)) and tuple(v) not in (("hifi", 375, 15), ("hifi", 375, 15, "ol")))

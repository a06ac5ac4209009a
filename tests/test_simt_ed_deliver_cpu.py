from simt_suite import reexport, FULL

# (default selection: one one-word band on the small read set - the whole streaming pass with the ED part, three batches, both slots; HAO_SIMT_FULL=1: every case
# and the contract's edges)
reexport(globals(), "test_gpu_ed_deliver", only=None if FULL else ("test_streamed_batches_carry_their_window_alignment",),
         drop=lambda v: not FULL and isinstance(v, (tuple, list)) and tuple(v) != ("hifi", 375, 15, "ol"))

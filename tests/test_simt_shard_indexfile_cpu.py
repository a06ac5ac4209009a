from simt_suite import reexport

# (default selection: the set with N sites, both worlds - save, load with both kinds of cuts, the reference-written file, round trip, failures, the unsharded
# engine; HAO_SIMT_FULL=1: every scenario)
reexport(globals(), "test_gpu_shard_indexfile", keep={"nn"})

from simt_suite import reexport, FULL

# (default selection: the worlds of 2 and 3 and the multi-chunk gather over the set with N sites and taken re-placements, the digest, the host-fed calls and the
# contracts - which stream the tight HiFi configuration through an attached view; HAO_SIMT_FULL=1: every case.  The RCCL test needs two GPUs:
# tests/test_dist_gather_cpu.py runs its worker over the emulated transport)
reexport(globals(), "test_gpu_shard_f3", skip=("test_rccl_gather_between_processes",),
         drop=lambda v: not FULL and isinstance(v, (tuple, list)) and len(v) == 3 and v[0] != "nn")

from simt_suite import reexport

reexport(globals(), "test_gpu_ladder_adv", skip=("test_two_rank_world_after_the_gather",))      # (the loopback world: one emulated engine per host thread, left to the device)

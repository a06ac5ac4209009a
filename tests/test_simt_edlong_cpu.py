from simt_suite import reexport, FULL

reexport(globals(), "test_gpu_edlong", keep=("ont",), replace={"big": [FULL]})      # (the two upper-end pairs per list: ~7000 columns of a 64-lane segment each, under HAO_SIMT_FULL only)

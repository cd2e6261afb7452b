"""What tests/test_gpu_downscale_plane_sweeps.py sends content through, as data: tests/test_downscale_planes_abi.py holds REACHED
against the code object without importing the sweeps."""
ROWS = ("encode", "size_table", "rd_table")
VARIANTS = [1, 2]                                                   # the source's chroma step: planar (I420, YV12), paired (NV12, NV21)
FORMS = {1: ("i420", "yv12"), 2: ("nv12", "nv21")}                  # the presets a variant's cases alternate between
REACHED = [(row, cstep) for row in ROWS for cstep in VARIANTS]      # every sweep runs both variants through every row

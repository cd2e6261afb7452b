"""What tests/test_gpu_downscale_sweeps.py sends content through, as data: tests/test_downscale_abi.py holds REACHED against the
code object without importing the sweeps."""
ROWS = ("encode", "size_table", "rd_table")
VARIANTS = [3, 4]                                                   # bytes per source pixel
REACHED = [(row, C) for row in ROWS for C in VARIANTS]              # every sweep runs both variants through every row

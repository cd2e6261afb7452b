"""What tests/test_gpu_float_pixels_sweeps.py sends content through, as data: tests/test_float_pixels_abi.py holds REACHED
against the code object without importing the sweeps."""
import float_planes as fp

ROWS = ("encode", "size_table", "rd_table")
VARIANTS = [(kind, Cs) for kind in fp.KINDS for Cs in (3, 4)]
REACHED = [(row, kind, Cs) for row in ROWS for kind, Cs in VARIANTS]     # every sweep runs every variant through every row

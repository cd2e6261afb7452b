"""What tests/test_gpu_downscale_word_sweeps.py sends content through, as data: tests/test_downscale_words_abi.py holds REACHED
against the code object without importing the sweeps."""
ROWS = ("encode", "size_table", "rd_table")
VARIANTS = [2, 4]                                                   # the source's chroma step: planar (I010), word pairs (P010)
FORMS = {2: "i010", 4: "p010"}                                      # the preset of a variant's cases: low-aligned shift 2, high-aligned shift 8
REACHED = [(row, cstep) for row in ROWS for cstep in VARIANTS]      # every sweep runs both variants through every row

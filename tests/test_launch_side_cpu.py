"""tests/launch_side.py checked on the host: the decoy and real frame sets differ in every oracle record, the batch lengths of the
divisor switch are where div_magic puts them, and udiv's quotient is exact for those two launches where the documented condition
(n * d < 2^32 for the largest index) promises it.  This stands beside tests/test_gpu_grid_extents.py and does not replace it."""
import numpy as np
import pytest

import launch_side as LS

SHAPES = ((144, 80, 9), (48, 32, 3))


def _restated_magic(d, n_max):
    """div_magic of m1v_kernels.hip, restated from its text: uint32 m, 64-bit n_max * d."""
    ok = d >= 2 and (n_max * d) % (1 << 64) < (1 << 32)
    return (np.uint32(((1 << 32) // d + 1) & 0xFFFFFFFF) if ok else np.uint32(0)).item()


@pytest.mark.parametrize("kind", LS.KINDS)
def test_decoy_and_real_records_differ_in_every_frame(orc, kind):
    for W, H, n in SHAPES:
        decoy, real = LS.frame_sets(kind, W, H, n)
        assert decoy.shape == real.shape == (n, H, W, 4 if kind == "packed4" else 3)
        for q in (12, 4):
            assert LS.records_differ(orc, decoy, real, 3, q, orc.MODE_FULL), (kind, W, H, q)
    if kind == "packed4":       # the strip kernel's case: 640 x 480 STRICT with 4 channels
        decoy, real = LS.frame_sets(kind, 640, 480, 4)
        assert LS.records_differ(orc, decoy, real, 0, 12, orc.MODE_STRICT)


@pytest.mark.parametrize("size, want", (((3840, 2160), (516, 517)), ((7680, 4320), (32, 33)), ((1920, 1080), (8256, 8257))))
def test_switch_batches(size, want):
    cols, rows = LS.tile_grid(*size)
    tpf = cols * rows
    assert {(3840, 2160): 1020, (7680, 4320): 4080, (1920, 1080): 255}[size] == tpf
    last, nxt = LS.switch_batches(cols, rows)
    assert (last, nxt) == want
    for n, magic in ((last, True), (nxt, False)):
        group, frame, col, units = LS.launch_divisors(cols, rows, n)
        assert units == n * tpf and group[0] == 8 * tpf and frame[0] == tpf and col[0] == cols
        assert group[1] == _restated_magic(8 * tpf, units) and frame[1] == _restated_magic(tpf, units)
        assert (group[1] != 0) == magic, "the group divisor switches between these two batches"
        assert frame[1] != 0 and col[1] != 0, "the smaller divisors stay magic on both sides"


@pytest.mark.parametrize("size", ((3840, 2160), (7680, 4320)))
def test_udiv_is_exact_at_the_switch(size):
    cols, rows = LS.tile_grid(*size)
    tpf = cols * rows
    for n in LS.switch_batches(cols, rows):
        group, frame, col, units = LS.launch_divisors(cols, rows, n)
        top = np.arange(max(units - 4096, 0), units, dtype=np.uint64)
        for dm in (group, frame):
            d = dm[0]
            mult = np.arange(d, units, d, dtype=np.uint64)
            idx = np.unique(np.concatenate([top, mult, mult - 1, np.array([0, units - 1], np.uint64)]))
            got = (idx * np.uint64(dm[1])) >> np.uint64(32) if dm[1] else idx // np.uint64(d)
            assert np.array_equal(got, idx // np.uint64(d)), (size, n, dm)
        tiles = np.arange(tpf, dtype=np.uint64)     # the tile column split of every tile of a frame
        assert np.array_equal((tiles * np.uint64(col[1])) >> np.uint64(32), tiles // np.uint64(cols))
        # frame_unit_of sends the launch's last and first workgroups, and those about the full groups' end, to valid (frame, unit) pairs
        edge = (n // 8) * group[0]
        for b in {0, units - 1, max(edge - 1, 0), min(edge, units - 1)}:
            f, u = LS.frame_unit_of(b, n, group, frame)
            assert 0 <= f < n and 0 <= u < tpf, (b, f, u)
        seen = {LS.frame_unit_of(b, n, group, frame) for b in range(units - 4096, units)}
        assert len(seen) == 4096


def test_gate_length_rule():
    assert LS.gate_ms(0.1) == 20.0 and LS.gate_ms(1.0) == 20.0 and LS.gate_ms(3.0) == 60.0


def test_rolled_colours_visit_every_slot():
    a, b = LS.rolled_colours(0), LS.rolled_colours(5, 4)
    assert a.shape == (4096, 4096, 3) and b.shape == (4096, 4096, 4)
    flat = b.reshape(-1, 4)
    assert tuple(flat[5][:3]) == (0, 0, 0) and tuple(a.reshape(-1, 3)[0x123456]) == (0x12, 0x34, 0x56)
    c = 0x00FF80        # any colour lies at pixel (c + k) mod 2^24 of frame k: over nine frames in every slot of a group of four
    assert tuple(LS.rolled_colours(3).reshape(-1, 3)[c + 3]) == (0x00, 0xFF, 0x80)
    assert {(c + k) % 4 for k in range(9)} == {0, 1, 2, 3}

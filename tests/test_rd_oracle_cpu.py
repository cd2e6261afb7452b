"""CPU tests of the rd checker (tests/rd_oracle.py): the measure of include/mpeg1_hip.h computed from the oracle alone, pinned on
the smooth gradient of DESIGN.md, where the byte rule's "largest that fits" and the least distortion part ways."""
import numpy as np

import rd_oracle as rd


def test_gradient_table_is_pinned(orc):
    W, H = 352, 288
    pic = rd.gradient_frame(W, H)
    sizes = [len(orc.encode_frame(pic, W, H, 0, q, orc.MODE_FULL)) for q in rd.GRADIENT_QUALITIES]
    dist = [rd.frame_distortion(orc, pic, W, H, q, orc.MODE_FULL) for q in rd.GRADIENT_QUALITIES]
    assert tuple(sizes) == rd.GRADIENT_BYTES
    assert tuple(dist) == rd.GRADIENT_D
    table_s, table_d, status = rd.rd_table(orc, pic[None], rd.GRADIENT_QUALITIES, orc.MODE_FULL)
    assert [r[0] for r in table_s] == sizes and [r[0] for r in table_d] == dist and status == [0] * 8


def test_the_two_picks_at_8000_bytes(orc):
    q = rd.GRADIENT_QUALITIES
    assert q[rd.largest_that_fits(rd.GRADIENT_BYTES, 8000)] == 92
    k, over = rd.pick(rd.BEST_IN_BUDGET, rd.GRADIENT_BYTES, rd.GRADIENT_D, 8000)
    assert (q[k], over) == (38, False)
    # the distortion rule: the smallest record within 1.5 M is quality 38's again; nothing is within 100 000
    k, over = rd.pick(rd.SMALLEST_AT_DISTORTION, rd.GRADIENT_BYTES, rd.GRADIENT_D, 1_500_000)
    assert (q[k], over) == (38, False)
    k, over = rd.pick(rd.SMALLEST_AT_DISTORTION, rd.GRADIENT_BYTES, rd.GRADIENT_D, 100_000)
    assert (q[k], over) == (76, True)
    k, over = rd.pick(rd.BEST_IN_BUDGET, rd.GRADIENT_BYTES, rd.GRADIENT_D, 3000)
    assert (q[k], over) == (5, True)
    # a candidate out of the running is skipped; with all out the frame goes to candidate 0
    k, over = rd.pick(rd.BEST_IN_BUDGET, rd.GRADIENT_BYTES, rd.GRADIENT_D, 8000, out=(3,))
    assert (q[k], over) == (25, False)
    assert rd.pick(rd.BEST_IN_BUDGET, rd.GRADIENT_BYTES, rd.GRADIENT_D, 8000, out=range(8)) == (0, False)


def test_pick_ties():
    # equal distortion: the smaller record, then the smaller k; none fits: the smallest record, ties by k alone
    assert rd.pick(rd.BEST_IN_BUDGET, [50, 40, 40], [7, 7, 7], 60) == (1, False)
    assert rd.pick(rd.BEST_IN_BUDGET, [50, 50, 60], [9, 3, 1], 10) == (0, True)
    assert rd.pick(rd.SMALLEST_AT_DISTORTION, [40, 40, 30], [5, 4, 9], 6) == (1, False)
    assert rd.pick(rd.SMALLEST_AT_DISTORTION, [40, 30, 30], [8, 8, 9], 6) == (1, True)


def test_levels_are_the_truncated_quotients(orc):
    """The helper's levels at quality q are sign(c) * (|c| // d) of its raw coefficients and divisors."""
    rng = np.random.default_rng(12)
    W, H = 64, 48
    pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    c = orc.frame_coefficients(pic, W, H, 100, orc.MODE_FULL).astype(np.int64)
    assert np.array_equal(rd.divisors_zigzag(orc, 100), np.ones(64, np.int64))
    for q in (1, 12, 50, 77, 92):
        d = rd.divisors_zigzag(orc, q)
        lv = orc.frame_coefficients(pic, W, H, q, orc.MODE_FULL).astype(np.int64)
        assert np.array_equal(lv, np.sign(c) * (np.abs(c) // d[None, :])), q
        # every term of D is a non-negative integer and a carried position costs at most what a dropped one does
        err = c - lv * d[None, :]
        assert np.all(err * err <= c * c)


def test_carried_positions_follow_the_reference_walk():
    import hard_content
    rng = np.random.default_rng(3)
    z = rng.integers(-3, 4, (200, 64)) * (rng.random((200, 64)) < 0.3)
    z[:50, 0] = 0
    keep = rd.carried(z)
    for b in range(len(z)):
        want = hard_content._emitted_levels(z[b])
        got = [int(z[b, p]) for p in range(1, 64) if keep[b, p]]
        assert keep[b, 0] and got == want, b

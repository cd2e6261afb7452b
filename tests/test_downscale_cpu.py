"""CPU checks of the downscale layout's model and inputs (tests/downscale.py) and of its Python side (downscale_strides, the
branch of Mpeg1Encoder._check_input), without a device: down2 against a per-pixel loop; its rounding; that the sources tell the
four pixels of a cell apart; the strides of contiguous tensors, windows and channels-last views; and the refusals of tensors that
are not on the device."""
import numpy as np
import pytest

import downscale as ds


def _loop(src, order):
    n, H2, W2, _ = src.shape
    out = np.zeros((n, H2 // 2, W2 // 2, 3), dtype=np.uint8)
    for f in range(n):
        for y in range(H2 // 2):
            for x in range(W2 // 2):
                for c in range(3):
                    i = 2 - c if order == "bgr" else c      # the byte of the source pixel that holds colour c
                    s = int(src[f, 2 * y, 2 * x, i]) + int(src[f, 2 * y, 2 * x + 1, i]) + int(src[f, 2 * y + 1, 2 * x, i]) + \
                        int(src[f, 2 * y + 1, 2 * x + 1, i])
                    out[f, y, x, c] = (s + 2) >> 2
    return out


@pytest.mark.parametrize("C", ds.WIDTHS)
@pytest.mark.parametrize("order", ds.ORDERS)
def test_down2_against_a_per_pixel_loop(order, C):
    src = ds.noise_source(3 + C, 2, 4, 6, C)
    assert src.shape == (2, 8, 12, C)
    got = ds.down2(src, order)
    assert got.shape == (2, 4, 6, 3) and got.dtype == np.uint8
    assert np.array_equal(got, _loop(src, order))
    if C == 4:      # the 4th byte never reaches the picture
        other = src.copy()
        other[..., 3] ^= 0xff
        assert np.array_equal(ds.down2(other, order), got)


def test_rounding_every_remainder_and_the_ends():
    """All four remainders of the sum mod 4 occur on noise; a remainder of 2 (the tie) goes up, 1 down, 3 up; 4 * 255 gives 255 and
    0 gives 0."""
    src = ds.noise_source(1, 1, 16, 16)
    s = src.astype(np.int64)
    sums = s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]
    got = ds.down2(src).astype(np.int64)
    assert set(np.unique(sums % 4).tolist()) == {0, 1, 2, 3}
    assert np.array_equal(got[sums % 4 == 0], sums[sums % 4 == 0] // 4)
    assert np.array_equal(got[sums % 4 == 1], (sums[sums % 4 == 1] - 1) // 4)
    assert np.array_equal(got[sums % 4 == 2], (sums[sums % 4 == 2] + 2) // 4)      # ties go up
    assert np.array_equal(got[sums % 4 == 3], (sums[sums % 4 == 3] + 1) // 4)
    for values, want in (((255, 255, 255, 255), 255), ((0, 0, 0, 0), 0), ((255, 255, 255, 254), 255), ((0, 0, 0, 1), 0),
                         ((1, 1, 0, 0), 1), ((1, 0, 0, 0), 0), ((255, 254, 254, 254), 254), ((3, 2, 2, 2), 2)):
        for shift in range(4):
            cell = values[shift:] + values[:shift]
            assert np.all(ds.down2(ds.cell_source(cell, 1, 2, 3)) == want), (cell, want)


def test_replicated_sources_give_the_picture_back():
    px = np.random.default_rng(5).integers(0, 256, (2, 6, 8, 3), dtype=np.uint8)
    for order in ds.ORDERS:
        src = ds.replicated_source(px, order)
        assert src.shape == (2, 12, 16, 3)
        assert np.array_equal(ds.down2(src, order), px)
    assert np.array_equal(ds.replicated_source(px, "bgr"), ds.replicated_source(px, "rgb")[..., ::-1])


@pytest.mark.parametrize("C", ds.WIDTHS)
def test_the_noise_source_tells_the_four_pixels_of_a_cell_apart(C):
    """Replacing one of the four source pixels of every cell by its horizontal or vertical neighbour in the cell changes the
    rendition: a kernel that reads a wrong pixel of the cell, or one of them twice, cannot pass on this source.  A byte keeps
    its value only when the replaced byte's difference d leaves (sum + d + 2) >> 2 where it was, which needs |d| < 4: 7 of 256
    values of a uniform difference at the most, so more than 95 of 100 bytes and all but a handful of cells must change."""
    H, W = 32, 48
    src = ds.noise_source(17, 1, H, W, C)
    base = ds.down2(src)
    for dy in (0, 1):
        for dx in (0, 1):
            for ny, nx in ((dy, 1 - dx), (1 - dy, dx)):
                other = src.copy()
                other[:, dy::2, dx::2] = src[:, ny::2, nx::2]
                got = ds.down2(other)
                changed = got != base
                assert changed.mean() > 0.95, (dy, dx, ny, nx, changed.mean())
                assert changed.any(axis=3).sum() >= H * W - 8, (dy, dx, ny, nx, int(changed.any(axis=3).sum()))
    # ... and a source shifted by one source pixel or one source row is another picture
    assert (ds.down2(np.roll(src, 1, axis=2)) != base).mean() > 0.95
    assert (ds.down2(np.roll(src, 1, axis=1)) != base).mean() > 0.95


def test_host_buffer_places_the_source_and_nothing_else():
    src = ds.noise_source(2, 2, 4, 8, 4)
    for P in ds.WIDTHS:
        where = dict(pad=13, gap=5, window=(3, 1), margin=(2, 3))
        a, (pitch, frame, at) = ds.host_buffer(src, P, fill_seed=1, **where)
        b, _ = ds.host_buffer(src, P, fill_seed=2, **where)
        assert pitch == (3 + 16 + 2) * P + 13 and frame == (1 + 8 + 3) * pitch + 5 and at == ds.GUARD + pitch + 3 * P
        assert len(a) == 2 * ds.GUARD + 2 * frame
        same = np.zeros(len(a), dtype=bool)
        for f in range(2):
            for y in range(8):
                for x in range(16):
                    o = at + f * frame + y * pitch + x * P
                    assert a[o:o + 3].tolist() == src[f, y, x, :3].tolist()
                    same[o:o + 3] = True
        assert np.array_equal(a[same], b[same])
        assert (a[~same] != b[~same]).mean() > 0.9      # everything else is the fill's noise


# ---- downscale_strides ----------------------------------------------------------------------------------------------------------
def test_strides_of_contiguous_tensors_windows_and_channels_last_views():
    from ec504_imageencoder_amd import downscale_layout_preset, downscale_strides
    W, H, n = 48, 32, 3
    for C in (3, 4):
        shape = (n, 2 * H, 2 * W, C)
        strides = (2 * H * 2 * W * C, 2 * W * C, C, 1)
        for order in ds.ORDERS:
            assert downscale_strides(shape, strides, "nhwc", order) == downscale_layout_preset(W, H, C, order)
            # the channels-last view of the same memory
            assert downscale_strides((n, C, 2 * H, 2 * W), (strides[0], 1, strides[1], strides[2]), "nchw", order) == \
                downscale_layout_preset(W, H, C, order)
    # a window x[:, 1:1+2H, 3:3+2W, :3] of a [n, 2H + 5, 2W + 7, 4] surface
    Hs, Ws = 2 * H + 5, 2 * W + 7
    lay = downscale_strides((n, 2 * H, 2 * W, 3), (Hs * Ws * 4, Ws * 4, 4, 1))
    assert lay == dict(row_pitch=Ws * 4, frame_stride=Hs * Ws * 4, pixel_step=4, order=0, factor=2)
    # a single frame's stride is the extent of the read contract
    lay = downscale_strides((1, 2 * H, 2 * W, 3), (123, Ws * 4, 4, 1), order="bgr")
    assert lay == dict(row_pitch=Ws * 4, frame_stride=(2 * H - 1) * Ws * 4 + 2 * W * 4, pixel_step=4, order=1, factor=2)
    for shape, strides, dims in (((n, 2 * H, 2 * W), (1, 1, 1), "nhwc"),                         # not 4-D
                                 ((n, 2 * H + 1, 2 * W, 3), (1, 2 * W * 3, 3, 1), "nhwc"),       # an odd extent
                                 ((n, 2 * H, 2 * W - 1, 3), (1, 2 * W * 3, 3, 1), "nhwc"),
                                 ((n, 2 * H, 2 * W, 2), (2 * H * 2 * W * 3, 2 * W * 3, 3, 1), "nhwc"),       # two channels
                                 ((n, 2 * H, 2 * W, 3), (2 * H * 2 * W * 3, 2 * W * 3, 3, 2), "nhwc"),       # bytes of a pixel apart
                                 ((n, 3, 2 * H, 2 * W), (3 * 2 * H * 2 * W, 2 * H * 2 * W, 2 * W, 1), "nchw"),   # planar
                                 ((n, 2 * H, 2 * W, 3), (2 * H * 2 * W * 5, 2 * W * 5, 5, 1), "nhwc"),       # a pixel step of 5
                                 ((n, 2 * H, 2 * W, 4), (2 * H * 2 * W * 3, 2 * W * 3, 3, 1), "nhwc"),       # a step below C
                                 ((n, 2 * H, 2 * W, 3), (2 * H * 2 * W * 3, 2 * W * 3 - 1, 3, 1), "nhwc"),   # a pitch below the row
                                 ((n, 2 * H, 2 * W, 3), (-1, 2 * W * 3, 3, 1), "nhwc"),
                                 ((n, 2 * H, 2 * W, 3), (2 * H * 2 * W * 3, 2 * W * 3, 3, 1), "nwhc")):
        with pytest.raises(ValueError):
            downscale_strides(shape, strides, dims)
    with pytest.raises(ValueError):
        downscale_strides((n, 2 * H, 2 * W, 3), (2 * H * 2 * W * 3, 2 * W * 3, 3, 1), "nhwc", "gbr")


# ---- _check_input on tensors that are not on the device ---------------------------------------------------------------------------
def _encoder_without_a_device(W, H, lay):
    """An Mpeg1Encoder object with the state _check_input reads and no library handle behind it."""
    from ec504_imageencoder_amd import Mpeg1Encoder
    enc = Mpeg1Encoder.__new__(Mpeg1Encoder)
    enc._h = None
    enc.width, enc.height, enc.channels = W, H, 3
    enc._input, enc._table_on, enc._planes_on = ("downscale_layout", lay), False, False
    return enc


def test_check_input_refusals_without_a_device():
    import torch
    from ec504_imageencoder_amd import downscale_layout_preset
    W, H, n = 8, 4, 2
    enc = _encoder_without_a_device(W, H, downscale_layout_preset(W, H, 3))
    src = torch.zeros((n, 2 * H, 2 * W, 3), dtype=torch.uint8)
    for wrong, match in ((src.float(), "takes torch.uint8 tensors, not torch.float32"), (src.to(torch.int8), "takes torch.uint8"),
                         (src.numpy(), "takes torch.uint8"), (src, "must be a CUDA tensor")):
        with pytest.raises(AssertionError, match=match):
            enc._check_input(wrong)
    # the rest of the branch, on a tensor that says it is on the device

    class OnDevice(torch.Tensor):
        is_cuda = True

    def dev(t):
        return t.as_subclass(OnDevice)

    enc._check_input(dev(src))
    enc._check_input(dev(src[:1]))
    enc._check_input(dev(src.permute(0, 3, 1, 2)))                          # channels-last strides
    rendition = torch.zeros((n, H, W, 3), dtype=torch.uint8)
    for wrong in (rendition, src[0], src[:, ::2], src[:, :, ::2], src[..., :2], torch.zeros((n, 3, 2 * H, 2 * W), dtype=torch.uint8),
                  torch.zeros((n, 2 * H, 2 * W + 2, 3), dtype=torch.uint8)[:, :, :2 * W],     # another row pitch
                  torch.zeros((n, 2 * H, 2 * W, 4), dtype=torch.uint8),                     # another pixel step
                  torch.zeros((n + 1, 2 * H + 2, 2 * W, 3), dtype=torch.uint8)[:n, :2 * H]):  # another frame stride
        with pytest.raises(AssertionError):
            enc._check_input(dev(wrong))
    # a window of a four-byte surface under its own layout, and one whose storage ends inside its last pixel
    from ec504_imageencoder_amd import downscale_strides
    big = torch.zeros((n, 2 * H + 2, 2 * W + 2, 4), dtype=torch.uint8)
    win = big[:, 1:1 + 2 * H, 1:1 + 2 * W, :3]
    enc = _encoder_without_a_device(W, H, downscale_strides(tuple(win.shape), tuple(win.stride())))
    enc._check_input(dev(win))
    flat = torch.zeros(n * (2 * H + 2) * (2 * W + 2) * 4 - 1, dtype=torch.uint8)
    short = torch.as_strided(flat, (n, 2 * H + 2, 2 * W + 2, 3), ((2 * H + 2) * (2 * W + 2) * 4, (2 * W + 2) * 4, 4, 1))[:, 2:, 2:]
    assert tuple(short.stride()) == tuple(win.stride())
    with pytest.raises(AssertionError, match="storage ends inside the last pixel"):
        enc._check_input(dev(short))
    enc._h = None

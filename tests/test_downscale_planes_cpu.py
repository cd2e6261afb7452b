"""CPU checks of the downscale plane layout's model and inputs (tests/downscale_planes.py) and of its Python side (the branch of
extent Mpeg1Encoder._check_input asks for), without a device: the model against a per-sample loop and its rounding; the identity on replicated
sources in every form and placement; that the placement writes the addressed bytes and nothing else; the record oracle on the
model's frame against the oracle proper where a picture exists; and a census that the noise inputs of the GPU arithmetic test are
sensitive — every plausible mistake of a kernel changes a record on every size used there."""
import numpy as np
import pytest

import downscale_planes as dp
import plane_oracle

# the sizes and modes of tests/test_gpu_downscale_planes.py's arithmetic test
CASES = ((16, 16, "full"), (48, 32, "full"), (144, 80, "full"), (112, 160, "strict"))
QUALITIES = (12, 50)


def _loop(frame, lay, W, H):
    Y, Cb, Cr = np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)
    for out, off, pitch, step in ((Y, lay["y_offset"], lay["y_pitch"], 1), (Cb, lay["cb_offset"], lay["c_pitch"], lay["c_step"]),
                                  (Cr, lay["cr_offset"], lay["c_pitch"], lay["c_step"])):
        for y in range(out.shape[0]):
            for x in range(out.shape[1]):
                at = off + 2 * y * pitch + 2 * x * step
                out[y, x] = (int(frame[at]) + int(frame[at + step]) + int(frame[at + pitch]) + int(frame[at + pitch + step]) + 2) >> 2
    return Y, Cb, Cr


@pytest.mark.parametrize("where", (dp.TIGHT, dp.PITCHED, dict(spread=True, cpad=3)), ids=("tight", "pitched", "spread"))
@pytest.mark.parametrize("preset", dp.PRESETS)
def test_model_against_a_per_sample_loop(preset, where):
    if where.get("spread") and dp.CSTEP[preset] == 2:
        where = dict(cpad=3)
    W, H, n = 8, 4, 2
    src = dp.noise_source(3, n, H, W)
    host, lay, at, span = dp.host_buffer(src, preset, fill_seed=1, **where)
    want = dp.model_frames(src)
    for f in range(n):
        frame = host[at + f * lay["frame_stride"]:]
        Y, Cb, Cr, i420 = dp.down2_planes(frame, lay, W, H)
        assert Y.shape == (H, W) and Cb.shape == Cr.shape == (H // 2, W // 2) and i420.shape == (W * H * 3 // 2,)
        for got, loop in zip((Y, Cb, Cr), _loop(frame, lay, W, H)):
            assert np.array_equal(got, loop)
        assert np.array_equal(i420, want[f])
        assert np.array_equal(i420, np.concatenate([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)]))


def test_rounding_every_remainder_and_the_ends():
    """All four remainders of the sum mod 4 occur on noise; a remainder of 2 (the tie) goes up, 1 down, 3 up; 4 * 255 + 2 = 1022
    gives 255 and 0 gives 0."""
    src = dp.noise_source(1, 1, 16, 16)
    for plane in src:
        s = plane.astype(np.int64)
        sums = s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]
        got = dp.box(plane).astype(np.int64)
        assert set(np.unique(sums % 4).tolist()) == {0, 1, 2, 3}
        assert np.array_equal(got[sums % 4 == 0], sums[sums % 4 == 0] // 4)
        assert np.array_equal(got[sums % 4 == 1], (sums[sums % 4 == 1] - 1) // 4)
        assert np.array_equal(got[sums % 4 == 2], (sums[sums % 4 == 2] + 2) // 4)      # ties go up
        assert np.array_equal(got[sums % 4 == 3], (sums[sums % 4 == 3] + 1) // 4)
    assert (4 * 255 + 2) == 1022 and 1022 >> 2 == 255
    for values, want in (((255, 255, 255, 255), 255), ((0, 0, 0, 0), 0), ((255, 255, 255, 254), 255), ((0, 0, 0, 1), 0),
                         ((1, 1, 0, 0), 1), ((1, 0, 0, 0), 0), ((255, 254, 254, 254), 254), ((3, 2, 2, 2), 2)):
        for shift in range(4):
            cell = values[shift:] + values[:shift]
            other = tuple(255 - v for v in cell)
            Y, Cb, Cr = (dp.box(p) for p in dp.cell_source(cell, other, cell[::-1], 1, 4, 6))
            assert np.all(Y == want) and np.all(Cr == want) and np.all(Cb == (sum(other) + 2) >> 2), (cell, want)


@pytest.mark.parametrize("preset", dp.PRESETS)
def test_replicated_sources_give_the_planes_back(preset):
    rng = np.random.default_rng(5)
    W, H, n = 16, 8, 2
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, H, W), (n, H // 2, W // 2), (n, H // 2, W // 2)))
    want = np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], 1)
    src = dp.replicated_planes(y, cb, cr)
    assert [p.shape for p in src] == [(n, 2 * H, 2 * W), (n, H, W), (n, H, W)]
    assert np.array_equal(dp.model_frames(src), want)
    # the packed frames are the tight preset's ...
    from ec504_imageencoder_amd import downscale_plane_layout_preset
    tight = downscale_plane_layout_preset(W, H, preset)
    packed = dp.replicated_source(y, cb, cr, preset)
    assert packed.shape == (n, 6 * W * H) and tight["frame_stride"] == 6 * W * H
    assert dp.geometry(W, H, preset)[0] == tight
    for f in range(n):
        assert np.array_equal(dp.down2_planes(packed[f], tight, W, H)[3], want[f])
    # ... and what the placements hold, tight and pitched
    for where in (dp.TIGHT, dp.PITCHED):
        host, lay, at, span = dp.host_buffer(src, preset, fill_seed=2, **where)
        for f in range(n):
            assert np.array_equal(dp.down2_planes(host[at + f * lay["frame_stride"]:], lay, W, H)[3], want[f])
        if not where:
            assert np.array_equal(host[at:at + n * 6 * W * H].reshape(n, -1), packed)


@pytest.mark.parametrize("preset", dp.PRESETS)
def test_host_buffer_places_the_source_and_nothing_else(preset):
    W, H, n = 8, 4, 2
    src = dp.noise_source(2, n, H, W)
    for where in (dp.TIGHT, dp.PITCHED, dict(spread=True) if dp.CSTEP[preset] == 1 else dict(cpad=1)):
        a, lay, at, span = dp.host_buffer(src, preset, fill_seed=1, **where)
        b, _, _, _ = dp.host_buffer(src, preset, fill_seed=2, **where)
        assert len(a) == at + n * lay["frame_stride"] + dp.GUARD and at >= dp.GUARD and span <= lay["frame_stride"]
        same = dp.addressed(lay, n, W, H, at, len(a))
        assert same.sum() == n * 6 * W * H                     # no two samples share a byte
        assert np.array_equal(a[same], b[same])
        if (~same).sum() > 200:
            assert (a[~same] != b[~same]).mean() > 0.9          # everything else is the fill's noise
    lay, span, at = dp.geometry(W, H, preset, **dp.PITCHED)
    assert at == dp.GUARD + 1 and lay["y_pitch"] % 4 and lay["c_pitch"] % 4 and lay["frame_stride"] == span + 5
    assert lay["y_pitch"] == 6 + 2 * W + 2 + 13 and lay["y_offset"] == 2 * lay["y_pitch"] + 6


# ---- the record oracle on the model's frame -----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,mode,qf", [(48, 32, "full", 12), (48, 32, "full", 50), (112, 160, "strict", 12)])
def test_the_record_oracle_on_the_models_frame_equals_the_oracle_on_a_converted_picture(orc, W, H, mode, qf):
    """A picture exists for every rendition whose chroma planes are the head of a converted picture's: the reference addresses
    its full-resolution Cb / Cr plane with stride W / 2 (encoder.h:347-348), so what it codes as chroma is the first
    (W / 2) * (H / 2) bytes of each plane read as an H / 2 x W / 2 plane.  The source that repeats the picture's luma plane and
    those two 2 x 2 has them as its rendition, and plane_oracle.encode_layout on the model's I420 frame is orc.encode_frame on the
    picture (as tests/test_planes_abi.py pins the two oracles to each other on reference-style planes)."""
    from ec504_imageencoder_amd import plane_layout_preset
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    rng = np.random.default_rng(W * 1000 + H + qf)
    yy, xx = np.mgrid[0:H, 0:W]                    # gradient + noise: encodable at these qualities, every block different
    base = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * 2 + yy * 5) % 256], axis=-1)
    rgb = ((base + rng.integers(0, 48, (H, W, 3))) % 256).astype(np.uint8)
    Y, Cb, Cr = (np.asarray(p, dtype=np.uint8).reshape(-1) for p in orc.convert(rgb))
    quarter = (W // 2) * (H // 2)
    y, cb, cr = Y.reshape(1, H, W), Cb[:quarter].reshape(1, H // 2, W // 2), Cr[:quarter].reshape(1, H // 2, W // 2)
    assert len(np.unique(cb)) > 20 and len(np.unique(cr)) > 20
    frame = dp.model_frames(dp.replicated_planes(y, cb, cr))[0]
    assert np.array_equal(frame, np.concatenate([Y, Cb[:quarter], Cr[:quarter]]))
    got = plane_oracle.encode_layout(frame, plane_layout_preset(W, H, "i420"), W, H, 7, qf, m)
    assert got == orc.encode_frame(rgb, W, H, 7, qf, m)


# ---- the census: the noise inputs are sensitive ---------------------------------------------------------------------------------
def _records(orc, frames, W, H, mode, q):
    from ec504_imageencoder_amd import plane_layout_preset
    lay = plane_layout_preset(W, H, "i420")
    m = orc.MODE_FULL if mode == "full" else orc.MODE_STRICT
    return [plane_oracle.encode_layout(frames[f], lay, W, H, f, q, m) for f in range(frames.shape[0])]


def _frames_of(planes):
    n = planes[0].shape[0]
    return np.concatenate([p.reshape(n, -1) for p in planes], 1)


def _mutants(src, xe, ye):
    """{name: the I420 frames a kernel with that mistake would code}; xe x ye: the coded region in rendition samples."""
    Y, Cb, Cr = (p.astype(np.uint16) for p in src)
    quad = lambda s: (s[:, 0::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 0::2], s[:, 1::2, 1::2])
    u8 = lambda a: a.astype(np.uint8)
    out = {}
    out["a truncating average"] = _frames_of([u8(sum(quad(s)) >> 2) for s in (Y, Cb, Cr)])
    out["the top-left sample"] = _frames_of([u8(quad(s)[0]) for s in (Y, Cb, Cr)])
    out["Cb and Cr exchanged"] = _frames_of([dp.box(src[0]), dp.box(src[2]), dp.box(src[1])])
    # the other byte phase of an interleaved pair: the first component's lanes get the second's samples, the second's get the
    # first's one sample further
    ahead = np.roll(src[1], -1, axis=2)
    out["the phases of a pair exchanged"] = _frames_of([dp.box(src[0]), dp.box(src[2]), dp.box(ahead)])

    def repeated(s, axis, last):
        t = s.copy()
        if axis == 1:
            t[:, last] = s[:, last - 1]
        else:
            t[:, :, last] = s[:, :, last - 1]
        return t

    out["the last source row of the region repeated"] = _frames_of(
        [dp.box(repeated(src[0], 1, 2 * ye - 1)), dp.box(repeated(src[1], 1, ye - 1)), dp.box(repeated(src[2], 1, ye - 1))])
    out["the last source column of the region repeated"] = _frames_of(
        [dp.box(repeated(src[0], 2, 2 * xe - 1)), dp.box(repeated(src[1], 2, xe - 1)), dp.box(repeated(src[2], 2, xe - 1))])

    def skip_a_row(s):                 # rows 2y and 2y + 2 (the last cell: 2y and 2y + 1, there is no row behind it)
        below = np.concatenate([s[:, 2::2], s[:, -1:]], 1)
        return u8((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + below[:, :, 0::2] + below[:, :, 1::2] + 2) >> 2)

    out["rows 2y and 2y + 2"] = _frames_of([skip_a_row(s) for s in (Y, Cb, Cr)])
    # ... per plane, so that a mistake in one plane's path alone shows too
    good = [dp.box(p) for p in src]
    for i, name in enumerate(("luma", "Cb", "Cr")):
        planes = list(good)
        planes[i] = u8(sum(quad((Y, Cb, Cr)[i])) >> 2)
        out[f"a truncating average in {name} alone"] = _frames_of(planes)
    return out


@pytest.mark.parametrize("W,H,mode", CASES)
def test_census_every_mutant_changes_a_record_on_every_size(orc, W, H, mode):
    xe, ye = orc.region(orc.MODE_FULL if mode == "full" else orc.MODE_STRICT, W, H)
    src = dp.noise_source(W * 100 + H, 3, H, W)
    good = dp.model_frames(src)
    mutants = _mutants(src, xe, ye)
    assert len(mutants) == 10
    for q in QUALITIES:
        want = _records(orc, good, W, H, mode, q)
        for name, frames in mutants.items():
            assert frames.shape == good.shape
            got = _records(orc, frames, W, H, mode, q)
            assert any(g != w for g, w in zip(got, want)), (name, W, H, mode, q)


# ---- the extent Mpeg1Encoder._check_input holds a tensor's rows against -------------------------------------------------------------
def test_the_source_extent_of_the_coded_region():
    """downscale_plane_layout_extent against the last addressed byte of the coded region's samples, counted from the model's own
    addressing, for xe < W and ye < H, in every form and placement.  (The refusals of _check_input itself are held on a real
    encoder by tests/test_gpu_downscale_planes.py.)"""
    from ec504_imageencoder_amd import downscale_plane_layout_preset
    from ec504_imageencoder_amd.encoder import downscale_plane_layout_extent
    W, H, strips, mb_rows = 40, 24, 2, 1                    # xe = 32 < W, ye = 16 < H
    for preset in dp.PRESETS:
        for where in (dp.TIGHT, dp.PITCHED):
            lay = dp.geometry(W, H, preset, **where)[0]
            if not where:
                assert lay == downscale_plane_layout_preset(W, H, preset)
            last = int(np.flatnonzero(dp.addressed(lay, 1, 16 * strips, 16 * mb_rows, 0, lay["frame_stride"]))[-1])
            assert downscale_plane_layout_extent(lay, strips, mb_rows) == last + 1, (preset, where)
    lay = downscale_plane_layout_preset(W, H, "nv12")
    E = downscale_plane_layout_extent(lay, strips, mb_rows)
    assert E == 4 * W * H + (16 - 1) * 2 * W + (32 - 1) * 2 + 1 + 1 and E < 6 * W * H

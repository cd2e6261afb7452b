"""One call of the encoder each, synchronised and brought to the host as lists and bytes, with the noise frames and the oracle's
records that the GPU tests hold them against.  Every function is handed torch (the value of a torch_cuda fixture) and the
encoder, so importing this module touches no GPU."""
import ctypes as C

import numpy as np

import plane_oracle
import rd_oracle as rd


def _frames(rng, n, W, H, channels, amp=256):
    """n frames of noise (amp 256) or of gentle noise around mid-grey (small amp)."""
    shape = (n, H, W, channels)
    if amp >= 256:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (128 - amp // 2 + rng.integers(0, amp, shape)).astype(np.uint8)


def _mixed_frames(rng, n, W, H, channels, amps=(4, 40, 256, 120)):
    """Frames whose record sizes differ a lot: flat, gentle and full noise in turn."""
    return np.concatenate([_frames(rng, 1, W, H, channels, amps[f % len(amps)]) for f in range(n)])


def _oracle_sizes(orc, rgb, mode, q, channels):
    W, H = rgb.shape[2], rgb.shape[1]
    return [len(orc.encode_frame(rgb[f], W, H, f, int(q), mode, channels=channels)) for f in range(rgb.shape[0])]


def _oracle(orc, rgb, first, qs, mode, channels):
    W, H = rgb.shape[2], rgb.shape[1]
    recs = [orc.encode_frame(rgb[f], W, H, first + f, int(qs[f]), mode, channels=channels) for f in range(rgb.shape[0])]
    return b"".join(recs), [len(r) for r in recs]


def _table(torch, enc, dev, quals):
    st = torch.full((len(quals),), 0x40, dtype=torch.int32, device="cuda")
    t = enc.frame_size_table(dev, quals, status=st)
    enc.flush()
    torch.cuda.synchronize()
    return t.cpu().numpy().tolist(), [int(x) for x in st.cpu()]


def _encode(torch, enc, dev, first, quality=None):
    """One asynchronous encode into a worst-case buffer -> (bytes, sizes); the status word must be 0."""
    n = dev.shape[0]
    out = torch.empty(enc.frame_bound * max(n, 1), dtype=torch.uint8, device="cuda")
    out, sizes, meta = enc.encode(dev, first, out=out, quality=quality)
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    assert status & 0xFFFFFFFF == 0, status
    return out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()]


def _frame_rule(s, cap):
    """m1v_encode_budget_device's rule on a table s[k][f]: the largest candidate that fits, else the smallest."""
    pick = []
    for f in range(len(s[0])):
        fits = [k for k in range(len(s)) if s[k][f] <= cap]
        pick.append(fits[-1] if fits else 0)
    return pick, [f for f in range(len(s[0])) if s[pick[f]][f] > cap]


def _oracle_on_buffer(orc, buf, n, lay, base, W, H, first, qs, mode):
    """plane_oracle's records of the frames as they lie in the device buffer (asserts that every frame is encodable)."""
    host = buf.cpu().numpy()
    return [plane_oracle.encode_layout(host[base + f * lay["frame_stride"]:], lay, W, H, first + f, qs[f], mode) for f in range(n)]


def _rd(torch, enc, dev, quals):
    """(sizes, distortion, status) of one frame_rd_table call as lists."""
    st = torch.full((len(quals),), 0x40, dtype=torch.int32, device="cuda")
    s, d = enc.frame_rd_table(dev, quals, status=st)
    enc.flush()
    torch.cuda.synchronize()
    return s.cpu().numpy().tolist(), d.cpu().numpy().tolist(), [int(x) for x in st.cpu()]


def _rd_device(torch, enc, dev, cands, rule, limit, first, limits=None, want_chosen=True, want_dist=True):
    """One m1v_encode_rd_device call through the C entry point -> (bytes, sizes, chosen, distortion, status)."""
    from ec504_imageencoder_amd import _ffi
    n = dev.shape[0]
    out = torch.empty(enc.frame_bound * max(n, 1), dtype=torch.uint8, device="cuda")
    sizes = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    chosen = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") if want_chosen else None
    dist = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda") if want_dist else None
    meta = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_limits = torch.tensor(list(limits), dtype=torch.int64).cuda() if limits is not None else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    cbuf = (C.c_uint8 * len(cands))(*cands)
    rc = _ffi.lib().m1v_encode_rd_device(enc._h, p(dev), n, first, cbuf, len(cands), rule, int(limit), p(d_limits), p(chosen), p(out),
                                         out.numel(), p(sizes), p(dist), C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _ffi.last_error()
    enc.flush()
    torch.cuda.synchronize()
    total, status = (int(x) for x in meta.cpu())
    return (out[:total].cpu().numpy().tobytes(), [int(s) for s in sizes[:n].cpu()],
            [int(c) for c in chosen[:n].cpu()] if want_chosen else None,
            [int(d) for d in dist[:n].cpu()] if want_dist else None, status & 0xFFFFFFFF)


def _model(rule, s, d, limits, out=()):
    """The model's picks for every frame of a table s / d [k][f]: (k per frame, frames over their limit)."""
    picks, over = [], []
    for f in range(len(s[0])):
        k, o = rd.pick(rule, [row[f] for row in s], [row[f] for row in d], limits[f], out)
        picks.append(k)
        if o:
            over.append(f)
    return picks, over


def _unencodable(enc, n):
    """The picture of test_unencodable_level_is_reported, tiled: at quality 92 every block has |level| 308 after a zero."""
    yy = np.mgrid[0:enc.height, 0:enc.width][0]
    a = ((yy % 8) < 4).astype(np.uint8) * 255
    return np.ascontiguousarray(np.broadcast_to(a[None, :, :, None], (n, enc.height, enc.width, enc.channels)))

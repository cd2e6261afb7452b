"""The checker of the rd table and of the rate-distortion picks — TEST INFRASTRUCTURE ONLY (no tests in this module).

The distortion comes from the oracle alone (include/mpeg1_hip.h, "Distortion and rate-distortion picks"): the raw coefficients
of a frame are its levels at quality 100, where every divisor is 1; the levels at quality q come from the same call; the
divisors in zigzag order are the quantised image of the scaled matrix itself under divisors of 1.  For plane layouts the
coefficients come from hard_content.plane_coefficients on the samples plane_oracle.layout_samplers addresses.  The module also
holds a Python model of the two pick rules of m1v_encode_rd_device."""
import numpy as np

UNENCODABLE = 1
BEST_IN_BUDGET, SMALLEST_AT_DISTORTION = 0, 1


def divisors_zigzag(orc, q):
    """The 64 divisors of quality q in zigzag position."""
    return orc.quant_zigzag(orc.scale_qmatrix(q), np.ones(64, np.int32)).astype(np.int64)


def carried(levels):
    """bool [blocks, 64]: position 0 and the AC positions the record codes — the non-zero levels at p >= 1 below the first
    p >= 1 whose level and whose predecessor's level are both non-zero."""
    nz = np.asarray(levels).reshape(-1, 64) != 0
    pair = nz[:, 1:] & nz[:, :-1]                                 # column p - 1: the pair (p - 1, p)
    stop = np.where(pair.any(1), pair.argmax(1) + 1, 64)
    pos = np.arange(64)[None, :]
    return (pos == 0) | (nz & (pos >= 1) & (pos < stop[:, None]))


def block_distortion(c, levels, d):
    """int64 [blocks]: sum over carried p of (c - l d)^2 + sum over the others of c^2."""
    c = np.asarray(c, np.int64).reshape(-1, 64)
    lv = np.asarray(levels, np.int64).reshape(-1, 64)
    err = c - lv * np.asarray(d, np.int64)[None, :]
    return np.where(carried(lv), err * err, c * c).sum(1)


def frame_distortion(orc, rgb, W, H, q, mode, channels=3):
    """D(frame, q) of one packed frame [H, W, channels]."""
    c = orc.frame_coefficients(rgb, W, H, 100, mode, channels)
    lv = orc.frame_coefficients(rgb, W, H, int(q), mode, channels)
    return int(block_distortion(c, lv, divisors_zigzag(orc, q)).sum())


def frame_encodable(orc, rgb, W, H, q, mode, channels=3):
    try:
        orc.encode_frame(rgb, W, H, 0, int(q), mode, channels)
        return True
    except ValueError:
        return False


def rd_table(orc, rgb, quals, mode, channels=3):
    """(sizes [K][n], distortion [K][n], status [K]) of packed frames [n, H, W, channels]; a row whose status carries
    UNENCODABLE holds None where the oracle cannot code the frame."""
    n, H, W = rgb.shape[:3]
    sizes, dist, status = [], [], []
    for q in quals:
        row_s, row_d, st = [], [], 0
        for f in range(n):
            try:
                row_s.append(len(orc.encode_frame(rgb[f], W, H, f, int(q), mode, channels)))
            except ValueError:
                row_s.append(None)
                st = UNENCODABLE
            row_d.append(frame_distortion(orc, rgb[f], W, H, q, mode, channels))
        sizes.append(row_s)
        dist.append(row_d)
        status.append(st)
    return sizes, dist, status


def plane_frame_blocks(frame, layout, W, H, mode, orc):
    """The three planes' samples of one frame as the macroblock loops see them: (luma [ye, xe], cb, cr [ye / 2, xe / 2])."""
    import plane_oracle
    xe, ye = orc.region(mode, W, H)
    luma_block, chroma_block = plane_oracle.layout_samplers(frame, layout)
    Y = np.zeros((ye, xe), np.uint8)
    Cb, Cr = np.zeros((ye // 2, xe // 2), np.uint8), np.zeros((ye // 2, xe // 2), np.uint8)
    for x in range(0, xe, 16):
        for y in range(0, ye, 16):
            for b in range(4):
                bx, by = x + (b % 2) * 8, y + (b // 2) * 8
                Y[by:by + 8, bx:bx + 8] = luma_block(bx, by)
            Cb[y // 2:y // 2 + 8, x // 2:x // 2 + 8] = chroma_block(0, x, y)
            Cr[y // 2:y // 2 + 8, x // 2:x // 2 + 8] = chroma_block(1, x, y)
    return Y, Cb, Cr


def plane_frame_distortion(orc, frame, layout, W, H, q, mode):
    """D(frame, q) of one frame of planes (a flat uint8 array from the frame's base) under a plane layout."""
    import hard_content
    d = divisors_zigzag(orc, q)
    return int(sum(block_distortion(hard_content.plane_coefficients(orc, p, 100), hard_content.plane_coefficients(orc, p, q), d).sum()
                   for p in plane_frame_blocks(frame, layout, W, H, mode, orc)))


def pick(rule, sizes, dist, limit, out=()):
    """The candidate index k that m1v_encode_rd_device picks for one frame and whether the frame is over its limit.
    sizes, dist: the frame's record size and distortion per candidate; out: the candidates out of the running."""
    ks = [k for k in range(len(sizes)) if k not in out]
    if not ks:
        return 0, False
    if rule == BEST_IN_BUDGET:
        fit = [k for k in ks if sizes[k] <= limit]
        if fit:
            return min(fit, key=lambda k: (dist[k], sizes[k], k)), False
        return min(ks, key=lambda k: (sizes[k], k)), True
    ok = [k for k in ks if dist[k] <= limit]
    if ok:
        return min(ok, key=lambda k: (sizes[k], dist[k], k)), False
    return min(ks, key=lambda k: (dist[k], sizes[k], k)), True


def largest_that_fits(sizes, limit):
    """The rule of m1v_encode_budget_device: the largest k whose record fits, else 0."""
    fit = [k for k in range(len(sizes)) if sizes[k] <= limit]
    return fit[-1] if fit else 0


def gradient_frame(W, H):
    """The smooth gradient of DESIGN.md's table: R = x * 255 // W, G = y * 255 // H, B = (x + y) * 255 // (W + H)."""
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(np.stack([x * 255 // W, y * 255 // H, (x + y) * 255 // (W + H)], -1).astype(np.uint8))


GRADIENT_QUALITIES = (5, 12, 25, 38, 50, 64, 76, 92)
GRADIENT_BYTES = (3149, 4915, 6272, 7815, 8497, 8936, 9930, 7507)
GRADIENT_D = (27369167, 9614405, 2832887, 1400207, 1232963, 855643, 499606, 21412120)

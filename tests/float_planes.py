"""What the float plane tests share (tests/test_float_planes_cpu.py, tests/test_gpu_float_planes.py): the rule of
include/mpeg1_hip.h ("Float plane layout") in numpy and in exact rational arithmetic, sample types as bit patterns (bf16 has no
numpy dtype: uint16 patterns shifted into fp32), and builders of test contents, each a pure function of its arguments.

A sample array is always held as its bit patterns: uint16 for "float16" and "bfloat16", uint32 for "float32"."""
import fractions

import numpy as np

KINDS = ("float16", "bfloat16", "float32")
BYTES = {"float16": 2, "bfloat16": 2, "float32": 4}
SCALE = {"unit": 255.0, "byte": 1.0}


def to_f32(bits, kind):
    """The fp32 values of an array of bit patterns of `kind` (exact for all three)."""
    bits = np.asarray(bits)
    if kind == "float16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    if kind == "bfloat16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert kind == "float32"
    return bits.astype(np.uint32).view(np.float32)


def from_f32(values, kind):
    """Bit patterns of `kind` for fp32 values that the type holds exactly (asserted)."""
    values = np.asarray(values, dtype=np.float32)
    if kind == "float16":
        bits = values.astype(np.float16).view(np.uint16)
    elif kind == "bfloat16":
        bits = (values.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    else:
        bits = values.view(np.uint32).copy()
    back = to_f32(bits, kind)
    assert np.array_equal(back.view(np.uint32), values.view(np.uint32)), f"values are not exact in {kind}"
    return bits


def rule_bytes(bits, kind, rng):
    """THE rule: np.clip(np.where(np.isnan(t), 0, np.rint(t)), 0, 255) with t = x.astype(np.float32) * np.float32(scale)."""
    with np.errstate(all="ignore"):
        t = to_f32(bits, kind) * np.float32(SCALE[rng])
        assert t.dtype == np.float32
        return np.clip(np.where(np.isnan(t), np.float32(0), np.rint(t)), 0, 255).astype(np.uint8)


def round_to_f32(q):
    """A non-negative Fraction rounded once to fp32, ties to even, as a Fraction; None = it rounds to +inf."""
    if q == 0:
        return q
    e = q.numerator.bit_length() - q.denominator.bit_length()       # 2^(e-1) < q < 2^(e+1)
    if fractions.Fraction(2) ** e > q:
        e -= 1                                                      # 2^e <= q < 2^(e+1)
    ulp = fractions.Fraction(2) ** (max(e, -126) - 23)
    n = q / ulp
    lo = n.numerator // n.denominator
    rest = n - lo
    half = fractions.Fraction(1, 2)
    lo += 1 if rest > half or (rest == half and lo & 1) else 0
    out = lo * ulp
    return None if out >= fractions.Fraction(2) ** 128 else out


def exact_byte(bits, kind, rng):
    """The byte of ONE bit pattern by the definition in exact rational arithmetic: the sample as a Fraction, the product rounded
    once to fp32 (ties to even), that rounded to an integer (ties to even: Fraction.__round__), clamped."""
    f = to_f32(np.array([bits]), kind)[0]
    if np.isnan(f) or f <= 0:               # NaN; -0, +0 and every negative value: the product is NaN or <= 0
        return 0
    if np.isinf(f):
        return 255
    t = round_to_f32(fractions.Fraction(float(f)) * fractions.Fraction(SCALE[rng]))
    if t is None:
        return 255
    return int(min(max(round(t), 0), 255))


def boundary_values():
    """The 765 fp32 values around the rounding boundaries of range unit: the nearest fp32 to (k + 0.5) / 255 for k = 0 ... 254 and
    each one's two neighbours, as bit patterns (uint32), sorted."""
    mid = np.array([np.float32(fractions.Fraction(2 * k + 1, 510)) for k in range(255)], dtype=np.float32)
    bits = mid.view(np.uint32)
    out = np.sort(np.concatenate([bits - np.uint32(1), bits, bits + np.uint32(1)]))
    assert len(np.unique(out)) == 765
    return out


def ties_byte_range(kind):
    """k + 0.5 for every k the type holds exactly (0 ... 254; bf16: k < 128), as bit patterns."""
    ks = np.arange(128 if kind == "bfloat16" else 255)
    return from_f32(ks.astype(np.float32) + np.float32(0.5), kind)


def all_patterns(kind):
    """Every pattern of a 16-bit type; for float32 the fp32 images of all fp16 and all bf16 patterns."""
    p = np.arange(65536, dtype=np.uint32)
    if kind != "float32":
        return p.astype(np.uint16)
    return np.concatenate([to_f32(p, "float16").view(np.uint32), to_f32(p, "bfloat16").view(np.uint32)])


def special_f32():
    """fp32 patterns the definition names: +-0, +-inf, NaNs of both signs (quiet, signalling, several payloads), the largest and
    the smallest denormal of both signs, +-FLT_MAX, +-FLT_MIN."""
    return np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fa5a5a5,
                     0xffffffff, 0x7fffffff, 0x7fc12345, 0x007fffff, 0x807fffff, 0x00000001, 0x80000001, 0x7f7fffff, 0xff7fffff,
                     0x00800000, 0x80800000], dtype=np.uint32)


def tie_picture(rounding="even"):
    """The tie picture as the bytes a front half with that rounding of ties would code: 256 x 256, 1,024 flat 8 x 8 blocks, block b
    holding k + 0.5 with k = perm[b] % 255 (perm a fixed permutation of 0 ... 1023), R = G = B, range byte.  Returns (k per
    pixel as int [256, 256], bytes uint8 [256, 256, 3] under `rounding`: "even", "up" (k + 1) or "down" (k))."""
    perm = np.random.default_rng(23).permutation(1024) % 255
    k = np.kron(perm.reshape(32, 32), np.ones((8, 8), dtype=np.int64))
    byte = {"even": k + (k & 1), "up": k + 1, "down": k}[rounding].astype(np.uint8)
    return k, np.repeat(byte[:, :, None], 3, axis=2)


def tie_picture_samples(kind):
    """The tie picture as samples of `kind` [3, 256, 256] (bit patterns), and the bytes the rule gives for them [256, 256, 3].
    bf16 holds k + 0.5 only for k < 128: its picture takes k % 128."""
    k, _ = tie_picture()
    if kind == "bfloat16":
        k = k % 128
    plane = from_f32(k.astype(np.float32) + np.float32(0.5), kind)
    byte = (k + (k & 1)).astype(np.uint8)
    return np.stack([plane] * 3), np.repeat(byte[:, :, None], 3, axis=2)


def boundary_picture():
    """The 765 boundary values as flat 8 x 8 blocks of a 256 x 256 fp32 picture (block b holds value b % 765), R = G = B, range
    unit: (samples uint32 [3, 256, 256], the rule's bytes uint8 [256, 256, 3])."""
    vals = boundary_values()[np.arange(1024) % 765]
    plane = np.kron(vals.reshape(32, 32).astype(np.uint64), np.ones((8, 8), dtype=np.uint64)).astype(np.uint32)
    byte = rule_bytes(plane, "float32", "unit")
    return np.stack([plane] * 3), np.repeat(byte[:, :, None], 3, axis=2)


def jitter_noise(seed, n, H, W, kind, rng="unit", amplitude=256):
    """Noise whose samples are (byte + jitter) / 255 (range unit) or byte + jitter (range byte), jitter uniform in +-0.49,
    rounded to `kind`: (samples as bit patterns [n, 3, H, W], the rule's bytes as a packed picture uint8 [n, H, W, 3]).  The
    rule's bytes are computed from the rounded samples, so they are the byte drawn wherever the type resolves the jitter and
    whatever the rule says elsewhere."""
    g = np.random.default_rng(seed)
    byte = g.integers(0, amplitude, (n, 3, H, W)).astype(np.float64)
    x = (byte + g.uniform(-0.49, 0.49, byte.shape)) / (255.0 if rng == "unit" else 1.0)
    x32 = x.astype(np.float32)
    if kind == "float16":
        bits = x32.astype(np.float16).view(np.uint16)
    elif kind == "bfloat16":    # round to nearest even on the upper 16 bits
        u = x32.view(np.uint32)
        bits = ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    else:
        bits = x32.view(np.uint32).copy()
    return bits, np.ascontiguousarray(rule_bytes(bits, kind, rng).transpose(0, 2, 3, 1))

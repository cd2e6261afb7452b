"""The reference's fine-grained ABI: libencoder.so exports all 52 functions + 14 data objects of the
reference's shared library as a CPU link-compatibility shim (csrc/compat_primitives.c).  CPU-only tests:
export list, code tables against the SHA-256 self-checks recorded in SURVEY §8(a), a block-level comparison
with the oracle, and — where the reference is present — the reference's OWN main.c compiled against the
reference's OWN header (driver inside main.o) linked to this library: byte-identical files."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ec504_imageencoder_amd", "libencoder.so")

FUNCS = """bitvector_fwrite bitvector_new bitvector_put_bit check_dimensions convert_rgb_to_ycbcr encode_block_end
encode_block_header_i encode_macroblock_header_i equalize_coefficients extract_8x8_block fast_DCT mpeg1_file_header mpeg1_gop
mpeg1_packet_header mpeg1_picture_header mpeg1_sequence_header mpeg1_slice mpeg1_sys_header quantization run_length_encode
subsampling_420 write_to_bitstream zigzag_scanning DCT IDCT VLC_encode bitvector_clone bitvector_concat bitvector_expand_size
bitvector_init bitvector_pos bitvector_print bitvector_put_binstring bitvector_put_byte bitvector_put_byte_ent
bitvector_put_byte_off bitvector_toarray concat_char convert_ycbcr_to_rgb dequantization display_u8arr encode_blk_coeff
encode_coeff_sz_fast encode_macblk_address_value encode_macblk_encoding_value encode_macroblock_end fast_IDCT insert_8x8_block
mpeg1_sequence_end print_array scale_quantization_matrix upsampling""".split()
DATA = """Q_MATRIX ZIGZAG_ORDER START_FILE START_PICTURE blk_coeff_1_f blk_coeff_1_n blk_coeff_end blk_rle_lookup blk_rle_table
dc_sz_chroma_table dc_sz_luma_table encoding_table mv_encoding_table slice_start_code""".split()


class VlcEntry(C.Structure):
    _fields_ = [("binstring", C.c_char_p), ("bit_len", C.c_uint)]


class RleEntry(C.Structure):
    _fields_ = [("run", C.c_uint), ("level", C.c_uint), ("code", VlcEntry)]


class BitVector(C.Structure):
    _fields_ = [("value", C.POINTER(C.c_char)), ("bits", C.c_longlong), ("cursor", C.c_longlong), ("cap", C.c_longlong)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ec504_imageencoder_amd", "csrc")], check=True)
    return C.CDLL(LIB)


def test_every_reference_symbol_is_exported(lib):
    assert len(FUNCS) == 52 and len(DATA) == 14
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in FUNCS + DATA if s not in exported]


def test_code_tables_match_the_survey_checksums(lib):
    def sha(lines):
        return hashlib.sha256("".join(lines).encode()).hexdigest()
    rle = (RleEntry * 111).in_dll(lib, "blk_rle_table")
    assert sha([f"{e.run},{e.level},{e.code.binstring.decode()}\n" for e in rle[:110]]) == \
        "508a2ffc3678d52df51e5af2c3626b8c7faf7a7f22318026f569430c37c179fc"
    assert rle[110].code.binstring is None
    addr = (VlcEntry * 36).in_dll(lib, "encoding_table")
    assert sha([f"{i},{addr[i].binstring.decode()}\n" for i in range(1, 36)]) == \
        "a25beba38c1785b06eb62336b26831cd836e2820f54bc828fd2b330e8111e6cb"
    luma = (VlcEntry * 9).in_dll(lib, "dc_sz_luma_table")
    chroma = (VlcEntry * 9).in_dll(lib, "dc_sz_chroma_table")
    assert sha([f"{i},{luma[i].binstring.decode()}\n" for i in range(9)]) == \
        "7c49a3e85605f063ae117472b2bb2e651ff8c36707f7553a9f7818cdec4c5b6d"
    assert sha([f"{i},{chroma[i].binstring.decode()}\n" for i in range(9)]) == \
        "febd3155447adfde60381e2de01392ad9f0393eb27434fe8f5560d1790fbfd28"
    look = (C.c_uint * 33).in_dll(lib, "blk_rle_lookup")
    assert list(look)[:4] == [0, 39, 57, 62] and look[32] == 110


def test_block_chain_matches_the_oracle(lib, orc):
    """fast_DCT -> quantization -> zigzag_scanning -> run_length_encode -> encode_block_header_i -> encode_block_end
    through the shim == the oracle's bits, on random and extreme blocks."""
    lib.bitvector_new.restype = C.POINTER(BitVector)
    lib.bitvector_new.argtypes = [C.c_char_p, C.c_longlong]
    rng = np.random.default_rng(5)
    blocks = [rng.integers(0, 256, 64, dtype=np.uint8) for _ in range(200)]
    blocks += [np.full(64, v, np.uint8) for v in (0, 255)] + [(rng.integers(0, 2, 64) * 255).astype(np.uint8) for _ in range(50)]
    for qf in (12, 50, 90):
        for blk in blocks:
            dct = np.zeros(64, np.float64)
            lib.fast_DCT(blk.ctypes.data_as(C.c_void_p), dct.ctypes.data_as(C.c_void_p))
            assert np.array_equal(dct.astype(np.int32), orc.fdct(blk))
            qz, zz, pairs = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(136, np.int32)
            lib.quantization(dct.ctypes.data_as(C.c_void_p), qz.ctypes.data_as(C.c_void_p), qf)
            lib.zigzag_scanning(qz.ctypes.data_as(C.c_void_p), zz.ctypes.data_as(C.c_void_p))
            assert np.array_equal(zz, orc.quant_zigzag(dct.astype(np.int32), orc.scale_qmatrix(qf)))
            lib.run_length_encode(zz.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p))
            for luma in (1, 0):
                rc, want = orc.encode_block_bits(luma, zz)
                if rc != 0:
                    continue
                bv = lib.bitvector_new(b"", 8)
                lib.encode_block_header_i(luma, pairs.ctypes.data_as(C.c_void_p), bv)
                lib.encode_block_end(bv)
                n = bv.contents.cap
                raw = C.string_at(bv.contents.value, (n + 7) // 8)
                assert "".join(f"{x:08b}" for x in raw)[:n] == want


def test_block_coder_over_the_whole_code_space(lib, orc):
    """run_length_encode -> encode_block_header_i -> encode_block_end through the shim over tests/code_space.exhaustive_groups:
    every run row with every level -255..255 behind a DC level of 1 and of 0, every DC level -2042..2042, luma and chroma.  The
    shim's own copy of the 110-entry table, its escapes and its DC size tables give the oracle's bits, entry by entry."""
    import code_space as cs
    lib.bitvector_new.restype = C.POINTER(BitVector)
    lib.bitvector_new.argtypes = [C.c_char_p, C.c_longlong]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    pairs = np.zeros(136, np.int32)
    for name, blocks in cs.exhaustive_groups().items():
        for luma, zz in blocks:
            rc, want = orc.encode_block_bits(luma, zz)
            assert rc == 0
            lib.run_length_encode(zz.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p))
            bv = lib.bitvector_new(b"", 8)
            lib.encode_block_header_i(luma, pairs.ctypes.data_as(C.c_void_p), bv)
            lib.encode_block_end(bv)
            n = bv.contents.cap
            raw = C.string_at(bv.contents.value, (n + 7) // 8)
            got = "".join(f"{x:08b}" for x in raw)[:n]
            libc.free(C.cast(bv.contents.value, C.c_void_p))
            libc.free(C.cast(bv, C.c_void_p))
            assert got == want, (name, "luma" if luma else "chroma", "levels", zz[zz != 0].tolist(), got, want)


@pytest.mark.reference
def test_reference_main_object_links_and_matches(ref, lib, tmp_path):
    """main.o built from the reference's main.c AND the reference's header by `make -C oracle _ref` (the driver is inside main.o and needs
    the fine-grained symbols) + this library == the reference's own binary, byte for byte (.mpeg and .bit)."""
    from PIL import Image
    obj, exe = os.path.join(ROOT, "oracle", "_ref", "main_ref.o"), tmp_path / "legacy_encoder"   # `make -C oracle _ref`
    if not os.path.exists(obj):
        pytest.skip("oracle/_ref/main_ref.o not built (reference sources absent)")
    und = subprocess.run(["nm", "-u", str(obj)], capture_output=True, text=True).stdout
    needed = {l.split()[-1] for l in und.splitlines() if "GLIBC" not in l and " U " in l}
    assert "fast_DCT" in needed and "mpeg_encode_procedure" not in needed
    subprocess.run(["gcc", "-o", str(exe), str(obj), f"-L{os.path.dirname(LIB)}", "-lencoder",
                    f"-Wl,-rpath,{os.path.dirname(LIB)}", "-lm"], check=True)
    rng = np.random.default_rng(17)
    (tmp_path / "images").mkdir(); (tmp_path / "bitstreams").mkdir(); (tmp_path / "refbits").mkdir()
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (288, 352, 3), dtype=np.uint8)).save(str(tmp_path / "images" / f"f{i}.jpg"), quality=92)
    assert subprocess.run([str(exe)], cwd=tmp_path, stdout=subprocess.DEVNULL).returncode == 0
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_encoder_strict"), "images/", "refbits", "refbits/awesome_video.mpeg", "12"],
                   cwd=tmp_path, stdout=subprocess.DEVNULL, check=True)
    assert (tmp_path / "bitstreams" / "awesome_video.mpeg").read_bytes() == (tmp_path / "refbits" / "awesome_video.mpeg").read_bytes()
    for k in (1, 2, 3):
        assert (tmp_path / "bitstreams" / f"image_{k}.bit").read_bytes() == (tmp_path / "refbits" / f"image_{k}.bit").read_bytes()


def _bits(bv):
    n = bv.contents.cap
    raw = C.string_at(bv.contents.value, (n + 7) // 8)
    return "".join(f"{x:08b}" for x in raw)[:n]


@pytest.mark.reference
def test_decoder_side_symbols_match_the_reference(ref, lib):
    """the decoder-side / unused helpers the library exports for link compatibility — DCT, IDCT,
    fast_IDCT, dequantization, upsampling, insert_8x8_block, subsampling_420, encode_macblk_encoding_value,
    mpeg1_sequence_end (image_processing.c:157,438,452,492,607,641,114; vlc.c:108; mpeg1_enc.c:96) — against the
    reference's own shared library (oracle/_ref/libencoder_ref.so) on random inputs, bit for bit."""
    R = ref.lib()
    rng = np.random.default_rng(41)
    vp = C.c_void_p

    def ptr(a):
        return a.ctypes.data_as(vp)

    # DCT / IDCT: float accumulator updated per term -> bitwise equal floats / bytes
    blocks = [rng.integers(0, 256, 64, dtype=np.uint8) for _ in range(300)] + [np.full(64, v, np.uint8) for v in (0, 1, 128, 255)]
    for blk in blocks:
        a, b = np.zeros(64, np.float32), np.zeros(64, np.float32)
        lib.DCT(ptr(blk), ptr(a))
        R.DCT(ptr(blk), ptr(b))
        assert a.tobytes() == b.tobytes()
        back_a, back_b = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        lib.IDCT(ptr(a), ptr(back_a))
        R.IDCT(ptr(b), ptr(back_b))
        assert np.array_equal(back_a, back_b)
    for _ in range(300):  # IDCT on coefficients that were never a DCT output (clamping both ways, ties of round())
        coef = (rng.standard_normal(64) * rng.choice([1.0, 30.0, 400.0])).astype(np.float32)
        if rng.integers(0, 2):
            coef = np.round(coef * 2) / 2
        coef = coef.astype(np.float32)
        a, b = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        lib.IDCT(ptr(coef), ptr(a))
        R.IDCT(ptr(coef), ptr(b))
        assert np.array_equal(a, b)

    # fast_IDCT (the reference's "inverse" re-applies the forward network; pinned as is) and dequantization
    for _ in range(500):
        dct = np.round(rng.standard_normal(64) * rng.choice([2.0, 60.0, 900.0])).astype(np.float64)
        a, b = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        lib.fast_IDCT(ptr(dct), ptr(a))
        R.fast_IDCT(ptr(dct), ptr(b))
        assert np.array_equal(a, b)
        q = rng.integers(-300, 300, 64).astype(np.int32)
        da, db = np.zeros(64, np.float64), np.zeros(64, np.float64)
        lib.dequantization(ptr(q), ptr(da))
        R.dequantization(ptr(q), ptr(db))
        assert da.tobytes() == db.tobytes()

    # subsampling_420 -> upsampling, even dimensions (the reference reads / leaves gaps out of bounds for odd ones)
    u8p = C.POINTER(C.c_uint8)
    libc = C.CDLL(None)
    libc.free.argtypes = [vp]
    for (W, H) in ((16, 16), (48, 32), (352, 288)):
        cb = rng.integers(0, 256, W * H, dtype=np.uint8)
        cr = rng.integers(0, 256, W * H, dtype=np.uint8)
        outs = []
        for L in (lib, R):
            L.subsampling_420.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(u8p), C.POINTER(u8p)]
            L.upsampling.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(u8p), C.POINTER(u8p)]
            s1, s2, f1, f2 = u8p(), u8p(), u8p(), u8p()
            L.subsampling_420(ptr(cb), ptr(cr), W, H, C.byref(s1), C.byref(s2))
            sub = (C.string_at(s1, (W // 2) * (H // 2)), C.string_at(s2, (W // 2) * (H // 2)))
            L.upsampling(s1, s2, W, H, C.byref(f1), C.byref(f2))
            outs.append(sub + (C.string_at(f1, W * H), C.string_at(f2, W * H)))
            for p in (s1, s2, f1, f2):
                libc.free(p)
        assert outs[0] == outs[1]

    # insert_8x8_block
    for _ in range(20):
        W = int(rng.integers(8, 40))
        plane_a = rng.integers(0, 256, W * 24, dtype=np.uint8)
        plane_b = plane_a.copy()
        blk = rng.integers(0, 256, 64, dtype=np.uint8)
        x0, y0 = int(rng.integers(0, W - 7)), int(rng.integers(0, 17))
        lib.insert_8x8_block(ptr(plane_a), W, x0, y0, ptr(blk))
        R.insert_8x8_block(ptr(plane_b), W, x0, y0, ptr(blk))
        assert np.array_equal(plane_a, plane_b)

    # motion-vector code words (unused by an I-frame encoder): every value, including the out-of-range NULLs
    for L in (lib, R):
        L.encode_macblk_encoding_value.restype = C.POINTER(BitVector)
        L.encode_macblk_encoding_value.argtypes = [C.c_int]
    for v in range(-20, 21):
        a, b = lib.encode_macblk_encoding_value(v), R.encode_macblk_encoding_value(v)
        assert bool(a) == bool(b)
        if a:
            assert _bits(a) == _bits(b) and a.contents.cursor == b.contents.cursor

    a, b = (C.c_uint8 * 4)(), (C.c_uint8 * 4)()
    lib.mpeg1_sequence_end(a)
    R.mpeg1_sequence_end(b)
    assert bytes(a) == bytes(b) == b"\x00\x00\x01\xb7"


def test_deliberate_differences_of_the_shim(lib, tmp_path):
    """What the shim does NOT copy from the reference, asserted so that the list in compat_primitives.c stays true:
    convert_ycbcr_to_rgb converts the planes it is given (image_processing.c:650 reads the buffer it has just malloc'ed);
    bitvector_fwrite / bitvector_toarray keep the valid bits of a final partial byte (bit_vector.c:136-144 writes a
    stale byte); concat_char returns heap memory (mpeg1_enc.c:145 returns a pointer to its own stack frame)."""
    class Img(C.Structure):
        _fields_ = [("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("data", C.POINTER(C.c_uint8))]
    rng = np.random.default_rng(3)
    W, H = 16, 8
    Y, Cb, Cr = (rng.integers(0, 256, W * H, dtype=np.uint8) for _ in range(3))
    img = Img(W, H, 3, None)
    lib.convert_ycbcr_to_rgb(Y.ctypes.data_as(C.c_void_p), Cb.ctypes.data_as(C.c_void_p), Cr.ctypes.data_as(C.c_void_p), C.byref(img))
    got = np.frombuffer(C.string_at(img.data, W * H * 3), np.uint8).reshape(-1, 3)
    y, cb, cr = Y.astype(np.float64), Cb.astype(np.float64) - 128, Cr.astype(np.float64) - 128
    want = np.stack([np.trunc(y + 1.402 * cr), np.trunc(y - 0.344136 * cb - 0.714136 * cr), np.trunc(y + 1.772 * cb)], 1)
    assert np.array_equal(got, np.clip(want, 0, 255).astype(np.uint8))
    C.CDLL(None).free(C.cast(img.data, C.c_void_p))

    lib.bitvector_new.restype = C.POINTER(BitVector)
    lib.bitvector_new.argtypes = [C.c_char_p, C.c_longlong]
    bv = lib.bitvector_new(b"1011011101", 16)  # 10 bits: one whole byte + 2 valid bits
    out = (C.c_char * 4)()
    lib.bitvector_toarray.argtypes = [C.POINTER(BitVector), C.c_void_p]
    assert lib.bitvector_toarray(bv, out) == 2 and bytes(out)[:2] == bytes([0b10110111, 0b01000000])

    lib.concat_char.restype = C.c_void_p
    lib.concat_char.argtypes = [C.c_char_p, C.c_char_p]
    p = lib.concat_char(b"abcdefgh", b"ijklmnop")
    assert p and C.string_at(p, 16) == b"abcdefghijklmnop"  # sizeof(char *) = 8 bytes of each, as the reference counts them
    C.CDLL(None).free(C.c_void_p(p))

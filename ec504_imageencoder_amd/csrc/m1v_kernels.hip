// ec504_imageencoder_amd/csrc/m1v_kernels.hip — MI355X (gfx950 / CDNA4) kernels and the C-ABI of
// include/mpeg1_hip.h.  Written for gfx950 only: 64-wide waves, LDS-staged bit packing, 5 waves per SIMD.
//
// Data layout in HBM
//   input    n_frames x (H x W x C) interleaved u8, as the reference's Image::data (jpeg_handler.h:6-11)
//            (or, with a surface layout, windows of pitched surfaces: m1v_set_input_layout)
//   scratch  one compact slot per unit of the encode kernel (a tile of 8 strips x 4 macroblock rows, or a run of 256 blocks)
//            + an overflow arena of worst-case slots; a strip = 16-pixel-wide COLUMN of macroblocks (encoder.h:238
//            iterates x outermost) and is byte aligned (encoder.h:442), so strips are independent units of bit packing;
//            a segment table (bits, where) per (frame, segment, strip); per-strip bit counters, per-frame byte totals
//   output   contiguous frame records  PKT SEQ GOP PIC strips 00000000  (encoder.h:196-458)
//
// Kernels
//   k_encode_tiles    (m1v_tiles.h) the encode kernel of every 3-channel picture: a workgroup per tile of 8 strips x 4
//                     macroblock rows, pixels in as whole 128-byte lines by LDS-DMA, one lane per 8x8 block
//   k_encode_surface, k_size_table_surface   (m1v_tiles.h, m1v_encode_tile_body.h, m1v_size_table_body.h) the same tile
//                     encode and size table on windows of pitched surfaces, 3- or 4-byte pixels in R,G,B or B,G,R order
//                     (m1v_set_input_layout: row r of frame f at base + f * frame stride + r * row pitch)
//   k_encode_planes, k_size_table_planes     (m1v_planes.h, the same two bodies) the tile encode and size table on planar and
//                     semi-planar YCbCr frames (m1v_set_plane_layout: reference planes, I420 / YV12, NV12 / NV21, pitched
//                     windows of them): no colour stage, bytes straight into the fp32 FDCT
//   k_encode_rgb_planes, k_size_table_rgb_planes, k_rd_table_rgb_planes   (m1v_rgb_planes.h, the same bodies) the tile kernels on
//                     planes of R, G and B bytes (m1v_set_rgb_plane_layout: NCHW uint8 tensors in any plane order): the colour
//                     stage of the surface kernels on de-interleaved bytes
//   k_encode_float_planes, k_size_table_float_planes, k_rd_table_float_planes   (m1v_float_planes.h, the same bodies) the tile
//                     kernels on planes of fp16, bf16 or fp32 samples of R, G and B (m1v_set_float_plane_layout: NCHW float
//                     tensors): each sample becomes a byte by one rule (float_sample_to_byte), then the stage above
//   k_float_pixels_encode, k_float_pixels_size_table, k_float_pixels_rd_table   (m1v_float_pixels.h, the same bodies) the tile
//                     kernels on float samples of R, G and B interleaved per pixel (m1v_set_float_pixel_layout: NHWC and
//                     channels-last float tensors, RGBA16F / RGBA32F targets), by the same rule
//   k_downscale_encode, k_downscale_size_table, k_downscale_rd_table   (m1v_downscale.h, the same bodies) the tile kernels on the
//                     2 x 2 box average of byte surfaces of twice the encoder's width and height (m1v_set_downscale_layout):
//                     the rendition is averaged in registers and never written
//   k_half_planes_encode, k_half_planes_size_table, k_half_planes_rd_table   (m1v_downscale_planes.h, the same bodies) the tile
//                     kernels on the 2 x 2 box average of planar and semi-planar YCbCr frames of twice the encoder's width and
//                     height (m1v_set_downscale_plane_layout), by the same rule
//   k_half_words_encode, k_half_words_size_table, k_half_words_rd_table   (m1v_downscale_words.h, the same bodies) the tile
//                     kernels on the 2 x 2 box average of YCbCr frames of 16-bit words of twice the encoder's width and height
//                     (m1v_set_downscale_word_layout): averaged at the word's precision, then shifted down to a byte
//   k_encode_dense    the run kernel (4-channel pictures; round 2's hot kernel).  A frame's blocks, in
//                     stream order, are cut into runs of T consecutive blocks (default 256); one
//                     workgroup per (frame, run), one LANE per 8x8 block (Y0..Y3, Cb, Cr of each
//                     macroblock down the strip).  Per lane: 8 rows x 24 B of RGB -> component (three
//                     fp32 FMAs; an unfused fp64 fix-up where the fp32 result is within 2 eps of an
//                     integer, so results equal the reference's fp64 arithmetic bit for bit) ->
//                     two-pass integer FDCT in registers -> quantise -> zigzag positions staged in LDS
//                     as int8 (min AC divisor >= 8) or int16 -> DC/AC code words.  Bit lengths are
//                     prefix-summed across the workgroup (DPP wave scan, one barrier), the bits are
//                     OR-ed into an LDS image of the run (<= 2 byte-aligned strip segments) and stored
//                     once.  Workgroups are dealt to XCDs so one frame's runs share an L2.
//   k_encode_strips   one 64-lane workgroup per (frame, strip) for small pictures (< 64 blocks/strip)
//   k_dense_frame_layout   run kernel only: run metadata -> segment table, strip bit counts, frame bytes
//   k_assemble        (m1v_assemble.h) ONE launch behind every encode kernel: frame and strip offsets, the strips' segments
//                     at their final bit positions, frame headers, 16-bit length back-patch, trailer, sizes, status
//   k_size_table_tiles, k_size_table_rgba   (m1v_tiles.h, m1v_size_table_body.h) record sizes at up to 8 qualities in one pass of the
//                     tile workgroup, for 3- and 4-channel pictures; k_size_table_sizes writes them out
//   k_rd_table_tiles, _rgba, _surface, _planes   (the same body with its distortion stage) the size table plus the exact
//                     distortion of every frame at every quality; k_rd_table_sizes writes both out.  k_rd_pick picks a candidate
//                     per frame by both (m1v_encode_rd_device)
//   k_coefficients    FDCT+quant+zigzag only (BASELINE config 2)
//   k_convert, k_subsample, k_synth   plane conversion / 4:2:0 / synthetic input
//
// Reference citations are file:line under /root/reference.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <utility>
#include <algorithm>
#include <vector>

#include "../../include/mpeg1_hip.h"

#define M1V_HD __host__ __device__ __forceinline__
#include "fdct_f32.h"

#pragma clang fp contract(off) // colour conversion must stay unfused (image_processing.c:104-106)

namespace {

// ------------------------------------------------------------------------------------------------
// constant geometry
// ------------------------------------------------------------------------------------------------
constexpr int kWave = 64;
// VLC table, one private copy per wave in LDS (192 words: a wave fills and reads only its own copy, so the waves of a
// workgroup need not meet between the pixel stage and the entropy stage):
//   [0, 32)    per run row r = run - 1:  first entry | entries << 8   (vlc.c:172-174, the offset index)
//   [32, 142)  the 110 run/level entries in the reference's order, (bits << 16) | code  (vlc.c:176-288)
//   [144, 153) luma DC size codes, [160, 169) chroma DC size codes              (vlc.c:121-144)
constexpr int kAcRows = 32;
constexpr int kVlcRowInfo = 0, kVlcEntries = 32, kVlcDcLuma = 144, kVlcDcChroma = 160, kVlcWords = 192;
constexpr int kMaxBlockBits = 886;
constexpr int kDefaultLdsWords = 4096;            // 16 KiB strip image in LDS (strip-per-workgroup kernel)

// zigzag position of natural-order coefficient [u][i] (image_processing.c:28-37)
__host__ __device__ constexpr int scan_pos(int k) {
    constexpr int t[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                           3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                           10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                           21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return t[k];
}
// natural-order index of zigzag position p
__host__ __device__ constexpr int scan_inv(int p) {
    for (int k = 0; k < 64; k++)
        if (scan_pos(k) == p) return k;
    return -1;
}

// LDS staging of one block's 64 quantised levels, "zigzag class" layout.  A block owns kStageStride consecutive
// words (an odd stride: the lanes of a wave hit different banks).  Narrow form (one BYTE per level, exact whenever no
// AC level can reach +-128, which the host decides from the quantiser alone): word (p & 7) + 8 (p >> 5) holds the
// levels at zigzag positions p, p+8, p+16, p+24 in its four bytes.  Wide form (int16): word (p & 15) + 16 (p >> 5)
// holds positions p and p+16.  The point of the layout: the "is this byte non-zero" flags of one word, computed for
// all four bytes at once, land on zigzag positions that differ by 8, so ONE shift puts them in place in the 64-bit
// non-zero mask (stage_nonzero_mask) — 1.25 instructions per coefficient instead of a compare, a select and an OR.
// The run kernels fill the words with one LDS byte (halfword) store per level (block_to_stage) and read them back for the mask;
// the tile kernels build the same words in registers and store them whole (StagePack, m1v_tiles.h).
constexpr int kStageStride8 = 17, kStageStride16 = 33;
__host__ __device__ constexpr int stage_byte8(int p) { return ((p & 7) + 8 * (p >> 5)) * 4 + ((p >> 3) & 3); }
__host__ __device__ constexpr int stage_byte16(int p) { return ((p & 15) + 16 * (p >> 5)) * 4 + 2 * ((p >> 4) & 1); }

// Device-resident tables, built by m1v_create.
struct Tables {
    float rq[64];               // inflated reciprocal of the scaled quantiser, natural order [u][i]
    float rq_t[64];             // the same, transposed [i][u]: one 32-byte scalar load per column pass
    uint32_t vlc[kVlcWords];    // see kVlc*
    uint8_t hdr[256][44];       // PKT SEQ GOP PIC for hour = 0..255, length field zero
};

struct Geometry {
    int W, H, C;
    int n_strips, n_mbrows;     // x_extent/16, y_extent/16
    int half_w;                 // W / 2 (stride of the chroma quirk, encoder.h:347)
    uint32_t strip_cap;         // bytes of one scratch slot (multiple of 16)
    unsigned long long frame_bytes;
};

#ifdef M1V_STAMPS
// Diagnostic build only (tools/stamps.py): per-phase cycle sums, lane 0 of every wave adds the cycles it
// spent between two stamps into stamps[phase].  Never compiled into the shipped library.
#define STAMP(ph)                                                                                  \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        unsigned long long now_ = __builtin_amdgcn_s_memtime();                                    \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                                        \
        if ((threadIdx.x & 63) == 0) atomicAdd(&a.stamps[ph], now_ - stamp_t_);                    \
        stamp_t_ = __builtin_amdgcn_s_memtime();                                                   \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    } while (0)
#define STAMP_INIT() unsigned long long stamp_t_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F)
#elif defined(M1V_MARKS)
// Analysis build only (tools/isa_phases.py): comment markers in the .s between phases.
#define STAMP(ph) asm volatile("; PHASE_MARK " #ph ::: "memory")
#define STAMP_INIT() asm volatile("; PHASE_MARK start" ::: "memory")
#else
#define STAMP(ph) do { } while (0)
#define STAMP_INIT() do { } while (0)
#endif

struct EncodeArgs {
    Geometry g;
    const uint8_t *rgb;
    const Tables *tab;
    const float *rq_all;        // quantiser of every quality (see frame_rq_t)
    const uint32_t *qsel;       // [frame]: where the frame's quantiser lies in rq_all
    uint8_t *scratch;           // [frame][strip][strip_cap]
    uint2 *seg;                 // [frame][strip]: (bits of the strip, where it starts in scratch: 4-byte words) — one segment per strip
    unsigned long long *strip_ctr;   // [frame][strip]: bits of the strip
    unsigned long long *frame_bytes; // [frame]: every strip adds its bytes (zero before the batch: k_assemble of the batch before)
    uint32_t *status;
    int n_frames;
    int threads;                // workgroup size
    int lds_words;              // capacity of the LDS strip image
    unsigned long long *stamps; // diagnostic builds only
};

// ------------------------------------------------------------------------------------------------
// pixel stage
// ------------------------------------------------------------------------------------------------

// One colour component, exactly as image_processing.c:104-106 evaluates it: fp64, left to right,
// one rounding per operation, truncation to u8.  (k0,kr,kg,kb) select Y / Cb / Cr:
//   Y  = 0.299 r + 0.587 g + 0.114 b              -> (0,   .299,     .587,     .114)
//   Cb = 128 - 0.168736 r - 0.331264 g + 0.5 b     -> (128, -.168736, -.331264, .5)
//   Cr = 128 + 0.5 r - 0.418688 g - 0.081312 b     -> (128, .5,       -.418688, -.081312)
// a - c*x == a + (-c)*x and 0 + c*x == c*x hold exactly in IEEE arithmetic.
__device__ __forceinline__ int component_fp64(int r, int g, int b, double k0, double kr, double kg,
                                              double kb) {
    double acc = k0 + kr * (double)r;
    acc = acc + kg * (double)g;
    acc = acc + kb * (double)b;
    return (int)acc;
}

struct CompCoef {
    double k0, kr, kg, kb;
};
__device__ __forceinline__ CompCoef comp_coef(int comp) { // 0 = Y, 1 = Cb, 2 = Cr
    CompCoef c;
    c.k0 = comp == 0 ? 0.0 : 128.0;
    c.kr = comp == 0 ? 0.299 : (comp == 1 ? -0.168736 : 0.5);
    c.kg = comp == 0 ? 0.587 : (comp == 1 ? -0.331264 : -0.418688);
    c.kb = comp == 0 ? 0.114 : (comp == 1 ? 0.5 : -0.081312);
    return c;
}

// fp32 coefficients of the same three formulas, for the fast path below.  k0 carries +256 + kEps.
constexpr float kEps = 1.5e-4f;
struct CompCoefF {
    float k0, kr, kg, kb;
    CompCoef d; // the reference's fp64 coefficients of the same component, for the pixels the fp32 form cannot decide
};
__device__ __forceinline__ CompCoefF comp_coef_f(int comp) {
    CompCoefF c;
    c.k0 = (comp == 0 ? 0.0f : 128.0f) + 256.0f + kEps;
    c.kr = comp == 0 ? 0.299f : (comp == 1 ? -0.168736f : 0.5f);
    c.kg = comp == 0 ? 0.587f : (comp == 1 ? -0.331264f : -0.418688f);
    c.kb = comp == 0 ? 0.114f : (comp == 1 ? 0.5f : -0.081312f);
    c.d = comp_coef(comp);
    return c;
}
// The same for a wave whose lanes all convert luma (first = true) or convert Cb in lanes 0-31 and Cr in lanes 32-63 (the
// waves of a tile, m1v_tiles.h): a scalar branch and, on the chroma side, one select per register — a third of the vector
// instructions the general three-way selects of comp_coef_f take per wave (12 registers; the fp64 ones are loop invariants
// the compiler sets up in front of the rows either way).
__device__ __forceinline__ CompCoefF comp_coef_wave(bool luma_wave, int lane) {
    CompCoefF c;
    if (luma_wave) {
        asm volatile(""); // keeps the branch: two arms of selects would be merged back into three-way selects
        c = comp_coef_f(0);
    } else {
        asm volatile("");
        const CompCoefF cb = comp_coef_f(1), cr = comp_coef_f(2);
        const bool hi = lane >= 32;
        c.k0 = cb.k0;
        c.kr = hi ? cr.kr : cb.kr;
        c.kg = hi ? cr.kg : cb.kg;
        c.kb = hi ? cr.kb : cb.kb;
        c.d.k0 = cb.d.k0;
        c.d.kr = hi ? cr.d.kr : cb.d.kr;
        c.d.kg = hi ? cr.d.kg : cb.d.kg;
        c.d.kb = hi ? cr.d.kb : cb.d.kb;
    }
    return c;
}

// Same value as component_fp64 for every (r,g,b), at fp32 cost, and already the float the fp32 FDCT (fdct_f32.h) takes.
// The exact rational value x of a formula is a multiple of 1e-6 in [0, 255.5].  Three fp32 FMAs starting from
// k0 + 256 + eps give t = x + 256 + eps + e with |e| < 1e-4 < eps (three half-ulps of 2^-15, three coefficient
// roundings, the rounding of the constant); the reference's fp64 result differs from x by < 1e-12.  t lies in
// [256, 512) for every input, so the float's exponent is fixed and its low 15 mantissa bits are the fraction:
//     raw pixel      p = t with those 15 bits cleared = 256 + trunc(t - 256)     (one v_and_b32; kPxBiasF + value)
//     fraction       d = t - p                                                   (exact)
// If d >= kFracLow (> 2 eps) then x >= trunc(t - 256) + d - eps - 1e-4 lies at least 0.5e-4 above that integer and,
// as d < 1, at least eps - 1e-4 below the next one: trunc(fp64 result) == trunc(t - 256).  Otherwise (x an exact
// integer — where fp64 rounding decides the byte — or less than 1.5e-4 above one: 0.16 % of the pixels) the lane
// re-evaluates the reference's fp64 expression.  The row's smallest d is reduced with v_min3_f32 (two pixels per
// instruction) and compared once per row.  Raw pixels keep their bias through the FDCT: every multiplier input of the
// butterflies is a difference (bias cancels), only the DC sum carries 64 * kPxBiasF, removed in fdct_col_f.
// Proof over all 2^24 triples x 3 components: tools/colour_fast_proof.c (host) and the GPU tests.
constexpr float kFracLow = 10.0f / 32768.0f;
__device__ __forceinline__ float component_t(uint32_t r, uint32_t g, uint32_t b, const CompCoefF &k) {
    float t = fmaf((float)b, k.kb, k.k0);
    t = fmaf((float)g, k.kg, t);
    return fmaf((float)r, k.kr, t);
}
__device__ __forceinline__ float clear_fraction(float t) { return __uint_as_float(__float_as_uint(t) & 0xffff8000u); }
// raw pixel (kPxBiasF + value) of one component, per-pixel branch (plane conversion and the byte-load input mode)
__device__ __forceinline__ float component_raw(uint32_t r, uint32_t g, uint32_t b, const CompCoefF &k) {
    const float t = component_t(r, g, b, k);
    float p = clear_fraction(t);
    if (t - p < kFracLow) {
        const CompCoef &d = k.d;
        p = m1vf::kPxBiasF + (float)component_fp64((int)r, (int)g, (int)b, d.k0, d.kr, d.kg, d.kb);
    }
    return p;
}

#define M1V_CONST_AS __attribute__((address_space(4)))

// Per-frame quality.  rq_all holds Tables::rq_t of every quality factor, [quality - 1][64] (m1v_create; the entry of the
// encoder's own quality is bit-identical to its Tables::rq_t), and qsel[frame] is the offset in floats of the frame's entry:
// the encoder's own quality for every frame on the plain path, the caller's per-frame choice (k_frame_quality) otherwise.
// The frame is workgroup-uniform, so the selection is ONE scalar load per workgroup, in front of the table's own scalar
// loads; no branch, no vector load.
__device__ __forceinline__ const float *frame_rq_t(const float *rq_all, const uint32_t *qsel, int frame) {
    const M1V_CONST_AS uint32_t *sel = reinterpret_cast<const M1V_CONST_AS uint32_t *>(reinterpret_cast<uintptr_t>(qsel));
    return rq_all + sel[frame];
}


// The tile kernels run their fp32 arithmetic rounded TOWARD MINUS INFINITY: fdct_row_f<float, true> takes two floors of
// products that round (fdct_f32.h) and needs that mode; the colour sums are proven for it as well as for the default
// (tools/colour_fast_proof.c down: the same pixels are flagged, none is wrong), the reciprocal quantiser likewise
// (tests/test_host_tables.py), and everything else in the stage is exact.  MODE[1:0] = 2; the fp64 mode bits (the colour
// fallback re-evaluates the reference's expression) stay at round-to-nearest.  The frame's base pointer passes through the
// statement, so no load of a pixel — and no arithmetic on one — can be scheduled in front of the switch; so do the two tile
// coordinates, the results of the kernel's last integer divisions (the compiler expands those through v_rcp_iflag_f32 and a
// float multiply: they stay in the default mode; tests/test_abi.py checks the code object for both).
// The run kernel keeps the default mode and the integer form: measured 1 % faster there (profiles/r03_ab_history.txt).
// The switch writes MODE bits 1:0 only (offset 0, width 2): the fp32 denormal bits 5:4 keep the kernel descriptor's value,
// denormals enabled, which the luma waves' colour sums rely on (luma_sums_denormal: flushed, every colour byte would read
// as 0).  No flush flag belongs in the Makefile for the same reason; tests/test_luma_denormal_cpu.py reads the descriptors.
__device__ __forceinline__ const uint8_t *pixel_stage_rounds_down(const uint8_t *frame_base, int &u0, int &u1) {
    unsigned long long p = (unsigned long long)(uintptr_t)frame_base;
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 2" : "+s"(p), "+s"(u0), "+s"(u1));
    return (const uint8_t *)(uintptr_t)p;
}

struct __attribute__((aligned(4))) Row24 {
    uint32_t d[6];
};

// 8 pixels of one block row (24 or 32 bytes already in registers) -> 8 raw pixels.  One "is any pixel of this row
// uncertain?" branch per row instead of one per pixel: the branch is taken by about half of the waves, and then only
// the flagged pixels redo the fp64 expression.
// ORDER: M1V_ORDER_BGR = colour ch is byte 2 - ch of the pixel.  The permutation is applied where the bytes are extracted: the
// arithmetic below sees (r, g, b) in the orders tools/colour_fast_proof.c proves.
template <int BPP, bool LEAN, int ORDER = 0, typename RowT>
__device__ __forceinline__ void convert_row(const RowT &v, const CompCoefF &k, float out[8]) {
    auto chan = [&](int j, int ch) -> uint32_t {
        int byte = BPP * j + (ORDER ? 2 - ch : ch);
        return (v.d[byte >> 2] >> ((byte & 3) * 8)) & 0xffu;
    };
    float lowest = 1.0f;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const float t0 = component_t(chan(j, 0), chan(j, 1), chan(j, 2), k);
        const float t1 = component_t(chan(j + 1, 0), chan(j + 1, 1), chan(j + 1, 2), k);
        out[j] = clear_fraction(t0);
        out[j + 1] = clear_fraction(t1);
        lowest = fminf(fminf(lowest, t0 - out[j]), t1 - out[j + 1]);
    }
    if (lowest < kFracLow) { // rare: redo the row's flagged pixels in the reference's arithmetic
        // Written as a recomputation from the row's bytes (same instructions, same values); on the main path (aligned
        // 3-byte pixels) the compiler instead keeps the eight sums alive across the branch (measured 8 % faster than
        // recomputing: the branch is taken for half of the rows).  The input modes with more raw registers per row (4-byte
        // pixels, funnel-shifted rows) cannot afford those eight registers inside the 96-VGPR budget (200+ B of scratch
        // per lane): LEAN hides the bytes' origin behind an empty asm and so forces the recomputation.
        RowT w = v;
        if constexpr (LEAN) {
#pragma unroll
            for (int i = 0; i < (int)(sizeof(RowT) / 4); i++) asm("" : "+v"(w.d[i]));
        }
        auto chan2 = [&](int j, int ch) -> uint32_t {
            int byte = BPP * j + (ORDER ? 2 - ch : ch);
            return (w.d[byte >> 2] >> ((byte & 3) * 8)) & 0xffu;
        };
        const CompCoef &d = k.d;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t r = chan2(j, 0), gg = chan2(j, 1), b = chan2(j, 2);
            const float t = component_t(r, gg, b, k);
            if (t - clear_fraction(t) < kFracLow)
                out[j] = m1vf::kPxBiasF + (float)component_fp64((int)r, (int)gg, (int)b, d.k0, d.kr, d.kg, d.kb);
        }
    }
}

// The three FMAs of component_t for a wave whose lanes all convert LUMA from packed R,G,B bytes (waves 0, 1 of a tile,
// m1v_tiles.h), without the twenty-four v_cvt_f32_ubyteN of a row (4.75 cycles each against 2.5 for a v_and_b32 with a literal,
// profiles/r01_valu_rates.txt).  A colour byte is taken where it lies in its dword, position q = (3j + ch) & 3, and read as a
// float:
//     w & (0xff << 8q), q = 0, 1, 2  =  b * 2^(8q - 149);      w >> 24, q = 3  =  b * 2^-149 (the scale of q = 0)
// a denormal, which v_fma_f32 takes at full rate.  Its coefficient is fl32(k_ch) * 2^(125 - 8q) (a literal: the wave's
// component is a compile-time constant) and the sum starts from (k0 + 256 + eps) * 2^-24.  A power-of-two rescale of an fp32
// coefficient is exact and every product is the unit-scale product * 2^-24, so every FMA rounds where component_t's does, in
// round-to-nearest and in the wave's round-down mode: t' = t * 2^-24 bit for bit in the mantissa, in [2^-16, 2^-15), normal.
// Needs fp32 denormals enabled (the compiler's default for gfx950; pixel_stage_rounds_down leaves MODE's denormal bits alone).
// Proof over all 2^24 triples x the four dword phases of a pixel, both rounding modes: tools/colour_fast_proof.c denormal [down].
__device__ __forceinline__ void luma_sums_denormal(const Row24 &v, float k0, float t[8]) {
    constexpr float kY[3] = {0.299f, 0.587f, 0.114f};
    constexpr float kScale[4] = {0x1p125f, 0x1p117f, 0x1p109f, 0x1p125f}; // by byte position q
    auto chan = [&](int j, int ch) -> float {
        const int byte = 3 * j + ch, q = byte & 3;
        const uint32_t w = v.d[byte >> 2];
        return __uint_as_float(q == 3 ? w >> 24 : w & (0xffu << (8 * q)));
    };
    auto coef = [&](int j, int ch) -> float { return kY[ch] * kScale[(3 * j + ch) & 3]; };
#pragma unroll
    for (int j = 0; j < 8; j++) {
        t[j] = fmaf(chan(j, 2), coef(j, 2), k0);
        t[j] = fmaf(chan(j, 1), coef(j, 1), t[j]);
        t[j] = fmaf(chan(j, 0), coef(j, 0), t[j]);
    }
}

// convert_row<3, ., 0> of the tile kernels that round down (m1v_tiles.h): one wave-uniform branch around the eight sums — the
// luma waves take luma_sums_denormal, the chroma wave component_t with its per-lane coefficients — and ONE tail for both,
// which reads a sum's bit pattern and so does not care which of the two scales it has (the exponent is fixed at either):
//     fraction       the low 15 mantissa bits L as an integer; t - p < kFracLow  <=>  L < 10   (t - p = L * 2^-15 exactly)
//     raw pixel      (bits & 0x007f8000) | bits(256.0f) = clear_fraction(t)                      (ONE v_and_or_b32)
// so the luma pixels return to unit scale without a multiply.  Only the eight sums live across the rare branch (the pixels are
// cut from them behind it; a flagged pixel's sum is replaced by its raw pixel, which the and-or leaves as it is): eight
// registers fewer than convert_row holds there, at no instruction more.  The rare branch is convert_row's: the same pixels
// flagged, the reference's fp64 expression with the wave's k.d, no fp64 FMA.  It is marked unlikely (taken by about half of
// the rows, but its code — eight pixels' fp64 expressions — is placed behind the kernel's hot path, not between the rows).
// The two constants of the row that need a vector register (v_fmamk_f32 takes its addend, v_and_or_b32 its third operand, from
// one), set up once in front of the rows: opaque, or the compiler moves them into a register again in every row.
struct TileRowConst {
    float k0;      // (256 + eps) * 2^-24: where a luma sum starts
    uint32_t bias; // bits of kPxBiasF
};
__device__ __forceinline__ TileRowConst tile_row_const() {
    TileRowConst c = {(256.0f + kEps) * 0x1p-24f, __float_as_uint(m1vf::kPxBiasF)};
    asm("" : "+v"(c.k0), "+v"(c.bias));
    return c;
}
__device__ __forceinline__ void convert_row_tile(const Row24 &v, const CompCoefF &k, const TileRowConst &c, bool luma_wave, float out[8]) {
    float t[8];
    if (luma_wave) {
        luma_sums_denormal(v, c.k0, t);
    } else {
        auto chan = [&](int j, int ch) -> uint32_t { return (v.d[(3 * j + ch) >> 2] >> (((3 * j + ch) & 3) * 8)) & 0xffu; };
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = component_t(chan(j, 0), chan(j, 1), chan(j, 2), k);
    }
    uint32_t L[8], lowest = 0x7fffu;
#pragma unroll
    for (int j = 0; j < 8; j++) L[j] = __float_as_uint(t[j]) & 0x7fffu;
#pragma unroll
    for (int j = 0; j < 8; j += 2) lowest = min(min(lowest, L[j]), L[j + 1]);
    if (__builtin_expect(lowest < 10u, 0)) { // redo the row's flagged pixels in the reference's arithmetic
        // (the bytes' origin is hidden, as convert_row's LEAN does: a byte at position 0 or 3 was masked to its own value by
        // the luma sums, and left visible the twelve of them stay in registers across the branch)
        Row24 w = v;
#pragma unroll
        for (int i = 0; i < 6; i++) asm("" : "+v"(w.d[i]));
        const CompCoef &d = k.d;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (L[j] < 10u) {
                auto byte_of = [&](int ch) -> int { return (int)((w.d[(3 * j + ch) >> 2] >> (((3 * j + ch) & 3) * 8)) & 0xffu); };
                t[j] = m1vf::kPxBiasF + (float)component_fp64(byte_of(0), byte_of(1), byte_of(2), d.k0, d.kr, d.kg, d.kb);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t p;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(p) : "v"(t[j]), "s"(0x007f8000u), "v"(c.bias));
        out[j] = __uint_as_float(p);
    }
}

// 8 pixels of one block row -> 8 raw pixels.  FAST: C == 3 and the row starts 4-byte aligned.
template <bool FAST>
__device__ __forceinline__ void load_row(const uint8_t *p, int C, const CompCoefF &k, float out[8]) {
    if (FAST) {
        Row24 v = *reinterpret_cast<const Row24 *>(p);
        convert_row<3, false>(v, k, out);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint8_t *q = p + j * C;
            out[j] = component_raw(q[0], q[1], q[2], k);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// block stage: the reference's integer FDCT (image_processing.c:192-307) in exact fp32 arithmetic, in registers:
// fdct_f32.h (m1vf::fdct_row_f, m1vf::fdct_col_f).
// ------------------------------------------------------------------------------------------------

// Truncating division by the scaled quantiser (image_processing.c:367) as one fp32 multiply by an
// inflated reciprocal rq = fl((1/d)(1+2^-20)): exact for |n| < 2^15, 1 <= d <= 4150
// (tests/test_host_tables.py checks every (n, d) pair on the host).  n arrives as a float holding the integer.
__device__ __forceinline__ int quant(float n, float rq) { return (int)(n * rq); }

// Where block `bidx` of a strip reads its 64 pixels (encoder.h:275-278 luma, :347-348 chroma).
// Returns the index of the first pixel and the row stride, both in pixels.
struct BlockSrc {
    uint32_t first;  // 32-bit on purpose (m1v_create rejects frames of 4 GiB and more): a row's address is then a uniform
    uint32_t stride; // 64-bit frame base + a 32-bit lane offset, which the load instruction adds itself
    int blk;    // 0..5 inside the macroblock: Y0 Y1 Y2 Y3 Cb Cr
    __device__ int comp() const { return blk < 4 ? 0 : blk - 3; } // 0 Y, 1 Cb, 2 Cr (derived: one register less to keep)
};
__device__ __forceinline__ BlockSrc block_source(const Geometry &g, int strip, int bidx) {
    BlockSrc s;
    int mb = bidx / 6;
    s.blk = bidx - mb * 6;
    if (s.blk < 4) {
        int x0 = strip * 16 + (s.blk & 1) * 8;
        int y0 = mb * 16 + (s.blk >> 1) * 8;
        s.first = (uint32_t)y0 * (uint32_t)g.W + (uint32_t)x0;
        s.stride = (uint32_t)g.W;
    } else { // full-resolution Cb/Cr plane addressed with stride W/2 at (x/2, y/2)
        s.first = (uint32_t)(mb * 8) * (uint32_t)g.half_w + (uint32_t)(strip * 8);
        s.stride = (uint32_t)g.half_w;
    }
    return s;
}


// raw pixels of one block -> the 64 quantised levels, natural order q[u*8+i] (BASELINE config 2 kernel)
template <bool FAST>
__device__ __forceinline__ void block_coefficients(const Geometry &g, const uint8_t *frame,
                                                   const BlockSrc &s, const float *rq, int q[64]) {
    float rows[64];
    CompCoefF k = comp_coef_f(s.comp());
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float px[8];
        load_row<FAST>(frame + (size_t)((s.first + (uint32_t)i * s.stride) * (uint32_t)g.C), g.C, k, px);
        m1vf::fdct_row_f<float, false>(px, &rows[i * 8]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float c[8];
        m1vf::fdct_col_f<float>(rows[0 * 8 + i], rows[1 * 8 + i], rows[2 * 8 + i], rows[3 * 8 + i], rows[4 * 8 + i],
                                rows[5 * 8 + i], rows[6 * 8 + i], rows[7 * 8 + i], c, i == 0 ? 8.0f * m1vf::kPxBiasF : 0.0f);
#pragma unroll
        for (int u = 0; u < 8; u++) q[u * 8 + i] = quant(c[u], rq[u * 8 + i]);
    }
}

// ------------------------------------------------------------------------------------------------
// entropy stage
// ------------------------------------------------------------------------------------------------

// One run/level code word (vlc.c:315-385 with the reference's indexing): r = run - 1 >= 0,
// level != 0.  Table code when row r holds an entry for |level| - 1 (for r = 0 that is the entry of |level| + 1, and
// "11" for |level| = 1: the table's first entry is stored as that special case), else the escape "000001" + 6-bit run
// + 8 or 16 bits of level (vlc.c:346-381); |level| >= 256 cannot be coded (the reference dereferences NULL): `bad`.
// Branch-free: both table reads use an index that is always valid and the choice is made by selects, so a wave whose
// lanes disagree executes one instruction stream.  NARROW: |level| < 128 is guaranteed (byte staging).
template <bool NARROW>
__device__ __forceinline__ void ac_code(const uint32_t *vlc, int r, int level, uint32_t &code, uint32_t &bits, uint32_t &bad) {
    const uint32_t L = (uint32_t)(level < 0 ? -level : level);
    const uint32_t info = vlc[kVlcRowInfo + min(r, kAcRows - 1)];
    const bool in_table = r < kAcRows && L - 1u < (info >> 8);
    const uint32_t e = vlc[kVlcEntries + (in_table ? (info & 0xffu) + L - 1u : 0u)];
    const uint32_t head = (1u << 6) | ((uint32_t)r & 0x3fu); // "000001" + 6-bit run
    const uint32_t lo = (uint32_t)level & 0xffu;              // (u8)(+L) or (u8)(-L)
    uint32_t esc = (head << 8) | lo, esc_bits = 20;
    if (!NARROW) {
        const bool wide = L >= 128u;
        esc = wide ? (head << 16) | (level < 0 ? 0x8000u : 0u) | lo : esc;
        esc_bits = wide ? 28 : 20;
        bad |= (!in_table && L >= 256u) ? 1u : 0u;
    }
    code = in_table ? (e & 0xffffu) : esc;
    bits = in_table ? (e >> 16) : esc_bits;
}

// Pass 1 of a block: all its bits in a 64-bit register (when they fit) and their count.
//   hdr/hlen : DC part (mpeg1_blk.c:73-102), with the macroblock header "11" (mpeg1_blk.c:38-51) in front for
//              block 0
//   emit     : bit p set = the AC coefficient at zigzag position p is coded.  VLC_encode stops at the first pair
//              with run 0 (image_processing.c:421): that is the first p >= 1 with both p-1 and p non-zero.
// The register simply keeps shifting: if the count ends above 64 its content is meaningless and the block is walked
// again by pass 2 (walk_codes); no per-code bookkeeping.
template <bool NARROW, typename Fetch>
__device__ __forceinline__ void block_bits_pass1(uint32_t hdr, int hlen, bool dc_nonzero, unsigned long long emit,
                                                 const uint32_t *vlc, Fetch fetch, unsigned long long &acc, int &tot,
                                                 uint32_t &bad) {
    acc = hdr;
    tot = hlen;
    int prev = dc_nonzero ? 0 : -1;
    while (emit) {
        const int p = __builtin_ctzll(emit);
        emit &= emit - 1;
        const int r = p - prev - 2; // (zeros before this coefficient, image_processing.c:716-722) - 1, vlc.c:326
        prev = p;
        uint32_t code, bits;
        ac_code<NARROW>(vlc, r, fetch(p), code, bits, bad);
        acc = (acc << bits) | code;
        tot += (int)bits;
    }
    acc = (acc << 2) | 0x2u; // EOB "10", mpeg1_blk.c:115-117
    tot += 2;
}

// The same walk, code word by code word into `sink` (pass 2 of the rare blocks that exceed 64 bits).
template <bool NARROW, typename Fetch, typename Sink>
__device__ __forceinline__ void walk_codes(uint32_t hdr, int hlen, bool dc_nonzero, unsigned long long emit,
                                           const uint32_t *vlc, Fetch fetch, Sink &sink) {
    sink(hdr, hlen);
    int prev = dc_nonzero ? 0 : -1;
    uint32_t bad = 0;
    while (emit) {
        const int p = __builtin_ctzll(emit);
        emit &= emit - 1;
        const int r = p - prev - 2;
        prev = p;
        uint32_t code, bits;
        ac_code<NARROW>(vlc, r, fetch(p), code, bits, bad);
        sink(code, (int)bits);
    }
    sink(0x2u, 2);
}

// MSB-first OR of `bits` code bits at absolute bit position `pos` of a zero-initialised word image.
// Words are kept big-endian-logical (bit 31 = earliest bit); SWAP stores them byte-swapped so that a
// little-endian memory image is already the byte stream (used by the global-memory fallback).
template <bool SWAP>
__device__ __forceinline__ void or_code(uint32_t *img, uint32_t pos, uint32_t code, int bits) {
    uint32_t w = pos >> 5, sh = pos & 31u;
    unsigned long long v = (unsigned long long)code << (64 - bits - (int)sh);
    uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (SWAP) {
        hi = __builtin_bswap32(hi);
        lo = __builtin_bswap32(lo);
    }
    if (hi) atomicOr(&img[w], hi);
    if (lo) atomicOr(&img[w + 1], lo);
}

// exclusive prefix sum over the workgroup; every thread gets its offset, `total` the grand total
__device__ __forceinline__ uint32_t block_scan_exclusive(uint32_t v, uint32_t *wave_sums, int nthreads,
                                                         uint32_t &total) {
    int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        uint32_t o = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) wave_sums[wave] = incl;
    __syncthreads();
    int nw = nthreads >> 6;
    if (wave == 0) {
        uint32_t s = lane < nw ? wave_sums[lane] : 0;
        uint32_t si = s;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            uint32_t o = __shfl_up(si, d, kWave);
            if (lane >= d) si += o;
        }
        if (lane < nw) wave_sums[lane] = si - s; // exclusive
        if (lane == nw - 1) wave_sums[16] = si;
    }
    __syncthreads();
    uint32_t off = wave_sums[wave] + incl - v;
    total = wave_sums[16];
    __syncthreads();
    return off;
}

// Inclusive prefix sum across the 64 lanes of a wave with DPP row shifts / row broadcasts (gfx9 family):
// no index registers, 7 VALU adds.  row_shr:n = 0x110+n, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t v) {
    uint32_t x = v;
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xe, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xc, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
    return x;
}
// inclusive prefix sum across the first 16 lanes only (one DPP row)
__device__ __forceinline__ uint32_t row_scan_inclusive(uint32_t v) {
    uint32_t x = v;
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xe, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xc, false);
    return x;
}

// Same, with ONE barrier: every wave redoes the (<= 16 entry) scan of the wave totals itself.  `ws` must
// hold 2 x 16 words; callers alternate `parity` so that a buffer is rewritten only after another barrier.
__device__ __forceinline__ uint32_t block_scan_exclusive_1b(uint32_t v, uint32_t *ws, int parity, int nthreads,
                                                            uint32_t &total) {
    int lane = threadIdx.x & (kWave - 1);
    int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t incl = wave_scan_inclusive(v);
    uint32_t *buf = ws + parity * 16;
    if (lane == kWave - 1) buf[wave] = incl;
    __syncthreads();
    int nw = nthreads >> 6;
    uint32_t s = lane < nw ? buf[lane] : 0;
    uint32_t si = row_scan_inclusive(s);
    uint32_t wave_off = (uint32_t)__builtin_amdgcn_readlane((int)(si - s), wave);
    total = (uint32_t)__builtin_amdgcn_readlane((int)si, nw - 1);
    return wave_off + incl - v;
}

// XCD-aware (frame, strip) of a workgroup: consecutive workgroup ids round-robin over the 8 XCDs,
// so give each XCD whole frames (its L2 then sees every 128-byte line of the frame once).
__device__ __forceinline__ void frame_strip_of(unsigned b, int n_frames, int n_strips, int &frame,
                                               int &strip) {
    unsigned per_group = 8u * (unsigned)n_strips;
    unsigned full = (unsigned)n_frames / 8u;
    if (b < full * per_group) {
        unsigned g = b / per_group, r = b - g * per_group;
        frame = (int)(g * 8u + (r & 7u));
        strip = (int)(r >> 3);
    } else {
        unsigned t = b - full * per_group;
        frame = (int)(full * 8u + t / (unsigned)n_strips);
        strip = (int)(t % (unsigned)n_strips);
    }
}

// Division of a workgroup index by a launch constant without the compiler's float-reciprocal expansion (15 vector
// instructions per division and wave): q = high half of n * m with m = floor(2^32 / d) + 1, exact while n * d < 2^32 — the
// host checks that for the largest index of the launch and passes m = 0 (plain division) otherwise.  Scalar multiplies only.
struct DivMagic {
    uint32_t d, m;
};
M1V_HD DivMagic div_magic(uint32_t d, unsigned long long n_max) {
    DivMagic r;
    r.d = d;
    r.m = (d >= 2 && n_max * d < (1ull << 32)) ? (uint32_t)((1ull << 32) / d) + 1u : 0u;
    return r;
}
__device__ __forceinline__ uint32_t udiv(uint32_t n, const DivMagic &k) { return k.m ? __umulhi(n, k.m) : n / k.d; }
// frame_strip_of with the launch's three divisors prepared: group = 8 * per_frame, per_frame
__device__ __forceinline__ void frame_unit_of(uint32_t b, int n_frames, const DivMagic &group, const DivMagic &per_frame, int &frame,
                                              int &unit) {
    const uint32_t full = (uint32_t)n_frames / 8u;
    if (b < full * group.d) {
        const uint32_t gq = udiv(b, group), r = b - gq * group.d;
        frame = (int)(gq * 8u + (r & 7u));
        unit = (int)(r >> 3);
    } else {
        const uint32_t t = b - full * group.d, q = udiv(t, per_frame);
        frame = (int)(full * 8u + q);
        unit = (int)(t - q * per_frame.d);
    }
}

#ifndef M1V_WAVES_PER_EU
#define M1V_WAVES_PER_EU 5
#endif
#ifndef M1V_DENSE_KEEP
#define M1V_DENSE_KEEP 8 // row-pass outputs of the run kernels stay unpacked (RowStore)
#endif

// ---- pieces shared by the two encode kernels -----------------------------------------------------

// Issue the 8 row loads (8 x 24 B) of one block.
// Input modes of the dense kernel: 0 = byte loads (4 channels, or a buffer that is not 4-byte aligned),
// 1 = 3 channels and every block row starts on a 4-byte boundary (width % 8 == 0): 24-byte loads,
// 2 = 3 channels, block rows start anywhere in a 4-byte aligned buffer: 28 bytes from the dword at or below the row
//     start, funnel-shifted by the lane's misalignment (v_alignbyte_b32).
struct __attribute__((aligned(4))) Row28 {
    uint32_t d[7];
};
__device__ __forceinline__ void load_block_rows(const uint8_t *fbase, const BlockSrc &src, Row28 raw[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t *p = fbase + (size_t)((src.first + (uint32_t)i * src.stride) * 3u);
        const uint32_t m = (uint32_t)(uintptr_t)p & 3u;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p - m);
#pragma unroll
        for (int k = 0; k < 6; k++) raw[i].d[k] = q[k];
        // the seventh dword holds row bytes only when the row is misaligned; an aligned row must not touch it (it can lie
        // beyond the end of the buffer), a misaligned one shares it with a byte of the row, i.e. with a mapped page
        raw[i].d[6] = q[m ? 6 : 5];
    }
}
//     3 = 4 channels in a 4-byte aligned buffer: 32-byte rows (always aligned); rows 0..3 are requested up front, rows
//     4..7 from inside the row loop (64 raw registers would not fit next to the row-pass values).
struct __attribute__((aligned(4))) Row32 {
    uint32_t d[8];
};
__device__ __forceinline__ void load_block_rows(const uint8_t *fbase, const BlockSrc &src, Row32 raw[8]) {
#pragma unroll
    for (int i = 0; i < 4; i++)
        raw[i] = *reinterpret_cast<const Row32 *>(fbase + (size_t)((src.first + (uint32_t)i * src.stride) * 4u));
}
__device__ __forceinline__ Row24 row_bytes(const Row24 &v, const uint8_t *) { return v; }
__device__ __forceinline__ Row24 row_bytes(const Row28 &v, const uint8_t *p) {
    const uint32_t m = (uint32_t)(uintptr_t)p & 3u;
    Row24 r;
#pragma unroll
    for (int k = 0; k < 6; k++) r.d[k] = __builtin_amdgcn_alignbyte(v.d[k + 1], v.d[k], m);
    return r;
}
__device__ __forceinline__ void load_block_rows(const uint8_t *fbase, const BlockSrc &src, Row24 raw[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++)
        raw[i] = *reinterpret_cast<const Row24 *>(fbase + (size_t)((src.first + (uint32_t)i * src.stride) * 3u));
}

// rows: convert + row pass as each row's bytes arrive; columns: column pass + quantise + stage in LDS +
// non-zero mask, one column at a time (nothing but rows[] stays live).  Returns the DC level.
// The 64 outputs of the row pass, held until the column pass.  Columns KEEP..7 are stored as f16 PAIRS: every row output
// except column 0 (the plain sum, which also carries the pixel bias 8 * 256) is an integer of magnitude <= 1020, the sum
// without its bias one of magnitude <= 2040 (fdct_f32.h; tools/fdct_f32_proof.cpp checks the bounds), and f16 holds every
// integer up to 2048 exactly, so packing (v_cvt_pkrtz_f16_f32) and unpacking (v_cvt_f32_f16) lose nothing.  Column 0 always
// stays a float (KEEP >= 2).  All eight columns packed (66 VGPRs, 6 waves per SIMD) measured 0.3-2.6 % slower in a sustained
// run than all eight unpacked at 5 waves (profiles/r03_ab_history.txt) and was removed in round 4.
typedef __fp16 m1v_h2 __attribute__((ext_vector_type(2)));
template <int KEEP>
struct RowStore {
    static_assert(KEEP >= 2 && KEEP <= 8 && (8 - KEEP) % 2 == 0, "pairs of columns are packed; column 0 stays a float");
    static constexpr float kBias0 = 8.0f * m1vf::kPxBiasF; // what column 0 still carries on top of the sum
    float f[8][KEEP + 1];
    m1v_h2 h[8][(8 - KEEP) / 2 + 1];
    __device__ __forceinline__ void put(int r, const float out[8]) {
#pragma unroll
        for (int c = 0; c < KEEP; c++) f[r][c] = out[c];
#pragma unroll
        for (int c = KEEP; c < 8; c += 2) {
            m1v_h2 v = __builtin_amdgcn_cvt_pkrtz(out[c], out[c + 1]);
            // pinned here (volatile statements keep their order, and the next row's LDS read is one): left to itself the
            // scheduler sinks all packing behind the last row and the unpacked values spill
            asm volatile("" : "+v"(v));
            h[r][(c - KEEP) / 2] = v;
        }
    }
    __device__ __forceinline__ float get(int r, int c) const {
        if (c < KEEP) return f[r][c];
        return (float)h[r][(c - KEEP) / 2][(c - KEEP) & 1];
    }
};

template <int FAST, bool STAGE8, typename RowT>
__device__ __forceinline__ int block_to_stage(const Geometry &g, const uint8_t *fbase, const BlockSrc &src,
                                              const RowT raw[8], const float *rq_global, uint32_t *blk, uint32_t &lds_addr) {
    // constant address space: the table then stays a scalar load behind the volatile statements of RowStore::put
    const M1V_CONST_AS float *rq_t = reinterpret_cast<const M1V_CONST_AS float *>(reinterpret_cast<uintptr_t>(rq_global));
    RowStore<M1V_DENSE_KEEP> rows;
    CompCoefF k = comp_coef_f(src.comp());
    Row32 late[FAST == 3 ? 4 : 1];
    (void)late;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float px[8];
        if constexpr (FAST == 3) {
            if (i == 1) { // rows 4..7: requested once row 0 has been consumed
#pragma unroll
                for (int r = 0; r < 4; r++)
                    late[r] = *reinterpret_cast<const Row32 *>(fbase + (size_t)((src.first + (uint32_t)(r + 4) * src.stride) * 4u));
            }
            convert_row<4, true>(i < 4 ? raw[i] : late[i - 4], k, px);
        } else if constexpr (FAST != 0) {
            convert_row<3, FAST == 2>(row_bytes(raw[i], fbase + (size_t)((src.first + (uint32_t)i * src.stride) * 3u)), k, px);
        } else {
            load_row<false>(fbase + (size_t)((src.first + (uint32_t)i * src.stride) * (uint32_t)g.C), g.C, k, px);
        }
        float ro[8];
        m1vf::fdct_row_f<float, false>(px, ro); // default rounding mode: see pixel_stage_rounds_down
        rows.put(i, ro);
    }
    int dc = 0;
    lds_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)blk;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float c[8];
        m1vf::fdct_col_f<float>(rows.get(0, i), rows.get(1, i), rows.get(2, i), rows.get(3, i), rows.get(4, i), rows.get(5, i),
                                rows.get(6, i), rows.get(7, i), c, i == 0 ? RowStore<M1V_DENSE_KEEP>::kBias0 : 0.0f);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int q = quant(c[u], rq_t[i * 8 + u]);
            const int p = scan_pos(u * 8 + i);
            if (p == 0) dc = q; // the DC level may not fit the staged width: it stays in a register
            // one LDS byte (halfword) store per level, straight from the converted register: no packing on the vector
            // ALU.  Inline asm: plain stores are merged back into packed words by the compiler, and volatile ones (or
            // volatile asm) turn the scalar loads of the quantiser table into per-lane vector loads.  The asm
            // statements are pure as far as the compiler knows; the address register, passed in-out, chains them (and the
            // reads of stage_nonzero_mask) in program order.
            if (STAGE8)
                asm("ds_write_b8 %0, %1 offset:%2" : "+v"(lds_addr) : "v"(q), "n"(stage_byte8(p)));
            else
                asm("ds_write_b16 %0, %1 offset:%2" : "+v"(lds_addr) : "v"(q), "n"(stage_byte16(p)));
        }
    }
    return dc;
}

// Bit p set = the staged level at zigzag position p is non-zero.  Byte (or halfword) granular "non-zero" flags of a
// whole word: ((w & 0x7f..) + 0x7f..) | w has the top bit of every non-zero field set; the layout (stage_byte8/16)
// makes one shift put a word's flags on their zigzag positions.  Position 0 (DC) is the caller's.
template <bool STAGE8>
__device__ __forceinline__ unsigned long long stage_nonzero_mask(const uint32_t *blk, uint32_t lds_addr) {
    constexpr int kWords = STAGE8 ? 16 : 32;
    uint32_t w[kWords];
    // The staging stores are inline asm (block_to_stage), so the reads are too, chained behind them by lds_addr.  Eight
    // ds_read2_b32 AND their s_waitcnt in ONE statement: the compiler's waitcnt pass does not see LDS operations inside asm,
    // so nothing may sit between a read and the wait that covers it (a register copy there would copy stale bits).
    unsigned long long pr[kWords / 2];
#pragma unroll
    for (int j = 0; j < kWords / 2; j += 8)
        asm("ds_read2_b32 %0, %8 offset0:%9 offset1:%10\n\tds_read2_b32 %1, %8 offset0:%11 offset1:%12\n\t"
            "ds_read2_b32 %2, %8 offset0:%13 offset1:%14\n\tds_read2_b32 %3, %8 offset0:%15 offset1:%16\n\t"
            "ds_read2_b32 %4, %8 offset0:%17 offset1:%18\n\tds_read2_b32 %5, %8 offset0:%19 offset1:%20\n\t"
            "ds_read2_b32 %6, %8 offset0:%21 offset1:%22\n\tds_read2_b32 %7, %8 offset0:%23 offset1:%24\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(pr[j]), "=&v"(pr[j + 1]), "=&v"(pr[j + 2]), "=&v"(pr[j + 3]), "=&v"(pr[j + 4]), "=&v"(pr[j + 5]),
              "=&v"(pr[j + 6]), "=&v"(pr[j + 7]), "+v"(lds_addr)
            : "n"(2 * j), "n"(2 * j + 1), "n"(2 * j + 2), "n"(2 * j + 3), "n"(2 * j + 4), "n"(2 * j + 5), "n"(2 * j + 6),
              "n"(2 * j + 7), "n"(2 * j + 8), "n"(2 * j + 9), "n"(2 * j + 10), "n"(2 * j + 11), "n"(2 * j + 12),
              "n"(2 * j + 13), "n"(2 * j + 14), "n"(2 * j + 15));
#pragma unroll
    for (int j = 0; j < kWords / 2; j++) {
        w[2 * j] = (uint32_t)pr[j];
        w[2 * j + 1] = (uint32_t)(pr[j] >> 32);
    }
    uint32_t half[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (STAGE8) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t t = ((w[h * 8 + j] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w[h * 8 + j];
                half[h] |= (t >> (7 - j)) & (0x01010101u << j);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t t = ((w[h * 16 + j] & 0x7fff7fffu) + 0x7fff7fffu) | w[h * 16 + j];
                half[h] |= (t >> (15 - j)) & (0x00010001u << j);
            }
        }
    }
    return ((unsigned long long)half[1] << 32) | half[0];
}

template <bool STAGE8>
__device__ __forceinline__ int fetch_level(const uint32_t *blk, int p) {
    if (STAGE8) {
        const uint32_t w = blk[(p & 7) + 8 * (p >> 5)];
        return (int)(w << (24 - 8 * ((p >> 3) & 3))) >> 24;
    } else {
        const uint32_t w = blk[(p & 15) + 16 * (p >> 5)];
        return (p & 16) ? ((int)w >> 16) : ((int)(w << 16) >> 16);
    }
}

// DC part of a block (mpeg1_blk.c:73-102) with the macroblock header "11" (mpeg1_blk.c:38-51) in front
// for block 0 of a macroblock.
__device__ __forceinline__ void dc_header(int dc, bool luma, int blk, const uint32_t *vlc, uint32_t &hdr,
                                          int &hlen) {
    if (dc != 0) {
        int coe = dc < 0 ? -dc : dc;
        int low = coe & 0xff;
        int sz = low ? 32 - __builtin_clz((unsigned)low) : 1;
        uint32_t e = vlc[(luma ? kVlcDcLuma : kVlcDcChroma) + sz];
        if (dc < 0) coe ^= 1 << (sz - 1);
        hdr = ((e & 0xffffu) << sz) | ((uint32_t)coe & 0xffu & ((1u << sz) - 1u));
        hlen = (int)(e >> 16) + sz;
    } else { // "100" / "00"
        hdr = luma ? 0x4u : 0x0u;
        hlen = luma ? 3 : 2;
    }
    if (blk == 0) { // macroblock_address_increment "1" + type "1"
        hdr |= 3u << hlen;
        hlen += 2;
    }
}

// AC positions VLC_encode codes: the non-zeros below the first position whose predecessor is non-zero too
__device__ __forceinline__ unsigned long long emit_set(unsigned long long nz) {
    unsigned long long stop = nz & (nz << 1);
    unsigned long long below = stop ? ((stop & (~stop + 1)) - 1) : ~0ull;
    return nz & ~1ull & below;
}

// One lane's block bits: the first 64 in a register (the common case is the whole block), the count always.
struct BlockBits {
    unsigned long long acc;
    int tot;
    __device__ bool spilled() const { return tot > 64; }
};

// OR a block's bits into a zeroed word image at bit offset `off` (LDS image: logical big-endian words;
// global image: byte-swapped so that memory is already the byte stream).
template <bool GLOBAL, typename Walk>
__device__ __forceinline__ void put_block(uint32_t *img, uint32_t off, const BlockBits &b, Walk walk) {
    if (!b.spilled()) {
        unsigned long long A = b.acc << (64 - b.tot);
        uint32_t w = off >> 5, sh = off & 31u;
        uint32_t w0 = (uint32_t)(A >> (32 + sh));
        uint32_t w1 = (uint32_t)(A >> sh);
        uint32_t w2 = sh ? ((uint32_t)A << (32 - sh)) : 0u;
        if (GLOBAL) {
            w0 = __builtin_bswap32(w0);
            w1 = __builtin_bswap32(w1);
            w2 = __builtin_bswap32(w2);
        }
        if (w0) atomicOr(&img[w], w0);
        if (w1) atomicOr(&img[w + 1], w1);
        if (w2) atomicOr(&img[w + 2], w2);
    } else {
        uint32_t pos = off;
        auto sink = [&](uint32_t code, int bits) {
            or_code<GLOBAL>(img, pos, code, bits);
            pos += bits;
        };
        walk(sink);
    }
}

// slice header (mpeg1_blk.c:12-16): 00 00 01, strip+1 (uint8 wrap), quant_scale = 1 in 5 bits, a 0 bit: 38 bits
__device__ __forceinline__ uint32_t slice_word0(int strip) { return 0x00000100u | ((uint32_t)(strip + 1) & 0xffu); }
constexpr uint32_t kSliceWord1 = 0x08000000u;

// ---- kernel 1: one workgroup per strip (pictures with fewer than 64 blocks per strip, e.g. the
//      reference's 96x144 region: 54 blocks) ---------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(kWave) void k_encode_strips(EncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Geometry &g = a.g;
    const int T = a.threads; // == 64
    const int tid = threadIdx.x;
    uint32_t *vlc = lds;                           // kVlcWords (one wave)
    uint32_t *wave_sums = vlc + kVlcWords;         // 32
    uint32_t *stage = wave_sums + 32;              // T blocks x kStageStride16 words (int16 levels)
    uint32_t *image = stage + kStageStride16 * T;  // a.lds_words

    int frame, strip;
    frame_strip_of(blockIdx.x, a.n_frames, g.n_strips, frame, strip);
    const uint8_t *fbase = a.rgb + (unsigned long long)frame * g.frame_bytes;
    uint32_t *slot32 = reinterpret_cast<uint32_t *>(
        a.scratch + ((unsigned long long)frame * g.n_strips + strip) * g.strip_cap);

    const int blocks_per_strip = g.n_mbrows * 6;
    const bool valid = tid < blocks_per_strip;
    BlockSrc src;
    Row24 raw[8];
    if (valid) {
        src = block_source(g, strip, tid);
        if (FAST) load_block_rows(fbase, src, raw);
    }
    for (int i = tid; i < kVlcWords; i += T) vlc[i] = a.tab->vlc[i];
    for (int i = tid; i < a.lds_words; i += T) image[i] = 0;
    __syncthreads();

    unsigned long long nz = 0;
    int dc = 0;
    uint32_t *blk = stage + tid * kStageStride16;
    if (valid) {
        uint32_t lds_addr;
        dc = block_to_stage<FAST ? 1 : 0, false>(g, fbase, src, raw, frame_rq_t(a.rq_all, a.qsel, frame), blk, lds_addr);
        nz = (stage_nonzero_mask<false>(blk, lds_addr) & ~1ull) | (dc != 0 ? 1ull : 0ull);
    }
    auto fetch = [&](int p) -> int { return fetch_level<false>(blk, p); };

    uint32_t hdr = 0, bad = 0;
    int hlen = 0;
    unsigned long long emit = 0;
    BlockBits bb = {0, 0};
    if (valid) {
        dc_header(dc, src.blk < 4, src.blk, vlc, hdr, hlen);
        emit = emit_set(nz);
        block_bits_pass1<false>(hdr, hlen, dc != 0, emit, vlc, fetch, bb.acc, bb.tot, bad);
    }
    uint32_t strip_bits;
    uint32_t off = block_scan_exclusive_1b((uint32_t)bb.tot, wave_sums, 0, T, strip_bits) + 38;
    uint32_t end_bits = 38 + strip_bits;
    const bool global_mode = ((end_bits + 63) >> 5) > (uint32_t)a.lds_words; // image too large for LDS
    uint32_t *img = image;
    if (global_mode) {
        uint32_t cap_words = g.strip_cap >> 2;
        for (uint32_t i = tid; i < cap_words; i += T) slot32[i] = 0;
        __syncthreads();
        img = slot32;
    }
    if (tid == 0) {
        uint32_t h0 = slice_word0(strip), h1 = kSliceWord1;
        atomicOr(&img[0], global_mode ? __builtin_bswap32(h0) : h0);
        atomicOr(&img[1], global_mode ? __builtin_bswap32(h1) : h1);
    }
    if (valid) {
        auto walk = [&](auto &sink) { walk_codes<false>(hdr, hlen, dc != 0, emit, vlc, fetch, sink); };
        if (global_mode)
            put_block<true>(slot32, off, bb, walk);
        else
            put_block<false>(image, off, bb, walk);
    }
    __syncthreads();
    // store the strip (zero bits pad it to a byte, encoder.h:442-443)
    if (!global_mode) {
        uint32_t nwords = (end_bits + 31) >> 5;
        for (uint32_t i = tid; i < nwords; i += T) slot32[i] = __builtin_bswap32(image[i]);
    }
    if (tid == 0) {
        const unsigned long long idx = (unsigned long long)frame * g.n_strips + strip;
        a.seg[idx] = make_uint2(end_bits, (uint32_t)((idx * g.strip_cap) >> 2));
        a.strip_ctr[idx] = end_bits;
        atomicAdd(&a.frame_bytes[frame], (unsigned long long)((end_bits + 7) >> 3)); // zero bits pad the strip to a byte, encoder.h:442-443
    }
    if (bad) atomicOr(a.status, (uint32_t)M1V_STATUS_UNENCODABLE);
}

// ---- kernel 2 (the dominant one): dense runs of blocks -----------------------------------------------
// The blocks of a frame in emission order (strip-major, then macroblock, then Y0 Y1 Y2 Y3 Cb Cr) are cut
// into runs of T consecutive blocks, one workgroup (T lanes, no idle lane) per run.  T <= blocks per
// strip, so a run touches at most two strips: segment 0 (lanes < nA) continues or starts strip s0,
// segment 1 (lanes >= nA) starts strip s0+1.  Each segment is packed on its own from a word boundary of
// the workgroup's image (with the 38-bit slice header in front when it starts a strip); k_assemble
// later concatenates the segments of a strip with the necessary bit shift.
struct DenseArgs {
    Geometry g;
    const uint8_t *rgb;
    const Tables *tab;
    const float *rq_all;    // quantiser of every quality (see frame_rq_t)
    const uint32_t *qsel;   // [frame]: where the frame's quantiser lies in rq_all
    uint8_t *scratch;       // [frame][run][slot_bytes] compact slots (a run whose image fits the LDS image), then the overflow
                            // arena: arena_slots x run_cap, handed out by an atomic counter to the runs that build in global memory
    uint32_t *run_meta;     // [frame][run][4]: bits of segment 0, bits of segment 1, first word of segment 1, where the run's
                            // bytes are (offset from `scratch` in 4-byte words)
    uint32_t *arena_next;   // the counter (cleared by the assemble kernel of the batch before)
    uint32_t slot_bytes, arena_slots;
    unsigned long long arena_off; // byte offset of the arena inside scratch
    uint32_t *status;
    int n_frames;
    int threads;            // T
    int runs_per_frame;
    int lds_words;          // capacity of the LDS image of the run's bits
    int zero_iters;         // ceil(lds_words / T): rounds of T words that clear it
    uint32_t run_cap;       // bytes of one arena slot: the worst case of a run
    unsigned long long *stamps;
};

template <int FAST, bool STAGE8>
__global__ __launch_bounds__(384) __attribute__((amdgpu_waves_per_eu(M1V_WAVES_PER_EU, M1V_WAVES_PER_EU)))
void k_encode_dense(DenseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Geometry &g = a.g;
    const int T = a.threads;
    const int tid = threadIdx.x;
    constexpr int kStride = STAGE8 ? kStageStride8 : kStageStride16;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t *vlc = lds + wave * kVlcWords;        // this wave's private copy of the VLC table
    uint32_t *wave_sums = lds + (T >> 6) * kVlcWords; // 32 (16 wave totals, [16] = prefix inside the boundary wave)
    uint32_t *stage = wave_sums + 32;              // T blocks x kStride words
    uint32_t *image = stage + kStride * T;         // a.lds_words

    int frame, run;
    frame_strip_of(blockIdx.x, a.n_frames, a.runs_per_frame, frame, run);
    const uint8_t *fbase = a.rgb + (unsigned long long)frame * g.frame_bytes;
    const unsigned long long run_index = (unsigned long long)frame * a.runs_per_frame + run;
    uint32_t *slot32 = reinterpret_cast<uint32_t *>(a.scratch + run_index * a.slot_bytes); // compact slot (common case)

    STAMP_INIT();
    const int bps = g.n_mbrows * 6;                 // blocks per strip
    const int nb = g.n_strips * bps;                // blocks per frame
    const int first = run * T;                      // first block of the run
    const int s0 = first / bps;                     // strip of segment 0 (wave-uniform)
    const int pos0 = first - s0 * bps;              // position of the run's first block inside strip s0
    const int nA = min(T, bps - pos0);              // lanes of segment 0
    const int gb = first + tid;
    const bool valid = gb < nb;
    const bool in_b = tid >= nA;                    // lane belongs to segment 1 (strip s0 + 1)
    const bool has_b = first + nA < nb && nA < T;

    // ---- where this lane's block lies: before any vector load is in flight.  (With the table loads issued first, the
    //      compiler's v_mad_u64_u32 of the block arithmetic took the register of a pending table word as the unused upper
    //      half of its 64-bit addend, and every pixel load waited for that word: one full memory latency per workgroup.)
    BlockSrc src;
    using RowT = typename std::conditional<FAST == 3, Row32, typename std::conditional<FAST == 2, Row28, Row24>::type>::type;
    RowT raw[8];
    {
        // a run touches at most two strips (T <= blocks per strip), so the lane's strip needs no division; lanes past the
        // end of the frame (last run only) re-load the frame's last block
        const int strip = valid ? s0 + (in_b ? 1 : 0) : g.n_strips - 1;
        const int bidx = valid ? (in_b ? tid - nA : pos0 + tid) : bps - 1;
        src = block_source(g, strip, bidx);
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- table loads first, then every pixel load of this lane's block: the in-order vmcnt lets the
    //      tables be consumed while the pixels are still in flight ----
    uint32_t vlcv[kVlcWords / kWave];
#pragma unroll
    for (int j = 0; j < kVlcWords / kWave; j++) vlcv[j] = a.tab->vlc[lane + j * kWave];
    // keep the table loads in front of the pixel loads (the scheduler otherwise hoists the pixel loads); a scheduling
    // barrier, not a memory clobber: a clobber would turn the later scalar table loads into vector loads
    __builtin_amdgcn_sched_barrier(0);
    // Every lane loads (lanes past the end of the frame — last run only — re-load the frame's last block): outside any
    // branch the sixteen loads stay countable, so the waits for the table words below are vmcnt(16) and the rows are
    // consumed as they arrive (vmcnt(14), (12), ...) instead of after the last one.
    {
        if (FAST) load_block_rows(fbase, src, raw);
    }

    // ---- workgroup prologue, under the latency of those loads ----
#pragma unroll
    for (int j = 0; j < kVlcWords / kWave; j++) vlc[lane + j * kWave] = vlcv[j];
#pragma unroll 1
    for (int k = 0; k < a.zero_iters; k++) image[k * T + tid] = 0; // the allocation is rounded up to a multiple of T words
    STAMP(0);

    unsigned long long nz = 0;
    int dc = 0;
    uint32_t *blk = stage + tid * kStride;
    if (valid) {
        uint32_t lds_addr;
        dc = block_to_stage<FAST, STAGE8, RowT>(g, fbase, src, raw, frame_rq_t(a.rq_all, a.qsel, frame), blk, lds_addr);
        nz = (stage_nonzero_mask<STAGE8>(blk, lds_addr) & ~1ull) | (dc != 0 ? 1ull : 0ull);
    }
    // No barrier here: pass 1 below reads only the lane's own staged levels and the wave's own copy of the VLC table.
    // The image zeroed in the prologue is first touched in pass 2, behind the barrier of the scan.
    STAMP(2);
    auto fetch = [&](int p) -> int { return fetch_level<STAGE8>(blk, p); };

    uint32_t hdr = 0, bad = 0;
    int hlen = 0;
    unsigned long long emit = 0;
    BlockBits bb = {0, 0};
    if (valid) {
        dc_header(dc, src.blk < 4, src.blk, vlc, hdr, hlen);
        emit = emit_set(nz);
        block_bits_pass1<STAGE8>(hdr, hlen, dc != 0, emit, vlc, fetch, bb.acc, bb.tot, bad);
    }
    STAMP(4);

    // ---- exclusive scan of the bit counts; PA = bits of segment 0's blocks ----
    uint32_t incl = wave_scan_inclusive((uint32_t)bb.tot);
    if (lane == kWave - 1) wave_sums[wave] = incl;
    if (tid == nA - 1) wave_sums[16] = incl;       // prefix inside the wave that holds segment 0's last lane
    __syncthreads();
    const int nw = T >> 6;
    uint32_t wsum = lane < nw ? wave_sums[lane] : 0;
    uint32_t wincl = row_scan_inclusive(wsum);
    uint32_t wave_off = (uint32_t)__builtin_amdgcn_readlane((int)(wincl - wsum), wave);
    uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)wincl, nw - 1);
    const int wA = __builtin_amdgcn_readfirstlane((nA - 1) >> 6);
    uint32_t PA = (uint32_t)__builtin_amdgcn_readlane((int)(wincl - wsum), wA) + wave_sums[16];
    uint32_t P = wave_off + incl - (uint32_t)bb.tot;
    STAMP(5);

    const uint32_t origin0 = pos0 == 0 ? 38u : 0u;          // segment 0 starts its strip
    const uint32_t bits0 = origin0 + PA;
    const uint32_t base1 = ((bits0 + 31) >> 5) + 1;         // first image word of segment 1
    const uint32_t bits1 = has_b ? 38u + (total - PA) : 0u;
    const uint32_t end_words = has_b ? base1 + ((bits1 + 31) >> 5) : ((bits0 + 31) >> 5);
    const uint32_t off = in_b ? base1 * 32u + 38u + (P - PA) : origin0 + P;

    auto slice_headers = [&](uint32_t *img, bool swapped) {
        if (pos0 == 0) {
            uint32_t h0 = slice_word0(s0), h1 = kSliceWord1;
            atomicOr(&img[0], swapped ? __builtin_bswap32(h0) : h0);
            atomicOr(&img[1], swapped ? __builtin_bswap32(h1) : h1);
        }
        if (has_b) {
            uint32_t h0 = slice_word0(s0 + 1), h1 = kSliceWord1;
            atomicOr(&img[base1], swapped ? __builtin_bswap32(h0) : h0);
            atomicOr(&img[base1 + 1], swapped ? __builtin_bswap32(h1) : h1);
        }
    };
    auto walk = [&](auto &sink) { walk_codes<STAGE8>(hdr, hlen, dc != 0, emit, vlc, fetch, sink); };
    uint32_t *meta = a.run_meta + run_index * 4;

    // ---- image too large for LDS (rare): build it with global atomics in a zeroed, worst-case sized slot taken from
    //      the overflow arena.  A branch of its own that ends the kernel, so that the common path below keeps its
    //      uniform slot pointer (merging the two pointers into one variable measured 3 % slower on the common path).
    if (end_words + 2 > (uint32_t)a.lds_words) {
        if (tid == 0) wave_sums[17] = atomicAdd(a.arena_next, 1u);
        __syncthreads();
        const uint32_t got = wave_sums[17];
        if (got >= a.arena_slots) { // arena exhausted: the caller re-encodes after m1v_reserve_scratch (M1V_E_SCRATCH)
            if (tid == 0) {
                atomicOr(a.status, (uint32_t)M1V_STATUS_SCRATCH);
                meta[0] = meta[1] = 0;
                meta[2] = meta[3] = 0;
            }
            return;
        }
        const unsigned long long where = a.arena_off + (unsigned long long)got * a.run_cap;
        uint32_t *big = reinterpret_cast<uint32_t *>(a.scratch + where);
        for (uint32_t i = tid; i < (a.run_cap >> 2); i += T) big[i] = 0;
        __syncthreads();
        if (tid == 0) {
            slice_headers(big, true);
            meta[0] = bits0;
            meta[1] = bits1;
            meta[2] = base1;
            meta[3] = (uint32_t)(where >> 2);
        }
        if (valid) put_block<true>(big, off, bb, walk);
        if (bad) atomicOr(a.status, (uint32_t)M1V_STATUS_UNENCODABLE);
        return;
    }

    // ---- common path: OR the bits into the LDS image, store it once to the run's compact slot ----
    if (tid == 0) {
        slice_headers(image, false);
        meta[0] = bits0;
        meta[1] = bits1;
        meta[2] = base1;
        meta[3] = (uint32_t)((run_index * a.slot_bytes) >> 2);
    }
    if (valid) put_block<false>(image, off, bb, walk);
    STAMP(6);
    __syncthreads();
    STAMP(7);
    for (uint32_t i = tid; i < end_words; i += T) slot32[i] = __builtin_bswap32(image[i]);
    if (bad) atomicOr(a.status, (uint32_t)M1V_STATUS_UNENCODABLE);
    STAMP(8);
}

// ------------------------------------------------------------------------------------------------
// layout + gather
// ------------------------------------------------------------------------------------------------
// PKT SEQ GOP PIC in front of a frame's strips with the 16-bit length back-patched (encoder.h:198-230, :448-453:
// (u16)(bytes after the length field's word) - 4) and the four trailing bytes (encoder.h:456-458, observed zero);
// threads 0..47 of the workgroup that assembles the frame's first strips
__device__ __forceinline__ void frame_header_and_trailer(const Tables *tab, uint8_t *out, unsigned long long fo,
                                                         unsigned long long fs, int index, int t) {
    if (t < 44) {
        uint8_t v = tab->hdr[index & 255][t];
        const uint32_t fwd = (uint32_t)((fs - 4ull) - 4ull - 4ull) & 0xffffu;
        if (t == 4) v = (uint8_t)(fwd >> 8);
        if (t == 5) v = (uint8_t)(fwd & 0xff);
        out[fo + t] = v;
    } else if (t < 48) {
        out[fo + fs - 4 + (t - 44)] = 0;
    }
}

#include "m1v_assemble.h"

// ---- run kernels: strips are concatenations of run segments ----------------------------------------
struct DenseGeom {
    int n_frames, n_strips, bps, T, runs_per_frame;
};

// Segment of strip s contributed by run w: which of the run's two segments, its bit count, its bytes.
__device__ __forceinline__ uint32_t dense_segment(const DenseGeom &d, const uint32_t *meta_frame, int w, int s,
                                                  uint32_t &word_off) {
    int s0w = (w * d.T) / d.bps;
    const uint32_t *m = meta_frame + (size_t)w * 4;
    if (s0w == s) {
        word_off = m[3];
        return m[0];
    }
    word_off = m[3] + m[2];
    return m[1];
}

// One workgroup per frame: the run segments of every strip, in the form k_assemble takes them: seg[frame][q][strip] =
// (bits, where), padded with empty segments up to `segs` per strip; the strips' bit totals; the frame's bytes.
__global__ __launch_bounds__(256) void k_dense_frame_layout(DenseGeom d, int segs, const uint32_t *run_meta, uint2 *seg,
                                                            unsigned long long *strip_ctr, unsigned long long *frame_bytes) {
    __shared__ unsigned long long wsum[4];
    const int f = blockIdx.x;
    const uint32_t *mf = run_meta + (size_t)f * d.runs_per_frame * 4;
    unsigned long long bytes = 0;
    for (int s = threadIdx.x; s < d.n_strips; s += 256) {
        const size_t i = (size_t)f * d.n_strips + s;
        const int w_lo = (s * d.bps) / d.T, w_hi = ((s + 1) * d.bps - 1) / d.T; // w_hi - w_lo + 1 <= segs
        uint32_t bits = 0;
        for (int q = 0; q < segs; q++) {
            uint32_t boff = 0, L = 0;
            if (w_lo + q <= w_hi) L = dense_segment(d, mf, w_lo + q, s, boff);
            seg[((size_t)f * segs + q) * d.n_strips + s] = make_uint2(L, boff);
            bits += L;
        }
        strip_ctr[i] = bits;
        bytes += (bits + 7) >> 3; // zero bits pad the strip to a byte, encoder.h:442-443
    }
    bytes = wave_sum_u64(bytes);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = bytes;
    __syncthreads();
    if (threadIdx.x == 0) frame_bytes[f] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

constexpr int kMaxCandidates = 8; // qualities of one budget call or size table

#include "m1v_tiles.h"
#include "m1v_planes.h"
#include "m1v_step2.h"
#include "m1v_rgb_planes.h"
#include "m1v_float_planes.h"
#include "m1v_float_pixels.h"
#include "m1v_downscale.h"
#include "m1v_downscale_planes.h"
#include "m1v_downscale_words.h"

// ---- per-frame quality and frame-size budgets (m1v_encode_quality_device, m1v_frame_sizes_device, m1v_encode_budget_device) ----
struct QualityArgs {
    const uint8_t *quality;                  // [frame] the caller's qualities, or null
    int uniform;                             // the quality of every frame when `quality` and `probe_sizes` are null
    int max_q;                               // the encoder's quality factor (1..100): the largest valid entry
    // budget: probe_sizes[k * stride + frame] = record bytes of the frame at cand[k] (strictly increasing)
    const unsigned long long *probe_sizes;
    int stride, n_cand;
    uint8_t cand[kMaxCandidates];
    const unsigned long long *budget;        // [frame] per-frame budgets, or null: max_bytes for every frame
    unsigned long long max_bytes;
    const uint32_t *probe_status;            // [n_cand] status words of the probes
    const uint32_t *pick_status;             // [1] k_rate_pick's status word (batch budget, bitrate), or null
    int n_frames;
    uint32_t *qsel;                          // out: [frame] offset of the frame's entry in rq_all
    uint8_t *chosen;                         // out (budget, may be null): [frame] the quality picked
    uint32_t *status;                        // the batch's status word (M1V_STATUS_QUALITY, M1V_STATUS_OVER_BUDGET, ...)
};

// One lane per frame: the frame's quality -> its offset in rq_all.  An entry outside 1..max_q sets M1V_STATUS_QUALITY and
// encodes at max_q (every plan of the encoder holds there; the batch's output is undefined, as with the other status bits).
// Budget form: the largest candidate whose probed record fits the frame's budget, else the smallest and
// M1V_STATUS_OVER_BUDGET; a probe that ran out of overflow scratch (sizes undefined) passes M1V_STATUS_SCRATCH on.  After
// k_rate_pick (the caller's qualities are its picks) its status word's M1V_STATUS_OVER_BUDGET and M1V_STATUS_SCRATCH pass on.
__global__ __launch_bounds__(256) void k_frame_quality(QualityArgs a) {
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    uint32_t bits = 0;
    if (f == 0 && a.probe_sizes)
        for (int k = 0; k < a.n_cand; k++) bits |= a.probe_status[k] & (uint32_t)M1V_STATUS_SCRATCH;
    if (f == 0 && a.pick_status) bits |= *a.pick_status & (uint32_t)(M1V_STATUS_OVER_BUDGET | M1V_STATUS_SCRATCH);
    if (f < a.n_frames) {
        int q;
        if (a.probe_sizes) {
            const unsigned long long cap = a.budget ? a.budget[f] : a.max_bytes;
            int pick = -1;
            for (int k = 0; k < a.n_cand; k++)
                if (a.probe_sizes[(size_t)k * a.stride + f] <= cap) pick = k;
            if (pick < 0) bits |= (uint32_t)M1V_STATUS_OVER_BUDGET;
            q = a.cand[pick < 0 ? 0 : pick];
            if (a.chosen) a.chosen[f] = (uint8_t)q;
        } else {
            q = a.quality ? (int)a.quality[f] : a.uniform;
        }
        if (q < 1 || q > a.max_q) {
            bits |= (uint32_t)M1V_STATUS_QUALITY;
            q = a.max_q;
        }
        a.qsel[f] = (uint32_t)(q - 1) * 64u;
    }
    if (bits) atomicOr(a.status, bits);
}

// ---- rate-distortion picks (m1v_encode_rd_device) ------------------------------------------------------------------------------
// k_rd_pick stands where k_frame_quality stands in a budget call: one lane per frame, between the rd table and the encode.  From
// sizes / dist[k * stride + frame] it picks a candidate per frame by one of two rules (include/mpeg1_hip.h), writes the frame's
// offset in rq_all, its quality (chosen, may be null) and the picked candidate's distortion (frame_dist, may be null), and ORs
// M1V_STATUS_OVER_BUDGET / M1V_STATUS_OVER_DISTORTION into the batch's status word.  A candidate whose table status carries
// M1V_STATUS_UNENCODABLE (its rows are undefined) is out of the running for every frame; with every candidate out the frames go
// to candidate 0, whose encode reports the bit itself.
struct RdPickArgs {
    const unsigned long long *sizes, *dist;  // [k * stride + frame]
    int stride, n_cand, n_frames;
    uint8_t cand[kMaxCandidates];
    int rule;                                // M1V_RD_BEST_IN_BUDGET, M1V_RD_SMALLEST_AT_DISTORTION
    const unsigned long long *limits;        // [frame] per-frame limits, or null: `limit` for every frame
    unsigned long long limit;
    const uint32_t *table_status;            // [n_cand] status words of the rd table
    uint32_t *qsel;                          // out: [frame] offset of the frame's entry in rq_all
    uint8_t *chosen;                         // out (may be null): [frame] the quality picked
    unsigned long long *frame_dist;          // out (may be null): [frame] the distortion at the pick
    uint32_t *status;                        // the batch's status word
};

__global__ __launch_bounds__(256) void k_rd_pick(RdPickArgs a) {
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    if (f >= a.n_frames) return;
    const bool by_bytes = a.rule == M1V_RD_BEST_IN_BUDGET;
    const unsigned long long lim = a.limits ? a.limits[f] : a.limit;
    // bound = what the limit bounds (bytes | distortion), other = what is minimised under it (distortion | bytes)
    int pick = -1, least = -1;
    unsigned long long pick_bound = 0, pick_other = 0, least_bound = 0, least_other = 0;
    for (int k = 0; k < a.n_cand; k++) {
        if (a.table_status[k] & (uint32_t)M1V_STATUS_UNENCODABLE) continue;
        const unsigned long long s = a.sizes[(size_t)k * a.stride + f], d = a.dist[(size_t)k * a.stride + f];
        const unsigned long long bound = by_bytes ? s : d, other = by_bytes ? d : s;
        // within the limit: the least `other`, ties by the smaller `bound`, then the smaller k
        if (bound <= lim && (pick < 0 || other < pick_other || (other == pick_other && bound < pick_bound))) {
            pick = k;
            pick_bound = bound;
            pick_other = other;
        }
        // nothing within it: the least `bound`; ties by the smaller record (the distortion rule only), then the smaller k
        if (least < 0 || bound < least_bound || (!by_bytes && bound == least_bound && other < least_other)) {
            least = k;
            least_bound = bound;
            least_other = other;
        }
    }
    uint32_t bits = 0;
    if (pick < 0 && least >= 0) bits = by_bytes ? (uint32_t)M1V_STATUS_OVER_BUDGET : (uint32_t)M1V_STATUS_OVER_DISTORTION;
    const int k = pick >= 0 ? pick : (least >= 0 ? least : 0);
    a.qsel[f] = (uint32_t)(a.cand[k] - 1) * 64u;
    if (a.chosen) a.chosen[f] = a.cand[k];
    if (a.frame_dist) a.frame_dist[f] = a.dist[(size_t)k * a.stride + f];
    if (bits) atomicOr(a.status, bits);
}

// ---- batch byte budgets and constant bitrate (m1v_encode_batch_budget_device, m1v_encode_cbr_device) ---------------------
// k_rate_pick: ONE workgroup between the size table and the encode, on the caller's stream.  It picks a candidate per frame
// from the table (sizes[k * stride + frame], k < n_cand, candidates' qualities strictly increasing) by one of two rules
// (include/mpeg1_hip.h), writes the candidate's quality to chosen[frame] (the encode's per-frame qualities) and writes its status
// word: M1V_STATUS_OVER_BUDGET, and the table's M1V_STATUS_SCRATCH (k_frame_quality passes both on to the batch's status
// word).  Written, not OR'ed: nothing needs clearing between calls.  Integer arithmetic, no scratch, no atomics.
constexpr int kPickThreads = 1024;
constexpr int kPickWaves = kPickThreads / kWave;
constexpr int kCbrChunk = 512; // frames of the table staged in LDS per step of the bitrate walk

struct PickArgs {
    const unsigned long long *sizes; // [k * stride + frame] record bytes at candidate k
    int stride, n_cand, n_frames;
    unsigned long long cand;         // byte k: the quality of candidate k
    const uint32_t *table_status;    // [n_cand] status words of the size table
    unsigned long long budget;       // batch form: bytes for the sum of the batch's records
    long long rate, capacity;        // bitrate form: refill per frame (>= 1), buffer capacity (rate .. 2^62 - 1)
    const long long *level_in;       // bitrate form: bytes available to the first frame (may be level_out)
    long long *level_out;            //   and to the frame after the batch
    uint8_t *chosen;                 // out: [frame] the quality picked
    uint32_t *status;                // out: [1]
};

__device__ __forceinline__ uint8_t cand_quality(unsigned long long cand, int k) { return (uint8_t)(cand >> (8 * k)); }
__device__ __forceinline__ long long readlane_i64(long long v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// Batch form (kCbr = false).  T[k] = sum of row k; top = the largest k with T[k] <= budget (none: every frame at candidate 0 and
// M1V_STATUS_OVER_BUDGET; top = n_cand - 1: every frame there).  Otherwise every frame goes to top or top + 1.  With
// d[f] = s[top + 1][f] - s[top][f], the upgrades with d <= 0 are free and always taken; the others go cheapest first, (d, f)
// ascending, while they fit: frame f is upgraded iff the positive d up to and including its own in that order sum to at most
// room = budget - T[top] + (the bytes the free upgrades save).  Each frame's prefix sum is one pass over every frame's key
// (d << 32 | frame), staged in LDS a block at a time: n^2 / kPickThreads compare-and-adds per lane.  A record is shorter than
// 4 GiB (m1v_create bounds a frame's input below 4 GiB; a record holds at most 2.6 bytes per pixel), so d < 2^32 and the keys
// order as (d, f) do.
// Bitrate form (kCbr = true).  level = min(*level_in, capacity); per frame in order: the largest candidate whose record fits
// level, else candidate 0 and M1V_STATUS_OVER_BUDGET; level = min(capacity, level - record + rate) (negative: a debt the later
// refills repay; it stays above -2^63 while the stream owes less than 2^62 bytes).  *level_out = level.  The walk is wave 0's:
// a chunk of the table is staged in LDS, [frame][candidate], and lane 8j + k holds candidate k of frame j of a step of eight,
// so that the chain from one frame to the next is a compare, a ballot, a readlane and the level update.
template <bool kCbr>
__global__ __launch_bounds__(kPickThreads) void k_rate_pick(PickArgs a) {
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    const int n = a.n_frames, K = a.n_cand;
    uint32_t bits = 0;
    if (n > 0)
        for (int k = 0; k < K; k++) bits |= a.table_status[k] & (uint32_t)M1V_STATUS_SCRATCH;
    if constexpr (kCbr) {
        __shared__ long long stage[kCbrChunk * kMaxCandidates];
        __shared__ uint8_t picks[kCbrChunk];
        long long level = *a.level_in; // (every read of level_in comes before the write of level_out)
        level = level < a.capacity ? level : a.capacity;
        bool over = false;
        for (int f0 = 0; f0 < n; f0 += kCbrChunk) {
            const int cnt = min(kCbrChunk, n - f0);
            for (int i = t; i < kCbrChunk * kMaxCandidates; i += kPickThreads) {
                const int k = i / kCbrChunk, j = i % kCbrChunk; // (coalesced reads along a row)
                stage[j * kMaxCandidates + k] = k < K && j < cnt ? (long long)a.sizes[(size_t)k * a.stride + f0 + j] : 0x7fffffffffffffffll;
            }
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane(wave) == 0) {
                for (int j0 = 0; j0 < cnt; j0 += 8) {
                    const long long s = stage[j0 * kMaxCandidates + lane];
                    int mine = 0;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (j0 + j < cnt) {
                            const uint32_t fit = (uint32_t)(__ballot(s <= level) >> (8 * j)) & 0xffu;
                            const int k = fit ? 31 - __clz((int)fit) : 0;
                            over |= fit == 0;
                            level -= readlane_i64(s, 8 * j + k);
                            level += a.rate;
                            level = level < a.capacity ? level : a.capacity;
                            if ((lane >> 3) == j) mine = k;
                        }
                    }
                    if ((lane & 7) == 0 && j0 + (lane >> 3) < cnt) picks[j0 + (lane >> 3)] = (uint8_t)mine;
                }
            }
            __syncthreads();
            for (int j = t; j < cnt; j += kPickThreads) a.chosen[f0 + j] = cand_quality(a.cand, picks[j]);
        }
        if (t == 0) { // (lane 0 of wave 0: it walked)
            *a.level_out = level;
            *a.status = bits | (over ? (uint32_t)M1V_STATUS_OVER_BUDGET : 0u);
        }
    } else {
        __shared__ unsigned long long part[kPickWaves][2 * kMaxCandidates]; // per wave: T[k], then the savings of k -> k + 1
        __shared__ unsigned long long tot[2 * kMaxCandidates];
        __shared__ unsigned long long keys[kPickThreads];
        unsigned long long sum[kMaxCandidates], save[kMaxCandidates];
#pragma unroll
        for (int k = 0; k < kMaxCandidates; k++) sum[k] = save[k] = 0;
        for (int f = t; f < n; f += kPickThreads) {
            unsigned long long prev = 0;
#pragma unroll
            for (int k = 0; k < kMaxCandidates; k++)
                if (k < K) {
                    const unsigned long long s = a.sizes[(size_t)k * a.stride + f];
                    sum[k] += s;
                    if (k > 0 && s < prev) save[k - 1] += prev - s;
                    prev = s;
                }
        }
#pragma unroll
        for (int k = 0; k < kMaxCandidates; k++) {
            const unsigned long long s = wave_sum_u64(sum[k]), v = wave_sum_u64(save[k]);
            if (lane == 0) {
                part[wave][k] = s;
                part[wave][kMaxCandidates + k] = v;
            }
        }
        __syncthreads();
        if (t < 2 * kMaxCandidates) {
            unsigned long long s = 0;
            for (int w = 0; w < kPickWaves; w++) s += part[w][t];
            tot[t] = s;
        }
        __syncthreads();
        int top = -1;
        for (int k = 0; k < K; k++)
            if (tot[k] <= a.budget) top = k;
        if (top < 0 || top == K - 1) {
            const uint8_t q = cand_quality(a.cand, top < 0 ? 0 : top);
            for (int f = t; f < n; f += kPickThreads) a.chosen[f] = q;
        } else {
            const unsigned long long room = a.budget - tot[top] + tot[kMaxCandidates + top];
            const unsigned long long *lo = a.sizes + (size_t)top * a.stride, *hi = lo + a.stride;
            for (int f0 = 0; f0 < n; f0 += kPickThreads) {
                const int f = f0 + t;
                const long long d = f < n ? (long long)(hi[f] - lo[f]) : 0;
                const unsigned long long own = ((unsigned long long)(d > 0xffffffffll ? 0xffffffffll : (d > 0 ? d : 0)) << 32) | (uint32_t)f;
                unsigned long long acc = 0; // the positive d whose keys are <= own
                for (int c0 = 0; c0 < n; c0 += kPickThreads) {
                    const int cnt = min(kPickThreads, n - c0), steps = (cnt + 7) & ~7;
                    __syncthreads(); // (the previous block's keys are read)
                    if (t < cnt) {
                        const long long dj = (long long)(hi[c0 + t] - lo[c0 + t]);
                        keys[t] = ((unsigned long long)(dj > 0xffffffffll ? 0xffffffffll : (dj > 0 ? dj : 0)) << 32) | (uint32_t)(c0 + t);
                    } else if (t < steps) {
                        keys[t] = 0; // adds nothing
                    }
                    __syncthreads();
                    if (f < n && d > 0 && acc <= room) {
                        for (int j = 0; j < steps; j += 8) {
#pragma unroll
                            for (int u = 0; u < 8; u++) {
                                const unsigned long long kj = keys[j + u];
                                acc += kj <= own ? (kj >> 32) : 0ull;
                            }
                        }
                    }
                }
                if (f < n) a.chosen[f] = cand_quality(a.cand, d <= 0 || acc <= room ? top + 1 : top);
            }
        }
        if (t == 0) *a.status = bits | (top < 0 ? (uint32_t)M1V_STATUS_OVER_BUDGET : 0u);
    }
}

#include "m1v_rd_rate.h"
#include "m1v_streams.h"
#include "m1v_span_budget.h"

// The probe's place of k_assemble (one workgroup per frame): each record's size (its strips' bytes + 48 bytes of headers and
// trailer, what k_assemble derives) and the status word, and the same counter hand-over — the set the next call adds into is
// cleared for the frames this launch reaches (the host clears the rest).  Nothing is assembled, nothing written to d_out.
struct SizesArgs {
    int n_frames, n_strips, next_frames;
    const unsigned long long *frame_bytes;
    const uint32_t *enc_words;
    unsigned long long *next_strip_ctr, *next_frame_bytes;
    uint32_t *next_words;
    unsigned long long *out_sizes; // may be null
    uint32_t *out_status;
};
__global__ __launch_bounds__(256) void k_frame_sizes(SizesArgs a) {
    const int f = blockIdx.x;
    if (f < a.next_frames)
        for (int s = threadIdx.x; s < a.n_strips; s += 256) a.next_strip_ctr[(size_t)f * a.n_strips + s] = 0ull;
    if (threadIdx.x == 0) {
        if (a.out_sizes) a.out_sizes[f] = 48ull + a.frame_bytes[f];
        if (f < a.next_frames) a.next_frame_bytes[f] = 0ull;
        if (f == a.n_frames - 1) {
            *a.out_status = a.enc_words[0];
            a.next_words[0] = 0u;
            a.next_words[2] = 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// partial pipelines
// ------------------------------------------------------------------------------------------------
struct CoefArgs {
    Geometry g;
    const uint8_t *rgb;
    const Tables *tab;
    int16_t *out;
    int n_frames;
};

template <bool FAST>
__global__ __launch_bounds__(256) void k_coefficients(CoefArgs a) {
    const Geometry &g = a.g;
    int blocks_per_strip = g.n_mbrows * 6;
    int bidx = blockIdx.x * 256 + threadIdx.x;
    int strip = blockIdx.y, frame = blockIdx.z;
    if (bidx >= blocks_per_strip) return;
    BlockSrc s = block_source(g, strip, bidx);
    int q[64];
    block_coefficients<FAST>(g, a.rgb + (unsigned long long)frame * g.frame_bytes, s, a.tab->rq, q);
    int16_t *o = a.out + (((size_t)frame * g.n_strips + strip) * blocks_per_strip + bidx) * 64;
    uint32_t *o32 = reinterpret_cast<uint32_t *>(o);
#pragma unroll
    for (int m = 0; m < 32; m++)
        o32[m] = ((uint32_t)q[scan_inv(2 * m)] & 0xffffu) | ((uint32_t)q[scan_inv(2 * m + 1)] << 16);
}

__global__ __launch_bounds__(256) void k_convert(const uint8_t *rgb, int C, unsigned long long npx_frame,
                                                 int n_frames, uint8_t *planes) {
    unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long total = npx_frame * (unsigned long long)n_frames;
    for (; i < total; i += (unsigned long long)gridDim.x * 256) {
        unsigned long long f = i / npx_frame, p = i - f * npx_frame;
        const uint8_t *q = rgb + i * C;
        uint32_t r = q[0], gg = q[1], b = q[2];
        uint8_t *o = planes + f * 3 * npx_frame;
        o[p] = (uint8_t)(int)(component_raw(r, gg, b, comp_coef_f(0)) - m1vf::kPxBiasF);
        o[npx_frame + p] = (uint8_t)(int)(component_raw(r, gg, b, comp_coef_f(1)) - m1vf::kPxBiasF);
        o[2 * npx_frame + p] = (uint8_t)(int)(component_raw(r, gg, b, comp_coef_f(2)) - m1vf::kPxBiasF);
    }
}

// The same planes, four pixels per lane (frames whose pixel count is a multiple of 4, 4-byte aligned buffers): the 12 or
// 16 input bytes arrive as dwords, every byte is converted once and feeds all three components, ONE fraction test covers the
// group's twelve sums (the fp64 re-evaluation runs only behind it), and each plane gets one packed dword store.
// HBM-bound: 3 or 4 bytes in, 3 bytes out per pixel.
template <int C>
__global__ __launch_bounds__(256) void k_convert4(const uint32_t *rgb, unsigned long long groups_frame, int n_frames,
                                                  uint32_t *planes) {
    const CompCoefF ky = comp_coef_f(0), kcb = comp_coef_f(1), kcr = comp_coef_f(2); // uniform: scalar registers
    const unsigned long long total = groups_frame * (unsigned long long)n_frames;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long f = i / groups_frame, gidx = i - f * groups_frame;
        uint32_t w[C];
#pragma unroll
        for (int k = 0; k < C; k++) w[k] = rgb[i * C + k];
        float lowest = 1.0f, t[3][4], p[3][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            auto chan = [&](int ch) -> uint32_t {
                int byte = C * j + ch;
                return (w[byte >> 2] >> ((byte & 3) * 8)) & 0xffu;
            };
            const float r = (float)chan(0), g = (float)chan(1), b = (float)chan(2);
            t[0][j] = fmaf(r, ky.kr, fmaf(g, ky.kg, fmaf(b, ky.kb, ky.k0)));
            t[1][j] = fmaf(r, kcb.kr, fmaf(g, kcb.kg, fmaf(b, kcb.kb, kcb.k0)));
            t[2][j] = fmaf(r, kcr.kr, fmaf(g, kcr.kg, fmaf(b, kcr.kb, kcr.k0)));
#pragma unroll
            for (int c = 0; c < 3; c++) {
                p[c][j] = clear_fraction(t[c][j]);
                lowest = fminf(lowest, t[c][j] - p[c][j]);
            }
        }
        if (lowest < kFracLow) { // rare: some sum of the group is a tie (or next to one) of the reference's formulas
#pragma unroll
            for (int j = 0; j < 4; j++) {
                auto chan = [&](int ch) -> int {
                    int byte = C * j + ch;
                    return (int)((w[byte >> 2] >> ((byte & 3) * 8)) & 0xffu);
                };
#pragma unroll
                for (int c = 0; c < 3; c++)
                    if (t[c][j] - p[c][j] < kFracLow) {
                        const CompCoef d = comp_coef(c);
                        p[c][j] = m1vf::kPxBiasF + (float)component_fp64(chan(0), chan(1), chan(2), d.k0, d.kr, d.kg, d.kb);
                    }
            }
        }
        // p = 256 + value: the value is the top 8 mantissa bits
        const unsigned long long plane_words = groups_frame;
        uint32_t *o = planes + f * 3 * plane_words + gidx;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) packed |= ((__float_as_uint(p[c][j]) >> 15) & 0xffu) << (8 * j);
            o[c * plane_words] = packed;
        }
    }
}

__global__ __launch_bounds__(256) void k_subsample(const uint8_t *cb, const uint8_t *cr, int W, int H,
                                                   uint8_t *cbs, uint8_t *crs) {
    int sw = W / 2, sh = H / 2;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= sw * sh) return;
    int y = (i / sw) * 2, x = (i % sw) * 2;
    size_t a = (size_t)y * W + x, c = (size_t)(y + 1) * W + x;
    cbs[i] = (uint8_t)((cb[a] + cb[a + 1] + cb[c] + cb[c + 1]) / 4);
    crs[i] = (uint8_t)((cr[a] + cr[a + 1] + cr[c] + cr[c + 1]) / 4);
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_synth(uint8_t *rgb, unsigned long long bytes_per_frame,
                                               int n_frames, unsigned long long seed,
                                               unsigned long long first_index) {
    unsigned long long words = (bytes_per_frame + 7) >> 3;
    unsigned long long total = words * (unsigned long long)n_frames;
    unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    for (; i < total; i += (unsigned long long)gridDim.x * 256) {
        unsigned long long f = i / words, j = i - f * words;
        unsigned long long v = splitmix64(seed + (first_index + f) * 0x9E3779B97F4A7C15ull + j);
        uint8_t *dst = rgb + f * bytes_per_frame + 8 * j;
        unsigned long long left = bytes_per_frame - 8 * j;
        if (left >= 8 && ((uintptr_t)dst & 7) == 0) {
            *reinterpret_cast<unsigned long long *>(dst) = v;
        } else {
            for (unsigned k = 0; k < 8 && k < left; k++) dst[k] = (uint8_t)(v >> (8 * k));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan of an encoder and the launches of a batch from it (the C-ABI itself: m1v_runtime.h)
// ------------------------------------------------------------------------------------------------
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, const char *detail = "", const char *detail2 = "") {
    snprintf(g_err, sizeof g_err, fmt, detail, detail2);
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(M1V_E_HIP, #expr ": %s", hipGetErrorString(e_));         \
    } while (0)

} // namespace

#ifndef M1V_TILE_RING
#define M1V_TILE_RING 2
#endif

// Which encode kernel serves a batch.  Tiles (k_encode_tiles, m1v_tiles.h): 3-channel pictures, any width and alignment — the
// default; with a surface layout (m1v_set_input_layout) k_encode_surface in their place, for 3 and 4 channels.  Runs: k_encode_dense (4-channel pictures, and whatever the test hooks force: m1v_debug_set_path, a forced input mode, a
// forced run length), or k_encode_strips where a strip has fewer than 64 blocks.
enum class Producer { tiles, dense, strips };

// What the encoder's settings decide (plan_for): the producer kernel, its launch shape, the layout of its scratch, k_assemble's shape.
struct Plan {
    Producer producer;
    int block;              // workgroup size of the producer (dense: the run length T)
    size_t lds_bytes;       // its dynamic LDS
    int units;              // its workgroups per frame: tiles, runs or strips
    int image_words;        // LDS image of a unit's bits
    int zero_iters;         // dense: passes of the run's lanes over that image to clear it
    int tile_cols, tile_rows;
    uint32_t luma_region, chroma_region; // tiles: LDS bytes of a wave's ring / staging region
    uint32_t run_cap;       // worst-case bytes of one unit = one slot of the overflow arena
    uint32_t slot_bytes;    // compact slot of a unit (what the LDS image can hold)
    uint32_t arena_slots;
    size_t arena_off;
    size_t scratch_bytes, meta_bytes, seg_bytes; // per batch state (meta: run metadata, dense only)
    int segs;               // segments per strip: tile rows (tiles), or the most runs a strip can touch (run kernels)
    int asm_group, asm_lanes_log2; // k_assemble: strips per workgroup, lanes per segment
    // The fused size table (k_size_table_tiles; k_size_table_rgba for 4-channel encoders, whatever their producer is): its
    // own tile grid (tile_cols x tile_rows above), set when table_units != 0
    int table_units;        // its workgroups per frame, 0 = no fused table: one probe per quality
    uint32_t table_region;  // its LDS bytes of a wave's ring / staging region
    size_t table_lds_bytes; // and its dynamic LDS
};

struct m1v_encoder {
    int device = 0;
    Geometry g = {};
    int qf = 0, mode = 0, max_frames = 0;
    int batch_limit = 0;    // what bounds a call's frames beside max_frames: the device's smaller grid extent in y and z (m1v_create)
    bool dense = false;     // blocks per strip >= 64: k_encode_dense, else one workgroup per strip
    bool narrow = false;    // no AC level can reach +-128: one byte per staged level
    bool fast_ok = false;   // geometry allows the 4-byte-aligned 24-byte row loads
    // settings that plan_for reads (m1v_reserve_scratch, m1v_set_pipelined and the m1v_debug_set_* hooks change them)
    int lds_words = 0;          // forced LDS image, 0 = default of the kernel in use
    bool reserve_worst = false; // overflow arena sized for every run (m1v_reserve_scratch, or a forced tiny LDS image)
    int forced_mode = -1;       // m1v_debug_set_input_mode: -1 = pick by geometry and alignment
    int forced_path = -1;       // m1v_debug_set_path: -1 = by geometry, 0 = runs, 1 = tiles
    int forced_T = 0;           // run length forced by m1v_debug_set_dense_threads (0 = default)
    bool pipelined = false;     // layout + gather of batch k on `side` while batch k+1 encodes on the caller's stream
    // m1v_debug_set_assemble_shape: k_assemble's strips per workgroup and lanes per segment, 0 = the plan's own (one record, so
    // that a refused or failed call leaves both as they were)
    struct AsmShape { int group, lanes_log2; } forced_asm = {0, 0};
    // What the debug hooks force, as each place that reads them asks.  The four differ on purpose:
    // m1v_coefficients_device: its run-shaped kernel has no run length, so a forced one does not select it
    bool runs_by_path_or_mode() const { return forced_path == 0 || forced_mode >= 0; }
    // plan_for's producer: a forced run length selects the run kernels too, unless the path hook says tiles
    bool forced_to_runs() const { return runs_by_path_or_mode() || (forced_path < 0 && forced_T > 0); }
    // the layout setters: a forced run length refuses a tile-only layout even beside a forced tile path (lifting that would apply it)
    bool run_hook_set() const { return runs_by_path_or_mode() || forced_T > 0; }
    // plan_for's 4-channel fused table: every hook keeps one probe per quality, the A/B reference inside one process
    bool any_hook_set() const { return forced_path >= 0 || forced_mode >= 0 || forced_T != 0; }
    // The sample format of a float layout, as float_format checks and fills it: the M1V_SAMPLE_* and M1V_RANGE_* values it was set
    // with, a sample's bytes, and the factor that takes a sample to a byte's range
    struct FloatFormat { int sample, range; uint32_t bytes; float scale; };
    // The input layout in force, no zeros: its kind, the frame stride every kind but packed has, and one member per kind.  Only the
    // member of the kind in force is set and read (kind_facts: what the host knows of each kind).
    struct Layout {
        enum class Kind { packed, surface, samples, rgb_planes, float_planes, float_pixels, downscale, downscale_planes, downscale_words } kind = Kind::packed;
        unsigned long long frame_stride = 0;  // bytes from a frame's first byte to the next frame's
        // m1v_set_frame_table / m1v_set_plane_table: d_rgb is a device array of one 64-bit address per frame, or of three (one per
        // plane); frame_stride is kept and unused.  Part of the record, so every setter's fresh record turns tables off and a
        // failed setter leaves the mode as it was.
        enum class Table { off, frames, planes } table = Table::off;
        struct Surface { uint32_t row_pitch; int order; } surface = {}; // m1v_set_input_layout: windows of a pitched surface, M1V_ORDER_* pixels
        // m1v_set_plane_layout (y_step 1), m1v_set_sample_layout: Y, Cb, Cr samples where they lie (m1v_planes.h, m1v_step2.h);
        // extent: bytes of a frame the kernels may read (the read contract of mpeg1_hip.h)
        struct Samples { uint32_t y_off, cb_off, cr_off, y_pitch, c_pitch, y_step, c_step; unsigned long long extent; } samples = {};
        RgbPlaneFrontArgs rgb_planes = {}; // m1v_set_rgb_plane_layout: planes of R, G and B bytes, as their kernels take them (m1v_rgb_planes.h)
        FloatFormat fmt = {};                // the samples of a float plane or float pixel layout
        // m1v_set_float_plane_layout: planes of fp16, bf16 or fp32 samples of R, G and B, as their kernels take them (m1v_float_planes.h)
        FloatPlaneFrontArgs float_planes = {};
        // m1v_set_float_pixel_layout: float samples of R, G and B interleaved per pixel, as their kernels take them
        // (m1v_float_pixels.h), with the pixel step in bytes
        struct FloatPixels { FloatPixelFrontArgs front; uint32_t pixel_step; } float_pixels = {};
        // m1v_set_downscale_layout: byte surfaces of twice the encoder's width and height, as their kernels take them
        // (m1v_downscale.h), with the source pixel step in bytes
        struct Downscale { DownscaleFrontArgs front; uint32_t pixel_step; } downscale = {};
        // m1v_set_downscale_plane_layout: Y, Cb, Cr planes of twice the encoder's width and height, as their kernels take them
        // (m1v_downscale_planes.h; front.lim from the source's extent), with the chroma step in bytes
        struct DownscalePlanes { HalfPlaneFrontArgs front; uint32_t c_step; } downscale_planes = {};
        // m1v_set_downscale_word_layout: Y, Cb, Cr planes of 16-bit words of twice the encoder's width and height, as their
        // kernels take them (m1v_downscale_words.h; front.lim from the source's extent), with the chroma step in bytes
        struct DownscaleWords { HalfWordFrontArgs front; uint32_t c_step; } downscale_words = {};
        bool tiles_only() const { return kind != Kind::packed; }
    } layout;
    Plan plan = {};             // the plan configure_path set up
    unsigned calls = 0;
    hipStream_t side = nullptr;
    uint32_t *d_tile_order = nullptr; // tile-row processing order of the tile kernel (tile_row_order_for), [tile_rows]
    int tile_order_rows = 0;          // for how many tile rows d_tile_order was built
    Tables *d_tab = nullptr;
    // Per-frame quality (frame_rq_t): Tables::rq_t of every quality [100][64]; the selection of the plain path (the encoder's
    // own quality, [max_frames]); the selection k_frame_quality writes; the budget call's probes ([kMaxCandidates][max_frames]
    // sizes, kMaxCandidates status words) and its choice when the caller does not want it
    float *d_rq_all = nullptr;
    float *d_dq_all = nullptr;  // the divisors themselves, indexed as d_rq_all (the rd table's distortion stage)
    uint32_t *d_qsel_own = nullptr, *d_qsel = nullptr;
    unsigned long long *d_probe_sizes = nullptr;
    unsigned long long *d_probe_dist = nullptr; // m1v_encode_rd_device: the distortions beside d_probe_sizes, same shape
    uint32_t *d_probe_status = nullptr;
    uint8_t *d_chosen = nullptr;
    uint32_t *d_pick_status = nullptr; // k_rate_pick's status word (batch-budget and bitrate calls)
    RdStep *d_rd_steps = nullptr;      // k_rd_chains' step table [max_frames][kMaxCandidates] (m1v_encode_rd_batch_device, m1v_rd_batch_pick_device)
    int32_t *d_span_chunks = nullptr;  // k_span_plan's prefix [M1V_MAX_STREAMS + 1] (m1v_span_budget.h); like the step table it lives from
                                       // the plan to the pick, both on the caller's stream: one serves both batches of pipelined mode
    int narrow_q = 0;           // the largest quality whose levels stage in one byte (e->narrow for the encoder's own)
    // The size table's counters: the k_size_table_* / k_rd_table_* kernels add, k_size_table_sizes / k_rd_table_sizes reads and
    // clears what they added.
    struct TableCounters {
        unsigned long long *strip_ctr = nullptr;   // [kMaxCandidates][max_frames][strip]
        unsigned long long *frame_bytes = nullptr; // [kMaxCandidates][max_frames]
        unsigned long long *frame_dist = nullptr;  // [kMaxCandidates][max_frames] the rd table's distortion sums
        uint32_t *words = nullptr;                 // [kMaxCandidates] status words
        bool poisoned = false;                     // a call returned an error after its probe may have added: clear in full
    } table;
    // What an encode kernel adds to and k_assemble reads.  Two sets per Batch, taken in turns: the assemble kernel of call j clears
    // the set call j + 1 will add to (the one call j - 1 used), so no launch and no memset stands between two batches.
    struct Counters {
        unsigned long long *strip_ctr = nullptr;   // [frame][strip] bits of the strip (tile kernel: + arrivals << 40)
        unsigned long long *frame_bytes = nullptr; // [frame] bytes of the frame's strips
        uint32_t *words = nullptr;                 // [0] status bits of the encode kernel, [1] sink for callers without a status word, [2] arena counter
        int dirty_frames = 0;                      // frames of the set's last batch that nobody has cleared yet
        int32_t *frame_index = nullptr;            // [max_frames] a streams batch: each frame's index in its stream (k_streams_map)
    };
    // Everything one batch owns between its encode kernel and the end of its assembly.  Two sets, so that in
    // pipelined mode batch k+1 can encode while batch k is still being assembled.
    struct Batch {
        uint8_t *scratch = nullptr;
        uint32_t *run_meta = nullptr; // run kernels: [frame][run][4]
        uint2 *seg = nullptr;         // [frame][segment][strip] (bits, where): what a strip is concatenated from
        size_t scratch_bytes = 0, meta_bytes = 0, seg_bytes = 0; // sizes of the three above
        Counters ctr[2];
        unsigned turn = 0;
        hipEvent_t enc_done = nullptr, gather_done = nullptr;
        bool gather_pending = false;
        bool poisoned = false;        // a call that took a counter set returned an error: neither set is known to be clear
    } batch[2];
    unsigned long long *d_stamps = nullptr;
    // device-side staging of the host-buffer entry points, kept between calls
    struct HostPath {
        uint8_t *d_in = nullptr, *d_out = nullptr, *d_planes = nullptr;
        unsigned long long *d_meta = nullptr;
        size_t in_cap = 0, out_cap = 0, planes_cap = 0, meta_cap = 0;
        hipStream_t copy_in = nullptr, work = nullptr; // upload stream; convert/encode/download stream
        hipEvent_t uploaded[2] = {};
    } hp;
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
};

using LayoutKind = m1v_encoder::Layout::Kind;
using TableMode = m1v_encoder::Layout::Table;
using FloatFormat = m1v_encoder::FloatFormat;

// What the host knows of a layout kind, apart from its kernels' arguments (launch_tiles) and its registry entries (tile_variant).
// The entry points that ask what kind is in force read a row; none keeps a list of kinds.
struct KindFacts {
    const char *name, *setter, *getter; // how messages call the kind, its setter, and the getter that can describe it
    int plane_getters;                  // what m1v_plane_layout_in_force and m1v_sample_layout_in_force answer: 1 theirs to describe, 0 none
                                        // in force (m1v_input_layout describes it), M1V_E_ARG naming `getter`, as m1v_input_layout then does
    const char *no_frame_table;         // why m1v_set_frame_table refuses the kind; null: a frame table serves it
    const char *no_plane_table;         // why m1v_set_plane_table refuses the kind; null: a plane table serves it
    const char *misaligned;             // the refusal of frames that are no multiple of the float format's sample size; null: bytes, at any address
};
#pragma clang diagnostic push
#pragma clang diagnostic error "-Wswitch" // a kind without a row does not compile
static KindFacts kind_facts(LayoutKind kind) {
    switch (kind) {
    case LayoutKind::packed: // (the surface layout's default)
        return {"packed input", "m1v_set_input_layout", "m1v_input_layout", 0,
                "a frame table needs a surface, plane, sample or RGB plane layout: packed frames go through a table after "
                "m1v_set_input_layout(enc, width * channels, 0, order)",
                "a plane table needs a plane layout (m1v_set_plane_layout) or an RGB plane layout (m1v_set_rgb_plane_layout): "
                "packed pixels have no planes",
                nullptr};
    case LayoutKind::surface:
        return {"a surface layout", "m1v_set_input_layout", "m1v_input_layout", 0, nullptr,
                "a surface layout has one plane: m1v_set_frame_table serves it", nullptr};
    case LayoutKind::samples: return {"a plane layout", "m1v_set_plane_layout", "m1v_plane_layout_in_force", 1, nullptr, nullptr, nullptr};
    case LayoutKind::rgb_planes:
        return {"an RGB plane layout", "m1v_set_rgb_plane_layout", "m1v_rgb_plane_layout_in_force", M1V_E_ARG, nullptr, nullptr, nullptr};
    case LayoutKind::float_planes:
        return {"a float plane layout", "m1v_set_float_plane_layout", "m1v_float_plane_layout_in_force", M1V_E_ARG,
                "a frame table does not serve a float plane layout (m1v_set_float_plane_layout): float frames behind a table are not covered",
                "a plane table does not serve a float plane layout (m1v_set_float_plane_layout): float planes behind separate pointers are "
                "not covered",
                "a float plane layout is in force (m1v_set_float_plane_layout): d_rgb must be a multiple of the sample size"};
    case LayoutKind::float_pixels:
        return {"a float pixel layout", "m1v_set_float_pixel_layout", "m1v_float_pixel_layout_in_force", M1V_E_ARG,
                "a frame table does not serve a float pixel layout (m1v_set_float_pixel_layout): float frames behind a table are not covered",
                "a plane table does not serve a float pixel layout (m1v_set_float_pixel_layout): interleaved pixels have no planes, and "
                "float frames behind a table are not covered",
                "a float pixel layout is in force (m1v_set_float_pixel_layout): d_rgb must be a multiple of the sample size"};
    case LayoutKind::downscale:
        return {"a downscale layout", "m1v_set_downscale_layout", "m1v_downscale_layout_in_force", M1V_E_ARG,
                "a frame table does not serve a downscale layout (m1v_set_downscale_layout): downscaled frames behind a table are not covered",
                "a plane table does not serve a downscale layout (m1v_set_downscale_layout): interleaved pixels have no planes, and "
                "downscaled frames behind a table are not covered",
                nullptr};
    case LayoutKind::downscale_planes:
        return {"a downscale plane layout", "m1v_set_downscale_plane_layout", "m1v_downscale_plane_layout_in_force", M1V_E_ARG,
                "a frame table does not serve a downscale plane layout (m1v_set_downscale_plane_layout): downscaled frames behind a "
                "table are not covered",
                "a plane table does not serve a downscale plane layout (m1v_set_downscale_plane_layout): downscaled planes behind "
                "separate pointers are not covered",
                nullptr};
    case LayoutKind::downscale_words:
        return {"a downscale word layout", "m1v_set_downscale_word_layout", "m1v_downscale_word_layout_in_force", M1V_E_ARG,
                "a frame table does not serve a downscale word layout (m1v_set_downscale_word_layout): downscaled frames behind a "
                "table are not covered",
                "a plane table does not serve a downscale word layout (m1v_set_downscale_word_layout): downscaled planes behind "
                "separate pointers are not covered",
                nullptr};
    }
}
#pragma clang diagnostic pop
// ... of the layout in force as its getters and the plane table see it: to them a sample layout with y_step 2 is a kind of its
// own, which m1v_plane_layout cannot hold and whose planes no table can name
static KindFacts kind_facts(const m1v_encoder::Layout &l) {
    if (l.kind == LayoutKind::samples && l.samples.y_step == 2)
        return {"a layout with samples two bytes apart", "m1v_set_sample_layout", "m1v_sample_layout_in_force", 1, nullptr,
                "a plane table does not serve a (2, 4) sample layout: packed 4:2:2 has no planes, and P010 with separate Y and UV "
                "pointers is not covered",
                nullptr};
    return kind_facts(l.kind);
}

// The one check of a float layout's sample type and range, for the presets and the setters; fills what the rest of the host reads
static int float_format(int sample, int range, FloatFormat &out) {
    const uint32_t bytes = sample == M1V_SAMPLE_F16 || sample == M1V_SAMPLE_BF16 ? 2 : (sample == M1V_SAMPLE_F32 ? 4 : 0);
    if (!bytes) return fail(M1V_E_ARG, "unknown sample type (M1V_SAMPLE_F16, M1V_SAMPLE_BF16, M1V_SAMPLE_F32)%s");
    if (range != M1V_RANGE_UNIT && range != M1V_RANGE_BYTE) return fail(M1V_E_ARG, "unknown range (M1V_RANGE_UNIT, M1V_RANGE_BYTE)%s");
    out = {sample, range, bytes, range == M1V_RANGE_UNIT ? 255.0f : 1.0f};
    return M1V_OK;
}
// ... and of what a float layout gives in bytes (`fields`: all of them ORed; `what`: their names, as the refusal lists them)
static int whole_samples(const FloatFormat &f, unsigned long long fields, const char *what) {
    if (fields % f.bytes == 0) return M1V_OK;
    return fail(M1V_E_ARG, "%s must be multiples of the sample size (%s bytes)", what, f.bytes == 2 ? "2" : "4");
}

// The order in which a frame's tile rows are processed.  Tile row R (macroblock rows 4R..4R+3) reads its luma from picture
// rows [64R, 64R+64) and — the chroma quirk, encoder.h:347-348 — its chroma from rows [16R, 16R+16), i.e. from one quarter of
// the luma region of tile row R/4.  Every byte of the top quarter of the picture is therefore read twice, once as luma and once
// as some other tile row's chroma, and the second read is an L2 hit only if few tile rows pass between the two (an XCD's L2 holds
// 5.7 tile rows of a 3840x2160 frame, 11 of a 1920x1080 one).  Which read comes first does not matter.  So this is the layout of
// the tree "R is the parent of 4R .. 4R+3" on a line that keeps parents and children close: every node sits in the MIDDLE of
// its children, the two smallest subtrees directly beside it, the larger ones outside.  Top to bottom (round 2) four chroma
// reads in five miss at 4K (HBM traffic 1.22x the algorithmic bytes); a depth-first walk (round 3) still loses the later
// children of every inner node (1.07x); this order loses three edges of 33 (1.02x in an LRU model of the L2, tools/l2_order_sim.py).
static void tile_row_order_for(int tile_rows, std::vector<uint32_t> &order) {
    std::vector<int> size((size_t)tile_rows, 1);
    for (int r = tile_rows - 1; r >= 1; r--) size[(size_t)(r / 4)] += size[(size_t)r]; // children have larger indices than parents
    struct Arrange {
        int tile_rows;
        const std::vector<int> &size;
        std::vector<uint32_t> run(int r) const {
            std::vector<int> ch;
            for (int c = 4 * r; c < 4 * r + 4; c++)
                if (c > 0 && c < tile_rows) ch.push_back(c);
            std::stable_sort(ch.begin(), ch.end(), [&](int x, int y) { return size[(size_t)x] < size[(size_t)y]; });
            std::vector<uint32_t> left, right;
            for (size_t i = 0; i < ch.size(); i++) {
                const std::vector<uint32_t> a = run(ch[i]);
                if (i == 0) left.insert(left.end(), a.begin(), a.end());          // smallest: directly in front of r
                else if (i == 1) right.insert(right.begin(), a.begin(), a.end()); // next: directly behind r
                else if (i == 2) left.insert(left.begin(), a.begin(), a.end());   // the larger ones outside
                else right.insert(right.end(), a.begin(), a.end());
            }
            left.push_back((uint32_t)r);
            left.insert(left.end(), right.begin(), right.end());
            return left;
        }
    };
    order = Arrange{tile_rows, size}.run(0);
}

// The region of a width x height picture that `mode` codes: every whole macroblock, or the reference's 96x144 corner
struct CodedRegion {
    int xe, ye;
    CodedRegion(int width, int height, int mode) : xe(mode == M1V_MODE_FULL ? (width & ~15) : 96), ye(mode == M1V_MODE_FULL ? (height & ~15) : 144) {}
    bool fits(int width, int height) const { return xe <= width && ye <= height; }
    // worst case of a strip: its slice header, then per macroblock row two bits and six blocks
    unsigned long long strip_bits() const { return 38ull + (unsigned long long)(ye / 16) * (2 + 6 * kMaxBlockBits); }
};

// The tile grid over a picture (the tile kernels, the fused size table, k_coefficient_tiles)
struct TileGrid {
    int cols, rows;
    explicit TileGrid(const Geometry &g) : cols((g.n_strips + kTileStrips - 1) / kTileStrips), rows((g.n_mbrows + kTileMbRows - 1) / kTileMbRows) {}
    int units() const { return cols * rows; }
};

// LDS bytes of a wave's region in those kernels: its ring of pixel slots, or the `stage_words` it stages per lane if that is more
static uint32_t wave_region(size_t stage_words) {
    return (std::max<uint32_t>((uint32_t)M1V_TILE_RING * kTileSlot, (uint32_t)(kWave * stage_words * 4)) + 15u) & ~15u;
}

// The plan of an encoder: a pure function of its geometry, its quality and its settings; M1V_E_ARG for settings that cannot
// launch.  e.forced_T: run length of the run kernels (0 = default: 256 blocks = 4 waves, one per SIMD, so that 5 workgroups of
// 96-VGPR waves share a CU; or the largest multiple of 64 that the strip holds when it has fewer than 256 blocks).
static int plan_for(const m1v_encoder &e, Plan &out) {
    const Geometry &g = e.g;
    const int bps = g.n_mbrows * 6;
    const size_t stride = e.narrow ? kStageStride8 : kStageStride16;
    Plan p = {};
    // Tiles for every 3-channel picture: 1.3-4x faster than the run kernel where that cannot use its aligned 24-byte row loads
    // (widths that are not a multiple of 8, buffers off a 4-byte boundary), 1 % faster at 4K (the order of the tile rows keeps
    // the chroma re-reads in L2, tile_row_order_for), and 0.5-1 % faster per step on aligned 1080p in a sustained run
    // (profiles/r03_ab_history.txt).  The run kernel serves 4-channel input and the m1v_debug_set_* hooks.
    // A surface layout takes the same plan for 3 and 4 channels (k_encode_surface; no hook can be set beside it), and so does a
    // plane layout (k_encode_planes, 3 channels).
    const TileGrid grid(g);
    if (e.layout.tiles_only() || (g.C == 3 && !e.forced_to_runs())) {
        p.producer = Producer::tiles;
        p.block = kTileThreads;
        p.tile_cols = grid.cols;
        p.tile_rows = grid.rows;
        p.units = grid.units();
        p.luma_region = p.chroma_region = wave_region(stride);
        // worst case of a tile: 8 word-aligned segments of 24 blocks of <= 886 + 2 bits, 8 slice headers, slack
        p.run_cap = (uint32_t)(((((size_t)kTileThreads * (kMaxBlockBits + 2) + kTileStrips * (38 + 32) + 64 + 7) / 8) + 32 + 15) & ~(size_t)15);
        // LDS image of the tile's bits (192 blocks: ~115 words at quality 12 on noise), scaled with the quantiser like the
        // run kernels' (512 words per 256 blocks at quality <= 25) + the segments' word alignment and slice headers
        p.image_words = e.lds_words > 0 ? e.lds_words : (e.qf <= 25 ? 400 : (e.qf <= 50 ? 784 : (e.qf <= 76 ? 1552 : 3088)));
        p.image_words = (p.image_words + 3) & ~3; // cleared 16 bytes per lane
        p.lds_bytes = (size_t)kTileFixedWords * 4 + 2 * (size_t)p.luma_region + p.chroma_region + (size_t)p.image_words * 4;
        p.segs = p.tile_rows;
        p.table_units = p.units;
    } else if (e.dense) {
        const int T = e.forced_T > 0 ? e.forced_T : (bps >= 256 ? 256 : (bps / kWave) * kWave);
        if (T < kWave || T > 384 || T % kWave || T > bps) return fail(M1V_E_ARG, "bad dense run length%s");
        p.producer = Producer::dense;
        p.block = T;
        p.units = (g.n_strips * bps + T - 1) / T;
        // worst case of a run: two word-aligned segments of at most T blocks of <= 886 + 2 bits, two slice headers, slack
        p.run_cap = (uint32_t)(((((size_t)T * (kMaxBlockBits + 2) + 2 * 38 + 3 * 32 + 7) / 8) + 32 + 15) & ~(size_t)15);
        // LDS image of the run's bits: zeroing it costs time, outgrowing it the slow global-atomics path.  A run of 256
        // blocks needs ~150 words at quality 12 on noise; scale the default with the quantiser (finer quantisers emit
        // more bits per block).  The compact scratch slot of a run is exactly that image.
        p.image_words = e.lds_words > 0 ? e.lds_words : (e.qf <= 25 ? 512 : (e.qf <= 50 ? 1024 : (e.qf <= 76 ? 2048 : 4096)));
        const size_t zero_iters = ((size_t)p.image_words + T - 1) / T;
        p.zero_iters = (int)zero_iters; // (small whenever the LDS check below passes)
        p.lds_bytes = ((size_t)(T / kWave) * kVlcWords + 32 + stride * T + zero_iters * T) * 4;
        p.meta_bytes = (size_t)e.max_frames * p.units * 4 * sizeof(uint32_t);
        p.segs = (bps + T - 1) / T + 1; // the most runs whose blocks one strip can hold
    } else {
        p.producer = Producer::strips;
        p.block = kWave;
        p.units = g.n_strips;
        p.image_words = e.lds_words > 0 ? e.lds_words : kDefaultLdsWords;
        p.lds_bytes = ((size_t)kVlcWords + 32 + (size_t)kStageStride16 * kWave + (size_t)p.image_words) * 4;
        p.scratch_bytes = (size_t)e.max_frames * g.n_strips * g.strip_cap;
        p.segs = 1; // a strip is one piece
    }
    if (p.lds_bytes > 160 * 1024) return fail(M1V_E_ARG, "LDS budget exceeded: the LDS image is too large%s");
    // The fused size table of a 4-channel encoder (k_size_table_rgba): the tile workgroup over the picture, whichever run kernel
    // encodes it.  The test hooks that force a path, an input mode or a run length keep one probe per quality: the A/B
    // reference inside one process.
    if (g.C == 4 && !e.any_hook_set()) {
        p.tile_cols = grid.cols;
        p.tile_rows = grid.rows;
        p.table_units = grid.units();
    }
    if (p.table_units) {
        // per wave: the ring, or the staged levels at the widest quality the encoder allows; no image
        p.table_region = wave_region(stride);
        p.table_lds_bytes = (size_t)kTableFixedWords * 4 + 3 * (size_t)p.table_region;
        if (p.table_lds_bytes > 160 * 1024) return fail(M1V_E_ARG, "LDS budget exceeded: the size table does not fit%s");
    }
    if (p.producer != Producer::strips) {
        // Scratch: one compact slot per unit + an overflow arena of worst-case slots for the units whose image outgrows LDS
        // (handed out by an atomic counter).  By default the arena holds 1/256 of the units (quality 12 noise needs none);
        // m1v_reserve_scratch(enc, 1) sizes it for all of them — what every run had in round 1, 47x the payload.
        // + 128: an odd number of 128-byte lines, so that the slots (of which only the first third is written at quality
        // 12) do not all start on the same few memory channels (a power-of-two stride measured 3 % slower)
        const size_t units = (size_t)e.max_frames * p.units;
        p.slot_bytes = (uint32_t)((((size_t)p.image_words * 4 + 127) & ~(size_t)127) | 128);
        p.arena_slots = (uint32_t)(e.reserve_worst ? units : (units / 256 > 32 ? units / 256 : (units < 32 ? units : 32)));
        p.arena_off = units * p.slot_bytes;
        p.scratch_bytes = p.arena_off + (size_t)p.arena_slots * p.run_cap;
    }
    if ((p.scratch_bytes >> 2) >= (1ull << 32)) return fail(M1V_E_ARG, "scratch beyond 16 GiB: lower max_frames%s");
    p.seg_bytes = (size_t)e.max_frames * g.n_strips * p.segs * sizeof(uint2);
    // k_assemble (m1v_assemble.h): strips per workgroup so that a group's bytes fit its 14-KiB LDS image (eight workgroups per CU) in one pass on noise at
    // this quality (19 bits per block at quality 12; anything larger takes more passes), a power of two (the eight
    // strips of a tile column share their scratch lines); lanes per segment (four words each) ~ the words a segment holds.
    const int qscale = e.qf <= 25 ? 1 : (e.qf <= 50 ? 2 : (e.qf <= 76 ? 4 : 8));
    const size_t bpb = 22u * (size_t)qscale;
    const size_t strip_est = (38 + (size_t)g.n_mbrows * (2 + 6 * bpb)) / 8 + 1;
    p.asm_group = 1;
    while (p.asm_group < kAsmMaxGroup && (size_t)(2 * p.asm_group) * strip_est * 5 / 4 <= kAsmImageBytes && 2 * p.asm_group <= g.n_strips) p.asm_group *= 2;
    const size_t seg_blocks = p.producer == Producer::tiles ? (size_t)kTileSegBlocks : (size_t)(p.producer == Producer::dense ? p.block : bps);
    const size_t seg_words = seg_blocks * bpb / 32;
    p.asm_lanes_log2 = 1; // four words per lane: enough lanes for 1.6 x the expected words, at most one DPP row
    while (p.asm_lanes_log2 < 4 && ((size_t)4 << p.asm_lanes_log2) * 5 < seg_words * 8) p.asm_lanes_log2++;
    // m1v_debug_set_assemble_shape (it has checked the values): any shape is correct, the plan's own is the fast one
    if (e.forced_asm.group > 0) p.asm_group = e.forced_asm.group;
    if (e.forced_asm.lanes_log2 > 0) p.asm_lanes_log2 = e.forced_asm.lanes_log2;
    out = p;
    return M1V_OK;
}

// Every kernel that takes dynamic LDS: the launches pick from it (tile_variant, run_kernel) and m1v_create raises the limit of
// each.  [narrow staging] last; a null entry is a variant that does not exist.
//   tile[TileFamily::row][tile_variant()]: the tile-shaped kernels of every input layout, each filled in beside its name
//   table[...][...]: their kt_* twins of a frame table (m1v_set_frame_table); null for the packed variants, which take none
//   dense, strips [input mode]: the pixel loads of the run kernels (load_block_rows): 1 = aligned rows, 2 = any row offset in an
//   aligned buffer (3 channels), 3 = aligned 4-channel pixels, 0 = byte loads.  The strip kernel has modes 0 and 1 and stages
//   every level wide.
enum TileVariant { kPacked3, kPacked4, kSurfaceRgb3, kSurfaceBgr3, kSurfaceRgb4, kSurfaceBgr4, kPlanes, kPlanesPaired, kStep2, kRgbPlanes, kFloatPlanesF16, kFloatPlanesBf16,
                   kFloatPlanesF32, kFloatPixelsF16x3, kFloatPixelsF16x4, kFloatPixelsBf16x3, kFloatPixelsBf16x4, kFloatPixelsF32x3, kFloatPixelsF32x4,
                   kDownscale3, kDownscale4, kHalfPlanes, kHalfPlanesPaired, kHalfWords, kHalfWordsPaired,
                   kTileVariants };
enum TileRow { kEncode, kSizeTable, kRdTable, kTileRows };
//   planes[...][...]: their kp_* twins of a plane table (m1v_set_plane_table); kPlanes, kPlanesPaired and kRgbPlanes only
struct Kernels { const void *tile[kTileRows][kTileVariants][2], *table[kTileRows][kTileVariants][2], *planes[kTileRows][kTileVariants][2], *dense[4][2], *strips[2][2]; };
// K<wide>, K<narrow> with the tile ring and the variant's own template arguments behind it
#define M1V_PAIR(DST, K, ...) ((DST)[0] = (const void *)&K<false, M1V_TILE_RING, ##__VA_ARGS__>, (DST)[1] = (const void *)&K<true, M1V_TILE_RING, ##__VA_ARGS__>)
// one layout variant's encode, size-table and rd-table kernels: k_encode_<NAME>, k_size_table_<NAME>, k_rd_table_<NAME>, and kt_* of each
#define M1V_TILE_VARIANT(V, NAME, ...)                                                                                            \
    (M1V_PAIR(k.tile[kEncode][V], k_encode_##NAME, ##__VA_ARGS__), M1V_PAIR(k.tile[kSizeTable][V], k_size_table_##NAME, ##__VA_ARGS__), \
     M1V_PAIR(k.tile[kRdTable][V], k_rd_table_##NAME, ##__VA_ARGS__),                                                             \
     M1V_PAIR(k.table[kEncode][V], kt_encode_##NAME, ##__VA_ARGS__), M1V_PAIR(k.table[kSizeTable][V], kt_size_table_##NAME, ##__VA_ARGS__), \
     M1V_PAIR(k.table[kRdTable][V], kt_rd_table_##NAME, ##__VA_ARGS__))
// the float plane kernels of one sample type: no kt_* or kp_* twins (float frames and planes behind tables are not covered)
#define M1V_FLOAT_VARIANT(V, T)                                                                                                   \
    (M1V_PAIR(k.tile[kEncode][V], k_encode_float_planes, T), M1V_PAIR(k.tile[kSizeTable][V], k_size_table_float_planes, T),      \
     M1V_PAIR(k.tile[kRdTable][V], k_rd_table_float_planes, T))
// the float pixel kernels of one sample type and pixel width (m1v_float_pixels.h): no table twins either
#define M1V_FLOAT_PIXEL_VARIANT(V, T, C)                                                                                          \
    (M1V_PAIR(k.tile[kEncode][V], k_float_pixels_encode, T, C), M1V_PAIR(k.tile[kSizeTable][V], k_float_pixels_size_table, T, C), \
     M1V_PAIR(k.tile[kRdTable][V], k_float_pixels_rd_table, T, C))
// the downscale kernels of one source pixel width (m1v_downscale.h): no table twins either
#define M1V_DOWNSCALE_VARIANT(V, C)                                                                                               \
    (M1V_PAIR(k.tile[kEncode][V], k_downscale_encode, C), M1V_PAIR(k.tile[kSizeTable][V], k_downscale_size_table, C),            \
     M1V_PAIR(k.tile[kRdTable][V], k_downscale_rd_table, C))
// the downscaled plane kernels of one chroma step (m1v_downscale_planes.h): no table twins either
#define M1V_HALF_PLANE_VARIANT(V, CSTEP)                                                                                          \
    (M1V_PAIR(k.tile[kEncode][V], k_half_planes_encode, CSTEP), M1V_PAIR(k.tile[kSizeTable][V], k_half_planes_size_table, CSTEP), \
     M1V_PAIR(k.tile[kRdTable][V], k_half_planes_rd_table, CSTEP))
// the downscaled word kernels of one chroma step (m1v_downscale_words.h): no table twins either
#define M1V_HALF_WORD_VARIANT(V, CSTEP)                                                                                           \
    (M1V_PAIR(k.tile[kEncode][V], k_half_words_encode, CSTEP), M1V_PAIR(k.tile[kSizeTable][V], k_half_words_size_table, CSTEP),   \
     M1V_PAIR(k.tile[kRdTable][V], k_half_words_rd_table, CSTEP))
// ... and its kp_* kernels of a plane table
#define M1V_PLANE_TABLE_VARIANT(V, NAME, ...)                                                                                     \
    (M1V_PAIR(k.planes[kEncode][V], kp_encode_##NAME, ##__VA_ARGS__), M1V_PAIR(k.planes[kSizeTable][V], kp_size_table_##NAME, ##__VA_ARGS__), \
     M1V_PAIR(k.planes[kRdTable][V], kp_rd_table_##NAME, ##__VA_ARGS__))
static const Kernels kKernels = [] {
    Kernels k = {{}, {}, {},
                 {{(const void *)&k_encode_dense<0, false>, (const void *)&k_encode_dense<0, true>},
                  {(const void *)&k_encode_dense<1, false>, (const void *)&k_encode_dense<1, true>},
                  {(const void *)&k_encode_dense<2, false>, (const void *)&k_encode_dense<2, true>},
                  {(const void *)&k_encode_dense<3, false>, (const void *)&k_encode_dense<3, true>}},
                 {{(const void *)&k_encode_strips<false>, (const void *)&k_encode_strips<false>},
                  {(const void *)&k_encode_strips<true>, (const void *)&k_encode_strips<true>}}};
    M1V_PAIR(k.tile[kEncode][kPacked3], k_encode_tiles); // (the packed kernels have no frame-table twins)
    M1V_PAIR(k.tile[kSizeTable][kPacked3], k_size_table_tiles);
    M1V_PAIR(k.tile[kRdTable][kPacked3], k_rd_table_tiles);
    M1V_PAIR(k.tile[kSizeTable][kPacked4], k_size_table_rgba); // (packed 4-channel pictures encode on the run kernels)
    M1V_PAIR(k.tile[kRdTable][kPacked4], k_rd_table_rgba);
    M1V_TILE_VARIANT(kSurfaceRgb3, surface, 3, M1V_ORDER_RGB);
    M1V_TILE_VARIANT(kSurfaceBgr3, surface, 3, M1V_ORDER_BGR);
    M1V_TILE_VARIANT(kSurfaceRgb4, surface, 4, M1V_ORDER_RGB);
    M1V_TILE_VARIANT(kSurfaceBgr4, surface, 4, M1V_ORDER_BGR);
    M1V_TILE_VARIANT(kPlanes, planes, 1);
    M1V_TILE_VARIANT(kPlanesPaired, planes, 2);
    M1V_TILE_VARIANT(kStep2, step2);
    M1V_TILE_VARIANT(kRgbPlanes, rgb_planes);
    M1V_PLANE_TABLE_VARIANT(kPlanes, planes, 1);
    M1V_PLANE_TABLE_VARIANT(kPlanesPaired, planes, 2);
    M1V_PLANE_TABLE_VARIANT(kRgbPlanes, rgb_planes);
    M1V_FLOAT_VARIANT(kFloatPlanesF16, F16Sample);
    M1V_FLOAT_VARIANT(kFloatPlanesBf16, Bf16Sample);
    M1V_FLOAT_VARIANT(kFloatPlanesF32, F32Sample);
    M1V_FLOAT_PIXEL_VARIANT(kFloatPixelsF16x3, F16Sample, 3);
    M1V_FLOAT_PIXEL_VARIANT(kFloatPixelsF16x4, F16Sample, 4);
    M1V_FLOAT_PIXEL_VARIANT(kFloatPixelsBf16x3, Bf16Sample, 3);
    M1V_FLOAT_PIXEL_VARIANT(kFloatPixelsBf16x4, Bf16Sample, 4);
    M1V_FLOAT_PIXEL_VARIANT(kFloatPixelsF32x3, F32Sample, 3);
    M1V_FLOAT_PIXEL_VARIANT(kFloatPixelsF32x4, F32Sample, 4);
    M1V_DOWNSCALE_VARIANT(kDownscale3, 3);
    M1V_DOWNSCALE_VARIANT(kDownscale4, 4);
    M1V_HALF_PLANE_VARIANT(kHalfPlanes, 1);
    M1V_HALF_PLANE_VARIANT(kHalfPlanesPaired, 2);
    M1V_HALF_WORD_VARIANT(kHalfWords, 2);
    M1V_HALF_WORD_VARIANT(kHalfWordsPaired, 4);
    return k;
}();
#undef M1V_HALF_WORD_VARIANT
#undef M1V_HALF_PLANE_VARIANT
#undef M1V_DOWNSCALE_VARIANT
#undef M1V_FLOAT_PIXEL_VARIANT
#undef M1V_FLOAT_VARIANT
#undef M1V_PLANE_TABLE_VARIANT
#undef M1V_TILE_VARIANT
#undef M1V_PAIR

// defined in m1v_runtime.h
static int profile_event(m1v_encoder *e, hipStream_t st);
static int fail_encode_at(int stage);
static hipError_t counters_clear(const m1v_encoder *e, m1v_encoder::Counters &c, hipStream_t st);
static hipError_t table_clear(const m1v_encoder *e, hipStream_t st);

static bool fast_path(const m1v_encoder *e, const uint8_t *d_rgb) {
    return e->fast_ok && ((uintptr_t)d_rgb & 3) == 0;
}

static int encoder_quality(const m1v_encoder *e) { return std::min(std::max(e->qf, 1), 100); }

// The tile-shaped kernels' variant for the layout in force (Kernels::tile): the one place that maps channels, byte order and
// sample steps to an instantiation
static TileVariant tile_variant(const m1v_encoder *e) {
    static_assert(M1V_SAMPLE_F16 == 0 && M1V_SAMPLE_BF16 == 1 && M1V_SAMPLE_F32 == 2 && kFloatPlanesF32 == kFloatPlanesF16 + 2 &&
                  kFloatPixelsBf16x3 == kFloatPixelsF16x3 + 2 && kFloatPixelsF32x4 == kFloatPixelsF16x3 + 5, "the float variants' order");
    const m1v_encoder::Layout &l = e->layout;
    const bool four = e->g.C == 4;
    switch (l.kind) {
    case LayoutKind::rgb_planes: return kRgbPlanes;
    // (the float variants lie in the order of the M1V_SAMPLE_* values; those of pixels [type][3 | 4 samples per pixel])
    case LayoutKind::float_planes: return (TileVariant)(kFloatPlanesF16 + l.fmt.sample);
    case LayoutKind::float_pixels: return (TileVariant)(kFloatPixelsF16x3 + 2 * l.fmt.sample + (l.float_pixels.pixel_step == 4u * l.fmt.bytes ? 1 : 0));
    case LayoutKind::downscale: return l.downscale.pixel_step == 4u ? kDownscale4 : kDownscale3;
    case LayoutKind::downscale_planes: return l.downscale_planes.c_step == 2u ? kHalfPlanesPaired : kHalfPlanes;
    case LayoutKind::downscale_words: return l.downscale_words.c_step == 4u ? kHalfWordsPaired : kHalfWords;
    case LayoutKind::samples: return l.samples.y_step == 2 ? kStep2 : (l.samples.c_step == 2 ? kPlanesPaired : kPlanes);
    case LayoutKind::surface: return l.surface.order == M1V_ORDER_BGR ? (four ? kSurfaceBgr4 : kSurfaceBgr3) : (four ? kSurfaceRgb4 : kSurfaceRgb3);
    case LayoutKind::packed: return four ? kPacked4 : kPacked3;
    }
}

// the run kernel (plan: dense or strips) for this input pointer
static const void *run_kernel(const m1v_encoder *e, const uint8_t *d_rgb) {
    const bool aligned4 = ((uintptr_t)d_rgb & 3) == 0, fast = fast_path(e, d_rgb);
    if (e->plan.producer == Producer::strips) return kKernels.strips[fast ? 1 : 0][e->narrow ? 1 : 0];
    int mode = fast ? 1 : (aligned4 && e->g.C == 3 ? 2 : (aligned4 && e->g.C == 4 ? 3 : 0));
    if (e->forced_mode == 0 || (e->forced_mode == 2 && mode == 1)) mode = e->forced_mode; // only modes that are valid here
    return kKernels.dense[mode][e->narrow ? 1 : 0];
}

// One launch of a kernel that takes its arguments as one struct, with profile events around it
static int launch_profiled(m1v_encoder *e, const void *kernel, size_t grid, int block, void *arg, size_t lds, hipStream_t st) {
    void *args[] = {arg};
    if (e->prof && profile_event(e, st) != M1V_OK) return M1V_E_HIP;
    (void)hipLaunchKernel(kernel, dim3((unsigned)grid), dim3((unsigned)block), args, lds, st);
    if (e->prof && profile_event(e, st) != M1V_OK) return M1V_E_HIP;
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

// What TileArgs and TableArgs share: the input, the tables and the tile grid of the plan over n_frames
template <typename Args>
static void fill_tile_grid(const m1v_encoder *e, const uint8_t *d_rgb, int n_frames, Args &a) {
    const Plan &p = e->plan;
    a.g = e->g;
    a.rgb = d_rgb;
    a.tab = e->d_tab;
    a.rq_all = e->d_rq_all;
    a.n_frames = n_frames;
    a.tile_cols = p.tile_cols;
    a.tile_rows = p.tile_rows;
    a.tiles_per_frame = p.tile_cols * p.tile_rows; // (Plan::units of the tile producer, Plan::table_units)
    const unsigned long long units = (unsigned long long)n_frames * (unsigned long long)a.tiles_per_frame;
    a.div_group = div_magic(8u * (uint32_t)a.tiles_per_frame, units);
    a.div_frame = div_magic((uint32_t)a.tiles_per_frame, units);
    a.div_cols = div_magic((uint32_t)p.tile_cols, (unsigned long long)a.tiles_per_frame);
    a.tile_row_order = e->d_tile_order;
}

// What a tile-shaped kernel's base arguments are wrapped in for each layout kind, and their row of Kernels::tile
template <typename Base> struct TileFamily;
template <> struct TileFamily<TileArgs> { static constexpr TileRow row = kEncode; using Surface = SurfaceArgs; using Samples = PlaneArgs; using RgbPlanes = RgbPlaneArgs; using FloatPlanes = FloatPlaneArgs; using FloatPixels = FloatPixelArgs; using Downscale = DownscaleArgs; using DownscalePlanes = HalfPlaneArgs; using DownscaleWords = HalfWordArgs; };
template <> struct TileFamily<TableArgs> { static constexpr TileRow row = kSizeTable; using Surface = SurfaceTableArgs; using Samples = PlaneTableArgs; using RgbPlanes = RgbPlaneTableArgs; using FloatPlanes = FloatPlaneTableArgs; using FloatPixels = FloatPixelTableArgs; using Downscale = DownscaleTableArgs; using DownscalePlanes = HalfPlaneTableArgs; using DownscaleWords = HalfWordTableArgs; };
template <> struct TileFamily<RdTableArgs> { static constexpr TileRow row = kRdTable; using Surface = SurfaceRdArgs; using Samples = PlaneRdArgs; using RgbPlanes = RgbPlaneRdArgs; using FloatPlanes = FloatPlaneRdArgs; using FloatPixels = FloatPixelRdArgs; using Downscale = DownscaleRdArgs; using DownscalePlanes = HalfPlaneRdArgs; using DownscaleWords = HalfWordRdArgs; };

// The tile-shaped kernel of a's family over the grid a carries (fill_tile_grid), with a wrapped for the layout in force
template <typename Args>
static int launch_tiles(m1v_encoder *e, bool narrow, Args &a, size_t grid, size_t lds, hipStream_t st) {
    using Family = TileFamily<Args>;
    const m1v_encoder::Layout &l = e->layout;
    // (a frame table has the kt_* twin of the variant's kernel, which reads a.rgb as the table and not the stride: frame_table_entry)
    // (a plane table has the kp_* twin, which reads a.rgb as three addresses per frame: plane_table_row, PlaneBases)
    const auto &rows = l.table == TableMode::planes ? kKernels.planes : (l.table == TableMode::frames ? kKernels.table : kKernels.tile);
    const void *kernel = rows[Family::row][tile_variant(e)][narrow ? 1 : 0];
    if (!kernel) return fail(M1V_E_ARG, "no kernel serves the table mode in force with this layout%s"); // (m1v_set_plane_table refuses those layouts)
    auto launch = [&](auto &&arg) { return launch_profiled(e, kernel, grid, kTileThreads, &arg, lds, st); };
    const m1v_encoder::Layout::Samples &s = l.samples;
    const unsigned long long stride = l.frame_stride;
    if (l.table == TableMode::planes) {
        if (l.kind == LayoutKind::rgb_planes) return launch(RgbPlanePtrArgs<Args>{a, l.rgb_planes});
        // one limit per chroma plane, relative to its own pointer: the last offset at which a 16-byte unit may start, from the
        // plane's extent E_p = p_off + (rows - 1) * c_pitch + row bytes (the read contract of mpeg1_hip.h), rounded up to whole dwords
        const unsigned long long xe = (unsigned long long)e->g.n_strips * 16, ye = (unsigned long long)e->g.n_mbrows * 16;
        const unsigned long long c_rows = (ye / 2 - 1) * s.c_pitch + (xe / 2 - 1) * s.c_step + 1;
        auto lim = [&](uint32_t off) { return (uint32_t)(((off + c_rows + 3ull) & ~3ull) - 16ull); };
        return launch(PlanePtrArgs<Args>{a, {s.y_off, s.cb_off, s.cr_off, s.y_pitch, s.c_pitch, lim(s.cb_off), lim(s.cr_off)}});
    }
    switch (l.kind) {
    case LayoutKind::surface: return launch(typename Family::Surface{a, stride, l.surface.row_pitch});
    case LayoutKind::samples: // (the 16-byte unit that ends with the frame's extent, rounded up to whole dwords, is the last one a plane kernel may load)
        return launch(typename Family::Samples{a, {s.y_off, s.cb_off, s.cr_off, s.y_pitch, s.c_pitch, (uint32_t)(((s.extent + 3ull) & ~3ull) - 16ull)}, stride});
    case LayoutKind::rgb_planes: return launch(typename Family::RgbPlanes{a, l.rgb_planes, stride});
    case LayoutKind::float_planes: return launch(typename Family::FloatPlanes{a, l.float_planes, stride});
    case LayoutKind::float_pixels: return launch(typename Family::FloatPixels{a, l.float_pixels.front, stride});
    case LayoutKind::downscale: return launch(typename Family::Downscale{a, l.downscale.front, stride});
    case LayoutKind::downscale_planes: return launch(typename Family::DownscalePlanes{a, l.downscale_planes.front, stride});
    case LayoutKind::downscale_words: return launch(typename Family::DownscaleWords{a, l.downscale_words.front, stride});
    case LayoutKind::packed: return launch(a);
    }
}

// With a frame or plane table on, d_rgb is read as 64-bit words by scalar loads: refused here, in front of every launch, when misaligned.
// So are float frames whose samples would not be naturally aligned (KindFacts::misaligned; the float layouts have no table mode).
static int check_frame_table(const m1v_encoder *e, const uint8_t *d_rgb) {
    const char *misaligned = kind_facts(e->layout.kind).misaligned;
    if (misaligned && ((uintptr_t)d_rgb & (e->layout.fmt.bytes - 1u)) != 0) return fail(M1V_E_ARG, "%s", misaligned);
    if (e->layout.table == TableMode::off || ((uintptr_t)d_rgb & 7) == 0) return M1V_OK;
    if (e->layout.table == TableMode::planes)
        return fail(M1V_E_ARG, "a plane table is on (m1v_set_plane_table): d_rgb is an array of three 64-bit plane addresses per frame and must be 8-byte aligned%s");
    return fail(M1V_E_ARG, "a frame table is on (m1v_set_frame_table): d_rgb is an array of 64-bit frame addresses and must be 8-byte aligned%s");
}

// The frame count of one call, in front of everything it queues: within max_frames, and within the grid extents of the device,
// since k_assemble takes the batch's frames as its grid's y and the run-shaped k_coefficients as its grid's z (m1v_batch_limit).
static int check_grid_frames(const m1v_encoder *e, int n_frames) {
    if (n_frames > e->batch_limit)
        return fail(M1V_E_ARG, "n_frames exceeds the %s frames of one batch on this device (m1v_batch_limit: a grid's y and z extent)",
                    std::to_string(e->batch_limit).c_str());
    return M1V_OK;
}
static int check_batch_frames(const m1v_encoder *e, int n_frames) {
    if (n_frames < 0 || n_frames > e->max_frames) return fail(M1V_E_ARG, "n_frames exceeds max_frames%s");
    return check_grid_frames(e, n_frames);
}

// From its construction on, an error return leaves counters half used: the flag tells the next call to clear them first
struct PoisonOnReturn {
    bool *flag;
    ~PoisonOnReturn() { if (flag) *flag = true; }
};

// The counter hand-over of a batch's last kernel (k_assemble or k_frame_sizes): it clears the first next_frames frames of the set
// the next batch on this Batch adds to.  What a longer batch than this one left there beyond n_frames is cleared here, on gs.
template <typename Args>
static int hand_over(Args &a, m1v_encoder::Counters &cur, m1v_encoder::Counters &nxt, int n_frames, int n_strips, hipStream_t gs) {
    a.next_strip_ctr = nxt.strip_ctr;
    a.next_frame_bytes = nxt.frame_bytes;
    a.next_words = nxt.words;
    if (nxt.dirty_frames > n_frames) {
        HIP_TRY(hipMemsetAsync(nxt.strip_ctr, 0, (size_t)nxt.dirty_frames * n_strips * 8, gs));
        HIP_TRY(hipMemsetAsync(nxt.frame_bytes, 0, (size_t)nxt.dirty_frames * 8, gs));
        nxt.dirty_frames = 0;
    }
    a.next_frames = nxt.dirty_frames;
    nxt.dirty_frames = 0;
    cur.dirty_frames = n_frames;
    return M1V_OK;
}

// What writes the per-frame selection (e->d_qsel) of a batch that is not encoded at the encoder's own quality: launch() queues,
// on st, whatever does (k_frame_quality; k_rd_pick; k_rd_batch_pick, then k_frame_quality: m1v_runtime.h) with `args`, the
// batch's counter set (its words[0] is the batch's status word) and n_frames.  One step per batch: a batch cannot be given two.
// own_quality: the step leaves the selection alone and the batch is encoded at the encoder's own quality.  finish (may be null)
// queues what the step needs behind k_assemble, on the stream k_assemble runs on (a streams batch: k_streams_finish).
struct EncodeOut;
struct Selection {
    int (*launch)(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, int n_frames, hipStream_t st);
    void *args;
    bool own_quality = false;
    int (*finish)(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, const EncodeOut &o, int n_frames, hipStream_t gs) = nullptr;
};

// Where a batch's results go (the last five arguments of m1v_encode_device).  A probe writes frame_sizes and status only.
struct EncodeOut {
    uint8_t *out;
    size_t cap;
    uint64_t *frame_sizes, *total;
    uint32_t *status;
};

// One batch through the encode kernel of the encoder's plan.  sel == null: every frame at the encoder's own quality (the plain
// path); otherwise sel's step first writes the per-frame selection, behind the poison / hand-over logic and fail stage 1 and in
// front of the producer kernel, on the caller's stream.  An empty batch returns before it.  probe: the counter hand-over ends in
// k_frame_sizes instead of k_assemble (record sizes and status only; o.out is not touched).
static int encode_batch(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index, const Selection *sel, bool probe,
                        const EncodeOut &o, void *stream) {
    if (!e || (!d_rgb && n_frames > 0) || (!o.out && !probe)) return fail(M1V_E_ARG, "null pointer%s"); // (an empty batch reads no input)
    if (const int rc = check_batch_frames(e, n_frames)) return rc;
    if (const int rc = check_frame_table(e, d_rgb)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(e->device));
    m1v_encoder::Batch &bt = e->batch[e->pipelined ? (e->calls++ & 1u) : 0];
    hipStream_t gs = e->pipelined ? e->side : st;   // stream of the layout + gather kernels
    if (e->pipelined && bt.gather_pending)           // this set's previous gather must have drained its scratch
        HIP_TRY(hipStreamWaitEvent(st, bt.gather_done, 0));
    if (bt.poisoned) {
        // The last call on this Batch failed after it took a counter set: its kernels may have added to one set and left
        // the other uncleared.  Behind everything already queued on the internal stream (the failed call's layout and
        // assembly, whose completion event may never have been recorded), clear both sets in full.
        if (e->pipelined) {
            HIP_TRY(hipEventRecord(bt.gather_done, gs));
            HIP_TRY(hipStreamWaitEvent(st, bt.gather_done, 0));
        }
        for (m1v_encoder::Counters &c : bt.ctr) HIP_TRY(counters_clear(e, c, st));
        bt.poisoned = false;
    }
    if (n_frames == 0) {
        if (o.total) HIP_TRY(hipMemsetAsync(o.total, 0, 8, st));
        if (o.status) HIP_TRY(hipMemsetAsync(o.status, 0, 4, st));
        return M1V_OK;
    }
    const Geometry &g = e->g;
    const Plan &p = e->plan;
    if (!bt.scratch || !bt.seg || (p.producer == Producer::dense && !bt.run_meta))
        return fail(M1V_E_HIP, "the encoder has no scratch (an earlier allocation failed)%s");
    // the counters this batch adds to, and the set the next batch of this Batch will use (k_assemble clears it)
    m1v_encoder::Counters &cur = bt.ctr[bt.turn & 1u], &nxt = bt.ctr[(bt.turn + 1u) & 1u];
    bt.turn++;
    PoisonOnReturn poison{&bt.poisoned};
    if (fail_encode_at(1) != M1V_OK) return M1V_E_HIP;
    if (sel)
        if (const int rc = sel->launch(e, sel->args, cur, n_frames, st)) return rc;
    const uint32_t *qsel = sel && !sel->own_quality ? e->d_qsel : e->d_qsel_own;
    // the plan's producer kernel over n_frames
    const size_t grid = (size_t)n_frames * p.units;
    int rc;
    if (p.producer == Producer::tiles) {
        TileArgs a;
        fill_tile_grid(e, d_rgb, n_frames, a);
        a.qsel = qsel;
        a.scratch = bt.scratch;
        a.seg = bt.seg;
        a.strip_ctr = cur.strip_ctr;
        a.frame_bytes = cur.frame_bytes;
        a.arena_next = cur.words + 2;
        a.slot_bytes = p.slot_bytes;
        a.arena_slots = p.arena_slots;
        a.arena_off = p.arena_off;
        a.status = cur.words;
        a.lds_words = p.image_words;
        a.run_cap = p.run_cap;
        a.luma_region = p.luma_region;
        a.chroma_region = p.chroma_region;
        a.stamps = e->d_stamps;
        rc = launch_tiles(e, e->narrow, a, grid, p.lds_bytes, st);
    } else if (p.producer == Producer::dense) {
        DenseArgs a;
        a.g = g;
        a.rgb = d_rgb;
        a.tab = e->d_tab;
        a.rq_all = e->d_rq_all;
        a.qsel = qsel;
        a.scratch = bt.scratch;
        a.run_meta = bt.run_meta;
        a.status = cur.words;
        a.n_frames = n_frames;
        a.threads = p.block;
        a.runs_per_frame = p.units;
        a.lds_words = p.image_words;
        a.run_cap = p.run_cap;
        a.slot_bytes = p.slot_bytes;
        a.arena_slots = p.arena_slots;
        a.arena_off = p.arena_off;
        a.arena_next = cur.words + 2;
        a.stamps = e->d_stamps;
        a.zero_iters = p.zero_iters;
        rc = launch_profiled(e, run_kernel(e, d_rgb), grid, p.block, &a, p.lds_bytes, st);
    } else {
        EncodeArgs a;
        a.g = g;
        a.rgb = d_rgb;
        a.tab = e->d_tab;
        a.rq_all = e->d_rq_all;
        a.qsel = qsel;
        a.scratch = bt.scratch;
        a.seg = bt.seg;
        a.strip_ctr = cur.strip_ctr;
        a.frame_bytes = cur.frame_bytes;
        a.status = cur.words;
        a.n_frames = n_frames;
        a.threads = p.block;
        a.lds_words = p.image_words;
        a.stamps = e->d_stamps;
        rc = launch_profiled(e, run_kernel(e, d_rgb), grid, p.block, &a, p.lds_bytes, st);
    }
    if (rc != M1V_OK) return rc;
    if (e->pipelined) { // the layout + gather stream waits for the producer
        HIP_TRY(hipEventRecord(bt.enc_done, st));
        HIP_TRY(hipStreamWaitEvent(gs, bt.enc_done, 0));
    }
    if (p.producer == Producer::dense) {
        DenseGeom d;
        d.n_frames = n_frames;
        d.n_strips = g.n_strips;
        d.bps = g.n_mbrows * 6;
        d.T = p.block;
        d.runs_per_frame = p.units;
        hipLaunchKernelGGL(k_dense_frame_layout, dim3(n_frames), dim3(256), 0, gs, d, p.segs, bt.run_meta, bt.seg, cur.strip_ctr,
                           cur.frame_bytes);
        HIP_TRY(hipGetLastError());
    }
    if (fail_encode_at(2) != M1V_OK) return M1V_E_HIP;
    if (probe) {
        // ---- record sizes and status only, with k_assemble's counter hand-over ----
        SizesArgs sa;
        sa.n_frames = n_frames;
        sa.n_strips = g.n_strips;
        sa.frame_bytes = cur.frame_bytes;
        sa.enc_words = cur.words;
        if (const int rc = hand_over(sa, cur, nxt, n_frames, g.n_strips, gs)) return rc;
        sa.out_sizes = (unsigned long long *)o.frame_sizes;
        sa.out_status = o.status ? o.status : cur.words + 1;
        hipLaunchKernelGGL(k_frame_sizes, dim3((unsigned)n_frames), dim3(256), 0, gs, sa);
        HIP_TRY(hipGetLastError());
    } else {
        // ---- frame offsets, strip offsets, concatenation, headers, sizes, status: one launch (m1v_assemble.h) ----
        AssembleArgs ga;
        ga.n_frames = n_frames;
        ga.n_strips = g.n_strips;
        ga.segs = p.segs;
        ga.group = p.asm_group;
        ga.lanes_log2 = p.asm_lanes_log2;
        ga.img_words = kAsmImageBytes / 4;
        ga.div_segs = div_magic((uint32_t)p.segs, (unsigned long long)p.asm_group * (unsigned long long)p.segs);
        ga.scratch = bt.scratch;
        ga.seg = bt.seg;
        ga.strip_ctr = cur.strip_ctr;
        ga.frame_bytes = cur.frame_bytes;
        ga.enc_words = cur.words;
        if (const int rc = hand_over(ga, cur, nxt, n_frames, g.n_strips, gs)) return rc;
        ga.tab = e->d_tab;
        ga.out = o.out;
        ga.out_cap = o.cap;
        ga.out_sizes = (unsigned long long *)o.frame_sizes;
        ga.out_total = (unsigned long long *)o.total;
        ga.out_status = o.status ? o.status : cur.words + 1;
        ga.first_index = first_frame_index;
        ga.stamps = e->d_stamps;
        const dim3 grid((unsigned)((g.n_strips + p.asm_group - 1) / p.asm_group), (unsigned)n_frames);
        const size_t lds = (size_t)(kAsmImageBytes / 4 + kAsmFixedWords) * sizeof(uint32_t);
        if (p.scratch_bytes >= (1ull << 32))
            hipLaunchKernelGGL(k_assemble<true>, grid, dim3(kAsmThreads), lds, gs, ga);
        else
            hipLaunchKernelGGL(k_assemble<false>, grid, dim3(kAsmThreads), lds, gs, ga);
        HIP_TRY(hipGetLastError());
        if (sel && sel->finish)
            if (const int rc = sel->finish(e, sel->args, cur, o, n_frames, gs)) return rc;
    }
    if (fail_encode_at(3) != M1V_OK) return M1V_E_HIP;
    if (e->pipelined) {
        HIP_TRY(hipEventRecord(bt.gather_done, gs));
        bt.gather_pending = true;
    }
    poison.flag = nullptr;
    return M1V_OK;
}

// The fused size table (Plan::table_units): the size-table kernel of the layout in force (launch_tiles on the kSizeTable row of the
// registry: k_size_table_tiles for packed 3-channel input, k_size_table_rgba for 4 channels, one kernel family per layout kind
// beside them), then k_size_table_sizes, both on the caller's stream (no Batch, no scratch: in pipelined mode too).  qualities: 1..8, strictly increasing, each <= the encoder's quality (checked by the caller).
// sizes[k * stride + frame], status[k] (may be null).  Fail hooks: 1 before the probe kernel, 2 before the sizes kernel, 3 after.
// dist != null: the rd table (the k_rd_table_* kernels and k_rd_table_sizes in their places), dist[k * stride + frame] beside the sizes.
static int size_table_fused(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const uint8_t *qualities, int n_q,
                            unsigned long long *sizes, unsigned long long *dist, size_t stride, uint32_t *status, hipStream_t st) {
    if (const int rc = check_frame_table(e, d_rgb)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    m1v_encoder::TableCounters &tc = e->table;
    const Plan &p = e->plan;
    if (!tc.strip_ctr || !p.table_units) return fail(M1V_E_HIP, "the encoder has no size-table counters%s");
    if (tc.poisoned) { // the last call failed after its probe kernel may have added: clear every counter first
        HIP_TRY(table_clear(e, st));
        tc.poisoned = false;
    }
    if (n_frames == 0) return M1V_OK;
    PoisonOnReturn poison{&tc.poisoned};
    if (fail_encode_at(1) != M1V_OK) return M1V_E_HIP;
    TableArgs a;
    fill_tile_grid(e, d_rgb, n_frames, a);
    for (int k = 0; k < kMaxCandidates; k++) a.qoff[k] = k < n_q ? (uint32_t)(qualities[k] - 1) * 64u : 0u;
    a.n_q = n_q;
    a.strip_ctr = tc.strip_ctr;
    a.frame_bytes = tc.frame_bytes;
    a.status = tc.words;
    a.region = p.table_region;
    const bool narrow = qualities[n_q - 1] <= e->narrow_q;
    const size_t grid = (size_t)n_frames * p.table_units;
    if (dist) {
        RdTableArgs ra = {a, e->d_dq_all, tc.frame_dist};
        if (const int rc = launch_tiles(e, narrow, ra, grid, p.table_lds_bytes + kRdPartWords * 4, st)) return rc;
    } else if (const int rc = launch_tiles(e, narrow, a, grid, p.table_lds_bytes, st)) {
        return rc;
    }
    if (fail_encode_at(2) != M1V_OK) return M1V_E_HIP;
    TableSizesArgs sa;
    sa.n_frames = n_frames;
    sa.n_strips = e->g.n_strips;
    sa.strip_ctr = tc.strip_ctr;
    sa.frame_bytes = tc.frame_bytes;
    sa.status = tc.words;
    sa.out_sizes = sizes;
    sa.stride = stride;
    sa.out_status = status;
    if (dist) {
        const RdSizesArgs rs = {sa, tc.frame_dist, dist};
        hipLaunchKernelGGL(k_rd_table_sizes, dim3((unsigned)n_frames, (unsigned)n_q), dim3(256), 0, st, rs);
    } else {
        hipLaunchKernelGGL(k_size_table_sizes, dim3((unsigned)n_frames, (unsigned)n_q), dim3(256), 0, st, sa);
    }
    HIP_TRY(hipGetLastError());
    if (fail_encode_at(3) != M1V_OK) return M1V_E_HIP;
    poison.flag = nullptr;
    return M1V_OK;
}

// the C-ABI: object lifetime, buffers, the entry points, delivery, the host path, profiling, debug hooks
#include "m1v_runtime.h"

// ec504_imageencoder_amd/csrc/m1v_downscale_words.h — the tile kernels on 2:1 downscaled renditions of YCbCr frames with 16-bit
// samples (m1v_set_downscale_word_layout): the encoder has the rendition's size W x H, the frames are true 4:2:0 sources of
// 2 W x 2 H luma words and W x H words per chroma component (P010 / P012 / P016, yuv420p10le / 12le / 16le, pitched windows of
// them included), every sample a 16-bit little-endian word, and the picture that is coded is the 2 x 2 box average of each plane,
// taken at the full word precision and then shifted down to a byte.  Not a standalone header: included by m1v_kernels.hip behind
// m1v_downscale_planes.h.  The workgroup, bit stage, scratch slots, segment table and counters are those of m1v_tiles.h (the
// kernel bodies are the same headers); only the front half is new.
//
// The bytes.  Frame f starts at F = base + f * frame_stride.
//     source luma word (X, Y)              F + y_off + Y * y_pitch + 2 X
//     source word (U, V) of chroma plane p F + p_off + V * c_pitch + U * CSTEP          CSTEP = c_step = 2 or 4
// The rendition's luma sample (x, y) is
//     a = (w(2x, 2y) + w(2x + 1, 2y) + w(2x, 2y + 1) + w(2x + 1, 2y + 1) + 2) >> 2        w: the source words of that plane
//     sample = min(a >> shift, 255)                                                       shift = 0 .. 8, uniform
// and sample (u, v) of chroma plane p, u < W / 2, v < H / 2, is the same expression over that plane's source words: a is an exact
// integer, half rounded up, the shift truncates, a box filter per plane without a chroma-siting correction.  The record is the one
// k_encode_planes gives for the tightly packed I420 frame of those samples: 256 + sample as fp32, fdct_row_f<float, false>,
// default rounding mode, no colour conversion and no fp64.
//
// Front half (HalfWordFront<CSTEP>::run).  The lanes own the blocks they own in k_encode_tiles and HalfPlaneFront:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]
// A lane's block row is 8 neighbouring rendition samples = 16 source words in each of two source rows:
//     luma, chroma CSTEP 2   32 contiguous bytes per source row   2 x global_load_dwordx4   16 VGPRs for both source rows
//     chroma CSTEP 4         64 bytes per source row, every other halfword the lane's component   4 x global_load_dwordx4
// The loads are of a type declared aligned(1) (QuadAlign1): any byte alignment of base, offsets, pitches and stride is taken.
// Per dword w of a 32-byte unit, (w & 0xffff) + (w >> 16) is the horizontal pair sum of one rendition sample (at most 2 * 65535,
// 17 bits); per pair of neighbouring dwords of a 64-byte unit, the chosen halfword of each ((w >> phase) & 0xffff, phase 0 or 16)
// adds to the same.  Nothing is packed: every pair sum and every 2 x 2 sum (at most 4 * 65535 + 2 < 2^18) has a 32-bit register
// of its own, so no carry can reach a neighbour.  The upper source row is summed into 8 registers as it is used and the lower row
// adds to them (as in DownscaleFront), then + 2, >> 2, >> shift, min(.., 255).  Both source rows of block row i + 1 are requested
// before row i goes through the DCT; the samples of row i are operands of the empty asm in front of that request (settle, as in
// m1v_downscale_planes.h), so that the compiler does not keep the raw words of two block rows alive: with CSTEP 4 one block
// row's raw words are 32 VGPRs.  No LDS is used in front of the staging: plan_for's regions stay as they are.  The compiler
// counts vmcnt for these loads (plain C++ loads); what the caller requested first (the wave's VLC table, LDS-DMA) is older in the
// queue than every row, and the front half ends on vmcnt(0), so the table has landed when it returns, as behind HalfPlaneFront.
//
// Read contract (include/mpeg1_hip.h): of frame f only bytes of [F, F + E) rounded up to the next 4-byte boundary are read (the
// header allows the rounding, counted from F; these kernels read nothing behind F + E), E = the source's extent: the largest
// offset + (rows - 1) * pitch + row bytes over the three planes with rows = 2 ye (luma) and ye (chroma), row bytes = 4 xe (luma)
// and (xe - 1) * CSTEP + 2 (chroma), xe x ye = 16 n_strips x 16 n_mbrows the coded region in rendition samples.  Unaddressed
// bytes inside that range may be read and never influence the output.  Proof.
//     luma wave     y = 16 mb + 8 (block row) + i with mb = min(m0 + .., n_mbrows - 1), so 2y + 1 <= 2 ye - 1;
//                   x = 16 (s0 + min(strip, strips_here - 1)) + 8 (left|right), so x + 8 <= 16 n_strips = xe and the unit's 32
//                   bytes [4x, 4x + 32) end at 4 (x + 8) <= 4 xe <= 4 W: 32 addressed bytes, no luma unit overhangs its row
//     chroma wave   v = 8 mb + i <= ye / 2 - 1, so 2v + 1 <= ye - 1; u = 8 (s0 + min(strip, strips_here - 1)), so
//                   u + 8 <= 8 n_strips = xe / 2
//         CSTEP 2   the unit's 32 bytes [4u, 4u + 32) end at 4 (u + 8) <= 4 * 8 * n_strips = 2 xe = (xe - 1) * 2 + 2: 32 addressed
//                   bytes, no overhang
//         CSTEP 4   the unit's 64 bytes start at o = p_off + V * c_pitch + 8u; its addressed bytes are the words at o, o + 4, ..
//                   o + 60, the last of them the row's word (xe - 1) at most, which ends at (xe - 1) * 4 + 2, so o + 62 <= E.
//                   The last two bytes, o + 62 and o + 63, belong to the other component or to nobody: for the component that
//                   comes second in a pair they lie behind the row, and in the last chroma row of a tightly packed P010 frame
//                   that is two bytes past E.
// `lim` = E - 64 is the last offset a 64-byte unit may start at.  A unit at o > lim is fetched two bytes earlier and the other
// halfword phase is picked (the high half of each dword): its addressed bytes end at o + 62 <= E, so the 64 bytes from o - 2 end
// with the extent at the latest, and o - 2 >= lim - 1 >= 0 starts inside it.  A unit at o <= lim ends at o + 64 <= E.  The fetch
// and the pick are decided by the same comparison of the same offset, per source row (the HalfPlaneFront rule with 64-byte
// units).  lim >= 1 needs E >= 65; the smallest frame, a 16 x 16 rendition, addresses 32 luma rows of 64 bytes: E >= 2048,
// lim >= 1984.  Lanes outside the picture (last tile column / row) repeat the last strip's / macroblock row's unit, as in
// m1v_tiles.h.  The largest byte offset inside a frame is below E < 2^32 (the setter), so 32-bit offsets do not wrap.

struct HalfWordFrontArgs {
    uint32_t y_off, cb_off, cr_off; // bytes from the frame's base to word (0, 0) of each SOURCE plane
    uint32_t y_pitch, c_pitch;      // bytes between source luma rows / source chroma rows
    uint32_t lim;                   // the last offset at which a 64-byte unit may start (see the read contract above)
    uint32_t shift;                 // 0 .. 8: the average's bits that are dropped below the sample
};

template <int CSTEP>
struct HalfWordFront {
    static_assert(CSTEP == 2 || CSTEP == 4, "one plane per chroma component, or interleaved word pairs");
    HalfWordFrontArgs p;
    static constexpr int kQuads = CSTEP; // 16-byte loads of the widest unit of one source row

    struct Raw { uint32_t w[2][4 * kQuads]; }; // [upper | lower source row]

    __device__ __forceinline__ static void load16(const uint8_t *src, uint32_t *w) {
        const QuadAlign1 v = *reinterpret_cast<const QuadAlign1 *>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    // The loads that follow stay behind the arithmetic that gave these values: the next block row is not requested while this one
    // still occupies its registers
    __device__ __forceinline__ static void settle(uint32_t (&b)[8]) {
        asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]) : : "memory");
    }

    // The template parameters and arguments of HalfPlaneFront::run
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the downscaled word kernels stay in the default rounding mode");
        (void)comp;
        (void)ring;
        const bool chroma = wave == 2;
        const bool wide = CSTEP == 4 && chroma; // 64-byte units (wave-uniform)
        const uint32_t L = (uint32_t)lane;
        // ---- the lane's unit of the upper source row of row 0 of its block: byte offset inside the frame (the proof above;
        //      rendition row y is source rows 2y and 2y + 1, rendition sample x starts at source word 2x) ----
        const uint32_t last_strip = (uint32_t)strips_here - 1u;
        const uint32_t pitch = chroma ? p.c_pitch : p.y_pitch;
        uint32_t unit0;
        if (!chroma) {
            const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(L >> 5), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min((L >> 1) & 7u, last_strip)) * 16u + (L & 1u) * 8u;
            unit0 = p.y_off + (mb * 16u + ((L >> 4) & 1u) * 8u) * 2u * pitch + x * 4u;
        } else {
            const uint32_t mb = (uint32_t)min(m0 + (int)((L >> 3) & 3u), g.n_mbrows - 1);
            const uint32_t u = ((uint32_t)s0 + min(L & 7u, last_strip)) * 8u;
            unit0 = (L >= 32u ? p.cr_off : p.cb_off) + mb * 8u * 2u * pitch + u * (2u * CSTEP);
        }
        // Both source rows of block row i; a 64-byte unit beyond `lim` starts two bytes earlier (the same comparison picks the
        // halfword phase in `average`)
        auto load_row = [&](int i, Raw &raw) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint32_t off = unit0 + (uint32_t)(2 * i + r) * pitch;
                if (wide) off -= off > p.lim ? 2u : 0u;
                load16(fbase + off, raw.w[r]);
                load16(fbase + off + 16u, raw.w[r] + 4);
                if constexpr (CSTEP == 4) if (wide) {
                    load16(fbase + off + 32u, raw.w[r] + 8);
                    load16(fbase + off + 48u, raw.w[r] + 12);
                }
            }
        };
        // the 8 rendition samples of block row i, one per register
        auto average = [&](int i, const Raw &raw, uint32_t (&b)[8]) {
            if (!wide) {
#pragma unroll
                for (int k = 0; k < 8; k++) b[k] = (raw.w[0][k] & 0xffffu) + (raw.w[0][k] >> 16); // at most 2 * 65535
#pragma unroll
                for (int k = 0; k < 8; k++) b[k] += (raw.w[1][k] & 0xffffu) + (raw.w[1][k] >> 16); // at most 4 * 65535
            } else if constexpr (CSTEP == 4) {
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const uint32_t phase = unit0 + (uint32_t)(2 * i + r) * pitch > p.lim ? 16u : 0u;
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const uint32_t pair = ((raw.w[r][2 * k] >> phase) & 0xffffu) + ((raw.w[r][2 * k + 1] >> phase) & 0xffffu);
                        b[k] = r == 0 ? pair : b[k] + pair;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) b[k] = min(((b[k] + 2u) >> 2) >> p.shift, 255u);
        };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then both source rows of row 0; the caller's
        //      other prologue work runs while they travel ----
        first();
        Raw raw;
        load_row(0, raw);
        meanwhile();

#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t b[8];
            average(i, raw, b);
            settle(b);
            if (i + 1 < 8) load_row(i + 1, raw); // travels while row i goes through the DCT
            asm volatile("" ::: "memory");
            // the sample is the raw pixel: kPxBiasF + value, the input of the fp32 FDCT (as in HalfPlaneFront)
            float px[8];
#pragma unroll
            for (int k = 0; k < 8; k++) px[k] = m1vf::kPxBiasF + (float)b[k];
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
        wait_vm<0>(); // the caller's first() has landed (it is older than every row; the compiler does not count LDS-DMA)
    }
};

// The layout travels in the kernels' own argument structs, which wrap the bases' (as HalfPlaneArgs): Geometry stays as it is.
struct HalfWordArgs {
    TileArgs t;
    HalfWordFrontArgs pl;
    unsigned long long frame_stride; // bytes from a source frame's base to the next frame's
};
struct HalfWordTableArgs {
    TableArgs t;
    HalfWordFrontArgs pl;
    unsigned long long frame_stride;
};
struct HalfWordRdArgs {
    RdTableArgs t;
    HalfWordFrontArgs pl;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_HALF_WORD_INPUT                                                                        \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const HalfWordFront<CSTEP> half_word_front = {pa.pl}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF half_word_front.template run

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void k_half_words_encode(HalfWordArgs pa) {
    M1V_HALF_WORD_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

// (the table kernels are not pinned to five waves per SIMD as those of m1v_downscale_planes.h are: left alone they take 95 VGPRs
// with CSTEP 2, which is five waves as it stands, and 100 - 108 with CSTEP 4, four waves; pinned, the CSTEP 4 kernels take 96 and
// 20 bytes of scratch, the 32 raw registers of an interleaved block row being what does not fit.  The encode kernels take 85 - 91
// and 94 - 101.  What the fifth wave would be worth in time is not measured)
template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void k_half_words_size_table(HalfWordTableArgs pa) {
    M1V_HALF_WORD_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void k_half_words_rd_table(HalfWordRdArgs pa) {
    M1V_HALF_WORD_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

// m1v_downscale_words_to_i420_device: the samples the kernels above code, as tightly packed I420, uint8 [n][W * H * 3 / 2].
// Elementwise: a thread averages one rendition sample from its four source words and stores its byte; grid = (samples of a
// rendition frame, frames).  The chroma step and the shift are run-time values.  Reads addressed bytes only (byte loads: the
// words lie at any address).
struct HalfWordBytesArgs {
    const uint8_t *src;
    uint8_t *dst;
    HalfWordFrontArgs pl;
    unsigned long long frame_stride;
    uint32_t width, height, c_step; // the rendition's width and height
};

__global__ __launch_bounds__(256) void k_half_words_to_i420(HalfWordBytesArgs a) {
    const uint32_t luma = a.width * a.height, quarter = luma / 4u, half_w = a.width / 2u;
    const uint32_t sample = blockIdx.x * 256u + threadIdx.x;
    if (sample >= luma + 2u * quarter) return;
    uint32_t off, pitch, step;
    if (sample < luma) {
        const uint32_t y = sample / a.width, x = sample - y * a.width;
        off = a.pl.y_off + 2u * y * a.pl.y_pitch + 4u * x;
        pitch = a.pl.y_pitch;
        step = 2u;
    } else {
        const uint32_t c = sample - luma, second = c >= quarter ? 1u : 0u, at = c - second * quarter;
        const uint32_t v = at / half_w, u = at - v * half_w;
        off = (second ? a.pl.cr_off : a.pl.cb_off) + 2u * v * a.pl.c_pitch + 2u * u * a.c_step;
        pitch = a.pl.c_pitch;
        step = a.c_step;
    }
    const uint8_t *s = a.src + (unsigned long long)blockIdx.y * a.frame_stride + off;
    const uint8_t *t = s + pitch; // the lower source row
    auto word = [](const uint8_t *q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8; };
    const uint32_t sum = word(s) + word(s + step) + word(t) + word(t + step);
    a.dst[(unsigned long long)blockIdx.y * (luma + 2u * quarter) + sample] = (uint8_t)min(((sum + 2u) >> 2) >> a.pl.shift, 255u);
}

// ec504_imageencoder_amd/csrc/m1v_downscale_planes.h — the tile kernels on 2:1 downscaled renditions of planar and semi-planar
// YCbCr frames (m1v_set_downscale_plane_layout): the encoder has the rendition's size W x H, the frames are true 4:2:0 sources of
// 2 W x 2 H luma samples and W x H samples per chroma component (I420, YV12, NV12, NV21, pitched windows of them included), and the
// picture that is coded is the 2 x 2 box average of each plane.  Not a standalone header: included by m1v_kernels.hip behind
// m1v_downscale.h.  The workgroup, bit stage, scratch slots, segment table and counters are those of m1v_tiles.h (the kernel
// bodies are the same headers); only the front half is new.
//
// The bytes.  Frame f starts at F = base + f * frame_stride.
//     source luma sample (X, Y)              F + y_off + Y * y_pitch + X
//     source sample (U, V) of chroma plane p F + p_off + V * c_pitch + U * CSTEP          CSTEP = c_step = 1 or 2
// The rendition's luma sample (x, y) is
//     (s(2x, 2y) + s(2x + 1, 2y) + s(2x, 2y + 1) + s(2x + 1, 2y + 1) + 2) >> 2          s: the source samples of that plane
// and sample (u, v) of chroma plane p, u < W / 2, v < H / 2, is the same expression over that plane's source samples: an exact
// integer, half rounded up, a box filter per plane without a chroma-siting correction.  The record is the one k_encode_planes
// gives for the tightly packed I420 frame of those samples: 256 + sample as fp32, fdct_row_f<float, false>, default rounding mode,
// no colour conversion and no fp64.
//
// Front half (HalfPlaneFront<CSTEP>::run).  The lanes own the blocks they own in k_encode_tiles and PlaneFront:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]
// A lane's block row is 8 neighbouring rendition samples = 16 source samples in each of two source rows:
//     luma, chroma CSTEP 1   16 contiguous bytes per source row   1 x global_load_dwordx4   8 VGPRs for both source rows
//     chroma CSTEP 2         32 bytes per source row, every other one the lane's component   2 x global_load_dwordx4   16 VGPRs
// The loads are of a type declared aligned(1) (QuadAlign1): any byte alignment of base, offsets, pitches and stride is taken.
// Per dword w of a 16-byte unit, (w & 0x00ff00ff) + ((w >> 8) & 0x00ff00ff) is the two horizontal pair sums as 16-bit halves; the
// two source rows add, then + 0x00020002, >> 2, & 0x00ff00ff: a half holds at most 4 * 255 + 2 = 1022, so no carry crosses.  Per
// dword w of a 32-byte unit, t = w & 0x00ff00ff (or (w >> 8) & 0x00ff00ff for the other byte phase) holds the component's two
// samples and (t + (t >> 16)) & 0xffff is their sum.  Both source rows of block row i + 1 are requested before row i goes
// through the DCT; the averaged bytes of row i are operands of the empty asm in front of that request (settle, as in
// m1v_downscale.h), so that the compiler does not keep the raw bytes of two block rows alive.  No LDS is used in front of the
// staging: plan_for's regions stay as they are.  The compiler counts vmcnt for these loads (plain C++ loads); what the caller
// requested first (the wave's VLC table, LDS-DMA) is older in the queue than every row, and the front half ends on vmcnt(0), so
// the table has landed when it returns, as behind DownscaleFront.
//
// Read contract (include/mpeg1_hip.h): of frame f only bytes of [F, F + E) rounded up to the next 4-byte boundary are read (the
// header allows the rounding, counted from F; these kernels read nothing behind F + E), E = the source's extent: the largest offset + (rows - 1) * pitch + row bytes over the three planes with rows = 2 ye (luma) and ye
// (chroma), row bytes = 2 xe (luma) and (xe - 1) * CSTEP + 1 (chroma), xe x ye = 16 n_strips x 16 n_mbrows the coded region in
// rendition samples.  Unaddressed bytes inside that range may be read and never influence the output.  Proof.
//     luma wave     y = 16 mb + 8 (block row) + i with mb = min(m0 + .., n_mbrows - 1), so 2y + 1 <= 2 ye - 1;
//                   x = 16 (s0 + min(strip, strips_here - 1)) + 8 (left|right), so x + 8 <= 16 n_strips = xe and the unit's 16
//                   bytes [2x, 2x + 16) end at 2 (x + 8) <= 2 xe <= 2 W: 16 addressed bytes, no luma unit overhangs its row
//     chroma wave   v = 8 mb + i <= ye / 2 - 1, so 2v + 1 <= ye - 1; u = 8 (s0 + min(strip, strips_here - 1)), so
//                   u + 8 <= 8 n_strips = xe / 2
//         CSTEP 1   the unit's 16 bytes [2u, 2u + 16) end at 2 (u + 8) <= 2 * 8 * n_strips = xe <= W: 16 addressed bytes, no
//                   overhang
//         CSTEP 2   the unit's 32 bytes start at o = p_off + V * c_pitch + 4u; its addressed bytes are o, o + 2, .. o + 30, the
//                   last of them the row's (xe - 1) * 2 + 1st byte at most, so o + 31 <= E.  The 32nd byte, o + 31, belongs to
//                   the other component or to nobody: for the component that comes second in a pair it lies one byte behind the
//                   row, and in the last chroma row of a tightly packed NV12 frame that is one byte past E.
// `lim` = E - 32 is the last offset a 32-byte unit may start at.  A unit at o > lim is fetched one byte earlier and the other
// byte phase is picked: its addressed bytes end at o + 31 <= E, so the 32 bytes from o - 1 end with the extent at the latest, and
// o - 1 >= lim >= 0 starts inside it.  A unit at o <= lim ends at o + 32 <= E.  The fetch and the pick are decided by the same
// comparison of the same offset, per source row (the PlaneFront rule with 32-byte units, without its rounding of E).  lim >= 0
// needs E >= 32; the smallest frame, a 16 x 16 rendition, addresses 32 luma rows of 32 bytes: E >= 1024, lim >= 992.
// Lanes outside the picture (last tile column / row) repeat the last strip's / macroblock row's unit, as in m1v_tiles.h.  The
// largest byte offset inside a frame is below E < 2^32 (the setter), so 32-bit offsets do not wrap.

struct HalfPlaneFrontArgs {
    uint32_t y_off, cb_off, cr_off; // bytes from the frame's base to sample (0, 0) of each SOURCE plane
    uint32_t y_pitch, c_pitch;      // bytes between source luma rows / source chroma rows
    uint32_t lim;                   // the last offset at which a 32-byte unit may start (see the read contract above)
};

template <int CSTEP>
struct HalfPlaneFront {
    static_assert(CSTEP == 1 || CSTEP == 2, "one plane per chroma component, or interleaved pairs");
    HalfPlaneFrontArgs p;
    static constexpr int kQuads = CSTEP; // 16-byte loads of the widest unit of one source row

    struct Raw { uint32_t w[2][4 * kQuads]; }; // [upper | lower source row]

    __device__ __forceinline__ static void load16(const uint8_t *src, uint32_t *w) {
        const QuadAlign1 v = *reinterpret_cast<const QuadAlign1 *>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    // The loads that follow stay behind the arithmetic that gave these values: the next block row is not requested while this one
    // still occupies its registers
    __device__ __forceinline__ static void settle(uint32_t (&b)[4]) {
        asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : : "memory");
    }

    // The template parameters and arguments of DownscaleFront::run
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the downscaled plane kernels stay in the default rounding mode");
        (void)comp;
        (void)ring;
        const bool chroma = wave == 2;
        const bool wide = CSTEP == 2 && chroma; // 32-byte units (wave-uniform)
        const uint32_t L = (uint32_t)lane;
        // ---- the lane's unit of the upper source row of row 0 of its block: byte offset inside the frame (the proof above;
        //      rendition row y is source rows 2y and 2y + 1, rendition sample x starts at source sample 2x) ----
        const uint32_t last_strip = (uint32_t)strips_here - 1u;
        const uint32_t pitch = chroma ? p.c_pitch : p.y_pitch;
        uint32_t unit0;
        if (!chroma) {
            const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(L >> 5), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min((L >> 1) & 7u, last_strip)) * 16u + (L & 1u) * 8u;
            unit0 = p.y_off + (mb * 16u + ((L >> 4) & 1u) * 8u) * 2u * pitch + x * 2u;
        } else {
            const uint32_t mb = (uint32_t)min(m0 + (int)((L >> 3) & 3u), g.n_mbrows - 1);
            const uint32_t u = ((uint32_t)s0 + min(L & 7u, last_strip)) * 8u;
            unit0 = (L >= 32u ? p.cr_off : p.cb_off) + mb * 8u * 2u * pitch + u * (2u * CSTEP);
        }
        // Both source rows of block row i; a 32-byte unit beyond `lim` starts one byte earlier (the same comparison picks the
        // byte phase in `average`)
        auto load_row = [&](int i, Raw &raw) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint32_t off = unit0 + (uint32_t)(2 * i + r) * pitch;
                if (wide) off -= off > p.lim ? 1u : 0u;
                load16(fbase + off, raw.w[r]);
                if constexpr (CSTEP == 2) if (wide) load16(fbase + off + 16u, raw.w[r] + 4);
            }
        };
        // the 8 rendition samples of block row i: b[k] = sample 2k | sample 2k + 1 << 16
        auto average = [&](int i, const Raw &raw, uint32_t (&b)[4]) {
            if (!wide) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t a = raw.w[0][k], c = raw.w[1][k];
                    const uint32_t sum = (a & 0x00ff00ffu) + ((a >> 8) & 0x00ff00ffu) + (c & 0x00ff00ffu) + ((c >> 8) & 0x00ff00ffu);
                    b[k] = ((sum + 0x00020002u) >> 2) & 0x00ff00ffu;
                }
            } else if constexpr (CSTEP == 2) {
                uint32_t shift[2];
#pragma unroll
                for (int r = 0; r < 2; r++) shift[r] = unit0 + (uint32_t)(2 * i + r) * pitch > p.lim ? 8u : 0u;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    uint32_t s[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const uint32_t ta = (raw.w[0][2 * k + h] >> shift[0]) & 0x00ff00ffu;
                        const uint32_t tc = (raw.w[1][2 * k + h] >> shift[1]) & 0x00ff00ffu;
                        s[h] = (ta + (ta >> 16) + tc + (tc >> 16)) & 0xffffu; // at most 1020
                    }
                    b[k] = (((s[0] | s[1] << 16) + 0x00020002u) >> 2) & 0x00ff00ffu;
                }
            }
        };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then both source rows of row 0; the caller's
        //      other prologue work runs while they travel ----
        first();
        Raw raw;
        load_row(0, raw);
        meanwhile();

#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t b[4];
            average(i, raw, b);
            settle(b);
            if (i + 1 < 8) load_row(i + 1, raw); // travels while row i goes through the DCT
            asm volatile("" ::: "memory");
            // the byte is the raw pixel: kPxBiasF + value, the input of the fp32 FDCT (as in PlaneFront)
            float px[8];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                px[2 * k] = m1vf::kPxBiasF + (float)(b[k] & 0xffu);
                px[2 * k + 1] = m1vf::kPxBiasF + (float)(b[k] >> 16);
            }
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
        wait_vm<0>(); // the caller's first() has landed (it is older than every row; the compiler does not count LDS-DMA)
    }
};

// The layout travels in the kernels' own argument structs, which wrap the bases' (as DownscaleArgs): Geometry stays as it is.
struct HalfPlaneArgs {
    TileArgs t;
    HalfPlaneFrontArgs pl;
    unsigned long long frame_stride; // bytes from a source frame's base to the next frame's
};
struct HalfPlaneTableArgs {
    TableArgs t;
    HalfPlaneFrontArgs pl;
    unsigned long long frame_stride;
};
struct HalfPlaneRdArgs {
    RdTableArgs t;
    HalfPlaneFrontArgs pl;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_HALF_PLANE_INPUT                                                                       \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const HalfPlaneFront<CSTEP> half_plane_front = {pa.pl}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF half_plane_front.template run

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void k_half_planes_encode(HalfPlaneArgs pa) {
    M1V_HALF_PLANE_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

// (the table kernels are pinned to five waves per SIMD as k_encode_planes is: left alone the allocator gives them 96 - 99 VGPRs,
// which with CSTEP 1 misses five waves by one to three registers; pinned they take 91 - 95, without scratch.  The encode kernel
// takes 55 - 76 unpinned)
template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_half_planes_size_table(HalfPlaneTableArgs pa) {
    M1V_HALF_PLANE_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_half_planes_rd_table(HalfPlaneRdArgs pa) {
    M1V_HALF_PLANE_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

// m1v_downscale_planes_to_i420_device: the samples the kernels above code, as tightly packed I420, uint8 [n][W * H * 3 / 2].
// Elementwise: a thread averages one rendition sample from its four source samples and stores its byte; grid = (samples of a
// rendition frame, frames).  The chroma step is a run-time value.  Reads addressed bytes only.
struct HalfPlaneBytesArgs {
    const uint8_t *src;
    uint8_t *dst;
    HalfPlaneFrontArgs pl;
    unsigned long long frame_stride;
    uint32_t width, height, c_step; // the rendition's width and height
};

__global__ __launch_bounds__(256) void k_half_planes_to_i420(HalfPlaneBytesArgs a) {
    const uint32_t luma = a.width * a.height, quarter = luma / 4u, half_w = a.width / 2u;
    const uint32_t sample = blockIdx.x * 256u + threadIdx.x;
    if (sample >= luma + 2u * quarter) return;
    uint32_t off, pitch, step;
    if (sample < luma) {
        const uint32_t y = sample / a.width, x = sample - y * a.width;
        off = a.pl.y_off + 2u * y * a.pl.y_pitch + 2u * x;
        pitch = a.pl.y_pitch;
        step = 1u;
    } else {
        const uint32_t c = sample - luma, second = c >= quarter ? 1u : 0u, at = c - second * quarter;
        const uint32_t v = at / half_w, u = at - v * half_w;
        off = (second ? a.pl.cr_off : a.pl.cb_off) + 2u * v * a.pl.c_pitch + 2u * u * a.c_step;
        pitch = a.pl.c_pitch;
        step = a.c_step;
    }
    const uint8_t *s = a.src + (unsigned long long)blockIdx.y * a.frame_stride + off;
    const uint8_t *t = s + pitch; // the lower source row
    a.dst[(unsigned long long)blockIdx.y * (luma + 2u * quarter) + sample] = (uint8_t)(((uint32_t)s[0] + s[step] + t[0] + t[step] + 2u) >> 2);
}

// ec504_imageencoder_amd/csrc/m1v_float_pixels.h — the tile kernels on frames whose R, G and B samples are floats interleaved per
// pixel (m1v_set_float_pixel_layout): [n, H, W, 3] and [n, H, W, 4] tensors of fp16, bf16 or fp32, channels-last model outputs,
// RGBA16F / RGBA32F render targets, pitched windows of them.  Not a standalone header: included by m1v_kernels.hip behind
// m1v_float_planes.h, whose sample types and conversion (float_sample_to_byte) it uses.  The workgroup, bit stage, scratch slots,
// segment table and counters are those of m1v_tiles.h (the kernel bodies are the same headers); only the front half is new.
//
// The samples.  Frame f starts at F = base + f * frame_stride; sample i (0, 1, 2) of pixel (x, y) is the S bytes at
//     F + y * row_pitch + x * P + i * S          P = pixel_step = C * S, C = 3 or 4 samples per pixel
// Samples 0, 1, 2 are R, G, B (M1V_ORDER_RGB) or B, G, R (M1V_ORDER_BGR); a 4th sample is skipped.  The byte of a sample is
// float_sample_to_byte, and the record is the one k_encode_tiles gives for the interleaved picture of those bytes:
// convert_row_planes on RowPlanes, fdct_row_f<float, false>, default rounding mode.
//
// Front half (FloatPixelFront<T, C>::run).  The lanes own the blocks they own in k_encode_tiles.  A lane's block row is 8
// neighbouring pixels = one contiguous run of 8 * P bytes, loaded straight into registers one row ahead of the row it converts:
//     S = 2, C = 3    48 bytes   3 x global_load_dwordx4    12 VGPRs
//     S = 2, C = 4    64 bytes   4 x global_load_dwordx4    16 VGPRs   (the 4th samples travel and are dropped)
//     S = 4, C = 3    96 bytes   6 x global_load_dwordx4    24 VGPRs
//     S = 4, C = 4   128 bytes   8 x global_load_dwordx3    24 VGPRs   (12 bytes per pixel: the 4th sample is never loaded, so a
//                                                                       row in flight stays within the 24 VGPRs of the budget)
// The samples become packed bytes of RowPlanes as they arrive, so only one row of raw samples is ever held.  The order costs no
// instantiation: the R and B dwords of RowPlanes are swapped after packing when the layout says B, G, R (a uniform select).  No
// LDS is used in front of the staging: plan_for's regions stay as they are.  Rejected: an LDS transpose of whole tile rows (the
// ring of RgbPlaneFront with a slot of 16 * 8 * P bytes per strip takes the CU from six workgroups to four or fewer, as for the
// float planes), and 16-byte loads with a shuffle between lanes for fp32 RGBA (a lane's 128 bytes would then be 32 VGPRs in flight,
// or a cross-lane exchange per row that adds vector instructions to the front half).  The compiler counts vmcnt for these loads
// (plain C++ loads); what the caller requested first (the wave's VLC table, LDS-DMA) is older in the queue than every row, and the
// front half ends on vmcnt(0), so the table has landed when it returns, as behind FloatPlaneFront.
//
// Read contract (include/mpeg1_hip.h): of frame f only bytes of the rows [F + y * row_pitch, F + y * row_pitch + W * P), y in
// 0 .. H - 1, are read.  Proof.  A lane's load is the 8 pixels x .. x + 7 of picture row y, the bytes [x * P, (x + 8) * P) of that
// row (S = 4, C = 4: of each pixel only its first 12 bytes):
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]: y = 16 mb + 8 (block row) + i with mb = min(m0 + ..,
//                   n_mbrows - 1), so y <= 16 n_mbrows - 1 <= H - 1; x = 16 (s0 + min(strip, strips_here - 1)) + 8 (left|right), so
//                   x + 8 <= 16 n_strips <= W
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]: chroma row 8 mb + i of width W / 2 (the quirk, encoder.h:347-348) is the
//                   left (i even) or right (i odd) half of picture row y = 4 mb + (i >> 1) <= 4 n_mbrows - 1 <= H - 1;
//                   x = (i & 1) * W / 2 + 8 (s0 + min(strip, strips_here - 1)), so x + 8 <= W / 2 + 8 n_strips <= W
// so (x + 8) * P <= W * P: no load overhangs a row, and there is no limit to clamp at.  Lanes outside the picture (last tile
// column / row) repeat the last strip's / macroblock row's pixels, as in m1v_tiles.h.  The largest byte offset inside a frame is
// below (H - 1) * row_pitch + W * P < 2^32 (the setter), so 32-bit offsets do not wrap.  row_pitch and frame_stride are multiples
// of S (the setter) and d_rgb is (the calls), so every sample is naturally aligned; a row may start at any multiple of S, that is
// at any pixel of a larger surface, and the loads assume no more.

// 12 bytes of an fp32 pixel that starts at any multiple of 4
typedef uint32_t TripleAlign4 __attribute__((ext_vector_type(3), aligned(4)));

struct FloatPixelFrontArgs {
    uint32_t row_pitch; // bytes from a picture row to the next
    float scale;        // 255.0f (M1V_RANGE_UNIT) or 1.0f (M1V_RANGE_BYTE)
    uint32_t bgr;       // 0: samples 0, 1, 2 are R, G, B; 1: B, G, R
};

template <typename T, int C>
struct FloatPixelFront {
    static_assert(C == 3 || C == 4, "three or four samples per pixel");
    FloatPixelFrontArgs p;
    static constexpr int S = T::kBytes;
    static constexpr uint32_t P = (uint32_t)(C * S);          // bytes of a pixel
    static constexpr bool kSkip4th = S == 4 && C == 4;        // 12-byte loads per pixel
    static constexpr int kWords = kSkip4th ? 24 : 2 * C * S; // dwords of a lane's 8 pixels in registers

    typedef typename T::Quad Quad;
    struct Raw { uint32_t w[kWords]; };

    __device__ __forceinline__ static void load8(const uint8_t *src, Raw &raw) {
        if constexpr (kSkip4th) {
#pragma unroll
            for (int x = 0; x < 8; x++) {
                const TripleAlign4 v = *reinterpret_cast<const TripleAlign4 *>(src + 16 * x);
                raw.w[3 * x] = v.x; raw.w[3 * x + 1] = v.y; raw.w[3 * x + 2] = v.z;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kWords / 4; q++) {
                const Quad v = *reinterpret_cast<const Quad *>(src + 16 * q);
                raw.w[4 * q] = v.x; raw.w[4 * q + 1] = v.y; raw.w[4 * q + 2] = v.z; raw.w[4 * q + 3] = v.w;
            }
        }
    }
    // sample i of the 8 pixels as the two dwords of RowPlanes
    __device__ __forceinline__ void pack8(const Raw &raw, int i, uint32_t &lo, uint32_t &hi) const {
        uint32_t b[8];
#pragma unroll
        for (int x = 0; x < 8; x++) {
            uint32_t bits;
            if constexpr (S == 4) {
                bits = raw.w[(kSkip4th ? 3 : C) * x + i];
            } else {
                const int h = C * x + i; // the halfword
                bits = (raw.w[h >> 1] >> ((h & 1) * 16)) & 0xffffu;
            }
            b[x] = float_sample_to_byte<T>(bits, p.scale);
        }
        lo = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
        hi = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
    }

    // The template parameters and arguments of FloatPlaneFront::run
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the float pixel kernels stay in the default rounding mode");
        (void)comp;
        (void)ring;
        const bool chroma = wave == 2;
        const uint32_t L = (uint32_t)lane;
        // ---- the lane's 8 pixels of row 0 of its block: byte offset inside the frame (the proof above) ----
        const uint32_t last_strip = (uint32_t)strips_here - 1u;
        uint32_t in_frame;
        if (!chroma) {
            const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(L >> 5), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min((L >> 1) & 7u, last_strip)) * 16u + (L & 1u) * 8u;
            in_frame = (mb * 16u + ((L >> 4) & 1u) * 8u) * p.row_pitch + x * P;
        } else {
            const uint32_t mb = (uint32_t)min(m0 + (int)((L >> 3) & 3u), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min(L & 7u, last_strip)) * 8u;
            in_frame = mb * 4u * p.row_pitch + x * P;
        }
        // row i lies (i >> 1) * step2 + (i & 1) * step1 behind row 0 (uniform; i is a constant of the unrolled loop)
        const uint32_t step2 = chroma ? p.row_pitch : 2u * p.row_pitch, step1 = chroma ? (uint32_t)g.half_w * P : p.row_pitch;
        const uint8_t *row0 = fbase + in_frame;
        auto load_row = [&](int i, Raw &raw) { load8(row0 + ((size_t)(i >> 1) * step2 + (size_t)(i & 1) * step1), raw); };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then row 0; the caller's other prologue work
        //      runs while it travels ----
        first();
        Raw raw;
        load_row(0, raw);
        meanwhile();

        const CompCoefF kf = comp_coef_wave(!chroma, lane);
        const bool bgr = p.bgr != 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            RowPlanes v; // the row's bytes as they arrive; the registers of the raw samples then take row i + 1
            uint32_t s0lo, s0hi, s2lo, s2hi;
            pack8(raw, 0, s0lo, s0hi);
            pack8(raw, 1, v.d[2], v.d[3]);
            pack8(raw, 2, s2lo, s2hi);
            v.d[0] = bgr ? s2lo : s0lo;
            v.d[1] = bgr ? s2hi : s0hi;
            v.d[4] = bgr ? s0lo : s2lo;
            v.d[5] = bgr ? s0hi : s2hi;
            if (i + 1 < 8) load_row(i + 1, raw);
            asm volatile("" ::: "memory"); // the loads of row i + 1 stay in front of row i's arithmetic, those of row i + 2 behind
            float px[8];
            convert_row_planes(v, kf, px);
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
        wait_vm<0>(); // the caller's first() has landed (it is older than every row; the compiler does not count LDS-DMA)
    }
};

// The layout travels in the kernels' own argument structs (as FloatPlaneArgs): Geometry stays as it is.
struct FloatPixelArgs {
    TileArgs t;
    FloatPixelFrontArgs px;
    unsigned long long frame_stride; // bytes from a frame's base to the next frame's
};
struct FloatPixelTableArgs {
    TableArgs t;
    FloatPixelFrontArgs px;
    unsigned long long frame_stride;
};
struct FloatPixelRdArgs {
    RdTableArgs t;
    FloatPixelFrontArgs px;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_FLOAT_PIXELS_INPUT                                                                     \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const FloatPixelFront<T, C> float_pixel_front = {pa.px}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF float_pixel_front.template run

// (no amdgpu_waves_per_eu, as for the float planes: a row of raw samples in flight beside the row in work takes the kernels to
// four waves per SIMD)
template <bool STAGE8, int R, typename T, int C>
__global__ __launch_bounds__(kTileThreads) void k_float_pixels_encode(FloatPixelArgs pa) {
    M1V_FLOAT_PIXELS_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R, typename T, int C>
__global__ __launch_bounds__(kTileThreads) void k_float_pixels_size_table(FloatPixelTableArgs pa) {
    M1V_FLOAT_PIXELS_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, typename T, int C>
__global__ __launch_bounds__(kTileThreads) void k_float_pixels_rd_table(FloatPixelRdArgs pa) {
    M1V_FLOAT_PIXELS_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

// m1v_float_pixels_to_bytes_device: the bytes the kernels above code, as uint8 [n][H][W][3] in R, G, B order.  Elementwise: a
// thread converts the three colour samples of one pixel and stores their three bytes; grid = (pixels of a frame, frames).  The
// pixel step is a run-time value.  Reads addressed samples only: never a 4th sample.
struct FloatPixelBytesArgs {
    const uint8_t *src;
    uint8_t *dst;
    FloatPixelFrontArgs px;
    unsigned long long frame_stride;
    uint32_t width, height, pixel_step;
};

template <typename T>
__global__ __launch_bounds__(256) void k_float_pixels_to_bytes(FloatPixelBytesArgs a) {
    const uint32_t pixel = blockIdx.x * 256u + threadIdx.x;
    if (pixel >= a.width * a.height) return;
    const uint32_t y = pixel / a.width, x = pixel - y * a.width;
    const uint8_t *s = a.src + (unsigned long long)blockIdx.y * a.frame_stride + (y * a.px.row_pitch + x * a.pixel_step);
    uint32_t v[3];
    if constexpr (T::kBytes == 4) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(s);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else {
        const uint16_t *q = reinterpret_cast<const uint16_t *>(s);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    }
    const uint32_t first = a.px.bgr ? 2u : 0u;
    uint8_t *d = a.dst + ((unsigned long long)blockIdx.y * a.width * a.height + pixel) * 3u;
    d[0] = (uint8_t)float_sample_to_byte<T>(v[first], a.px.scale);
    d[1] = (uint8_t)float_sample_to_byte<T>(v[1], a.px.scale);
    d[2] = (uint8_t)float_sample_to_byte<T>(v[2 - first], a.px.scale);
}

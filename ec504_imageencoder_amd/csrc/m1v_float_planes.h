// ec504_imageencoder_amd/csrc/m1v_float_planes.h — the tile kernels on frames whose R, G and B samples are floats in three planes
// (m1v_set_float_plane_layout): NCHW tensors of fp16, bf16 or fp32 in any plane order, three planes of a 4-plane tensor, pitched
// windows.  Not a standalone header: included by m1v_kernels.hip behind m1v_rgb_planes.h.  The workgroup, bit stage, scratch slots,
// segment table and counters are those of m1v_tiles.h (the kernel bodies are the same headers); only the front half is new.
//
// The samples.  Frame f starts at F = base + f * frame_stride; component c of pixel (x, y) is the sample of S bytes at
//     F + c_off + y * row_pitch + x * S
// Its byte is float_sample_to_byte (the definition of include/mpeg1_hip.h, "Float plane layout"): the sample in fp32, one fp32
// multiplication by the scale, ties to even, NaN and negatives to 0, above 255 to 255.  The record is the one k_encode_rgb_planes
// gives for those bytes: convert_row_planes on RowPlanes, fdct_row_f<float, false>, default rounding mode.
//
// Front half (FloatPlaneFront<T>::run).  The lanes own the blocks they own in k_encode_tiles.  Direct loads, for all three types:
// a lane loads the 8 samples of its own block row of each plane into registers (S = 2: one global_load_dwordx4 per plane, 12
// VGPRs; S = 4: two per plane, 24 VGPRs), one row ahead of the row it converts; the samples become packed bytes as they arrive, so
// only one row of raw samples is ever held.  No LDS is used in front of the staging: plan_for's regions stay as they are.
// Rejected: the LDS-DMA ring of RgbPlaneFront with a slot of 3 * S / 2 KiB.  Two slots of 6 KiB at S = 4 take a workgroup to
// about 39 KiB and the CU from six workgroups to four, and either ring makes plan_for's regions depend on the layout in force;
// one fetch shape for the three types keeps one front half.  The compiler counts vmcnt for these loads (plain C++ loads); what the
// caller requested first (the wave's VLC table, LDS-DMA) is older in the queue than every row, and the front half ends on
// vmcnt(0), so the table has landed when it returns, as behind RgbPlaneFront.
//
// Read contract (include/mpeg1_hip.h): of frame f only bytes of the three ranges
//     [F + c_off, F + c_off + (H - 1) * row_pitch + W * S)
// are read, and of those only addressed samples.  Proof.  A load is the 8 samples x .. x + 7 of picture row y of one plane:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]: y = 16 mb + 8 (block row) + i with mb = min(m0 + ..,
//                   n_mbrows - 1), so y <= 16 n_mbrows - 1 <= H - 1; x = 16 (s0 + min(strip, strips_here - 1)) + 8 (left|right), so
//                   x + 7 <= 16 n_strips - 1 <= W - 1
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]: chroma row 8 mb + i of width W / 2 (the quirk, encoder.h:347-348) is the
//                   left (i even) or right (i odd) half of picture row y = 4 mb + (i >> 1) <= 4 n_mbrows - 1 <= H - 1;
//                   x = (i & 1) * W / 2 + 8 (s0 + min(strip, strips_here - 1)), so x + 7 <= W / 2 + 8 n_strips - 1 <= W - 1
// The 16 (S = 2) or 2 x 16 (S = 4) bytes of a load are exactly those 8 samples: no unit overhangs a half row as the uint8
// chroma unit does, and there is no limit to clamp at.  Lanes outside the picture (last tile column / row) repeat the last
// strip's / macroblock row's samples, as in m1v_tiles.h.  Offsets are multiples of S (the setter) and d_rgb is (the calls), so
// every sample is naturally aligned; a row may start at any multiple of S, and the loads assume no more.

// 16 bytes of a row that starts at any multiple of S
typedef uint32_t QuadAlign2 __attribute__((ext_vector_type(4), aligned(2)));
typedef uint32_t QuadAlign4 __attribute__((ext_vector_type(4), aligned(4)));
struct F16Sample { static constexpr int kBytes = 2; typedef QuadAlign2 Quad; };
struct Bf16Sample { static constexpr int kBytes = 2; typedef QuadAlign2 Quad; };
struct F32Sample { static constexpr int kBytes = 4; typedef QuadAlign4 Quad; };

// THE conversion (include/mpeg1_hip.h): bits = the sample's bit pattern in the low S bytes.  t = fp32(sample) * scale is one
// fp32 multiplication in the default rounding mode.  The clamp stands in front of the rounding, which gives the byte the
// definition names (0 and 255 are integers and the rounding is monotonic): v_med3_f32 returns the smallest of its operands that
// is not a NaN when one is (the ISA's definition: min3), so a NaN gives 0, as -inf, -0.0 and every negative value do.  c + 2^23
// is exact for no c but an integer: the default rounding mode rounds c to an integer, ties to even, into the sum's low mantissa
// bits.  Every denormal, flushed or not, gives 0.
template <typename T>
__device__ __forceinline__ uint32_t float_sample_to_byte(uint32_t bits, float scale) {
    float f;
    if constexpr (T::kBytes == 4) f = __uint_as_float(bits);
    else if constexpr (__is_same(T, Bf16Sample)) f = __uint_as_float(bits << 16);
    else f = (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
    const float t = f * scale;
    const float c = __builtin_amdgcn_fmed3f(t, 0.0f, 255.0f);
    return __float_as_uint(c + 8388608.0f) & 0xffu;
}

struct FloatPlaneFrontArgs {
    uint32_t r_off, g_off, b_off; // bytes from the frame's base to pixel (0, 0) of each plane
    uint32_t row_pitch;           // bytes from a picture row to the next, the same in the three planes
    float scale;                  // 255.0f (M1V_RANGE_UNIT) or 1.0f (M1V_RANGE_BYTE)
};

template <typename T>
struct FloatPlaneFront {
    FloatPlaneFrontArgs p;
    static constexpr int S = T::kBytes, kWords = 2 * S; // dwords of a lane's 8 samples of one plane

    typedef typename T::Quad Quad;
    struct Raw { uint32_t w[3][kWords]; };

    __device__ __forceinline__ static void load8(const uint8_t *src, uint32_t (&w)[kWords]) {
#pragma unroll
        for (int q = 0; q < kWords / 4; q++) {
            const Quad v = *reinterpret_cast<const Quad *>(src + 16 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    }
    // the 8 samples of a plane as the two dwords of RowPlanes
    __device__ __forceinline__ void pack8(const uint32_t (&w)[kWords], uint32_t &lo, uint32_t &hi) const {
        uint32_t b[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t bits = S == 4 ? w[j] : (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
            b[j] = float_sample_to_byte<T>(bits, p.scale);
        }
        lo = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
        hi = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
    }

    // The template parameters and arguments of RgbPlaneFront::run; the ring is not used (R does not apply either)
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the float plane kernels stay in the default rounding mode");
        (void)comp;
        (void)ring;
        const bool chroma = wave == 2;
        const uint32_t L = (uint32_t)lane;
        // ---- the lane's 8 samples of row 0 of its block: byte offset inside a plane (the proof above) ----
        const uint32_t last_strip = (uint32_t)strips_here - 1u;
        uint32_t in_plane;
        if (!chroma) {
            const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(L >> 5), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min((L >> 1) & 7u, last_strip)) * 16u + (L & 1u) * 8u;
            in_plane = (mb * 16u + ((L >> 4) & 1u) * 8u) * p.row_pitch + x * (uint32_t)S;
        } else {
            const uint32_t mb = (uint32_t)min(m0 + (int)((L >> 3) & 3u), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min(L & 7u, last_strip)) * 8u;
            in_plane = mb * 4u * p.row_pitch + x * (uint32_t)S;
        }
        // row i lies (i >> 1) * step2 + (i & 1) * step1 behind row 0 (uniform; i is a constant of the unrolled loop)
        const uint32_t step2 = chroma ? p.row_pitch : 2u * p.row_pitch, step1 = chroma ? (uint32_t)g.half_w * (uint32_t)S : p.row_pitch;
        auto load_row = [&](int i, Raw &raw) {
            const uint8_t *row = fbase + ((size_t)(i >> 1) * step2 + (size_t)(i & 1) * step1);
            load8(row + (p.r_off + in_plane), raw.w[0]);
            load8(row + (p.g_off + in_plane), raw.w[1]);
            load8(row + (p.b_off + in_plane), raw.w[2]);
        };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then row 0; the caller's other prologue work
        //      runs while it travels ----
        first();
        Raw raw;
        load_row(0, raw);
        meanwhile();

        const CompCoefF kf = comp_coef_wave(!chroma, lane);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            RowPlanes v; // the row's bytes as they arrive; the registers of the raw samples then take row i + 1
            pack8(raw.w[0], v.d[0], v.d[1]);
            pack8(raw.w[1], v.d[2], v.d[3]);
            pack8(raw.w[2], v.d[4], v.d[5]);
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

// The layout travels in the kernels' own argument structs (as RgbPlaneArgs): Geometry stays as it is.
struct FloatPlaneArgs {
    TileArgs t;
    FloatPlaneFrontArgs pl;
    unsigned long long frame_stride; // bytes from a frame's base to the next frame's
};
struct FloatPlaneTableArgs {
    TableArgs t;
    FloatPlaneFrontArgs pl;
    unsigned long long frame_stride;
};
struct FloatPlaneRdArgs {
    RdTableArgs t;
    FloatPlaneFrontArgs pl;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_FLOAT_PLANES_INPUT                                                                     \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const FloatPlaneFront<T> float_plane_front = {pa.pl}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF float_plane_front.template run

// (no amdgpu_waves_per_eu: a row of raw samples in flight beside the row in work does not fit the 96 registers of five waves per
// SIMD without scratch; the kernels take four)
template <bool STAGE8, int R, typename T>
__global__ __launch_bounds__(kTileThreads) void k_encode_float_planes(FloatPlaneArgs pa) {
    M1V_FLOAT_PLANES_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R, typename T>
__global__ __launch_bounds__(kTileThreads) void k_size_table_float_planes(FloatPlaneTableArgs pa) {
    M1V_FLOAT_PLANES_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, typename T>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_float_planes(FloatPlaneRdArgs pa) {
    M1V_FLOAT_PLANES_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

// m1v_float_planes_to_bytes_device: the bytes the kernels above code, as uint8 [n][3][H][W] in R, G, B order.  Elementwise: a
// thread converts two neighbouring samples of a row (the width is even) and stores their two bytes; grid = (pairs of a plane,
// frames, 3).  Reads addressed samples only.
struct FloatBytesArgs {
    const uint8_t *src;
    uint8_t *dst;
    FloatPlaneFrontArgs pl;
    unsigned long long frame_stride;
    uint32_t width, height;
};

template <typename T>
__global__ __launch_bounds__(256) void k_float_planes_to_bytes(FloatBytesArgs a) {
    const uint32_t half = a.width >> 1, pair = blockIdx.x * 256u + threadIdx.x;
    if (pair >= half * a.height) return;
    const uint32_t y = pair / half, x = 2u * (pair - y * half), c = blockIdx.z;
    const uint32_t off = (c == 0 ? a.pl.r_off : (c == 1 ? a.pl.g_off : a.pl.b_off)) + y * a.pl.row_pitch + x * (uint32_t)T::kBytes;
    const uint8_t *s = a.src + (unsigned long long)blockIdx.y * a.frame_stride + off;
    uint32_t b0, b1;
    if constexpr (T::kBytes == 4) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(s);
        b0 = q[0];
        b1 = q[1];
    } else {
        const uint16_t *q = reinterpret_cast<const uint16_t *>(s);
        b0 = q[0];
        b1 = q[1];
    }
    const unsigned long long plane = (unsigned long long)a.width * a.height;
    uint8_t *d = a.dst + ((unsigned long long)blockIdx.y * 3u + c) * plane + (unsigned long long)y * a.width + x;
    *reinterpret_cast<uint16_t *>(d) = (uint16_t)(float_sample_to_byte<T>(b0, a.pl.scale) | float_sample_to_byte<T>(b1, a.pl.scale) << 8);
}

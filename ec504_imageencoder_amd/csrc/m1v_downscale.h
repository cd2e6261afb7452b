// ec504_imageencoder_amd/csrc/m1v_downscale.h — the tile kernels on 2:1 downscaled renditions of byte surfaces
// (m1v_set_downscale_layout): the encoder has the rendition's size W x H, the frames are 2 W x 2 H surfaces of 3- or 4-byte
// pixels, pitched windows of them included, and the picture that is coded is their 2 x 2 box average.  Not a standalone header:
// included by m1v_kernels.hip behind m1v_float_pixels.h, whose shape it has.  The workgroup, bit stage, scratch slots, segment
// table and counters are those of m1v_tiles.h (the kernel bodies are the same headers); only the front half is new.
//
// The bytes.  Frame f starts at F = base + f * frame_stride; byte i (0, 1, 2) of SOURCE pixel (X, Y) is at
//     F + Y * row_pitch + X * P + i          P = pixel_step = C = 3 or 4 bytes per source pixel
// Bytes 0, 1, 2 are R, G, B (M1V_ORDER_RGB) or B, G, R (M1V_ORDER_BGR); a 4th byte is skipped.  The byte of colour c of rendition
// pixel (x, y) is
//     (s(2x, 2y) + s(2x + 1, 2y) + s(2x, 2y + 1) + s(2x + 1, 2y + 1) + 2) >> 2          s: the source bytes of that colour
// an exact integer, half rounded up.  The record is the one k_encode_tiles gives for the interleaved picture of those bytes:
// convert_row_planes on RowPlanes, fdct_row_f<float, false>, default rounding mode.
//
// Front half (DownscaleFront<C>::run).  The lanes own the blocks they own in k_encode_tiles.  A lane's block row is 8 neighbouring
// rendition pixels = 16 source pixels in each of two source rows, each ONE contiguous run of 16 * P bytes:
//     C = 3    48 bytes per source row   3 x global_load_dwordx4    12 VGPRs
//     C = 4    64 bytes per source row   4 x global_load_dwordx4    16 VGPRs   (the 4th bytes travel and are dropped)
// Only one source row of raw bytes is ever held.  The upper row is summed into 12 dwords of 16-bit pairs as it arrives (per pair of
// rendition pixels x, x + 1: halves (c0[x], c1[x]), (c0[x+1], c1[x+1]), (c2[x], c2[x+1]); a dword of two bytes 16 bits apart is a
// byte permute or a mask and shift, and the two source pixels of a cell add as packed halves, at most 4 * 255 = 1020 per half, so no carry crosses).
// Its registers then take the lower row, which travels while the row before goes through the DCT; the lower row adds into the same
// pairs, (sum + 2) >> 2 under 0x00ff00ff gives the bytes, and they are packed to RowPlanes.  The schedule of one block row i:
//     upper(i + 1) requested | row i converted to float | upper(i + 1) summed | lower(i + 1) requested | DCT of row i
// Each request stands behind an empty asm statement that takes the values just computed from the raw registers as operands
// (settle): a memory clobber alone orders the loads among themselves but lets the compiler sink the sums below the next request,
// which keeps two source rows of raw bytes alive (145 to 157 VGPRs); with the operands it is 118 to 128.
// The order costs no instantiation: the c0 and c2 dwords of RowPlanes are swapped after packing when the layout says B, G, R (a
// uniform select).  No LDS is used in front of the staging: plan_for's regions stay as they are.  The 16-byte loads are of a type
// declared aligned(1): any byte alignment of base, pitch and stride is taken, and each is still one global_load_dwordx4.
// Rejected: both source rows in flight at once (32 VGPRs of raw bytes for C = 4 beside the row in work); byte loads; an LDS
// transpose of tile rows (plan_for's regions would depend on the layout).  The compiler counts vmcnt for these loads (plain C++
// loads); what the caller requested first (the wave's VLC table, LDS-DMA) is older in the queue than every row, and the front half
// ends on vmcnt(0), so the table has landed when it returns, as behind FloatPixelFront.
//
// Read contract (include/mpeg1_hip.h): of frame f only bytes of the source rows [F + Y * row_pitch, F + Y * row_pitch + 2 W * P),
// Y in 0 .. 2 H - 1, are read.  Proof.  A lane's two loads are the 16 source pixels 2x .. 2x + 15 of source rows 2y and 2y + 1, the
// bytes [2x * P, (2x + 16) * P) of each, for the 8 rendition pixels x .. x + 7 of rendition row y:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]: y = 16 mb + 8 (block row) + i with mb = min(m0 + ..,
//                   n_mbrows - 1), so y <= 16 n_mbrows - 1 <= H - 1; x = 16 (s0 + min(strip, strips_here - 1)) + 8 (left|right), so
//                   x + 8 <= 16 n_strips <= W
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]: chroma row 8 mb + i of width W / 2 (the quirk, encoder.h:347-348) is the
//                   left (i even) or right (i odd) half of rendition row y = 4 mb + (i >> 1) <= 4 n_mbrows - 1 <= H - 1;
//                   x = (i & 1) * W / 2 + 8 (s0 + min(strip, strips_here - 1)), so x + 8 <= W / 2 + 8 n_strips <= W
// so 2y + 1 <= 2 H - 1 and (2x + 16) * P = 2 (x + 8) * P <= 2 W * P: no load overhangs a source row, and there is no limit to
// clamp at.  Lanes outside the picture (last tile column / row) repeat the last strip's / macroblock row's pixels, as in
// m1v_tiles.h.  The largest byte offset inside a frame is below (2 H - 1) * row_pitch + 2 W * P < 2^32 (the setter), so 32-bit
// offsets do not wrap.

// 16 bytes at any address
typedef uint32_t QuadAlign1 __attribute__((ext_vector_type(4), aligned(1)));

struct DownscaleFrontArgs {
    uint32_t row_pitch; // bytes from a SOURCE row to the next
    uint32_t bgr;       // 0: bytes 0, 1, 2 are R, G, B; 1: B, G, R
};

// (byte a of the row in w) | (byte b) << 16: two source bytes as packed halves (a and b are constants of the unrolled loops: a
// byte permute or a mask and shift)
template <int N>
__device__ __forceinline__ uint32_t byte_pair(const uint32_t (&w)[N], int a, int b) {
    return ((w[a >> 2] >> (8 * (a & 3))) & 0xffu) | (((w[b >> 2] >> (8 * (b & 3))) & 0xffu) << 16);
}

template <int C>
struct DownscaleFront {
    static_assert(C == 3 || C == 4, "three or four bytes per source pixel");
    DownscaleFrontArgs p;
    static constexpr uint32_t P = (uint32_t)C; // bytes of a source pixel
    static constexpr int kWords = 4 * C;       // dwords of a lane's 16 source pixels of one source row

    struct Raw { uint32_t w[kWords]; };
    // per pair q of rendition pixels (2q, 2q + 1): t[3q] = (c0, c1) of pixel 2q, t[3q + 1] = (c0, c1) of pixel 2q + 1,
    // t[3q + 2] = c2 of both, as 16-bit halves
    struct Sums { uint32_t t[12]; };

    __device__ __forceinline__ static void load16(const uint8_t *src, Raw &raw) {
#pragma unroll
        for (int q = 0; q < kWords / 4; q++) {
            const QuadAlign1 v = *reinterpret_cast<const QuadAlign1 *>(src + 16 * q);
            raw.w[4 * q] = v.x; raw.w[4 * q + 1] = v.y; raw.w[4 * q + 2] = v.z; raw.w[4 * q + 3] = v.w;
        }
    }
    // the horizontal sums of one source row: source pixel k's byte i is byte C * k + i of the row
    __device__ __forceinline__ static void sum_row(const Raw &raw, Sums &s) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = 4 * q; // the first of the pair's four source pixels
            s.t[3 * q] = byte_pair(raw.w, C * k, C * k + 1) + byte_pair(raw.w, C * (k + 1), C * (k + 1) + 1);
            s.t[3 * q + 1] = byte_pair(raw.w, C * (k + 2), C * (k + 2) + 1) + byte_pair(raw.w, C * (k + 3), C * (k + 3) + 1);
            s.t[3 * q + 2] = byte_pair(raw.w, C * k + 2, C * (k + 2) + 2) + byte_pair(raw.w, C * (k + 1) + 2, C * (k + 3) + 2);
        }
    }
    // the upper row's sums and the lower row's raw bytes to the bytes of the 8 rendition pixels, as RowPlanes holds them
    __device__ __forceinline__ void finish_row(const Sums &upper, const Raw &raw, RowPlanes &v) const {
        Sums lower;
        sum_row(raw, lower);
        uint32_t b[12]; // a byte in each half
#pragma unroll
        for (int j = 0; j < 12; j++) b[j] = ((upper.t[j] + lower.t[j] + 0x00020002u) >> 2) & 0x00ff00ffu;
        uint32_t c0[2], c1[2], c2[2];
#pragma unroll
        for (int h = 0; h < 2; h++) { // rendition pixels 4h .. 4h + 3
            const uint32_t u = b[6 * h] | b[6 * h + 1] << 8;     // bytes c0[4h], c0[4h+1], c1[4h], c1[4h+1]
            const uint32_t w = b[6 * h + 3] | b[6 * h + 4] << 8; // ... of pixels 4h + 2, 4h + 3
            c0[h] = (u & 0xffffu) | w << 16;
            c1[h] = u >> 16 | (w & 0xffff0000u);
            const uint32_t m = b[6 * h + 2], n = b[6 * h + 5];   // c2 of pixels (4h, 4h + 1) and (4h + 2, 4h + 3)
            c2[h] = (m & 0xffu) | (m >> 8 & 0xff00u) | (n & 0xffu) << 16 | (n >> 16) << 24;
        }
        const bool bgr = p.bgr != 0;
        v.d[0] = bgr ? c2[0] : c0[0];
        v.d[1] = bgr ? c2[1] : c0[1];
        v.d[2] = c1[0];
        v.d[3] = c1[1];
        v.d[4] = bgr ? c0[0] : c2[0];
        v.d[5] = bgr ? c0[1] : c2[1];
    }


    // The loads that follow stay behind the arithmetic that gave these values: the next source row is not requested while
    // this one still occupies its registers
    __device__ __forceinline__ static void settle(Sums &s) {
        asm volatile("" : "+v"(s.t[0]), "+v"(s.t[1]), "+v"(s.t[2]), "+v"(s.t[3]), "+v"(s.t[4]), "+v"(s.t[5]), "+v"(s.t[6]), "+v"(s.t[7]),
                          "+v"(s.t[8]), "+v"(s.t[9]), "+v"(s.t[10]), "+v"(s.t[11]) : : "memory");
    }
    __device__ __forceinline__ static void settle(RowPlanes &v) {
        asm volatile("" : "+v"(v.d[0]), "+v"(v.d[1]), "+v"(v.d[2]), "+v"(v.d[3]), "+v"(v.d[4]), "+v"(v.d[5]) : : "memory");
    }
    // The template parameters and arguments of FloatPixelFront::run
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the downscale kernels stay in the default rounding mode");
        (void)comp;
        (void)ring;
        const bool chroma = wave == 2;
        const uint32_t L = (uint32_t)lane;
        // ---- the lane's 16 source pixels of the upper source row of row 0 of its block: byte offset inside the frame (the proof
        //      above; rendition row y is source rows 2y and 2y + 1, rendition pixel x starts at source byte 2x * P) ----
        const uint32_t last_strip = (uint32_t)strips_here - 1u;
        uint32_t in_frame;
        if (!chroma) {
            const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(L >> 5), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min((L >> 1) & 7u, last_strip)) * 16u + (L & 1u) * 8u;
            in_frame = (mb * 16u + ((L >> 4) & 1u) * 8u) * 2u * p.row_pitch + x * 2u * P;
        } else {
            const uint32_t mb = (uint32_t)min(m0 + (int)((L >> 3) & 3u), g.n_mbrows - 1);
            const uint32_t x = ((uint32_t)s0 + min(L & 7u, last_strip)) * 8u;
            in_frame = mb * 4u * 2u * p.row_pitch + x * 2u * P;
        }
        // rendition row i lies (i >> 1) * step2 + (i & 1) * step1 behind row 0 (uniform; i is a constant of the unrolled loop)
        const size_t pitch = p.row_pitch;
        const size_t step2 = chroma ? 2u * pitch : 4u * pitch, step1 = chroma ? (size_t)g.half_w * 2u * P : 2u * pitch;
        const uint8_t *row0 = fbase + in_frame;
        auto load_row = [&](int i, int lower, Raw &raw) { load16(row0 + ((size_t)(i >> 1) * step2 + (size_t)(i & 1) * step1 + (size_t)lower * pitch), raw); };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then the upper source row of row 0; the
        //      caller's other prologue work runs while it travels ----
        first();
        Raw raw;
        Sums upper;
        load_row(0, 0, raw);
        meanwhile();
        sum_row(raw, upper);
        settle(upper);
        load_row(0, 1, raw);

        const CompCoefF kf = comp_coef_wave(!chroma, lane);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            RowPlanes v; // the row's bytes; the registers of the raw bytes then take the upper source row of row i + 1
            finish_row(upper, raw, v);
            settle(v);
            if (i + 1 < 8) load_row(i + 1, 0, raw);
            asm volatile("" ::: "memory"); // the loads of row i + 1 stay in this order between row i's arithmetic
            float px[8];
            convert_row_planes(v, kf, px);
            if (i + 1 < 8) {
                sum_row(raw, upper);
                settle(upper);
                load_row(i + 1, 1, raw);
                asm volatile("" ::: "memory");
            }
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
        wait_vm<0>(); // the caller's first() has landed (it is older than every row; the compiler does not count LDS-DMA)
    }
};

// The layout travels in the kernels' own argument structs (as FloatPixelArgs): Geometry stays as it is.
struct DownscaleArgs {
    TileArgs t;
    DownscaleFrontArgs px;
    unsigned long long frame_stride; // bytes from a source frame's base to the next frame's
};
struct DownscaleTableArgs {
    TableArgs t;
    DownscaleFrontArgs px;
    unsigned long long frame_stride;
};
struct DownscaleRdArgs {
    RdTableArgs t;
    DownscaleFrontArgs px;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_DOWNSCALE_INPUT                                                                        \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const DownscaleFront<C> downscale_front = {pa.px}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF downscale_front.template run

// (no amdgpu_waves_per_eu, as for the float pixels: a source row of raw bytes and the upper row's sums beside the row in work take
// the kernels to four waves per SIMD)
template <bool STAGE8, int R, int C>
__global__ __launch_bounds__(kTileThreads) void k_downscale_encode(DownscaleArgs pa) {
    M1V_DOWNSCALE_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R, int C>
__global__ __launch_bounds__(kTileThreads) void k_downscale_size_table(DownscaleTableArgs pa) {
    M1V_DOWNSCALE_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, int C>
__global__ __launch_bounds__(kTileThreads) void k_downscale_rd_table(DownscaleRdArgs pa) {
    M1V_DOWNSCALE_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

// m1v_downscale_to_bytes_device: the bytes the kernels above code, as uint8 [n][H][W][3] in R, G, B order.  Elementwise: a thread
// averages the three colours of one rendition pixel from its four source pixels and stores their three bytes; grid = (pixels of
// a rendition frame, frames).  The pixel step is a run-time value.  Reads addressed bytes only: never a 4th byte.
struct DownscaleBytesArgs {
    const uint8_t *src;
    uint8_t *dst;
    DownscaleFrontArgs px;
    unsigned long long frame_stride;
    uint32_t width, height, pixel_step; // the rendition's width and height
};

__global__ __launch_bounds__(256) void k_downscale_to_bytes(DownscaleBytesArgs a) {
    const uint32_t pixel = blockIdx.x * 256u + threadIdx.x;
    if (pixel >= a.width * a.height) return;
    const uint32_t y = pixel / a.width, x = pixel - y * a.width;
    const uint8_t *s = a.src + (unsigned long long)blockIdx.y * a.frame_stride + (2u * y * a.px.row_pitch + 2u * x * a.pixel_step);
    const uint8_t *t = s + a.px.row_pitch; // the lower source row
    uint32_t v[3];
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = ((uint32_t)s[i] + s[a.pixel_step + i] + t[i] + t[a.pixel_step + i] + 2u) >> 2;
    const uint32_t first = a.px.bgr ? 2u : 0u;
    uint8_t *d = a.dst + ((unsigned long long)blockIdx.y * a.width * a.height + pixel) * 3u;
    d[0] = (uint8_t)v[first];
    d[1] = (uint8_t)v[1];
    d[2] = (uint8_t)v[2 - first];
}

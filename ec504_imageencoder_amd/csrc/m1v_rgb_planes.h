// ec504_imageencoder_amd/csrc/m1v_rgb_planes.h — the tile kernels on frames whose R, G and B bytes lie in three planes
// (m1v_set_rgb_plane_layout): NCHW uint8 tensors in any plane order, three planes of a 4-plane tensor, pitched windows, row-
// interleaved planes.  Not a standalone header: included by m1v_kernels.hip behind m1v_step2.h.  The workgroup, bit stage, scratch
// slots, segment table and counters are those of m1v_tiles.h (the kernel bodies are the same headers); only the front half is new.
//
// The bytes.  Frame f starts at F = base + f * frame_stride; component c of pixel (x, y) is the byte at
//     F + c_off + y * row_pitch + x
// and the record is the one the packed kernels give for the interleaved picture [y][x] = (R, G, B) of those bytes: colour
// conversion (fp32 fast path, fp64 for the ties, in the order tools/colour_fast_proof.c proves), the chroma quirk
// (encoder.h:347-348) and everything behind it.  Default rounding mode, fdct_row_f<float, false>: the surface kernels' pixel stage.
//
// Front half (RgbPlaneFront::run, the fetch shape of tile_pixel_rows).  The lanes own the blocks they own in k_encode_tiles.  One
// row-step of a wave = TWO 1-KiB global_load_lds_dwordx4 into a 2-KiB ring slot, R slots, 16 instructions per wave, the vmcnt
// sequence of tile_pixel_rows.  A slot holds the row-step's bytes of R at 0, of G at 512 and of B at 1024:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]: row i of the wave's 64 blocks is, in each plane, 4 picture
//                   rows x 128 contiguous bytes = 512 bytes = 32 units of 16 bytes, unit = [picture row:2][strip:3]; lane
//                   L's 8 bytes of a plane lie at L * 8.  First instruction: lanes 0-31 the units of R, lanes 32-63 those of G;
//                   second instruction: lanes 0-31 the units of B (lanes 32-63 repeat them into the slot's unused last 512 bytes)
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3].  Plane "row" r' = 8 mb + i of width W/2 (the quirk) is the left (r' even) or
//                   right (r' odd) half of picture row r'/2 = 4 mb + (i >> 1): row i is, in each plane, 4 macroblock rows x 64
//                   contiguous bytes = 256 bytes = 16 units, unit = [mb row:2][two strips:2]; the Cb lane and the Cr lane of a
//                   macroblock read the same 8 bytes of each plane, at (L & 31) * 8, fetched once.  Lanes 16-31 and 48-63 repeat the
//                   units of lanes 0-15 and 32-47 into the unused second half of each plane's 512 bytes.
// The unit a lane requests is one expression in all three waves: plane (lane >> 5 | 2), row (lane >> sh) & 3, unit in the row
// lane & ((1 << sh) - 1), with sh = 3 (luma) or 2 (chroma) wave-uniform, and four uniform row offsets to choose from.  No EXEC
// mask and no branch on the wave kind around the DMA.  The lane then takes 8 bytes of R, of G and of B with three ds_read_b64 at
// one address + 0 / 512 / 1024: lanes 0-31 (32-63) read 256 contiguous bytes, conflict-free.
// Units outside the picture region (last tile column / row) repeat the last strip's / macroblock row's unit, as in m1v_tiles.h.
//
// Read contract (include/mpeg1_hip.h): of frame f only bytes of the three ranges [F + c_off, F + c_off + (H - 1) * row_pitch + W)
// are read.  A luma unit is one strip's 16 addressed bytes of one plane.  A chroma unit is two strips' 8 pixels; with an odd number
// of strips in the last tile column the last unit of a half row holds 8 addressed bytes and 8 bytes behind them.  For a left half
// those are the first bytes of the right half.  For a right half the unit ends at most at x = W / 2 + 8 n_strips + 8 <= W + 8 of
// picture row 4 mb + (i >> 1) <= H / 4 - 1: at least 3 H / 4 >= 12 rows of row_pitch >= W >= 16 bytes in front of the range's end.

struct RgbPlaneFrontArgs {
    uint32_t r_off, g_off, b_off; // bytes from the frame's base to pixel (0, 0) of each plane
    uint32_t row_pitch;           // bytes from a picture row to the next, the same in the three planes
};

// the three 8-byte groups of a block row: d[2 c], d[2 c + 1] = pixels 0-3, 4-7 of component c
struct __attribute__((aligned(4))) RowPlanes {
    uint32_t d[6];
};

// convert_row on de-interleaved bytes: the same sums in the same order, the same flag, the same fp64 tie path (m1v_kernels.hip)
__device__ __forceinline__ void convert_row_planes(const RowPlanes &v, const CompCoefF &k, float out[8]) {
    auto chan = [&](int j, int ch) -> uint32_t { return (v.d[2 * ch + (j >> 2)] >> ((j & 3) * 8)) & 0xffu; };
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
        const CompCoef &d = k.d;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t r = chan(j, 0), gg = chan(j, 1), b = chan(j, 2);
            const float t = component_t(r, gg, b, k);
            if (t - clear_fraction(t) < kFracLow)
                out[j] = m1vf::kPxBiasF + (float)component_fp64((int)r, (int)gg, (int)b, d.k0, d.kr, d.kg, d.kb);
        }
    }
}

struct RgbPlaneFront {
    RgbPlaneFrontArgs p;

    // The template parameters and arguments of tile_pixel_rows; DOWN, BPP, SURFACE, ORDER, comp and the row pitch argument do not
    // apply (the kernels set DOWN = false: the integer row pass in the default rounding mode).
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the RGB plane kernels stay in the default rounding mode");
        (void)comp;
        constexpr uint32_t kSlot = 2048, kPlane = 512;
        const bool chroma = wave == 2;
        auto uniform = [](uint32_t v) { // an opaque scalar, as in tile_pixel_rows
            asm volatile("" : "+s"(v));
            return v;
        };
        const uint32_t L = (uint32_t)lane;
        // the four row offsets a wave's lanes choose from (uniform): luma = the wave's two macroblock rows x (upper | lower blocks),
        // chroma = the tile's four macroblock rows (row 0 of a chroma block of macroblock row mb is the left half of picture row 4 mb)
        auto row_off = [&](uint32_t k) {
            if (!chroma) {
                const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(k >> 1), g.n_mbrows - 1);
                return (mb * 16u + (k & 1u) * 8u) * p.row_pitch + (uint32_t)s0 * 16u;
            }
            const uint32_t mb = (uint32_t)min(m0 + (int)k, g.n_mbrows - 1);
            return mb * 4u * p.row_pitch + (uint32_t)s0 * 8u;
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        // ---- the lane's 16-byte units of row-step 0 (first / second instruction): byte offsets from the frame's base ----
        const uint32_t sh = chroma ? 2u : 3u;                                                  // uniform
        const uint32_t vw = chroma ? (((uint32_t)strips_here * 8u + 15u) & ~15u) : (uint32_t)strips_here * 16u; // bytes of a row fetched
        const uint32_t k = (L >> sh) & 3u;
        const uint32_t in_plane = (k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3))) + min((L & ((1u << sh) - 1u)) * 16u, vw - 16u);
        const uint32_t voff_a = (L >= 32u ? p.g_off : p.r_off) + in_plane;
        const uint32_t voff_b = p.b_off + in_plane;
        // ---- the lane's 8 bytes of R inside slot 0; G and B lie kPlane and 2 kPlane further ----
        const uint32_t lane_row = ring + ((chroma ? L & 31u : L) << 3);
        // row-step r lies (r >> 1) * step2 + (r & 1) * step1 behind row-step 0 (uniform; r is a constant of the unrolled loop)
        const uint32_t step2 = chroma ? p.row_pitch : 2u * p.row_pitch, step1 = chroma ? (uint32_t)g.half_w : p.row_pitch;
        auto issue_row = [&](int r) { // row-step r -> slot r % R.  M0 is set once: the second instruction's offset:1024 moves its LDS
                                      // address AND its source address, so its base is 1024 lower (tile_pixel_rows)
            const uint8_t *sb = fbase + ((size_t)(r >> 1) * step2 + (size_t)(r & 1) * step1);
            const uint32_t dst = ring + (uint32_t)(r % R) * kSlot;
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, %4\n\tglobal_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(voff_a), "v"(voff_b), "s"(dst), "s"(sb), "s"(sb - 1024));
        };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then R row-steps; the caller's other prologue
        //      work runs while they travel ----
        first();
#pragma unroll
        for (int r = 0; r < R; r++) issue_row(r);
        meanwhile();

        // ---- rows out of the ring as they land, the freed slot refilled with row i + R ----
        const CompCoefF kf = comp_coef_wave(!chroma, lane);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int newest = (i - 1 + R < 7) ? (i - 1 + R) : 7; // newest row-step requested so far
            const int behind = newest - i;                         // row-steps that may still be in flight: two instructions each
            if (behind == 0) wait_vm<0>(); else if (behind == 1) wait_vm<2>(); else if (behind == 2) wait_vm<4>();
            else if (behind == 3) wait_vm<6>(); else if (behind == 4) wait_vm<8>(); else if (behind == 5) wait_vm<10>();
            else if (behind == 6) wait_vm<12>(); else wait_vm<14>();
            unsigned long long cr, cg, cb;
            asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %3 offset:%4\n\tds_read_b64 %2, %3 offset:%5\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(cr), "=&v"(cg), "=&v"(cb)
                         : "v"(lane_row + (uint32_t)(i % R) * kSlot), "n"(kPlane), "n"(2 * kPlane));
            if (i + R < 8) issue_row(i + R);
            RowPlanes v;
            v.d[0] = (uint32_t)cr; v.d[1] = (uint32_t)(cr >> 32);
            v.d[2] = (uint32_t)cg; v.d[3] = (uint32_t)(cg >> 32);
            v.d[4] = (uint32_t)cb; v.d[5] = (uint32_t)(cb >> 32);
            float px[8];
            convert_row_planes(v, kf, px);
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
    }
};

// The layout travels in the kernels' own argument structs (as SurfaceArgs and PlaneArgs): Geometry stays as it is.
struct RgbPlaneArgs {
    TileArgs t;
    RgbPlaneFrontArgs pl;
    unsigned long long frame_stride; // bytes from a frame's base to the next frame's
};
struct RgbPlaneTableArgs {
    TableArgs t;
    RgbPlaneFrontArgs pl;
    unsigned long long frame_stride;
};
struct RgbPlaneRdArgs {
    RdTableArgs t;
    RgbPlaneFrontArgs pl;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_RGB_PLANES_INPUT(TABLE)                                                                \
    constexpr bool SURFACE = true, FRAME_TABLE = TABLE, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const RgbPlaneFront rgb_plane_front = {pa.pl}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF rgb_plane_front.template run

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_encode_rgb_planes(RgbPlaneArgs pa) {
    M1V_RGB_PLANES_INPUT(false);
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_size_table_rgb_planes(RgbPlaneTableArgs pa) {
    M1V_RGB_PLANES_INPUT(false);
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_rgb_planes(RgbPlaneRdArgs pa) {
    M1V_RGB_PLANES_INPUT(false);
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

// The same three of a frame table (m1v_set_frame_table): pa.t.rgb holds one 64-bit frame address per frame, pa.frame_stride is not read
template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void kt_encode_rgb_planes(RgbPlaneArgs pa) {
    M1V_RGB_PLANES_INPUT(true);
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void kt_size_table_rgb_planes(RgbPlaneTableArgs pa) {
    M1V_RGB_PLANES_INPUT(true);
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void kt_rd_table_rgb_planes(RgbPlaneRdArgs pa) {
    M1V_RGB_PLANES_INPUT(true);
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

// ---- plane table (m1v_set_plane_table, include/mpeg1_hip.h "Plane table"): one pointer per plane, the kp_* kernels ----
// RgbPlaneFront with every offset relative to its own plane's pointer.  A struct of its own beside RgbPlaneFront, not a parameter
// of it: the k_* and kt_* kernels stay the parent's device code text for text this way.
// `fbase` is the address of the frame's three table entries (R, G, B; plane_table_row), loaded with scalar loads.  The first
// instruction of a row-step reads R in lanes 0-31 and G in lanes 32-63, so it takes one 64-bit address per lane
// (global_load_lds_dwordx4 v[lo:hi], off): the lane's plane pointer + offset, kept in two registers, plus the row-step's uniform
// offset.  The second reads B alone and stays on a scalar base, the B pointer, 1024 lower as before.  The vmcnt sequence is
// RgbPlaneFront's.  Rejected: two scalar-base instructions under EXEC halves, three instructions per row-step and another vmcnt
// sequence.  There is no clamp in this front half: the one unit that runs past its addressed bytes ends in one of the first
// H / 4 rows of its own plane's range (the read contract above), so the argument already was per plane.
struct RgbPlanePtrFront {
    RgbPlaneFrontArgs p;

    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the RGB plane kernels stay in the default rounding mode");
        (void)comp;
        constexpr uint32_t kSlot = 2048, kPlane = 512;
        const bool chroma = wave == 2;
        auto uniform = [](uint32_t v) { // an opaque scalar, as in tile_pixel_rows
            asm volatile("" : "+s"(v));
            return v;
        };
        const PlaneBases bases = PlaneBases::load(fbase);
        const uint32_t L = (uint32_t)lane;
        // the four row offsets a wave's lanes choose from (uniform), as in RgbPlaneFront
        auto row_off = [&](uint32_t k) {
            if (!chroma) {
                const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(k >> 1), g.n_mbrows - 1);
                return (mb * 16u + (k & 1u) * 8u) * p.row_pitch + (uint32_t)s0 * 16u;
            }
            const uint32_t mb = (uint32_t)min(m0 + (int)k, g.n_mbrows - 1);
            return mb * 4u * p.row_pitch + (uint32_t)s0 * 8u;
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        // ---- the lane's 16-byte units of row-step 0: the first instruction's as an address, the second's as an offset from the B pointer ----
        const uint32_t sh = chroma ? 2u : 3u;                                                  // uniform
        const uint32_t vw = chroma ? (((uint32_t)strips_here * 8u + 15u) & ~15u) : (uint32_t)strips_here * 16u; // bytes of a row fetched
        const uint32_t k = (L >> sh) & 3u;
        const uint32_t in_plane = (k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3))) + min((L & ((1u << sh) - 1u)) * 16u, vw - 16u);
        const unsigned long long addr_a = (L >= 32u ? bases.p[1] + p.g_off : bases.p[0] + p.r_off) + in_plane;
        const uint32_t voff_b = p.b_off + in_plane;
        const uint8_t *b_base = reinterpret_cast<const uint8_t *>(static_cast<uintptr_t>(bases.p[2]));
        // ---- the lane's 8 bytes of R inside slot 0; G and B lie kPlane and 2 kPlane further ----
        const uint32_t lane_row = ring + ((chroma ? L & 31u : L) << 3);
        // row-step r lies (r >> 1) * step2 + (r & 1) * step1 behind row-step 0 (uniform; r is a constant of the unrolled loop)
        const uint32_t step2 = chroma ? p.row_pitch : 2u * p.row_pitch, step1 = chroma ? (uint32_t)g.half_w : p.row_pitch;
        auto issue_row = [&](int r) { // row-step r -> slot r % R.  M0 is set once: the second instruction's offset:1024 moves its LDS
                                      // address AND its source address, so its base is 1024 lower (tile_pixel_rows)
            const unsigned long long off = (unsigned long long)(r >> 1) * step2 + (unsigned long long)(r & 1) * step1;
            const uint32_t dst = ring + (uint32_t)(r % R) * kSlot;
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %2, %4 offset:1024\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(addr_a + off), "v"(voff_b), "s"(dst), "s"(b_base + off - 1024));
        };

        first();
#pragma unroll
        for (int r = 0; r < R; r++) issue_row(r);
        meanwhile();

        // ---- rows out of the ring as they land, the freed slot refilled with row i + R ----
        const CompCoefF kf = comp_coef_wave(!chroma, lane);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int newest = (i - 1 + R < 7) ? (i - 1 + R) : 7; // newest row-step requested so far
            const int behind = newest - i;                         // row-steps that may still be in flight: two instructions each
            if (behind == 0) wait_vm<0>(); else if (behind == 1) wait_vm<2>(); else if (behind == 2) wait_vm<4>();
            else if (behind == 3) wait_vm<6>(); else if (behind == 4) wait_vm<8>(); else if (behind == 5) wait_vm<10>();
            else if (behind == 6) wait_vm<12>(); else wait_vm<14>();
            unsigned long long cr, cg, cb;
            asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %3 offset:%4\n\tds_read_b64 %2, %3 offset:%5\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(cr), "=&v"(cg), "=&v"(cb)
                         : "v"(lane_row + (uint32_t)(i % R) * kSlot), "n"(kPlane), "n"(2 * kPlane));
            if (i + R < 8) issue_row(i + R);
            RowPlanes v;
            v.d[0] = (uint32_t)cr; v.d[1] = (uint32_t)(cr >> 32);
            v.d[2] = (uint32_t)cg; v.d[3] = (uint32_t)(cg >> 32);
            v.d[4] = (uint32_t)cb; v.d[5] = (uint32_t)(cb >> 32);
            float px[8];
            convert_row_planes(v, kf, px);
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
    }
};

// pa.t.rgb holds three 64-bit plane addresses per frame; there is no frame stride
template <typename Base>
struct RgbPlanePtrArgs {
    Base t;
    RgbPlaneFrontArgs pl;
};
#define M1V_RGB_PLANE_PTR_INPUT                                                                    \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = true;                        \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    constexpr unsigned long long frame_stride = 0;                                                 \
    const RgbPlanePtrFront rgb_plane_front = {pa.pl}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void kp_encode_rgb_planes(RgbPlanePtrArgs<TileArgs> pa) {
    M1V_RGB_PLANE_PTR_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void kp_size_table_rgb_planes(RgbPlanePtrArgs<TableArgs> pa) {
    M1V_RGB_PLANE_PTR_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void kp_rd_table_rgb_planes(RgbPlanePtrArgs<RdTableArgs> pa) {
    M1V_RGB_PLANE_PTR_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

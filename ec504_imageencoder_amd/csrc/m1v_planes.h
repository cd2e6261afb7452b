// ec504_imageencoder_amd/csrc/m1v_planes.h — the tile kernels on planar and semi-planar YCbCr frames (m1v_set_plane_layout).
// Not a standalone header: included by m1v_kernels.hip behind m1v_tiles.h, whose workgroup, bit stage, scratch slots, segment
// table and counters it keeps (the kernel bodies are the same headers); only the front half is new.
//
// The bytes.  Frame f starts at F = base + f * frame_stride.  The macroblock at (x, y) takes
//     luma block k, row i          the 8 bytes at  F + y_off + (y + 8 (k / 2) + i) * y_pitch + x + 8 (k % 2)
//     chroma plane p, row i, j     the byte at     F + p_off + (y / 2 + i) * c_pitch + (x / 2 + j) * c_step
// which is encoder.h:347-348 (the Cb / Cr plane addressed with stride W / 2) when the planes are the reference's full-resolution
// ones with c_pitch = W / 2, and ordinary 4:2:0 sampling when they are half-resolution planes of that pitch (I420, YV12) or one
// plane of interleaved pairs (NV12, NV21: c_step = 2).  No colour conversion, no fp64, default rounding mode.
//
// Front half (PlaneFront::run, in the place of tile_pixel_rows).  The lanes own the blocks they own in k_encode_tiles:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]: row i of the wave's 64 blocks is 4 picture rows x 128
//                   contiguous bytes = 512 bytes, lane L's 8 bytes at L * 8
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]
//                   CSTEP 1: row i = 2 planes x 4 macroblock rows x 64 bytes = 512 bytes, lane L's 8 bytes at L * 8
//                   CSTEP 2: 2 planes x 4 macroblock rows x 128 bytes = 1024 bytes, lane L's 16 bytes (every other one is its
//                            plane's sample) at L * 16; with NV12 the Cr lanes fetch the Cb lanes' bytes one byte further
// One global_load_lds_dwordx4 of a wave moves 1 KiB = one ring slot:
//     CSTEP 1   two row-steps (lanes 0-31 row 2t, lanes 32-63 row 2t + 1): 4 instructions per wave.  The ring of R * 2 KiB holds
//               all four (R = 2), so they are all requested up front and the row loop waits vmcnt(3), (2), (1), (0), once per
//               two rows
//     CSTEP 2   one row-step (a luma wave's lanes 32-63 repeat lanes 0-31 into the slot's unused half, so that the three waves
//               run one instruction stream and one vmcnt count): 8 instructions, 2 R slots in flight, vmcnt(3) five times, then
//               (2), (1), (0)
// Units outside the picture region (last tile column / row) repeat the last strip's / macroblock row's unit, as in m1v_tiles.h.
//
// Read contract (include/mpeg1_hip.h): nothing outside [F, F + E) rounded up to 4 bytes is read, E = the frame's extent (one
// past the last addressed byte).  Every luma unit is 16 addressed bytes.  Two kinds of chroma unit end behind their last
// addressed byte, and in the last chroma row of the plane that ends a tightly packed frame that is past E:
//     CSTEP 1   with an odd number of strips in the last tile column the row's last unit holds 8 addressed bytes and 8 bytes
//               behind the row (tightly packed I420 / YV12)
//     CSTEP 2   the 16th byte of a unit belongs to the other component, or to nobody: for the component that comes second in
//               a pair it lies one byte behind the row (the Cr lanes of tightly packed NV12)
// `lim` = (E rounded up to 4) - 16 is the last offset a unit may start at.  A unit at u > lim is fetched kBack = 8 (CSTEP 1) or
// 1 (CSTEP 2) bytes earlier: its addressed bytes end at u + 8 resp. u + 15 <= E, so the 16 bytes end inside the frame, and
// u - kBack > lim - 8 >= 0 (E >= 256) starts inside it.  The lane that owns the block reads its 8 bytes from the unit's second
// half (CSTEP 1) or picks the odd bytes instead of the even ones (CSTEP 2).  Both sides derive the move from the same offset,
// so no flag travels.  A unit of 16 addressed bytes has u <= E - 16 <= lim and never moves.

struct PlaneFrontArgs {
    uint32_t y_off, cb_off, cr_off; // bytes from the frame's base to sample (0, 0) of each plane
    uint32_t y_pitch, c_pitch;      // bytes between luma rows / chroma rows of the addressing above
    uint32_t lim;                   // the last offset at which a 16-byte unit may start (see the read contract above)
};

template <int CSTEP>
struct PlaneFront {
    PlaneFrontArgs p;

    // The template parameters and arguments of tile_pixel_rows; DOWN, BPP, SURFACE, ORDER, comp and the row pitch do not apply
    // (the kernels set DOWN = false: the integer row pass in the default rounding mode).
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the plane kernels stay in the default rounding mode");
        static_assert(CSTEP == 1 || CSTEP == 2, "one plane per chroma component, or interleaved pairs");
        (void)comp;
        constexpr int kPerIns = CSTEP == 1 ? 2 : 1; // row-steps one instruction carries
        constexpr int kIns = 8 / kPerIns;           // instructions per wave
        constexpr int kSlots = 2 * R;               // 1-KiB slots of the ring
        constexpr int kAhead = kIns < kSlots ? kIns : kSlots;
        constexpr uint32_t kSlot = 1024;
        const bool chroma = wave == 2;
        auto uniform = [](uint32_t v) { // an opaque scalar, as in tile_pixel_rows
            asm volatile("" : "+s"(v));
            return v;
        };
        const uint32_t L = (uint32_t)lane;
        const uint32_t pitch = chroma ? p.c_pitch : p.y_pitch;
        // the four row offsets a wave's lanes choose from (uniform): luma = the wave's two macroblock rows x (upper | lower blocks),
        // chroma = the tile's four macroblock rows
        auto row_off = [&](uint32_t k) {
            if (!chroma) {
                const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(k >> 1), g.n_mbrows - 1);
                return (mb * 16u + (k & 1u) * 8u) * p.y_pitch + p.y_off + (uint32_t)s0 * 16u;
            }
            const uint32_t mb = (uint32_t)min(m0 + (int)k, g.n_mbrows - 1);
            return mb * 8u * p.c_pitch + (uint32_t)s0 * (8u * CSTEP);
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        auto pick = [&](uint32_t k) { return k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3)); };

        // ---- the lane's 16-byte unit of instruction 0: byte offset from the frame's base ----
        uint32_t unit0;
        {
            const uint32_t u = CSTEP == 1 ? (L & 31u) : L;              // unit inside the row-step
            const uint32_t rs = CSTEP == 1 ? (L >> 5) : 0u;            // which row-step of the instruction
            uint32_t k, wu, vw, plane;
            if (!chroma) {
                k = (u >> 3) & 3u;
                wu = u & 7u;
                vw = (uint32_t)strips_here * 16u;
                plane = 0u;
            } else if (CSTEP == 1) {
                k = (u >> 2) & 3u;
                wu = u & 3u;
                vw = ((uint32_t)strips_here * 8u + 15u) & ~15u;
                plane = (u >> 4) ? p.cr_off : p.cb_off;
            } else {
                k = (u >> 3) & 3u;
                wu = u & 7u;
                vw = (uint32_t)strips_here * 16u;
                plane = (u >> 5) ? p.cr_off : p.cb_off;
            }
            unit0 = pick(k) + plane + rs * pitch + min(wu * 16u, vw - 16u);
        }
        // ---- where the lane's block row lies in a slot, and (CSTEP 1) the unit it comes from, for the shift at `lim` ----
        const uint32_t lane_row = ring + (L << ((CSTEP == 2 && chroma) ? 4 : 3));
        // offset of the unit that holds row 0 of the lane's block (chroma wave; a luma unit never moves)
        const uint32_t own0 = chroma ? pick((L >> 3) & 3u) + (L >= 32u ? p.cr_off : p.cb_off) + (CSTEP == 1 ? ((L >> 1) & 3u) : (L & 7u)) * 16u : 0u;
        constexpr uint32_t kBack = CSTEP == 1 ? 8u : 1u; // how far a unit beyond `lim` moves back

        const uint32_t step = (uint32_t)kPerIns * pitch;
        auto issue = [&](int t) { // instruction t -> slot t % kSlots
            uint32_t voff = unit0 + (uint32_t)t * step;
            voff = voff > p.lim ? voff - kBack : voff;
            dma16(voff, ring + (uint32_t)(t % kSlots) * kSlot, fbase);
        };

        // ---- what the caller adds first (older in the vmcnt queue than the rows), then the ring's fill; the caller's other
        //      prologue work runs while they travel ----
        first();
#pragma unroll
        for (int t = 0; t < kAhead; t++) issue(t);
        meanwhile();

#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int t = i / kPerIns;
            if (i % kPerIns == 0) {
                const int newest = (t - 1 + kSlots < kIns - 1) ? (t - 1 + kSlots) : (kIns - 1); // newest instruction requested so far
                const int behind = newest - t;
                if (behind == 0) wait_vm<0>(); else if (behind == 1) wait_vm<1>(); else if (behind == 2) wait_vm<2>();
                else if (behind == 3) wait_vm<3>(); else if (behind == 4) wait_vm<4>(); else if (behind == 5) wait_vm<5>();
                else if (behind == 6) wait_vm<6>(); else wait_vm<7>();
            }
            uint32_t addr = lane_row + (uint32_t)(t % kSlots) * kSlot + (uint32_t)(i % kPerIns) * 512u;
            const bool moved = chroma && own0 + (uint32_t)i * pitch > p.lim; // the unit of this row was fetched kBack bytes earlier
            if (CSTEP == 1) addr += moved ? 8u : 0u;
            uint32_t lo, hi;
            if (CSTEP == 1) {
                unsigned long long v;
                asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr));
                lo = (uint32_t)v;
                hi = (uint32_t)(v >> 32);
            } else {
                unsigned long long v0, v1;
                asm volatile("ds_read_b64 %0, %2\n\tds_read_b64 %1, %2 offset:8\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v0), "=&v"(v1) : "v"(addr));
                // chroma: the even bytes of the 16 (the odd ones of a unit that moved back one byte); luma: the first 8
                const uint32_t sel = moved ? 0x07050301u : 0x06040200u;
                const uint32_t even_lo = __builtin_amdgcn_perm((uint32_t)(v0 >> 32), (uint32_t)v0, sel);
                const uint32_t even_hi = __builtin_amdgcn_perm((uint32_t)(v1 >> 32), (uint32_t)v1, sel);
                lo = chroma ? even_lo : (uint32_t)v0;
                hi = chroma ? even_hi : (uint32_t)(v0 >> 32);
            }
            if (i % kPerIns == kPerIns - 1 && t + kSlots < kIns) issue(t + kSlots);
            // the byte is the raw pixel: kPxBiasF + value, the input of the fp32 FDCT
            float px[8];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                px[j] = m1vf::kPxBiasF + (float)((lo >> (8 * j)) & 0xffu);
                px[4 + j] = m1vf::kPxBiasF + (float)((hi >> (8 * j)) & 0xffu);
            }
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
    }
};

// The layout travels in the kernels' own argument structs (as SurfaceArgs): Geometry stays as it is.
struct PlaneArgs {
    TileArgs t;
    PlaneFrontArgs pl;
    unsigned long long frame_stride; // bytes from a frame's base to the next frame's
};
struct PlaneTableArgs {
    TableArgs t;
    PlaneFrontArgs pl;
    unsigned long long frame_stride;
};

// the bodies' input-layout names: the frame base is taken as for a surface (base + frame * frame_stride, default rounding mode)
#define M1V_PLANE_INPUT(TABLE)                                                                     \
    constexpr bool SURFACE = true, FRAME_TABLE = TABLE, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const PlaneFront<CSTEP> plane_front = {pa.pl}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF plane_front.template run

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_encode_planes(PlaneArgs pa) {
    M1V_PLANE_INPUT(false);
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void k_size_table_planes(PlaneTableArgs pa) {
    M1V_PLANE_INPUT(false);
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

struct PlaneRdArgs {
    RdTableArgs t;
    PlaneFrontArgs pl;
    unsigned long long frame_stride;
};
template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_planes(PlaneRdArgs pa) {
    M1V_PLANE_INPUT(false);
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

// The same three of a frame table (m1v_set_frame_table): pa.t.rgb holds one 64-bit frame address per frame, pa.frame_stride is not read
template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void kt_encode_planes(PlaneArgs pa) {
    M1V_PLANE_INPUT(true);
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void kt_size_table_planes(PlaneTableArgs pa) {
    M1V_PLANE_INPUT(true);
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void kt_rd_table_planes(PlaneRdArgs pa) {
    M1V_PLANE_INPUT(true);
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

// ---- plane table (m1v_set_plane_table, include/mpeg1_hip.h "Plane table"): one pointer per plane, the kp_* kernels ----
// PlaneFront with every offset relative to its own plane's pointer P and one limit per chroma plane.  A struct of its own beside
// PlaneFront, not a parameter of it: the k_* and kt_* kernels stay the parent's device code text for text this way.
// `fbase` is the address of the frame's three table entries (plane_table_row), loaded with scalar loads.  One chroma instruction
// covers Cb and Cr, so it takes its source from one 64-bit address per lane (global_load_lds_dwordx4 v[lo:hi], off: dma16_at):
// the lane's plane pointer, selected by the bit that selects its plane offset, plus the 32-bit offset of the unit.  The luma
// waves run the same instruction stream with the Y pointer in every lane, and the vmcnt sequence is PlaneFront's.  Rejected: two
// scalar-base instructions under EXEC halves, which doubles the chroma wave's DMA instructions and gives it a vmcnt sequence of
// its own beside the luma waves'.
// The clamp, per plane.  lim_p = (E_p rounded up to 4) - 16 with E_p = p_off + (ye / 2 - 1) * c_pitch + (xe / 2 - 1) * CSTEP + 1,
// relative to P.  A unit of plane p at offset u moves back kBack when u > lim_p; the fetch side (`issue`) and the read side
// (`moved` / `own0`) both compare the unit's offset from its own plane's pointer with that plane's limit, so they agree as
// before.  A unit of 16 addressed bytes has u + 16 <= E_p, so u <= lim_p: it never moves, and luma units, all of them such, are
// held against no limit.
//     CSTEP 1   a unit at u > lim_p holds 8 addressed bytes: u + 8 <= E_p, so the 16 bytes from u - 8 end inside [P, P + E_p).
//               The smallest plane is that of a 16 x 16 picture, 8 rows of 8 bytes: E_p >= 64, lim_p >= 48 and u - 8 > 40 starts
//               inside it (the single-base argument leaned on E >= 256, which one plane need not reach)
//     CSTEP 2   a unit's addressed bytes end at u + 15 <= E_p, so the 16 bytes from u - 1 end inside the range; E_p >= 7 * 16 + 15,
//               lim_p >= 112 and u - 1 > 111.  With both entries on one NV12 plane (offsets 0 and 1) E_cr = E_cb + 1: the 16th
//               byte of Cb's last unit is Cr's last sample, inside Cb's range rounded up to 4.  Each plane is held to its own
//               range, and no read leaves either
struct PlanePtrFrontArgs {
    uint32_t y_off, cb_off, cr_off; // bytes from each plane's pointer to its sample (0, 0)
    uint32_t y_pitch, c_pitch;
    uint32_t lim_cb, lim_cr;        // the last offset from the Cb / Cr pointer at which a 16-byte unit may start
};

template <int CSTEP>
struct PlanePtrFront {
    PlanePtrFrontArgs p;

    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the plane kernels stay in the default rounding mode");
        static_assert(CSTEP == 1 || CSTEP == 2, "one plane per chroma component, or interleaved pairs");
        (void)comp;
        constexpr int kPerIns = CSTEP == 1 ? 2 : 1; // row-steps one instruction carries
        constexpr int kIns = 8 / kPerIns;           // instructions per wave
        constexpr int kSlots = 2 * R;               // 1-KiB slots of the ring
        constexpr int kAhead = kIns < kSlots ? kIns : kSlots;
        constexpr uint32_t kSlot = 1024;
        const bool chroma = wave == 2;
        auto uniform = [](uint32_t v) { // an opaque scalar, as in tile_pixel_rows
            asm volatile("" : "+s"(v));
            return v;
        };
        const PlaneBases bases = PlaneBases::load(fbase);
        const uint32_t L = (uint32_t)lane;
        const uint32_t pitch = chroma ? p.c_pitch : p.y_pitch;
        // the four row offsets a wave's lanes choose from (uniform), as in PlaneFront
        auto row_off = [&](uint32_t k) {
            if (!chroma) {
                const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(k >> 1), g.n_mbrows - 1);
                return (mb * 16u + (k & 1u) * 8u) * p.y_pitch + p.y_off + (uint32_t)s0 * 16u;
            }
            const uint32_t mb = (uint32_t)min(m0 + (int)k, g.n_mbrows - 1);
            return mb * 8u * p.c_pitch + (uint32_t)s0 * (8u * CSTEP);
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        auto pick = [&](uint32_t k) { return k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3)); };

        // ---- the lane's 16-byte unit of instruction 0: byte offset from its plane's pointer, and which plane that is ----
        uint32_t unit0;
        bool fetch_cr = false;
        {
            const uint32_t u = CSTEP == 1 ? (L & 31u) : L;              // unit inside the row-step
            const uint32_t rs = CSTEP == 1 ? (L >> 5) : 0u;            // which row-step of the instruction
            uint32_t k, wu, vw, plane;
            if (!chroma) {
                k = (u >> 3) & 3u;
                wu = u & 7u;
                vw = (uint32_t)strips_here * 16u;
                plane = 0u;
            } else if (CSTEP == 1) {
                k = (u >> 2) & 3u;
                wu = u & 3u;
                vw = ((uint32_t)strips_here * 8u + 15u) & ~15u;
                fetch_cr = (u >> 4) != 0u;
                plane = fetch_cr ? p.cr_off : p.cb_off;
            } else {
                k = (u >> 3) & 3u;
                wu = u & 7u;
                vw = (uint32_t)strips_here * 16u;
                fetch_cr = (u >> 5) != 0u;
                plane = fetch_cr ? p.cr_off : p.cb_off;
            }
            unit0 = pick(k) + plane + rs * pitch + min(wu * 16u, vw - 16u);
        }
        // the lane's plane pointer and that plane's limit on the fetch side (a luma unit never moves) ...
        const unsigned long long base_lane = chroma ? (fetch_cr ? bases.p[2] : bases.p[1]) : bases.p[0];
        const uint32_t lim_fetch = chroma ? (fetch_cr ? p.lim_cr : p.lim_cb) : 0xffffffffu;
        // ... and, on the read side, the limit of the plane the lane's own block lies in
        const uint32_t lim_own = L >= 32u ? p.lim_cr : p.lim_cb;
        // ---- where the lane's block row lies in a slot, and (CSTEP 1) the unit it comes from, for the shift at the limit ----
        const uint32_t lane_row = ring + (L << ((CSTEP == 2 && chroma) ? 4 : 3));
        // offset of the unit that holds row 0 of the lane's block (chroma wave; a luma unit never moves)
        const uint32_t own0 = chroma ? pick((L >> 3) & 3u) + (L >= 32u ? p.cr_off : p.cb_off) + (CSTEP == 1 ? ((L >> 1) & 3u) : (L & 7u)) * 16u : 0u;
        constexpr uint32_t kBack = CSTEP == 1 ? 8u : 1u; // how far a unit beyond its plane's limit moves back

        const uint32_t step = (uint32_t)kPerIns * pitch;
        auto issue = [&](int t) { // instruction t -> slot t % kSlots
            uint32_t voff = unit0 + (uint32_t)t * step;
            voff = voff > lim_fetch ? voff - kBack : voff;
            dma16_at(base_lane + voff, ring + (uint32_t)(t % kSlots) * kSlot);
        };

        first();
#pragma unroll
        for (int t = 0; t < kAhead; t++) issue(t);
        meanwhile();

#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int t = i / kPerIns;
            if (i % kPerIns == 0) {
                const int newest = (t - 1 + kSlots < kIns - 1) ? (t - 1 + kSlots) : (kIns - 1); // newest instruction requested so far
                const int behind = newest - t;
                if (behind == 0) wait_vm<0>(); else if (behind == 1) wait_vm<1>(); else if (behind == 2) wait_vm<2>();
                else if (behind == 3) wait_vm<3>(); else if (behind == 4) wait_vm<4>(); else if (behind == 5) wait_vm<5>();
                else if (behind == 6) wait_vm<6>(); else wait_vm<7>();
            }
            uint32_t addr = lane_row + (uint32_t)(t % kSlots) * kSlot + (uint32_t)(i % kPerIns) * 512u;
            const bool moved = chroma && own0 + (uint32_t)i * pitch > lim_own; // the unit of this row was fetched kBack bytes earlier
            if (CSTEP == 1) addr += moved ? 8u : 0u;
            uint32_t lo, hi;
            if (CSTEP == 1) {
                unsigned long long v;
                asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr));
                lo = (uint32_t)v;
                hi = (uint32_t)(v >> 32);
            } else {
                unsigned long long v0, v1;
                asm volatile("ds_read_b64 %0, %2\n\tds_read_b64 %1, %2 offset:8\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v0), "=&v"(v1) : "v"(addr));
                // chroma: the even bytes of the 16 (the odd ones of a unit that moved back one byte); luma: the first 8
                const uint32_t sel = moved ? 0x07050301u : 0x06040200u;
                const uint32_t even_lo = __builtin_amdgcn_perm((uint32_t)(v0 >> 32), (uint32_t)v0, sel);
                const uint32_t even_hi = __builtin_amdgcn_perm((uint32_t)(v1 >> 32), (uint32_t)v1, sel);
                lo = chroma ? even_lo : (uint32_t)v0;
                hi = chroma ? even_hi : (uint32_t)(v0 >> 32);
            }
            if (i % kPerIns == kPerIns - 1 && t + kSlots < kIns) issue(t + kSlots);
            float px[8];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                px[j] = m1vf::kPxBiasF + (float)((lo >> (8 * j)) & 0xffu);
                px[4 + j] = m1vf::kPxBiasF + (float)((hi >> (8 * j)) & 0xffu);
            }
            float ro[8];
            m1vf::fdct_row_f<float, false>(px, ro);
            rows.put(i, ro);
        }
    }
};

// pa.t.rgb holds three 64-bit plane addresses per frame; there is no frame stride
template <typename Base>
struct PlanePtrArgs {
    Base t;
    PlanePtrFrontArgs pl;
};
#define M1V_PLANE_PTR_INPUT                                                                        \
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = true;                        \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    constexpr unsigned long long frame_stride = 0;                                                 \
    const PlanePtrFront<CSTEP> plane_front = {pa.pl}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void kp_encode_planes(PlanePtrArgs<TileArgs> pa) {
    M1V_PLANE_PTR_INPUT;
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void kp_size_table_planes(PlanePtrArgs<TableArgs> pa) {
    M1V_PLANE_PTR_INPUT;
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R, int CSTEP>
__global__ __launch_bounds__(kTileThreads) void kp_rd_table_planes(PlanePtrArgs<RdTableArgs> pa) {
    M1V_PLANE_PTR_INPUT;
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

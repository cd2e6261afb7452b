// ec504_imageencoder_amd/csrc/m1v_step2.h — the tile kernels on frames whose luma samples lie two bytes apart and whose chroma
// samples lie four bytes apart (m1v_set_sample_layout with y_step = 2, c_step = 4): packed 4:2:2 (YUY2, UYVY, YVYU) and the
// high bytes of P010 / P012 / P016.  Not a standalone header: included by m1v_kernels.hip behind m1v_planes.h, whose argument
// structs (PlaneFrontArgs, PlaneArgs, PlaneTableArgs, PlaneRdArgs) and kernel bodies it keeps; only the front half is new.
//
// The bytes.  Frame f starts at F = base + f * frame_stride.  The macroblock at (x, y) takes
//     luma block k, row i, sample j     the byte at  F + y_off + (y + 8 (k / 2) + i) * y_pitch + (x + 8 (k % 2) + j) * 2
//     chroma plane p, row i, sample j   the byte at  F + p_off + (y / 2 + i) * c_pitch + (x / 2 + j) * 4
// with |cb_off - cr_off| <= 3: both components of a macroblock lie in the same 32 bytes, which start at c_lo = min(cb_off, cr_off).
// No colour conversion, no fp64, default rounding mode: the pixel stage behind the byte pick is the plane kernels'.
//
// Front half (Step2Front::run, the shape of PlaneFront<2>).  One global_load_lds_dwordx4 of a wave moves one row-step = 1 KiB
// = one ring slot; lane F requests the 16-byte unit that lands at F * 16, the same expression in all three waves:
//     luma wave     lane = [mb row:1][block row:1][strip:3][left|right:1]: row i of the wave's 64 blocks is 4 picture rows x 256
//                   contiguous bytes; lane L's 16 bytes lie at L * 16, its 8 samples are every other byte of them
//     chroma wave   lane = [Cb|Cr:1][mb row:2][strip:3]: row i is 4 macroblock rows x 8 strips x 32 bytes, fetched once as two
//                   half-units of 16 bytes per macroblock (F = [mb row:2][strip:3][half:1]).  The Cb lane and the Cr lane of a
//                   macroblock read the same 32 bytes at (L & 31) * 32 and pick every fourth byte at their own phase
//                   own_off - c_lo
// 8 instructions per wave, four 1-KiB slots, vmcnt(3) five times, then (2), (1), (0).  All three waves run one instruction
// stream: no EXEC mask, no branch on the wave kind; what differs is wave-uniform (scalar selects) or a per-lane selector.
//
// Byte picks: v_perm_b32 with the selector in a register.  The lane reads two groups of 16 bytes, X and Y (luma: Y = X + 8, the
// second half of its unit and 8 bytes of the next lane's that no selector names; chroma: Y = X + 16, the second half-unit), and
// builds each dword of four samples as perm(perm(w3, w2, S), perm(w1, w0, S), C):
//     luma     S = 0x06040200 (the even bytes of w0, w1), C = 0x03020100 (the first pick as it is)
//     chroma   S = 0x04000400 + phase * 0x01010101 (byte `phase` of each word of a pair, in bytes 0, 1 and again in 2, 3),
//              C = 0x07060100 (bytes 0, 1 of the first pick, 2, 3 of the second)
// A selector moves k bytes on by adding k * 0x01010101: every index stays below 8 (see the read contract).
// Units outside the picture region (last tile column / row) repeat the last strip's / macroblock row's unit, as in m1v_tiles.h.
//
// Read contract (include/mpeg1_hip.h): nothing outside [F, F + E) rounded up to 4 bytes is read, E = the frame's extent (one
// past the last addressed byte).  Every unit ends behind its last addressed byte: a luma unit u has its samples at u, u + 2, ...,
// u + 14 and ends one byte behind them; a chroma half-unit h has samples of both components between h and h + 12 + d,
// d = |cb_off - cr_off|, and ends 3 - d bytes behind them.  In the last row of a tightly packed frame that tail can lie past E
// rounded up (UYVY luma, YUY2 chroma, P010 chroma).  `lim` = (E rounded up to 4) - 16 is the last offset a fetch may start at.
// A fetch at v > lim starts kBack bytes earlier, kBack = the unit's unaddressed tail: 1 (luma), 3 - d (chroma).  Its last
// addressed byte is v + 15 - kBack < E, so the moved fetch ends at v - kBack + 16 <= E; and v - kBack > lim - 3 >= 0 (E >= 256)
// starts inside the frame.  With kBack = 0 (d = 3) the unit's last byte is addressed, v + 16 <= E, and v > lim does not occur.
// The first half-unit of a macroblock lies 16 bytes in front of addressed bytes and never moves.  The lane that consumes a unit
// derives the move from the same offset comparison and adds kBack to its byte phase, so nothing passes between lanes: luma
// index <= 6 + 1, chroma index <= 4 + phase + kBack <= 4 + d + 3 - d = 7.

struct Step2Front {
    PlaneFrontArgs p;

    // The template parameters and arguments of tile_pixel_rows; DOWN, BPP, SURFACE, ORDER, comp and the row pitch do not apply
    // (the kernels set DOWN = false: the integer row pass in the default rounding mode).
    template <int R, int KEEP, bool DOWN, int BPP, bool SURFACE, int ORDER, typename First, typename Meanwhile>
    __device__ __forceinline__ void run(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0, int m0,
                                        int strips_here, int comp, First first, Meanwhile meanwhile, RowStore<KEEP> &rows,
                                        uint32_t = 0) const {
        static_assert(!DOWN, "the step-2 kernels stay in the default rounding mode");
        (void)comp;
        constexpr int kIns = 8;       // instructions per wave: one row-step each
        constexpr int kSlots = 2 * R; // 1-KiB slots of the ring
        constexpr int kAhead = kIns < kSlots ? kIns : kSlots;
        constexpr uint32_t kSlot = 1024;
        const bool chroma = wave == 2;
        auto uniform = [](uint32_t v) { // an opaque scalar, as in tile_pixel_rows
            asm volatile("" : "+s"(v));
            return v;
        };
        const uint32_t L = (uint32_t)lane;
        const uint32_t pitch = chroma ? p.c_pitch : p.y_pitch;
        const uint32_t c_lo = min(p.cb_off, p.cr_off), c_d = max(p.cb_off, p.cr_off) - c_lo;
        // the four row offsets a wave's lanes choose from (uniform): luma = the wave's two macroblock rows x (upper | lower blocks),
        // chroma = the tile's four macroblock rows; a strip is 32 bytes wide in both
        auto row_off = [&](uint32_t k) {
            if (!chroma) {
                const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(k >> 1), g.n_mbrows - 1);
                return (mb * 16u + (k & 1u) * 8u) * p.y_pitch + p.y_off + (uint32_t)s0 * 32u;
            }
            const uint32_t mb = (uint32_t)min(m0 + (int)k, g.n_mbrows - 1);
            return mb * 8u * p.c_pitch + c_lo + (uint32_t)s0 * 32u;
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        auto pick = [&](uint32_t k) { return k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3)); };

        // ---- the lane's 16-byte unit of instruction 0 (byte offset from the frame's base), and the unit that holds row 0 of the
        //      lane's own block: the same one in a luma wave, the macroblock's first half-unit in the chroma wave ----
        const uint32_t unit0 = pick(L >> 4) + min((L & 15u) * 16u, (uint32_t)strips_here * 32u - 16u);
        const uint32_t own0 = chroma ? pick((L >> 3) & 3u) + (L & 7u) * 32u : unit0;
        const uint32_t y_ahead = chroma ? 16u : 0u;                    // where the unit of group Y starts behind own0
        const uint32_t back = chroma ? 3u - c_d : 1u;                  // kBack: how far a unit beyond `lim` moves back
        const uint32_t back_sel = back * 0x01010101u;
        // ---- the lane's two groups of 16 bytes in slot 0, and its selectors ----
        const uint32_t addr_x = ring + (chroma ? (L & 31u) << 5 : L << 4);
        const uint32_t addr_y = addr_x + (chroma ? 16u : 8u);
        const uint32_t phase = (L >= 32u ? p.cr_off : p.cb_off) - c_lo; // chroma wave
        const uint32_t sel = chroma ? 0x04000400u + phase * 0x01010101u : 0x06040200u;
        const uint32_t comb = chroma ? 0x07060100u : 0x03020100u;

        auto issue = [&](int t) { // instruction t -> slot t % kSlots
            uint32_t voff = unit0 + (uint32_t)t * pitch;
            voff = voff > p.lim ? voff - back : voff;
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
            const int newest = (i - 1 + kSlots < kIns - 1) ? (i - 1 + kSlots) : (kIns - 1); // newest instruction requested so far
            const int behind = newest - i;
            if (behind == 0) wait_vm<0>(); else if (behind == 1) wait_vm<1>(); else if (behind == 2) wait_vm<2>();
            else if (behind == 3) wait_vm<3>(); else if (behind == 4) wait_vm<4>(); else if (behind == 5) wait_vm<5>();
            else if (behind == 6) wait_vm<6>(); else wait_vm<7>();
            const uint32_t slot = (uint32_t)(i % kSlots) * kSlot;
            // the units of this row that were fetched kBack bytes earlier
            const uint32_t own = own0 + (uint32_t)i * pitch;
            const uint32_t sel_x = sel + (own > p.lim ? back_sel : 0u), sel_y = sel + (own + y_ahead > p.lim ? back_sel : 0u);
            unsigned long long x0, x1, y0, y1;
            asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %4 offset:8\n\tds_read_b64 %2, %5\n\tds_read_b64 %3, %5 offset:8\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(x0), "=&v"(x1), "=&v"(y0), "=&v"(y1)
                         : "v"(addr_x + slot), "v"(addr_y + slot));
            if (i + kSlots < kIns) issue(i + kSlots);
            const uint32_t lo = __builtin_amdgcn_perm(__builtin_amdgcn_perm((uint32_t)(x1 >> 32), (uint32_t)x1, sel_x),
                                                      __builtin_amdgcn_perm((uint32_t)(x0 >> 32), (uint32_t)x0, sel_x), comb);
            const uint32_t hi = __builtin_amdgcn_perm(__builtin_amdgcn_perm((uint32_t)(y1 >> 32), (uint32_t)y1, sel_y),
                                                      __builtin_amdgcn_perm((uint32_t)(y0 >> 32), (uint32_t)y0, sel_y), comb);
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

// the bodies' input-layout names, as M1V_PLANE_INPUT
#define M1V_STEP2_INPUT(TABLE)                                                                     \
    constexpr bool SURFACE = true, FRAME_TABLE = TABLE, PLANE_TABLE = false;                       \
    constexpr int BPP = 3, ORDER = 0;                                                              \
    constexpr uint32_t row_pitch = 0;                                                              \
    const unsigned long long frame_stride = pa.frame_stride;                                       \
    const Step2Front step2_front = {pa.pl}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF step2_front.template run

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_encode_step2(PlaneArgs pa) {
    M1V_STEP2_INPUT(false);
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_size_table_step2(PlaneTableArgs pa) {
    M1V_STEP2_INPUT(false);
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_step2(PlaneRdArgs pa) {
    M1V_STEP2_INPUT(false);
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

// The same three of a frame table (m1v_set_frame_table): pa.t.rgb holds one 64-bit frame address per frame, pa.frame_stride is not read
template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void kt_encode_step2(PlaneArgs pa) {
    M1V_STEP2_INPUT(true);
    const TileArgs &a = pa.t;
#include "m1v_encode_tile_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void kt_size_table_step2(PlaneTableArgs pa) {
    M1V_STEP2_INPUT(true);
    const TableArgs &a = pa.t;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void kt_rd_table_step2(PlaneRdArgs pa) {
    M1V_STEP2_INPUT(true);
    M1V_RD_INPUT(pa.t);
#include "m1v_size_table_body.h"
}

#undef M1V_FRONT_HALF
#define M1V_FRONT_HALF tile_pixel_rows

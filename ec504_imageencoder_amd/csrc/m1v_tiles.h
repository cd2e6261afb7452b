// ec504_imageencoder_amd/csrc/m1v_tiles.h — the TILE form of the hot kernel (gfx950).  Not a standalone header: it is
// included by m1v_kernels.hip inside its anonymous namespace, behind the pieces it shares with the run kernels
// (colour conversion, fp32 FDCT, staging layout, VLC walk, bit packing helpers).
//
// Why tiles.  A strip is a 16-pixel wide COLUMN of macroblocks (encoder.h:238 iterates x outermost), i.e. 48 bytes of
// every 128-byte line of the picture; the run kernels (one lane per block down a strip, 24-byte row loads per lane)
// touch ~37 lines with every wave load and fetch every line 2.7 times into some L1 (profiles/r02_memory_path_pmc.txt:
// 4.8 x L1 fills per pixel byte).  Here a workgroup owns a TILE of 8 adjacent strips x 4 macroblock rows
// (128 x 64 pixels: rows of 384 bytes = three whole lines) and brings it in with LDS-DMA
// (global_load_lds_dwordx4: 1 KiB of whole lines per wave instruction, no vector registers), through a small ring of
// row-steps per wave; lanes then take their 24-byte block rows out of LDS.
//
//   workgroup = 3 waves = 192 lanes = the tile's 192 blocks (image_processing.c:138-150 extract_8x8_block order does
//   not matter before the bits are placed):
//     wave 0, 1   luma: macroblock rows 2w, 2w+1 of the tile.  lane = [mb row:1][block row (Y0Y1 | Y2Y3):1][strip:3][Y left|right:1]
//                 so row-step i of the wave (row i of each of its 64 blocks) is 4 picture rows x 384 contiguous bytes
//                 = 1536 bytes, and lane L's 24 bytes sit at L * 24: conflict-free ds_read_b64 x 3.
//     wave 2      chroma: Cb (lanes 0..31) and Cr (32..63) of the tile's 32 macroblocks; both read the SAME 24 bytes
//                 (encoder.h:347-348: the full-resolution plane addressed with stride W/2), which arrive once:
//                 row-step = 4 macroblock rows x 192 bytes.
//   Row-steps travel in a ring of R slots per wave (wave-private: ordered by the wave's own vmcnt, no barrier); the
//   staged levels of the wave's blocks later reuse the ring's bytes.
//
// Bits.  A tile holds 8 strip SEGMENTS (24 consecutive blocks of the strip's stream each).  Lanes write their block's
// bit count to LDS in emission order; after ONE barrier every wave scans all 192 counts itself (no second barrier),
// segments start on word boundaries of the tile's LDS image, and the tile records (bits, where) per segment;
// k_assemble (m1v_assemble.h) concatenates a strip's segments (encoder.h:442-445).

constexpr int kTileStrips = 8, kTileMbRows = 4;
constexpr int kTileThreads = kTileStrips * kTileMbRows * 6; // 192
constexpr int kTileSegBlocks = kTileMbRows * 6;             // 24 blocks of one strip
constexpr int kTileSlot = 2048;                             // bytes of one ring slot = one row-step of a wave (two 1-KiB LDS-DMA instructions)
// LDS words in front of the per-wave regions: one VLC table per wave, bit counts, prefix sums (+ total), segment table, spare
constexpr int kTileVlc = 0, kTileCnt = 3 * kVlcWords, kTileG = kTileCnt + 192, kTileSegTab = kTileG + 196, kTileMisc = kTileSegTab + 16,
              kTileFixedWords = kTileMisc + 4; // 984 words

struct TileArgs {
    Geometry g;
    const uint8_t *rgb;
    const Tables *tab;
    const float *rq_all;    // quantiser of every quality (frame_rq_t)
    const uint32_t *qsel;   // [frame]: where the frame's quantiser lies in rq_all
    uint8_t *scratch;       // [frame][tile][slot_bytes] compact slots, then the overflow arena (as the run kernels)
    uint2 *seg;             // [frame][tile row][strip]: bits of the segment, where it starts (4-byte words from `scratch`)
    unsigned long long *strip_ctr;   // [frame][strip]: every tile adds (1 << 40 | its segment's bits) with ONE returning atomic: the tile
                                     // that sees tile_rows - 1 arrivals in front of it completes the strip and knows its bits
    unsigned long long *frame_bytes; // [frame]: that tile adds the strip's bytes (both zero before the batch: k_assemble of the batch
                                     // before clears them)
    uint32_t *arena_next;
    uint32_t slot_bytes, arena_slots;
    unsigned long long arena_off;
    uint32_t *status;
    int n_frames;
    int tile_cols, tile_rows, tiles_per_frame;
    DivMagic div_group, div_frame, div_cols; // 8 * tiles_per_frame, tiles_per_frame, tile_cols (udiv)
    const uint32_t *tile_row_order; // [tile_rows] (32-bit: a scalar load): which tile row the k-th group of tile_cols workgroups of a frame takes
    int lds_words;          // capacity of the LDS image of the tile's bits
    uint32_t run_cap;       // bytes of one arena slot: the worst case of a tile
    uint32_t luma_region, chroma_region; // LDS bytes of a wave's ring / staging region
    unsigned long long *stamps; // diagnostic builds only: [0..11] luma waves, [12..23] the chroma wave
};

// One LDS-DMA instruction: 16 bytes per active lane from (sbase + voff) to LDS (ldsdst + 16 * lane).  M0 carries the
// destination and is the compiler's: saved and restored inside the statement (cdna_hip_programming.md, inline asm).
__device__ __forceinline__ void dma16(uint32_t voff, uint32_t ldsdst, const uint8_t *sbase) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(ldsdst), "s"(sbase));
}
__device__ __forceinline__ void dma4(uint32_t voff, uint32_t ldsdst, const void *sbase) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(ldsdst), "s"(sbase));
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N));
}
// workgroup barrier that orders LDS only: the wave's LDS operations are retired, global operations in flight (the
// LDS-DMA row-steps) stay in flight across it (__syncthreads() would wait for them)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// 24 bytes at an 8-byte aligned LDS address; loads and their wait in ONE statement (the compiler's waitcnt pass does
// not see LDS operations inside asm)
__device__ __forceinline__ Row24 ring_read24(uint32_t addr) {
    unsigned long long r0, r1, r2;
    asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %3 offset:8\n\tds_read_b64 %2, %3 offset:16\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2)
                 : "v"(addr));
    Row24 v;
    v.d[0] = (uint32_t)r0; v.d[1] = (uint32_t)(r0 >> 32);
    v.d[2] = (uint32_t)r1; v.d[3] = (uint32_t)(r1 >> 32);
    v.d[4] = (uint32_t)r2; v.d[5] = (uint32_t)(r2 >> 32);
    return v;
}

// 32 bytes (eight 4-byte pixels) at a 16-byte aligned LDS address, as ring_read24
__device__ __forceinline__ Row32 ring_read32(uint32_t addr) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 r0, r1;
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(r0), "=&v"(r1)
                 : "v"(addr));
    Row32 v;
    v.d[0] = r0.x; v.d[1] = r0.y; v.d[2] = r0.z; v.d[3] = r0.w;
    v.d[4] = r1.x; v.d[5] = r1.y; v.d[6] = r1.z; v.d[7] = r1.w;
    return v;
}

// ---- packed staging -----------------------------------------------------------------------------------------------------
// The run kernels stage a block with one LDS byte (halfword) store per level and read the words back for the non-zero mask
// (block_to_stage, stage_nonzero_mask).  The tile kernels build the same staging words in registers instead: every level
// passes through one v_cvt_i32_f32 anyway, and as an SDWA instruction that conversion writes its result into byte k
// (halfword k) of a register and leaves the other bytes as they are (dst_sel:BYTE_k dst_unused:UNUSED_PRESERVE; the first
// write to a word takes UNUSED_PAD, which clears the rest: no register is initialised).  Packing so costs no vector
// instruction, a finished word leaves as half of a ds_write2_b32, and the mask comes from the registers the lane holds.
//
// Levels are taken in the order of the column pass, n = 8 i + u (column i, row u of the coefficient matrix).  One asm
// statement per level: the conversion of level n, then the quantiser multiply of level n + 1.  gfx950 wants one wait state
// between a VALU write with a destination select and a VALU read of that register; inside asm nobody inserts it, so every
// statement ends in an instruction without a destination select (the multiply; s_nop after the last level) and whatever the
// compiler puts behind a statement is safe.  The statements are pure as far as the compiler knows (not volatile: the scalar
// loads of the quantiser table stay scalar, m1v_kernels.hip block_to_stage); the word registers chain them.
template <int... Is, typename F>
__device__ __forceinline__ void static_for_each(std::integer_sequence<int, Is...>, F &&f) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) { static_for_each(std::make_integer_sequence<int, N>{}, f); }

template <bool STAGE8>
struct StagePack {
    static constexpr int kWords = STAGE8 ? 16 : 32, kParts = STAGE8 ? 4 : 2;
    static constexpr int pos(int n) { return scan_pos((n & 7) * 8 + (n >> 3)); } // zigzag position of level n
    static constexpr int word(int n) { return (STAGE8 ? stage_byte8(pos(n)) : stage_byte16(pos(n))) >> 2; }
    static constexpr int part(int n) { return STAGE8 ? (stage_byte8(pos(n)) & 3) : ((stage_byte16(pos(n)) >> 1) & 1); }
    // level 0 is the DC level (zigzag position 0): it stays in a register, its byte of word 0 stays zero
    static constexpr bool first(int n) { // the first level written to its word
        for (int k = 1; k < n; k++)
            if (word(k) == word(n)) return false;
        return true;
    }
    static constexpr int done(int w) { // the column whose levels complete word w
        int last = 0;
        for (int n = 1; n < 64; n++)
            if (word(n) == w) last = n;
        return last >> 3;
    }
    // Finished words leave in pairs, in the order they finish: member `which` of the k-th pair that is complete behind column
    // `col`, or -1.  (The number of words is even, so no word is left over behind column 7.)
    static constexpr int pair(int col, int k, int which) {
        int held = -1;
        for (int c = 0; c < 8; c++) {
            int seen = 0;
            for (int w = 0; w < kWords; w++) {
                if (done(w) != c) continue;
                if (held < 0) {
                    held = w;
                    continue;
                }
                if (c == col && seen == k) return which ? w : held;
                seen++;
                held = -1;
            }
        }
        return -1;
    }

    uint32_t w[kWords];
    float t; // the product of the level that is converted next

    // level N into its word; `next` = coefficient x reciprocal of the level behind it
    template <int N, bool LAST = false>
    __device__ __forceinline__ void convert(float c_next, float rq_next) {
        constexpr int W = word(N), P = part(N);
        if constexpr (LAST) {
            if constexpr (STAGE8)
                asm("v_cvt_i32_f32_sdwa %0, %1 dst_sel:BYTE_%2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\ts_nop 0" : "+v"(w[W]) : "v"(t), "n"(P));
            else
                asm("v_cvt_i32_f32_sdwa %0, %1 dst_sel:WORD_%2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\ts_nop 0" : "+v"(w[W]) : "v"(t), "n"(P));
        } else if constexpr (first(N)) { // (early clobber: the word may not take the register of c_next)
            if constexpr (STAGE8)
                asm("v_cvt_i32_f32_sdwa %0, %2 dst_sel:BYTE_%5 dst_unused:UNUSED_PAD src0_sel:DWORD\n\tv_mul_f32 %1, %4, %3"
                    : "=&v"(w[W]), "=v"(t) : "v"(t), "v"(c_next), "s"(rq_next), "n"(P));
            else
                asm("v_cvt_i32_f32_sdwa %0, %2 dst_sel:WORD_%5 dst_unused:UNUSED_PAD src0_sel:DWORD\n\tv_mul_f32 %1, %4, %3"
                    : "=&v"(w[W]), "=v"(t) : "v"(t), "v"(c_next), "s"(rq_next), "n"(P));
        } else {
            if constexpr (STAGE8)
                asm("v_cvt_i32_f32_sdwa %0, %2 dst_sel:BYTE_%5 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\tv_mul_f32 %1, %4, %3"
                    : "+v"(w[W]), "=v"(t) : "v"(t), "v"(c_next), "s"(rq_next), "n"(P));
            else
                asm("v_cvt_i32_f32_sdwa %0, %2 dst_sel:WORD_%5 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\tv_mul_f32 %1, %4, %3"
                    : "+v"(w[W]), "=v"(t) : "v"(t), "v"(c_next), "s"(rq_next), "n"(P));
        }
    }
    // Level N = 8 I + U arrives as coefficient c with its reciprocal rq: the level in front of it is converted (with N's multiply
    // in the same statement), the words that column I - 1 completed leave once its last level is in.  Returns the DC level for
    // N = 0, otherwise 0.
    template <int N>
    __device__ __forceinline__ int level(float c, float rq, uint32_t &lds_addr) {
        if constexpr (N == 0) {
            return quant(c, rq);
        } else if constexpr (N == 1) {
            t = c * rq;
            return 0;
        } else {
            convert<N - 1>(c, rq);
            if constexpr ((N & 7) == 0) store<(N >> 3) - 1>(lds_addr);
            return 0;
        }
    }
    __device__ __forceinline__ void finish(uint32_t &lds_addr) {
        convert<63, true>(0.0f, 0.0f);
        store<7>(lds_addr);
    }
    // the words complete behind column COL, two per LDS instruction, chained through the address register as the byte stores
    // of the run kernels are
    template <int COL, int K = 0>
    __device__ __forceinline__ void store(uint32_t &lds_addr) {
        constexpr int A = pair(COL, K, 0), B = pair(COL, K, 1);
        if constexpr (A >= 0) {
            asm("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" : "+v"(lds_addr) : "v"(w[A]), "v"(w[B]), "n"(A), "n"(B));
            store<COL, K + 1>(lds_addr);
        }
    }
    // stage_nonzero_mask on the registers (bit 0, the DC level's, is clear: the caller sets it), then the stores are waited
    // for: the lane's LDS reads of its staged levels (tile_fetch_level) come behind this statement, and so does every use of the
    // mask, so the wait sits behind the mask arithmetic.
    __device__ __forceinline__ unsigned long long mask_and_fence(uint32_t &lds_addr) const {
        uint32_t half[2] = {0u, 0u};
        if constexpr (STAGE8) {
            // Byte staging: v_lerp_u8(w, ~0, 0) = (byte + 255) >> 1 per byte sets bit 7 of a byte exactly when the byte is
            // non-zero: one instruction for a word's flags instead of three ((w & 0x7f..) + 0x7f.. | w).  Word j's flags belong
            // at bit j of each byte: the words are taken in order, the collected flags move down one bit per word and
            // v_bfi_b32 takes bit 7 of every byte from the new word: three instructions per word, five to six before.  What
            // else word 0's lerp leaves in bits 0..6 has been shifted through a bit 7, and so replaced, by the time word 7 is
            // in.  (asm: written in C++ the compiler reassociates the chain into shifts, ANDs and ORs of its own, a third more.)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                uint32_t acc = __builtin_amdgcn_lerp(w[h * 8], ~0u, 0u);
#pragma unroll
                for (int j = 1; j < 8; j++) {
                    const uint32_t f = __builtin_amdgcn_lerp(w[h * 8 + j], ~0u, 0u), down = acc >> 1;
                    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(acc) : "s"(0x80808080u), "v"(f), "v"(down));
                }
                half[h] = acc;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 2; h++) {
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t f = ((w[h * 16 + j] & 0x7fff7fffu) + 0x7fff7fffu) | w[h * 16 + j];
                    half[h] |= (f >> (15 - j)) & (0x00010001u << j);
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(half[0]), "+v"(half[1]), "+v"(lds_addr) : : "memory");
        return ((unsigned long long)half[1] << 32) | half[0];
    }
};
// (tests/test_stage_packing.py replays the whole plan; here only its first pair: the narrow form finishes no word before column 4)
static_assert(StagePack<true>::pair(3, 0, 0) == -1 && StagePack<true>::pair(4, 0, 0) == 0 && StagePack<true>::pair(4, 0, 1) == 1, "narrow staging plan");

// ---- the code walk of the tile kernels ----------------------------------------------------------------------------------
// The same walk as the run kernels' (block_bits_pass1, walk_codes in m1v_kernels.hip: one coded level per trip, branch-free,
// ac_code for the code word) with a cheaper trip; the run kernels keep theirs instruction for instruction.
//
// The staged level at zigzag position p, by ONE sign-extending LDS read at the level's own byte (halfword): no word read, no
// computed shift amount, no shift pair.  The address is stage_byte8(p) / stage_byte16(p), written as bit moves:
//   narrow  ((p & 7) + 8 (p >> 5)) * 4 + ((p >> 3) & 3)  =  (p & 32) | rotl5(p & 31, 2)       (bits 4..0 rotated left by two)
//   wide    ((p & 15) + 16 (p >> 5)) * 4 + 2 ((p >> 4) & 1)  =  (p & 15) << 2 | (p & 32) << 1 | (p & 16) >> 3
// (tests/test_bits_trip_cpu.py checks both forms against the layout for every p).
typedef int16_t __attribute__((may_alias)) staged_i16;
__host__ __device__ constexpr uint32_t tile_stage_byte8(uint32_t p) { return (p & 32u) | (((((p & 31u) << 5) | (p & 31u)) >> 3) & 31u); }
__host__ __device__ constexpr uint32_t tile_stage_byte16(uint32_t p) { return ((p & 15u) << 2) | ((p & 32u) << 1) | ((p & 16u) >> 3); }
template <bool STAGE8>
__device__ __forceinline__ int tile_fetch_level(const uint32_t *blk, uint32_t p) {
    int level;
    if constexpr (STAGE8)
        level = reinterpret_cast<const int8_t *>(blk)[tile_stage_byte8(p)];
    else
        level = *reinterpret_cast<const staged_i16 *>(reinterpret_cast<const char *>(blk) + tile_stage_byte16(p));
    // (opaque: ac_code also takes the level's low byte, and seeing that use the compiler loads the byte unsigned and extends
    //  the sign with an instruction of its own)
    asm("" : "+v"(level));
    return level;
}
static_assert(tile_stage_byte8(0) == stage_byte8(0) && tile_stage_byte8(27) == stage_byte8(27) && tile_stage_byte8(63) == stage_byte8(63), "narrow staging address");
static_assert(tile_stage_byte16(0) == stage_byte16(0) && tile_stage_byte16(27) == stage_byte16(27) && tile_stage_byte16(63) == stage_byte16(63), "wide staging address");

// The coded positions of `emit` in ascending order, each with its run - 1 (ac_code's r), by shifting the set out: `rest` holds
// the positions behind the one coded last (`pos`), its lowest set bit z zeros further on.  One 64-bit shift per trip instead
// of emit &= emit - 1 (a 64-bit subtract and two ANDs), and the run comes from z, not from a difference of positions.
// emit's bit 0 (the DC level's) is clear, so the set starts shifted by one: z <= 62 and the shift count z + 1 stays below 64.
// A zero DC level is one more zero in front of the FIRST coded level only (image_processing.c:716-722): `lead` is -1 from the
// second trip on, and the compiler peels the first trip off the loop, so the loop itself adds a constant.
template <typename Each>
__device__ __forceinline__ void tile_walk_emit(bool dc_nonzero, unsigned long long emit, Each each) {
    unsigned long long rest = emit >> 1;
    int pos = 0;
    int lead = dc_nonzero ? -1 : 0;
    while (rest) {
        const int z = __builtin_ctzll(rest);
        rest >>= z + 1;
        pos += z + 1;
        const int r = z + lead;
        __builtin_assume(r >= 0 && r < 63); // (no two neighbours in emit_set, and not position 1 behind a non-zero DC level)
        each(pos, r);
        lead = -1;
    }
}
// block_bits_pass1 and walk_codes on that walk
template <bool NARROW, typename Fetch>
__device__ __forceinline__ void tile_bits_pass1(uint32_t hdr, int hlen, bool dc_nonzero, unsigned long long emit, const uint32_t *vlc,
                                                Fetch fetch, unsigned long long &acc, int &tot, uint32_t &bad) {
    unsigned long long bits_acc = hdr;
    int n = hlen;
    tile_walk_emit(dc_nonzero, emit, [&](int p, int r) {
        uint32_t code, bits;
        ac_code<NARROW>(vlc, r, fetch(p), code, bits, bad);
        bits_acc = (bits_acc << bits) | code;
        n += (int)bits;
    });
    acc = (bits_acc << 2) | 0x2u; // EOB "10", mpeg1_blk.c:115-117
    tot = n + 2;
}
template <bool NARROW, typename Fetch, typename Sink>
__device__ __forceinline__ void tile_walk_codes(uint32_t hdr, int hlen, bool dc_nonzero, unsigned long long emit, const uint32_t *vlc,
                                                Fetch fetch, Sink &sink) {
    sink(hdr, hlen);
    uint32_t bad = 0;
    tile_walk_emit(dc_nonzero, emit, [&](int p, int r) {
        uint32_t code, bits;
        ac_code<NARROW>(vlc, r, fetch(p), code, bits, bad);
        sink(code, (int)bits);
    });
    sink(0x2u, 2);
}

// column pass + quantise + stage in LDS; returns the DC level, nz = the non-zero mask of the AC levels (bit 0 clear)
template <bool STAGE8, int KEEP>
__device__ __forceinline__ int columns_to_stage(const RowStore<KEEP> &rows, const M1V_CONST_AS float *rq_t, uint32_t &lds_addr,
                                                unsigned long long &nz) {
    int dc = 0;
    StagePack<STAGE8> pk;
    static_for<8>([&](auto I) {
        constexpr int i = decltype(I)::value;
        float c[8];
        m1vf::fdct_col_f<float>(rows.get(0, i), rows.get(1, i), rows.get(2, i), rows.get(3, i), rows.get(4, i), rows.get(5, i),
                                rows.get(6, i), rows.get(7, i), c, i == 0 ? RowStore<KEEP>::kBias0 : 0.0f);
        static_for<8>([&](auto U) {
            constexpr int u = decltype(U)::value;
            dc |= pk.template level<i * 8 + u>(c[u], rq_t[i * 8 + u], lds_addr);
        });
    });
    pk.finish(lds_addr);
    nz = pk.mask_and_fence(lds_addr);
    return dc;
}

// Row-pass outputs stay unpacked (RowStore<8>: 64 registers, 96 VGPRs = 5 waves per SIMD).  Packing all of them as f16 pairs
// (66 VGPRs, 6 waves per SIMD) won 2 % while the launches came in bursts of a few and the chip boosted, and lost 0.5-2.5 % in a
// sustained run, where the package sits at its 1400 W limit and the 96 extra conversions per block cost more than the sixth
// wave hides (tools/sustained.py, profiles/r03_ab_history.txt); that form was removed in round 4.
#ifndef M1V_TILE_KEEP
#define M1V_TILE_KEEP 8
#endif
// the 16-bit staging of qualities above 76 needs a few registers more in the column stage: three column pairs packed there
// (85 VGPRs; 4 unpacked columns already spill 40 bytes per lane)
#ifndef M1V_TILE_KEEP_WIDE
#define M1V_TILE_KEEP_WIDE 2
#endif
// Diagnostic build only (-DM1V_TILE_STAMPS, tools/tile_stamps.py): cycles a wave spends in each phase, kept in scalar
// registers and added to TileArgs::stamps once at the end (a global atomic inside the row loop would join the vmcnt queue).
#ifdef M1V_TILE_STAMPS
#define TSTAMP(ph)                                                                                 \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                              \
        asm volatile("s_waitcnt lgkmcnt(0)");                                                      \
        tstamp_[ph] += now_ - tstamp_t_;                                                           \
        tstamp_t_ = now_;                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    } while (0)
#define TSTAMP_INIT()                                                                              \
    unsigned long long tstamp_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                          \
    unsigned long long tstamp_t_ = __builtin_amdgcn_s_memtime();                                   \
    asm volatile("s_waitcnt lgkmcnt(0)")
#define TSTAMP_FLUSH()                                                                             \
    do {                                                                                           \
        if (lane == 0)                                                                             \
            for (int ph_ = 0; ph_ < 12; ph_++) atomicAdd(&a.stamps[ph_ + (chroma ? 12 : 0)], tstamp_[ph_]); \
    } while (0)
#else
#define TSTAMP(ph) do { } while (0)
#define TSTAMP_INIT() do { } while (0)
#define TSTAMP_FLUSH() do { } while (0)
#endif

#ifndef M1V_TILE_LEAN
#define M1V_TILE_LEAN false
#endif
// the input layout of the packed kernels, for the kernel bodies that are shared with the surface kernels as headers
#define M1V_PACKED_INPUT                                                                           \
    constexpr bool SURFACE = false, FRAME_TABLE = false, PLANE_TABLE = false;                      \
    constexpr int ORDER = 0;                                                                       \
    constexpr uint32_t row_pitch = 0;                                                              \
    constexpr unsigned long long frame_stride = 0
// the front half the kernel bodies call (m1v_planes.h puts its own in this place for the plane kernels)
#define M1V_FRONT_HALF tile_pixel_rows

// The frame base in the kt_* kernels, the instantiations of a frame table (m1v_set_frame_table; FRAME_TABLE in the bodies) beside
// every kernel that takes a layout: `rgb` is a device array of one 64-bit address per frame, and the layout's frame_stride is not
// read.  `frame` is workgroup-uniform (frame_unit_of on blockIdx.x), so this is one 8-byte scalar load where the k_* kernels have a
// scalar multiply-add.  The table has kernels of its own, not a runtime select in the k_* kernels: with the select the stride
// encodes of two layouts measured outside their A/A spread against the parent's (DESIGN.md "Frame tables").
__device__ __forceinline__ const uint8_t *frame_table_entry(const uint8_t *rgb, int frame) {
    return reinterpret_cast<const uint8_t *>(static_cast<uintptr_t>(reinterpret_cast<const unsigned long long *>(rgb)[frame]));
}
// The kp_* kernels, the instantiations of a plane table (m1v_set_plane_table; PLANE_TABLE in the bodies) beside the plane and RGB
// plane kernels: `rgb` is a device array uint64_t[n_frames][3] of one address per plane.  The body hands the front half the
// address of the frame's row of the table in the place of the frame base; PlaneBases::load turns it into the three plane
// addresses with scalar loads (the row's address is workgroup-uniform).  Kernels of their own for the reason above.
__device__ __forceinline__ const uint8_t *plane_table_row(const uint8_t *rgb, int frame) { return rgb + (unsigned long long)frame * 24ull; }
struct PlaneBases {
    unsigned long long p[3]; // Y, Cb, Cr or R, G, B
    static __device__ __forceinline__ PlaneBases load(const uint8_t *row) {
        // (written out: left to the compiler, the loads of the RGB plane kernels became vector loads and the B pointer a VGPR pair)
        unsigned long long p0, p1, p2;
        asm volatile("s_load_dwordx2 %0, %3, 0x0\n\ts_load_dwordx2 %1, %3, 0x8\n\ts_load_dwordx2 %2, %3, 0x10\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(p0), "=&s"(p1), "=&s"(p2)
                     : "s"(row));
        return {{p0, p1, p2}};
    }
};
// dma16 from one 64-bit address per lane (no scalar base): where one wave instruction reads two planes of a plane table
__device__ __forceinline__ void dma16_at(unsigned long long vaddr, uint32_t ldsdst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(vaddr), "s"(ldsdst));
}
#ifndef M1V_TILE_WAVES_PER_EU
#define M1V_TILE_WAVES_PER_EU 5
#endif

// The front half of a tile wave (shared by k_encode_tiles and k_coefficient_tiles): brings the wave's 64 blocks in through
// its LDS ring and leaves the 64 row-pass outputs of the lane's block in `rows`.  `ring` = LDS byte address of the wave's
// region; wave 0, 1 = luma, wave 2 = chroma (see the head of this file); `first` / `meanwhile`: see below.  DOWN: the row
// pass takes its rounded-down form (the wave has switched MODE: pixel_stage_rounds_down); false = the integer form of the run
// kernels, right in the default mode (k_size_table_tiles).
// BPP = 4: 4-byte pixels (the alpha byte is skipped), the front half of k_size_table_rgba.  The same workgroup, ring and
// vmcnt count; a picture row of a tile is 8 x 16 x 4 = 512 bytes, so
//     luma    row-step = 4 pieces x 512 = the 2048 bytes of the slot: units 0..63 (pieces 0, 1) | units 64..127 (pieces 2, 3);
//             lane L's 32 bytes sit at L * 32
//     chroma  row-step = 4 macroblock rows x 256 bytes = ONE instruction; the second repeats it into the slot's other half
// and every strip is a whole number of 16-byte units (64 luma, 32 chroma): no unit straddles the tile's last strip.
// SURFACE: the picture is a window of a pitched surface (k_encode_surface, k_size_table_surface): picture row y starts at
// fbase + y * row_pitch, W is even.  The lanes' offsets and the LDS layout are the packed ones; only the scalar row offsets
// change:
//     luma    row-step i of a block row = picture row + i: i * row_pitch further
//     chroma  the quirk's plane "row" r' = 8 * mb + i of width W/2 (encoder.h:347-348) is the left (r' even) or right (r' odd)
//             half of picture row r'/2: (4 * mb + (i >> 1)) * row_pitch + (i & 1) * (W/2) * BPP
// ORDER: M1V_ORDER_BGR = the colour bytes of a pixel are B, G, R (convert_row takes byte 2 - ch).
template <int R, int KEEP, bool DOWN = true, int BPP = 3, bool SURFACE = false, int ORDER = 0, typename First, typename Meanwhile>
__device__ __forceinline__ void tile_pixel_rows(const Geometry &g, const uint8_t *fbase, uint32_t ring, int wave, int lane, int s0,
                                                int m0, int strips_here, int comp, First first, Meanwhile meanwhile,
                                                RowStore<KEEP> &rows, uint32_t row_pitch = 0) {
    const bool chroma = wave == 2;
    // ---- the lane's share of the wave's DMA.  One row-step = TWO 1-KiB LDS-DMA instructions into a 2-KiB ring slot, the
    //      same for the luma waves and the chroma wave (no branch, no EXEC mask, one vmcnt count):
    //        luma    units 0..63 | units 64..95 (lanes 32..63 repeat them into the slot's unused last 512 bytes)
    //        chroma  macroblock rows 0, 1 (2 x 192 bytes, lanes 0..23; the others repeat) | rows 2, 3, at +1024
    //      Pieces outside the picture region (last tile column / row) re-read bytes of the last strip / macroblock row;
    //      the lanes that own those blocks are not `valid`. ----
    uint32_t pitch;          // bytes from row i to row i + 1 of a block
    uint32_t voff_a, voff_b; // this lane's 16 bytes of row 0 (first / second instruction): byte offset from the frame base
    uint32_t lane_row;       // LDS address of the lane's 24 bytes inside slot 0
    // The four row offsets a wave's lanes choose from are products of UNIFORM values (scalar multiplies); a lane picks its own by
    // compare and select: per-lane 32-bit multiplies and the division of the lane index by 24 are quarter-rate instructions.
    const uint32_t third = (uint32_t)(lane >= 24) + (uint32_t)(lane >= 48); // lane / 24
    auto uniform = [](uint32_t v) { // an opaque scalar (the compiler removes a readfirstlane of a value it knows to be uniform)
        asm volatile("" : "+s"(v));
        return v;
    };
    if constexpr (BPP == 4) {
        const uint32_t piece = (uint32_t)lane >> (chroma ? 4 : 5); // which of the instruction's pieces the lane's unit lies in
        const uint32_t row_px = chroma ? (uint32_t)g.half_w : (uint32_t)g.W;
        pitch = row_px * 4u;
        const uint32_t vw = (uint32_t)strips_here * (chroma ? 32u : 64u); // bytes of a piece that lie inside the picture region
        const uint32_t within = min(((uint32_t)lane & (chroma ? 15u : 31u)) * 16u, vw - 16u);
        auto row_off = [&](uint32_t pc) { // uniform
            if (!chroma) {
                const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(pc >> 1), g.n_mbrows - 1);
                if constexpr (SURFACE) return (mb * 16u + (pc & 1u) * 8u) * row_pitch + (uint32_t)s0 * 64u;
                return ((mb * 16u + (pc & 1u) * 8u) * row_px + (uint32_t)s0 * 16u) * 4u;
            }
            const uint32_t mb = (uint32_t)min(m0 + (int)pc, g.n_mbrows - 1);
            if constexpr (SURFACE) return (mb * 4u) * row_pitch + (uint32_t)s0 * 32u;
            return ((mb * 8u) * row_px + (uint32_t)s0 * 8u) * 4u;
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        if (!chroma) {
            voff_a = (piece ? r1 : r0) + within;
            voff_b = (piece ? r3 : r2) + within;
            lane_row = ring + ((uint32_t)lane << 5);
        } else {
            voff_a = voff_b = (piece == 0 ? r0 : (piece == 1 ? r1 : (piece == 2 ? r2 : r3))) + within;
            lane_row = ring + (((uint32_t)lane & 31u) << 5); // [macroblock row:2][strip:3] x 32 bytes; Cb and Cr read the same
        }
    } else if (!chroma) {
        pitch = (uint32_t)g.W * 3u;
        const uint32_t vw = (uint32_t)strips_here * 48u;
        // 16-byte unit L of the 1536-byte row-step: piece = L / 24 = picture row of the step, `within` inside its 384 bytes
        auto row_off = [&](uint32_t piece) { // uniform
            const uint32_t mb = (uint32_t)min(m0 + 2 * wave + (int)(piece >> 1), g.n_mbrows - 1);
            if constexpr (SURFACE) return (mb * 16u + (piece & 1u) * 8u) * row_pitch + (uint32_t)s0 * 48u;
            return ((mb * 16u + (piece & 1u) * 8u) * (uint32_t)g.W + (uint32_t)s0 * 16u) * 3u;
        };
        // (opaque: left visible, the compiler folds the selects back into per-lane multiplies)
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        // first instruction: units 0..63 -> pieces 0, 1, 2
        voff_a = (third == 0 ? r0 : (third == 1 ? r1 : r2)) + min(((uint32_t)lane - (third << 4) - (third << 3)) * 16u, vw - 16u);
        // second instruction: units 64 + (lane & 31) = 64..95 -> piece 2 (units 64..71) or 3
        const uint32_t l5 = (uint32_t)lane & 31u;
        voff_b = l5 < 8u ? r2 + min((16u + l5) * 16u, vw - 16u) : r3 + min((l5 - 8u) * 16u, vw - 16u);
        lane_row = ring + ((uint32_t)lane << 4) + ((uint32_t)lane << 3);
    } else {
        pitch = (uint32_t)g.half_w * 3u;
        const uint32_t vw = (uint32_t)strips_here * 24u;
        // (an odd number of strips ends in the middle of a 16-byte unit: that unit is still fetched whole — up to 8 bytes
        //  past the tile's last strip, still inside the first quarter of the frame, where all chroma sources lie.  SURFACE: a
        //  right half ends where its picture row ends, so the 8 bytes are row padding or the next row's first bytes: the row is
        //  one of the first H/4 of the window, far in front of the last row's end)
        const uint32_t L = (uint32_t)lane - (third << 4) - (third << 3), piece = (uint32_t)(L >= 12u), within = min((L - (piece << 3) - (piece << 2)) * 16u, ((vw + 15u) & ~15u) - 16u);
        auto row_off = [&](uint32_t mbrow) { // uniform
            const uint32_t mb = (uint32_t)min(m0 + (int)mbrow, g.n_mbrows - 1);
            if constexpr (SURFACE) return (mb * 4u) * row_pitch + (uint32_t)s0 * 24u;
            return ((mb * 8u) * (uint32_t)g.half_w + (uint32_t)s0 * 8u) * 3u;
        };
        const uint32_t r0 = uniform(row_off(0)), r1 = uniform(row_off(1)), r2 = uniform(row_off(2)), r3 = uniform(row_off(3));
        voff_a = (piece ? r1 : r0) + within;
        voff_b = (piece ? r3 : r2) + within;
        const uint32_t mrow = ((uint32_t)lane >> 3) & 3u, l3 = (uint32_t)lane & 7u;
        lane_row = ring + (mrow >> 1) * 1024u + (mrow & 1u) * 192u + (l3 << 4) + (l3 << 3);
    }
    constexpr uint32_t kSlot = 2048;
    // SURFACE: row-step r lies (r >> 1) * step2 + (r & 1) * step1 behind row-step 0 (uniform; r is a constant of the unrolled loop)
    const uint32_t step2 = chroma ? row_pitch : 2u * row_pitch, step1 = chroma ? (uint32_t)g.half_w * (uint32_t)BPP : row_pitch;
    auto issue_row = [&](int r) { // row-step r -> slot r % R.  M0 (the LDS destination) is set once: the second instruction's
                                  // offset:1024 moves its LDS address AND its source address, so its base is 1024 lower
        const uint8_t *sb = SURFACE ? fbase + ((size_t)(r >> 1) * step2 + (size_t)(r & 1) * step1) : fbase + (size_t)r * pitch;
        const uint32_t dst = ring + (uint32_t)(r % R) * kSlot;
        uint32_t keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, %4\n\tglobal_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff_a), "v"(voff_b), "s"(dst), "s"(sb), "s"(sb - 1024));
    };

    // ---- everything this wave needs from memory is requested up front: what the caller adds (older in the vmcnt queue than
    //      the rows), then R row-steps; the caller's other prologue work runs while they travel ----
    first();
#pragma unroll
    for (int r = 0; r < R; r++) issue_row(r);
    meanwhile();

    // ---- rows out of the ring as they land, the freed slot refilled with row i + R ----
    (void)comp;
    // packed R,G,B bytes in the kernels that round down: the luma waves take their colour sums from denormal operands
    // (convert_row_tile, m1v_kernels.hip)
    constexpr bool kLumaRow = DOWN && BPP == 3 && !SURFACE && ORDER == 0;
    const CompCoefF kf = comp_coef_wave(!chroma, lane);
    TileRowConst row_const = {};
    if constexpr (kLumaRow) row_const = tile_row_const();
    (void)row_const;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int newest = (i - 1 + R < 7) ? (i - 1 + R) : 7; // newest row-step requested so far
        const int behind = newest - i;                         // row-steps that may still be in flight: two instructions each
        if (behind == 0) wait_vm<0>(); else if (behind == 1) wait_vm<2>(); else if (behind == 2) wait_vm<4>();
        else if (behind == 3) wait_vm<6>(); else if (behind == 4) wait_vm<8>(); else if (behind == 5) wait_vm<10>();
        else if (behind == 6) wait_vm<12>(); else wait_vm<14>();
        float px[8];
        if constexpr (BPP == 4) {
            const Row32 v = ring_read32(lane_row + (uint32_t)(i % R) * kSlot);
            if (i + R < 8) issue_row(i + R);
            convert_row<4, true, ORDER>(v, kf, px);
        } else {
            const Row24 v = ring_read24(lane_row + (uint32_t)(i % R) * kSlot);
            if (i + R < 8) issue_row(i + R);
            if constexpr (kLumaRow) {
                // one wave-uniform branch per row-step around the eight colour sums only: the ring read, the refill, the tie branch
                // and the row pass exist once.  (opaque per row-step: branches on one visible condition would be threaded into
                // two copies of the whole stage)
                convert_row_tile(v, kf, row_const, uniform((uint32_t)wave) != 2u, px);
            } else {
                convert_row<3, M1V_TILE_LEAN, ORDER>(v, kf, px);
            }
        }
        float ro[8];
        m1vf::fdct_row_f<float, DOWN>(px, ro); // DOWN: the wave rounds down, pixel_stage_rounds_down()
        rows.put(i, ro);
    }
}


template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_encode_tiles(TileArgs a) {
    constexpr int BPP = 3;
    M1V_PACKED_INPUT;
#include "m1v_encode_tile_body.h"
}

// The same tile encode on a window of a pitched surface, 3- or 4-byte pixels in R,G,B or B,G,R order (m1v_set_input_layout).
// The layout travels in the kernel's own argument struct: Geometry, which every kernel's kernarg segment carries, stays as it is.
// Output: the tile path's scratch, segment table and counters; k_assemble and k_frame_sizes serve it unchanged.
struct SurfaceArgs {
    TileArgs t;
    unsigned long long frame_stride; // bytes from a frame's first pixel to the next frame's
    uint32_t row_pitch;              // bytes from a picture row to the next
};
template <bool STAGE8, int R, int BPP, int ORDER>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_encode_surface(SurfaceArgs sa) {
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;
    const TileArgs &a = sa.t;
    const uint32_t row_pitch = sa.row_pitch;
    const unsigned long long frame_stride = sa.frame_stride;
#include "m1v_encode_tile_body.h"
}
// ... and of a frame table (m1v_set_frame_table): sa.t.rgb holds one 64-bit frame address per frame, sa.frame_stride is not read
template <bool STAGE8, int R, int BPP, int ORDER>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void kt_encode_surface(SurfaceArgs sa) {
    constexpr bool SURFACE = true, FRAME_TABLE = true, PLANE_TABLE = false;
    const TileArgs &a = sa.t;
    const uint32_t row_pitch = sa.row_pitch;
    const unsigned long long frame_stride = sa.frame_stride;
#include "m1v_encode_tile_body.h"
}

// ---- BASELINE config 2 on tiles: FDCT + quantise + zigzag only (image_processing.c:192-381), int16 levels out ----------
// The same front half as k_encode_tiles; the 64 levels of a block are staged as int16 at their zigzag index (block stride 34
// words: 8-byte aligned, two lanes per bank), and the tile's eight strip segments (24 consecutive blocks = 3 KiB of the
// output each) leave as whole 128-byte lines: 8 bytes per lane and store instruction, consecutive lanes consecutive bytes.
struct CoefTileArgs {
    Geometry g;
    const uint8_t *rgb;
    const Tables *tab;
    int16_t *out; // [frame][strip][macroblock][Y0 Y1 Y2 Y3 Cb Cr][64]
    int n_frames, tile_cols, tile_rows, tiles_per_frame;
    uint32_t region; // LDS bytes of a wave's ring / staging region
};
constexpr int kCoefStride = 34; // words per staged block

template <int R>
__global__ __launch_bounds__(kTileThreads) __attribute__((amdgpu_waves_per_eu(M1V_TILE_WAVES_PER_EU, M1V_TILE_WAVES_PER_EU)))
void k_coefficient_tiles(CoefTileArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Geometry &g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)lds;
    int frame, tile;
    frame_strip_of(blockIdx.x, a.n_frames, a.tiles_per_frame, frame, tile);
    const int tr = tile / a.tile_cols, tc = tile - tr * a.tile_cols;
    int s0 = tc * kTileStrips, m0 = tr * kTileMbRows;
    const uint8_t *fbase = pixel_stage_rounds_down(a.rgb + (unsigned long long)frame * g.frame_bytes, s0, m0);
    const int strips_here = min(kTileStrips, g.n_strips - s0), mrows_here = min(kTileMbRows, g.n_mbrows - m0);
    const int comp = wave == 2 ? 1 + (lane >> 5) : 0;

    RowStore<M1V_TILE_KEEP> rows;
    tile_pixel_rows<R, M1V_TILE_KEEP>(g, fbase, lds0 + (uint32_t)wave * a.region, wave, lane, s0, m0, strips_here, comp, [] {}, [] {}, rows);

    // column pass + quantise; level of zigzag position p -> int16 p of the lane's staged block (the ring is drained: its bytes are reused)
    const M1V_CONST_AS float *rq_t = reinterpret_cast<const M1V_CONST_AS float *>(reinterpret_cast<uintptr_t>(a.tab->rq_t));
    uint32_t lds_addr = lds0 + (uint32_t)wave * a.region + (uint32_t)lane * (kCoefStride * 4u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float c[8];
        m1vf::fdct_col_f<float>(rows.get(0, i), rows.get(1, i), rows.get(2, i), rows.get(3, i), rows.get(4, i), rows.get(5, i),
                                rows.get(6, i), rows.get(7, i), c, i == 0 ? RowStore<M1V_TILE_KEEP>::kBias0 : 0.0f);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int q = quant(c[u], rq_t[i * 8 + u]);
            asm("ds_write_b16 %0, %1 offset:%2" : "+v"(lds_addr) : "v"(q), "n"(2 * scan_pos(u * 8 + i)));
        }
    }
    // every wave's blocks staged (the barrier takes the address register the stores are chained through)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::"v"(lds_addr) : "memory");

    // store: unit = 16 bytes (two 8-byte LDS reads: the staged blocks are 8-byte aligned); a strip segment = 24 blocks x 8
    // units, in emission order (macroblock row, then Y0 Y1 Y2 Y3 Cb Cr)
    const int bps = g.n_mbrows * 6;
    const unsigned char *lds_bytes = reinterpret_cast<const unsigned char *>(lds);
    const int units_valid = mrows_here * 6 * 8;
#pragma unroll
    for (int t = 0; t < kTileStrips * kTileSegBlocks * 8 / kTileThreads; t++) {
        const int u = tid + t * kTileThreads;
        const int j = u / (kTileSegBlocks * 8), within = u - j * (kTileSegBlocks * 8);
        if (j >= strips_here || within >= units_valid) continue;
        const int b = within >> 3, part = within & 7, m = b / 6, blk = b - m * 6;
        // who staged block (j, m, blk): see the lane order of the luma / chroma waves at the head of this file
        const int w_src = blk < 4 ? (m >> 1) : 2;
        const int l_src = blk < 4 ? (m & 1) * 32 + (blk >> 1) * 16 + j * 2 + (blk & 1) : (blk - 4) * 32 + m * 8 + j;
        const unsigned char *from = lds_bytes + (size_t)w_src * a.region + (size_t)l_src * (kCoefStride * 4) + part * 16;
        const uint2 lo = *reinterpret_cast<const uint2 *>(from), hi = *reinterpret_cast<const uint2 *>(from + 8);
        int16_t *o = a.out + (((size_t)frame * g.n_strips + (size_t)(s0 + j)) * bps + (size_t)m0 * 6) * 64;
        *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(o) + (size_t)within * 16) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
}


// ---- the size table (m1v_frame_size_table_device): record sizes of every frame at up to 8 qualities in one pass ---------
// The tile front half runs ONCE per block: colour, row pass, column pass.  The 64 coefficients then stay in registers, and
// for each quality k the lane quantises them with that quality's table, stages the levels (the ring's bytes, as k_encode_tiles),
// builds the non-zero mask and counts the block's bits with the pass 1 of k_encode_tiles (dc_header, emit_set,
// block_bits_pass1).  No bits are placed: no pass 2, no LDS image, no compact slot, no overflow arena.  After one barrier lane
// k * 8 + j of wave 0 sums segment j at quality k and adds it to strip_ctr with the arrival count of k_encode_tiles; the tile
// that completes a strip adds its bytes to frame_bytes.  k_size_table_sizes turns those into sizes and clears them.
// The wave stays in the default rounding mode: the row pass takes the integer form of the run kernels (fdct_row_f<float, false>).
struct TableArgs {
    Geometry g;
    const uint8_t *rgb;
    const Tables *tab;
    const float *rq_all;                 // quantiser of every quality (frame_rq_t)
    uint32_t qoff[kMaxCandidates];       // [k] where quality k's quantiser lies in rq_all
    int n_q;
    unsigned long long *strip_ctr;       // [k][frame][strip]: (arrivals << 40) | bits, as TileArgs::strip_ctr
    unsigned long long *frame_bytes;     // [k][frame]: bytes of the frame's strips
    uint32_t *status;                    // [k]: M1V_STATUS_UNENCODABLE
    int n_frames, tile_cols, tile_rows, tiles_per_frame;
    DivMagic div_group, div_frame, div_cols; // as TileArgs
    const uint32_t *tile_row_order;
    uint32_t region;                     // LDS bytes of a wave's ring / staging region
};
// LDS words in front of the per-wave regions: one VLC table per wave, the bit counts [quality][block in emission order]
constexpr int kTableCnt = 3 * kVlcWords, kTableFixedWords = kTableCnt + kMaxCandidates * kTileThreads;

// what the body's distortion stage (the k_rd_table_* kernels below) reads, for the kernels that write sizes only
#define M1V_SIZES_ONLY                                                                             \
    constexpr bool RD = false;                                                                     \
    constexpr const float *rd_dq = nullptr;                                                        \
    constexpr unsigned long long *rd_dist = nullptr

// The body of both kernels is csrc/m1v_size_table_body.h, included into each with BPP = the bytes per pixel of its input (a
// shared inline function would do, but the compiler then numbers the registers of the 3-channel kernel differently: its
// code stays the parent's instruction for instruction this way).
template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_size_table_tiles(TableArgs a) {
    constexpr int BPP = 3;
    M1V_PACKED_INPUT;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}
// The same for 4-channel pictures, whatever kernel encodes them: the table places no bits, so it does not have to share the
// shape of the encoder's producer (k_encode_dense, or k_encode_strips for short strips).
template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_size_table_rgba(TableArgs a) {
    constexpr int BPP = 4;
    M1V_PACKED_INPUT;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}
// The same on a window of a pitched surface (m1v_set_input_layout), the front half of k_encode_surface.
struct SurfaceTableArgs {
    TableArgs t;
    unsigned long long frame_stride;
    uint32_t row_pitch;
};
template <bool STAGE8, int R, int BPP, int ORDER>
__global__ __launch_bounds__(kTileThreads) void k_size_table_surface(SurfaceTableArgs sa) {
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;
    const TableArgs &a = sa.t;
    const uint32_t row_pitch = sa.row_pitch;
    const unsigned long long frame_stride = sa.frame_stride;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}
// (of a frame table)
template <bool STAGE8, int R, int BPP, int ORDER>
__global__ __launch_bounds__(kTileThreads) void kt_size_table_surface(SurfaceTableArgs sa) {
    constexpr bool SURFACE = true, FRAME_TABLE = true, PLANE_TABLE = false;
    const TableArgs &a = sa.t;
    const uint32_t row_pitch = sa.row_pitch;
    const unsigned long long frame_stride = sa.frame_stride;
    M1V_SIZES_ONLY;
#include "m1v_size_table_body.h"
}

// The size table's place of k_frame_sizes (one workgroup per frame and quality): the record size (48 bytes of headers and trailer
// + the strips' bytes) into out_sizes[k * stride + frame], the status word of quality k into out_status[k], and every counter
// the probe added to cleared for the next call.
struct TableSizesArgs {
    int n_frames, n_strips;
    unsigned long long *strip_ctr, *frame_bytes; // [k][frame][strip], [k][frame]
    uint32_t *status;                            // [k]
    unsigned long long *out_sizes;
    unsigned long long stride;
    uint32_t *out_status;                        // [k], or null
};
__global__ __launch_bounds__(256) void k_size_table_sizes(TableSizesArgs a) {
    const unsigned long long kf = (unsigned long long)blockIdx.y * (unsigned)a.n_frames + blockIdx.x;
    for (int s = threadIdx.x; s < a.n_strips; s += 256) a.strip_ctr[kf * (unsigned)a.n_strips + s] = 0ull;
    if (threadIdx.x == 0) {
        a.out_sizes[blockIdx.y * a.stride + blockIdx.x] = 48ull + a.frame_bytes[kf];
        a.frame_bytes[kf] = 0ull;
        if (blockIdx.x == 0) {
            if (a.out_status) a.out_status[blockIdx.y] = a.status[blockIdx.y];
            a.status[blockIdx.y] = 0u;
        }
    }
}

// ---- the rate-distortion table (m1v_frame_rd_table_device): the size table plus the distortion of every frame at every quality ----
// The size-table body with its distortion stage (RD): per quality a second statically unrolled pass over the 64 coefficients in
// their registers, a sum per wave (DPP), a sum per tile in LDS (3 x kMaxCandidates words behind the waves' regions) and one
// 64-bit atomic per tile and quality into frame_dist[k][frame].  The arguments wrap TableArgs, as SurfaceTableArgs does: the
// kernarg layout of the size-table kernels stays as it is.
struct RdTableArgs {
    TableArgs t;
    const float *dq_all;             // the divisors of every quality, in the index order of rq_all (exact small integers)
    unsigned long long *frame_dist;  // [k][frame]: sum of the frame's block distortions
};
constexpr int kRdPartWords = 3 * kMaxCandidates; // LDS words of the per-wave sums
#define M1V_RD_INPUT(ra)                                                                           \
    constexpr bool RD = true;                                                                      \
    const TableArgs &a = (ra).t;                                                                   \
    const float *rd_dq = (ra).dq_all;                                                              \
    unsigned long long *rd_dist = (ra).frame_dist

template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_tiles(RdTableArgs ra) {
    constexpr int BPP = 3;
    M1V_PACKED_INPUT;
    M1V_RD_INPUT(ra);
#include "m1v_size_table_body.h"
}
template <bool STAGE8, int R>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_rgba(RdTableArgs ra) {
    constexpr int BPP = 4;
    M1V_PACKED_INPUT;
    M1V_RD_INPUT(ra);
#include "m1v_size_table_body.h"
}
struct SurfaceRdArgs {
    RdTableArgs t;
    unsigned long long frame_stride;
    uint32_t row_pitch;
};
template <bool STAGE8, int R, int BPP, int ORDER>
__global__ __launch_bounds__(kTileThreads) void k_rd_table_surface(SurfaceRdArgs sa) {
    constexpr bool SURFACE = true, FRAME_TABLE = false, PLANE_TABLE = false;
    const uint32_t row_pitch = sa.row_pitch;
    const unsigned long long frame_stride = sa.frame_stride;
    M1V_RD_INPUT(sa.t);
#include "m1v_size_table_body.h"
}
// (of a frame table)
template <bool STAGE8, int R, int BPP, int ORDER>
__global__ __launch_bounds__(kTileThreads) void kt_rd_table_surface(SurfaceRdArgs sa) {
    constexpr bool SURFACE = true, FRAME_TABLE = true, PLANE_TABLE = false;
    const uint32_t row_pitch = sa.row_pitch;
    const unsigned long long frame_stride = sa.frame_stride;
    M1V_RD_INPUT(sa.t);
#include "m1v_size_table_body.h"
}

// k_size_table_sizes for the rd table: sizes, distortions and status out, every counter the pass added to cleared
struct RdSizesArgs {
    TableSizesArgs s;
    unsigned long long *frame_dist; // [k][frame]
    unsigned long long *out_dist;   // out_dist[k * s.stride + frame]
};
__global__ __launch_bounds__(256) void k_rd_table_sizes(RdSizesArgs ra) {
    const TableSizesArgs &a = ra.s;
    const unsigned long long kf = (unsigned long long)blockIdx.y * (unsigned)a.n_frames + blockIdx.x;
    for (int s = threadIdx.x; s < a.n_strips; s += 256) a.strip_ctr[kf * (unsigned)a.n_strips + s] = 0ull;
    if (threadIdx.x == 0) {
        a.out_sizes[blockIdx.y * a.stride + blockIdx.x] = 48ull + a.frame_bytes[kf];
        ra.out_dist[blockIdx.y * a.stride + blockIdx.x] = ra.frame_dist[kf];
        a.frame_bytes[kf] = 0ull;
        ra.frame_dist[kf] = 0ull;
        if (blockIdx.x == 0) {
            if (a.out_status) a.out_status[blockIdx.y] = a.status[blockIdx.y];
            a.status[blockIdx.y] = 0u;
        }
    }
}

// ec504_imageencoder_amd/csrc/m1v_size_table_body.h — the body of k_size_table_tiles, k_size_table_rgba and k_size_table_surface
// (m1v_tiles.h), included inside each kernel.  In scope: STAGE8, R (template parameters), TableArgs a, and the input layout:
// BPP (bytes per pixel), SURFACE, ORDER, row_pitch, frame_stride (tile_pixel_rows), FRAME_TABLE, PLANE_TABLE; M1V_FRONT_HALF names the front half (as in
// m1v_encode_tile_body.h).
// RD (a constant in scope) = true makes it the body of the k_rd_table_* kernels: the same sizes plus the distortion of every
// frame and quality into rd_dist[k][frame], with rd_dq = the divisors of every quality in the index order of rq_all (M1V_SIZES_ONLY
// sets the three for the size-table kernels, whose code the RD statements leave as it was).
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Geometry &g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool chroma = wave == 2; // wave-uniform
    constexpr int kStride = STAGE8 ? kStageStride8 : kStageStride16;
    const uint32_t *vlc = lds + wave * kVlcWords;
    uint32_t *cnt = lds + kTableCnt;
    [[maybe_unused]] uint32_t *rd_part = lds + kTableFixedWords + 3u * (a.region / 4u); // RD: [quality][wave] sums, behind the waves' regions
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const uint32_t region_off = (uint32_t)kTableFixedWords * 4u + (uint32_t)wave * a.region; // bytes from lds

    // the tile and its place in the tile-row order: as k_encode_tiles
    int frame, tile;
    frame_unit_of(blockIdx.x, a.n_frames, a.div_group, a.div_frame, frame, tile);
    const int tk = (int)udiv((uint32_t)tile, a.div_cols), tc = tile - tk * a.tile_cols;
    const int tr = (int)a.tile_row_order[tk];
    const int s0 = tc * kTileStrips, m0 = tr * kTileMbRows;
    const uint8_t *fbase;
    if constexpr (SURFACE && PLANE_TABLE) fbase = plane_table_row(a.rgb, frame); // (the kp_* kernels: the frame's three entries of the plane table)
    else if constexpr (SURFACE && FRAME_TABLE) fbase = frame_table_entry(a.rgb, frame); // (the kt_* kernels: a.rgb is the frame table)
    else fbase = a.rgb + (unsigned long long)frame * (SURFACE ? frame_stride : g.frame_bytes);
    auto owner = [&](int ln, int &j, int &m, int &blk) {
        if (!chroma) {
            m = 2 * wave + (ln >> 5);
            blk = ((ln >> 4) & 1) * 2 + (ln & 1);
            j = (ln >> 1) & 7;
        } else {
            m = (ln >> 3) & 3;
            blk = 4 + (ln >> 5);
            j = ln & 7;
        }
    };
    const int strips_here = min(kTileStrips, g.n_strips - s0); // >= 1
    int comp;
    {
        int j_, m_, blk_;
        owner(lane, j_, m_, blk_);
        comp = blk_ < 4 ? 0 : blk_ - 3;
    }

    // ---- pixel stage, once: the wave's VLC table is requested in front of the rows ----
    RowStore<8> rows;
    M1V_FRONT_HALF<R, 8, false, BPP, SURFACE, ORDER>(
        g, fbase, lds0 + region_off, wave, lane, s0, m0, strips_here, comp,
        [&]() {
#pragma unroll
            for (int q = 0; q < kVlcWords / kWave; q++)
                dma4((uint32_t)lane * 4u, lds0 + (uint32_t)(wave * kVlcWords + q * kWave) * 4u, a.tab->vlc + q * kWave);
        },
        [] {}, rows, row_pitch);
    // ---- column pass, once: coef[u * 8 + i] = coefficient (row u, column i) ----
    float coef[64];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float c[8];
        m1vf::fdct_col_f<float>(rows.get(0, i), rows.get(1, i), rows.get(2, i), rows.get(3, i), rows.get(4, i), rows.get(5, i),
                                rows.get(6, i), rows.get(7, i), c, i == 0 ? RowStore<8>::kBias0 : 0.0f);
#pragma unroll
        for (int u = 0; u < 8; u++) coef[u * 8 + i] = c[u];
    }
    // RD.  With t = l * d (what a decoder would put in the place of coefficient c), a position the record carries costs
    // (c - t)^2 and any other position c^2, so  D(block) = sum of c^2 over all 64  -  sum of t * (2c - t) over the carried ones.
    // Every fp32 value here is an exact integer: |c| <= 2040, l * d lies between 0 and c (truncating division), so
    // 0 <= t * (2c - t) = c^2 - (c - t)^2 <= c^2 < 2^23, and every partial sum is at most the sum of c^2 of the block, which is
    // below 2^24 (about the sum of the 64 squared pixels, <= 4.2 M).
    [[maybe_unused]] float sumsq = 0.0f;
    if constexpr (RD) {
#pragma unroll
        for (int t = 0; t < 64; t++) sumsq = __builtin_fmaf(coef[t], coef[t], sumsq);
    }
    int j, m, blk;
    {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        owner(ln, j, m, blk);
    }
    const bool valid = j < strips_here && m0 + m < g.n_mbrows;
    const int e = j * kTileSegBlocks + m * 6 + blk; // position in the tile's emission order (strip, macroblock, block)
    // every row-step has landed and has been read: the ring's bytes now hold the staged levels of the wave's blocks
    const uint32_t *blkp = lds + region_off / 4u + lane * kStride;
    auto fetch = [&](int p) -> int { return tile_fetch_level<STAGE8>(blkp, (uint32_t)p); };

    // ---- per quality: quantise, stage, mask, count (pass 1) ----
    uint32_t bad_q = 0; // bit k: an unencodable level at quality k
    for (int k = 0; k < a.n_q; k++) {
        const M1V_CONST_AS float *rq_t = reinterpret_cast<const M1V_CONST_AS float *>(reinterpret_cast<uintptr_t>(a.rq_all + a.qoff[k]));
        uint32_t lds_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint32_t *)blkp;
        // the staging stores (asm, chained through lds_addr) stay behind the previous quality's reads of the staged levels
        asm volatile("" : "+v"(lds_addr) : : "memory");
        int dc = 0;
        StagePack<STAGE8> pk; // the staging words in registers (m1v_tiles.h), levels in the order of the column pass
        static_for<64>([&](auto N) {
            constexpr int n = decltype(N)::value, i = n >> 3, u = n & 7;
            dc |= pk.template level<n>(coef[u * 8 + i], rq_t[i * 8 + u], lds_addr);
        });
        pk.finish(lds_addr);
        const unsigned long long nz = pk.mask_and_fence(lds_addr) | (dc != 0 ? 1ull : 0ull);
        uint32_t hdr = 0, bad = 0;
        int hlen = 0;
        BlockBits bb = {0, 0};
        dc_header(dc, blk < 4, blk, vlc, hdr, hlen);
        tile_bits_pass1<STAGE8>(hdr, hlen, dc != 0, emit_set(nz), vlc, fetch, bb.acc, bb.tot, bad);
        cnt[k * kTileThreads + e] = valid ? (uint32_t)bb.tot : 0u;
        bad_q |= (valid && bad) ? 1u << k : 0u;
        if constexpr (RD) {
            // a second pass over the coefficients in their registers (static indices): the level again, as quant() yields it
            // (the same product, truncated), and the bit of the position in the set the record carries (DC + emit_set)
            const M1V_CONST_AS float *dq_t = reinterpret_cast<const M1V_CONST_AS float *>(reinterpret_cast<uintptr_t>(rd_dq + a.qoff[k]));
            const unsigned long long keep = emit_set(nz) | 1ull;
            const uint32_t keep_lo = (uint32_t)keep, keep_hi = (uint32_t)(keep >> 32);
            float gain = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; i++) {
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int p = scan_pos(u * 8 + i);
                    const float c = coef[u * 8 + i];
                    const float t = __builtin_truncf(c * rq_t[i * 8 + u]) * dq_t[i * 8 + u];
                    const float w = __builtin_fmaf(2.0f, c, -t);
                    const int carried = (int)((p < 32 ? keep_lo : keep_hi) << (31 - (p & 31))) >> 31; // 0 or -1
                    gain = __builtin_fmaf(__uint_as_float(__float_as_uint(t) & (uint32_t)carried), w, gain);
                }
            }
            // lanes outside the picture ran on re-read bytes: they add nothing.  A wave's sum is below 64 * 2^24.
            const uint32_t dw = wave_sum_u32(valid ? (uint32_t)(sumsq - gain) : 0u);
            if (lane == 0) rd_part[k * 3 + wave] = dw;
        }
    }
    lds_barrier();

    // ---- wave 0, lane k * 8 + j: segment j at quality k (24 consecutive counts), then the strip's arrival ----
    if (wave == 0) {
        const int k = lane >> 3, jj = lane & 7;
        if (k < a.n_q && jj < strips_here) {
            const uint4 *c4 = reinterpret_cast<const uint4 *>(cnt + k * kTileThreads + jj * kTileSegBlocks);
            uint32_t bits = tr == 0 ? 38u : 0u; // the strip starts in this tile: slice header in front (mpeg1_blk.c:12-16)
#pragma unroll
            for (int t = 0; t < kTileSegBlocks / 4; t++) {
                const uint4 v = c4[t];
                bits += v.x + v.y + v.z + v.w;
            }
            const unsigned long long kf = (unsigned long long)k * (unsigned)a.n_frames + (unsigned)frame;
            const unsigned long long before = atomicAdd(a.strip_ctr + kf * (unsigned)g.n_strips + (unsigned)(s0 + jj),
                                                        (1ull << kCtrCountShift) | (unsigned long long)bits);
            if ((uint32_t)(before >> kCtrCountShift) == (uint32_t)a.tile_rows - 1u)
                atomicAdd(&a.frame_bytes[kf], ((before & kCtrBitsMask) + bits + 7ull) >> 3);
            if constexpr (RD)
                if (jj == 0) atomicAdd(rd_dist + kf, (unsigned long long)rd_part[k * 3] + rd_part[k * 3 + 1] + rd_part[k * 3 + 2]);
        }
    }
    for (uint32_t b = bad_q; b; b &= b - 1u) atomicOr(&a.status[__builtin_ctz(b)], (uint32_t)M1V_STATUS_UNENCODABLE); // (rare)

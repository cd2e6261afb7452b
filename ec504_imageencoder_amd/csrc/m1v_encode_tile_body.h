// ec504_imageencoder_amd/csrc/m1v_encode_tile_body.h — the body of k_encode_tiles and k_encode_surface (m1v_tiles.h), included
// inside each kernel (a shared inline function would do, but the compiler may then number the registers of k_encode_tiles
// differently: its code stays the parent's instruction for instruction this way).  In scope: STAGE8, R (template parameters),
// TileArgs a, and the input layout: BPP (bytes per pixel), SURFACE, ORDER, row_pitch, frame_stride (tile_pixel_rows), FRAME_TABLE, PLANE_TABLE.  The front
// half is named by the macro M1V_FRONT_HALF: tile_pixel_rows, or PlaneFront::run for the plane kernels (m1v_planes.h).
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const Geometry &g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool chroma = wave == 2; // wave-uniform
    constexpr int kStride = STAGE8 ? kStageStride8 : kStageStride16;

    uint32_t *vlc = lds + kTileVlc + wave * kVlcWords, *cnt = lds + kTileCnt, *G = lds + kTileG, *segtab = lds + kTileSegTab, *misc = lds + kTileMisc;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)lds;
    const uint32_t region_off = (uint32_t)kTileFixedWords * 4u + (uint32_t)wave * a.luma_region; // bytes from lds
    uint32_t *image = lds + kTileFixedWords + (2u * a.luma_region + a.chroma_region) / 4u;

    int frame, tile;
    frame_unit_of(blockIdx.x, a.n_frames, a.div_group, a.div_frame, frame, tile);
    // Tile rows are taken in an order that keeps the chroma quirk's re-reads in L2 (tile_row_order_for): the tile's position
    // in that order only decides WHEN it runs; everything it writes is indexed by the tile row itself.
    const int tk = (int)udiv((uint32_t)tile, a.div_cols), tc = tile - tk * a.tile_cols;
    const int tr = (int)a.tile_row_order[tk];
    tile = tr * a.tile_cols + tc;
    int s0 = tc * kTileStrips, m0 = tr * kTileMbRows;
    // (a surface kernel stays in the default rounding mode: the integer row pass, as the size-table kernels)
    const uint8_t *fbase;
    if constexpr (SURFACE && PLANE_TABLE) fbase = plane_table_row(a.rgb, frame); // (the kp_* kernels: the frame's three entries of the plane table)
    else if constexpr (SURFACE && FRAME_TABLE) fbase = frame_table_entry(a.rgb, frame); // (the kt_* kernels: a.rgb is the frame table)
    else if constexpr (SURFACE) fbase = a.rgb + (unsigned long long)frame * frame_stride;
    else fbase = pixel_stage_rounds_down(a.rgb + (unsigned long long)frame * g.frame_bytes, s0, m0);
    const unsigned long long tile_index = (unsigned long long)frame * a.tiles_per_frame + tile;

    // ---- which block a lane owns: strip j and macroblock row m inside the tile, block inside the macroblock (Y0 Y1 Y2 Y3 Cb Cr) ----
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

    // ---- pixel stage (tile_pixel_rows): the wave's own copy of the VLC table is requested first (a wave reads only its own
    //      copy, so the waves of a tile do not meet before the bit counts are exchanged), the image is cleared while the
    //      first rows travel (it is first touched in pass 2, behind the barrier of the bit counts) ----
    TSTAMP_INIT();
    const uint32_t ring = lds0 + region_off; // LDS byte address of this wave's region
    constexpr int kKeep = STAGE8 ? M1V_TILE_KEEP : M1V_TILE_KEEP_WIDE;
    RowStore<kKeep> rows;
    M1V_FRONT_HALF<R, kKeep, !SURFACE, BPP, SURFACE, ORDER>(
        g, fbase, ring, wave, lane, s0, m0, strips_here, comp,
        [&]() {
#pragma unroll
            for (int q = 0; q < kVlcWords / kWave; q++)
                dma4((uint32_t)lane * 4u, lds0 + (uint32_t)(kTileVlc + wave * kVlcWords + q * kWave) * 4u, a.tab->vlc + q * kWave);
        },
        [&]() {
            uint4 *image4 = reinterpret_cast<uint4 *>(image); // 16-byte aligned, a.lds_words % 4 == 0 (configure_path)
            for (int k = tid; k < (a.lds_words >> 2); k += kTileThreads) image4[k] = make_uint4(0u, 0u, 0u, 0u);
        },
        rows, row_pitch);
    const M1V_CONST_AS float *rq_t = reinterpret_cast<const M1V_CONST_AS float *>(reinterpret_cast<uintptr_t>(frame_rq_t(a.rq_all, a.qsel, frame)));
    // every row-step has landed and has been read: the ring's bytes now hold the staged levels of the wave's blocks
    uint32_t *blkp = lds + region_off / 4u + lane * kStride;
    uint32_t lds_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)blkp;
    TSTAMP(2);
    unsigned long long nz_ac;
    const int dc = columns_to_stage<STAGE8, kKeep>(rows, rq_t, lds_addr, nz_ac);
    const unsigned long long nz = nz_ac | (dc != 0 ? 1ull : 0ull);
    TSTAMP(3);
    // The lane's place in the tile, derived again behind the pixel and column stages (from an opaque copy of the lane id, in a
    // volatile statement, which stays behind the volatile wait of the staging: five values less to carry through the stages,
    // whose register budget decides the waves per SIMD)
    int j, m, blk;
    {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        owner(ln, j, m, blk);
    }
    const bool valid = j < strips_here && m0 + m < g.n_mbrows;
    const int e = j * kTileSegBlocks + m * 6 + blk; // position in the tile's emission order (strip, macroblock, block)

    // ---- entropy pass 1 (private: own staged levels, shared read-only VLC table) ----
    auto fetch = [&](int p) -> int { return tile_fetch_level<STAGE8>(blkp, (uint32_t)p); };
    uint32_t hdr = 0, bad = 0;
    int hlen = 0;
    BlockBits bb = {0, 0};
    dc_header(dc, blk < 4, blk, vlc, hdr, hlen);
    const unsigned long long emit = emit_set(nz);
    // one coefficient per trip: two per trip (half the dependent LDS round trips) measured no faster in bursts and 1 % slower in
    // a sustained run — the lanes with a single coefficient left do the second one's work for nothing (r03_ab_history.txt)
    tile_bits_pass1<STAGE8>(hdr, hlen, dc != 0, emit, vlc, fetch, bb.acc, bb.tot, bad);
    if (!valid) {
        bb.tot = 0;
        bad = 0;
    }
    cnt[e] = (uint32_t)bb.tot;
    TSTAMP(4);
    lds_barrier();
    TSTAMP(5);

    // ---- every wave scans the 192 counts (emission order) itself: no second barrier ----
    //      (the three reads and their wait in one statement, as the ring reads: one instruction less than three plain reads)
    uint32_t c0;
    unsigned long long c12;
    asm volatile("ds_read_b32 %0, %2\n\tds_read2_b32 %1, %2 offset0:64 offset1:128\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(c0), "=&v"(c12)
                 : "v"(lds0 + (uint32_t)(kTileCnt + lane) * 4u));
    const uint32_t c1 = (uint32_t)c12, c2 = (uint32_t)(c12 >> 32);
    const uint32_t i0 = wave_scan_inclusive(c0), i1 = wave_scan_inclusive(c1), i2 = wave_scan_inclusive(c2);
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)i0, 63), t1 = (uint32_t)__builtin_amdgcn_readlane((int)i1, 63);
    G[lane] = i0 - c0;                 // all three waves store the same values: whichever lands last, a wave reads what
    G[64 + lane] = t0 + i1 - c1;       // it wrote itself
    G[128 + lane] = t0 + t1 + i2 - c2;
    if (lane == 63) G[192] = t0 + t1 + i2;
    // segment table: lanes 0..7 = the tile's strips
    const uint32_t slice_bits = tr == 0 ? 38u : 0u; // the strip starts in this tile: slice header in front (mpeg1_blk.c:12-16)
    const uint32_t gs = G[min(lane, 8) * kTileSegBlocks];
    const uint32_t gs_next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gs, 0x101, 0xf, 0xf, true); // row_shl:1
    const uint32_t seg_bits = lane < strips_here ? slice_bits + (gs_next - gs) : 0u;
    const uint32_t seg_words = lane < 8 ? (seg_bits + 31u) >> 5 : 0u;
    const uint32_t seg_incl = row_scan_inclusive(seg_words);
    const uint32_t end_words = (uint32_t)__builtin_amdgcn_readlane((int)seg_incl, 7);
    if (lane < 8) {
        segtab[2 * lane] = gs;
        segtab[2 * lane + 1] = seg_incl - seg_words;
    }
    const uint32_t my_gs = segtab[2 * j], my_base = segtab[2 * j + 1];
    const uint32_t off = my_base * 32u + slice_bits + (G[e] - my_gs);
    TSTAMP(6);

    auto walk = [&](auto &sink) { tile_walk_codes<STAGE8>(hdr, hlen, dc != 0, emit, vlc, fetch, sink); };
    // The strip's bit total (wave 0, lanes < strips_here): one returning atomic per segment; the tile whose add finds every other
    // tile row of the strip already counted knows the strip's bits and adds its bytes (zero bits pad a strip to a byte,
    // encoder.h:442-443) to the frame's total.  Only the values the atomics return travel between tiles: no fence.
    // (uniform 64-bit bases + 32-bit lane offsets: per-lane 64-bit index products are quarter-rate multiplies)
    unsigned long long *const strip_ctr_s0 = a.strip_ctr + ((unsigned long long)frame * (unsigned)g.n_strips + (unsigned)s0);
    auto strip_arrives = [&](uint32_t bits) -> unsigned long long {
#ifdef M1V_TILE_NOCOMPLETE // timing build (wrong sizes): what the returning atomic and the completion cost
        __hip_atomic_fetch_add(strip_ctr_s0 + lane, (1ull << kCtrCountShift) | (unsigned long long)bits,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return 0ull;
#endif
        return atomicAdd(strip_ctr_s0 + lane, (1ull << kCtrCountShift) | (unsigned long long)bits);
    };
    auto strip_completes = [&](unsigned long long before, uint32_t bits) {
        if ((uint32_t)(before >> kCtrCountShift) == (uint32_t)a.tile_rows - 1u)
            atomicAdd(&a.frame_bytes[frame], ((before & kCtrBitsMask) + bits + 7ull) >> 3);
    };
    // seg[frame][tile row][strip]: the tile's eight entries are 64 contiguous bytes (strip-major they were eight 32-byte
    // sectors 8 * tile_rows bytes apart: 256 bytes of write traffic for 64)
    uint2 *seg_out = a.seg + (((unsigned long long)frame * (unsigned)a.tile_rows + (unsigned)tr) * (unsigned)g.n_strips + (unsigned)s0) + lane; // lanes < strips_here
    auto slice_headers = [&](uint32_t *img, bool swapped) { // wave 0, lanes < strips_here
        if (tr == 0) {
            const uint32_t h0 = slice_word0(s0 + lane), h1 = kSliceWord1, w = seg_incl - seg_words;
            atomicOr(&img[w], swapped ? __builtin_bswap32(h0) : h0);
            atomicOr(&img[w + 1], swapped ? __builtin_bswap32(h1) : h1);
        }
    };

    // ---- image too large for LDS (rare): global atomics in a worst-case slot of the overflow arena ----
    if (end_words + 2 > (uint32_t)a.lds_words) {
        if (tid == 0) misc[0] = atomicAdd(a.arena_next, 1u);
        __syncthreads();
        const uint32_t got = misc[0];
        if (got >= a.arena_slots) { // arena exhausted: the caller re-encodes after m1v_reserve_scratch
            if (tid == 0) atomicOr(a.status, (uint32_t)M1V_STATUS_SCRATCH);
            if (wave == 0 && lane < strips_here) {
                *seg_out = make_uint2(0u, 0u);
                strip_completes(strip_arrives(0u), 0u); // sizes stay consistent; the batch is flagged and encoded again
            }
            return;
        }
        const unsigned long long where = a.arena_off + (unsigned long long)got * a.run_cap;
        uint32_t *big = reinterpret_cast<uint32_t *>(a.scratch + where);
        for (uint32_t i = tid; i < (a.run_cap >> 2); i += kTileThreads) big[i] = 0;
        __syncthreads();
        if (wave == 0 && lane < strips_here) {
            slice_headers(big, true);
            *seg_out = make_uint2(seg_bits, (uint32_t)(where >> 2) + (seg_incl - seg_words));
            strip_completes(strip_arrives(seg_bits), seg_bits);
        }
        if (valid) put_block<true>(big, off, bb, walk);
        if (bad) atomicOr(a.status, (uint32_t)M1V_STATUS_UNENCODABLE);
        return;
    }

    // ---- common path: OR the bits into the LDS image, store it once to the tile's compact slot ----
    unsigned long long arrived = 0; // requested here, looked at behind pass 2 and the store
    if (wave == 0 && lane < strips_here) {
        slice_headers(image, false);
        *seg_out = make_uint2(seg_bits, (uint32_t)((tile_index * a.slot_bytes) >> 2) + (seg_incl - seg_words));
        arrived = strip_arrives(seg_bits);
    }
    if (valid) put_block<false>(image, off, bb, walk);
    TSTAMP(7);
    lds_barrier();
    TSTAMP(8);
    // (in front of the stores: the answer has been back since pass 2, and waiting for it here does not wait for the stores)
    if (wave == 0 && lane < strips_here) strip_completes(arrived, seg_bits);
    uint32_t *slot32 = reinterpret_cast<uint32_t *>(a.scratch + tile_index * a.slot_bytes);
    for (uint32_t i = tid; i < end_words; i += kTileThreads) slot32[i] = __builtin_bswap32(image[i]);
    if (bad) atomicOr(a.status, (uint32_t)M1V_STATUS_UNENCODABLE);
    TSTAMP(9);
    TSTAMP_FLUSH();

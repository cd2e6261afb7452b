// ec504_imageencoder_amd/csrc/m1v_runtime.h — the C-ABI of include/mpeg1_hip.h around the plan and the launches of
// m1v_kernels.hip: object lifetime, buffer allocation, counters (an alloc / clear / free trio per kind), streams and events, the
// quality, size-table and rate entry points, delivery, the host path, profiling and the debug hooks.  The calls that take
// candidates share one argument check (check_candidate_call, the pick-only calls included), one table step (own_table, into the
// encoder's own buffers), one description of the table a pick reads (PickTable, the encoder's own or the caller's) and one launch
// site per pick kernel; what writes a batch's per-frame selection reaches encode_batch as a Selection (the select_by_* steps; a
// batch of many streams, m1v_streams.h, is one too: select_streams in front of the encode kernel, finish_streams behind k_assemble;
// with a budget per stream, m1v_span_budget.h: select_span_budget in its place).
// The input layouts (packed, surface, plane / sample, RGB plane, float plane, float pixel): a setter, a getter and a preset each, the
// two table modes and the two to-bytes calls; what differs per kind beyond a setter's own checks is a row of kind_facts.
// Geometry (CodedRegion, TileGrid, wave_region), the kernel registry (kKernels), the layout record with kind_facts and float_format,
// and the hook predicates of m1v_encoder come from m1v_kernels.hip.  Not standalone: included once, at the end of m1v_kernels.hip.

namespace {

// scaled quantiser matrix, image_processing.c:314-343 (float scale factor, double division,
// round half away from zero, floor of 1)
void scaled_matrix(int qf, int q[64]) {
    static const unsigned char base[64] = {
        8,  16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34,
        34, 38, 22, 22, 26, 27, 29, 34, 37, 40, 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32,
        35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83};
    if (qf < 1) qf = 1;
    if (qf > 100) qf = 100;
    float sf = qf < 50 ? (float)(5000.0 / qf) : (float)(200.0 - 2 * qf);
    for (int k = 0; k < 64; k++) {
        float prod = (float)base[k] * sf;
        int v = (int)round((double)prod / 100.0);
        q[k] = v < 1 ? 1 : v;
    }
}

// The VLC table of the kernels (layout: kVlc*).  Run/level code words without sign bit as the reference stores them
// (vlc.c:176-288), in its order, with its offset index (vlc.c:172-174); the reference's indexing rule (vlc.c:329-339)
// reads row r = run - 1 at |level| - 1, so in row 0 entry idx codes level idx + 2 — except idx 0, which the rule
// replaces by the special "11" and which is therefore stored that way here.  DC size codes: vlc.c:121-144.
void build_vlc_table(uint32_t t[kVlcWords]) {
    static const unsigned char row_len[32] = {39, 18, 5, 4, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2,
                                              2,  1,  1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    static const unsigned char code[110] = {
        0x04, 0x05, 0x06, 0x26, 0x21, 0x0a, 0x1d, 0x18, 0x13, 0x10, 0x1a, 0x19, 0x18, 0x17, 0x1f, 0x1e,
        0x1d, 0x1c, 0x1b, 0x1a, 0x19, 0x18, 0x17, 0x16, 0x15, 0x14, 0x13, 0x12, 0x11, 0x10, 0x18, 0x17,
        0x16, 0x15, 0x14, 0x13, 0x12, 0x11, 0x10, 0x03, 0x06, 0x25, 0x0c, 0x1b, 0x16, 0x15, 0x1f, 0x1e,
        0x1d, 0x1c, 0x1b, 0x1a, 0x19, 0x13, 0x12, 0x11, 0x10, 0x05, 0x04, 0x0b, 0x14, 0x14, 0x07, 0x24,
        0x1c, 0x13, 0x06, 0x0f, 0x12, 0x07, 0x09, 0x12, 0x05, 0x1e, 0x14, 0x04, 0x15, 0x07, 0x11, 0x05,
        0x11, 0x27, 0x10, 0x23, 0x1a, 0x22, 0x19, 0x20, 0x18, 0x0e, 0x17, 0x0d, 0x16, 0x08, 0x15, 0x1f,
        0x1a, 0x19, 0x17, 0x16, 0x1f, 0x1e, 0x1d, 0x1c, 0x1b, 0x1f, 0x1e, 0x1d, 0x1c, 0x1b};
    static const unsigned char bits[110] = {
        4,  5,  7,  8,  8,  10, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 14, 14,
        14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3,  6,  8,  10, 12,
        13, 13, 15, 15, 15, 15, 15, 15, 15, 16, 16, 16, 16, 4,  7,  10, 12, 13, 5,  8,  12, 13,
        5,  10, 12, 6,  10, 13, 6,  12, 16, 6,  12, 7,  12, 7,  13, 8,  13, 8,  16, 8,  16, 8,
        16, 10, 16, 10, 16, 10, 15, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 16, 16, 16, 16, 16};
    memset(t, 0, kVlcWords * sizeof(uint32_t));
    int first = 0;
    for (int r = 0; r < kAcRows; r++) {
        t[kVlcRowInfo + r] = (uint32_t)first | ((uint32_t)row_len[r] << 8);
        first += row_len[r];
    }
    for (int e = 0; e < 110; e++) t[kVlcEntries + e] = ((uint32_t)bits[e] << 16) | code[e];
    t[kVlcEntries] = (2u << 16) | 0x3u; // run 1, |level| 1 -> "11" (vlc.c:329-334 with first == 0)
    static const unsigned char lc[9] = {0x4, 0x0, 0x1, 0x5, 0x6, 0xE, 0x1E, 0x3E, 0x7E};
    static const unsigned char lb[9] = {3, 2, 2, 3, 3, 4, 5, 6, 7};
    static const unsigned char cc[9] = {0x0, 0x1, 0x2, 0x6, 0xE, 0x1E, 0x3E, 0x7E, 0xFE};
    static const unsigned char cb[9] = {2, 2, 2, 3, 4, 5, 6, 7, 8};
    for (int i = 0; i < 9; i++) {
        t[kVlcDcLuma + i] = ((uint32_t)lb[i] << 16) | lc[i];
        t[kVlcDcChroma + i] = ((uint32_t)cb[i] << 16) | cc[i];
    }
}

void put_timestamp(uint8_t *o, uint8_t prefix, uint32_t v) { // mpeg1_enc.c:59-64, :67-71
    o[0] = (uint8_t)(prefix | ((v & 0xe0000000u) >> 28));
    o[1] = (uint8_t)((v & 0x1fe00000u) >> 21);
    o[2] = (uint8_t)(0x01 | ((v & 0x001fc000u) >> 13));
    o[3] = (uint8_t)((v & 0x00003fc0u) >> 6);
    o[4] = (uint8_t)(0x01 | ((v & 0x0000003fu) << 1));
}

// PKT(16) SEQ(12) GOP(8) PIC(8) of the frame whose uint8 `hour` is given (encoder.h:37-63,186-230)
void build_frame_header(uint8_t h[44], int W, int H, int hour) {
    memset(h, 0, 44);
    h[2] = 0x01; h[3] = 0xe0;                                  // packet, stream id 0 (mpeg1_enc.c:47-77)
    uint32_t ts = (uint32_t)(1 + 3600 * hour);
    ts = (uint32_t)((double)ts * 1.2);
    ts += 0xbeef;
    put_timestamp(h + 6, 0x31, ts);
    ts -= 0xbeef;
    put_timestamp(h + 11, 0x11, ts);
    uint8_t *s = h + 16;                                       // sequence (mpeg1_enc.c:81-94)
    unsigned w = (unsigned)W & 0xffu, hh = (unsigned)H & 0xffu; // uint8_t width/height, encoder.h:186-187
    s[2] = 0x01; s[3] = 0xb3;
    s[4] = (uint8_t)((w & 0xff0) >> 4);
    s[5] = (uint8_t)(((w & 0xf) << 4) | ((hh & 0xf00) >> 8));
    s[6] = (uint8_t)(hh & 0xff);
    s[7] = 0x14; s[8] = 0xff; s[9] = 0xff; s[10] = 0xe0; s[11] = 0x18;
    uint8_t *g = h + 28;                                       // GOP (mpeg1_enc.c:103-113)
    g[2] = 0x01; g[3] = 0xb8;
    g[4] = (uint8_t)((hour & 0x1f) << 2);
    g[5] = 0x08; g[6] = 0x00; g[7] = 0x40;
    uint8_t *p = h + 36;                                       // picture (mpeg1_enc.c:120-129)
    p[2] = 0x01; p[3] = 0x00; p[4] = 0x00; p[5] = 0x0f; p[6] = 0xff; p[7] = 0xf8;
}

} // namespace

template <typename T>
static hipError_t ensure_device(T **p, size_t *cap, size_t need) {
    if (need <= *cap) return hipSuccess;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t err = hipMalloc(p, need);
    if (err == hipSuccess) *cap = need;
    return err;
}

static int g_fail_alloc_in = 0; // test hook (m1v_debug_fail_alloc): the n-th allocation of configure_path from now fails
template <typename T>
static hipError_t plan_malloc(T **p, size_t bytes) {
    if (g_fail_alloc_in > 0 && --g_fail_alloc_in == 0) return hipErrorOutOfMemory;
    return hipMalloc(p, bytes);
}
static int g_fail_encode_at = 0; // test hook (m1v_debug_fail_encode): the stage at which the next encode returns M1V_E_HIP
static int fail_encode_at(int stage) {
    if (g_fail_encode_at != stage) return M1V_OK;
    g_fail_encode_at = 0;
    return fail(M1V_E_HIP, "injected failure (m1v_debug_fail_encode)%s");
}

// A counter set: cleared in full on a stream; allocated (through plan_malloc) and cleared before the allocation returns; freed.
static hipError_t counters_clear(const m1v_encoder *e, m1v_encoder::Counters &c, hipStream_t st) {
    c.dirty_frames = 0;
    hipError_t err = hipMemsetAsync(c.strip_ctr, 0, (size_t)e->max_frames * e->g.n_strips * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(c.frame_bytes, 0, (size_t)e->max_frames * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(c.words, 0, 4 * sizeof(uint32_t), st);
    return err; // (frame_index holds no count: every streams batch writes what it reads)
}
static bool counters_alloc(const m1v_encoder *e, m1v_encoder::Counters &c) {
    return plan_malloc(&c.strip_ctr, (size_t)e->max_frames * e->g.n_strips * 8) == hipSuccess &&
           plan_malloc(&c.frame_bytes, (size_t)e->max_frames * 8) == hipSuccess && plan_malloc(&c.words, 4 * sizeof(uint32_t)) == hipSuccess &&
           plan_malloc(&c.frame_index, (size_t)e->max_frames * sizeof(int32_t)) == hipSuccess &&
           hipMemsetAsync(c.frame_index, 0, (size_t)e->max_frames * sizeof(int32_t), nullptr) == hipSuccess &&
           counters_clear(e, c, nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
}
static void counters_free(m1v_encoder::Counters &c) {
    (void)hipFree(c.strip_ctr);
    (void)hipFree(c.frame_bytes);
    (void)hipFree(c.words);
    (void)hipFree(c.frame_index);
}

// The size table's counters: the same three and the rd table's distortion sums (allocated by m1v_create, so not through plan_malloc)
static hipError_t table_clear(const m1v_encoder *e, hipStream_t st) {
    const m1v_encoder::TableCounters &t = e->table;
    const size_t kf = (size_t)kMaxCandidates * e->max_frames;
    hipError_t err = hipMemsetAsync(t.strip_ctr, 0, kf * e->g.n_strips * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(t.frame_bytes, 0, kf * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(t.frame_dist, 0, kf * 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(t.words, 0, kMaxCandidates * sizeof(uint32_t), st);
    return err;
}
static hipError_t table_alloc(m1v_encoder *e) {
    m1v_encoder::TableCounters &t = e->table;
    const size_t kf = (size_t)kMaxCandidates * e->max_frames;
    hipError_t err = hipMalloc(&t.strip_ctr, kf * e->g.n_strips * 8);
    if (err == hipSuccess) err = hipMalloc(&t.frame_bytes, kf * 8);
    if (err == hipSuccess) err = hipMalloc(&t.frame_dist, kf * 8);
    if (err == hipSuccess) err = hipMalloc(&t.words, kMaxCandidates * sizeof(uint32_t));
    if (err == hipSuccess) err = table_clear(e, nullptr);
    return err == hipSuccess ? hipStreamSynchronize(nullptr) : err;
}
static void table_free(m1v_encoder::TableCounters &t) {
    (void)hipFree(t.strip_ctr);
    (void)hipFree(t.frame_bytes);
    (void)hipFree(t.frame_dist);
    (void)hipFree(t.words);
}

// A constant table of m1v_create: allocated and uploaded
template <typename T>
static hipError_t upload(T **dst, const T *src, size_t count) {
    const hipError_t err = hipMalloc(dst, count * sizeof(T));
    return err == hipSuccess ? hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice) : err;
}

static void batch_free(m1v_encoder::Batch &bt) {
    (void)hipFree(bt.scratch);
    (void)hipFree(bt.run_meta);
    (void)hipFree(bt.seg);
    for (m1v_encoder::Counters &c : bt.ctr) counters_free(c);
    if (bt.enc_done) (void)hipEventDestroy(bt.enc_done);
    if (bt.gather_done) (void)hipEventDestroy(bt.gather_done);
}

static int profile_event(m1v_encoder *e, hipStream_t st) {
    if (e->ev_used == e->ev.size()) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        e->ev.push_back(ev);
    }
    HIP_TRY(hipEventRecord(e->ev[e->ev_used++], st));
    return M1V_OK;
}

// The launches profiled since the last read: their count, their sum and the first `cap` of their times; forgets them.
static int profile_times(m1v_encoder *e, float *ms, int cap, int *launches, double *total_ms) {
    HIP_TRY(hipSetDevice(e->device));
    double sum = 0;
    int n = 0;
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(e->ev[i + 1]));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e->ev[i], e->ev[i + 1]));
        if (n < cap) ms[n] = t;
        sum += t;
        n++;
    }
    e->ev_used = 0;
    if (launches) *launches = n;
    if (total_ms) *total_ms = sum;
    return M1V_OK;
}

// Makes the encoder's plan (plan_for) and (re)allocates what it needs.  New buffers are allocated FIRST and swapped in, together
// with the plan they belong to, only when every allocation has succeeded: a failed call (the worst-case arena of
// m1v_reserve_scratch is large) leaves the encoder as it was.  Every device allocation goes through plan_malloc: the
// fault-injection hook reaches all of them.
static int configure_path(m1v_encoder *e) {
    Plan p;
    if (const int rc = plan_for(*e, p)) return rc;
    const int sets = e->pipelined ? 2 : 1;
    struct Fresh {
        m1v_encoder::Batch b;
        bool new_scratch, new_meta, new_seg, new_fixed;
    } fresh[2] = {};
    uint32_t *fresh_order = nullptr;
    const bool new_order = p.tile_rows != 0 && e->tile_order_rows != p.tile_rows; // the tile kernel's and the fused size table's
    bool ok = true;
    for (int i = 0; i < sets && ok; i++) {
        const m1v_encoder::Batch &bt = e->batch[i];
        Fresh &f = fresh[i];
        f.new_scratch = p.scratch_bytes != bt.scratch_bytes || !bt.scratch;
        f.new_meta = p.meta_bytes != 0 && (p.meta_bytes != bt.meta_bytes || !bt.run_meta); // (tiles and strips keep the array)
        f.new_seg = p.seg_bytes != bt.seg_bytes || !bt.seg;
        f.new_fixed = !bt.enc_done;
        if (f.new_scratch) ok = plan_malloc(&f.b.scratch, p.scratch_bytes) == hipSuccess;
        if (ok && f.new_meta) ok = plan_malloc(&f.b.run_meta, p.meta_bytes) == hipSuccess;
        if (ok && f.new_seg) ok = plan_malloc(&f.b.seg, p.seg_bytes) == hipSuccess;
        if (ok && f.new_fixed) {
            for (m1v_encoder::Counters &c : f.b.ctr) ok = ok && counters_alloc(e, c);
            ok = ok && hipEventCreateWithFlags(&f.b.gather_done, hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&f.b.enc_done, hipEventDisableTiming) == hipSuccess;
        }
    }
    if (ok && new_order) {
        std::vector<uint32_t> order;
        tile_row_order_for(p.tile_rows, order);
        ok = plan_malloc(&fresh_order, order.size() * sizeof(uint32_t)) == hipSuccess &&
             hipMemcpy(fresh_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        for (Fresh &f : fresh) batch_free(f.b);
        (void)hipFree(fresh_order);
        (void)hipGetLastError();
        return fail(M1V_E_HIP, "allocation failed (the encoder keeps its previous configuration)%s");
    }
    // ---- commit ----
    for (int i = 0; i < sets; i++) {
        m1v_encoder::Batch &bt = e->batch[i];
        Fresh &f = fresh[i];
        if (f.new_scratch) {
            (void)hipFree(bt.scratch);
            bt.scratch = f.b.scratch;
            bt.scratch_bytes = p.scratch_bytes;
        }
        if (f.new_meta) {
            (void)hipFree(bt.run_meta);
            bt.run_meta = f.b.run_meta;
            bt.meta_bytes = p.meta_bytes;
        }
        if (f.new_seg) {
            (void)hipFree(bt.seg);
            bt.seg = f.b.seg;
            bt.seg_bytes = p.seg_bytes;
        }
        if (f.new_fixed) {
            bt.ctr[0] = f.b.ctr[0];
            bt.ctr[1] = f.b.ctr[1];
            bt.turn = 0;
            bt.poisoned = false;
            bt.enc_done = f.b.enc_done;
            bt.gather_done = f.b.gather_done;
        }
    }
    if (new_order) {
        (void)hipFree(e->d_tile_order);
        e->d_tile_order = fresh_order;
        e->tile_order_rows = p.tile_rows;
    }
    e->plan = p;
    return M1V_OK;
}

// A setting that changes the plan: set behind everything queued on the device, and put back when the new plan cannot be set up
template <typename T>
static int reconfigure(m1v_encoder *e, T m1v_encoder::*field, T value) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const T before = e->*field;
    e->*field = value;
    const int rc = configure_path(e);
    if (rc != M1V_OK) e->*field = before;
    return rc;
}

// What takes packed input only: the entry points that do not go through the producer / table kernels, and the hooks that force
// the run kernels
static int packed_only(const m1v_encoder *e) {
    if (!e->layout.tiles_only()) return M1V_OK;
    const KindFacts f = kind_facts(e->layout.kind);
    return fail(M1V_E_ARG, "packed input only: %s is set (%s)", f.name, f.setter);
}

// A getter that cannot describe the layout in force names the one that can
static int ask_its_getter(const m1v_encoder *e) {
    const KindFacts f = kind_facts(e->layout);
    return fail(M1V_E_ARG, "%s is in force: ask %s", f.name, f.getter);
}

// The preamble of the getters of Y, Cb, Cr layouts: 1 = a plane or sample layout is in force, 0 = none is (packed or surface input),
// else the refusal that names the getter to ask
static int samples_in_force(const m1v_encoder *e) {
    const int answer = kind_facts(e->layout).plane_getters;
    return answer < 0 ? ask_its_getter(e) : answer;
}

// What rows of `row` bytes that lie `pitch` apart must satisfy in the surface, float pixel and downscale setters: a pitch not below the row,
// the rows of a frame (`what` the refusal calls them) below 4 GiB, a frame stride not below them
static int rows_fit(unsigned long long pitch, unsigned long long row, unsigned long long H, unsigned long long frame_stride,
                    const char *pitch_below_row, const char *what, const char *stride_below_rows) {
    if (pitch < row) return fail(M1V_E_ARG, "%s", pitch_below_row);
    const unsigned long long limit = 1ull << 32, extent = (H - 1) * pitch + row;
    if (pitch >= limit || extent >= limit) return fail(M1V_E_ARG, "a %s of 4 GiB or more (byte offsets inside a frame are 32-bit)", what);
    if (frame_stride < extent) return fail(M1V_E_ARG, "%s", stride_below_rows);
    return M1V_OK;
}

// The launches behind the to-bytes calls, 65535 frames (a grid's y extent) each: `kind` must be in force (`needs`: the refusal
// where it is not); kernels: the call's kernel per M1V_SAMPLE_* value; args(frames, bytes): its argument struct for the frames from
// `frames` on, written from `bytes` on; grid: the launch over n frames
template <typename MakeArgs, typename Grid>
static int float_to_bytes(m1v_encoder *e, LayoutKind kind, const char *needs, const void *const (&kernels)[3], const void *d_frames,
                          int n_frames, uint8_t *d_bytes, void *stream, MakeArgs args, Grid grid) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != kind) return fail(M1V_E_ARG, "%s", needs);
    if (n_frames < 0 || ((!d_frames || !d_bytes) && n_frames > 0)) return fail(M1V_E_ARG, "null pointer or negative n_frames%s");
    if (const int rc = check_frame_table(e, static_cast<const uint8_t *>(d_frames))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const unsigned long long frame_out = 3ull * (unsigned)e->g.W * (unsigned)e->g.H;
    for (int done = 0; done < n_frames; done += 65535) {
        auto a = args(static_cast<const uint8_t *>(d_frames) + (unsigned long long)done * e->layout.frame_stride, d_bytes + (unsigned long long)done * frame_out);
        void *argv[] = {&a};
        HIP_TRY(hipLaunchKernel(kernels[e->layout.fmt.sample], grid((unsigned)std::min(n_frames - done, 65535)), dim3(256u), argv, 0, (hipStream_t)stream));
    }
    return M1V_OK;
}

// The shared tail of the layout setters, behind their argument checks: a layout of the tile kernels and a hook that forces the run
// kernels refuse each other; then the new plan, or the layout that was in force
static int apply_layout(m1v_encoder *e, const m1v_encoder::Layout &want) {
    if (want.tiles_only() && e->run_hook_set())
        return fail(M1V_E_ARG, "a debug hook has forced this encoder to the run kernels, which take packed input only%s");
    return reconfigure(e, &m1v_encoder::layout, want);
}

extern "C" {

const char *m1v_last_error(void) { return g_err; }

int m1v_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int m1v_warm_up(int device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(nullptr)); // creates the context
    hipFuncAttributes attr;    // loads this library's code object for the device
    HIP_TRY(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_assemble<false>)));
    return M1V_OK;
}

size_t m1v_file_prolog(uint8_t out[27]) {
    static const uint8_t pack[9] = {0x00, 0x00, 0x01, 0xba, 0x21, 0x00, 0x01, 0x00, 0x01};
    memcpy(out, pack, 9);
    uint32_t rate = (2202035u & 0x3fffffu) | 0x400000u; // mpeg1_enc.c:14-16
    rate = (rate << 1) | 1u;
    out[9] = (uint8_t)(rate >> 16); out[10] = (uint8_t)(rate >> 8); out[11] = (uint8_t)rate;
    uint8_t *s = out + 12;                                 // mpeg1_enc.c:24-44, packet_num 0xe6
    s[0] = 0; s[1] = 0; s[2] = 1; s[3] = 0xbb; s[4] = 0; s[5] = 9;
    s[6] = (uint8_t)(rate >> 16); s[7] = (uint8_t)(rate >> 8); s[8] = (uint8_t)rate;
    s[9] = 0; s[10] = 0x21; s[11] = 0xff; s[12] = 0xe0; s[13] = 0xe0; s[14] = 0xe6;
    return 27;
}

int m1v_create(m1v_encoder **out, int device, int width, int height, int channels,
               int quality_factor, int mode, int max_frames) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    *out = nullptr;
    if (width <= 0 || height <= 0 || channels < 3 || channels > 4 || max_frames <= 0)
        return fail(M1V_E_ARG, "bad geometry%s");
    if (mode != M1V_MODE_STRICT && mode != M1V_MODE_FULL) return fail(M1V_E_ARG, "bad mode%s");
    const CodedRegion coded(width, height, mode);
    if (!coded.fits(width, height)) return fail(M1V_E_ARG, "picture smaller than the 96x144 region the reference encodes%s");
    if (coded.xe == 0 || coded.ye == 0) return fail(M1V_E_ARG, "picture smaller than one macroblock%s");
    if ((unsigned long long)width * height * channels >= (1ull << 32))
        return fail(M1V_E_ARG, "a frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
    int n = m1v_device_count();
    if (n <= 0) return fail(M1V_E_NODEVICE, "no HIP device%s");
    if (device < 0 || device >= n) return fail(M1V_E_ARG, "device index out of range%s");
    HIP_TRY(hipSetDevice(device));
    int grid_y = 0, grid_z = 0;
    HIP_TRY(hipDeviceGetAttribute(&grid_y, hipDeviceAttributeMaxGridDimY, device));
    HIP_TRY(hipDeviceGetAttribute(&grid_z, hipDeviceAttributeMaxGridDimZ, device));

    m1v_encoder *e = new m1v_encoder();
    e->device = device;
    e->batch_limit = std::min(grid_y, grid_z);
    e->qf = quality_factor;
    e->mode = mode;
    e->max_frames = max_frames;
    Geometry &g = e->g;
    g.W = width; g.H = height; g.C = channels;
    g.n_strips = coded.xe / 16; g.n_mbrows = coded.ye / 16;
    g.half_w = width / 2;
    g.frame_bytes = (unsigned long long)width * height * channels;
    g.strip_cap = (uint32_t)((((coded.strip_bits() + 7) / 8) + 16 + 15) & ~15ull);
    e->dense = g.n_mbrows * 6 >= kWave;
    e->fast_ok = channels == 3 && (width % 8) == 0;

    // Per-frame quality: the transposed reciprocal table of every quality ([100][64], frame_rq_t); Tables::rq_t is the row of the
    // encoder's own quality, Tables::rq that row in natural order
    const int own = encoder_quality(e);
    std::vector<float> rq_all(100 * 64), dq_all(100 * 64); // (dq_all: the divisors themselves, for the rd table)
    int min_ac = 0;
    for (int qf = 1; qf <= 100; qf++) {
        int q[64];
        scaled_matrix(qf, q);
        for (int u = 0; u < 8; u++)
            for (int i = 0; i < 8; i++) {
                rq_all[(size_t)(qf - 1) * 64 + i * 8 + u] = (float)((1.0 / q[u * 8 + i]) * (1.0 + 1.0 / 1048576.0));
                dq_all[(size_t)(qf - 1) * 64 + i * 8 + u] = (float)q[u * 8 + i];
            }
        const int ac = *std::min_element(q + 1, q + 64);
        if (qf == own) min_ac = ac;
        if (ac >= 8) e->narrow_q = qf; // (the divisors shrink as the quality grows)
    }
    // One byte per staged level is exact iff no AC level can reach +-128.  |AC coefficient| of the
    // reference's FDCT on u8 pixels is at most 1022 (127.5 * 8 + the +2 rounding bias, reached at (0,4), (4,0),
    // (4,4); tests/test_host_tables.py::test_fdct_output_range), so 128 * (smallest AC divisor) >= 1024
    // suffices: quality factors <= 76.
    e->narrow = min_ac >= 8;
    Tables *t = new Tables();
    const float *rq_t = &rq_all[(size_t)(own - 1) * 64];
    memcpy(t->rq_t, rq_t, sizeof t->rq_t);
    for (int u = 0; u < 8; u++)
        for (int i = 0; i < 8; i++) t->rq[u * 8 + i] = rq_t[i * 8 + u];
    build_vlc_table(t->vlc);
    for (int h = 0; h < 256; h++) build_frame_header(t->hdr[h], width, height, h);
    const std::vector<uint32_t> sel((size_t)max_frames, (uint32_t)(own - 1) * 64u);

    hipError_t err = upload(&e->d_tab, t, 1);
    delete t;
    if (err == hipSuccess) err = upload(&e->d_rq_all, rq_all.data(), rq_all.size());
    if (err == hipSuccess) err = upload(&e->d_dq_all, dq_all.data(), dq_all.size());
    if (err == hipSuccess) err = upload(&e->d_qsel_own, sel.data(), sel.size());
    if (err == hipSuccess) err = upload(&e->d_qsel, sel.data(), sel.size());
    if (err == hipSuccess) err = hipMalloc(&e->d_probe_sizes, (size_t)kMaxCandidates * max_frames * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMalloc(&e->d_probe_dist, (size_t)kMaxCandidates * max_frames * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMalloc(&e->d_rd_steps, (size_t)kMaxCandidates * max_frames * sizeof(RdStep));
    if (err == hipSuccess) err = hipMalloc(&e->d_span_chunks, (M1V_MAX_STREAMS + 1) * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc(&e->d_probe_status, kMaxCandidates * sizeof(uint32_t));
    if (err == hipSuccess) err = hipMalloc(&e->d_chosen, (size_t)max_frames);
    if (err == hipSuccess) err = hipMalloc(&e->d_pick_status, sizeof(uint32_t));
    if (err == hipSuccess) err = table_alloc(e);
#if defined(M1V_STAMPS) || defined(M1V_TILE_STAMPS) || defined(M1V_ASM_STAMPS)
    if (err == hipSuccess) err = hipMalloc(&e->d_stamps, (32 + 8 * 65536) * 8); // [32] phase sums, then a timeline of 8 stamps per workgroup
    if (err == hipSuccess) err = hipMemset(e->d_stamps, 0, (32 + 8 * 65536) * 8);
#endif
    if (err == hipSuccess) err = configure_path(e) == M1V_OK ? hipSuccess : hipErrorOutOfMemory;
    const void *const *registered = &kKernels.tile[0][0][0]; // (Kernels holds nothing but kernels)
    for (size_t k = 0; k < sizeof kKernels / sizeof *registered; k++)
        if (err == hipSuccess && registered[k]) err = hipFuncSetAttribute(registered[k], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (err != hipSuccess) {
        fail(M1V_E_HIP, "allocation failed: %s", hipGetErrorString(err));
        m1v_destroy(e);
        return M1V_E_HIP;
    }
    *out = e;
    return M1V_OK;
}

void m1v_destroy(m1v_encoder *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    for (hipEvent_t ev : e->ev) (void)hipEventDestroy(ev);
    (void)hipFree(e->d_tab);
    (void)hipFree(e->d_rq_all);
    (void)hipFree(e->d_dq_all);
    (void)hipFree(e->d_qsel_own);
    (void)hipFree(e->d_qsel);
    (void)hipFree(e->d_probe_sizes);
    (void)hipFree(e->d_probe_dist);
    (void)hipFree(e->d_rd_steps);
    (void)hipFree(e->d_span_chunks);
    (void)hipFree(e->d_probe_status);
    (void)hipFree(e->d_chosen);
    (void)hipFree(e->d_pick_status);
    table_free(e->table);
    for (m1v_encoder::Batch &bt : e->batch) batch_free(bt);
    if (e->side) (void)hipStreamDestroy(e->side);
    (void)hipFree(e->hp.d_in);
    (void)hipFree(e->hp.d_out);
    (void)hipFree(e->hp.d_planes);
    (void)hipFree(e->hp.d_meta);
    if (e->hp.copy_in) (void)hipStreamDestroy(e->hp.copy_in);
    if (e->hp.work) (void)hipStreamDestroy(e->hp.work);
    for (hipEvent_t ev : e->hp.uploaded)
        if (ev) (void)hipEventDestroy(ev);
    (void)hipFree(e->d_stamps);
    (void)hipFree(e->d_tile_order);
    delete e;
}

int m1v_batch_limit(const m1v_encoder *e) { return e ? std::min(e->max_frames, e->batch_limit) : 0; }
int m1v_strips(const m1v_encoder *e) { return e ? e->g.n_strips : 0; }
int m1v_mb_rows(const m1v_encoder *e) { return e ? e->g.n_mbrows : 0; }
size_t m1v_frame_bytes_in(const m1v_encoder *e) { return e ? (size_t)e->g.frame_bytes : 0; }

size_t m1v_frame_bound_for(int width, int height, int mode) {
    const CodedRegion coded(width, height, mode);
    if (width <= 0 || height <= 0 || coded.xe <= 0 || coded.ye <= 0 || !coded.fits(width, height)) return 0;
    return 44 + (size_t)(coded.xe / 16) * (size_t)((coded.strip_bits() + 7) / 8) + 4;
}

size_t m1v_frame_bound(const m1v_encoder *e) { return e ? m1v_frame_bound_for(e->g.W, e->g.H, e->mode) : 0; }

int m1v_debug_set_lds_words(m1v_encoder *e, int words) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    // (a small forced image sends many units to the overflow arena: M1V_STATUS_SCRATCH)
    return reconfigure(e, &m1v_encoder::lds_words, words > 0 ? (words < 4 ? 4 : words) : 0);
}

int m1v_reserve_scratch(m1v_encoder *e, int worst_case) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->plan.producer == Producer::strips) return M1V_OK;
    return reconfigure(e, &m1v_encoder::reserve_worst, worst_case != 0); // (on failure the previous arena is still in place)
}

size_t m1v_scratch_bytes(const m1v_encoder *e) { return e ? e->plan.scratch_bytes * (e->pipelined ? 2 : 1) : 0; }

int m1v_set_pipelined(m1v_encoder *e, int enable) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    for (m1v_encoder::Batch &bt : e->batch) bt.gather_pending = false;
    e->calls = 0;
    if (enable && !e->side) {
        // highest priority: the few memory-bound workgroups of layout + gather should take the first slots the (much longer,
        // arithmetic-bound) encode kernel of the next batch frees, not queue behind its whole grid
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, greatest));
    }
    // (when the second set of buffers cannot be allocated the encoder stays as it was)
    return reconfigure(e, &m1v_encoder::pipelined, enable != 0);
}

int m1v_flush(m1v_encoder *e, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    HIP_TRY(hipSetDevice(e->device));
    // The mark stays set: a later m1v_encode_device on ANOTHER stream must still wait for this set's gather before its
    // encode kernel overwrites the scratch (waiting for an event that has completed costs nothing).
    for (m1v_encoder::Batch &bt : e->batch) {
        if (e->pipelined && bt.poisoned) { // a failed call may have left an assembly on the internal stream without its event
            HIP_TRY(hipEventRecord(bt.gather_done, e->side));
            bt.gather_pending = true;
        }
        if (bt.gather_pending) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, bt.gather_done, 0));
    }
    return M1V_OK;
}

int m1v_debug_set_input_mode(m1v_encoder *e, int mode) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (mode != -1 && mode != 0 && mode != 2) return fail(M1V_E_ARG, "input mode must be -1 (auto), 0 (byte loads) or 2 (funnel)%s");
    if (mode != -1)
        if (const int rc = packed_only(e)) return rc;
    return reconfigure(e, &m1v_encoder::forced_mode, mode); // an input mode is a property of the run kernels: forcing one selects them
}

int m1v_debug_set_dense_threads(m1v_encoder *e, int threads) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (!e->dense) return M1V_OK;
    if (threads > 0)
        if (const int rc = packed_only(e)) return rc;
    // a run length is a property of the run kernels: forcing one selects them
    return reconfigure(e, &m1v_encoder::forced_T, threads > 0 ? threads : 0);
}

int m1v_debug_set_path(m1v_encoder *e, int path) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (path < -1 || path > 1) return fail(M1V_E_ARG, "path must be -1 (by geometry), 0 (runs) or 1 (tiles)%s");
    if (path == 1 && e->g.C != 3) return fail(M1V_E_ARG, "the tile kernel takes 3-channel pictures%s");
    if (path == 0)
        if (const int rc = packed_only(e)) return rc;
    return reconfigure(e, &m1v_encoder::forced_path, path);
}

int m1v_debug_assemble_shape(const m1v_encoder *e, int out[4]) {
    if (!e || !out) return fail(M1V_E_ARG, "null encoder or output%s");
    out[0] = e->plan.asm_group;
    out[1] = e->plan.asm_lanes_log2;
    out[2] = e->plan.segs;
    out[3] = e->plan.producer == Producer::tiles ? 0 : (e->plan.producer == Producer::dense ? 1 : 2);
    return M1V_OK;
}

int m1v_debug_set_assemble_shape(m1v_encoder *e, int group, int lanes_log2) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    // only what plan_for can produce: the launch and the kernel hold no other shape
    if (group < 0 || group > kAsmMaxGroup || (group & (group - 1)) || group > e->g.n_strips)
        return fail(M1V_E_ARG, "group must be 0 (the plan's own) or a power of two, at most 16 and at most the number of strips%s");
    if (lanes_log2 < 0 || lanes_log2 > 4) return fail(M1V_E_ARG, "lanes_log2 must be 0 (the plan's own) or 1..4%s");
    return reconfigure(e, &m1v_encoder::forced_asm, m1v_encoder::AsmShape{group, lanes_log2});
}

int m1v_set_input_layout(m1v_encoder *e, size_t row_pitch_bytes, size_t frame_stride_bytes, int order) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (order != M1V_ORDER_RGB && order != M1V_ORDER_BGR) return fail(M1V_E_ARG, "order must be M1V_ORDER_RGB or M1V_ORDER_BGR%s");
    const Geometry &g = e->g;
    m1v_encoder::Layout want;
    if (row_pitch_bytes != 0 || frame_stride_bytes != 0 || order != M1V_ORDER_RGB) {
        want.kind = LayoutKind::surface;
        if (g.W & 1) return fail(M1V_E_ARG, "a surface layout needs an even width (the chroma plane is addressed with stride width / 2)%s");
        const unsigned long long row = (unsigned long long)g.W * g.C, pitch = row_pitch_bytes ? row_pitch_bytes : row;
        want.frame_stride = frame_stride_bytes ? frame_stride_bytes : (unsigned long long)g.H * pitch; // (0: the rows, no gap)
        if (const int rc = rows_fit(pitch, row, (unsigned long long)g.H, want.frame_stride, "row pitch below width * channels", "window",
                                    "frame stride below the bytes a frame's window spans"))
            return rc;
        want.surface = {(uint32_t)pitch, order};
    }
    return apply_layout(e, want);
}

int m1v_input_layout(const m1v_encoder *e, size_t *row_pitch_bytes, size_t *frame_stride_bytes, int *order) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    const m1v_encoder::Layout &l = e->layout;
    if (kind_facts(l).plane_getters != 0) return ask_its_getter(e);
    static_assert(M1V_ORDER_RGB == 0, "packed input leaves the record's zeros: (0, 0, M1V_ORDER_RGB)");
    if (row_pitch_bytes) *row_pitch_bytes = l.surface.row_pitch;
    if (frame_stride_bytes) *frame_stride_bytes = (size_t)l.frame_stride;
    if (order) *order = l.surface.order;
    return M1V_OK;
}

int m1v_plane_layout_preset(int width, int height, int preset, m1v_plane_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (preset < M1V_PLANES_REFERENCE || preset > M1V_PLANES_NV21) return fail(M1V_E_ARG, "unknown plane layout preset%s");
    const size_t W = (size_t)width, H = (size_t)height, luma = W * H;
    m1v_plane_layout l = {};
    l.y_pitch = W;
    if (preset == M1V_PLANES_REFERENCE) { // what m1v_convert_device writes: three full-resolution planes, chroma addressed with W / 2
        l.cb_offset = luma;
        l.cr_offset = 2 * luma;
        l.c_pitch = W / 2;
        l.c_step = 1;
        l.frame_stride = 3 * luma;
    } else {
        if ((width | height) & 1) return fail(M1V_E_ARG, "a 4:2:0 preset needs an even width and height%s");
        const size_t quarter = (W / 2) * (H / 2);
        const bool planar = preset == M1V_PLANES_I420 || preset == M1V_PLANES_YV12;
        const bool cr_first = preset == M1V_PLANES_YV12 || preset == M1V_PLANES_NV21;
        const size_t second = planar ? quarter : 1;
        l.cb_offset = luma + (cr_first ? second : 0);
        l.cr_offset = luma + (cr_first ? 0 : second);
        l.c_step = planar ? 1 : 2;
        l.c_pitch = planar ? W / 2 : W;
        l.frame_stride = luma * 3 / 2;
    }
    *out = l;
    return M1V_OK;
}

int m1v_sample_layout_preset(int width, int height, int preset, m1v_sample_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (preset < M1V_SAMPLES_YUY2 || preset > M1V_SAMPLES_P010) return fail(M1V_E_ARG, "unknown sample layout preset%s");
    if ((width | height) & 1) return fail(M1V_E_ARG, "a sample layout preset needs an even width and height%s");
    const size_t W = (size_t)width, H = (size_t)height;
    m1v_sample_layout l = {};
    l.y_step = 2;
    l.c_step = 4;
    l.y_pitch = 2 * W;
    if (preset == M1V_SAMPLES_P010) { // a plane of 16-bit luma words, then one of Cb, Cr word pairs: the high byte of each word
        l.y_offset = 1;
        l.cb_offset = 2 * W * H + 1;
        l.cr_offset = 2 * W * H + 3;
        l.c_pitch = 2 * W;
        l.frame_stride = 3 * W * H;
    } else { // groups of four bytes = two pixels; chroma from the even picture rows
        l.y_offset = preset == M1V_SAMPLES_UYVY ? 1 : 0;
        l.cb_offset = preset == M1V_SAMPLES_YUY2 ? 1 : (preset == M1V_SAMPLES_UYVY ? 0 : 3);
        l.cr_offset = preset == M1V_SAMPLES_YUY2 ? 3 : (preset == M1V_SAMPLES_UYVY ? 2 : 1);
        l.c_pitch = 4 * W;
        l.frame_stride = 2 * W * H;
    }
    *out = l;
    return M1V_OK;
}

// (m1v_set_plane_layout ends here too, with y_step 1: the checks of include/mpeg1_hip.h on the two steps, then on offsets,
// pitches and the frame's extent with the steps put in, then the reconfiguration)
int m1v_set_sample_layout(m1v_encoder *e, const m1v_sample_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "a plane layout needs an encoder created with 3 channels%s");
        const unsigned long long y_step = layout->y_step ? layout->y_step : 1, step = layout->c_step ? layout->c_step : 1;
        if (!((y_step == 1 && step <= 2) || (y_step == 2 && step == 4)))
            return fail(M1V_E_ARG, "(y_step, c_step) must be (1, 1), (1, 2) or (2, 4) (0 = 1)%s");
        if (step == 4 && std::max(layout->cb_offset, layout->cr_offset) - std::min(layout->cb_offset, layout->cr_offset) > 3)
            return fail(M1V_E_ARG, "with c_step 4 the chroma offsets must lie within one 4-byte group%s");
        if (layout->frame_stride == 0) return fail(M1V_E_ARG, "a plane layout needs a frame stride%s");
        const unsigned long long W = (unsigned long long)g.W, half = W / 2;
        if (layout->y_pitch != 0 && layout->y_pitch < W * y_step) return fail(M1V_E_ARG, "luma pitch below width * y_step%s");
        if (layout->c_pitch != 0 && layout->c_pitch < half * step) return fail(M1V_E_ARG, "chroma pitch below (width / 2) * c_step%s");
        const unsigned long long y_pitch = layout->y_pitch ? layout->y_pitch : W * y_step, c_pitch = layout->c_pitch ? layout->c_pitch : half * step;
        // the frame's extent: the read contract of mpeg1_hip.h (rows and row bytes of the region the encoder codes)
        const unsigned long long xe = (unsigned long long)g.n_strips * 16, ye = (unsigned long long)g.n_mbrows * 16;
        const unsigned long long limit = 1ull << 32;
        if (y_pitch >= limit || c_pitch >= limit || layout->y_offset >= limit || layout->cb_offset >= limit || layout->cr_offset >= limit)
            return fail(M1V_E_ARG, "a frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        const unsigned long long y_rows = (ye - 1) * y_pitch + (xe - 1) * y_step + 1;             // one past the last addressed luma byte
        const unsigned long long c_rows = (ye / 2 - 1) * c_pitch + (xe / 2 - 1) * step + 1; // one past a plane's last addressed byte
        const unsigned long long extent = std::max(layout->y_offset + y_rows,
                                                   std::max<unsigned long long>(layout->cb_offset, layout->cr_offset) + c_rows);
        if (extent >= limit) return fail(M1V_E_ARG, "a frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        if (layout->frame_stride < extent) return fail(M1V_E_ARG, "frame stride below the bytes a frame's planes span%s");
        want.kind = LayoutKind::samples;
        want.samples = {(uint32_t)layout->y_offset, (uint32_t)layout->cb_offset, (uint32_t)layout->cr_offset, (uint32_t)y_pitch,
                        (uint32_t)c_pitch, (uint32_t)y_step, (uint32_t)step, extent};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_set_plane_layout(m1v_encoder *e, const m1v_plane_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (!layout) return m1v_set_sample_layout(e, nullptr);
    if (layout->c_step > 2) return fail(M1V_E_ARG, "c_step must be 1 or 2 (0 = 1)%s");
    const m1v_sample_layout l = {layout->y_offset, layout->cb_offset, layout->cr_offset, layout->y_pitch, layout->c_pitch, 1, layout->c_step, layout->frame_stride};
    return m1v_set_sample_layout(e, &l);
}

int m1v_plane_layout_in_force(const m1v_encoder *e, m1v_plane_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = samples_in_force(e); rc != 1) return rc;
    const m1v_encoder::Layout::Samples &s = e->layout.samples;
    if (s.y_step == 2) return ask_its_getter(e);
    if (out) *out = {s.y_off, s.cb_off, s.cr_off, s.y_pitch, s.c_pitch, s.c_step, (size_t)e->layout.frame_stride};
    return 1;
}

int m1v_sample_layout_in_force(const m1v_encoder *e, m1v_sample_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = samples_in_force(e); rc != 1) return rc;
    const m1v_encoder::Layout::Samples &s = e->layout.samples;
    if (out) *out = {s.y_off, s.cb_off, s.cr_off, s.y_pitch, s.c_pitch, s.y_step, s.c_step, (size_t)e->layout.frame_stride};
    return 1;
}

int m1v_rgb_plane_layout_preset(int width, int height, int order, m1v_rgb_plane_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (order < M1V_RGB_PLANES_RGB || order > M1V_RGB_PLANES_GBR) return fail(M1V_E_ARG, "unknown RGB plane order%s");
    const uint64_t plane = (uint64_t)width * (uint64_t)height;
    // which of the three planes, in memory order, holds R, G and B
    static const int at[3][3] = {{0, 1, 2}, {2, 1, 0}, {2, 0, 1}};
    *out = {at[order][0] * plane, at[order][1] * plane, at[order][2] * plane, (uint64_t)width, 3 * plane};
    return M1V_OK;
}

// What three planes of `row` bytes per picture row (width bytes, or width * S of a float layout) must satisfy, behind the check of
// the pitch: the frame below 4 GiB, no shared bytes, a frame stride that covers them
static int three_planes_fit(const unsigned long long off[3], unsigned long long pitch, unsigned long long row, unsigned long long H,
                            unsigned long long frame_stride) {
    const unsigned long long limit = 1ull << 32;
    const unsigned long long lo = std::min(off[0], std::min(off[1], off[2])), hi = std::max(off[0], std::max(off[1], off[2]));
    if (pitch >= limit || hi >= limit || hi + (H - 1) * pitch + row >= limit)
        return fail(M1V_E_ARG, "a frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
    // Two planes may share a byte range only as a row interleave.  Row y1 of the plane at the lower offset and row y2 of the
    // other share a byte when |d + (y2 - y1) * pitch| < row, d = the distance of the offsets = q * pitch + r: y2 - y1 = -q
    // leaves r, y2 - y1 = -q - 1 leaves r - pitch, every other difference is further away.
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++) {
            const unsigned long long d = off[a] < off[b] ? off[b] - off[a] : off[a] - off[b], q = d / pitch, r = d % pitch;
            if ((r < row && q <= H - 1) || (pitch - r < row && q + 1 <= H - 1))
                return fail(M1V_E_ARG, "two planes share bytes (planes may interleave by rows only)%s");
        }
    if (frame_stride < hi + (H - 1) * pitch + row - lo) return fail(M1V_E_ARG, "frame stride below the bytes a frame's planes span%s");
    return M1V_OK;
}

int m1v_set_rgb_plane_layout(m1v_encoder *e, const m1v_rgb_plane_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "an RGB plane layout needs an encoder created with 3 channels%s");
        if (g.W & 1) return fail(M1V_E_ARG, "an RGB plane layout needs an even width (the chroma plane is addressed with stride width / 2)%s");
        const unsigned long long W = (unsigned long long)g.W, pitch = layout->row_pitch;
        if (pitch < W) return fail(M1V_E_ARG, "row pitch below the width%s");
        const unsigned long long off[3] = {layout->r_offset, layout->g_offset, layout->b_offset};
        if (const int rc = three_planes_fit(off, pitch, W, (unsigned long long)g.H, layout->frame_stride)) return rc;
        want.kind = LayoutKind::rgb_planes;
        want.rgb_planes = {(uint32_t)off[0], (uint32_t)off[1], (uint32_t)off[2], (uint32_t)pitch};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_rgb_plane_layout_in_force(const m1v_encoder *e, m1v_rgb_plane_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::rgb_planes) return 0;
    const RgbPlaneFrontArgs &p = e->layout.rgb_planes;
    if (out) *out = {p.r_off, p.g_off, p.b_off, p.row_pitch, e->layout.frame_stride};
    return 1;
}

int m1v_float_plane_layout_preset(int width, int height, int order, int sample, int range, m1v_float_plane_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    FloatFormat fmt;
    if (const int rc = float_format(sample, range, fmt)) return rc;
    const uint64_t S = fmt.bytes;
    m1v_rgb_plane_layout bytes;
    if (const int rc = m1v_rgb_plane_layout_preset(width, height, order, &bytes)) return rc;
    *out = {bytes.r_offset * S, bytes.g_offset * S, bytes.b_offset * S, bytes.row_pitch * S, bytes.frame_stride * S, sample, range};
    return M1V_OK;
}

int m1v_set_float_plane_layout(m1v_encoder *e, const m1v_float_plane_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "a float plane layout needs an encoder created with 3 channels%s");
        if (g.W & 1) return fail(M1V_E_ARG, "a float plane layout needs an even width (the chroma plane is addressed with stride width / 2)%s");
        if (const int rc = float_format(layout->sample, layout->range, want.fmt)) return rc;
        const unsigned long long row = (unsigned long long)g.W * want.fmt.bytes, pitch = layout->row_pitch;
        const unsigned long long off[3] = {layout->r_offset, layout->g_offset, layout->b_offset};
        if (const int rc = whole_samples(want.fmt, off[0] | off[1] | off[2] | pitch | layout->frame_stride, "offsets, row pitch and frame stride")) return rc;
        if (pitch < row) return fail(M1V_E_ARG, "row pitch below width * sample size%s");
        if (const int rc = three_planes_fit(off, pitch, row, (unsigned long long)g.H, layout->frame_stride)) return rc;
        want.kind = LayoutKind::float_planes;
        want.float_planes = {(uint32_t)off[0], (uint32_t)off[1], (uint32_t)off[2], (uint32_t)pitch, want.fmt.scale};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_float_plane_layout_in_force(const m1v_encoder *e, m1v_float_plane_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::float_planes) return 0;
    const FloatPlaneFrontArgs &f = e->layout.float_planes;
    if (out) *out = {f.r_off, f.g_off, f.b_off, f.row_pitch, e->layout.frame_stride, e->layout.fmt.sample, e->layout.fmt.range};
    return 1;
}

int m1v_float_planes_to_bytes_device(m1v_encoder *e, const void *d_frames, int n_frames, uint8_t *d_bytes, void *stream) {
    static const void *const kernels[3] = {(const void *)&k_float_planes_to_bytes<F16Sample>, (const void *)&k_float_planes_to_bytes<Bf16Sample>,
                                           (const void *)&k_float_planes_to_bytes<F32Sample>};
    return float_to_bytes(
        e, LayoutKind::float_planes, "m1v_float_planes_to_bytes_device needs a float plane layout in force (m1v_set_float_plane_layout)", kernels,
        d_frames, n_frames, d_bytes, stream,
        [e](const uint8_t *frames, uint8_t *bytes) {
            return FloatBytesArgs{frames, bytes, e->layout.float_planes, e->layout.frame_stride, (uint32_t)e->g.W, (uint32_t)e->g.H};
        },
        [e](unsigned n) { return dim3(((unsigned)e->g.W / 2u * (unsigned)e->g.H + 255u) / 256u, n, 3u); }); // (pairs of samples, per plane)
}

int m1v_float_pixel_layout_preset(int width, int height, int pixel_samples, int order, int sample, int range, m1v_float_pixel_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (pixel_samples != 3 && pixel_samples != 4) return fail(M1V_E_ARG, "a pixel has 3 or 4 samples%s");
    if (order != M1V_ORDER_RGB && order != M1V_ORDER_BGR) return fail(M1V_E_ARG, "unknown order (M1V_ORDER_RGB, M1V_ORDER_BGR)%s");
    FloatFormat fmt;
    if (const int rc = float_format(sample, range, fmt)) return rc;
    const uint64_t step = (uint64_t)pixel_samples * fmt.bytes, pitch = (uint64_t)width * step;
    *out = {pitch, (uint64_t)height * pitch, step, order, sample, range};
    return M1V_OK;
}

int m1v_set_float_pixel_layout(m1v_encoder *e, const m1v_float_pixel_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "a float pixel layout needs an encoder created with 3 channels (the pixel's sample count is the layout's)%s");
        if (g.W & 1) return fail(M1V_E_ARG, "a float pixel layout needs an even width (the chroma plane is addressed with stride width / 2)%s");
        if (layout->order != M1V_ORDER_RGB && layout->order != M1V_ORDER_BGR) return fail(M1V_E_ARG, "unknown order (M1V_ORDER_RGB, M1V_ORDER_BGR)%s");
        if (const int rc = float_format(layout->sample, layout->range, want.fmt)) return rc;
        const unsigned long long S = want.fmt.bytes, step = layout->pixel_step, pitch = layout->row_pitch;
        if (step == S)
            return fail(M1V_E_ARG, "a pixel step of one sample describes a plane, not pixels: m1v_set_float_plane_layout serves planar float frames%s");
        if (step != 3 * S && step != 4 * S) return fail(M1V_E_ARG, "pixel step must be 3 or 4 samples (%s bytes)", S == 2 ? "6 or 8" : "12 or 16");
        if (const int rc = whole_samples(want.fmt, pitch | layout->frame_stride, "row pitch and frame stride")) return rc;
        if (const int rc = rows_fit(pitch, (unsigned long long)g.W * step, (unsigned long long)g.H, layout->frame_stride,
                                    "row pitch below width * pixel step", "frame", "frame stride below the bytes a frame's rows span"))
            return rc;
        want.kind = LayoutKind::float_pixels;
        want.float_pixels = {{(uint32_t)pitch, want.fmt.scale, layout->order == M1V_ORDER_BGR ? 1u : 0u}, (uint32_t)step};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_float_pixel_layout_in_force(const m1v_encoder *e, m1v_float_pixel_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::float_pixels) return 0;
    const m1v_encoder::Layout::FloatPixels &f = e->layout.float_pixels;
    if (out) *out = {f.front.row_pitch, e->layout.frame_stride, f.pixel_step, (int32_t)(f.front.bgr ? M1V_ORDER_BGR : M1V_ORDER_RGB), e->layout.fmt.sample, e->layout.fmt.range};
    return 1;
}

int m1v_float_pixels_to_bytes_device(m1v_encoder *e, const void *d_frames, int n_frames, uint8_t *d_bytes, void *stream) {
    static const void *const kernels[3] = {(const void *)&k_float_pixels_to_bytes<F16Sample>, (const void *)&k_float_pixels_to_bytes<Bf16Sample>,
                                           (const void *)&k_float_pixels_to_bytes<F32Sample>};
    return float_to_bytes(
        e, LayoutKind::float_pixels, "m1v_float_pixels_to_bytes_device needs a float pixel layout in force (m1v_set_float_pixel_layout)", kernels,
        d_frames, n_frames, d_bytes, stream,
        [e](const uint8_t *frames, uint8_t *bytes) {
            const m1v_encoder::Layout::FloatPixels &f = e->layout.float_pixels;
            return FloatPixelBytesArgs{frames, bytes, f.front, e->layout.frame_stride, (uint32_t)e->g.W, (uint32_t)e->g.H, f.pixel_step};
        },
        [e](unsigned n) { return dim3(((unsigned)e->g.W * (unsigned)e->g.H + 255u) / 256u, n); }); // (pixels)
}

int m1v_downscale_layout_preset(int width, int height, int pixel_bytes, int order, int factor, m1v_downscale_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (pixel_bytes != 3 && pixel_bytes != 4) return fail(M1V_E_ARG, "a source pixel has 3 or 4 bytes%s");
    if (order != M1V_ORDER_RGB && order != M1V_ORDER_BGR) return fail(M1V_E_ARG, "unknown order (M1V_ORDER_RGB, M1V_ORDER_BGR)%s");
    if (factor != 2) return fail(M1V_E_ARG, "factor must be 2 (other factors are not covered)%s");
    const uint64_t pitch = 2 * (uint64_t)width * (uint64_t)pixel_bytes;
    *out = {pitch, 2 * (uint64_t)height * pitch, (uint64_t)pixel_bytes, order, factor};
    return M1V_OK;
}

int m1v_set_downscale_layout(m1v_encoder *e, const m1v_downscale_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "a downscale layout needs an encoder created with 3 channels (the source pixel's byte count is the layout's)%s");
        if (g.W & 1) return fail(M1V_E_ARG, "a downscale layout needs an even width (the chroma plane is addressed with stride width / 2)%s");
        if (layout->order != M1V_ORDER_RGB && layout->order != M1V_ORDER_BGR) return fail(M1V_E_ARG, "unknown order (M1V_ORDER_RGB, M1V_ORDER_BGR)%s");
        if (layout->factor != 2) return fail(M1V_E_ARG, "factor must be 2 (other factors are not covered)%s");
        const unsigned long long step = layout->pixel_step;
        if (step != 3 && step != 4) return fail(M1V_E_ARG, "pixel step must be 3 or 4 bytes%s");
        // (the source's rows: twice the encoder's width and height)
        if (const int rc = rows_fit(layout->row_pitch, 2ull * (unsigned long long)g.W * step, 2ull * (unsigned long long)g.H, layout->frame_stride,
                                    "row pitch below 2 * width * pixel step", "source frame",
                                    "frame stride below the bytes a source frame's rows span"))
            return rc;
        want.kind = LayoutKind::downscale;
        want.downscale = {{(uint32_t)layout->row_pitch, layout->order == M1V_ORDER_BGR ? 1u : 0u}, (uint32_t)step};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_downscale_layout_in_force(const m1v_encoder *e, m1v_downscale_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::downscale) return 0;
    const m1v_encoder::Layout::Downscale &d = e->layout.downscale;
    if (out) *out = {d.front.row_pitch, e->layout.frame_stride, d.pixel_step, (int32_t)(d.front.bgr ? M1V_ORDER_BGR : M1V_ORDER_RGB), 2};
    return 1;
}

int m1v_downscale_to_bytes_device(m1v_encoder *e, const void *d_frames, int n_frames, uint8_t *d_bytes, void *stream) {
    // (one kernel whatever the sample type: a byte layout leaves the float format's zeros)
    static const void *const kernels[3] = {(const void *)&k_downscale_to_bytes, (const void *)&k_downscale_to_bytes, (const void *)&k_downscale_to_bytes};
    return float_to_bytes(
        e, LayoutKind::downscale, "m1v_downscale_to_bytes_device needs a downscale layout in force (m1v_set_downscale_layout)", kernels,
        d_frames, n_frames, d_bytes, stream,
        [e](const uint8_t *frames, uint8_t *bytes) {
            const m1v_encoder::Layout::Downscale &d = e->layout.downscale;
            return DownscaleBytesArgs{frames, bytes, d.front, e->layout.frame_stride, (uint32_t)e->g.W, (uint32_t)e->g.H, d.pixel_step};
        },
        [e](unsigned n) { return dim3(((unsigned)e->g.W * (unsigned)e->g.H + 255u) / 256u, n); }); // (rendition pixels)
}

int m1v_downscale_plane_layout_preset(int width, int height, int preset, int factor, m1v_downscale_plane_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (preset == M1V_PLANES_REFERENCE) return fail(M1V_E_ARG, "the reference-style 4:4:4 planes are not a source of a downscale plane layout%s");
    if (preset < M1V_PLANES_I420 || preset > M1V_PLANES_NV21) return fail(M1V_E_ARG, "unknown plane layout preset%s");
    if ((width | height) & 1) return fail(M1V_E_ARG, "a downscale plane layout needs an even width and height%s");
    if (factor != 2) return fail(M1V_E_ARG, "factor must be 2 (other factors are not covered)%s");
    // the plane preset of the tightly packed 2 W x 2 H source
    const uint64_t W = (uint64_t)width, H = (uint64_t)height, luma = 4 * W * H, quarter = W * H;
    const bool planar = preset == M1V_PLANES_I420 || preset == M1V_PLANES_YV12;
    const bool cr_first = preset == M1V_PLANES_YV12 || preset == M1V_PLANES_NV21;
    const uint64_t second = planar ? quarter : 1;
    *out = {0, luma + (cr_first ? second : 0), luma + (cr_first ? 0 : second), 2 * W, planar ? W : 2 * W, planar ? 1u : 2u,
            luma * 3 / 2, factor, 0};
    return M1V_OK;
}

int m1v_set_downscale_plane_layout(m1v_encoder *e, const m1v_downscale_plane_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "a downscale plane layout needs an encoder created with 3 channels%s");
        if ((g.W | g.H) & 1) return fail(M1V_E_ARG, "a downscale plane layout needs an even width and height (the rendition's chroma planes are width / 2 x height / 2)%s");
        if (layout->factor != 2) return fail(M1V_E_ARG, "factor must be 2 (other factors are not covered)%s");
        if (layout->reserved != 0) return fail(M1V_E_ARG, "reserved must be 0%s");
        if (layout->c_step > 2) return fail(M1V_E_ARG, "c_step must be 1 or 2 (0 = 1)%s");
        if (layout->frame_stride == 0) return fail(M1V_E_ARG, "a downscale plane layout needs a frame stride%s");
        const unsigned long long W = (unsigned long long)g.W, step = layout->c_step ? layout->c_step : 1;
        if (layout->y_pitch != 0 && layout->y_pitch < 2 * W) return fail(M1V_E_ARG, "luma pitch below 2 * width%s");
        if (layout->c_pitch != 0 && layout->c_pitch < W * step) return fail(M1V_E_ARG, "chroma pitch below width * c_step%s");
        const unsigned long long y_pitch = layout->y_pitch ? layout->y_pitch : 2 * W, c_pitch = layout->c_pitch ? layout->c_pitch : W * step;
        // the source's extent: the read contract of mpeg1_hip.h (the plane layout's, taken on the source's rows)
        const unsigned long long xe = (unsigned long long)g.n_strips * 16, ye = (unsigned long long)g.n_mbrows * 16;
        const unsigned long long limit = 1ull << 32;
        if (y_pitch >= limit || c_pitch >= limit || layout->y_offset >= limit || layout->cb_offset >= limit || layout->cr_offset >= limit)
            return fail(M1V_E_ARG, "a source frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        const unsigned long long y_rows = (2 * ye - 1) * y_pitch + 2 * xe;          // one past the last addressed luma byte
        const unsigned long long c_rows = (ye - 1) * c_pitch + (xe - 1) * step + 1; // one past a chroma plane's last addressed byte
        const unsigned long long extent = std::max(layout->y_offset + y_rows,
                                                   std::max<unsigned long long>(layout->cb_offset, layout->cr_offset) + c_rows);
        if (extent >= limit) return fail(M1V_E_ARG, "a source frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        if (layout->frame_stride < extent) return fail(M1V_E_ARG, "frame stride below the bytes a source frame's planes span%s");
        want.kind = LayoutKind::downscale_planes;
        // (lim: the 32-byte unit that ends with the extent is the last one a kernel may load; extent >= 1024,
        // m1v_downscale_planes.h)
        want.downscale_planes = {{(uint32_t)layout->y_offset, (uint32_t)layout->cb_offset, (uint32_t)layout->cr_offset, (uint32_t)y_pitch,
                                  (uint32_t)c_pitch, (uint32_t)(extent - 32ull)}, (uint32_t)step};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_downscale_plane_layout_in_force(const m1v_encoder *e, m1v_downscale_plane_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::downscale_planes) return 0;
    const m1v_encoder::Layout::DownscalePlanes &d = e->layout.downscale_planes;
    if (out) *out = {d.front.y_off, d.front.cb_off, d.front.cr_off, d.front.y_pitch, d.front.c_pitch, d.c_step, e->layout.frame_stride, 2, 0};
    return 1;
}

int m1v_downscale_planes_to_i420_device(m1v_encoder *e, const void *d_src, int n_frames, void *d_dst, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::downscale_planes)
        return fail(M1V_E_ARG, "m1v_downscale_planes_to_i420_device needs a downscale plane layout in force (m1v_set_downscale_plane_layout)%s");
    if (n_frames < 0 || ((!d_src || !d_dst) && n_frames > 0)) return fail(M1V_E_ARG, "null pointer or negative n_frames%s");
    const m1v_encoder::Layout::DownscalePlanes &d = e->layout.downscale_planes;
    {   // the kernel reads the whole 2 W x 2 H source, which the setter held only to the coded region's extent
        const unsigned long long W = (unsigned long long)e->g.W, H = (unsigned long long)e->g.H;
        const unsigned long long whole = std::max((unsigned long long)d.front.y_off + (2 * H - 1) * d.front.y_pitch + 2 * W,
                                                  (unsigned long long)std::max(d.front.cb_off, d.front.cr_off) + (H - 1) * d.front.c_pitch + (W - 1) * d.c_step + 1);
        if (whole >= (1ull << 32))
            return fail(M1V_E_ARG, "m1v_downscale_planes_to_i420_device reads the whole source: a source frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        if (e->layout.frame_stride < whole)
            return fail(M1V_E_ARG, "m1v_downscale_planes_to_i420_device reads the whole source: frame stride below the bytes the whole source frame's planes span%s");
    }
    HIP_TRY(hipSetDevice(e->device));
    const unsigned long long frame_out = (unsigned long long)e->g.W * (unsigned long long)e->g.H * 3 / 2;
    for (int done = 0; done < n_frames; done += 65535) { // (a grid's y extent)
        HalfPlaneBytesArgs a = {static_cast<const uint8_t *>(d_src) + (unsigned long long)done * e->layout.frame_stride,
                                static_cast<uint8_t *>(d_dst) + (unsigned long long)done * frame_out, d.front, e->layout.frame_stride,
                                (uint32_t)e->g.W, (uint32_t)e->g.H, d.c_step};
        void *argv[] = {&a};
        HIP_TRY(hipLaunchKernel((const void *)&k_half_planes_to_i420, dim3(((unsigned)frame_out + 255u) / 256u, (unsigned)std::min(n_frames - done, 65535)),
                                dim3(256u), argv, 0, (hipStream_t)stream));
    }
    return M1V_OK;
}

int m1v_downscale_word_layout_preset(int width, int height, int preset, int factor, m1v_downscale_word_layout *out) {
    if (!out) return fail(M1V_E_ARG, "null out%s");
    if (width <= 0 || height <= 0) return fail(M1V_E_ARG, "bad geometry%s");
    if (preset < M1V_WORDS_P010 || preset > M1V_WORDS_I016) return fail(M1V_E_ARG, "unknown word layout preset%s");
    if ((width | height) & 1) return fail(M1V_E_ARG, "a downscale word layout needs an even width and height%s");
    if (factor != 2) return fail(M1V_E_ARG, "factor must be 2 (other factors are not covered)%s");
    // the tightly packed 2 W x 2 H source: 4 W H luma words, then W H words per chroma component
    const uint64_t W = (uint64_t)width, H = (uint64_t)height, luma = 8 * W * H, plane = 2 * W * H;
    const bool paired = preset == M1V_WORDS_P010;
    const int32_t shift = preset == M1V_WORDS_I010 ? 2 : preset == M1V_WORDS_I012 ? 4 : 8;
    *out = {0, luma, luma + (paired ? 2 : plane), 4 * W, paired ? 4 * W : 2 * W, paired ? 4u : 2u, luma + 2 * plane, factor, shift};
    return M1V_OK;
}

// One past the last addressed byte of a word source whose planes hold xe x ye rendition samples (the read contract of mpeg1_hip.h)
static unsigned long long word_source_extent(const HalfWordFrontArgs &f, unsigned long long step, unsigned long long xe, unsigned long long ye) {
    const unsigned long long y_rows = (2 * ye - 1) * f.y_pitch + 4 * xe;
    const unsigned long long c_rows = (ye - 1) * f.c_pitch + (xe - 1) * step + 2;
    return std::max(f.y_off + y_rows, (unsigned long long)std::max(f.cb_off, f.cr_off) + c_rows);
}

int m1v_set_downscale_word_layout(m1v_encoder *e, const m1v_downscale_word_layout *layout) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    m1v_encoder::Layout want;
    if (layout) {
        const Geometry &g = e->g;
        if (g.C != 3) return fail(M1V_E_ARG, "a downscale word layout needs an encoder created with 3 channels%s");
        if ((g.W | g.H) & 1) return fail(M1V_E_ARG, "a downscale word layout needs an even width and height (the rendition's chroma planes are width / 2 x height / 2)%s");
        if (layout->factor != 2) return fail(M1V_E_ARG, "factor must be 2 (other factors are not covered)%s");
        if (layout->shift < 0 || layout->shift > 8) return fail(M1V_E_ARG, "shift must be 0 .. 8%s");
        if (layout->c_step != 0 && layout->c_step != 2 && layout->c_step != 4) return fail(M1V_E_ARG, "c_step must be 2 or 4 (0 = 2)%s");
        const unsigned long long W = (unsigned long long)g.W, step = layout->c_step ? layout->c_step : 2;
        if (step == 4 && std::max(layout->cb_offset, layout->cr_offset) - std::min(layout->cb_offset, layout->cr_offset) > 3)
            return fail(M1V_E_ARG, "with c_step 4 the chroma offsets must lie within one 4-byte group%s");
        if (layout->frame_stride == 0) return fail(M1V_E_ARG, "a downscale word layout needs a frame stride%s");
        if (layout->y_pitch != 0 && layout->y_pitch < 4 * W) return fail(M1V_E_ARG, "luma pitch below 4 * width%s");
        if (layout->c_pitch != 0 && layout->c_pitch < W * step) return fail(M1V_E_ARG, "chroma pitch below width * c_step%s");
        const unsigned long long y_pitch = layout->y_pitch ? layout->y_pitch : 4 * W, c_pitch = layout->c_pitch ? layout->c_pitch : W * step;
        // the source's extent: the read contract of mpeg1_hip.h (the plane layout's, taken on the source's rows and words)
        const unsigned long long limit = 1ull << 32;
        if (y_pitch >= limit || c_pitch >= limit || layout->y_offset >= limit || layout->cb_offset >= limit || layout->cr_offset >= limit)
            return fail(M1V_E_ARG, "a source frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        HalfWordFrontArgs front = {(uint32_t)layout->y_offset, (uint32_t)layout->cb_offset, (uint32_t)layout->cr_offset, (uint32_t)y_pitch,
                                   (uint32_t)c_pitch, 0u, (uint32_t)layout->shift};
        const unsigned long long extent = word_source_extent(front, step, (unsigned long long)g.n_strips * 16, (unsigned long long)g.n_mbrows * 16);
        if (extent >= limit) return fail(M1V_E_ARG, "a source frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        if (layout->frame_stride < extent) return fail(M1V_E_ARG, "frame stride below the bytes a source frame's planes span%s");
        // (lim: the 64-byte unit that ends with the extent is the last one a kernel may load; extent >= 2048, m1v_downscale_words.h)
        front.lim = (uint32_t)(extent - 64ull);
        want.kind = LayoutKind::downscale_words;
        want.downscale_words = {front, (uint32_t)step};
        want.frame_stride = layout->frame_stride;
    }
    return apply_layout(e, want);
}

int m1v_downscale_word_layout_in_force(const m1v_encoder *e, m1v_downscale_word_layout *out) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::downscale_words) return 0;
    const m1v_encoder::Layout::DownscaleWords &d = e->layout.downscale_words;
    if (out) *out = {d.front.y_off, d.front.cb_off, d.front.cr_off, d.front.y_pitch, d.front.c_pitch, d.c_step, e->layout.frame_stride, 2, (int32_t)d.front.shift};
    return 1;
}

int m1v_downscale_words_to_i420_device(m1v_encoder *e, const void *d_src, int n_frames, void *d_dst, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (e->layout.kind != LayoutKind::downscale_words)
        return fail(M1V_E_ARG, "m1v_downscale_words_to_i420_device needs a downscale word layout in force (m1v_set_downscale_word_layout)%s");
    if (n_frames < 0 || ((!d_src || !d_dst) && n_frames > 0)) return fail(M1V_E_ARG, "null pointer or negative n_frames%s");
    const m1v_encoder::Layout::DownscaleWords &d = e->layout.downscale_words;
    {   // the kernel reads the whole 2 W x 2 H source, which the setter held only to the coded region's extent
        const unsigned long long whole = word_source_extent(d.front, d.c_step, (unsigned long long)e->g.W, (unsigned long long)e->g.H);
        if (whole >= (1ull << 32))
            return fail(M1V_E_ARG, "m1v_downscale_words_to_i420_device reads the whole source: a source frame of 4 GiB or more (byte offsets inside a frame are 32-bit)%s");
        if (e->layout.frame_stride < whole)
            return fail(M1V_E_ARG, "m1v_downscale_words_to_i420_device reads the whole source: frame stride below the bytes the whole source frame's planes span%s");
    }
    HIP_TRY(hipSetDevice(e->device));
    const unsigned long long frame_out = (unsigned long long)e->g.W * (unsigned long long)e->g.H * 3 / 2;
    for (int done = 0; done < n_frames; done += 65535) { // (a grid's y extent)
        HalfWordBytesArgs a = {static_cast<const uint8_t *>(d_src) + (unsigned long long)done * e->layout.frame_stride,
                               static_cast<uint8_t *>(d_dst) + (unsigned long long)done * frame_out, d.front, e->layout.frame_stride,
                               (uint32_t)e->g.W, (uint32_t)e->g.H, d.c_step};
        void *argv[] = {&a};
        HIP_TRY(hipLaunchKernel((const void *)&k_half_words_to_i420, dim3(((unsigned)frame_out + 255u) / 256u, (unsigned)std::min(n_frames - done, 65535)),
                                dim3(256u), argv, 0, (hipStream_t)stream));
    }
    return M1V_OK;
}

// The table mode is a field of the layout record in force: no plan, no allocation, nothing queued
int m1v_set_frame_table(m1v_encoder *e, int enable) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    const char *refusal = kind_facts(e->layout).no_frame_table;
    if (enable && refusal) return fail(M1V_E_ARG, "%s", refusal);
    e->layout.table = enable ? TableMode::frames : TableMode::off;
    return M1V_OK;
}

int m1v_frame_table(const m1v_encoder *e) { return e ? (e->layout.table == TableMode::frames ? 1 : 0) : -1; }

// The plane table is another value of the same field: each setter selects its own mode, either turns tables off
int m1v_set_plane_table(m1v_encoder *e, int enable) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    const char *refusal = kind_facts(e->layout).no_plane_table;
    if (enable && refusal) return fail(M1V_E_ARG, "%s", refusal);
    e->layout.table = enable ? TableMode::planes : TableMode::off;
    return M1V_OK;
}

int m1v_plane_table(const m1v_encoder *e) { return e ? (e->layout.table == TableMode::planes ? 1 : 0) : -1; }

int m1v_path_in_use(const m1v_encoder *e) { return e ? (e->plan.producer == Producer::tiles ? 1 : 0) : -1; }

int m1v_size_table_fused(const m1v_encoder *e) { return e ? (e->plan.table_units ? 1 : 0) : -1; }

void m1v_debug_fail_alloc(int nth) {
    // fault injection for the tests: inert unless the process was started with EC504_DEBUG_HOOKS=1
    const char *on = getenv("EC504_DEBUG_HOOKS");
    g_fail_alloc_in = (on && on[0] == '1' && nth > 0) ? nth : 0;
}

void m1v_debug_fail_encode(int stage) {
    // fault injection for the tests: inert unless the process was started with EC504_DEBUG_HOOKS=1
    const char *on = getenv("EC504_DEBUG_HOOKS");
    g_fail_encode_at = (on && on[0] == '1' && stage >= 1 && stage <= 3) ? stage : 0;
}

#if defined(M1V_STAMPS) || defined(M1V_TILE_STAMPS) || defined(M1V_ASM_STAMPS)
// diagnostic builds only: read and clear the per-phase cycle sums
int m1v_debug_read_stamps(m1v_encoder *e, unsigned long long out[32]) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, e->d_stamps, 32 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(e->d_stamps, 0, 32 * 8));
    return M1V_OK;
}
// diagnostic builds only: the per-workgroup timeline of the last k_assemble launch (8 stamps each)
int m1v_debug_read_timeline(m1v_encoder *e, unsigned long long *out, int workgroups) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, e->d_stamps + 32, (size_t)(workgroups > 65536 ? 65536 : workgroups) * 64, hipMemcpyDeviceToHost));
    return M1V_OK;
}
#endif

int m1v_profile_enable(m1v_encoder *e, int enable) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    e->prof = enable != 0;
    e->ev_used = 0;
    return M1V_OK;
}

int m1v_profile_read(m1v_encoder *e, int *launches, double *total_ms) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    return profile_times(e, nullptr, 0, launches, total_ms);
}

int m1v_profile_read_times(m1v_encoder *e, float *ms, int cap, int *launches) {
    if (!e || (cap > 0 && !ms)) return fail(M1V_E_ARG, "bad argument%s");
    return profile_times(e, ms, cap, launches, nullptr);
}

// ---- what writes a batch's per-frame selection (the steps a Selection of encode_batch names) ------------------------------------
static int select_by_quality(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, int n_frames, hipStream_t st) {
    uint32_t *const batch_status = cur.words;
    QualityArgs &qa = *static_cast<QualityArgs *>(args);
    qa.max_q = encoder_quality(e);
    qa.n_frames = n_frames;
    qa.qsel = e->d_qsel;
    qa.status = batch_status;
    hipLaunchKernelGGL(k_frame_quality, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, st, qa);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

static int select_by_rd(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, int n_frames, hipStream_t st) {
    uint32_t *const batch_status = cur.words;
    RdPickArgs &ra = *static_cast<RdPickArgs *>(args);
    ra.n_frames = n_frames;
    ra.qsel = e->d_qsel;
    ra.status = batch_status;
    hipLaunchKernelGGL(k_rd_pick, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, st, ra);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

// batch_status: an encode's status word (the pick ORs M1V_STATUS_OVER_DISTORTION into it), or null
static int launch_rd_batch_pick(RdBatchArgs &ba, uint32_t *batch_status, hipStream_t st) {
    ba.batch_status = batch_status;
    hipLaunchKernelGGL(k_rd_batch_pick, dim3((unsigned)((ba.n_frames * kMaxCandidates + kRdPickThreads - 1) / kRdPickThreads)),
                       dim3(kRdPickThreads), 0, st, ba);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

// The batch pick (here, where the batch's status word is known), then k_frame_quality on the qualities and status word it wrote
static int select_by_rd_batch(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, int n_frames, hipStream_t st) {
    RdBatchArgs &ba = *static_cast<RdBatchArgs *>(args);
    if (const int rc = launch_rd_batch_pick(ba, cur.words, st)) return rc;
    QualityArgs qa = {};
    qa.quality = ba.chosen;
    qa.pick_status = ba.status;
    return select_by_quality(e, &qa, cur, n_frames, st);
}

// A batch at one quality per frame (null: the encoder's own), which a pick may have written with its status word (pick_status,
// or null): k_frame_quality checks the qualities and passes the pick's status bits on
static int encode_at(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index, const uint8_t *d_quality,
                     const uint32_t *pick_status, bool probe, const EncodeOut &o, void *stream) {
    if (!d_quality) return encode_batch(e, d_rgb, n_frames, first_frame_index, nullptr, probe, o, stream);
    QualityArgs qa = {};
    qa.quality = d_quality;
    qa.pick_status = pick_status;
    const Selection sel = {select_by_quality, &qa};
    return encode_batch(e, d_rgb, n_frames, first_frame_index, &sel, probe, o, stream);
}

int m1v_encode_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                      uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                      uint32_t *d_status, void *stream) {
    return encode_batch(e, d_rgb, n_frames, first_frame_index, nullptr, false, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_encode_quality_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                              const uint8_t *d_quality, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                              uint64_t *d_total, uint32_t *d_status, void *stream) {
    return encode_at(e, d_rgb, n_frames, first_frame_index, d_quality, nullptr, false, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_frame_sizes_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const uint8_t *d_quality,
                           uint64_t *d_frame_sizes, uint32_t *d_status, void *stream) {
    return encode_at(e, d_rgb, n_frames, 0, d_quality, nullptr, true, {nullptr, 0, d_frame_sizes, nullptr, d_status}, stream);
}

// ---- candidates: the checks, the table, the picks ------------------------------------------------------------------------------
// The checks the candidate-taking calls share, in the order every one of them has: the encoder and what the call checks before
// its candidates (`first`); the candidates, 1..8 strictly increasing qualities, each within 1 .. the encoder's quality factor;
// n_frames; what it checks after them (`then`).  on_table: a pick-only call, whose candidates are the rows of a table the
// caller holds: there are no qualities (q is not read), only their number.
static int check_candidate_call(const m1v_encoder *e, bool first, const uint8_t *q, int n_q, int n_frames, bool then, bool on_table = false) {
    if (!e || !first || (!q && !on_table)) return fail(M1V_E_ARG, "null pointer%s");
    if (n_q < 1 || n_q > kMaxCandidates) return fail(M1V_E_ARG, on_table ? "1 to 8 candidates%s" : "1 to 8 candidate qualities%s");
    for (int k = 0; k < n_q && !on_table; k++)
        if (q[k] < 1 || q[k] > encoder_quality(e) || (k > 0 && q[k] <= q[k - 1]))
            return fail(M1V_E_ARG, "candidates must increase strictly within 1 .. the encoder's quality factor%s");
    if (const int rc = check_batch_frames(e, n_frames)) return rc;
    return then ? M1V_OK : fail(M1V_E_ARG, "null pointer%s");
}

static int check_rd_rule(int rule) {
    return rule == M1V_RD_BEST_IN_BUDGET || rule == M1V_RD_SMALLEST_AT_DISTORTION ? M1V_OK : fail(M1V_E_ARG, "unknown rate-distortion rule%s");
}

static int check_cbr_rate(uint64_t bytes_per_frame, uint64_t buffer_bytes) {
    if (bytes_per_frame == 0 || buffer_bytes < bytes_per_frame || buffer_bytes >= (1ull << 62))
        return fail(M1V_E_ARG, "bitrate: need 1 <= bytes_per_frame <= buffer_bytes < 2^62%s");
    return M1V_OK;
}

static const char kNotFused[] = "the rd table needs the fused size table (m1v_size_table_fused): a debug hook has forced this encoder%s";

// sizes[k * stride + frame] and status[k] of every quality: one fused pass where the plan has one (3-channel tile encoders,
// 4-channel encoders: m1v_size_table_fused); otherwise (a path, input mode or run length forced by a test hook) one probe call
// (as m1v_frame_sizes_device) per quality, each with its own counter hand-over, then (pipelined) a flush, so that every row is
// complete in stream order.
static int size_table(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const uint8_t *qualities, int n_q,
                      unsigned long long *sizes, size_t stride, uint32_t *status, void *stream) {
    if (e->plan.table_units)
        return size_table_fused(e, d_rgb, n_frames, qualities, n_q, sizes, nullptr, stride, status, (hipStream_t)stream);
    for (int k = 0; k < n_q; k++) {
        QualityArgs qa = {};
        qa.uniform = qualities[k];
        const Selection sel = {select_by_quality, &qa};
        const int rc = encode_batch(e, d_rgb, n_frames, 0, &sel, true,
                                    {nullptr, 0, (uint64_t *)(sizes + (size_t)k * stride), nullptr, status ? status + k : nullptr}, stream);
        if (rc != M1V_OK) return rc;
    }
    // (pipelined: the probes' sizes are written on the internal stream)
    return e->pipelined ? m1v_flush(e, stream) : M1V_OK;
}

int m1v_frame_size_table_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const uint8_t *qualities, int n_qualities,
                                uint64_t *d_sizes, uint32_t *d_status, void *stream) {
    // (an empty batch reads no input)
    if (const int rc = check_candidate_call(e, d_sizes && (d_rgb || n_frames <= 0), qualities, n_qualities, n_frames, true)) return rc;
    if (n_frames == 0) return M1V_OK;
    return size_table(e, d_rgb, n_frames, qualities, n_qualities, (unsigned long long *)d_sizes, (size_t)n_frames, d_status, stream);
}

int m1v_frame_rd_table_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const uint8_t *qualities, int n_qualities,
                              uint64_t *d_sizes, uint64_t *d_distortion, uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, d_sizes && d_distortion && (d_rgb || n_frames <= 0), qualities, n_qualities, n_frames, true))
        return rc;
    if (!e->plan.table_units) return fail(M1V_E_ARG, kNotFused);
    if (n_frames == 0) return M1V_OK;
    return size_table_fused(e, d_rgb, n_frames, qualities, n_qualities, (unsigned long long *)d_sizes, (unsigned long long *)d_distortion,
                            (size_t)n_frames, d_status, (hipStream_t)stream);
}

// The table a pick reads: the encoder's own (own_table) or one the caller holds (rows n_frames apart, no qualities)
struct PickTable {
    const unsigned long long *sizes, *dist; // [k * stride + frame]; dist null: a size table
    int stride, n_cand;
    unsigned long long cand;                // byte k: the quality of candidate k
    const uint32_t *status;                 // [n_cand] the table's status words, or null
};

static unsigned long long pack_candidates(const uint8_t *candidates, int n_candidates) {
    unsigned long long cand = 0;
    for (int k = 0; k < n_candidates; k++) cand |= (unsigned long long)candidates[k] << (8 * k);
    return cand;
}

static void unpack_candidates(unsigned long long cand, uint8_t out[kMaxCandidates]) { // (for the kernels that take them as an array)
    for (int k = 0; k < kMaxCandidates; k++) out[k] = (uint8_t)(cand >> (8 * k));
}

// The first step of every encode that takes candidates: every frame at every candidate into the encoder's own table
// (d_probe_sizes, d_probe_dist [kMaxCandidates][max_frames], d_probe_status), which t then describes.  with_dist: the rd table,
// which only the fused pass makes.
static int own_table(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const uint8_t *candidates, int n_candidates, bool with_dist,
                     void *stream, PickTable &t) {
    if (with_dist && !e->plan.table_units) return fail(M1V_E_ARG, kNotFused);
    const int rc = with_dist ? size_table_fused(e, d_rgb, n_frames, candidates, n_candidates, e->d_probe_sizes, e->d_probe_dist,
                                                (size_t)e->max_frames, e->d_probe_status, (hipStream_t)stream)
                             : size_table(e, d_rgb, n_frames, candidates, n_candidates, e->d_probe_sizes, (size_t)e->max_frames,
                                          e->d_probe_status, stream);
    t = {e->d_probe_sizes, with_dist ? e->d_probe_dist : nullptr, e->max_frames, n_candidates, pack_candidates(candidates, n_candidates),
         e->d_probe_status};
    return rc;
}

// k_rd_chains over a table (an empty batch has none), and what k_rd_batch_pick behind it reads; its outputs are the caller's to set
static int rd_batch_chains(m1v_encoder *e, const PickTable &t, int n_frames, int rule, uint64_t limit, hipStream_t st, RdBatchArgs &ba) {
    if (n_frames > 0) {
        RdChainArgs ca = {t.sizes, t.dist, t.stride, t.n_cand, n_frames, t.status, e->d_rd_steps};
        hipLaunchKernelGGL(k_rd_chains, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, st, ca);
        HIP_TRY(hipGetLastError());
    }
    ba = {};
    ba.dist = t.dist; ba.stride = t.stride; ba.n_cand = t.n_cand; ba.cand = t.cand; ba.table_status = t.status; // the table
    ba.steps = e->d_rd_steps;
    ba.n_frames = n_frames;
    ba.rule = rule;
    ba.limit = limit;
    return M1V_OK;
}

// k_rd_cbr_pick over a table (an empty batch too: it writes the level); ca comes with its outputs set (picks, chosen, pick_dist, status)
static int launch_rd_cbr_pick(const PickTable &t, int n_frames, uint64_t bytes_per_frame, uint64_t buffer_bytes, const int64_t *d_level_in,
                              int64_t *d_level_out, RdCbrArgs ca, hipStream_t st) {
    ca.sizes = t.sizes; ca.dist = t.dist; ca.stride = t.stride; ca.n_cand = t.n_cand; ca.cand = t.cand; ca.table_status = t.status; // the table
    ca.n_frames = n_frames;
    ca.rate = (long long)bytes_per_frame;
    ca.capacity = (long long)buffer_bytes;
    ca.level_in = (const long long *)d_level_in;
    ca.level_out = (long long *)d_level_out;
    hipLaunchKernelGGL(k_rd_cbr_pick, dim3(1), dim3(kPickThreads), 0, st, ca);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

// ---- the encodes that take candidates: their own checks, the table (own_table), their rule's parameters, the pick and encode ---
int m1v_encode_budget_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                             const uint8_t *candidates, int n_candidates, uint64_t max_frame_bytes,
                             const uint64_t *d_max_frame_bytes, uint8_t *d_chosen,
                             uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                             uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out)) return rc;
    PickTable t;
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, false, stream, t)) return rc;
    QualityArgs qa = {}; // k_frame_quality's budget form is the pick
    qa.probe_sizes = t.sizes; qa.stride = t.stride; qa.n_cand = t.n_cand; qa.probe_status = t.status; // the table
    unpack_candidates(t.cand, qa.cand);
    qa.budget = (const unsigned long long *)d_max_frame_bytes;
    qa.max_bytes = max_frame_bytes;
    qa.chosen = d_chosen ? d_chosen : e->d_chosen;
    const Selection sel = {select_by_quality, &qa};
    return encode_batch(e, d_rgb, n_frames, first_frame_index, &sel, false, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_encode_rd_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                         const uint8_t *candidates, int n_candidates, int rule, uint64_t limit, const uint64_t *d_limits,
                         uint8_t *d_chosen, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                         uint64_t *d_frame_distortion, uint64_t *d_total, uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out)) return rc;
    if (const int rc = check_rd_rule(rule)) return rc;
    PickTable t;
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, true, stream, t)) return rc;
    RdPickArgs ra = {};
    ra.sizes = t.sizes; ra.dist = t.dist; ra.stride = t.stride; ra.n_cand = t.n_cand; ra.table_status = t.status; // the table
    unpack_candidates(t.cand, ra.cand);
    ra.rule = rule;
    ra.limits = (const unsigned long long *)d_limits;
    ra.limit = limit;
    ra.chosen = d_chosen;
    ra.frame_dist = (unsigned long long *)d_frame_distortion;
    const Selection sel = {select_by_rd, &ra};
    return encode_batch(e, d_rgb, n_frames, first_frame_index, &sel, false, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

// A batch-budget or bitrate call after its arguments are checked: the size table, the pick (k_rate_pick, one workgroup) and the
// encode at the picked qualities, all on `stream` with no host wait.  pa holds the rule's parameters; the rest is set here.
static int rate_encode(m1v_encoder *e, PickArgs &pa, bool cbr, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                       const uint8_t *candidates, int n_candidates, uint8_t *d_chosen, const EncodeOut &o, void *stream) {
    PickTable t;
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, false, stream, t)) return rc;
    pa.sizes = t.sizes; pa.stride = t.stride; pa.n_cand = t.n_cand; pa.cand = t.cand; pa.table_status = t.status; // the table
    pa.n_frames = n_frames;
    pa.chosen = d_chosen ? d_chosen : e->d_chosen;
    pa.status = e->d_pick_status;
    const auto pick = cbr ? k_rate_pick<true> : k_rate_pick<false>;
    hipLaunchKernelGGL(pick, dim3(1), dim3(kPickThreads), 0, (hipStream_t)stream, pa);
    HIP_TRY(hipGetLastError());
    return encode_at(e, d_rgb, n_frames, first_frame_index, pa.chosen, pa.status, false, o, stream);
}

int m1v_encode_batch_budget_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                                   const uint8_t *candidates, int n_candidates, uint64_t batch_bytes, uint8_t *d_chosen,
                                   uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                                   uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out)) return rc;
    PickArgs pa = {};
    pa.budget = batch_bytes;
    return rate_encode(e, pa, false, d_rgb, n_frames, first_frame_index, candidates, n_candidates, d_chosen,
                       {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_encode_cbr_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                          const uint8_t *candidates, int n_candidates, uint64_t bytes_per_frame, uint64_t buffer_bytes,
                          const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_chosen,
                          uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_total,
                          uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out && d_level_in && d_level_out))
        return rc;
    if (const int rc = check_cbr_rate(bytes_per_frame, buffer_bytes)) return rc;
    PickArgs pa = {};
    pa.rate = (long long)bytes_per_frame;
    pa.capacity = (long long)buffer_bytes;
    pa.level_in = (const long long *)d_level_in;
    pa.level_out = (long long *)d_level_out;
    return rate_encode(e, pa, true, d_rgb, n_frames, first_frame_index, candidates, n_candidates, d_chosen,
                       {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

// ---- batch budgets and constant bitrate that pick by distortion (m1v_rd_rate.h) -------------------------------------------------
int m1v_encode_rd_batch_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                               const uint8_t *candidates, int n_candidates, int rule, uint64_t limit, uint8_t *d_chosen,
                               uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_frame_distortion,
                               uint64_t *d_total, uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out)) return rc;
    if (const int rc = check_rd_rule(rule)) return rc;
    PickTable t;
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, true, stream, t)) return rc;
    RdBatchArgs ba;
    if (const int rc = rd_batch_chains(e, t, n_frames, rule, limit, (hipStream_t)stream, ba)) return rc;
    ba.chosen = d_chosen ? d_chosen : e->d_chosen;
    ba.pick_dist = (unsigned long long *)d_frame_distortion;
    ba.status = e->d_pick_status;
    const Selection sel = {select_by_rd_batch, &ba};
    return encode_batch(e, d_rgb, n_frames, first_frame_index, &sel, false, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_encode_rd_cbr_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int first_frame_index,
                             const uint8_t *candidates, int n_candidates, uint64_t bytes_per_frame, uint64_t buffer_bytes,
                             const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_chosen,
                             uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes, uint64_t *d_frame_distortion,
                             uint64_t *d_total, uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out && d_level_in && d_level_out))
        return rc;
    if (const int rc = check_cbr_rate(bytes_per_frame, buffer_bytes)) return rc;
    PickTable t;
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, true, stream, t)) return rc;
    RdCbrArgs out = {};
    out.chosen = d_chosen ? d_chosen : e->d_chosen;
    out.pick_dist = (unsigned long long *)d_frame_distortion;
    out.status = e->d_pick_status;
    if (const int rc = launch_rd_cbr_pick(t, n_frames, bytes_per_frame, buffer_bytes, d_level_in, d_level_out, out, (hipStream_t)stream)) return rc;
    return encode_at(e, d_rgb, n_frames, first_frame_index, out.chosen, out.status, false, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

// The picks alone, on a table the caller holds ([k * n_frames + f])
int m1v_rd_batch_pick_device(m1v_encoder *e, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                             int n_frames, int n_candidates, int rule, uint64_t limit, uint8_t *d_picks,
                             uint64_t *d_pick_distortion, uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, d_sizes && d_distortion && d_picks && d_status, nullptr, n_candidates, n_frames, true, true)) return rc;
    if (const int rc = check_rd_rule(rule)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    if (n_frames == 0) {
        HIP_TRY(hipMemsetAsync(d_status, 0, 4, (hipStream_t)stream));
        return M1V_OK;
    }
    const PickTable t = {(const unsigned long long *)d_sizes, (const unsigned long long *)d_distortion, n_frames, n_candidates, 0, d_table_status};
    RdBatchArgs ba;
    if (const int rc = rd_batch_chains(e, t, n_frames, rule, limit, (hipStream_t)stream, ba)) return rc;
    ba.picks = d_picks;
    ba.pick_dist = (unsigned long long *)d_pick_distortion;
    ba.status = d_status;
    return launch_rd_batch_pick(ba, nullptr, (hipStream_t)stream);
}

int m1v_rd_cbr_pick_device(m1v_encoder *e, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                           int n_frames, int n_candidates, uint64_t bytes_per_frame, uint64_t buffer_bytes,
                           const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_picks, uint64_t *d_pick_distortion,
                           uint32_t *d_status, void *stream) {
    if (const int rc = check_candidate_call(e, d_sizes && d_distortion && d_picks && d_status, nullptr, n_candidates, n_frames,
                                            d_level_in && d_level_out, true))
        return rc;
    if (const int rc = check_cbr_rate(bytes_per_frame, buffer_bytes)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const PickTable t = {(const unsigned long long *)d_sizes, (const unsigned long long *)d_distortion, n_frames, n_candidates, 0, d_table_status};
    RdCbrArgs out = {};
    out.picks = d_picks;
    out.pick_dist = (unsigned long long *)d_pick_distortion;
    out.status = d_status;
    return launch_rd_cbr_pick(t, n_frames, bytes_per_frame, buffer_bytes, d_level_in, d_level_out, out, (hipStream_t)stream);
}

// ---- batches of many streams (m1v_streams.h) ----------------------------------------------------------------------------------
} // extern "C"

static int check_spans(const m1v_stream_span *d_spans, int n_streams) {
    if (!d_spans) return fail(M1V_E_ARG, "null spans%s");
    if (n_streams < 1 || n_streams > M1V_MAX_STREAMS) return fail(M1V_E_ARG, "n_streams must be 1 .. M1V_MAX_STREAMS%s");
    if ((uintptr_t)d_spans & 3) return fail(M1V_E_ARG, "the spans must be 4-byte aligned%s");
    return M1V_OK;
}

static int check_streams_rule(int rule) {
    return rule == M1V_STREAMS_LARGEST_THAT_FITS || rule == M1V_STREAMS_LEAST_DISTORTION ? M1V_OK : fail(M1V_E_ARG, "unknown streams rule%s");
}

// k_streams_bitrate over a table (an empty batch too: it writes the levels).  ra comes with its outputs, spans and rates set; its
// status word is cleared here, in front of the launch.
static int launch_streams_bitrate(const PickTable &t, int n_frames, int rule, StreamsRateArgs ra, hipStream_t st) {
    ra.sizes = t.sizes; ra.dist = t.dist; ra.stride = t.stride; ra.n_cand = t.n_cand; ra.cand = t.cand; ra.table_status = t.status; // the table
    ra.n_frames = n_frames;
    HIP_TRY(hipMemsetAsync(ra.status, 0, 4, st));
    const dim3 grid((unsigned)((ra.n_streams + kStreamsWaves - 1) / kStreamsWaves)), block(kStreamsWaves * kWave);
    if (rule == M1V_STREAMS_LEAST_DISTORTION)
        hipLaunchKernelGGL(k_streams_bitrate<M1V_STREAMS_LEAST_DISTORTION>, grid, block, 0, st, ra);
    else
        hipLaunchKernelGGL(k_streams_bitrate<M1V_STREAMS_LARGEST_THAT_FITS>, grid, block, 0, st, ra);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

static int check_spans_rule(int rule) {
    return rule == M1V_SPANS_LARGEST_THAT_FITS || rule == M1V_SPANS_LEAST_DISTORTION || rule == M1V_SPANS_SMALLEST_AT_DISTORTION
               ? M1V_OK
               : fail(M1V_E_ARG, "unknown spans rule%s");
}

// The budget per stream over a table (m1v_span_budget.h; an empty batch too: it writes the streams' status): k_span_plan into the
// encoder's prefix, k_rd_chains into its step table under the two rules that pick by distortion, then k_span_budget over
// n_streams + ceil(n_frames / 32) workgroups.  ba comes with its outputs, spans and limits set; its status word is cleared here,
// in front of the launches.  batch_status: an encode's status word, or null.
static int launch_span_budget(m1v_encoder *e, const PickTable &t, int n_frames, int rule, SpanBudgetArgs ba, uint32_t *batch_status, hipStream_t st) {
    ba.sizes = t.sizes; ba.dist = t.dist; ba.stride = t.stride; ba.n_cand = t.n_cand; ba.cand = t.cand; ba.table_status = t.status; // the table
    ba.n_frames = n_frames;
    ba.steps = e->d_rd_steps;
    ba.chunk_at = e->d_span_chunks;
    ba.batch_status = batch_status;
    HIP_TRY(hipMemsetAsync(ba.status, 0, 4, st));
    const SpanPlanArgs pa = {ba.spans, ba.n_streams, n_frames, e->d_span_chunks, ba.picks, ba.chosen, (uint8_t)t.cand}; // (byte 0: candidate 0)
    hipLaunchKernelGGL(k_span_plan, dim3(1), dim3(kSpanThreads), 0, st, pa);
    HIP_TRY(hipGetLastError());
    if (rule != M1V_SPANS_LARGEST_THAT_FITS && n_frames > 0) {
        const RdChainArgs ca = {t.sizes, t.dist, t.stride, t.n_cand, n_frames, t.status, e->d_rd_steps};
        hipLaunchKernelGGL(k_rd_chains, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, st, ca);
        HIP_TRY(hipGetLastError());
    }
    const dim3 grid((unsigned)(ba.n_streams + (n_frames + kSpanFrames - 1) / kSpanFrames)), block(kSpanThreads);
    if (rule == M1V_SPANS_LARGEST_THAT_FITS)
        hipLaunchKernelGGL(k_span_budget<M1V_SPANS_LARGEST_THAT_FITS>, grid, block, 0, st, ba);
    else if (rule == M1V_SPANS_LEAST_DISTORTION)
        hipLaunchKernelGGL(k_span_budget<M1V_SPANS_LEAST_DISTORTION>, grid, block, 0, st, ba);
    else
        hipLaunchKernelGGL(k_span_budget<M1V_SPANS_SMALLEST_AT_DISTORTION>, grid, block, 0, st, ba);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

// What a streams batch hands its Selection: the spans; the per-frame qualities, if any, and what wrote them (`bitrate` with `table`
// and `rule`: k_streams_bitrate; `budget` with `table`, `rule` and `ba`: the budget per stream; either is launched by the step,
// where the batch's status word is known); where the spans' bytes go.
struct StreamsStep {
    const m1v_stream_span *spans;
    int n_streams;
    QualityArgs qa;          // qa.quality null: the encoder's own quality
    bool bitrate;
    PickTable table;
    int rule;
    StreamsRateArgs ra;
    unsigned long long *stream_bytes;
    bool budget;
    SpanBudgetArgs ba;
};

static int select_streams(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, int n_frames, hipStream_t st) {
    StreamsStep &s = *static_cast<StreamsStep *>(args);
    const StreamsMapArgs ma = {s.spans, s.n_streams, n_frames, cur.frame_index, cur.words};
    hipLaunchKernelGGL(k_streams_map, dim3((unsigned)((s.n_streams + 255) / 256)), dim3(256), 0, st, ma);
    HIP_TRY(hipGetLastError());
    if (s.bitrate) {
        s.ra.batch_status = cur.words;
        if (const int rc = launch_streams_bitrate(s.table, n_frames, s.rule, s.ra, st)) return rc;
    }
    return s.qa.quality ? select_by_quality(e, &s.qa, cur, n_frames, st) : M1V_OK;
}

// The step of a batch with a budget per stream: the map, then the plan, the chains and the pick (launch_span_budget), then
// k_frame_quality on the qualities and the status word the pick wrote
static int select_span_budget(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, int n_frames, hipStream_t st) {
    StreamsStep &s = *static_cast<StreamsStep *>(args);
    const StreamsMapArgs ma = {s.spans, s.n_streams, n_frames, cur.frame_index, cur.words};
    hipLaunchKernelGGL(k_streams_map, dim3((unsigned)((s.n_streams + 255) / 256)), dim3(256), 0, st, ma);
    HIP_TRY(hipGetLastError());
    if (const int rc = launch_span_budget(e, s.table, n_frames, s.rule, s.ba, cur.words, st)) return rc;
    return select_by_quality(e, &s.qa, cur, n_frames, st);
}

static int finish_streams(m1v_encoder *e, void *args, const m1v_encoder::Counters &cur, const EncodeOut &o, int n_frames, hipStream_t gs) {
    const StreamsStep &s = *static_cast<StreamsStep *>(args);
    const int header_blocks = (n_frames + kStreamsFinishThreads - 1) / kStreamsFinishThreads;
    const int span_blocks = s.stream_bytes ? (s.n_streams + kStreamsFinishThreads / kWave - 1) / (kStreamsFinishThreads / kWave) : 0;
    const StreamsFinishArgs fa = {s.spans, s.n_streams, n_frames, cur.frame_bytes, cur.frame_index, e->d_tab, o.out,
                                  (unsigned long long)o.cap, s.stream_bytes, header_blocks};
    hipLaunchKernelGGL(k_streams_finish, dim3((unsigned)(header_blocks + span_blocks)), dim3(kStreamsFinishThreads), 0, gs, fa);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

// The encode of a streams batch: the step above around encode_batch (index 0 for k_assemble; k_streams_finish sets the headers)
static int encode_streams(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, StreamsStep &s, const EncodeOut &o, void *stream) {
    if (n_frames == 0 && s.stream_bytes) {
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMemsetAsync(s.stream_bytes, 0, (size_t)s.n_streams * 8, (hipStream_t)stream));
    }
    Selection sel = {s.budget ? select_span_budget : select_streams, &s};
    sel.own_quality = !s.qa.quality;
    sel.finish = finish_streams;
    return encode_batch(e, d_rgb, n_frames, 0, &sel, false, o, stream);
}

extern "C" {

int m1v_encode_streams_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const m1v_stream_span *d_spans, int n_streams,
                              const uint8_t *d_quality, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                              uint64_t *d_stream_bytes, uint64_t *d_total, uint32_t *d_status, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = check_spans(d_spans, n_streams)) return rc;
    if ((!d_rgb && n_frames > 0) || !d_out) return fail(M1V_E_ARG, "null pointer%s");
    if (const int rc = check_batch_frames(e, n_frames)) return rc;
    StreamsStep s = {};
    s.spans = d_spans;
    s.n_streams = n_streams;
    s.qa.quality = d_quality;
    s.stream_bytes = (unsigned long long *)d_stream_bytes;
    return encode_streams(e, d_rgb, n_frames, s, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_encode_streams_cbr_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const m1v_stream_span *d_spans, int n_streams,
                                  const uint8_t *candidates, int n_candidates, int rule, uint64_t bytes_per_frame,
                                  uint64_t buffer_bytes, const m1v_stream_rate *d_stream_rates, const int64_t *d_level_in,
                                  int64_t *d_level_out, uint8_t *d_chosen, uint8_t *d_out, size_t out_cap, uint64_t *d_frame_sizes,
                                  uint64_t *d_frame_distortion, uint64_t *d_stream_bytes, uint64_t *d_total, uint32_t *d_status,
                                  void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = check_spans(d_spans, n_streams)) return rc;
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out && d_level_in && d_level_out))
        return rc;
    if (const int rc = check_streams_rule(rule)) return rc;
    if (((uintptr_t)d_stream_rates & 7) != 0) return fail(M1V_E_ARG, "the stream rates must be 8-byte aligned%s");
    if (!d_stream_rates)
        if (const int rc = check_cbr_rate(bytes_per_frame, buffer_bytes)) return rc;
    const bool by_dist = rule == M1V_STREAMS_LEAST_DISTORTION;
    StreamsStep s = {};
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, by_dist, stream, s.table)) return rc;
    s.spans = d_spans;
    s.n_streams = n_streams;
    s.bitrate = true;
    s.rule = rule;
    s.ra.spans = d_spans;
    s.ra.n_streams = n_streams;
    s.ra.rates = d_stream_rates;
    s.ra.rate = (long long)bytes_per_frame;
    s.ra.capacity = (long long)buffer_bytes;
    s.ra.level_in = (const long long *)d_level_in;
    s.ra.level_out = (long long *)d_level_out;
    s.ra.chosen = d_chosen ? d_chosen : e->d_chosen;
    s.ra.pick_dist = (unsigned long long *)d_frame_distortion;
    s.ra.status = e->d_pick_status;
    s.qa.quality = s.ra.chosen;
    s.qa.pick_status = s.ra.status;
    s.stream_bytes = (unsigned long long *)d_stream_bytes;
    if (n_frames == 0) // (an empty batch has no Selection step: the pick alone moves the levels)
        if (const int rc = launch_streams_bitrate(s.table, 0, rule, s.ra, (hipStream_t)stream)) return rc;
    return encode_streams(e, d_rgb, n_frames, s, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_streams_cbr_pick_device(m1v_encoder *e, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                                int n_frames, int n_candidates, const m1v_stream_span *d_spans, int n_streams, int rule,
                                uint64_t bytes_per_frame, uint64_t buffer_bytes, const m1v_stream_rate *d_stream_rates,
                                const int64_t *d_level_in, int64_t *d_level_out, uint8_t *d_picks, uint64_t *d_pick_distortion,
                                uint32_t *d_status, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = check_spans(d_spans, n_streams)) return rc;
    if (const int rc = check_streams_rule(rule)) return rc;
    const bool by_dist = rule == M1V_STREAMS_LEAST_DISTORTION;
    if (const int rc = check_candidate_call(e, d_sizes && (d_distortion || !by_dist) && d_picks && d_status, nullptr, n_candidates, n_frames,
                                            d_level_in && d_level_out, true))
        return rc;
    if (((uintptr_t)d_stream_rates & 7) != 0) return fail(M1V_E_ARG, "the stream rates must be 8-byte aligned%s");
    if (!d_stream_rates)
        if (const int rc = check_cbr_rate(bytes_per_frame, buffer_bytes)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const PickTable t = {(const unsigned long long *)d_sizes, (const unsigned long long *)d_distortion, n_frames, n_candidates, 0, d_table_status};
    StreamsRateArgs ra = {};
    ra.spans = d_spans;
    ra.n_streams = n_streams;
    ra.rates = d_stream_rates;
    ra.rate = (long long)bytes_per_frame;
    ra.capacity = (long long)buffer_bytes;
    ra.level_in = (const long long *)d_level_in;
    ra.level_out = (long long *)d_level_out;
    ra.picks = d_picks;
    ra.pick_dist = (unsigned long long *)d_pick_distortion;
    ra.status = d_status;
    return launch_streams_bitrate(t, n_frames, rule, ra, (hipStream_t)stream);
}

int m1v_encode_streams_budget_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, const m1v_stream_span *d_spans, int n_streams,
                                     const uint8_t *candidates, int n_candidates, int rule, uint64_t limit,
                                     const uint64_t *d_stream_limits, uint8_t *d_chosen, uint8_t *d_out, size_t out_cap,
                                     uint64_t *d_frame_sizes, uint64_t *d_frame_distortion, uint64_t *d_stream_bytes,
                                     uint32_t *d_stream_status, uint64_t *d_total, uint32_t *d_status, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = check_spans(d_spans, n_streams)) return rc;
    if (const int rc = check_candidate_call(e, true, candidates, n_candidates, n_frames, (d_rgb || n_frames <= 0) && d_out)) return rc;
    if (const int rc = check_spans_rule(rule)) return rc;
    if (((uintptr_t)d_stream_limits & 7) != 0) return fail(M1V_E_ARG, "the stream limits must be 8-byte aligned%s");
    StreamsStep s = {};
    if (const int rc = own_table(e, d_rgb, n_frames, candidates, n_candidates, rule != M1V_SPANS_LARGEST_THAT_FITS, stream, s.table)) return rc;
    s.spans = d_spans;
    s.n_streams = n_streams;
    s.budget = true;
    s.rule = rule;
    s.ba.spans = d_spans;
    s.ba.n_streams = n_streams;
    s.ba.limits = (const unsigned long long *)d_stream_limits;
    s.ba.limit = limit;
    s.ba.chosen = d_chosen ? d_chosen : e->d_chosen;
    s.ba.pick_dist = (unsigned long long *)d_frame_distortion;
    s.ba.stream_status = d_stream_status;
    s.ba.status = e->d_pick_status;
    s.qa.quality = s.ba.chosen;
    s.qa.pick_status = s.ba.status;
    s.stream_bytes = (unsigned long long *)d_stream_bytes;
    if (n_frames == 0 && d_stream_status) { // (an empty batch has no Selection step)
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMemsetAsync(d_stream_status, 0, (size_t)n_streams * 4, (hipStream_t)stream));
    }
    return encode_streams(e, d_rgb, n_frames, s, {d_out, out_cap, d_frame_sizes, d_total, d_status}, stream);
}

int m1v_streams_budget_pick_device(m1v_encoder *e, const uint64_t *d_sizes, const uint64_t *d_distortion, const uint32_t *d_table_status,
                                   int n_frames, int n_candidates, const m1v_stream_span *d_spans, int n_streams, int rule,
                                   uint64_t limit, const uint64_t *d_stream_limits, uint8_t *d_picks, uint64_t *d_pick_distortion,
                                   uint32_t *d_stream_status, uint32_t *d_status, void *stream) {
    if (!e) return fail(M1V_E_ARG, "null encoder%s");
    if (const int rc = check_spans(d_spans, n_streams)) return rc;
    if (const int rc = check_spans_rule(rule)) return rc;
    const bool by_dist = rule != M1V_SPANS_LARGEST_THAT_FITS;
    if (const int rc = check_candidate_call(e, d_sizes && (d_distortion || !by_dist) && d_picks && d_status, nullptr, n_candidates, n_frames, true, true))
        return rc;
    if (((uintptr_t)d_stream_limits & 7) != 0) return fail(M1V_E_ARG, "the stream limits must be 8-byte aligned%s");
    HIP_TRY(hipSetDevice(e->device));
    const PickTable t = {(const unsigned long long *)d_sizes, (const unsigned long long *)d_distortion, n_frames, n_candidates, 0, d_table_status};
    SpanBudgetArgs ba = {};
    ba.spans = d_spans;
    ba.n_streams = n_streams;
    ba.limits = (const unsigned long long *)d_stream_limits;
    ba.limit = limit;
    ba.picks = d_picks;
    ba.pick_dist = (unsigned long long *)d_pick_distortion;
    ba.stream_status = d_stream_status;
    ba.status = d_status;
    return launch_span_budget(e, t, n_frames, rule, ba, nullptr, (hipStream_t)stream);
}

// ---- overlapped delivery to the host (include/mpeg1_hip.h) ----------------------------------------------------------
struct m1v_delivery {
    m1v_encoder *e;
    int device; // (the encoder may be destroyed before the delivery object is)
    size_t cap;
    int max_frames;
    uint8_t *d_out[2], *h_out[2];
    unsigned long long *d_meta[2], *h_meta[2];   // [0] total bytes, [1] status word (low 32 bits)
    unsigned long long *d_sizes[2], *h_sizes[2];
    hipStream_t side;
    hipEvent_t encoded[2], counted[2], delivered[2];
    bool in_flight[2];                            // delivered[b] has been recorded and not yet been waited for by an encode
    struct {
        const uint8_t *rgb;
        int n, first;
    } args[2];
    int pending;                                  // slot whose batch is encoded (or encoding) and not yet on its way, or -1
    unsigned step_no;
};

static int delivery_start(m1v_delivery *d, int b) { // the copy of slot b's batch, behind its encode
    m1v_encoder *e = d->e;
    HIP_TRY(hipStreamWaitEvent(d->side, d->encoded[b], 0));
    HIP_TRY(hipMemcpyAsync(d->h_meta[b], d->d_meta[b], 16, hipMemcpyDeviceToHost, d->side));
    HIP_TRY(hipEventRecord(d->counted[b], d->side));
    HIP_TRY(hipEventSynchronize(d->counted[b])); // the step's only host wait: the next encode is already queued
    unsigned long long total = d->h_meta[b][0];
    uint32_t status = (uint32_t)d->h_meta[b][1];
    if (status == M1V_STATUS_SCRATCH) { // recoverable: the worst case reserved (waits for the device), the same frames again
        int rc = m1v_reserve_scratch(e, 1);
        if (rc != M1V_OK) return rc;
        rc = m1v_encode_device(e, d->args[b].rgb, d->args[b].n, d->args[b].first, d->d_out[b], d->cap, (uint64_t *)d->d_sizes[b],
                               (uint64_t *)d->d_meta[b], reinterpret_cast<uint32_t *>(d->d_meta[b] + 1), d->side);
        if (rc != M1V_OK) return rc;
        if (e->pipelined) HIP_TRY(hipStreamWaitEvent(d->side, e->batch[(e->calls - 1u) & 1u].gather_done, 0));
        HIP_TRY(hipMemcpyAsync(d->h_meta[b], d->d_meta[b], 16, hipMemcpyDeviceToHost, d->side));
        HIP_TRY(hipStreamSynchronize(d->side));
        total = d->h_meta[b][0];
        status = (uint32_t)d->h_meta[b][1];
    }
    if (status & M1V_STATUS_UNENCODABLE) return fail(M1V_E_UNENCODABLE, "a level of 256 or more: the reference cannot code this batch%s");
    if (status & M1V_STATUS_NOSPACE) return fail(M1V_E_NOSPACE, "the delivery's output buffers are too small for this batch%s");
    if (status) return fail(M1V_E_SCRATCH, "the batch ran out of scratch twice%s");
    if (total > d->cap) return fail(M1V_E_NOSPACE, "the delivery's output buffers are too small for this batch%s");
    HIP_TRY(hipMemcpyAsync(d->h_out[b], d->d_out[b], total, hipMemcpyDeviceToHost, d->side));
    HIP_TRY(hipMemcpyAsync(d->h_sizes[b], d->d_sizes[b], (size_t)d->args[b].n * 8, hipMemcpyDeviceToHost, d->side));
    HIP_TRY(hipEventRecord(d->delivered[b], d->side));
    d->in_flight[b] = true;
    return b;
}

int m1v_delivery_create(m1v_encoder *e, size_t out_cap, m1v_delivery **out) {
    if (!e || !out) return fail(M1V_E_ARG, "null pointer%s");
    *out = nullptr;
    HIP_TRY(hipSetDevice(e->device));
    m1v_delivery *d = new m1v_delivery();
    memset(d, 0, sizeof *d);
    d->e = e;
    d->device = e->device;
    d->max_frames = e->max_frames;
    d->cap = out_cap ? out_cap : (size_t)e->max_frames * m1v_frame_bound(e);
    d->pending = -1;
    hipError_t err = hipStreamCreateWithFlags(&d->side, hipStreamNonBlocking);
    for (int b = 0; b < 2; b++) {
        if (err == hipSuccess) err = hipMalloc(&d->d_out[b], d->cap);
        if (err == hipSuccess) err = hipMalloc(&d->d_meta[b], 16);
        if (err == hipSuccess) err = hipMemset(d->d_meta[b], 0, 16);
        if (err == hipSuccess) err = hipMalloc(&d->d_sizes[b], (size_t)e->max_frames * 8);
        if (err == hipSuccess) err = hipHostMalloc(&d->h_out[b], d->cap, hipHostMallocDefault);
        if (err == hipSuccess) err = hipHostMalloc(&d->h_meta[b], 16, hipHostMallocDefault);
        if (err == hipSuccess) err = hipHostMalloc(&d->h_sizes[b], (size_t)e->max_frames * 8, hipHostMallocDefault);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&d->encoded[b], hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&d->counted[b], hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&d->delivered[b], hipEventDisableTiming);
    }
    if (err != hipSuccess) {
        fail(M1V_E_HIP, "allocation failed: %s", hipGetErrorString(err));
        m1v_delivery_destroy(d);
        return M1V_E_HIP;
    }
    *out = d;
    return M1V_OK;
}

void m1v_delivery_destroy(m1v_delivery *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->side) (void)hipStreamSynchronize(d->side);
    for (int b = 0; b < 2; b++) {
        (void)hipFree(d->d_out[b]);
        (void)hipFree(d->d_meta[b]);
        (void)hipFree(d->d_sizes[b]);
        (void)hipHostFree(d->h_out[b]);
        (void)hipHostFree(d->h_meta[b]);
        (void)hipHostFree(d->h_sizes[b]);
        if (d->encoded[b]) (void)hipEventDestroy(d->encoded[b]);
        if (d->counted[b]) (void)hipEventDestroy(d->counted[b]);
        if (d->delivered[b]) (void)hipEventDestroy(d->delivered[b]);
    }
    if (d->side) (void)hipStreamDestroy(d->side);
    delete d;
}

int m1v_delivery_step(m1v_delivery *d, const uint8_t *d_rgb, int n_frames, int first_frame_index, void *stream) {
    if (!d || !d_rgb) return fail(M1V_E_ARG, "null pointer%s");
    if (n_frames <= 0 || n_frames > d->max_frames) return fail(M1V_E_ARG, "n_frames exceeds max_frames%s");
    m1v_encoder *e = d->e;
    if (const int rc = check_batch_frames(e, n_frames)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(e->device));
    const int b = (int)(d->step_no++ & 1u);
    if (d->in_flight[b]) { // slot b's previous batch has left for the host before its buffers are written again
        HIP_TRY(hipStreamWaitEvent(st, d->delivered[b], 0));
        d->in_flight[b] = false;
    }
    const int rc = m1v_encode_device(e, d_rgb, n_frames, first_frame_index, d->d_out[b], d->cap, (uint64_t *)d->d_sizes[b],
                                     (uint64_t *)d->d_meta[b], reinterpret_cast<uint32_t *>(d->d_meta[b] + 1), st);
    if (rc != M1V_OK) { // slot b holds no batch: the next step uses it again, the pending batch in the other slot is untouched
        d->step_no--;
        return rc;
    }
    if (e->pipelined) HIP_TRY(m1v_flush(e, st) == M1V_OK ? hipSuccess : hipErrorUnknown);
    HIP_TRY(hipEventRecord(d->encoded[b], st));
    d->args[b].rgb = d_rgb;
    d->args[b].n = n_frames;
    d->args[b].first = first_frame_index;
    const int before = d->pending;
    d->pending = b;
    return before >= 0 ? delivery_start(d, before) : (int)M1V_DELIVERY_NONE;
}

int m1v_delivery_flush(m1v_delivery *d) {
    if (!d) return fail(M1V_E_ARG, "null pointer%s");
    HIP_TRY(hipSetDevice(d->e->device));
    const int before = d->pending;
    d->pending = -1;
    return before >= 0 ? delivery_start(d, before) : (int)M1V_DELIVERY_NONE;
}

uint64_t m1v_delivery_bytes(const m1v_delivery *d, int slot) { return d && slot >= 0 && slot <= 1 ? d->h_meta[slot][0] : 0; }

int m1v_delivery_wait(m1v_delivery *d, int slot, const uint8_t **host, uint64_t *bytes, const uint64_t **frame_sizes) {
    if (!d || slot < 0 || slot > 1) return fail(M1V_E_ARG, "bad slot%s");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipEventSynchronize(d->delivered[slot]));
    if (host) *host = d->h_out[slot];
    if (bytes) *bytes = d->h_meta[slot][0];
    if (frame_sizes) *frame_sizes = (const uint64_t *)d->h_sizes[slot];
    return M1V_OK;
}

/* Pinned host memory for callers of the host-buffer entry points: H2D/D2H copies from it run at the PCIe
 * rate instead of being staged by the runtime. */
void *m1v_alloc_host(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void *m1v_alloc_device(size_t bytes) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void m1v_free_device(void *p) { (void)hipFree(p); }
void m1v_free_host(void *p) {
    if (p) (void)hipHostFree(p);
}

long m1v_encode_planes_host(m1v_encoder *e, const uint8_t *rgb, int n_frames, int first_frame_index,
                            uint8_t *out, size_t out_cap, uint64_t *frame_sizes, uint8_t *planes) {
    if (!e || !rgb || !out) return fail(M1V_E_ARG, "null pointer%s");
    if (const int rc = packed_only(e)) return rc;
    if (const int rc = check_batch_frames(e, n_frames)) return rc;
    if (n_frames == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const size_t frame_in = (size_t)e->g.frame_bytes, frame_planes = (size_t)e->g.W * e->g.H * 3;
    size_t in_bytes = frame_in * n_frames;
    size_t bound = m1v_frame_bound(e) * (size_t)n_frames;
    size_t dcap = out_cap < bound ? out_cap : bound;
    m1v_encoder::HostPath &hp = e->hp;
    HIP_TRY(ensure_device(&hp.d_in, &hp.in_cap, in_bytes));
    HIP_TRY(ensure_device(&hp.d_out, &hp.out_cap, dcap));
    HIP_TRY(ensure_device(&hp.d_meta, &hp.meta_cap, (size_t)(n_frames + 2) * 8)); // [n] sizes, total, status
    if (planes) HIP_TRY(ensure_device(&hp.d_planes, &hp.planes_cap, frame_planes * n_frames));
    if (!hp.copy_in) { // all or nothing: a half-built set must not survive into the next call
        hipError_t err = hipStreamCreateWithFlags(&hp.copy_in, hipStreamNonBlocking);
        if (err == hipSuccess) err = hipStreamCreateWithFlags(&hp.work, hipStreamNonBlocking);
        for (hipEvent_t &ev : hp.uploaded)
            if (err == hipSuccess) err = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (err != hipSuccess) {
            if (hp.copy_in) (void)hipStreamDestroy(hp.copy_in);
            if (hp.work) (void)hipStreamDestroy(hp.work);
            for (hipEvent_t &ev : hp.uploaded) {
                if (ev) (void)hipEventDestroy(ev);
                ev = nullptr;
            }
            hp.copy_in = hp.work = nullptr;
            return fail(M1V_E_HIP, "stream creation failed: %s", hipGetErrorString(err));
        }
    }
    // From here on copies to and from the caller's buffers are in flight: every error return first waits for both
    // streams, so that the caller may free (or reuse) rgb / planes / out as soon as this function has returned.
    auto drained = [&](int rc) {
        (void)hipStreamSynchronize(hp.copy_in);
        (void)hipStreamSynchronize(hp.work);
        return rc;
    };
#define HIP_TRY_DRAIN(expr)                                                                        \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return drained(fail(M1V_E_HIP, #expr ": %s", hipGetErrorString(e_))); \
    } while (0)
    // copy_in: H2D half A, H2D half B.   work: [planes A -> host] while B uploads, [planes B -> host], encode all.
    const int half[3] = {0, planes && n_frames > 1 ? n_frames / 2 : n_frames, n_frames};
    for (int h = 0; h < 2; h++) {
        int f0 = half[h], nf = half[h + 1] - half[h];
        if (nf == 0) continue;
        HIP_TRY_DRAIN(hipMemcpyAsync(hp.d_in + frame_in * f0, rgb + frame_in * f0, frame_in * nf, hipMemcpyHostToDevice, hp.copy_in));
        HIP_TRY_DRAIN(hipEventRecord(hp.uploaded[h], hp.copy_in));
        HIP_TRY_DRAIN(hipStreamWaitEvent(hp.work, hp.uploaded[h], 0));
        if (planes) {
            int rc = m1v_convert_device(e, hp.d_in + frame_in * f0, nf, hp.d_planes + frame_planes * f0, hp.work);
            if (rc != M1V_OK) return drained(rc);
            HIP_TRY_DRAIN(hipMemcpyAsync(planes + frame_planes * f0, hp.d_planes + frame_planes * f0, frame_planes * nf,
                                   hipMemcpyDeviceToHost, hp.work));
        }
    }
    std::vector<unsigned long long> meta((size_t)n_frames + 2);
    uint32_t status = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        int r = m1v_encode_device(e, hp.d_in, n_frames, first_frame_index, hp.d_out, dcap, (uint64_t *)hp.d_meta,
                                  (uint64_t *)(hp.d_meta + n_frames), (uint32_t *)(hp.d_meta + n_frames + 1), hp.work);
        if (r != M1V_OK) return drained(r);
        if (m1v_flush(e, hp.work) != M1V_OK) return drained(M1V_E_HIP);
        HIP_TRY_DRAIN(hipMemcpyAsync(meta.data(), hp.d_meta, meta.size() * 8, hipMemcpyDeviceToHost, hp.work));
        HIP_TRY_DRAIN(hipStreamSynchronize(hp.work));
        status = (uint32_t)meta[(size_t)n_frames + 1];
        if (!(status & M1V_STATUS_SCRATCH) || attempt == 1) break;
        // more runs outgrew their compact scratch slot than the overflow arena holds: reserve the worst case, encode again
        int rr = m1v_reserve_scratch(e, 1);
        if (rr != M1V_OK) return drained(rr);
    }
    if (status & M1V_STATUS_SCRATCH) return drained(fail(M1V_E_SCRATCH, "scratch exhausted%s"));
    unsigned long long total = meta[n_frames];
    if (status & M1V_STATUS_UNENCODABLE)
        return fail(M1V_E_UNENCODABLE, "an AC level has |level| >= 256 (the reference crashes here)%s");
    if ((status & M1V_STATUS_NOSPACE) || total > out_cap) return fail(M1V_E_NOSPACE, "output buffer too small%s");
    HIP_TRY_DRAIN(hipMemcpy(out, hp.d_out, total, hipMemcpyDeviceToHost));
    if (frame_sizes)
        for (int f = 0; f < n_frames; f++) frame_sizes[f] = meta[f];
    return (long)total;
#undef HIP_TRY_DRAIN
}

long m1v_encode_host(m1v_encoder *e, const uint8_t *rgb, int n_frames, int first_frame_index,
                     uint8_t *out, size_t out_cap, uint64_t *frame_sizes) {
    return m1v_encode_planes_host(e, rgb, n_frames, first_frame_index, out, out_cap, frame_sizes, nullptr);
}

int m1v_coefficients_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, int16_t *d_coeffs,
                            void *stream) {
    if (!e || !d_rgb || !d_coeffs || n_frames < 0) return fail(M1V_E_ARG, "bad argument%s");
    if (const int rc = packed_only(e)) return rc;
    if (n_frames == 0) return M1V_OK;
    HIP_TRY(hipSetDevice(e->device));
    CoefArgs a;
    a.g = e->g;
    a.rgb = d_rgb;
    a.tab = e->d_tab;
    a.out = d_coeffs;
    a.n_frames = n_frames;
    if (e->g.C == 3 && !e->runs_by_path_or_mode()) { // tiles (any width, any alignment); the run-shaped kernel serves 4 channels
        CoefTileArgs t;
        t.g = e->g;
        t.rgb = d_rgb;
        t.tab = e->d_tab;
        t.out = d_coeffs;
        t.n_frames = n_frames;
        const TileGrid grid(e->g);
        t.tile_cols = grid.cols;
        t.tile_rows = grid.rows;
        t.tiles_per_frame = grid.units();
        t.region = wave_region(kCoefStride);
        hipLaunchKernelGGL((k_coefficient_tiles<M1V_TILE_RING>), dim3((unsigned)((size_t)n_frames * t.tiles_per_frame)),
                           dim3(kTileThreads), 3 * (size_t)t.region, (hipStream_t)stream, t);
        HIP_TRY(hipGetLastError());
        return M1V_OK;
    }
    // (the batch's frames are this grid's z: the long-batch rule; the tile form above has a one-dimensional grid.  The call is
    // not bound by max_frames: it uses no scratch)
    if (const int rc = check_grid_frames(e, n_frames)) return rc;
    int bps = e->g.n_mbrows * 6;
    dim3 grid((bps + 255) / 256, e->g.n_strips, n_frames);
    if (fast_path(e, d_rgb))
        hipLaunchKernelGGL(k_coefficients<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_coefficients<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

int m1v_convert_device(m1v_encoder *e, const uint8_t *d_rgb, int n_frames, uint8_t *d_planes,
                       void *stream) {
    if (!e || !d_rgb || !d_planes || n_frames < 0) return fail(M1V_E_ARG, "bad argument%s");
    if (const int rc = packed_only(e)) return rc;
    if (n_frames == 0) return M1V_OK;
    HIP_TRY(hipSetDevice(e->device));
    unsigned long long npx = (unsigned long long)e->g.W * e->g.H;
    unsigned long long total = npx * n_frames;
    if (npx % 4 == 0 && (((uintptr_t)d_rgb | (uintptr_t)d_planes) & 3) == 0) { // four pixels per lane, dword loads and stores
        total /= 4;
        unsigned blocks = (unsigned)((total + 255) / 256 > 131072 ? 131072 : (total + 255) / 256);
        if (e->g.C == 3)
            hipLaunchKernelGGL(k_convert4<3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)d_rgb,
                               npx / 4, n_frames, (uint32_t *)d_planes);
        else
            hipLaunchKernelGGL(k_convert4<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)d_rgb,
                               npx / 4, n_frames, (uint32_t *)d_planes);
        HIP_TRY(hipGetLastError());
        return M1V_OK;
    }
    unsigned blocks = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
    hipLaunchKernelGGL(k_convert, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_rgb, e->g.C, npx,
                       n_frames, d_planes);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

int m1v_convert_host(m1v_encoder *e, const uint8_t *rgb, int n_frames, uint8_t *planes) {
    if (!e || !rgb || !planes || n_frames < 0) return fail(M1V_E_ARG, "bad argument%s");
    if (const int rc = packed_only(e)) return rc;
    if (n_frames == 0) return M1V_OK;
    HIP_TRY(hipSetDevice(e->device));
    size_t in_bytes = (size_t)e->g.frame_bytes * n_frames;
    size_t out_bytes = (size_t)e->g.W * e->g.H * 3 * n_frames;
    m1v_encoder::HostPath &hp = e->hp;
    HIP_TRY(ensure_device(&hp.d_in, &hp.in_cap, in_bytes));
    HIP_TRY(ensure_device(&hp.d_planes, &hp.planes_cap, out_bytes));
    HIP_TRY(hipMemcpy(hp.d_in, rgb, in_bytes, hipMemcpyHostToDevice));
    int rc = m1v_convert_device(e, hp.d_in, n_frames, hp.d_planes, nullptr);
    if (rc != M1V_OK) return rc;
    HIP_TRY(hipMemcpy(planes, hp.d_planes, out_bytes, hipMemcpyDeviceToHost));
    return M1V_OK;
}

int m1v_subsample_device(m1v_encoder *e, const uint8_t *d_cb, const uint8_t *d_cr, uint8_t *d_cb_sub,
                         uint8_t *d_cr_sub, void *stream) {
    if (!e || !d_cb || !d_cr || !d_cb_sub || !d_cr_sub) return fail(M1V_E_ARG, "bad argument%s");
    if ((e->g.W | e->g.H) & 1) return fail(M1V_E_ARG, "odd dimensions: the reference reads out of bounds%s");
    HIP_TRY(hipSetDevice(e->device));
    int n = (e->g.W / 2) * (e->g.H / 2);
    hipLaunchKernelGGL(k_subsample, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_cb, d_cr,
                       e->g.W, e->g.H, d_cb_sub, d_cr_sub);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

int m1v_synth_device(uint8_t *d_rgb, size_t bytes_per_frame, int n_frames, uint64_t seed,
                     uint64_t first_frame_index, void *stream) {
    if (!d_rgb || n_frames < 0) return fail(M1V_E_ARG, "bad argument%s");
    if (n_frames == 0 || bytes_per_frame == 0) return M1V_OK;
    unsigned long long total = ((bytes_per_frame + 7) / 8) * (unsigned long long)n_frames;
    unsigned blocks = (unsigned)((total + 255) / 256 > 262144 ? 262144 : (total + 255) / 256);
    hipLaunchKernelGGL(k_synth, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_rgb,
                       (unsigned long long)bytes_per_frame, n_frames, (unsigned long long)seed,
                       (unsigned long long)first_frame_index);
    HIP_TRY(hipGetLastError());
    return M1V_OK;
}

} // extern "C"

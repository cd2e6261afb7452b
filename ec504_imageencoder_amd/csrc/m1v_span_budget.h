// A byte budget or a distortion ceiling per stream of a batch of many streams (m1v_encode_streams_budget_device,
// m1v_streams_budget_pick_device).  Included by m1v_kernels.hip behind m1v_streams.h.  The definition is stated in
// include/mpeg1_hip.h ("Streams: a budget per stream") and modelled in tests/streams_budget_model.py: the picks of span s are what
// the single-batch rule gives on the span's columns of the table alone, with the span's own limit.  Two kernels between the table
// and the encode (k_rd_chains, unchanged, between them under the two rules that pick by distortion), integer arithmetic only, no
// scratch:
//   k_span_plan    ONE workgroup: the exclusive prefix of max(1, ceil(n_s / 32)) over the clamped spans, chunk_at[n_streams + 1],
//                  and every frame's default (candidate 0), which a frame that no clamped span covers keeps
//   k_span_budget  workgroup w serves one chunk of 32 frames (256 step slots) of one span, which it finds by a search in
//                  chunk_at; the host launches n_streams + ceil(n_frames / 32) workgroups, which is at least chunk_at[n_streams]
//                  for spans that tile the batch (a span adds at most 1 + n_s / 32).  A workgroup stages only its own span
//                  through LDS, so the compares cost sum n_s^2, not n^2.
// Every index derived from a span is clamped into [0, n_frames] before it addresses anything (streams_span, m1v_streams.h).  With
// spans that overlap, chunk_at[n_streams] may pass the grid: the chunks behind it are not served and their frames keep the default.

// The wave's primitives on the builtins, own copies as in m1v_rd_rate.h and m1v_streams.h: a further caller of the helpers the
// older kernels use may change what those kernels compile to (tools/device_code_diff.py).
__device__ __forceinline__ unsigned long long sb_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t sb_from_lane_u32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }
__device__ __forceinline__ unsigned long long sb_from_lane_u64(unsigned long long v, int src) {
    return ((unsigned long long)sb_from_lane_u32((uint32_t)(v >> 32), src) << 32) | sb_from_lane_u32((uint32_t)v, src);
}
// The sum of v over the lanes whose numbers differ from this lane's only in the bits FROM .. TO (powers of two); every lane of
// such a group receives it.  Every lane of the wave must be active.
template <int FROM, int TO>
__device__ __forceinline__ unsigned long long sb_sum_u64(unsigned long long v, int lane) {
#pragma unroll
    for (int m = FROM; m <= TO; m <<= 1) v += sb_from_lane_u64(v, lane ^ m);
    return v;
}

constexpr int kSpanThreads = 256;
constexpr int kSpanFrames = kSpanThreads / kMaxCandidates; // frames of a chunk: one step slot per lane

__device__ __forceinline__ int span_chunks(const StreamsSpan &sp) {
    const int c = (sp.hi - sp.lo + kSpanFrames - 1) / kSpanFrames;
    return c > 0 ? c : 1; // (an empty span keeps one workgroup, which writes its status)
}

struct SpanPlanArgs {
    const m1v_stream_span *spans;
    int n_streams, n_frames;
    int32_t *chunk_at;      // out: [n_streams + 1] the first workgroup of every span, and their number
    uint8_t *picks, *chosen; // out (each may be null): [frame] candidate 0 | its quality
    uint8_t first_quality;
};

__global__ __launch_bounds__(kSpanThreads) void k_span_plan(SpanPlanArgs a) {
    __shared__ int wave_total[kSpanThreads / kWave];
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    for (int f = t; f < a.n_frames; f += kSpanThreads) {
        if (a.picks) a.picks[f] = 0;
        if (a.chosen) a.chosen[f] = a.first_quality;
    }
    // lane t holds `per` consecutive spans; their chunks, scanned over the wave, then over the workgroup's waves
    const int per = (a.n_streams + kSpanThreads - 1) / kSpanThreads;
    const int s0 = min(t * per, a.n_streams), s1 = min(s0 + per, a.n_streams);
    int mine = 0;
    for (int s = s0; s < s1; s++) mine += span_chunks(streams_span(a.spans, s, a.n_streams, a.n_frames));
    int incl = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = (int)sb_from_lane_u32((uint32_t)incl, max(lane - d, 0));
        incl += lane >= d ? up : 0;
    }
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    int at = incl - mine;
    for (int w = 0; w < wave; w++) at += wave_total[w];
    for (int s = s0; s < s1; s++) {
        a.chunk_at[s] = at;
        at += span_chunks(streams_span(a.spans, s, a.n_streams, a.n_frames));
    }
    if (t == kSpanThreads - 1) a.chunk_at[a.n_streams] = at; // (the last lane's spans, if it has any, are the last ones)
}

struct SpanBudgetArgs {
    const unsigned long long *sizes, *dist; // [k * stride + frame]; dist may be null under M1V_SPANS_LARGEST_THAT_FITS
    int stride, n_cand, n_frames;
    unsigned long long cand;                // byte k: the quality of candidate k
    const uint32_t *table_status;           // [n_cand] or null
    const RdStep *steps;                    // [frame][kMaxCandidates], k_rd_chains' (the two rules that pick by distortion)
    const m1v_stream_span *spans;
    int n_streams;
    const int32_t *chunk_at;                // k_span_plan's
    const unsigned long long *limits;       // [n_streams], or null: `limit` for every stream
    unsigned long long limit;
    uint8_t *picks, *chosen;                // out (each may be null): [frame] the candidate index | its quality
    unsigned long long *pick_dist;          // out (may be null): [frame] the pick's distortion
    uint32_t *stream_status;                // out (may be null): [n_streams] the stream's over bit, or 0
    uint32_t *status;                       // out: [1], cleared in front of the launch, OR'ed
    uint32_t *batch_status;                 // an encode's status word, which M1V_STATUS_OVER_DISTORTION is OR'ed into, or null
};

// M1V_SPANS_LARGEST_THAT_FITS is k_rate_pick<false>'s rule on the span: lane 8 j + k sums candidate k over every 32nd frame of the
// span (T[k], and what the frames that shrink from k to k + 1 save), `top` follows, and then the items are the chunk's 32 frames:
// the eight lanes of a frame share the span's keys (d << 32 | position in the span), staged 256 at a time, and add up the
// positive d whose keys come at or before the frame's own.
// The other two rules are k_rd_batch_pick's on the span: lane g of the chunk holds slot g & 7 of frame g >> 3 of the chunk, every
// workgroup stages the span's slots, 256 at a time, and every lane that holds a step adds up the cost of the span's steps
// before its own (dd / ds descending by exact cross products in 128 bits, then position in the span, then j).
template <int RULE>
__global__ __launch_bounds__(kSpanThreads) void k_span_budget(SpanBudgetArgs a) {
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    const int w = (int)blockIdx.x;
    if (w >= a.chunk_at[a.n_streams]) return;
    int s = 0, s_end = a.n_streams; // chunk_at[s] <= w < chunk_at[s_end]; chunk_at increases strictly
    while (s_end - s > 1) {
        const int mid = (s + s_end) >> 1;
        if (a.chunk_at[mid] <= w)
            s = mid;
        else
            s_end = mid;
    }
    const int chunk = w - a.chunk_at[s];
    const StreamsSpan sp = streams_span(a.spans, s, a.n_streams, a.n_frames);
    const int cnt = sp.hi - sp.lo;
    const unsigned long long limit = a.limits ? a.limits[s] : a.limit;
    bool over;
    if constexpr (RULE == M1V_SPANS_LARGEST_THAT_FITS) {
        __shared__ unsigned long long part[kSpanThreads / kWave][2 * kMaxCandidates]; // per wave: T[k], then the savings of k -> k + 1
        __shared__ unsigned long long tot[2 * kMaxCandidates];
        __shared__ unsigned long long keys[kSpanThreads];
        const int k = t & 7, K = a.n_cand;
        unsigned long long sum = 0, save = 0;
        if (k < K)
            for (int j = t >> 3; j < cnt; j += kSpanFrames) {
                const unsigned long long sz = a.sizes[(size_t)k * a.stride + sp.lo + j];
                sum += sz;
                if (k + 1 < K) {
                    const unsigned long long up = a.sizes[(size_t)(k + 1) * a.stride + sp.lo + j];
                    save += up < sz ? sz - up : 0ull;
                }
            }
        sum = sb_sum_u64<8, 32>(sum, lane);
        save = sb_sum_u64<8, 32>(save, lane);
        if (lane < kMaxCandidates) {
            part[wave][lane] = sum;
            part[wave][kMaxCandidates + lane] = save;
        }
        __syncthreads();
        if (t < 2 * kMaxCandidates) {
            unsigned long long v = 0;
            for (int i = 0; i < kSpanThreads / kWave; i++) v += part[i][t];
            tot[t] = v;
        }
        __syncthreads();
        int top = -1;
        for (int q = 0; q < K; q++)
            if (tot[q] <= limit) top = q;
        over = top < 0;
        const int j_own = chunk * kSpanFrames + (t >> 3);
        const bool have = j_own < cnt;
        int pick = top < 0 ? 0 : top;
        if (top >= 0 && top < K - 1) { // (the same for every lane of the workgroup)
            const unsigned long long room = limit - tot[top] + tot[kMaxCandidates + top];
            const unsigned long long *lo = a.sizes + (size_t)top * a.stride + sp.lo, *hi = lo + a.stride;
            const long long d = have ? (long long)(hi[j_own] - lo[j_own]) : 0;
            const unsigned long long own = ((unsigned long long)(d > 0xffffffffll ? 0xffffffffll : (d > 0 ? d : 0)) << 32) | (uint32_t)j_own;
            unsigned long long acc = 0; // the positive d whose keys are <= own
            for (int c0 = 0; c0 < cnt; c0 += kSpanThreads) {
                __syncthreads(); // (the previous block's keys are read)
                unsigned long long key = 0; // (behind the span's end: adds nothing)
                if (c0 + t < cnt) {
                    const long long dj = (long long)(hi[c0 + t] - lo[c0 + t]);
                    key = ((unsigned long long)(dj > 0xffffffffll ? 0xffffffffll : (dj > 0 ? dj : 0)) << 32) | (uint32_t)(c0 + t);
                }
                keys[t] = key;
                __syncthreads();
                if (have && d > 0) {
                    const int staged = (min(kSpanThreads, cnt - c0) + 7) & ~7; // (the keys behind the span's end are 0)
#pragma unroll 8
                    for (int i = k; i < staged; i += 8) {
                        const unsigned long long kj = keys[i];
                        acc += kj <= own ? (kj >> 32) : 0ull;
                    }
                }
            }
            acc = sb_sum_u64<1, 4>(acc, lane);
            pick = d <= 0 || acc <= room ? top + 1 : top;
        }
        if (have && k == 0) {
            const int f = sp.lo + j_own;
            if (a.picks) a.picks[f] = (uint8_t)pick;
            if (a.chosen) a.chosen[f] = cand_quality(a.cand, pick);
            if (a.pick_dist && a.dist) a.pick_dist[f] = a.dist[(size_t)pick * a.stride + f];
        }
    } else {
        __shared__ RdStep blk[kSpanThreads];
        __shared__ unsigned long long part[kSpanThreads / kWave][5];
        constexpr bool by_bytes = RULE == M1V_SPANS_LEAST_DISTORTION;
        const RdStep *steps = a.steps + (size_t)sp.lo * kMaxCandidates;
        const int g = chunk * kSpanThreads + t, total = cnt * kMaxCandidates; // slots of the span
        const RdStep own = g < total ? steps[g] : RdStep{0u, 0u, 0ull};
        const bool is_step = g < total && (g & 7) != 0 && own.ds != 0u;
        // sums[0] = the v0 records; the v0 distortions and all steps' gains in 32-bit halves (a sum of them may pass 2^64)
        unsigned long long sums[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
        u128 acc = 0;
        for (int c0 = 0; c0 < total; c0 += kSpanThreads) {
            __syncthreads(); // (the previous block is read)
            RdStep e = c0 + t < total ? steps[c0 + t] : RdStep{0u, 0u, 0ull};
            if ((t & 7) == 0) {
                sums[0] += e.ds;
                sums[1] += e.dd & 0xffffffffull;
                sums[2] += e.dd >> 32;
                e.ds = 0u; // (no step: it adds nothing below)
                e.dd = 0ull;
            } else {
                sums[3] += e.dd & 0xffffffffull;
                sums[4] += e.dd >> 32;
            }
            blk[t] = e;
            __syncthreads();
            if (is_step) {
                const int staged = (min(kSpanThreads, total - c0) + 7) & ~7; // (the slots behind the span's end hold no step)
                for (int i = 0; i < staged; i += 8) {
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const RdStep b = blk[i + u];
                        const u128 l = (u128)b.dd * (u128)own.ds, r = (u128)own.dd * (u128)b.ds;
                        const bool before = l > r || (l == r && c0 + i + u < g);
                        acc += before ? (u128)(by_bytes ? (unsigned long long)b.ds : b.dd) : (u128)0;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const unsigned long long v = sb_sum_u64<1, 32>(sums[i], lane);
            if (lane == 0) part[wave][i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 5; i++) {
            sums[i] = 0;
            for (int v = 0; v < kSpanThreads / kWave; v++) sums[i] += part[v][i];
        }
        const u128 start_d = ((u128)sums[2] << 32) + sums[1], gain = ((u128)sums[4] << 32) + sums[3], lim = limit;
        bool taken;
        if (by_bytes) {
            over = sums[0] > limit;
            taken = !over && is_step && (u128)sums[0] + acc + own.ds <= lim;
        } else {
            over = start_d - gain > lim;
            taken = is_step && start_d > lim && acc < start_d - lim;
        }
        const uint32_t mine = (uint32_t)(sb_ballot(taken) >> (lane & ~7)) & 0xffu;
        if (g < total && (lane & 7) == __popc(mine)) {
            const int f = sp.lo + (g >> 3), k = (int)own.k;
            if (a.picks) a.picks[f] = (uint8_t)k;
            if (a.chosen) a.chosen[f] = cand_quality(a.cand, k);
            if (a.pick_dist) a.pick_dist[f] = a.dist[(size_t)k * a.stride + f];
        }
    }
    if (chunk == 0 && t == 0) {
        constexpr uint32_t over_bit = RULE == M1V_SPANS_SMALLEST_AT_DISTORTION ? (uint32_t)M1V_STATUS_OVER_DISTORTION : (uint32_t)M1V_STATUS_OVER_BUDGET;
        uint32_t bits = over ? over_bit : 0u;
        if (a.stream_status) a.stream_status[s] = bits;
        if (!sp.ok) bits |= (uint32_t)M1V_STATUS_STREAMS;
        if (w == 0 && a.n_frames > 0 && a.table_status)
            for (int k = 0; k < a.n_cand; k++) bits |= a.table_status[k] & (uint32_t)M1V_STATUS_SCRATCH;
        if (bits) atomicOr(a.status, bits);
        if (a.batch_status && over && RULE == M1V_SPANS_SMALLEST_AT_DISTORTION) atomicOr(a.batch_status, over_bit);
    }
}

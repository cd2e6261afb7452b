// Batches of many streams (m1v_encode_streams_device, m1v_encode_streams_cbr_device, m1v_streams_cbr_pick_device).  Included by
// m1v_kernels.hip behind m1v_rd_rate.h.  The definition is stated in include/mpeg1_hip.h ("Streams") and modelled in
// tests/streams_model.py.  A batch is the concatenation of n_streams spans (m1v_stream_span, an array on the DEVICE that only
// kernels read); three kernels around the encode, integer arithmetic only, no scratch:
//   k_streams_map      one lane per span, in front of the encode kernel: checks that the spans tile the batch and expands them into
//                      the counter set's frame_index[max_frames]
//   k_streams_bitrate  one wave per stream, a grid of workgroups: the bitrate walk of k_rate_pick<true> / k_rd_cbr_pick over the
//                      span's columns of the table, one leaky bucket per stream
//   k_streams_finish   behind k_assemble (which ran with first_index 0 and is not edited): rewrites the 44 header bytes of every
//                      record that fitted from tab->hdr[frame_index[f] & 255] and sums each span's records
// Every index derived from a span is clamped into [0, n_frames] before it addresses anything.

// The wave's primitives on the builtins, own copies as in m1v_rd_rate.h: a further caller of the helpers the older kernels use
// may change what those kernels compile to (tools/device_code_diff.py).
__device__ __forceinline__ unsigned long long st_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ long long st_readlane_i64(long long v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// v of lane `src` (any lane of the wave, per lane)
__device__ __forceinline__ uint32_t st_from_lane_u32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }
__device__ __forceinline__ unsigned long long st_from_lane_u64(unsigned long long v, int src) {
    return ((unsigned long long)st_from_lane_u32((uint32_t)(v >> 32), src) << 32) | st_from_lane_u32((uint32_t)v, src);
}
// v to lane `dst` (the dst of a wave's lanes are a permutation)
__device__ __forceinline__ uint32_t st_to_lane_u32(uint32_t v, int dst) { return (uint32_t)__builtin_amdgcn_ds_permute(dst << 2, (int)v); }
__device__ __forceinline__ unsigned long long st_to_lane_u64(unsigned long long v, int dst) {
    return ((unsigned long long)st_to_lane_u32((uint32_t)(v >> 32), dst) << 32) | st_to_lane_u32((uint32_t)v, dst);
}
__device__ __forceinline__ unsigned long long st_wave_scan_u64(unsigned long long v, int lane) { // inclusive
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long up = st_from_lane_u64(v, max(lane - d, 0));
        v += lane >= d ? up : 0ull;
    }
    return v;
}

// Span s clamped into the batch: frames [lo, hi) (empty where the span lies outside), and whether it keeps the tiling rule
// against its neighbour in front: span 0 starts at 0, span s where span s - 1 ends, the last span ends at n_frames.
struct StreamsSpan {
    int lo, hi;
    int32_t first_index;
    bool ok;
};
__device__ __forceinline__ StreamsSpan streams_span(const m1v_stream_span *spans, int s, int n_streams, int n_frames) {
    const unsigned long long first = spans[s].first_frame, end = first + spans[s].n_frames, n = (unsigned long long)n_frames;
    const unsigned long long want = s == 0 ? 0ull : (unsigned long long)spans[s - 1].first_frame + spans[s - 1].n_frames;
    StreamsSpan out;
    out.lo = (int)(first < n ? first : n);
    out.hi = (int)(end < n ? end : n);
    out.first_index = spans[s].first_frame_index;
    out.ok = first == want && (s != n_streams - 1 || end == n);
    return out;
}

struct StreamsMapArgs {
    const m1v_stream_span *spans;
    int n_streams, n_frames;
    int32_t *frame_index; // out: [n_frames] the index, in its stream, of every frame a span covers
    uint32_t *status;     // the batch's status word: M1V_STATUS_STREAMS is OR'ed into it
};

__global__ __launch_bounds__(256) void k_streams_map(StreamsMapArgs a) {
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= a.n_streams) return;
    const StreamsSpan sp = streams_span(a.spans, s, a.n_streams, a.n_frames);
    if (!sp.ok) atomicOr(a.status, (uint32_t)M1V_STATUS_STREAMS);
    const uint32_t first = a.spans[s].first_frame; // (lo == first wherever the loop runs)
    for (int f = sp.lo; f < sp.hi; f++) a.frame_index[f] = (int32_t)((uint32_t)sp.first_index + ((uint32_t)f - first));
}

struct StreamsRateArgs {
    const unsigned long long *sizes, *dist; // [k * stride + frame]; dist may be null under the byte rule
    int stride, n_cand, n_frames;
    unsigned long long cand;                // byte k: the quality of candidate k
    const uint32_t *table_status;           // [n_cand] or null
    const m1v_stream_span *spans;
    int n_streams;
    const m1v_stream_rate *rates;           // [n_streams], or null: rate and capacity for every stream
    long long rate, capacity;
    const long long *level_in;              // [n_streams]
    long long *level_out;                   // [n_streams] (may be level_in: a wave reads its element before it writes it)
    uint8_t *picks, *chosen;                // out (each may be null): [frame] the candidate index | its quality
    unsigned long long *pick_dist;          // out (may be null): [frame] the pick's distortion
    uint32_t *status;                       // out: [1], cleared in front of the launch, OR'ed
    uint32_t *batch_status;                 // an encode's status word, which M1V_STATUS_STREAMS is OR'ed into, or null
};

constexpr int kStreamsWaves = 4; // streams per workgroup
constexpr long long kStreamsNever = 0x7fffffffffffffffll; // a record no level reaches

// Wave w of the grid walks stream w.  Lane 8j + k holds candidate k of frame j of a step of eight, loaded from the span's columns
// of the table one step ahead of the walk.  Byte rule: position = candidate, the LAST set bit of the frame's eight fits wins,
// else candidate 0.  Distortion rule: the eight lanes of a frame sort their candidates by (in the running, D, s, k) among
// themselves — each lane counts the seven others that come before it and sends its record to that position — so that the FIRST
// set bit wins, else the position of the smallest record.  The chain from frame to frame is a compare, a ballot, a readlane and
// the level update, all on the scalar side.
template <int RULE>
__global__ __launch_bounds__(kStreamsWaves * kWave) void k_streams_bitrate(StreamsRateArgs a) {
    __shared__ uint32_t group_bits;
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int s = (int)blockIdx.x * kStreamsWaves + wave;
    constexpr bool by_dist = RULE == M1V_STREAMS_LEAST_DISTORTION;
    if (t == 0) group_bits = 0u;
    __syncthreads();
    uint32_t bits = 0;
    if (blockIdx.x == 0 && wave == 0 && a.n_frames > 0 && a.table_status)
        for (int k = 0; k < a.n_cand; k++) bits |= a.table_status[k] & (uint32_t)M1V_STATUS_SCRATCH;
    if (s < a.n_streams) {
        const StreamsSpan sp = streams_span(a.spans, s, a.n_streams, a.n_frames);
        if (!sp.ok) bits |= (uint32_t)M1V_STATUS_STREAMS;
        unsigned long long r = (unsigned long long)a.rate, c = (unsigned long long)a.capacity;
        if (a.rates) {
            r = a.rates[s].bytes_per_frame;
            c = a.rates[s].buffer_bytes;
        }
        const bool rated = r >= 1ull && r <= c && c < (1ull << 62);
        const long long rate = (long long)r, cap = (long long)c;
        long long level = a.level_in[s];
        const int k = lane & 7, g = lane >> 3, cnt = sp.hi - sp.lo;
        if (!rated) { // the stream's frames at candidate 0, its level as it came
            bits |= (uint32_t)M1V_STATUS_STREAMS;
            for (int f = sp.lo + lane; f < sp.hi; f += kWave) {
                if (a.picks) a.picks[f] = 0;
                if (a.chosen) a.chosen[f] = cand_quality(a.cand, 0);
                if (a.pick_dist && a.dist) a.pick_dist[f] = a.dist[f];
            }
        } else {
            level = level < cap ? level : cap;
            uint32_t mask = 0; // the candidates in the running (the byte rule: all of them)
            for (int q = 0; q < a.n_cand; q++)
                if (!by_dist || !a.table_status || !(a.table_status[q] & (uint32_t)M1V_STATUS_UNENCODABLE)) mask |= 1u << q;
            mask = mask ? mask : 1u;
            const bool in = (mask >> k) & 1u;
            auto load = [&](int j0, long long &sz, unsigned long long &ds) {
                const int f = sp.lo + j0 + g;
                const bool there = in && j0 + g < cnt;
                sz = there ? (long long)a.sizes[(size_t)k * a.stride + f] : kStreamsNever;
                ds = by_dist && there ? a.dist[(size_t)k * a.stride + f] : ~0ull;
            };
            long long sz, sz_next = kStreamsNever;
            unsigned long long ds, ds_next = ~0ull;
            bool over = false;
            if (cnt > 0) load(0, sz, ds);
            for (int j0 = 0; j0 < cnt; j0 += 8) {
                if (j0 + 8 < cnt) load(j0 + 8, sz_next, ds_next);
                long long ps = sz;     // the record at this lane's position
                uint32_t pk = (uint32_t)k; // and its candidate
                uint32_t small = 0;    // distortion rule: byte j = the position of frame j's smallest record
                if (by_dist) {
                    int before_d = 0, before_s = 0; // the frame's candidates in front of this one by (in, D, s, k) | by (in, s, k)
#pragma unroll
                    for (int o = 0; o < 8; o++) {
                        const int src = (lane & ~7) + o;
                        const long long so = (long long)st_from_lane_u64((unsigned long long)sz, src);
                        const unsigned long long d_o = st_from_lane_u64(ds, src);
                        const bool o_in = (mask >> o) & 1u;
                        const bool by_s = so != sz ? so < sz : o < k;
                        const bool first_d = o_in != in ? o_in : (d_o != ds ? d_o < ds : by_s);
                        const bool first_s = o_in != in ? o_in : by_s;
                        before_d += o != k && first_d ? 1 : 0;
                        before_s += o != k && first_s ? 1 : 0;
                    }
                    const int dst = (lane & ~7) + before_d;
                    ps = (long long)st_to_lane_u64((unsigned long long)sz, dst);
                    pk = st_to_lane_u32((uint32_t)k, dst);
                    const bool least = before_s == 0;
                    const unsigned long long b0 = st_ballot(least && (before_d & 1)), b1 = st_ballot(least && (before_d & 2)),
                                             b2 = st_ballot(least && (before_d & 4));
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        small |= (uint32_t)((((b0 >> (8 * j)) & 0xffull) ? 1u : 0u) | (((b1 >> (8 * j)) & 0xffull) ? 2u : 0u) |
                                            (((b2 >> (8 * j)) & 0xffull) ? 4u : 0u))
                                 << (4 * j);
                }
                int mine = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if (j0 + j < cnt) {
                        const uint32_t fit = (uint32_t)(st_ballot(ps <= level) >> (8 * j)) & 0xffu;
                        int pos;
                        if (by_dist)
                            pos = fit ? __ffs((int)fit) - 1 : (int)((small >> (4 * j)) & 7u);
                        else
                            pos = fit ? 31 - __clz((int)fit) : 0;
                        over |= fit == 0;
                        level -= st_readlane_i64(ps, 8 * j + pos);
                        level += rate;
                        level = level < cap ? level : cap;
                        if (g == j) mine = pos;
                    }
                }
                const int pick = (int)st_from_lane_u32(pk, (lane & ~7) + mine) & 7;
                if (k == 0 && j0 + g < cnt) {
                    const int f = sp.lo + j0 + g;
                    if (a.picks) a.picks[f] = (uint8_t)pick;
                    if (a.chosen) a.chosen[f] = cand_quality(a.cand, pick);
                    if (a.pick_dist && a.dist) a.pick_dist[f] = a.dist[(size_t)pick * a.stride + f];
                }
                sz = sz_next;
                ds = ds_next;
            }
            if (over) bits |= (uint32_t)M1V_STATUS_OVER_BUDGET;
        }
        if (lane == 0) a.level_out[s] = level;
    }
    if (lane == 0 && bits) atomicOr(&group_bits, bits);
    __syncthreads();
    if (t == 0 && group_bits) {
        atomicOr(a.status, group_bits);
        if (a.batch_status && (group_bits & (uint32_t)M1V_STATUS_STREAMS)) atomicOr(a.batch_status, (uint32_t)M1V_STATUS_STREAMS);
    }
}

struct StreamsFinishArgs {
    const m1v_stream_span *spans;
    int n_streams, n_frames;
    const unsigned long long *frame_bytes; // [frame] bytes of the frame's strips, as k_assemble read them: the record is 48 more
    const int32_t *frame_index;            // k_streams_map's
    const Tables *tab;
    uint8_t *out;
    unsigned long long out_cap;
    unsigned long long *stream_bytes;      // out (may be null): [n_streams] bytes of each span's records
    int header_blocks;                     // workgroups that rewrite headers, 256 frames each; the rest sum spans
};

constexpr int kStreamsFinishThreads = 256;

// Workgroup b < header_blocks: where frames [256 b, 256 b + 256) start (the sum of the records in front of them, then a scan),
// and for those that fitted, as k_assemble decided it (offset + size <= out_cap), bytes 0..43 of the record from the header of
// the frame's own index, but for bytes 4 and 5 (the packet length, which k_assemble wrote).  The other workgroups: one wave per
// span, the sum of its records.
__global__ __launch_bounds__(kStreamsFinishThreads) void k_streams_finish(StreamsFinishArgs a) {
    __shared__ unsigned long long part[2][kStreamsFinishThreads / kWave];
    __shared__ unsigned long long at[kStreamsFinishThreads];
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    if ((int)blockIdx.x >= a.header_blocks) {
        const int s = ((int)blockIdx.x - a.header_blocks) * (kStreamsFinishThreads / kWave) + wave;
        if (s >= a.n_streams || !a.stream_bytes) return;
        const StreamsSpan sp = streams_span(a.spans, s, a.n_streams, a.n_frames);
        unsigned long long sum = 0;
        for (int f = sp.lo + lane; f < sp.hi; f += kWave) sum += 48ull + a.frame_bytes[f];
        sum = st_wave_scan_u64(sum, lane);
        if (lane == kWave - 1) a.stream_bytes[s] = sum;
        return;
    }
    const int f0 = (int)blockIdx.x * kStreamsFinishThreads, cnt = min(kStreamsFinishThreads, a.n_frames - f0);
    unsigned long long front = 0;
    for (int f = t; f < f0; f += kStreamsFinishThreads) front += 48ull + a.frame_bytes[f];
    const unsigned long long size = t < cnt ? 48ull + a.frame_bytes[f0 + t] : 0ull;
    front = st_wave_scan_u64(front, lane);
    const unsigned long long incl = st_wave_scan_u64(size, lane);
    if (lane == kWave - 1) {
        part[0][wave] = front;
        part[1][wave] = incl;
    }
    __syncthreads();
    unsigned long long start = incl - size;
    for (int w = 0; w < kStreamsFinishThreads / kWave; w++) start += part[0][w] + (w < wave ? part[1][w] : 0ull);
    at[t] = t < cnt && start + size <= a.out_cap ? start : ~0ull;
    __syncthreads();
    for (int i = t; i < cnt * 44; i += kStreamsFinishThreads) {
        const int j = i / 44, b = i - 44 * j;
        const unsigned long long fo = at[j];
        if (fo != ~0ull && b != 4 && b != 5) a.out[fo + b] = a.tab->hdr[a.frame_index[f0 + j] & 255][b];
    }
}

// Batch budgets and constant bitrate that pick by distortion (m1v_encode_rd_batch_device, m1v_encode_rd_cbr_device and the pick-only
// calls m1v_rd_batch_pick_device, m1v_rd_cbr_pick_device).  Included by m1v_kernels.hip behind k_rate_pick.
// The rules are stated in include/mpeg1_hip.h and modelled in tests/rd_rate_model.py.  Three kernels between the rd table
// (sizes / dist[k * stride + frame]) and the encode, all on the caller's stream, integer arithmetic only, no scratch:
//   k_rd_chains      one lane per frame: the frame's chain (lower convex hull) into the step table, steps[frame][8]
//   k_rd_batch_pick  one lane per step slot, a grid of workgroups: each step's place in the order of all steps by counting
//   k_rd_cbr_pick    ONE workgroup: k_rate_pick<true>'s walk over candidates sorted by (D, s, k) per frame
// A candidate whose table status carries M1V_STATUS_UNENCODABLE is out of the running; with every candidate out, candidate 0
// alone is in it.
typedef unsigned __int128 u128;

// Slot 0 of a frame: v0 (ds = its record, dd = its distortion).  Slot j >= 1: step j of the chain (ds > 0 bytes more, dd > 0
// distortion less, k = the vertex it reaches), or ds = dd = k = 0 behind the chain's end.
struct RdStep {
    uint32_t ds, k;
    unsigned long long dd;
};
static_assert(sizeof(RdStep) == 16, "one 128-bit load per step");

// The wave's ballot and 64-bit readlane, as k_rate_pick uses them.  Own copies on the builtins: with a second caller of HIP's
// __ballot or of readlane_i64 in this translation unit, the optimiser annotates their arguments otherwise and k_rate_pick<true>
// compiles to other instructions than before (tools/device_code_diff.py).
__device__ __forceinline__ unsigned long long rd_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ long long rd_readlane_i64(long long v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ uint32_t rd_running(const uint32_t *table_status, int n_cand) {
    uint32_t mask = 0;
    for (int k = 0; k < n_cand; k++)
        if (!table_status || !(table_status[k] & (uint32_t)M1V_STATUS_UNENCODABLE)) mask |= 1u << k;
    return mask ? mask : 1u;
}

struct RdChainArgs {
    const unsigned long long *sizes, *dist; // [k * stride + frame]
    int stride, n_cand, n_frames;
    const uint32_t *table_status;           // [n_cand], or null: every candidate is in the running
    RdStep *steps;                          // out: [frame][kMaxCandidates]
};

// v0 = the least record (ties: the less D, then the smaller k).  From vertex (cs, cd) the next vertex is, among the candidates
// with more bytes and less distortion, the one of the greatest (cd - D) / (s - cs), compared by cross products in 128 bits
// (ties: the smaller s, then the smaller k).  The K points stay in registers: every index below is a constant once unrolled.
__global__ __launch_bounds__(256) void k_rd_chains(RdChainArgs a) {
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    if (f >= a.n_frames) return;
    const uint32_t mask = rd_running(a.table_status, a.n_cand);
    unsigned long long s[kMaxCandidates], d[kMaxCandidates];
#pragma unroll
    for (int k = 0; k < kMaxCandidates; k++) {
        const bool in = (mask >> k) & 1u; // (mask holds no bit at or above n_cand)
        s[k] = in ? a.sizes[(size_t)k * a.stride + f] : 0ull;
        d[k] = in ? a.dist[(size_t)k * a.stride + f] : 0ull;
    }
    int v = -1;
    unsigned long long cs = 0, cd = 0;
#pragma unroll
    for (int k = 0; k < kMaxCandidates; k++)
        if (((mask >> k) & 1u) && (v < 0 || s[k] < cs || (s[k] == cs && d[k] < cd))) {
            v = k;
            cs = s[k];
            cd = d[k];
        }
    RdStep *out = a.steps + (size_t)f * kMaxCandidates;
    out[0] = RdStep{(uint32_t)cs, (uint32_t)v, cd};
    bool open = true;
#pragma unroll 1
    for (int j = 1; j < kMaxCandidates; j++) {
        int b = -1;
        unsigned long long bs = 0, bd = 0;
        if (open) {
#pragma unroll
            for (int k = 0; k < kMaxCandidates; k++)
                if (((mask >> k) & 1u) && s[k] > cs && d[k] < cd) {
                    bool take = b < 0;
                    if (!take) {
                        const u128 l = (u128)(cd - d[k]) * (u128)(bs - cs), r = (u128)(cd - bd) * (u128)(s[k] - cs);
                        take = l > r || (l == r && s[k] < bs);
                    }
                    if (take) {
                        b = k;
                        bs = s[k];
                        bd = d[k];
                    }
                }
        }
        if (b < 0) {
            open = false;
            out[j] = RdStep{0u, 0u, 0ull};
        } else {
            out[j] = RdStep{(uint32_t)(bs - cs), (uint32_t)b, cd - bd};
            cs = bs;
            cd = bd;
        }
    }
}

constexpr int kRdPickThreads = 256;

struct RdBatchArgs {
    const RdStep *steps;             // [frame][kMaxCandidates], k_rd_chains'
    const unsigned long long *dist;  // [k * stride + frame]
    int stride, n_frames, n_cand, rule;
    unsigned long long limit;        // bytes for the sum of the records | ceiling for the sum of the distortions
    unsigned long long cand;         // byte k: the quality of candidate k
    const uint32_t *table_status;    // [n_cand] or null
    uint8_t *picks;                  // out (may be null): [frame] the candidate index picked
    uint8_t *chosen;                 // out (may be null): [frame] its quality
    unsigned long long *pick_dist;   // out (may be null): [frame] its distortion
    uint32_t *status;                // out: [1], written
    uint32_t *batch_status;          // an encode's status word, which M1V_STATUS_OVER_DISTORTION is OR'ed into, or null
};

// Lane g of the grid holds slot g & 7 of frame g >> 3.  Step a comes before step b in the order of all steps iff
// dd_a * ds_b > dd_b * ds_a (exact, in 128 bits), or they are equal and a's slot number is the smaller (frame, then j).  Every
// workgroup stages all slots through LDS, 256 at a time, and every lane that holds a step adds up the cost (ds | dd) of the
// steps before its own: n * 8 cross products per lane, spread over n * 8 / 256 workgroups.  Along the way each workgroup sums
// the v0 slots (the start) and all steps (the chains' ends).  Byte rule: a step is taken iff start + the costs up to and
// including its own <= limit.  Distortion rule: iff the start less the gains before it is still above the limit.  The taken
// steps of a frame are its first ones (dd / ds never increases along a chain), so their count, from a ballot over the frame's
// eight lanes, is the slot whose vertex the frame ends at; that lane writes the frame's outputs.
__global__ __launch_bounds__(kRdPickThreads) void k_rd_batch_pick(RdBatchArgs a) {
    __shared__ RdStep blk[kRdPickThreads];
    __shared__ unsigned long long part[kRdPickThreads / kWave][5];
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    const int g = (int)(blockIdx.x * kRdPickThreads) + t, total = a.n_frames * kMaxCandidates;
    const bool by_bytes = a.rule == M1V_RD_BEST_IN_BUDGET;
    const RdStep own = g < total ? a.steps[g] : RdStep{0u, 0u, 0ull};
    const bool is_step = g < total && (g & 7) != 0 && own.ds != 0u;
    // sums[0] = the v0 records; the v0 distortions and all steps' gains in 32-bit halves (a sum of them may pass 2^64)
    unsigned long long sums[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    u128 acc = 0;
    for (int c0 = 0; c0 < total; c0 += kRdPickThreads) {
        __syncthreads(); // (the previous block is read)
        RdStep e = c0 + t < total ? a.steps[c0 + t] : RdStep{0u, 0u, 0ull};
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
            for (int i = 0; i < kRdPickThreads; i += 8) {
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
        const unsigned long long w = wave_sum_u64(sums[i]);
        if (lane == 0) part[wave][i] = w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; i++) {
        sums[i] = 0;
        for (int w = 0; w < kRdPickThreads / kWave; w++) sums[i] += part[w][i];
    }
    const u128 start_d = ((u128)sums[2] << 32) + sums[1], gain = ((u128)sums[4] << 32) + sums[3], lim = a.limit;
    bool over, taken;
    if (by_bytes) {
        over = sums[0] > a.limit;
        taken = !over && is_step && (u128)sums[0] + acc + own.ds <= lim;
    } else {
        over = start_d - gain > lim;
        taken = is_step && start_d > lim && acc < start_d - lim;
    }
    const uint32_t mine = (uint32_t)(rd_ballot(taken) >> (lane & ~7)) & 0xffu;
    if (g < total && (lane & 7) == __popc(mine)) {
        const int f = g >> 3, k = (int)own.k;
        if (a.picks) a.picks[f] = (uint8_t)k;
        if (a.chosen) a.chosen[f] = cand_quality(a.cand, k);
        if (a.pick_dist) a.pick_dist[f] = a.dist[(size_t)k * a.stride + f];
    }
    if (g == 0) {
        uint32_t bits = 0;
        if (a.table_status)
            for (int k = 0; k < a.n_cand; k++) bits |= a.table_status[k] & (uint32_t)M1V_STATUS_SCRATCH;
        if (over) bits |= by_bytes ? (uint32_t)M1V_STATUS_OVER_BUDGET : (uint32_t)M1V_STATUS_OVER_DISTORTION;
        *a.status = bits;
        if (a.batch_status && over && !by_bytes) atomicOr(a.batch_status, (uint32_t)M1V_STATUS_OVER_DISTORTION);
    }
}

struct RdCbrArgs {
    const unsigned long long *sizes, *dist; // [k * stride + frame]
    int stride, n_cand, n_frames;
    unsigned long long cand;         // byte k: the quality of candidate k
    const uint32_t *table_status;    // [n_cand] or null
    long long rate, capacity;        // as PickArgs'
    const long long *level_in;
    long long *level_out;
    uint8_t *picks, *chosen;         // out (each may be null): [frame] the candidate index | its quality
    unsigned long long *pick_dist;   // out (may be null): [frame] its distortion
    uint32_t *status;                // out: [1], written
};

// The bitrate walk of k_rate_pick<true> with "the least D that fits" for "the largest k that fits".  Which candidate of a frame
// has the least D among those that fit depends on the level, but their order by (D, s, k) does not: a lane per frame sorts the
// frame's candidates by it into LDS (position r of frame j: the record, and in perm[j] nibble r the candidate) and notes the
// position of the smallest record.  Wave 0 then walks as there, with the FIRST set bit of the ballot in place of the last, or
// the smallest record's position when nothing fits.  Candidates out of the running hold a record no level reaches.
__global__ __launch_bounds__(kPickThreads) void k_rd_cbr_pick(RdCbrArgs a) {
    __shared__ long long stage[kCbrChunk * kMaxCandidates];
    __shared__ uint32_t perm[kCbrChunk];
    __shared__ uint8_t smallest[kCbrChunk], picked[kCbrChunk];
    const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    const int n = a.n_frames;
    const uint32_t mask = rd_running(a.table_status, a.n_cand);
    uint32_t bits = 0;
    if (n > 0 && a.table_status)
        for (int k = 0; k < a.n_cand; k++) bits |= a.table_status[k] & (uint32_t)M1V_STATUS_SCRATCH;
    long long level = *a.level_in; // (every read of level_in comes before the write of level_out)
    level = level < a.capacity ? level : a.capacity;
    bool over = false;
    for (int f0 = 0; f0 < n; f0 += kCbrChunk) {
        const int cnt = min(kCbrChunk, n - f0);
        for (int j = t; j < kCbrChunk; j += kPickThreads) {
            long long s[kMaxCandidates];
            unsigned long long d[kMaxCandidates];
#pragma unroll
            for (int k = 0; k < kMaxCandidates; k++) {
                const bool in = j < cnt && ((mask >> k) & 1u);
                s[k] = in ? (long long)a.sizes[(size_t)k * a.stride + f0 + j] : 0x7fffffffffffffffll;
                d[k] = in ? a.dist[(size_t)k * a.stride + f0 + j] : ~0ull;
            }
            uint32_t order = 0;
            int least = -1;
            long long least_s = 0;
#pragma unroll
            for (int k = 0; k < kMaxCandidates; k++) {
                const bool in = (mask >> k) & 1u;
                int r = 0; // the candidates that come before k by (in the running, D, s, k)
#pragma unroll
                for (int o = 0; o < kMaxCandidates; o++) {
                    const bool o_in = (mask >> o) & 1u;
                    const bool first = o_in != in ? o_in : (d[o] != d[k] ? d[o] < d[k] : (s[o] != s[k] ? s[o] < s[k] : o < k));
                    r += o != k && first ? 1 : 0;
                }
                stage[j * kMaxCandidates + r] = in ? s[k] : 0x7fffffffffffffffll;
                order |= (uint32_t)k << (4 * r);
                if (in && (least < 0 || s[k] < least_s)) {
                    least = r;
                    least_s = s[k];
                }
            }
            perm[j] = order;
            smallest[j] = (uint8_t)least;
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(wave) == 0) {
            for (int j0 = 0; j0 < cnt; j0 += 8) {
                const long long s = stage[j0 * kMaxCandidates + lane];
                const int small = (int)smallest[j0 + (lane >> 3)];
                int mine = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if (j0 + j < cnt) {
                        const uint32_t fit = (uint32_t)(rd_ballot(s <= level) >> (8 * j)) & 0xffu;
                        const int r = fit ? __ffs((int)fit) - 1 : __builtin_amdgcn_readlane(small, 8 * j);
                        over |= fit == 0;
                        level -= rd_readlane_i64(s, 8 * j + r);
                        level += a.rate;
                        level = level < a.capacity ? level : a.capacity;
                        if ((lane >> 3) == j) mine = r;
                    }
                }
                if ((lane & 7) == 0 && j0 + (lane >> 3) < cnt)
                    picked[j0 + (lane >> 3)] = (uint8_t)((perm[j0 + (lane >> 3)] >> (4 * mine)) & 7u);
            }
        }
        __syncthreads();
        for (int j = t; j < cnt; j += kPickThreads) {
            const int k = (int)picked[j];
            if (a.picks) a.picks[f0 + j] = (uint8_t)k;
            if (a.chosen) a.chosen[f0 + j] = cand_quality(a.cand, k);
            if (a.pick_dist) a.pick_dist[f0 + j] = a.dist[(size_t)k * a.stride + f0 + j];
        }
    }
    if (t == 0) { // (lane 0 of wave 0: it walked)
        *a.level_out = level;
        *a.status = bits | (over ? (uint32_t)M1V_STATUS_OVER_BUDGET : 0u);
    }
}

// Object identity through a video (no reference counterpart): which object of one frame pair is which object
// of the next.
//
//   raft_object_overlap       the labels of pair t carried along the flow into the next frame and counted against the labels there
//   raft_match_objects        one-to-one matching of the slots from the counts (the greedy walk, as rounds of mutual best picks)
//   raft_chain_object_ids     identities handed on through S consecutive steps in one launch
//
// The definition is written down once in include/raft_hip.h and restated in NumPy in tests/test_object_track.py.  Everything here
// is an integer: the counts are integer sums taken with integer atomics, which do not depend on the order they arrive in; a
// landing pixel is ONE float32 addition and one rintf per component (contraction is off in this file); admissibility is one
// float64 product of exact integers and a float32, and one comparison.  So the result is a function of the input alone and repeats
// bit for bit.
//
// Launches, all on `stream`:
//   raft_object_overlap: two memsets (overlap, landed), then overlap_kernel: one pass over the pixels in 32 x 16 tiles (one
//      workgroup of 256 threads, two pixels per thread, csrc/components.hip's tiling).  A tile meets few distinct (a, b): its
//      counts are put together in LDS first -- `landed` in an array of one entry per slot, the pairs in a direct-mapped table of
//      128 entries keyed by a * K + b (a pair that finds its entry taken sends its own global atomic) -- and one thread per
//      non-empty entry sends one global atomic.  labels_next is gathered at the landing pixel; nothing is read that this launch
//      writes.
//   raft_match_objects: match_kernel, one workgroup of 1024 threads per image.  A round walks the K x K table once, coalesced:
//      every admissible pair whose two slots are free offers its key to its row's and to its column's maximum in LDS (integer
//      maxima: any order), then every free next slot whose column maximum is also its row's maximum takes that pair.  Keys are
//      unique, so the largest remaining pair is always mutual: a round that has a pair left matches one, and at most K rounds run.
//      The first round also takes the column maxima over ALL pairs with a count: `origin`.
//   raft_chain_object_ids: chain_kernel, one workgroup of 128 threads per video walks the S steps: thread b owns slot b, the
//      previous step's ids live in LDS, the unmatched filled slots are ranked by an ordered prefix scan (csrc/point_detect.hip's
//      refill).
// No workgroup waits for another; within a launch no workgroup reads global memory that another writes.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 16, kTile = kTileW * kTileH;      // pixels of a workgroup (two per thread)
constexpr int kMine = kTile / kThreads;
constexpr int kMaxSlots = RAFT_TRACK_OBJECTS_MAX;
constexpr int kCache = 128;                                            // a workgroup's direct-mapped LDS table of pairs
constexpr int kCacheShift = 25;                                        // 32 - log2(kCache)
constexpr int kMatchThreads = 1024;
constexpr int kChainThreads = kMaxSlots;
constexpr int kMaxGridY = 65535;
static_assert(kMaxSlots <= kThreads && kCache <= kThreads && (1 << (32 - kCacheShift)) == kCache, "one thread per table entry");
static_assert(kMaxSlots <= 0xFFFF, "a slot fits the 16 bits a key gives it");

__device__ __forceinline__ bool finite_f32(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }      // (a NaN fails)

// slot of a label, or -1: a label outside 1 .. K is background (the unsigned comparison also turns every negative label away)
__device__ __forceinline__ int slot_of(int32_t label, int K) {
    const uint32_t s = (uint32_t)label - 1u;
    return s < (uint32_t)K ? (int)s : -1;
}

// ---------------------------------------------------------------- raft_object_overlap
// xmax, ymax: the largest float32 that is <= W - 1, H - 1 (the numbers themselves up to 2^24): an integer-valued float is <= it
// iff it is <= W - 1, so the comparison is exact and an index never leaves the row
__global__ void __launch_bounds__(kThreads) overlap_kernel(const int32_t *__restrict__ labels_prev, const float *__restrict__ flow,
                                                           const int32_t *__restrict__ labels_next, int32_t *__restrict__ overlap,
                                                           int32_t *__restrict__ landed, int M, int H, int W, int K, int tiles_x,
                                                           float xmax, float ymax) {
    __shared__ int hkey[kCache];                          // the pairs this tile met (a * K + b; -1: free) and their counts
    __shared__ int hcnt[kCache];
    __shared__ int lcnt[kMaxSlots];                       // pixels of slot a that landed in frame
    const int tid = (int)threadIdx.x;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int64_t HW = (int64_t)H * W;
    for (int m = (int)blockIdx.y; m < M; m += (int)gridDim.y) {
        const int64_t base = (int64_t)m * HW;
        if (tid < kCache) hkey[tid] = -1, hcnt[tid] = 0;
        if (tid < kMaxSlots) lcnt[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int y = y0 + l / kTileW, x = x0 + l % kTileW;
            if (y >= H || x >= W) continue;
            const int64_t at = base + (int64_t)y * W + x;
            const int a = slot_of(labels_prev[at], K);
            if (a < 0) continue;
            const float u = flow[2 * at], v = flow[2 * at + 1];
            if (!finite_f32(u) || !finite_f32(v)) continue;
            const float fx = (float)x + u, fy = (float)y + v;
            const float qx = rintf(fx), qy = rintf(fy);
            if (!(qx >= 0.f && qx <= xmax && qy >= 0.f && qy <= ymax)) continue;      // (an infinite sum fails)
            atomicAdd(&lcnt[a], 1);
            const int b = slot_of(labels_next[base + (int64_t)(int)qy * W + (int)qx], K);
            if (b < 0) continue;
            const int pair = a * K + b;
            const uint32_t e = ((uint32_t)pair * 2654435761u) >> kCacheShift;
            const int old = atomicCAS(&hkey[e], -1, pair);
            if (old == -1 || old == pair)
                atomicAdd(&hcnt[e], 1);
            else
                atomicAdd(overlap + (int64_t)m * K * K + pair, 1);
        }
        __syncthreads();
        if (tid < kMaxSlots && lcnt[tid] != 0) atomicAdd(landed + (int64_t)m * K + tid, lcnt[tid]);      // (lcnt[a] != 0 only for a < K)
        if (tid < kCache && hkey[tid] >= 0) atomicAdd(overlap + (int64_t)m * K * K + hkey[tid], hcnt[tid]);
        __syncthreads();                                  // (the tables are rewritten for the next image)
    }
}

// ---------------------------------------------------------------- raft_match_objects
__device__ __forceinline__ u64 key_of(int32_t count, int a, int b) {
    return ((u64)(uint32_t)count << 32) | ((u64)(uint32_t)(0xFFFF - a) << 16) | (u64)(uint32_t)(0xFFFF - b);
}
__device__ __forceinline__ int key_prev(u64 key) { return 0xFFFF - (int)((key >> 16) & 0xFFFFu); }

__global__ void __launch_bounds__(kMatchThreads) match_kernel(const int32_t *__restrict__ overlap, const int32_t *__restrict__ landed,
                                                              const int32_t *__restrict__ area_next, float min_overlap,
                                                              int32_t *__restrict__ match, int32_t *__restrict__ match_overlap,
                                                              int32_t *__restrict__ origin, int K) {
    __shared__ u64 best_row[kMaxSlots], best_col[kMaxSlots], all_col[kMaxSlots];
    __shared__ int s_landed[kMaxSlots], s_area[kMaxSlots], s_match[kMaxSlots], s_count[kMaxSlots];
    __shared__ int used_prev[kMaxSlots];
    __shared__ int s_any;
    const int tid = (int)threadIdx.x;
    const int64_t m = blockIdx.x;
    const int32_t *tab = overlap + m * K * K;
    if (tid < K) {
        s_landed[tid] = landed[m * K + tid], s_area[tid] = area_next[m * K + tid];
        s_match[tid] = -1, s_count[tid] = 0, used_prev[tid] = 0, all_col[tid] = 0;
    }
    const double share = (double)min_overlap;
    for (int round = 0; round < K; ++round) {             // (every round that goes on matches a pair: at most K)
        if (tid < K) best_row[tid] = 0, best_col[tid] = 0;
        if (tid == 0) s_any = 0;
        __syncthreads();
        for (int i = tid; i < K * K; i += kMatchThreads) {
            const int32_t c = tab[i];
            if (c < 1) continue;
            const int a = i / K, b = i - a * K;
            const u64 key = key_of(c, a, b);
            if (round == 0) atomicMax(&all_col[b], key);
            if (used_prev[a] || s_match[b] >= 0) continue;
            const int la = s_landed[a], ar = s_area[b];
            if (!((double)c >= share * (double)(la < ar ? la : ar))) continue;
            atomicMax(&best_row[a], key), atomicMax(&best_col[b], key);
        }
        __syncthreads();
        if (tid < K && s_match[tid] < 0) {                // (a taken slot has offered nothing: its maxima are 0)
            const u64 key = best_col[tid];
            if (key != 0) {
                const int a = key_prev(key);
                if (best_row[a] == key) {                 // mutual: nobody else's best_col can equal best_row[a], keys are unique
                    s_match[tid] = a, s_count[tid] = (int)(uint32_t)(key >> 32), used_prev[a] = 1;
                    s_any = 1;
                }
            }
        }
        __syncthreads();
        if (!s_any) break;                                // (the same for every thread: read behind the barrier)
        __syncthreads();                                  // (s_any is cleared by the next round)
    }
    if (tid < K) {
        match[m * K + tid] = s_match[tid];
        if (match_overlap != nullptr) match_overlap[m * K + tid] = s_count[tid];
        if (origin != nullptr) origin[m * K + tid] = all_col[tid] != 0 ? key_prev(all_col[tid]) : -1;
    }
}

// ---------------------------------------------------------------- raft_chain_object_ids
// (ids_in / ids and born_in / born may be the same arrays when S == 1: no __restrict__ on them)
__global__ void __launch_bounds__(kChainThreads) chain_kernel(const int32_t *__restrict__ match, const int32_t *__restrict__ count, int t0,
                                                              const int32_t *ids_in, const int32_t *born_in,
                                                              int32_t *__restrict__ next_id, int32_t *ids, int32_t *born, int S, int N,
                                                              int K) {
    __shared__ int prev_id[kMaxSlots], prev_born[kMaxSlots], scan[kChainThreads];
    const int tid = (int)threadIdx.x;
    const int64_t n = blockIdx.x;
    const bool mine = tid < K;
    if (mine) prev_id[tid] = ids_in[n * K + tid], prev_born[tid] = born_in[n * K + tid];
    int32_t next = next_id[n];
    __syncthreads();                                      // the previous state is read before anything is written
    for (int s = 0; s < S; ++s) {
        const int64_t row = ((int64_t)s * N + n) * K;
        int cnt = count[(int64_t)s * N + n];
        cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
        int a = mine ? match[row + tid] : -1;
        if (a < 0 || a >= K) a = -1;
        const bool filled = mine && tid < cnt;
        const int flag = (filled && a < 0) ? 1 : 0;
        scan[tid] = flag;
        __syncthreads();
        for (int off = 1; off < kChainThreads; off <<= 1) {
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int rank = scan[tid] - flag, fresh = scan[kChainThreads - 1];
        int32_t id = -1, b0 = -1;
        if (filled) {
            if (a >= 0)
                id = prev_id[a], b0 = prev_born[a];
            else
                id = next + rank, b0 = t0 + s;
        }
        __syncthreads();                                  // every slot has read the step before
        if (mine) {
            prev_id[tid] = id, prev_born[tid] = b0;
            ids[row + tid] = id, born[row + tid] = b0;
        }
        next += fresh;
        __syncthreads();
    }
    if (tid == 0) next_id[n] = next;
}

// ---------------------------------------------------------------- host side
static inline bool aligned4(const void *p) { return (((uintptr_t)p) & 3u) == 0; }

// the largest float32 that is <= v (v >= 0)
static inline float float_at_most(int v) {
    float f = (float)v;
    if ((int64_t)f > (int64_t)v) f = nextafterf(f, 0.f);
    return f;
}

}   // namespace

extern "C" int raft_object_overlap(const int32_t *labels_prev, const float *flow, const int32_t *labels_next, int32_t *overlap,
                                   int32_t *landed, int M, int H, int W, int K, void *stream) {
    RAFT_REQUIRE_PTR(labels_prev);
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(labels_next);
    RAFT_REQUIRE_PTR(overlap);
    RAFT_REQUIRE_PTR(landed);
    RAFT_REQUIRE(M > 0 && H > 0 && W > 0 && K >= 1 && K <= kMaxSlots, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)H * W <= (((int64_t)1 << 31) - 1) / M, RAFT_E_SHAPE);                // M * H * W < 2^31
    RAFT_REQUIRE(aligned4(labels_prev) && aligned4(flow) && aligned4(labels_next) && aligned4(overlap) && aligned4(landed), RAFT_E_ALIGN);
    hipStream_t st = (hipStream_t)stream;
    RAFT_TRY((int)hipMemsetAsync(overlap, 0, (size_t)M * K * K * 4, st));
    RAFT_TRY((int)hipMemsetAsync(landed, 0, (size_t)M * K * 4, st));
    const int tiles_x = (W + kTileW - 1) / kTileW;
    const int64_t tiles = (int64_t)tiles_x * ((H + kTileH - 1) / kTileH);
    const dim3 grid((unsigned)tiles, (unsigned)(M < kMaxGridY ? M : kMaxGridY));
    overlap_kernel<<<grid, kThreads, 0, st>>>(labels_prev, flow, labels_next, overlap, landed, M, H, W, K, tiles_x, float_at_most(W - 1),
                                              float_at_most(H - 1));
    return raft_launch_status();
}

extern "C" int raft_match_objects(const int32_t *overlap, const int32_t *landed, const int32_t *area_next, float min_overlap,
                                  int32_t *match, int32_t *match_overlap, int32_t *origin, int M, int K, void *stream) {
    RAFT_REQUIRE_PTR(overlap);
    RAFT_REQUIRE_PTR(landed);
    RAFT_REQUIRE_PTR(area_next);
    RAFT_REQUIRE_PTR(match);
    RAFT_REQUIRE(M > 0 && K >= 1 && K <= kMaxSlots, RAFT_E_SHAPE);
    RAFT_REQUIRE(min_overlap > 0.f && min_overlap <= 1.f, RAFT_E_SHAPE);                        // (a NaN fails)
    RAFT_REQUIRE(aligned4(overlap) && aligned4(landed) && aligned4(area_next) && aligned4(match) && aligned4(match_overlap) &&
                     aligned4(origin), RAFT_E_ALIGN);
    match_kernel<<<(unsigned)M, kMatchThreads, 0, (hipStream_t)stream>>>(overlap, landed, area_next, min_overlap, match, match_overlap,
                                                                         origin, K);
    return raft_launch_status();
}

extern "C" int raft_chain_object_ids(const int32_t *match, const int32_t *count, int t0, const int32_t *ids_in, const int32_t *born_in,
                                     int32_t *next_id, int32_t *ids, int32_t *born, int S, int N, int K, void *stream) {
    RAFT_REQUIRE_PTR(match);
    RAFT_REQUIRE_PTR(count);
    RAFT_REQUIRE_PTR(ids_in);
    RAFT_REQUIRE_PTR(born_in);
    RAFT_REQUIRE_PTR(next_id);
    RAFT_REQUIRE_PTR(ids);
    RAFT_REQUIRE_PTR(born);
    RAFT_REQUIRE(S > 0 && N > 0 && K >= 1 && K <= kMaxSlots, RAFT_E_SHAPE);
    RAFT_REQUIRE(t0 >= 0 && (int64_t)t0 + S <= (((int64_t)1 << 31) - 1), RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)S * N <= (((int64_t)1 << 31) - 1) / K, RAFT_E_SHAPE);                 // S * N * K < 2^31
    RAFT_REQUIRE(aligned4(match) && aligned4(count) && aligned4(ids_in) && aligned4(born_in) && aligned4(next_id) && aligned4(ids) &&
                     aligned4(born), RAFT_E_ALIGN);
    chain_kernel<<<(unsigned)N, kChainThreads, 0, (hipStream_t)stream>>>(match, count, t0, ids_in, born_in, next_id, ids, born, S, N, K);
    return raft_launch_status();
}

// The range map of a flow (Wang et al. 2018, "Occlusion Aware Unsupervised Learning of Optical Flow"): a
// forward splat of the flow itself, as a second occlusion test next to the forward-backward check of flow_check.hip.
//
//   raft_flow_range_map_f32          range[n, y, x] = how much of the flow's source grid lands on (x, y) under bilinear weights
//   raft_flow_range_occlusion_f32    occluded_a = range of flow_b < threshold || flow_a leaves the frame; both directions
//   raft_flow_range_visibility_f32   the same test on the 2N flows of a bidirectional training step, as the mask of its loss:
//                                    visible = mask && !(apply && occluded), and the occluded share
//
// The accumulator, stated once.  The source pixel at integer (x, y) with vector (u, v): sx = float(x) + u, sy = float(y) + v, ONE
// float32 addition each (flow_sample.h's sample position).  It contributes iff -1 < sx < W and -1 < sy < H, compared on the
// floats (a NaN, an infinity or 1e30 fails before any conversion to an integer).  x0 = floor(sx), a = sx - x0 in float32,
// qa = (int)rintf(a * 4096) in 0 .. 4096, likewise y0, b, qb; the corner (x0 + dx, y0 + dy) receives the INTEGER weight
// (dx ? qa : 4096 - qa) * (dy ? qb : 4096 - qb), the four of which sum to exactly 2^24; a corner outside the frame or of weight 0
// receives nothing.  acc[n, cy, cx] is the uint64 sum of what lands there: integer sums are exact in any arrival order, so this
// scatter repeats bit for bit and equals its NumPy restatement (tests/test_range_occlusion.py) exactly.  uint64 because every
// vector of a frame may land on one pixel: 1961 * 2^24 > 2^32 at 37 x 53 already.
//
// Three phases on the caller's stream:
//   1. the accumulator is zeroed (hipMemsetAsync);
//   2. scatter: one thread per SOURCE pixel, a wave along a row; up to four no-return 64-bit integer atomic adds per vector,
//      into the workgroup's LDS window where the vector lands near its tile and at device scope into memory otherwise, then
//      one device-scope add per non-zero cell of the window, rows of consecutive 8-byte words;
//   3. finalise: one thread per DESTINATION pixel reads its sum once and writes the range, the masks, or the visibility mask
//      with the occluded count through the loss kernels' deterministic reduction (loss_common.h), as raft_flow_visibility_f32
//      does.
// Every comparison against the threshold is made on the integers: acc < T with T = (uint64)ceil(double(t) * 2^24).
#include "common.h"

#pragma clang fp contract(off)

#include "flow_sample.h"      // flow_taps: the in-frame test of a pixel's own vector
#include "loss_common.h"      // the deterministic reduction of raft_flow_range_visibility_f32's count
#include "splat_geometry.h"   // splat_taps: the in-range test and the four integer weights, shared with frame_splat.hip

namespace {

constexpr int kSplatThreads = 256;
constexpr int64_t kRangeMaxPixels = (int64_t)1 << 28;        // double(acc) * 2^-24 stays exact: acc <= H * W * 2^24 <= 2^52
constexpr int kRangeColumns = 64;                            // the records are summed as rows of 64, as flow_check.hip's are

typedef unsigned long long u64;

// The scatter.  A workgroup owns a tile of kTileW x kTileH SOURCE pixels (a wave reads one row of 64 vectors as a 512-byte run)
// and sums what lands within kHalo pixels of the tile in LDS first (64-bit LDS atomics), whatever lands further away goes
// straight to memory.  It then adds every non-zero cell of its window to memory, rows of consecutive 8-byte words: under a flow
// of a few pixels that is about one atomic per pixel instead of four (docs/NOTEBOOK.md section 31).  Integer sums: the split
// between LDS and memory changes no bit.  Slice s of the accumulator receives the vectors of src0's slice s (s < N) or of src1's
// slice s - N.  blockIdx.x: tile column; blockIdx.y: tile rows, blockIdx.z: slices (both strided: the grid is capped).
constexpr int kTileW = 64, kTileH = 32, kHalo = 8;
constexpr int kWinW = kTileW + 2 * kHalo, kWinH = kTileH + 2 * kHalo, kWinCells = kWinW * kWinH;      // 80 x 48 sums: 30 KB
static_assert(kTileW == 64 && kSplatThreads == 256 && kTileH % 4 == 0, "one wave per tile row, four rows in flight");

__global__ void __launch_bounds__(kSplatThreads) range_scatter_kernel(const float2 *__restrict__ src0, const float2 *__restrict__ src1,
                                                                      u64 *__restrict__ acc, int N, int H, int W, int slices,
                                                                      int tiles_y) {
    __shared__ u64 win[kWinCells];
    const int HW = H * W;
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x & 63), row = (int)(threadIdx.x >> 6);
    const int ox = (int)blockIdx.x * kTileW - kHalo;                        // the window's origin in the frame
    const float fW = (float)W, fH = (float)H;
    for (int s = blockIdx.z; s < slices; s += gridDim.z) {
        const float2 *src = s >= N ? src1 + (int64_t)(s - N) * HW : src0 + (int64_t)s * HW;
        u64 *dst = acc + (int64_t)s * HW;
        for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
            const int oy = ty * kTileH - kHalo;
            for (int i = threadIdx.x; i < kWinCells; i += kSplatThreads) win[i] = 0;
            __syncthreads();
            for (int k = 0; k < kTileH; k += 4) {
                const int y = ty * kTileH + row + k;
                if (x >= W || y >= H) continue;
                const float2 f = src[y * W + x];
                const float sx = (float)x + f.x, sy = (float)y + f.y;
                const SplatTaps g = splat_taps(sx, sy, fW, fH);                     // the in-range test and the weights (splat_geometry.h)
                if (!g.in) continue;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int cy = g.y0 + dy;
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int cx = g.x0 + dx;
                        const unsigned w = g.wx[dx] * g.wy[dy];                     // <= 2^24
                        if (w == 0u || cx < 0 || cx >= W || cy < 0 || cy >= H) continue;
                        const int lx = cx - ox, ly = cy - oy;
                        if ((unsigned)lx < (unsigned)kWinW && (unsigned)ly < (unsigned)kWinH)
                            atomicAdd(&win[ly * kWinW + lx], (u64)w);
                        else
                            atomicAdd(dst + (cy * W + cx), (u64)w);
                    }
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < kWinCells; i += kSplatThreads) {
                const u64 v = win[i];
                if (v == 0) continue;                                               // (only cells inside the frame were added to)
                const int ly = i / kWinW, lx = i - ly * kWinW;
                atomicAdd(dst + ((oy + ly) * W + (ox + lx)), v);
            }
            __syncthreads();                                                        // the window is zeroed again for the next tile
        }
    }
}

__global__ void __launch_bounds__(kSplatThreads) range_map_kernel(const u64 *__restrict__ acc, float *__restrict__ range, int HW,
                                                                  int slices) {
    const int p = (int)blockIdx.x * kSplatThreads + (int)threadIdx.x;
    if (p >= HW) return;
    for (int s = blockIdx.y; s < slices; s += gridDim.y) {
        const int64_t i = (int64_t)s * HW + p;
        range[i] = (float)((double)acc[i] * (1.0 / 16777216.0));
    }
}

// the test of one destination pixel: too little of the other flow lands here, or the pixel's own vector leaves the frame
__device__ __forceinline__ uint32_t range_occluded_at(u64 sum, u64 T, float2 own, int x, int y, int H, int W) {
    return (sum < T || !flow_taps(x, y, own, H, W).in) ? 1u : 0u;
}

// Slice s < N: direction a (own vector from own0, mask into occ0); slice s >= N: direction b.
__global__ void __launch_bounds__(kSplatThreads) range_occlusion_kernel(const u64 *__restrict__ acc, const float2 *__restrict__ own0,
                                                                        const float2 *__restrict__ own1, uint8_t *__restrict__ occ0,
                                                                        uint8_t *__restrict__ occ1, int N, int H, int W, int slices,
                                                                        u64 T) {
    const int HW = H * W;
    const int p = (int)blockIdx.x * kSplatThreads + (int)threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    for (int s = blockIdx.y; s < slices; s += gridDim.y) {
        const bool second = s >= N;                  // wave-uniform
        const int64_t base = (int64_t)(second ? s - N : s) * HW;
        const float2 own = ((second ? own1 : own0) + base)[p];
        (second ? occ1 : occ0)[base + p] = (uint8_t)range_occluded_at(acc[(int64_t)s * HW + p], T, own, x, y, H, W);
    }
}

// The in-step form: flow_visibility_kernel's walk, records and tail (flow_check.hip) with the range test in place of the
// consistency test.  Slice s of `flows` is tested against slice s of the accumulator.
__global__ void __launch_bounds__(kSplatThreads) range_visibility_kernel(const u64 *__restrict__ acc, const float2 *__restrict__ flows,
                                                                         const uint8_t *__restrict__ mask, uint8_t *__restrict__ visible,
                                                                         int N, int H, int W, u64 T, int apply,
                                                                         double *__restrict__ part) {
    const int HW = H * W;
    double cnt[1] = {0.0};
    for (int s = blockIdx.y; s < 2 * N; s += gridDim.y) {
        const int64_t base = (int64_t)s * HW;
        for (int64_t q = (int64_t)blockIdx.x * kSplatThreads + threadIdx.x; q < HW; q += (int64_t)gridDim.x * kSplatThreads) {
            const int p = (int)q, y = p / W, x = p - y * W;
            const uint32_t occ = range_occluded_at(acc[base + p], T, flows[base + p], x, y, H, W);
            cnt[0] += (double)occ;
            if (visible != nullptr) {
                const bool use = mask == nullptr || mask[base + p] != 0;
                visible[base + p] = (use && !(apply && occ)) ? 1 : 0;
            }
        }
    }
    raft_block_sum_store(cnt, part);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < kRangeColumns) {
        const int nparts = (int)(gridDim.x * gridDim.y), tail = nparts + (int)threadIdx.x;      // (the grid holds whole rows)
        if (tail < (nparts + kRangeColumns - 1) / kRangeColumns * kRangeColumns) part[tail] = 0.0;
    }
}

__global__ void __launch_bounds__(64) range_visibility_final_kernel(const double *__restrict__ part, int rows, double total,
                                                                    float *__restrict__ occluded_fraction) {
    __shared__ double tot[kRangeColumns];
    raft_sum_records(part, rows, tot);
    if (threadIdx.x == 0) {
        double count = 0.0;
        for (int k = 0; k < kRangeColumns; ++k) count += tot[k];
        occluded_fraction[0] = (float)(count / total);
    }
}

// what flow_check.hip asks of a flow's sizes (positive, fewer than 2^31 floats), and a frame the range map stays exact on
int range_sizes(int N, int H, int W) {
    RAFT_REQUIRE(N > 0 && H > 0 && W > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)W * 2 <= 0x7fffffff, RAFT_E_SHAPE);
    const int64_t limit = ((int64_t)1 << 31) - 1;
    RAFT_REQUIRE((int64_t)N <= limit / H && (int64_t)N * H <= limit / W && (int64_t)N * H * W <= limit / 2, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)H * W <= kRangeMaxPixels, RAFT_E_SHAPE);
    return RAFT_OK;
}

bool range_threshold_ok(float t) { return t > 0.f && t <= 1.f; }      // (a NaN fails)

u64 range_threshold_sum(float t) { return (u64)ceil((double)t * 16777216.0); }

dim3 range_grid(int H, int W, int64_t slices) {
    return dim3((unsigned)(((int64_t)H * W + kSplatThreads - 1) / kSplatThreads), (unsigned)(slices < 65535 ? slices : 65535));
}

// phases 1 and 2: `slices` accumulator slices of H * W sums from src0's (and, beyond N, src1's) vectors
int range_accumulate(const float *src0, const float *src1, void *workspace, int N, int H, int W, int slices, hipStream_t s) {
    RAFT_TRY((int)hipMemsetAsync(workspace, 0, (size_t)slices * H * W * sizeof(u64), s));
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const dim3 grid((unsigned)tiles_x, (unsigned)(tiles_y < 65535 ? tiles_y : 65535), (unsigned)(slices < 65535 ? slices : 65535));
    range_scatter_kernel<<<grid, kSplatThreads, 0, s>>>((const float2 *)src0, (const float2 *)src1, (u64 *)workspace, N, H, W, slices,
                                                        tiles_y);
    return raft_launch_status();
}

}   // namespace

extern "C" int64_t raft_flow_range_workspace_bytes(int slices, int H, int W) {
    if (slices <= 0 || range_sizes(slices, H, W) != RAFT_OK) return 0;
    return (int64_t)slices * H * W * (int64_t)sizeof(u64);
}

extern "C" int raft_flow_range_map_f32(const float *flow, float *range, int N, int H, int W, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(range);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_TRY(range_sizes(N, H, W));
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);      // read as float2; uint64 sums
    hipStream_t s = (hipStream_t)stream;
    RAFT_TRY(range_accumulate(flow, flow, workspace, N, H, W, N, s));
    range_map_kernel<<<range_grid(H, W, N), kSplatThreads, 0, s>>>((const u64 *)workspace, range, H * W, N);
    return raft_launch_status();
}

extern "C" int raft_flow_range_occlusion_f32(const float *flow_a, const float *flow_b, uint8_t *occluded_a, uint8_t *occluded_b, int N,
                                             int H, int W, float threshold, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(flow_a);
    RAFT_REQUIRE_PTR(flow_b);
    RAFT_REQUIRE_PTR(occluded_a);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_TRY(range_sizes(N, H, W));
    RAFT_REQUIRE(range_threshold_ok(threshold), RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)flow_a) | ((uintptr_t)flow_b) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);
    const int slices = occluded_b != nullptr ? 2 * N : N;
    hipStream_t s = (hipStream_t)stream;
    // frame A's sums come from flow_b (it lives on B's grid and lands on A's), frame B's from flow_a
    RAFT_TRY(range_accumulate(flow_b, flow_a, workspace, N, H, W, slices, s));
    range_occlusion_kernel<<<range_grid(H, W, slices), kSplatThreads, 0, s>>>((const u64 *)workspace, (const float2 *)flow_a,
                                                                             (const float2 *)flow_b, occluded_a, occluded_b, N, H, W,
                                                                             slices, range_threshold_sum(threshold));
    return raft_launch_status();
}

extern "C" int raft_flow_range_visibility_f32(const float *flows, const uint8_t *mask, uint8_t *visible, float *occluded_fraction, int N,
                                              int H, int W, float threshold, int apply, void *workspace, double *records, void *stream) {
    RAFT_REQUIRE_PTR(flows);
    RAFT_REQUIRE_PTR(occluded_fraction);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE_PTR(records);
    RAFT_REQUIRE(N > 0 && N < (1 << 29), RAFT_E_SHAPE);              // (2 * N below stays an int)
    RAFT_TRY(range_sizes(2 * N, H, W));
    RAFT_REQUIRE(range_threshold_ok(threshold), RAFT_E_SHAPE);
    RAFT_REQUIRE(apply == 0 || apply == 1, RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)flows) | ((uintptr_t)workspace) | ((uintptr_t)records)) & 7u) == 0, RAFT_E_ALIGN);
    const int64_t HW = (int64_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    // slice s < N (a forward flow) is tested against the sums of the backward flow s + N, and the other way round
    RAFT_TRY(range_accumulate(flows + (int64_t)N * HW * 2, flows, workspace, N, H, W, 2 * N, s));
    const int records_cap = (int)raft_flow_visibility_workspace_doubles() / kRangeColumns * kRangeColumns;      // whole rows of `records`
    const dim3 grid = raft_record_grid(2 * N, HW, records_cap);
    range_visibility_kernel<<<grid, kSplatThreads, 0, s>>>((const u64 *)workspace, (const float2 *)flows, mask, visible, N, H, W,
                                                          range_threshold_sum(threshold), apply, records);
    RAFT_TRY(raft_launch_status());
    const int rows = ((int)(grid.x * grid.y) + kRangeColumns - 1) / kRangeColumns;
    range_visibility_final_kernel<<<1, 64, 0, s>>>(records, rows, (double)(2 * N) * (double)HW, occluded_fraction);
    return raft_launch_status();
}

// The forward splat of FRAMES along a flow, and the frame in between two frames: flow_splat.hip's integer
// accumulator carried over to colour.
//
//   raft_splat_frames_{f32,u8_f32}             dst = the frame splatted to time t along its flow, weight = how much landed
//   raft_interpolate_frames_{f32,u8_f32,u8}    frame 1 splatted to t along the forward flow and frame 2 to 1 - t along the
//                                              backward flow in ONE scatter, blended per pixel, holes cross-faded
//
// The accumulator, stated once.  The source pixel at integer (x, y) of slice n with vector (u, v) and time t (float32):
// sx = float(x) + t * u, sy = float(y) + t * v, ONE float32 multiplication and ONE float32 addition each.  It contributes iff
// -1 < sx < W and -1 < sy < H (a NaN, an infinity or 1e30 fails) and, under a mask, mask[n, y, x] != 0.  The four corners and
// their integer weights w are splat_geometry.h's, the range map's own rule.  Each destination pixel holds C + 1 uint64 sums,
// consecutive in memory: W += w and per channel S_c += w * q_c, with q_c the byte of a uint8 frame or
// (int)rintf(fminf(fmaxf(value, 0), 255) * 256) of a float32 frame on 0 .. 255 (a NaN gives 0).  Integer sums are exact in any
// arrival order, so every entry repeats bit for bit and equals its NumPy restatement (tests/test_frame_splat.py) exactly.
// H * W <= 2^24 keeps every sum below 2^64: 2^24 (weight) * 65280 (value) * 2^24 (vectors on one pixel).
//
// Three phases on the caller's stream, as in flow_splat.hip:
//   1. the accumulator is zeroed (hipMemsetAsync);
//   2. scatter: one thread per SOURCE pixel, a wave along a row; up to 4 * (C + 1) no-return 64-bit integer atomic adds per
//      vector, into the workgroup's LDS window (C + 1 planes) where the vector lands near its tile and at device scope into
//      memory otherwise, then one device-scope add per non-zero word of the window: consecutive lanes take the consecutive
//      8-byte words of one pixel and of its row neighbours;
//   3. finalise: one thread per DESTINATION pixel reads its sums once and writes the result in float64 arithmetic.
#include "common.h"

#pragma clang fp contract(off)

#include "splat_geometry.h"   // splat_taps: the in-range test and the four integer weights, shared with flow_splat.hip

namespace {

constexpr int kFrameThreads = 256;
constexpr int kFrameMaxChannels = 4;
constexpr int64_t kFrameMaxPixels = (int64_t)1 << 24;        // 2^24 * 65280 * H * W < 2^64

typedef unsigned long long u64;

// A workgroup of 1024 owns a tile of kFTileW x kFTileH SOURCE pixels, a wave per row and 16 rows in flight, and sums what lands
// within kFHalo pixels of it in LDS: C + 1 planes of 80 x 48 sums, 120 KB at C = 3 and 150 KB at C = 4, so one workgroup (16 waves)
// per CU.  At t = 0.5 a vector moves its pixel by half its length, so the halo covers flows of up to 16 pixels; whatever lands
// further away goes straight to memory.  Smaller tiles, smaller workgroups and halos of 4 and 6 were slower (docs/NOTEBOOK.md
// section 37.4).
constexpr int kFTileW = 64, kFTileH = 32, kFHalo = 8;
constexpr int kFWinW = kFTileW + 2 * kFHalo, kFWinH = kFTileH + 2 * kFHalo, kFWinCells = kFWinW * kFWinH;
constexpr int kFScatterThreads = 1024, kFRows = kFScatterThreads / 64;
static_assert(kFTileW == 64 && kFScatterThreads % 64 == 0 && kFTileH % kFRows == 0, "one wave per tile row");
static_assert((kFrameMaxChannels + 1) * kFWinCells * 8 <= 160 * 1024, "the window fits the CU's LDS");

// the quantised value of one channel: an integer in 0 .. 255 (uint8) or 0 .. 65280 (float32 on 0 .. 255, in 1 / 256)
__device__ __forceinline__ unsigned frame_q(uint8_t v) { return (unsigned)v; }
__device__ __forceinline__ unsigned frame_q(float v) { return (unsigned)(int)rintf(fminf(fmaxf(v, 0.f), 255.f) * 256.f); }

// One direction of a scatter: the frames, their flow, the optional mask and the time the frames are splatted to.
struct SplatSide {
    const void *src;
    const float2 *flow;
    const uint8_t *mask;
    float t;
};

// Slice s of the accumulator receives side a's slice s (s < N) or side b's slice s - N.  blockIdx.x: tile column; blockIdx.y:
// tile rows, blockIdx.z: slices (both strided: the grid is capped).
template <typename T, int C>
__global__ void __launch_bounds__(kFScatterThreads) frame_scatter_kernel(SplatSide a, SplatSide b, u64 *__restrict__ acc, int N, int H, int W,
                                                                      int slices, int tiles_y) {
    constexpr int K = C + 1;
    __shared__ u64 win[K * kFWinCells];                                     // plane k of cell i at k * kFWinCells + i
    const int HW = H * W;
    const int x = (int)blockIdx.x * kFTileW + (int)(threadIdx.x & 63), row = (int)(threadIdx.x >> 6);
    const int ox = (int)blockIdx.x * kFTileW - kFHalo;                      // the window's origin in the frame
    const float fW = (float)W, fH = (float)H;
    for (int s = blockIdx.z; s < slices; s += gridDim.z) {
        const SplatSide side = s >= N ? b : a;                              // workgroup-uniform
        const int64_t base = (int64_t)(s >= N ? s - N : s) * HW;
        const T *src = (const T *)side.src + base * C;
        const float2 *flow = side.flow + base;
        const uint8_t *mask = side.mask != nullptr ? side.mask + base : nullptr;
        const float t = side.t;
        u64 *dst = acc + (int64_t)s * HW * K;
        for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
            const int oy = ty * kFTileH - kFHalo;
            for (int i = threadIdx.x; i < K * kFWinCells; i += kFScatterThreads) win[i] = 0;
            __syncthreads();
            for (int k = 0; k < kFTileH; k += kFRows) {
                const int y = ty * kFTileH + row + k;
                if (x >= W || y >= H) continue;
                const int p = y * W + x;
                if (mask != nullptr && mask[p] == 0) continue;
                const float2 f = flow[p];
                const float sx = (float)x + t * f.x, sy = (float)y + t * f.y;      // (contraction is off: a product, then a sum)
                const SplatTaps g = splat_taps(sx, sy, fW, fH);
                if (!g.in) continue;
                unsigned q[C];
#pragma unroll
                for (int c = 0; c < C; ++c) q[c] = frame_q(src[(int64_t)p * C + c]);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int cy = g.y0 + dy;
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int cx = g.x0 + dx;
                        const unsigned w = g.wx[dx] * g.wy[dy];                     // <= 2^24
                        if (w == 0u || cx < 0 || cx >= W || cy < 0 || cy >= H) continue;
                        const int lx = cx - ox, ly = cy - oy;
                        if ((unsigned)lx < (unsigned)kFWinW && (unsigned)ly < (unsigned)kFWinH) {
                            u64 *cell = &win[ly * kFWinW + lx];
                            atomicAdd(cell, (u64)w);
#pragma unroll
                            for (int c = 0; c < C; ++c) atomicAdd(cell + (c + 1) * kFWinCells, (u64)w * q[c]);
                        } else {
                            u64 *cell = dst + (int64_t)(cy * W + cx) * K;
                            atomicAdd(cell, (u64)w);
#pragma unroll
                            for (int c = 0; c < C; ++c) atomicAdd(cell + (c + 1), (u64)w * q[c]);
                        }
                    }
                }
            }
            __syncthreads();
            // word i of the window in the accumulator's own order: (cell, plane) = (i / K, i % K)
            for (int i = threadIdx.x; i < K * kFWinCells; i += kFScatterThreads) {
                const int cell = i / K, k = i - cell * K;
                if (win[cell] == 0) continue;                                       // nothing landed (only cells inside the frame were added to)
                const u64 v = win[k * kFWinCells + cell];
                if (v == 0) continue;
                const int ly = cell / kFWinW, lx = cell - ly * kFWinW;
                atomicAdd(dst + ((int64_t)((oy + ly) * W + (ox + lx)) * K + k), v);
            }
            __syncthreads();                                                        // the window is zeroed again for the next tile
        }
    }
}

// dst = S_c / W (0 where nothing landed), weight = W * 2^-24.  `scale`: 1 for uint8 frames, 1 / 256 for float32 frames.
__global__ void __launch_bounds__(kFrameThreads) frame_splat_final_kernel(const u64 *__restrict__ acc, float *__restrict__ dst,
                                                                          float *__restrict__ weight, int HW, int C, int slices,
                                                                          double scale) {
    const int p = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    if (p >= HW) return;
    for (int s = blockIdx.y; s < slices; s += gridDim.y) {
        const int64_t i = (int64_t)s * HW + p;
        const u64 *a = acc + i * (C + 1);
        const u64 w = a[0];
        for (int c = 0; c < C; ++c) dst[i * C + c] = w == 0 ? 0.f : (float)(((double)a[1 + c] / (double)w) * scale);
        if (weight != nullptr) weight[i] = (float)((double)w * (1.0 / 16777216.0));
    }
}

__device__ __forceinline__ void frame_store(float *p, double v) { *p = (float)v; }
__device__ __forceinline__ void frame_store(uint8_t *p, double v) { *p = (uint8_t)fmin(rint(v), 255.0); }

// The blend of the two splats of slice n (sums of slices n and n + N), or the cross-fade of the pixel's own two values in a hole.
template <typename T, typename O>
__global__ void __launch_bounds__(kFrameThreads) frame_interpolate_final_kernel(const u64 *__restrict__ acc, const T *__restrict__ image1,
                                                                                const T *__restrict__ image2, O *__restrict__ dst,
                                                                                uint8_t *__restrict__ holes, int HW, int C, int N, float t,
                                                                                double scale) {
    const int p = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    if (p >= HW) return;
    const double td = (double)t, ud = 1.0 - td;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const int64_t i = (int64_t)n * HW + p;
        const u64 *a1 = acc + i * (C + 1), *a2 = acc + (i + (int64_t)N * HW) * (C + 1);
        const double a = ud * (double)a1[0], b = td * (double)a2[0];
        const double den = a + b;
        const bool hole = !(den > 0.0);
        for (int c = 0; c < C; ++c) {
            double out;
            if (!hole) {
                const double s1 = ud * (double)a1[1 + c], s2 = td * (double)a2[1 + c];
                out = (s1 + s2) / den;
            } else {
                const double q1 = ud * (double)frame_q(image1[i * C + c]), q2 = td * (double)frame_q(image2[i * C + c]);
                out = q1 + q2;
            }
            frame_store(dst + (i * C + c), out * scale);
        }
        if (holes != nullptr) holes[i] = hole ? 1 : 0;
    }
}

// positive sizes, 1 .. 4 channels, a frame the sums stay below 2^64 on, and fewer than 2^31 elements in every tensor
int frame_sizes(int64_t slices, int H, int W, int C) {
    RAFT_REQUIRE(slices > 0 && H > 0 && W > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE(C >= 1 && C <= kFrameMaxChannels, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)H * W <= kFrameMaxPixels, RAFT_E_SHAPE);
    const int64_t limit = ((int64_t)1 << 31) - 1;
    RAFT_REQUIRE(slices <= limit / ((int64_t)H * W * kFrameMaxChannels), RAFT_E_SHAPE);
    return RAFT_OK;
}

dim3 frame_grid(int H, int W, int64_t slices) {
    return dim3((unsigned)(((int64_t)H * W + kFrameThreads - 1) / kFrameThreads), (unsigned)(slices < 65535 ? slices : 65535));
}

template <typename T, int C>
int frame_scatter_launch(const SplatSide &a, const SplatSide &b, u64 *acc, int N, int H, int W, int slices, hipStream_t s) {
    const int tiles_x = (W + kFTileW - 1) / kFTileW, tiles_y = (H + kFTileH - 1) / kFTileH;
    const dim3 grid((unsigned)tiles_x, (unsigned)(tiles_y < 65535 ? tiles_y : 65535), (unsigned)(slices < 65535 ? slices : 65535));
    frame_scatter_kernel<T, C><<<grid, kFScatterThreads, 0, s>>>(a, b, acc, N, H, W, slices, tiles_y);
    return raft_launch_status();
}

// phases 1 and 2: `slices` accumulator slices of H * W * (C + 1) sums from side a's (and, beyond N, side b's) pixels
template <typename T>
int frame_accumulate(const SplatSide &a, const SplatSide &b, void *workspace, int N, int H, int W, int C, int slices, hipStream_t s) {
    RAFT_TRY((int)hipMemsetAsync(workspace, 0, (size_t)slices * H * W * (C + 1) * sizeof(u64), s));
    u64 *acc = (u64 *)workspace;
    switch (C) {
        case 1: return frame_scatter_launch<T, 1>(a, b, acc, N, H, W, slices, s);
        case 2: return frame_scatter_launch<T, 2>(a, b, acc, N, H, W, slices, s);
        case 3: return frame_scatter_launch<T, 3>(a, b, acc, N, H, W, slices, s);
        default: return frame_scatter_launch<T, 4>(a, b, acc, N, H, W, slices, s);
    }
}

template <typename T> constexpr double frame_scale() { return 1.0; }
template <> constexpr double frame_scale<float>() { return 0.00390625; }

template <typename T>
int splat_frames(const T *src, const float *flow, const uint8_t *mask, float t, float *dst, float *weight, int N, int H, int W, int C,
                 void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_TRY(frame_sizes(N, H, W, C));
    RAFT_REQUIRE(t - t == 0.f, RAFT_E_SHAPE);                       // finite (a NaN or an infinity fails)
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);      // read as float2; uint64 sums
    hipStream_t s = (hipStream_t)stream;
    const SplatSide side = {src, (const float2 *)flow, mask, t};
    RAFT_TRY(frame_accumulate<T>(side, side, workspace, N, H, W, C, N, s));
    frame_splat_final_kernel<<<frame_grid(H, W, N), kFrameThreads, 0, s>>>((const u64 *)workspace, dst, weight, H * W, C, N,
                                                                          frame_scale<T>());
    return raft_launch_status();
}

template <typename T, typename O>
int interpolate_frames(const T *image1, const T *image2, const float *flow_forward, const float *flow_backward, const uint8_t *mask1,
                       const uint8_t *mask2, float t, O *dst, uint8_t *holes, int N, int H, int W, int C, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(image1);
    RAFT_REQUIRE_PTR(image2);
    RAFT_REQUIRE_PTR(flow_forward);
    RAFT_REQUIRE_PTR(flow_backward);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(N > 0 && N < (1 << 29), RAFT_E_SHAPE);              // (2 * N below stays an int)
    RAFT_TRY(frame_sizes(2 * (int64_t)N, H, W, C));
    RAFT_REQUIRE(t >= 0.f && t <= 1.f, RAFT_E_SHAPE);               // (a NaN fails)
    RAFT_REQUIRE(((((uintptr_t)flow_forward) | ((uintptr_t)flow_backward) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);
    hipStream_t s = (hipStream_t)stream;
    const SplatSide a = {image1, (const float2 *)flow_forward, mask1, t};
    const SplatSide b = {image2, (const float2 *)flow_backward, mask2, 1.f - t};
    RAFT_TRY(frame_accumulate<T>(a, b, workspace, N, H, W, C, 2 * N, s));
    frame_interpolate_final_kernel<T, O><<<frame_grid(H, W, N), kFrameThreads, 0, s>>>((const u64 *)workspace, image1, image2, dst, holes,
                                                                                      H * W, C, N, t, frame_scale<T>());
    return raft_launch_status();
}

}   // namespace

extern "C" int64_t raft_frame_splat_workspace_bytes(int slices, int H, int W, int C) {
    if (frame_sizes(slices, H, W, C) != RAFT_OK) return 0;
    return (int64_t)slices * H * W * (C + 1) * (int64_t)sizeof(u64);
}

extern "C" int raft_splat_frames_f32(const float *src, const float *flow, const uint8_t *mask, float t, float *dst, float *weight, int N,
                                     int H, int W, int C, void *workspace, void *stream) {
    return splat_frames<float>(src, flow, mask, t, dst, weight, N, H, W, C, workspace, stream);
}

extern "C" int raft_splat_frames_u8_f32(const uint8_t *src, const float *flow, const uint8_t *mask, float t, float *dst, float *weight,
                                        int N, int H, int W, int C, void *workspace, void *stream) {
    return splat_frames<uint8_t>(src, flow, mask, t, dst, weight, N, H, W, C, workspace, stream);
}

extern "C" int raft_interpolate_frames_f32(const float *image1, const float *image2, const float *flow_forward, const float *flow_backward,
                                           const uint8_t *mask1, const uint8_t *mask2, float t, float *dst, uint8_t *holes, int N, int H,
                                           int W, int C, void *workspace, void *stream) {
    return interpolate_frames<float, float>(image1, image2, flow_forward, flow_backward, mask1, mask2, t, dst, holes, N, H, W, C, workspace,
                                            stream);
}

extern "C" int raft_interpolate_frames_u8_f32(const uint8_t *image1, const uint8_t *image2, const float *flow_forward,
                                              const float *flow_backward, const uint8_t *mask1, const uint8_t *mask2, float t, float *dst,
                                              uint8_t *holes, int N, int H, int W, int C, void *workspace, void *stream) {
    return interpolate_frames<uint8_t, float>(image1, image2, flow_forward, flow_backward, mask1, mask2, t, dst, holes, N, H, W, C,
                                              workspace, stream);
}

extern "C" int raft_interpolate_frames_u8(const uint8_t *image1, const uint8_t *image2, const float *flow_forward,
                                          const float *flow_backward, const uint8_t *mask1, const uint8_t *mask2, float t, uint8_t *dst,
                                          uint8_t *holes, int N, int H, int W, int C, void *workspace, void *stream) {
    return interpolate_frames<uint8_t, uint8_t>(image1, image2, flow_forward, flow_backward, mask1, mask2, t, dst, holes, N, H, W, C,
                                                workspace, stream);
}

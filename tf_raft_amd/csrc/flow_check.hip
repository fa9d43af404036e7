// Where a predicted vector can be trusted (no reference counterpart): the backward warp of an image by a
// flow, and the forward-backward consistency test of two flows, one launch each.
//
//   raft_warp_f32 / raft_warp_u8_f32   dst[n, y, x, c] = src[n, :, :, c] sampled at (x + u, y + v), zero outside the frame
//   raft_flow_consistency_f32          occluded = !(in frame && |f + s|^2 <= alpha * (|f|^2 + |s|^2) + beta), s the OTHER flow
//                                      sampled at (x + u, y + v); both directions in one launch (Meister et al. 2018, UnFlow)
//   raft_flow_visibility_f32           the same test on the 2N flows of a bidirectional training step, as the mask of its loss:
//                                      visible = mask && !(apply && occluded), and the occluded share
//
// Both share one definition of the sample.  For the pixel at integer (x, y) with vector (u, v): sx = float(x) + u and
// sy = float(y) + v, ONE float32 addition each; the pixel is in frame iff 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails);
// x0 = floor(sx), x1 = min(x0 + 1, W - 1), a = sx - x0 (exact), likewise y0, y1, b, and the value is
//     (1 - b) * ((1 - a) * g[y0, x0] + a * g[y0, x1]) + b * ((1 - a) * g[y1, x0] + a * g[y1, x1])
// with every product and sum rounded on its own (contraction is switched off for this file).  This is ordinary bilinear
// interpolation, NOT the reference's bilinear_sampler (corr.py:28-69), whose ceil / floor weights vanish at integer coordinates.
//
// Both kernels are gathers bound by memory with no reuse worth staging: one thread per pixel, pixels of an image numbered along
// its rows, so a wave reads 64 consecutive flow vectors as one 512-byte run of float2 and writes its outputs as runs; the four
// taps of neighbouring lanes under a smooth flow are neighbours too.  blockIdx.y walks the images (and, for the consistency
// test, the two directions: slice n + N * d is image n of direction d).  No atomics, no memset, every output element is written
// exactly once.  Tap indices are clamped into the frame whatever the flow holds.  Measured at (4, 1080, 1920) (docs/NOTEBOOK.md
// section 21): a thread that owns four consecutive pixels and stores its mask bytes as one word is SLOWER (109 against 76 us: a
// wave's gathers then span four times the addresses), so a thread owns one pixel; reading the two taps of a row as one 16-byte
// load is faster (71 us) and is what the consistency test does.
#include "common.h"

#pragma clang fp contract(off)

#include "flow_sample.h"      // Taps, flow_taps, bilinear: shared with photometric_loss.hip
#include "loss_common.h"      // the deterministic reduction of raft_flow_visibility_f32's count

namespace {

constexpr int kFlowCheckThreads = 256;

// CT > 0: the channel count at compile time (the taps of all channels are issued together); CT == 0: any C
template <typename S, int CT>
__global__ void __launch_bounds__(kFlowCheckThreads) warp_kernel(const S *__restrict__ src, const float2 *__restrict__ flow,
                                                                 float *__restrict__ dst, uint8_t *__restrict__ inside, int N, int H,
                                                                 int W, int C) {
    const int HW = H * W;
    const int p = (int)blockIdx.x * kFlowCheckThreads + (int)threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    const int Cn = CT > 0 ? CT : C;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW;
        const Taps t = flow_taps(x, y, flow[base + p], H, W);
        const S *g = src + base * Cn;
        float *out = dst + (base + p) * Cn;
        if (CT > 0) {
            float v[CT > 0 ? CT : 1][4];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                v[c][0] = (float)g[(int64_t)t.o00 * CT + c];
                v[c][1] = (float)g[(int64_t)t.o01 * CT + c];
                v[c][2] = (float)g[(int64_t)t.o10 * CT + c];
                v[c][3] = (float)g[(int64_t)t.o11 * CT + c];
            }
#pragma unroll
            for (int c = 0; c < CT; ++c) out[c] = t.in ? bilinear(t, v[c][0], v[c][1], v[c][2], v[c][3]) : 0.f;
        } else {
            for (int c = 0; c < Cn; ++c) {
                const float g00 = (float)g[(int64_t)t.o00 * Cn + c], g01 = (float)g[(int64_t)t.o01 * Cn + c];
                const float g10 = (float)g[(int64_t)t.o10 * Cn + c], g11 = (float)g[(int64_t)t.o11 * Cn + c];
                out[c] = t.in ? bilinear(t, g00, g01, g10, g11) : 0.f;
            }
        }
        if (inside != nullptr) inside[base + p] = t.in ? 1 : 0;
    }
}

// One pixel of the test: the image's own flow vector f at (x, y) against `other` (the other direction's flow of the same image).
// PAIR: the two taps of a row come as ONE 16-byte load (sample_flow, flow_sample.h); needs W >= 2.  The comparison itself is
// flows_disagree, which flow_track.hip applies to a tracked point.
template <bool PAIR>
__device__ __forceinline__ uint32_t occluded_at(const float2 *__restrict__ other, float2 f, int x, int y, int H, int W, float alpha,
                                                 float beta) {
    const Taps t = flow_taps(x, y, f, H, W);
    const float2 s = sample_flow<PAIR>(other, t);
    return (t.in && !flows_disagree(f, s, alpha, beta)) ? 0u : 1u;      // (a NaN anywhere: occluded)
}

template <bool PAIR>
__global__ void __launch_bounds__(kFlowCheckThreads) flow_consistency_kernel(const float2 *__restrict__ flow_a,
                                                                             const float2 *__restrict__ flow_b,
                                                                             uint8_t *__restrict__ occluded_a,
                                                                             uint8_t *__restrict__ occluded_b, int N, int H, int W,
                                                                             int slices, float alpha, float beta) {
    const int HW = H * W;
    const int p = (int)blockIdx.x * kFlowCheckThreads + (int)threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    for (int s = blockIdx.y; s < slices; s += gridDim.y) {
        const bool second = s >= N;                  // wave-uniform: direction b is the same test with the roles swapped
        const int64_t base = (int64_t)(second ? s - N : s) * HW;
        const float2 *own = (second ? flow_b : flow_a) + base;
        const float2 *other = (second ? flow_a : flow_b) + base;
        (second ? occluded_b : occluded_a)[base + p] = (uint8_t)occluded_at<PAIR>(other, own[p], x, y, H, W, alpha, beta);
    }
}

// The in-step form of the test: the 2N flows of a bidirectional training step in ONE tensor, slice s
// against slice s + N (s < N) or s - N, the result inverted and ANDed with the caller's mask, and the occluded pixels counted.
// The same one-thread-per-pixel walk as above; where the record grid is smaller than the picture a workgroup strides over
// 256-pixel runs, so a wave still reads consecutive vectors.  The count is a per-thread float64 (exact for integers), one
// record per workgroup.  The final launch reads the records as rows of kVisibilityColumns and lets raft_sum_records add the
// columns side by side, 16 records per thread instead of 1024 behind one another in one (docs/NOTEBOOK.md section 30);
// workgroup (0, 0) zeroes the tail of the last row, so every record that is read was written by this launch.
constexpr int kVisibilityRecords = 1024;
constexpr int kVisibilityColumns = 64;
static_assert(kVisibilityRecords % kVisibilityColumns == 0 && kVisibilityColumns <= 64, "rows of records, one column per final thread");

template <bool PAIR>
__global__ void __launch_bounds__(kFlowCheckThreads) flow_visibility_kernel(const float2 *__restrict__ flows,
                                                                            const uint8_t *__restrict__ mask,
                                                                            uint8_t *__restrict__ visible, int N, int H, int W,
                                                                            float alpha, float beta, int apply,
                                                                            double *__restrict__ part) {
    const int HW = H * W;
    double acc[1] = {0.0};
    for (int s = blockIdx.y; s < 2 * N; s += gridDim.y) {
        const int64_t base = (int64_t)s * HW;
        const float2 *own = flows + base;
        const float2 *other = flows + (int64_t)(s >= N ? s - N : s + N) * HW;      // wave-uniform
        for (int64_t q = (int64_t)blockIdx.x * kFlowCheckThreads + threadIdx.x; q < HW; q += (int64_t)gridDim.x * kFlowCheckThreads) {
            const int p = (int)q, y = p / W, x = p - y * W;
            const uint32_t occ = occluded_at<PAIR>(other, own[p], x, y, H, W, alpha, beta);
            acc[0] += (double)occ;
            if (visible != nullptr) {
                const bool use = mask == nullptr || mask[base + p] != 0;
                visible[base + p] = (use && !(apply && occ)) ? 1 : 0;
            }
        }
    }
    raft_block_sum_store(acc, part);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < kVisibilityColumns) {
        const int nparts = (int)(gridDim.x * gridDim.y), tail = nparts + (int)threadIdx.x;      // (at most kVisibilityRecords records)
        if (tail < (nparts + kVisibilityColumns - 1) / kVisibilityColumns * kVisibilityColumns) part[tail] = 0.0;
    }
}

__global__ void __launch_bounds__(64) flow_visibility_final_kernel(const double *__restrict__ part, int rows, double total,
                                                                   float *__restrict__ occluded_fraction) {
    __shared__ double tot[kVisibilityColumns];
    raft_sum_records(part, rows, tot);
    if (threadIdx.x == 0) {
        double count = 0.0;
        for (int k = 0; k < kVisibilityColumns; ++k) count += tot[k];
        occluded_fraction[0] = (float)(count / total);
    }
}

// what both entries ask of their sizes: positive, W * C in an int, fewer than 2^31 elements in the largest tensor
int flow_check_sizes(int N, int H, int W, int C) {
    RAFT_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)W * C <= 0x7fffffff, RAFT_E_SHAPE);
    const int64_t limit = ((int64_t)1 << 31) - 1, per = C > 2 ? C : 2;
    RAFT_REQUIRE((int64_t)N <= limit / H && (int64_t)N * H <= limit / W && (int64_t)N * H * W <= limit / per, RAFT_E_SHAPE);
    return RAFT_OK;
}

dim3 flow_check_grid(int H, int W, int64_t slices) {
    return dim3((unsigned)(((int64_t)H * W + kFlowCheckThreads - 1) / kFlowCheckThreads), (unsigned)(slices < 65535 ? slices : 65535));
}

template <typename S>
int warp(const S *src, const float *flow, float *dst, uint8_t *inside, int N, int H, int W, int C, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(dst);
    RAFT_TRY(flow_check_sizes(N, H, W, C));
    RAFT_REQUIRE((((uintptr_t)flow) & 7u) == 0, RAFT_E_ALIGN);      // read as float2
    const dim3 grid = flow_check_grid(H, W, N);
    const float2 *f = (const float2 *)flow;
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: warp_kernel<S, 1><<<grid, kFlowCheckThreads, 0, s>>>(src, f, dst, inside, N, H, W, C); break;
        case 2: warp_kernel<S, 2><<<grid, kFlowCheckThreads, 0, s>>>(src, f, dst, inside, N, H, W, C); break;
        case 3: warp_kernel<S, 3><<<grid, kFlowCheckThreads, 0, s>>>(src, f, dst, inside, N, H, W, C); break;
        case 4: warp_kernel<S, 4><<<grid, kFlowCheckThreads, 0, s>>>(src, f, dst, inside, N, H, W, C); break;
        default: warp_kernel<S, 0><<<grid, kFlowCheckThreads, 0, s>>>(src, f, dst, inside, N, H, W, C); break;
    }
    return raft_launch_status();
}

}   // namespace

extern "C" int raft_warp_f32(const float *src, const float *flow, float *dst, uint8_t *inside, int N, int H, int W, int C,
                             void *stream) {
    return warp<float>(src, flow, dst, inside, N, H, W, C, stream);
}

extern "C" int raft_warp_u8_f32(const uint8_t *src, const float *flow, float *dst, uint8_t *inside, int N, int H, int W, int C,
                                void *stream) {
    return warp<uint8_t>(src, flow, dst, inside, N, H, W, C, stream);
}

extern "C" int raft_flow_consistency_f32(const float *flow_a, const float *flow_b, uint8_t *occluded_a, uint8_t *occluded_b, int N,
                                         int H, int W, float alpha, float beta, void *stream) {
    RAFT_REQUIRE_PTR(flow_a);
    RAFT_REQUIRE_PTR(flow_b);
    RAFT_REQUIRE_PTR(occluded_a);
    RAFT_TRY(flow_check_sizes(N, H, W, 2));
    RAFT_REQUIRE(alpha >= 0.f && alpha <= 3.402823466e38f && beta >= 0.f && beta <= 3.402823466e38f, RAFT_E_SHAPE);   // (a NaN fails)
    RAFT_REQUIRE(((((uintptr_t)flow_a) | ((uintptr_t)flow_b)) & 7u) == 0, RAFT_E_ALIGN);      // read as float2
    const int slices = occluded_b != nullptr ? 2 * N : N;
    const dim3 grid = flow_check_grid(H, W, slices);
    hipStream_t s = (hipStream_t)stream;
    const float2 *fa = (const float2 *)flow_a, *fb = (const float2 *)flow_b;
    if (W >= 2)
        flow_consistency_kernel<true><<<grid, kFlowCheckThreads, 0, s>>>(fa, fb, occluded_a, occluded_b, N, H, W, slices, alpha, beta);
    else
        flow_consistency_kernel<false><<<grid, kFlowCheckThreads, 0, s>>>(fa, fb, occluded_a, occluded_b, N, H, W, slices, alpha, beta);
    return raft_launch_status();
}

extern "C" int64_t raft_flow_visibility_workspace_doubles(void) { return kVisibilityRecords; }

extern "C" int raft_flow_visibility_f32(const float *flows, const uint8_t *mask, uint8_t *visible, float *occluded_fraction, int N,
                                        int H, int W, float alpha, float beta, int apply, double *workspace, void *stream) {
    RAFT_REQUIRE_PTR(flows);
    RAFT_REQUIRE_PTR(occluded_fraction);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(N > 0 && N < (1 << 29), RAFT_E_SHAPE);              // (2 * N below stays an int)
    RAFT_TRY(flow_check_sizes(2 * N, H, W, 2));
    RAFT_REQUIRE(alpha >= 0.f && alpha <= 3.402823466e38f && beta >= 0.f && beta <= 3.402823466e38f, RAFT_E_SHAPE);   // (a NaN fails)
    RAFT_REQUIRE(apply == 0 || apply == 1, RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)flows) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);      // read as float2; doubles
    const int64_t HW = (int64_t)H * W;
    const dim3 grid = raft_record_grid(2 * N, HW, kVisibilityRecords);
    hipStream_t s = (hipStream_t)stream;
    const float2 *f = (const float2 *)flows;
    if (W >= 2)
        flow_visibility_kernel<true><<<grid, kFlowCheckThreads, 0, s>>>(f, mask, visible, N, H, W, alpha, beta, apply, workspace);
    else
        flow_visibility_kernel<false><<<grid, kFlowCheckThreads, 0, s>>>(f, mask, visible, N, H, W, alpha, beta, apply, workspace);
    RAFT_TRY(raft_launch_status());
    const int rows = ((int)(grid.x * grid.y) + kVisibilityColumns - 1) / kVisibilityColumns;
    flow_visibility_final_kernel<<<1, 64, 0, s>>>(workspace, rows, (double)(2 * N) * (double)HW, occluded_fraction);
    return raft_launch_status();
}

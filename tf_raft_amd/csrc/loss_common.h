// What the loss and metric kernels share (metrics.hip, photometric_loss.hip, census_loss.hip; internal): the deterministic
// reduction, the weights of the sequence, and the host-side checks of their entry points.  The wave helpers at the top also
// serve augment.hip, flow_viz.hip and backward.hip.
//
// The reduction, stated here once.  Every thread accumulates its grid-stride share in float64.  A 256-thread workgroup then
// adds its values with raft_block_sum_store: an xor butterfly over each wave (offsets 32, 16, ... 1), the four wave totals
// through LDS, ((s0 + s1) + s2) + s3, into ONE record of NV doubles, record number blockIdx.y * gridDim.x + blockIdx.x.  A
// second, one-workgroup kernel adds the records in index order with raft_sum_records and normalises.  No atomics and no
// memset: every record that is read was written by the launch before it, and the same input gives the same bits.  The
// number of records is bounded by a grid-stride loop in the first kernel (raft_record_grid for the image-shaped ones).
// Changing any association here changes the bits of every loss and metric: tests/test_gpu_loss_parent_bits.py pins them,
// and docs/NOTEBOOK.md section 28 has what the helpers' form means to the compiler.
#pragma once

#include "common.h"

// ---------------------------------------------------------------- wave helpers (double, float, unsigned)
// Sum over the 64 lanes, in every lane: the xor butterfly with offsets 32, 16, ... 1.  raft_wave_sum_each sends several
// values through it side by side, in place (the order the kernels that reduce a pair were written in: the compiler's
// schedule depends on it, the results do not).
template <typename... T>
__device__ __forceinline__ void raft_wave_sum_each(T &...v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ((v += __shfl_xor(v, o, 64)), ...);
}

template <typename T>
__device__ __forceinline__ T raft_wave_sum(T v) {
    raft_wave_sum_each(v);
    return v;
}

__device__ __forceinline__ float raft_wave_max(float m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

// ---------------------------------------------------------------- workgroup step and final sum
// The NV per-thread sums of a 256-thread workgroup -> its record part[record][NV].  All threads of the workgroup call it.
// GRID_2D = false is the blockIdx.y == 0 case for kernels launched on a 1-D grid (they then do not ask for blockIdx.y).
template <bool GRID_2D = true, int NV>
__device__ __forceinline__ void raft_block_sum_store(double (&acc)[NV], double *__restrict__ part) {
    __shared__ double sh[4][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = raft_wave_sum(acc[k]);
        if (lane == 0) sh[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int64_t record = GRID_2D ? (int64_t)blockIdx.y * gridDim.x + blockIdx.x : (int64_t)blockIdx.x;
        part[record * NV + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
    }
}

// Thread k < NV adds column k of the records in index order into tot[k]; behind the barrier every thread of the (one)
// workgroup sees the totals when `tot` is the caller's __shared__ array.
template <int NV>
__device__ __forceinline__ void raft_sum_records(const double *__restrict__ part, int nparts, double (&tot)[NV]) {
    if (threadIdx.x < NV) {
        double s = 0.0;
        for (int r = 0; r < nparts; ++r) s += part[(int64_t)r * NV + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

// ---------------------------------------------------------------- the weights of the sequence
constexpr int kMaxPredictions = 64;

struct PredWeights {
    float w[kMaxPredictions];
};

// w_i = gamma ** (n - i - 1) (reference losses.py:17) by repeated multiplication in double, then (float)(w_i * num / den):
// ONE rounding to fp32.  The losses take the defaults (w_i * 1.0 / 1.0 is w_i); the gradient of sequence_loss folds its
// upstream / (2 * npix) in as num / den, multiplied first and divided second.
static inline PredWeights raft_pred_weights(double gamma, int n, double num = 1.0, double den = 1.0) {
    PredWeights pw = {};
    for (int i = 0; i < n; ++i) {
        double w = 1.0;
        for (int k = 0; k < n - i - 1; ++k) w *= gamma;
        pw.w[i] = (float)(w * num / den);
    }
    return pw;
}

// ---------------------------------------------------------------- host checks and the record grid
static inline bool raft_finite_nonneg(double v) { return v >= 0.0 && v <= 3.402823466e38; }      // (a NaN fails)

static inline bool raft_finite_f32(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }

// n predictions of (B, H, W) images with B*H*W*3 below 2^31: the kernels index an image's pixels and channels with int
static inline bool raft_loss_shape_ok(int n, int B, int H, int W) {
    if (!(n > 0 && B > 0 && H > 0 && W > 0)) return false;
    const int64_t limit = ((int64_t)1 << 31) - 1;
    return (int64_t)B <= limit / H && (int64_t)B * H <= limit / W && (int64_t)B * H * W <= limit / 3;
}

// Grid of a kernel whose blockIdx.y walks B images and whose blockIdx.x walks the HW pixels of an image, 256 per workgroup,
// both with grid-stride loops: at most max_records workgroups, images first.
static inline dim3 raft_record_grid(int B, int64_t HW, int max_records) {
    const int gy = B < max_records ? B : max_records;
    const int64_t blocks = (HW + 255) / 256, cap = max_records / gy;
    return dim3((unsigned)(blocks < cap ? blocks : cap), (unsigned)gy);
}

// ---------------------------------------------------------------- the supervised losses' pixel test
// valid' = valid & (|flow_gt| < max_flow), reference losses.py:11 / 28: x*x + y*y, then sqrt, each rounded on its own
__device__ __forceinline__ bool pixel_valid(float2 g, unsigned char v, float max_flow) {
#pragma clang fp contract(off)
    const float mag = sqrtf(g.x * g.x + g.y * g.y);
    return v != 0 && mag < max_flow;
}

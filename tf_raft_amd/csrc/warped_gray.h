// What the windowed data terms of the self-supervised loss share (census_loss.hip, ssim_loss.hip; internal; DESIGN.md sections 18
// and 19): both compare windows of g1 = gray(image1) with windows of the warped gray w_i of image2 under prediction i, in three
// launches.  Here, once: the gray value, the warp launch that fills the workspace planes g1 | w_i | M_i, the arguments of a term's
// sweep kernel, the write of a pixel's gradient from the sweep's sum, the final kernel, the workspace and the entries' host
// checks.  A term's own file holds its window arithmetic and its sweep kernel.
//
//   gray(c) = (0.299f*R + 0.587f*G) + 0.114f*B on 0..255
//   w_i(x)  = inside ? bilinear(taps of flow_sample.h under p_i, gray(image2)) : 0
//   interior(x, y) = RADIUS <= x <= W-1-RADIUS && RADIUS <= y <= H-1-RADIUS,      M_i = mask && inside_i && interior (as 1.f / 0.f)
//   term_i = sum_y M_i(y) * D(y) / (B*H*W),     out2 = {add_to + weight * sum_i w_i term_i, term_{n-1}},  w_i = (float)gamma^(n-i-1)
//   d term_i / d w(y) = -S(y) * inv_norm with S the sweep's sum over the pixel's window,  d/du = that * dW/du, d/dv = that * dW/dv
//
// As flow_sample.h: the including file switches contraction off at file scope first.
#pragma once

#include "loss_common.h"
#include "flow_sample.h"

namespace {

constexpr int kThreads = 256;         // (what raft_block_sum_store and raft_record_grid take a workgroup to be)
constexpr int kMaxRecords = 768;      // partial records of a sweep: 3 workgroups per CU, what the census sweep's 49 KiB of LDS let a CU hold
constexpr int kVals = 2;              // sum_i w_i * TERM_i, TERM_{n-1} (sums before normalisation)
constexpr int64_t kRecordBytes = (int64_t)kMaxRecords * kVals * (int64_t)sizeof(double);

__device__ __forceinline__ float gray(const float *__restrict__ c) { return (0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2]; }

// the four taps of gray(image2) of one image for a sample
__device__ __forceinline__ void gray_taps(const float *__restrict__ i2, const Taps &t, float (&q)[4]) {
    q[0] = gray(i2 + (int64_t)t.o00 * 3);
    q[1] = gray(i2 + (int64_t)t.o01 * 3);
    q[2] = gray(i2 + (int64_t)t.o10 * 3);
    q[3] = gray(i2 + (int64_t)t.o11 * 3);
}

// ---------------------------------------------------------------- launch 1: the planes
// One thread per pixel and prediction: g1 once, and per prediction w_i and M_i.
template <int RADIUS, bool MASK>
__global__ void __launch_bounds__(kThreads) warped_gray_kernel(const float *__restrict__ image1, const float *__restrict__ image2,
                                                               const uint8_t *__restrict__ mask, const float2 *__restrict__ preds,
                                                               int64_t stride2, int B, int H, int W, float *__restrict__ g1,
                                                               float *__restrict__ wv, float *__restrict__ valid) {
    const int HW = H * W;
    const int i = blockIdx.z;
    const int64_t npix = (int64_t)B * HW;
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW;
        const float *i2 = image2 + base * 3;
        for (int p = (int)blockIdx.x * kThreads + (int)threadIdx.x; p < HW; p += (int)gridDim.x * kThreads) {
            const int y = p / W, x = p - y * W;
            if (i == 0) g1[base + p] = gray(image1 + (base + p) * 3);
            const Taps t = flow_taps(x, y, preds[(int64_t)i * stride2 + base + p], H, W);
            float q[4];
            gray_taps(i2, t, q);
            const float w2 = bilinear(t, q[0], q[1], q[2], q[3]);
            const bool use = MASK ? mask[base + p] != 0 : true;
            const bool interior = x >= RADIUS && x <= W - 1 - RADIUS && y >= RADIUS && y <= H - 1 - RADIUS;
            wv[(int64_t)i * npix + base + p] = t.in ? w2 : 0.f;
            valid[(int64_t)i * npix + base + p] = (use && t.in && interior) ? 1.f : 0.f;
        }
    }
}

// ---------------------------------------------------------------- launch 2: what a term's sweep kernel takes and how it writes
struct SweepArgs {
    const float *image2;
    const float2 *preds;
    int64_t stride2, npix;
    int n_pred, H, W;
    float scale;                      // upstream * the term's weight
    float inv_norm;                   // 1 / (pairs or windows per pixel * B*H*W): census 1 / (48*npix), SSIM 1 / (18*npix)
    int accumulate;
    const float *g1, *wv, *valid;     // valid: M as 1.f / 0.f, so that a window row of it loads like a row of w
    float2 *d_preds;
};

// upstream * weight * w_i * d term_i / d (u, v) of one pixel from its S: the taps of g2 are gathered again (cheaper than a second
// and third plane per prediction in the workspace)
__device__ __forceinline__ void store_grad(const SweepArgs &a, int x, int y, int64_t at, int i, float wi, float S) {
    const int64_t n_base = at - ((int64_t)y * a.W + x);
    const Taps t = flow_taps(x, y, a.preds[(int64_t)i * a.stride2 + at], a.H, a.W);
    float q[4];
    gray_taps(a.image2 + n_base * 3, t, q);
    const float du = t.in ? bilinear_du(t, q[0], q[1], q[2], q[3]) : 0.f;
    const float dv = t.in ? bilinear_dv(t, q[0], q[1], q[2], q[3]) : 0.f;
    const float gw = 0.f - (a.scale * wi) * (S * a.inv_norm);
    float2 o = make_float2(gw * du, gw * dv);
    float2 *dst = a.d_preds + (int64_t)i * a.stride2 + at;
    if (a.accumulate) {
        const float2 was = *dst;
        o.x = was.x + o.x;
        o.y = was.y + o.y;
    }
    *dst = o;
}

// ---------------------------------------------------------------- launch 3: the records of the sweep -> out2
__global__ void __launch_bounds__(64) warped_final_kernel(const double *__restrict__ part, int nparts, double inv, double weight,
                                                          const float *add_to, float *out2) {
    __shared__ double tot[kVals];
    raft_sum_records(part, nparts, tot);
    if (threadIdx.x == 0) {
        const double before = add_to != nullptr ? (double)add_to[0] : 0.0;      // (read before out2 is written: they may be one address)
        out2[0] = (float)(before + weight * (tot[0] * inv));
        out2[1] = (float)(tot[1] * inv);
    }
}

// ---------------------------------------------------------------- host side of an entry
// records | g1: B*H*W floats | w: n*B*H*W floats | M: n*B*H*W floats
static inline int64_t warped_workspace_bytes(int n_predictions, int B, int H, int W) {
    if (!raft_loss_shape_ok(n_predictions, B, H, W) || n_predictions > kMaxPredictions) return 0;
    const int64_t npix = (int64_t)B * H * W;
    return kRecordBytes + 4 * npix + 8 * npix * n_predictions;
}

struct WarpedPlanes {
    double *part;
    float *g1, *wv, *valid;
};

static inline WarpedPlanes warped_planes(void *workspace, int64_t npix, int n_predictions) {
    WarpedPlanes p;
    p.part = (double *)workspace;
    p.g1 = (float *)((char *)workspace + kRecordBytes);
    p.wv = p.g1 + npix;
    p.valid = p.wv + npix * n_predictions;
    return p;
}

// The checks of raft_census_loss_f32 and raft_ssim_loss_f32 (include/raft_hip.h), in the order that decides which code a call
// with several faults gets.  `weight` is census_weight or ssim_weight.
static inline int warped_check_args(const float *image1, const float *image2, const float *preds, int64_t pred_stride,
                                    int n_predictions, int B, int H, int W, double gamma, float weight, float upstream,
                                    const float *out2, const float *d_preds, int accumulate, const void *workspace) {
    RAFT_REQUIRE_PTR(image1);
    RAFT_REQUIRE_PTR(image2);
    RAFT_REQUIRE_PTR(preds);
    RAFT_REQUIRE_PTR(out2);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(raft_loss_shape_ok(n_predictions, B, H, W), RAFT_E_SHAPE);
    RAFT_REQUIRE(pred_stride >= 2 * ((int64_t)B * H * W), RAFT_E_SHAPE);
    RAFT_REQUIRE(n_predictions <= kMaxPredictions && (pred_stride & 1) == 0, RAFT_E_UNSUPPORTED);
    RAFT_REQUIRE(raft_finite_nonneg(gamma) && raft_finite_nonneg(weight), RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_finite_f32(upstream), RAFT_E_SHAPE);
    RAFT_REQUIRE(accumulate == 0 || accumulate == 1, RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)preds) | ((uintptr_t)d_preds) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);   // float2 / double
    return RAFT_OK;
}

// The sweep's arguments of a checked call; `per_pixel` = 48 (pairs) or 18 (twice the nine windows): inv_norm is computed in double
// and rounded once.
static inline SweepArgs sweep_args(const float *image2, const float *preds, int64_t pred_stride, int n_predictions, int B, int H, int W,
                                   float scale, double per_pixel, float *d_preds, int accumulate, const WarpedPlanes &p) {
    SweepArgs a;
    a.image2 = image2, a.preds = (const float2 *)preds, a.stride2 = pred_stride / 2, a.npix = (int64_t)B * H * W;
    a.n_pred = n_predictions, a.H = H, a.W = W;
    a.scale = scale;
    a.inv_norm = (float)(1.0 / (per_pixel * (double)a.npix));
    a.accumulate = accumulate;
    a.g1 = p.g1, a.wv = p.wv, a.valid = p.valid, a.d_preds = (float2 *)d_preds;
    return a;
}

// The warp launch: min(blocks, 1024) x min(B, 64) x n workgroups, every loop of the kernel grid-strided.
template <int RADIUS>
static inline int launch_warped_gray(const float *image1, const uint8_t *mask, const SweepArgs &a, int B, const WarpedPlanes &p,
                                     hipStream_t s) {
    const int64_t blocks = ((int64_t)a.H * a.W + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)(B < 64 ? B : 64), (unsigned)a.n_pred);
    if (mask != nullptr)
        warped_gray_kernel<RADIUS, true><<<grid, kThreads, 0, s>>>(image1, a.image2, mask, a.preds, a.stride2, B, a.H, a.W, p.g1, p.wv, p.valid);
    else
        warped_gray_kernel<RADIUS, false><<<grid, kThreads, 0, s>>>(image1, a.image2, mask, a.preds, a.stride2, B, a.H, a.W, p.g1, p.wv, p.valid);
    return raft_launch_status();
}

// The final launch behind a sweep on `grid`.
static inline int launch_warped_final(const WarpedPlanes &p, dim3 grid, int64_t npix, float weight, const float *add_to, float *out2,
                                      hipStream_t s) {
    warped_final_kernel<<<1, 64, 0, s>>>(p.part, (int)(grid.x * grid.y), 1.0 / (double)npix, (double)weight, add_to, out2);
    return raft_launch_status();
}

}   // namespace

// Self-supervised sequence loss (no reference counterpart): a photometric term (frame 2 sampled under the
// predicted flow against frame 1, Charbonnier penalty) plus an edge-aware first-order smoothness term, summed over the n
// predictions of the loop with the weights gamma^(n-i-1) of sequence_loss, and d loss / d prediction_i.  ONE launch computes
// the value and the gradient: a training step needs both and they share the four gathers of every sample.
//
//   s = 1/255, rho(d) = sqrtf(d*d + eps*eps) (eps*eps rounded once to float32), w_i = (float)gamma^(n-i-1)
//   ph_i = sum mask * inside * rho(s * (image2 sampled at (x + u, y + v) - image1))_c          / (B*H*W*3)
//   sm_i = [sum wx * rho(p(x+1,y)_k - p(x,y)_k) + sum wy * rho(p(x,y+1)_k - p(x,y)_k)]          / (B*H*W*2)
//          wx(x,y) = expf(-edge_weight * mean_c |s * (image1(x+1,y)_c - image1(x,y)_c)|), wy likewise along y
//   loss = sum_i w_i * (ph_i + smooth_weight * sm_i),   out3 = {loss, ph_{n-1}, sm_{n-1}}
//
// The sample (position, in-frame test, taps, weights a and b) is flow_sample.h's, the one flow_check.hip uses.  `inside` and
// `mask` are constants of the gradient; dW2/du = (1-b)*(g01-g00) + b*(g11-g10), dW2/dv = (1-a)*(g10-g00) + a*(g11-g01) are that
// header's too: the one-sided derivative of the cell the taps come from (zero where x1 == x0).  The smoothness gradient is the adjoint written
// as a gather: with tx = wx*dx/rho(dx), ty = wy*dy/rho(dy),
//   d sm_i / d p(x,y)_k = (-tx(x,y) - ty(x,y) + tx(x-1,y) + ty(x,y-1)) / (B*H*W*2), terms that do not exist dropped.
//
// Mapping: one thread per pixel, pixels of an image numbered along its rows (flow_check.hip measured a thread that owns four
// pixels slower for these gathers); blockIdx.y walks the images; a thread loops over the n predictions.  Everything that does
// not depend on i is loaded or computed once per pixel: image1's three values, the mask byte, and the edge weights at (x,y),
// (x-1,y), (x,y-1).  The five-point flow stencil of a prediction is read through the cache (neighbouring lanes and the rows
// above and below read the same lines; not staged in LDS).  Deterministic: the reduction of loss_common.h, one record of
// kVals sums per workgroup, the number of records bounded by the grid-stride loops.  Every element of d_preds is written
// exactly once.
#include "loss_common.h"

#pragma clang fp contract(off)

#include "flow_sample.h"

namespace {

constexpr int kThreads = 256;         // (what raft_block_sum_store and raft_record_grid take a workgroup to be)
constexpr int kMaxRecords = 1024;     // partial records (4 workgroups per CU)
constexpr int kVals = 4;              // sum_i w_i * PH_i, sum_i w_i * SM_i, PH_{n-1}, SM_{n-1} (sums before normalisation)

struct LossConsts {
    float smooth_weight, edge_weight, eps2, upstream;
    float inv3, inv2;                 // 1 / (B*H*W*3), 1 / (B*H*W*2)
};

__device__ __forceinline__ float rho(float d, float eps2) { return sqrtf(d * d + eps2); }

// expf(-edge_weight * mean_c |s * (q_c - p_c)|)
__device__ __forceinline__ float edge_weight_of(const float (&p)[3], const float *__restrict__ q, float edge_weight) {
    const float s = 1.0f / 255.0f;
    const float m = ((fabsf(s * (q[0] - p[0])) + fabsf(s * (q[1] - p[1]))) + fabsf(s * (q[2] - p[2]))) / 3.0f;
    return expf(-edge_weight * m);
}

template <bool GRAD, bool MASK>
__global__ void __launch_bounds__(kThreads) photometric_loss_kernel(const float *__restrict__ image1, const float *__restrict__ image2,
                                                                    const uint8_t *__restrict__ mask, const float2 *__restrict__ preds,
                                                                    int64_t stride2, int n_pred, int B, int H, int W, PredWeights pw,
                                                                    LossConsts k, float2 *__restrict__ d_preds,
                                                                    double *__restrict__ part) {
    const int HW = H * W;
    const float s = 1.0f / 255.0f;
    double acc[kVals] = {0.0, 0.0, 0.0, 0.0};
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW;
        const float *i1 = image1 + base * 3, *i2 = image2 + base * 3;
        for (int p = (int)blockIdx.x * kThreads + (int)threadIdx.x; p < HW; p += (int)gridDim.x * kThreads) {
            const int y = p / W, x = p - y * W;
            const bool right = x < W - 1, down = y < H - 1, left = GRAD && x > 0, up = GRAD && y > 0;
            // ---- once per pixel: image1, the mask, the edge weights of the (up to) four differences this pixel takes part in
            float c[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = i1[(int64_t)p * 3 + ch];
            const bool use = MASK ? mask[base + p] != 0 : true;
            float wx = 0.f, wy = 0.f, wxl = 0.f, wyu = 0.f;
            if (right) wx = edge_weight_of(c, i1 + (int64_t)(p + 1) * 3, k.edge_weight);
            if (down) wy = edge_weight_of(c, i1 + (int64_t)(p + W) * 3, k.edge_weight);
            if (left) {
                float q[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) q[ch] = i1[(int64_t)(p - 1) * 3 + ch];
                wxl = edge_weight_of(q, c, k.edge_weight);            // wx(x-1, y): image1(x, y) - image1(x-1, y)
            }
            if (up) {
                float q[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) q[ch] = i1[(int64_t)(p - W) * 3 + ch];
                wyu = edge_weight_of(q, c, k.edge_weight);
            }
            // ---- per prediction
            for (int i = 0; i < n_pred; ++i) {
                const float2 *f = preds + (int64_t)i * stride2 + base;
                const float2 f0 = f[p];
                const Taps t = flow_taps(x, y, f0, H, W);
                float g[3][4];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    g[ch][0] = i2[(int64_t)t.o00 * 3 + ch];
                    g[ch][1] = i2[(int64_t)t.o01 * 3 + ch];
                    g[ch][2] = i2[(int64_t)t.o10 * 3 + ch];
                    g[ch][3] = i2[(int64_t)t.o11 * 3 + ch];
                }
                const float2 zero = make_float2(0.f, 0.f);
                const float2 fr = right ? f[p + 1] : zero, fd = down ? f[p + W] : zero;
                const float2 fl = left ? f[p - 1] : zero, fu = up ? f[p - W] : zero;
                // photometric
                const bool on = use && t.in;
                float ph = 0.f, gu = 0.f, gv = 0.f;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float w2 = bilinear(t, g[ch][0], g[ch][1], g[ch][2], g[ch][3]);
                    const float d = s * (w2 - c[ch]);
                    const float r = rho(d, k.eps2);
                    ph += r;
                    if (GRAD) {
                        const float q = (d / r) * s;
                        const float du = bilinear_du(t, g[ch][0], g[ch][1], g[ch][2], g[ch][3]);
                        const float dv = bilinear_dv(t, g[ch][0], g[ch][1], g[ch][2], g[ch][3]);
                        gu += q * du;
                        gv += q * dv;
                    }
                }
                ph = on ? ph : 0.f;
                // smoothness: the two differences this pixel owns
                const float dxu = fr.x - f0.x, dxv = fr.y - f0.y, dyu = fd.x - f0.x, dyv = fd.y - f0.y;
                const float rxu = rho(dxu, k.eps2), rxv = rho(dxv, k.eps2), ryu = rho(dyu, k.eps2), ryv = rho(dyv, k.eps2);
                const float sm = wx * (rxu + rxv) + wy * (ryu + ryv);        // (an edge weight that does not exist is 0)
                const double wi = (double)pw.w[i];
                acc[0] += wi * (double)ph;
                acc[1] += wi * (double)sm;
                if (i == n_pred - 1) {
                    acc[2] += (double)ph;
                    acc[3] += (double)sm;
                }
                if (GRAD) {
                    // -tx(x, y) - ty(x, y) of the owned differences + tx(x-1, y) + ty(x, y-1) of the left and upper neighbours';
                    // a term that does not exist has the edge weight 0 (and a finite difference: its neighbour reads as 0)
                    const float lu = f0.x - fl.x, lv = f0.y - fl.y, uu = f0.x - fu.x, uv = f0.y - fu.y;
                    const float su = (((0.f - wx * (dxu / rxu)) - wy * (dyu / ryu)) + wxl * (lu / rho(lu, k.eps2))) + wyu * (uu / rho(uu, k.eps2));
                    const float sv = (((0.f - wx * (dxv / rxv)) - wy * (dyv / ryv)) + wxl * (lv / rho(lv, k.eps2))) + wyu * (uv / rho(uv, k.eps2));
                    gu = on ? gu : 0.f;
                    gv = on ? gv : 0.f;
                    const float scale = k.upstream * pw.w[i];
                    float2 o;
                    o.x = scale * (gu * k.inv3 + k.smooth_weight * (su * k.inv2));
                    o.y = scale * (gv * k.inv3 + k.smooth_weight * (sv * k.inv2));
                    d_preds[(int64_t)i * stride2 + base + p] = o;
                }
            }
        }
    }
    raft_block_sum_store(acc, part);
}

__global__ void __launch_bounds__(64) photometric_loss_final_kernel(const double *__restrict__ part, int nparts, double inv3, double inv2,
                                                                    double smooth_weight, float *__restrict__ out3) {
    __shared__ double tot[kVals];
    raft_sum_records(part, nparts, tot);
    if (threadIdx.x == 0) {
        out3[0] = (float)(tot[0] * inv3 + smooth_weight * (tot[1] * inv2));
        out3[1] = (float)(tot[2] * inv3);
        out3[2] = (float)(tot[3] * inv2);
    }
}

}   // namespace

extern "C" int64_t raft_photometric_loss_workspace_doubles(void) { return (int64_t)kMaxRecords * kVals; }

extern "C" int raft_photometric_loss_f32(const float *image1, const float *image2, const uint8_t *mask, const float *preds,
                                         int64_t pred_stride, int n_predictions, int B, int H, int W, double gamma,
                                         float smooth_weight, float edge_weight, float eps, float upstream, float *out3,
                                         float *d_preds, double *workspace, void *stream) {
    RAFT_REQUIRE_PTR(image1);
    RAFT_REQUIRE_PTR(image2);
    RAFT_REQUIRE_PTR(preds);
    RAFT_REQUIRE_PTR(out3);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(raft_loss_shape_ok(n_predictions, B, H, W), RAFT_E_SHAPE);
    const int64_t npix = (int64_t)B * H * W;
    RAFT_REQUIRE(pred_stride >= 2 * npix, RAFT_E_SHAPE);
    RAFT_REQUIRE(n_predictions <= kMaxPredictions && (pred_stride & 1) == 0, RAFT_E_UNSUPPORTED);
    const float eps2 = eps * eps;                 // rho(0) = sqrtf(eps2) divides the gradient: it must be positive and finite
    RAFT_REQUIRE(eps > 0.f && eps2 > 0.f && eps2 <= 3.402823466e38f, RAFT_E_SHAPE);      // (a NaN fails)
    RAFT_REQUIRE(raft_finite_nonneg(gamma) && raft_finite_nonneg(smooth_weight) && raft_finite_nonneg(edge_weight), RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_finite_f32(upstream), RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)preds) | ((uintptr_t)d_preds) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);   // float2 / double

    const PredWeights pw = raft_pred_weights(gamma, n_predictions);
    LossConsts k;
    k.smooth_weight = smooth_weight, k.edge_weight = edge_weight, k.eps2 = eps2, k.upstream = upstream;
    const double inv3 = 1.0 / ((double)npix * 3.0), inv2 = 1.0 / ((double)npix * 2.0);
    k.inv3 = (float)inv3, k.inv2 = (float)inv2;
    const dim3 grid = raft_record_grid(B, (int64_t)H * W, kMaxRecords);
    hipStream_t s = (hipStream_t)stream;
    const float2 *pr = (const float2 *)preds;
    float2 *dp = (float2 *)d_preds;
    const int64_t stride2 = pred_stride / 2;
#define RAFT_PH_LAUNCH(G, M) \
    photometric_loss_kernel<G, M><<<grid, kThreads, 0, s>>>(image1, image2, mask, pr, stride2, n_predictions, B, H, W, pw, k, dp, workspace)
    if (d_preds != nullptr) {
        if (mask != nullptr) RAFT_PH_LAUNCH(true, true); else RAFT_PH_LAUNCH(true, false);
    } else {
        if (mask != nullptr) RAFT_PH_LAUNCH(false, true); else RAFT_PH_LAUNCH(false, false);
    }
#undef RAFT_PH_LAUNCH
    RAFT_TRY(raft_launch_status());
    photometric_loss_final_kernel<<<1, 64, 0, s>>>(workspace, (int)(grid.x * grid.y), inv3, inv2, (double)smooth_weight, out3);
    return raft_launch_status();
}

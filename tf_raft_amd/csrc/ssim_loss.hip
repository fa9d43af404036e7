// SSIM term of the self-supervised sequence loss (no reference counterpart): the structural-similarity data
// term of ARFlow-style recipes, with d term / d prediction_i.  Definitions (every product and sum rounded on its own):
//
//   gray, g1, g2, w_i(x) = inside ? bilinear(taps of flow_sample.h under p_i, g2) : 0      warped_gray.h's
//   C1 = (0.01f*255.f)^2, C2 = (0.03f*255.f)^2;  interior(z) = 1 <= zx <= W-2 && 1 <= zy <= H-2,  M_i = mask && inside_i && interior
//   over the 3x3 window of z, rows first, x = g1:   mx = (sum x) / 9.f,  mw = (sum w) / 9.f,
//   sxx = (sum (x-mx)*(x-mx)) / 9.f,  sww = (sum (w-mw)*(w-mw)) / 9.f,  sxw = (sum (x-mx)*(w-mw)) / 9.f
//   n1 = (2.f*mx)*mw + C1,  d1 = (mx*mx + mw*mw) + C1,  n2 = 2.f*sxw + C2,  d2 = (sxx + sww) + C2
//   S(z) = (n1*n2) / (d1*d2),   D(z) = (1.f - S(z)) / 2.f
//   ssim_i = sum_z M_i(z) * D(z) / (B*H*W),    out2 = {add_to + ssim_weight * sum_i w_i ssim_i, ssim_{n-1}},  w_i = (float)gamma^(n-i-1)
// d1 >= C1 and d2 >= C2 (the centred sums are not negative): no division comes near zero.
//
// Gradient as a gather.  With r1 = n1/d1, r2 = n2/d2 the derivatives of S by mw, sww (twice) and sxw of a window are
//   A = ((2.f*mx - (2.f*mw)*r1) * r2) / d1,     R = (2.f*r1) / d2,     Q2 = 0.f - R*r2
//   G(y) = sum over z in frame, |z - y|_inf <= 1, rows first, of M(z) ? (A(z) + Q2(z)*(w(y) - mw(z))) + R(z)*(x(y) - mx(z)) : 0
//   d ssim_i / d w(y) = -G(y) / (18*B*H*W),    d/du = that * dwdu(y), d/dv = that * dwdv(y)      (flow_sample.h's dW/du, dW/dv)
// (equal frames at zero flow: r1 = r2 = 1, A = 0 and Q2 = -R exactly, so G is exactly 0 as S is exactly 1).  A window with M = 1 is
// interior, so its nine pixels are in the frame: no window is ever read past a border.
//
// Mapping: the three launches of warped_gray.h, as census_loss.hip.  (1) warped_gray_kernel<1>: g1 once, and per prediction w_i
// and M_i (as 1.f / 0.f), into the workspace.  (2) ssim_sweep_kernel, one thread per pixel looping over the
// predictions.  A pixel whose 5x5 neighbourhood lies in the frame keeps the 25 values of g1 and the mx / sxx of its nine windows in
// registers (they do not depend on the prediction), reads per prediction the 5x5 of w_i and the 3x3 of M_i through the cache and
// forms D and G from them; the pixels nearer the border walk their windows one at a time.  store_grad gathers the four taps of g2
// again for dwdu / dwdv and touches the element of d_preds once.  (3) warped_final_kernel adds the sweep's records and normalises.
// Deterministic: the reduction of loss_common.h.
#include "loss_common.h"

#pragma clang fp contract(off)

#include "warped_gray.h"

namespace {

constexpr float kC1 = (0.01f * 255.f) * (0.01f * 255.f);
constexpr float kC2 = (0.03f * 255.f) * (0.03f * 255.f);

// ---------------------------------------------------------------- one 3x3 window (values rows first)
__device__ __forceinline__ float mean9(const float (&v)[9]) {
    float s = v[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) s = s + v[k];
    return s / 9.f;
}

// (sum (a - ma) * (b - mb)) / 9.f
__device__ __forceinline__ float cov9(const float (&a)[9], float ma, const float (&b)[9], float mb) {
    float s = (a[0] - ma) * (b[0] - mb);
#pragma unroll
    for (int k = 1; k < 9; ++k) s = s + (a[k] - ma) * (b[k] - mb);
    return s / 9.f;
}

struct Coefs {
    float A, Q2, R;
};

// S of a window from its moments and, for the gradient, the derivatives of S by mw, sww (twice) and sxw
template <bool GRAD>
__device__ __forceinline__ float ssim_of_moments(float mx, float sxx, float mw, float sww, float sxw, Coefs &c) {
    const float n1 = (2.f * mx) * mw + kC1;
    const float d1 = (mx * mx + mw * mw) + kC1;
    const float n2 = 2.f * sxw + kC2;
    const float d2 = (sxx + sww) + kC2;
    if (GRAD) {
        const float r1 = n1 / d1, r2 = n2 / d2;
        c.R = (2.f * r1) / d2;
        c.Q2 = 0.f - c.R * r2;
        c.A = ((2.f * mx - (2.f * mw) * r1) * r2) / d1;
    }
    return (n1 * n2) / (d1 * d2);
}

// A window's share of G at one of its pixels with values xy = x(y), wy = w(y)
__device__ __forceinline__ float window_share(const Coefs &c, float xy, float mx, float wy, float mw) {
    return (c.A + c.Q2 * (wy - mw)) + c.R * (xy - mx);
}

__device__ __forceinline__ void ssim_add_value(const SweepArgs &a, const PredWeights &pw, int i, float S, double (&acc)[kVals]) {
    const float D = (1.f - S) / 2.f;
    acc[0] += (double)pw.w[i] * (double)D;
    if (i == a.n_pred - 1) acc[1] += (double)D;
}

// the 3x3 window around p[0] (row pitch W), rows first
__device__ __forceinline__ void load9(const float *__restrict__ p, int W, float (&v)[9]) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) v[(dy + 1) * 3 + dx + 1] = p[dy * W + dx];
}

// Value only: the pixel's own window, where M = 1 (such a pixel is interior: the window is in the frame).
__device__ __forceinline__ void ssim_pixel_value(const SweepArgs &a, const PredWeights &pw, int64_t at, double (&acc)[kVals]) {
    float xs[9], ws[9], mx = 0.f, sxx = 0.f;
    bool have_x = false;
    for (int i = 0; i < a.n_pred; ++i) {
        const int64_t ib = (int64_t)i * a.npix + at;
        if (a.valid[ib] == 0.f) continue;
        if (!have_x) {
            load9(a.g1 + at, a.W, xs);
            mx = mean9(xs);
            sxx = cov9(xs, mx, xs, mx);
            have_x = true;
        }
        load9(a.wv + ib, a.W, ws);
        const float mw = mean9(ws);
        Coefs c;
        const float S = ssim_of_moments<false>(mx, sxx, mw, cov9(ws, mw, ws, mw), cov9(xs, mx, ws, mw), c);
        ssim_add_value(a, pw, i, S, acc);
    }
}

// Value and gradient of a pixel whose 5x5 neighbourhood lies in the frame, all predictions: no tests.  x5 (the neighbourhood of g1)
// and the mx / sxx of the nine windows stay in registers over the predictions.
__device__ __forceinline__ void ssim_pixel_whole(const SweepArgs &a, const PredWeights &pw, int x, int y, int64_t at,
                                                 double (&acc)[kVals]) {
    const int W = a.W;
    float x5[25], mxs[9], sxxs[9];
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int c = 0; c < 5; ++c) x5[r * 5 + c] = a.g1[at + (r - 2) * W + (c - 2)];
#pragma unroll
    for (int zr = 0; zr < 3; ++zr)
#pragma unroll
        for (int zc = 0; zc < 3; ++zc) {
            float xs[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) xs[k] = x5[(zr + k / 3) * 5 + zc + k % 3];
            const float mx = mean9(xs);
            mxs[zr * 3 + zc] = mx;
            sxxs[zr * 3 + zc] = cov9(xs, mx, xs, mx);
        }
    for (int i = 0; i < a.n_pred; ++i) {
        const int64_t ib = (int64_t)i * a.npix + at;
        float w5[25], m9[9];
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int c = 0; c < 5; ++c) w5[r * 5 + c] = a.wv[ib + (r - 2) * W + (c - 2)];
        load9(a.valid + ib, W, m9);
        float G = 0.f;
#pragma unroll
        for (int zr = 0; zr < 3; ++zr)
#pragma unroll
            for (int zc = 0; zc < 3; ++zc) {
                const int z = zr * 3 + zc;
                float xs[9], ws[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    xs[k] = x5[(zr + k / 3) * 5 + zc + k % 3];
                    ws[k] = w5[(zr + k / 3) * 5 + zc + k % 3];
                }
                const float mw = mean9(ws);
                Coefs c;
                const float S = ssim_of_moments<true>(mxs[z], sxxs[z], mw, cov9(ws, mw, ws, mw), cov9(xs, mxs[z], ws, mw), c);
                const float share = window_share(c, x5[12], mxs[z], w5[12], mw);
                G = G + (m9[z] != 0.f ? share : 0.f);
                if (z == 4 && m9[4] != 0.f) ssim_add_value(a, pw, i, S, acc);
            }
        store_grad(a, x, y, at, i, pw.w[i], G);
    }
}

// Value and gradient of a pixel nearer the border: the same windows in the same order, one at a time.  A window out of frame or
// with M = 0 (every window that is not interior) is dropped; one with M = 1 has its nine pixels in the frame.
__device__ __forceinline__ void ssim_pixel_edge(const SweepArgs &a, const PredWeights &pw, int x, int y, int64_t at,
                                                double (&acc)[kVals]) {
    const int H = a.H, W = a.W;
    const float xy = a.g1[at];
    for (int i = 0; i < a.n_pred; ++i) {
        const int64_t ib = (int64_t)i * a.npix + at;
        const float wy = a.wv[ib];
        float G = 0.f;
#pragma nounroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma nounroll
            for (int dx = -1; dx <= 1; ++dx) {
                const bool ok = y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W;
                const int off = ok ? dy * W + dx : 0;
                if (!ok || a.valid[ib + off] == 0.f) continue;
                float xs[9], ws[9];
                load9(a.g1 + at + off, W, xs);
                load9(a.wv + ib + off, W, ws);
                const float mx = mean9(xs), mw = mean9(ws);
                Coefs c;
                const float S = ssim_of_moments<true>(mx, cov9(xs, mx, xs, mx), mw, cov9(ws, mw, ws, mw), cov9(xs, mx, ws, mw), c);
                G = G + window_share(c, xy, mx, wy, mw);
                if (dy == 0 && dx == 0) ssim_add_value(a, pw, i, S, acc);
            }
        }
        store_grad(a, x, y, at, i, pw.w[i], G);
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(kThreads) ssim_sweep_kernel(SweepArgs a, int B, PredWeights pw, double *__restrict__ part) {
    const int H = a.H, W = a.W, HW = H * W;
    double acc[kVals] = {0.0, 0.0};
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW;
        for (int p = (int)blockIdx.x * kThreads + (int)threadIdx.x; p < HW; p += (int)gridDim.x * kThreads) {
            const int y = p / W, x = p - y * W;
            if (!GRAD)
                ssim_pixel_value(a, pw, base + p, acc);
            else if (x >= 2 && x <= W - 3 && y >= 2 && y <= H - 3)
                ssim_pixel_whole(a, pw, x, y, base + p, acc);
            else
                ssim_pixel_edge(a, pw, x, y, base + p, acc);
        }
    }
    raft_block_sum_store(acc, part);
}

}   // namespace

extern "C" int64_t raft_ssim_loss_workspace_bytes(int n_predictions, int B, int H, int W) {
    return warped_workspace_bytes(n_predictions, B, H, W);
}

extern "C" int raft_ssim_loss_f32(const float *image1, const float *image2, const uint8_t *mask, const float *preds,
                                  int64_t pred_stride, int n_predictions, int B, int H, int W, double gamma, float ssim_weight,
                                  float upstream, const float *add_to, float *out2, float *d_preds, int accumulate, void *workspace,
                                  void *stream) {
    RAFT_TRY(warped_check_args(image1, image2, preds, pred_stride, n_predictions, B, H, W, gamma, ssim_weight, upstream, out2, d_preds,
                               accumulate, workspace));
    const WarpedPlanes p = warped_planes(workspace, (int64_t)B * H * W, n_predictions);
    const SweepArgs a = sweep_args(image2, preds, pred_stride, n_predictions, B, H, W, upstream * ssim_weight, 18.0, d_preds, accumulate, p);
    hipStream_t s = (hipStream_t)stream;
    RAFT_TRY(launch_warped_gray<1>(image1, mask, a, B, p, s));
    const PredWeights pw = raft_pred_weights(gamma, n_predictions);
    const dim3 grid = raft_record_grid(B, (int64_t)H * W, kMaxRecords);
    if (d_preds != nullptr)
        ssim_sweep_kernel<true><<<grid, kThreads, 0, s>>>(a, B, pw, p.part);
    else
        ssim_sweep_kernel<false><<<grid, kThreads, 0, s>>>(a, B, pw, p.part);
    RAFT_TRY(raft_launch_status());
    return launch_warped_final(p, grid, a.npix, ssim_weight, add_to, out2, s);
}

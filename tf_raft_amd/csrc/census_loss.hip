// Soft census term of the self-supervised sequence loss (no reference counterpart): the data term that
// survives exposure changes, with d term / d prediction_i.  Definitions (every product and sum rounded on its own):
//
//   gray(c) = (0.299f*R + 0.587f*G) + 0.114f*B on 0..255,  g1 = gray(image1), g2 = gray(image2)
//   w_i(x)  = inside ? bilinear(taps of flow_sample.h under p_i, g2) : 0          (the warped gray)
//   f(d) = d / sqrtf(0.81f + d*d)   (soft ternary transform)      h(e) = e*e / (0.1f + e*e)   (soft Hamming distance)
//   interior(x, y) = 3 <= x <= W-4 && 3 <= y <= H-4,      M_i = mask && inside_i && interior
//   e(y, z) = f(w(z) - w(y)) - f(g1(z) - g1(y))
//   D(y) = (sum over the 48 neighbours z of y in a 7x7 patch, rows first, of h(e(y, z))) / 48.f
//   cen_i = sum_y M_i(y) * D(y) / (B*H*W),      out2 = {add_to + census_weight * sum_i w_i cen_i, cen_{n-1}},  w_i = (float)gamma^(n-i-1)
//
// Gradient as a gather (f is odd, h is even, both exactly in IEEE arithmetic, so e(z, y) = -e(y, z) and a pixel's two roles, as
// centre and as neighbour of a centre, collapse into ONE sweep over its 7x7 window):
//   S(y) = sum over z in frame, z != y, |z - y|_inf <= 3, rows first, of (M(y) + M(z)) * h'(e(y, z)) * f'(w(z) - w(y))
//   h'(e) = ((2*e)*0.1f) / (q*q), q = 0.1f + e*e        f'(d) = 0.81f / (r * sqrtf(r)), r = 0.81f + d*d
//   d cen_i / d w(y) = -S(y) / (48*B*H*W),    d/du = that * dwdu(y), d/dv = that * dwdv(y)  (the one-sided derivatives of the cell the
//   taps come from, 0 out of frame; `inside` and `mask` are constants of the gradient)
//
// Mapping: the three launches of warped_gray.h.  (1) warped_gray_kernel<3>: g1 once, and per prediction the warped gray w_i and M_i
// (as 1.f / 0.f), into the workspace.  (2) census_sweep_kernel, one thread per pixel looping over the predictions: the 48
// values f(g1(z) - g1(y)) do not depend on the prediction and are computed once per pixel (kept in the thread's own LDS column);
// per prediction the thread reads the 7x7 windows of w_i (and of M_i for the gradient) through the cache, as photometric_loss.hip
// reads its stencil, forms D and S from the same 48 pairs, and store_grad re-gathers the four taps of g2 for dwdu / dwdv and touches
// its element of d_preds once.  A pixel whose window lies in the frame takes a path without tests.  (3) warped_final_kernel adds
// the sweep's records and normalises.  Deterministic: the reduction of loss_common.h.
#include "loss_common.h"

#pragma clang fp contract(off)

#include "warped_gray.h"

namespace {

constexpr int kRadius = 3, kSide = 2 * kRadius + 1;
static_assert(kSide * kSide - 1 == 48, "the 48 neighbours of the definition");

__device__ __forceinline__ float soft_sign(float d) { return d / sqrtf(0.81f + d * d); }

// One pair (y, z): d = w(z) - w(y), fg = f(g1(z) - g1(y)), m = M(y) + M(z).  Adds h(e) to hs and, for the gradient, m * h'(e) * f'(d)
// to S when `ok` (z in frame).
template <bool GRAD>
__device__ __forceinline__ void census_pair(float d, float fg, float m, bool ok, float &hs, float &S) {
    const float r = 0.81f + d * d;
    const float sr = sqrtf(r);
    const float e = d / sr - fg;
    const float q = 0.1f + e * e;
    hs += (e * e) / q;
    if (GRAD) {
        const float term = (m * (((2.f * e) * 0.1f) / (q * q))) * (0.81f / (r * sr));
        S += ok ? term : 0.f;
    }
}

// One row of a pixel's window: seven values of w and, for the gradient, of M.
template <bool GRAD>
struct WindowRow {
    float w[kSide], m[GRAD ? kSide : 1];
    __device__ __forceinline__ void load(const float *__restrict__ wr, const float *__restrict__ mr) {
#pragma unroll
        for (int dx = -kRadius; dx <= kRadius; ++dx) {
            w[dx + kRadius] = wr[dx];
            if (GRAD) m[dx + kRadius] = mr[dx];
        }
    }
};

// A pixel whose 7x7 window lies in the frame, all predictions: no tests.  The values f(g1(z) - g1(y)) do not depend on the
// prediction: the thread computes them once and keeps them in its own column of `fg` (LDS; nobody else reads the column, so no
// barrier).  The rows of the window are a rolled loop: unrolled 48 times the compiler keeps several hundred values in flight and
// the gradient kernel runs at one wave per SIMD (measured: NOTEBOOK section 27).  `at` = the pixel's index over all images.
template <bool GRAD>
__device__ __forceinline__ void census_pixel_whole(const SweepArgs &a, const PredWeights &pw, int x, int y, int64_t at,
                                                   float (*fg)[kThreads], double (&acc)[kVals]) {
    const int W = a.W, tid = threadIdx.x;
    const float *gp = a.g1 + at;
    const float gc = gp[0];
#pragma nounroll
    for (int dy = -kRadius; dy <= kRadius; ++dy) {
        const float *gr = gp + dy * W;
#pragma unroll
        for (int dx = -kRadius; dx <= kRadius; ++dx) fg[(dy + kRadius) * kSide + dx + kRadius][tid] = soft_sign(gr[dx] - gc);
    }
    for (int i = 0; i < a.n_pred; ++i) {
        const int64_t ib = (int64_t)i * a.npix + at;
        const float mcf = a.valid[ib];
        const bool mc = mcf != 0.f;
        if (!GRAD && !mc) continue;
        const float *wp = a.wv + ib, *vp = a.valid + ib;
        const float wc = wp[0];
        float hs = 0.f, S = 0.f;
        // the next row of the window is loaded before the current one is worked on (its latency hides behind ~500 instructions)
        WindowRow<GRAD> cur, nxt;
        cur.load(wp - kRadius * W, vp - kRadius * W);
#pragma nounroll
        for (int dy = -kRadius; dy <= kRadius; ++dy) {
            const int dn = dy < kRadius ? dy + 1 : dy;          // (behind the last row: that row again, not a branch)
            nxt.load(wp + dn * W, vp + dn * W);
#pragma unroll
            for (int dx = -kRadius; dx <= kRadius; ++dx) {
                if (dy == 0 && dx == 0) continue;
                census_pair<GRAD>(cur.w[dx + kRadius] - wc, fg[(dy + kRadius) * kSide + dx + kRadius][tid],
                                  GRAD ? mcf + cur.m[dx + kRadius] : 0.f, true, hs, S);
            }
            cur = nxt;
        }
        if (mc) {
            const float D = hs / 48.f;
            acc[0] += (double)pw.w[i] * (double)D;
            if (i == a.n_pred - 1) acc[1] += (double)D;
        }
        if (GRAD) store_grad(a, x, y, at, i, pw.w[i], S);
    }
}

// A pixel whose window leaves the frame (gradient only: it is not interior, so M = 0 and it has no value of its own): the same
// pairs in the same order, neighbours out of frame read at a clamped position and dropped.  Rolled loops: these are few pixels.
__device__ __forceinline__ void census_pixel_edge(const SweepArgs &a, const PredWeights &pw, int x, int y, int64_t at) {
    const int H = a.H, W = a.W;
    const int64_t img = at - ((int64_t)y * W + x);
    const float gc = a.g1[at];
    for (int i = 0; i < a.n_pred; ++i) {
        const float *wp = a.wv + (int64_t)i * a.npix + img;
        const float *vp = a.valid + (int64_t)i * a.npix + img;
        const float wc = wp[y * W + x];
        float hs = 0.f, S = 0.f;
#pragma nounroll
        for (int dy = -kRadius; dy <= kRadius; ++dy) {
#pragma nounroll
            for (int dx = -kRadius; dx <= kRadius; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const bool ok = y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W;
                const int z = min(max(y + dy, 0), H - 1) * W + min(max(x + dx, 0), W - 1);
                census_pair<true>(wp[z] - wc, soft_sign(a.g1[img + z] - gc), vp[z], ok, hs, S);
            }
        }
        store_grad(a, x, y, at, i, pw.w[i], S);
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(kThreads) census_sweep_kernel(SweepArgs a, int B, PredWeights pw, double *__restrict__ part) {
    const int H = a.H, W = a.W, HW = H * W;
    __shared__ float fg[kSide * kSide][kThreads];          // 49 KiB: three workgroups per CU
    double acc[kVals] = {0.0, 0.0};
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW;
        for (int p = (int)blockIdx.x * kThreads + (int)threadIdx.x; p < HW; p += (int)gridDim.x * kThreads) {
            const int y = p / W, x = p - y * W;
            const bool whole = x >= kRadius && x <= W - 1 - kRadius && y >= kRadius && y <= H - 1 - kRadius;
            if (whole)
                census_pixel_whole<GRAD>(a, pw, x, y, base + p, fg, acc);
            else if (GRAD)
                census_pixel_edge(a, pw, x, y, base + p);
        }
    }
    raft_block_sum_store(acc, part);
}

}   // namespace

extern "C" int64_t raft_census_loss_workspace_bytes(int n_predictions, int B, int H, int W) {
    return warped_workspace_bytes(n_predictions, B, H, W);
}

extern "C" int raft_census_loss_f32(const float *image1, const float *image2, const uint8_t *mask, const float *preds,
                                    int64_t pred_stride, int n_predictions, int B, int H, int W, double gamma, float census_weight,
                                    float upstream, const float *add_to, float *out2, float *d_preds, int accumulate, void *workspace,
                                    void *stream) {
    RAFT_TRY(warped_check_args(image1, image2, preds, pred_stride, n_predictions, B, H, W, gamma, census_weight, upstream, out2, d_preds,
                               accumulate, workspace));
    const WarpedPlanes p = warped_planes(workspace, (int64_t)B * H * W, n_predictions);
    const SweepArgs a = sweep_args(image2, preds, pred_stride, n_predictions, B, H, W, upstream * census_weight, 48.0, d_preds, accumulate, p);
    hipStream_t s = (hipStream_t)stream;
    RAFT_TRY(launch_warped_gray<kRadius>(image1, mask, a, B, p, s));
    const PredWeights pw = raft_pred_weights(gamma, n_predictions);
    const dim3 grid = raft_record_grid(B, (int64_t)H * W, kMaxRecords);
    if (d_preds != nullptr)
        census_sweep_kernel<true><<<grid, kThreads, 0, s>>>(a, B, pw, p.part);
    else
        census_sweep_kernel<false><<<grid, kThreads, 0, s>>>(a, B, pw, p.part);
    RAFT_TRY(raft_launch_status());
    return launch_warped_final(p, grid, a.npix, census_weight, add_to, out2, s);
}

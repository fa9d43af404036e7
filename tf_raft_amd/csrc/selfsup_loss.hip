// Self-supervision term of the self-supervised step (no reference counterpart): the n predictions of a
// STUDENT pass over a crop of the frames against the last prediction of the full-frame TEACHER pass, read in place through the
// crop's window and held constant, Charbonnier penalty, summed with the weights gamma^(n-i-1) of sequence_loss; and
// d loss / d prediction_i.  ONE launch computes the value and the gradient.
//
//   rho(d) = sqrtf(d*d + eps2) (eps2 = eps*eps rounded once to float32), w_i = (float)gamma^(n-i-1), t = teacher[b, y+oy, x+ox]
//   used(b,y,x) = (teacher_visible == NULL || teacher_visible[b, y+oy, x+ox] != 0)
//              && (student_visible == NULL || student_visible[b, y, x] == 0) && t.x and t.y finite
//   dist_i = sum_used (rho(p_i.x - t.x) + rho(p_i.y - t.y)) / (B*H*W*2)
//   out3 = {add_to + weight * sum_i w_i * dist_i, dist_{n-1}, #used / (B*H*W)}
//   d_preds_i = ((upstream * weight) * w_i) * ((d / rho(d)) * inv2) where used, else 0;  inv2 = (float)(1 / (B*H*W*2))
//
// The kernel is bound by bytes: per pixel 8n of predictions, 8 of teacher, a byte per mask; with the gradient 8n written (and
// 8n more read when it accumulates).  Mapping: one thread per student pixel, pixels of a slice numbered along its rows,
// blockIdx.y walks the slices, a thread loops over the n predictions with float2 accesses; the teacher vector and the masks
// are loaded once per pixel.  A pixel that is not used reads no prediction.  Deterministic: the reduction of loss_common.h,
// one record of kVals sums per workgroup (the count of used pixels is one of them: integers in float64, exact).  Every element
// of d_preds is touched exactly once.
// What bounds the entry is not bytes but the one-workgroup sum, which walks the records behind one another at 0.1 us each:
// with 1024 records it took 105 us beside a main launch of 35 us (value only) to 50 us (with the gradient); with 256 records
// and all of a pixel's predictions in flight together it takes 28 us beside 94 / 79 us (docs/NOTEBOOK.md section 32).
#include "loss_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;         // (what raft_block_sum_store and raft_record_grid take a workgroup to be)
constexpr int kMaxRecords = 256;      // partial records: one workgroup per CU (the one-workgroup sum walks them serially, 0.1 us each)
constexpr int kVals = 3;              // sum_i w_i * S_i, S_{n-1} (sums before normalisation), #used
constexpr int kUnroll = 12;           // predictions whose loads a thread has in flight together

struct SelfsupConsts {
    float scale, inv2, eps2;          // upstream * weight, 1 / (B*H*W*2)
    int accumulate;
};

__device__ __forceinline__ float rho(float d, float eps2) { return sqrtf(d * d + eps2); }

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.402823466e38f; }      // (a NaN fails)

template <bool GRAD, bool TVIS, bool SVIS>
__global__ void __launch_bounds__(kThreads) selfsup_loss_kernel(const float2 *__restrict__ teacher, const uint8_t *__restrict__ tvis,
                                                                int Ht, int Wt, int oy, int ox, const uint8_t *__restrict__ svis,
                                                                const float2 *__restrict__ preds, int64_t stride2, int n_pred, int B,
                                                                int H, int W, PredWeights pw, SelfsupConsts k, float2 *d_preds,
                                                                double *__restrict__ part) {
    const int HW = H * W;
    double acc[kVals] = {0.0, 0.0, 0.0};
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW, tbase = (int64_t)n * Ht * Wt;
        for (int p = (int)blockIdx.x * kThreads + (int)threadIdx.x; p < HW; p += (int)gridDim.x * kThreads) {
            const int y = p / W, x = p - y * W;
            // ---- once per pixel: the teacher vector through the window, the two masks
            const int64_t tp = tbase + (int64_t)(y + oy) * Wt + (x + ox);
            const float2 t = teacher[tp];
            const unsigned char tb = TVIS ? tvis[tp] : 1, sb = SVIS ? svis[base + p] : 0;     // (loaded together: no test waits for a load)
            const bool used = ((int)finite_f32(t.x) & (int)finite_f32(t.y) & (int)(tb != 0) & (int)(sb == 0)) != 0;
            if (used) acc[2] += 1.0;
            if (!GRAD && !used) continue;
            // ---- per prediction, kUnroll at a time.  The loads of a group (and its weights) are issued together, with no branch
            // between them, and the arithmetic follows in the order of i: a thread that waited for each prediction in turn kept
            // one 8-byte load in flight and ran at an eighth of the stream-copy rate.  A group that reaches past the last
            // prediction loads the last one again (from the cache) and does not use it.
            const int last = n_pred - 1;
            for (int i0 = 0; i0 < n_pred; i0 += kUnroll) {
                float2 f[kUnroll], was[kUnroll];
                float wv[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    wv[u] = pw.w[min(i0 + u, last)];
                    f[u] = was[u] = make_float2(0.f, 0.f);
                }
                if (used) {
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) f[u] = preds[(int64_t)min(i0 + u, last) * stride2 + base + p];
                }
                if (GRAD && k.accumulate) {
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) was[u] = d_preds[(int64_t)min(i0 + u, last) * stride2 + base + p];
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int i = i0 + u;
                    if (i > last) break;
                    float2 o = make_float2(0.f, 0.f);
                    if (used) {
                        const float du = f[u].x - t.x, dv = f[u].y - t.y;
                        const float ru = rho(du, k.eps2), rv = rho(dv, k.eps2);
                        const float r = ru + rv;
                        acc[0] += (double)wv[u] * (double)r;
                        if (i == last) acc[1] += (double)r;
                        if (GRAD) {
                            const float scale = k.scale * wv[u];
                            o.x = scale * ((du / ru) * k.inv2);
                            o.y = scale * ((dv / rv) * k.inv2);
                        }
                    }
                    if (GRAD) {
                        if (k.accumulate) {           // one float32 addition to what is there
                            o.x = was[u].x + o.x;
                            o.y = was[u].y + o.y;
                        }
                        d_preds[(int64_t)i * stride2 + base + p] = o;
                    }
                }
            }
        }
    }
    raft_block_sum_store(acc, part);
}

__global__ void __launch_bounds__(64) selfsup_final_kernel(const double *__restrict__ part, int nparts, double inv2, double pixels,
                                                           double weight, const float *add_to, float *out3) {
    __shared__ double tot[kVals];
    raft_sum_records(part, nparts, tot);
    if (threadIdx.x == 0) {
        const double before = add_to != nullptr ? (double)add_to[0] : 0.0;      // (read before out3 is written: they may be one address)
        out3[0] = (float)(before + weight * (tot[0] * inv2));
        out3[1] = (float)(tot[1] * inv2);
        out3[2] = (float)(tot[2] / pixels);                                     // (an exact count, divided in double)
    }
}

}   // namespace

extern "C" int64_t raft_selfsup_loss_workspace_doubles(void) { return (int64_t)kMaxRecords * kVals; }

extern "C" int raft_selfsup_loss_f32(const float *teacher, const uint8_t *teacher_visible, int Ht, int Wt, int oy, int ox,
                                     const uint8_t *student_visible, const float *preds, int64_t pred_stride, int n_predictions, int B,
                                     int H, int W, double gamma, float weight, float eps, float upstream, const float *add_to,
                                     float *out3, float *d_preds, int accumulate, double *workspace, void *stream) {
    RAFT_REQUIRE_PTR(teacher);
    RAFT_REQUIRE_PTR(preds);
    RAFT_REQUIRE_PTR(out3);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(n_predictions > 0 && B > 0 && H > 0 && W > 0 && Ht > 0 && Wt > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE(oy >= 0 && ox >= 0 && (int64_t)oy + H <= Ht && (int64_t)ox + W <= Wt, RAFT_E_SHAPE);      // the window lies in the teacher
    const int64_t npix = (int64_t)B * H * W;
    RAFT_REQUIRE(raft_loss_shape_ok(n_predictions, B, Ht, Wt), RAFT_E_SHAPE);                              // (so npix fits too)
    RAFT_REQUIRE(pred_stride >= 2 * npix, RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_finite_nonneg(gamma) && raft_finite_nonneg(weight), RAFT_E_SHAPE);
    const float eps2 = eps * eps;                 // rho(0) = sqrtf(eps2) divides the gradient: it must be positive and finite
    RAFT_REQUIRE(eps > 0.f && eps2 > 0.f && eps2 <= 3.402823466e38f, RAFT_E_SHAPE);      // (a NaN fails)
    RAFT_REQUIRE(raft_finite_f32(upstream), RAFT_E_SHAPE);
    RAFT_REQUIRE(accumulate == 0 || accumulate == 1, RAFT_E_SHAPE);
    RAFT_REQUIRE(n_predictions <= kMaxPredictions && (pred_stride & 1) == 0, RAFT_E_UNSUPPORTED);
    RAFT_REQUIRE(((((uintptr_t)teacher) | ((uintptr_t)preds) | ((uintptr_t)d_preds) | ((uintptr_t)workspace)) & 7u) == 0,
                 RAFT_E_ALIGN);                   // float2 / double

    const PredWeights pw = raft_pred_weights(gamma, n_predictions);
    const double inv2 = 1.0 / ((double)npix * 2.0);
    SelfsupConsts k;
    k.scale = upstream * weight, k.inv2 = (float)inv2, k.eps2 = eps2, k.accumulate = accumulate;
    const dim3 grid = raft_record_grid(B, (int64_t)H * W, kMaxRecords);
    hipStream_t s = (hipStream_t)stream;
    const float2 *te = (const float2 *)teacher, *pr = (const float2 *)preds;
    float2 *dp = (float2 *)d_preds;
    const int64_t stride2 = pred_stride / 2;
#define RAFT_SS_LAUNCH(G, T, S)                                                                                                       \
    selfsup_loss_kernel<G, T, S><<<grid, kThreads, 0, s>>>(te, teacher_visible, Ht, Wt, oy, ox, student_visible, pr, stride2,            \
                                                           n_predictions, B, H, W, pw, k, dp, workspace)
#define RAFT_SS_MASKS(G)                                                                                                              \
    do {                                                                                                                              \
        if (teacher_visible != nullptr) {                                                                                             \
            if (student_visible != nullptr) RAFT_SS_LAUNCH(G, true, true); else RAFT_SS_LAUNCH(G, true, false);                       \
        } else {                                                                                                                      \
            if (student_visible != nullptr) RAFT_SS_LAUNCH(G, false, true); else RAFT_SS_LAUNCH(G, false, false);                     \
        }                                                                                                                             \
    } while (0)
    if (d_preds != nullptr) RAFT_SS_MASKS(true); else RAFT_SS_MASKS(false);
#undef RAFT_SS_MASKS
#undef RAFT_SS_LAUNCH
    RAFT_TRY(raft_launch_status());
    selfsup_final_kernel<<<1, 64, 0, s>>>(workspace, (int)(grid.x * grid.y), inv2, (double)npix, (double)weight, add_to, out3);
    return raft_launch_status();
}

// Second-order, edge-aware smoothness of the self-supervised loss (no reference counterpart): the
// regulariser that leaves an affine flow (a zoom, a rotation, a receding ground plane) alone, summed over the n predictions of
// the loop with the weights gamma^(n-i-1) of sequence_loss, and d loss / d prediction_i.  ONE launch computes the value and the
// gradient.  s, eps2, rho and w_i are photometric_loss.hip's; edge_weight and eps are the first-order term's own parameters.
//
//   s = 1/255, rho(d) = sqrtf(d*d + eps2) (eps2 = eps*eps rounded once to float32), w_i = (float)gamma^(n-i-1)
//   cx(x,y) = expf(-edge_weight * mean_c |s * (image1(x+1,y)_c - image1(x-1,y)_c)|) for 1 <= x <= W-2 (no term otherwise),
//   cy likewise along y for 1 <= y <= H-2;   Dx_k(x,y) = (p(x+1,y)_k - 2*p(x,y)_k) + p(x-1,y)_k, Dy_k likewise, k in {u, v}
//   sm2_i = [sum cx * rho(Dx_k) + sum cy * rho(Dy_k)] / (B*H*W*2)
//   out2 = {add_to + smooth2_weight * sum_i w_i * sm2_i, sm2_{n-1}}
// The gradient is the adjoint written as a gather: with qx_k = cx * (Dx_k / rho(Dx_k)), qy_k likewise, both +0 where no stencil
// is centred,
//   g_k(x,y) = ((qx_k(x-1,y) - 2*qx_k(x,y)) + qx_k(x+1,y)) + ((qy_k(x,y-1) - 2*qy_k(x,y)) + qy_k(x,y+1))
//   d_preds_i(x,y)_k (= or +=) ((upstream * smooth2_weight) * w_i) * (g_k * inv2),   inv2 = (float)(1 / (B*H*W*2))
//
// Mapping.  A 256-thread workgroup owns a tile of kTW x kTH = 32 x 8 pixels (a wave is two rows of 32: its global accesses are
// two runs of 256 bytes), one thread per pixel; blockIdx.y walks the images and blockIdx.x the tiles of an image, both with
// grid-stride loops, so that the number of partial records stays bounded.  What does not depend on i is computed once per
// tile and kept in registers: the thread's own cx and cy, and (threads 0..79, with the gradient) the edge weight of the one
// halo stencil the thread also evaluates.  Then the n predictions loop:
//   1. the tile of prediction i with a halo of 2 (1 without the gradient) goes to LDS, pixels outside the picture as (0, 0);
//      the loads of prediction i+1, and of d_preds_i when it accumulates, are issued here and stay in flight over 2. and 3.
//      (the barriers order LDS traffic only);
//   2. every thread evaluates the two stencils centred on its pixel, both components: their VALUE is counted here and only
//      here, and with the gradient their q goes to LDS; threads 0..79 evaluate one halo stencil each (the columns x0-1 and
//      x0+32 of qx, the rows y0-1 and y0+8 of qy) for its q alone.  A stencil is thus evaluated once per tile that reads it:
//      (34*8 + 32*10) * 2 / 256 = 4.6 square roots and 4.6 divisions per pixel and prediction, against 12 of each for a
//      gather straight from global memory;
//   3. every thread gathers g from the q's of LDS (its own from registers) and stores or accumulates its float2.
// LDS: P 12 x 37, QX 8 x 35, QY 10 x 33 float2 = 8432 bytes (+ 64 of the reduction).  The pitches are an odd number of 8-byte
// elements; every access is 8 bytes wide and a half-wave reads 32 consecutive elements of one row.
// Deterministic: the reduction of loss_common.h, one record of kVals sums per workgroup.  Every element of d_preds is touched
// exactly once.
#include "loss_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;         // (what raft_block_sum_store takes a workgroup to be)
constexpr int kTW = 32, kTH = 8;      // the tile: kTW * kTH == kThreads
constexpr int kMaxRecords = 1024;     // partial records (4 workgroups per CU)
constexpr int kVals = 2;              // sum_i w_i * S_i, S_{n-1} (sums before normalisation)
constexpr int kFold = 16;             // records the final kernel sums side by side: kVals * kFold <= 64 columns
constexpr int kHaloStencils = 2 * kTH + 2 * kTW;      // 80: two columns of qx, two rows of qy

static_assert(kTW * kTH == kThreads && kHaloStencils <= kThreads, "one thread per pixel, at most one halo stencil per thread");

struct Smooth2Consts {
    float scale, inv2, eps2, edge_weight;      // upstream * smooth2_weight, 1 / (B*H*W*2)
};

__device__ __forceinline__ float rho(float d, float eps2) { return sqrtf(d * d + eps2); }

// expf(-edge_weight * mean_c |s * (hi_c - lo_c)|), the pixels at offsets hi and lo of image1
__device__ __forceinline__ float edge_weight_between(const float *__restrict__ i1, int lo, int hi, float edge_weight) {
    const float s = 1.0f / 255.0f;
    const float *a = i1 + (int64_t)lo * 3, *b = i1 + (int64_t)hi * 3;
    const float m = ((fabsf(s * (b[0] - a[0])) + fabsf(s * (b[1] - a[1]))) + fabsf(s * (b[2] - a[2]))) / 3.0f;
    return expf(-edge_weight * m);
}

// base[off], or (0, 0) for off < 0 (a pixel outside the picture).  Written as a guarded load into a value: `c ? base[off] : zero`
// selects between two ADDRESSES and puts `zero` into private memory.
__device__ __forceinline__ float2 load_or_zero(const float2 *__restrict__ base, int off) {
    float2 v = make_float2(0.f, 0.f);
    if (off >= 0) v = base[off];
    return v;
}

__device__ __forceinline__ float2 second_difference(float2 hi, float2 mid, float2 lo) {
    return make_float2((hi.x - 2.0f * mid.x) + lo.x, (hi.y - 2.0f * mid.y) + lo.y);
}

template <bool GRAD, bool ACC>
__global__ void __launch_bounds__(kThreads) smooth2_loss_kernel(const float *__restrict__ image1, const float2 *__restrict__ preds,
                                                                int64_t stride2, int n_pred, int B, int H, int W, PredWeights pw,
                                                                Smooth2Consts k, float2 *d_preds, double *__restrict__ part) {
    constexpr int PH = GRAD ? 2 : 1;                          // halo of the prediction's tile
    constexpr int PR = kTH + 2 * PH, PC = kTW + 2 * PH;       // its rows and columns
    constexpr int PP = PC + 1, QXP = kTW + 3, QYP = kTW + 1;  // pitches: an odd number of float2
    constexpr int kLoads = (PR * PC + kThreads - 1) / kThreads;
    __shared__ float2 P[PR * PP];
    __shared__ float2 Q[GRAD ? kTH * QXP + (kTH + 2) * QYP : 1];          // qx (kTH x (kTW+2)), then qy ((kTH+2) x kTW)
    constexpr int QY0 = kTH * QXP;

    const int tid = (int)threadIdx.x, tx = tid & (kTW - 1), ty = tid / kTW;
    const int HW = H * W;
    const int tiles_x = (W + kTW - 1) / kTW, tiles = tiles_x * ((H + kTH - 1) / kTH);
    double acc[kVals] = {0.0, 0.0};
    for (int n = blockIdx.y; n < B; n += gridDim.y) {
        const int64_t base = (int64_t)n * HW;
        const float *i1 = image1 + base * 3;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int x0 = (t % tiles_x) * kTW, y0 = (t / tiles_x) * kTH;
            const int x = x0 + tx, y = y0 + ty, p = y * W + x;
            const bool inimg = x < W && y < H;
            // ---- once per tile: the edge weights of the thread's own two stencils and of its halo stencil
            const bool hasx = inimg && x >= 1 && x <= W - 2, hasy = inimg && y >= 1 && y <= H - 2;
            const float cx = hasx ? edge_weight_between(i1, p - 1, p + 1, k.edge_weight) : 0.f;
            const float cy = hasy ? edge_weight_between(i1, p - W, p + W, k.edge_weight) : 0.f;
            bool hhas = false;
            float ch = 0.f;
            int hc = 0, hs = 0, hq = 0;                       // centre and step of the halo stencil in P, its place in Q
            if (GRAD && tid < kHaloStencils) {
                if (tid < 2 * kTH) {                          // qx at column x0 - 1 (side 0) or x0 + kTW (side 1), row y0 + r
                    const int side = tid & 1, r = tid >> 1;
                    const int hx = side ? x0 + kTW : x0 - 1, hy = y0 + r;
                    hhas = hy < H && hx >= 1 && hx <= W - 2;
                    if (hhas) ch = edge_weight_between(i1, hy * W + hx - 1, hy * W + hx + 1, k.edge_weight);
                    hc = (r + PH) * PP + (side ? kTW + PH : PH - 1), hs = 1;
                    hq = r * QXP + (side ? kTW + 1 : 0);
                } else {                                      // qy at row y0 - 1 (side 0) or y0 + kTH (side 1), column x0 + c
                    const int side = (tid - 2 * kTH) / kTW, c = (tid - 2 * kTH) % kTW;
                    const int hx = x0 + c, hy = side ? y0 + kTH : y0 - 1;
                    hhas = hx < W && hy >= 1 && hy <= H - 2;
                    if (hhas) ch = edge_weight_between(i1, (hy - 1) * W + hx, (hy + 1) * W + hx, k.edge_weight);
                    hc = (side ? kTH + PH : PH - 1) * PP + (c + PH), hs = PP;
                    hq = QY0 + (side ? kTH + 1 : 0) * QYP + c;
                }
            }
            // ---- where the thread's share of the prediction's tile lies: offsets into the image (-1: outside) and into P
            int src[kLoads], dst[kLoads];
#pragma unroll
            for (int l = 0; l < kLoads; ++l) {
                const int e = tid + l * kThreads, r = e / PC, c = e - r * PC;
                const int gx = x0 - PH + c, gy = y0 - PH + r;
                const bool in = e < PR * PC && gx >= 0 && gx < W && gy >= 0 && gy < H;
                src[l] = in ? gy * W + gx : -1;
                dst[l] = e < PR * PC ? r * PP + c : -1;
            }
            float2 cur[kLoads];
#pragma unroll
            for (int l = 0; l < kLoads; ++l) cur[l] = load_or_zero(preds + base, src[l]);
            const int me = (ty + PH) * PP + (tx + PH);
            // ---- per prediction
            for (int i = 0; i < n_pred; ++i) {
#pragma unroll
                for (int l = 0; l < kLoads; ++l)
                    if (dst[l] >= 0) P[dst[l]] = cur[l];
                raft_barrier_lds();
                if (i + 1 < n_pred) {                         // in flight until the next iteration stores them to LDS
                    const float2 *f = preds + (int64_t)(i + 1) * stride2 + base;
#pragma unroll
                    for (int l = 0; l < kLoads; ++l) cur[l] = load_or_zero(f, src[l]);
                }
                float2 *out = GRAD ? d_preds + (int64_t)i * stride2 + base + p : nullptr;
                float2 was = make_float2(0.f, 0.f);
                if (GRAD && ACC && inimg) was = *out;
                // the two stencils centred on this pixel: the only place their value is counted
                const float2 pc = P[me];
                const float2 dx = second_difference(P[me + 1], pc, P[me - 1]), dy = second_difference(P[me + PP], pc, P[me - PP]);
                const float rxu = rho(dx.x, k.eps2), rxv = rho(dx.y, k.eps2), ryu = rho(dy.x, k.eps2), ryv = rho(dy.y, k.eps2);
                const float sm = cx * (rxu + rxv) + cy * (ryu + ryv);              // (an edge weight that does not exist is 0)
                acc[0] += (double)pw.w[i] * (double)sm;
                if (i == n_pred - 1) acc[1] += (double)sm;
                if (GRAD) {
                    const float2 qx = make_float2(hasx ? cx * (dx.x / rxu) : 0.f, hasx ? cx * (dx.y / rxv) : 0.f);
                    const float2 qy = make_float2(hasy ? cy * (dy.x / ryu) : 0.f, hasy ? cy * (dy.y / ryv) : 0.f);
                    Q[ty * QXP + tx + 1] = qx;
                    Q[QY0 + (ty + 1) * QYP + tx] = qy;
                    if (tid < kHaloStencils) {                // a halo copy: its q only, never its value
                        const float2 d = second_difference(P[hc + hs], P[hc], P[hc - hs]);
                        Q[hq] = make_float2(hhas ? ch * (d.x / rho(d.x, k.eps2)) : 0.f, hhas ? ch * (d.y / rho(d.y, k.eps2)) : 0.f);
                    }
                    raft_barrier_lds();
                    const float2 xl = Q[ty * QXP + tx], xr = Q[ty * QXP + tx + 2];
                    const float2 yu = Q[QY0 + ty * QYP + tx], yd = Q[QY0 + (ty + 2) * QYP + tx];
                    const float gu = ((xl.x - 2.0f * qx.x) + xr.x) + ((yu.x - 2.0f * qy.x) + yd.x);
                    const float gv = ((xl.y - 2.0f * qx.y) + xr.y) + ((yu.y - 2.0f * qy.y) + yd.y);
                    const float scale = k.scale * pw.w[i];
                    float2 o = make_float2(scale * (gu * k.inv2), scale * (gv * k.inv2));
                    if (ACC) {                                // one float32 addition to what is there
                        o.x = was.x + o.x;
                        o.y = was.y + o.y;
                    }
                    if (inimg) *out = o;
                } else {
                    raft_barrier_lds();                       // P is free for the next prediction
                }
            }
        }
    }
    raft_block_sum_store(acc, part);
}

// The one-workgroup sum.  raft_sum_records walks its records behind one another, 0.1 us each (selfsup_loss.hip measured it), so
// the records are read as rows of kFold records = kVals * kFold columns: 32 threads walk nparts / kFold rows side by side, and
// thread 0 adds the kFold column sums of each value in index order, then the records of the last, partial row in index order.
__global__ void __launch_bounds__(64) smooth2_final_kernel(const double *__restrict__ part, int nparts, double inv2, double weight,
                                                           const float *add_to, float *out2) {
    __shared__ double col[kVals * kFold];
    const int rows = nparts / kFold;
    raft_sum_records(part, rows, col);
    if (threadIdx.x == 0) {
        double tot[kVals];
#pragma unroll
        for (int v = 0; v < kVals; ++v) {
            double s = 0.0;
            for (int f = 0; f < kFold; ++f) s += col[f * kVals + v];
            for (int r = rows * kFold; r < nparts; ++r) s += part[(int64_t)r * kVals + v];
            tot[v] = s;
        }
        const double before = add_to != nullptr ? (double)add_to[0] : 0.0;      // (read before out2 is written: they may be one address)
        out2[0] = (float)(before + weight * (tot[0] * inv2));
        out2[1] = (float)(tot[1] * inv2);
    }
}

}   // namespace

extern "C" int64_t raft_smooth2_loss_workspace_doubles(void) { return (int64_t)kMaxRecords * kVals; }

extern "C" int raft_smooth2_loss_f32(const float *image1, const float *preds, int64_t pred_stride, int n_predictions, int B, int H,
                                     int W, double gamma, float smooth2_weight, float edge_weight, float eps, float upstream,
                                     const float *add_to, float *out2, float *d_preds, int accumulate, double *workspace,
                                     void *stream) {
    RAFT_REQUIRE_PTR(image1);
    RAFT_REQUIRE_PTR(preds);
    RAFT_REQUIRE_PTR(out2);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(raft_loss_shape_ok(n_predictions, B, H, W), RAFT_E_SHAPE);
    const int64_t npix = (int64_t)B * H * W;
    RAFT_REQUIRE(pred_stride >= 2 * npix, RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_finite_nonneg(gamma) && raft_finite_nonneg(smooth2_weight) && raft_finite_nonneg(edge_weight), RAFT_E_SHAPE);
    const float eps2 = eps * eps;                 // rho(0) = sqrtf(eps2) divides the gradient: it must be positive and finite
    RAFT_REQUIRE(eps > 0.f && eps2 > 0.f && eps2 <= 3.402823466e38f, RAFT_E_SHAPE);      // (a NaN fails)
    RAFT_REQUIRE(raft_finite_f32(upstream), RAFT_E_SHAPE);
    RAFT_REQUIRE(accumulate == 0 || accumulate == 1, RAFT_E_SHAPE);
    RAFT_REQUIRE(n_predictions <= kMaxPredictions && (pred_stride & 1) == 0, RAFT_E_UNSUPPORTED);
    RAFT_REQUIRE(((((uintptr_t)preds) | ((uintptr_t)d_preds) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);   // float2 / double

    const PredWeights pw = raft_pred_weights(gamma, n_predictions);
    const double inv2 = 1.0 / ((double)npix * 2.0);
    Smooth2Consts k;
    k.scale = upstream * smooth2_weight, k.inv2 = (float)inv2, k.eps2 = eps2, k.edge_weight = edge_weight;
    // blockIdx.y walks the images, blockIdx.x the tiles of an image: at most kMaxRecords workgroups, images first
    const int64_t tiles = (int64_t)((W + kTW - 1) / kTW) * ((H + kTH - 1) / kTH);
    const int gy = B < kMaxRecords ? B : kMaxRecords;
    const int64_t cap = kMaxRecords / gy;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap), (unsigned)gy);
    hipStream_t s = (hipStream_t)stream;
    const float2 *pr = (const float2 *)preds;
    float2 *dp = (float2 *)d_preds;
    const int64_t stride2 = pred_stride / 2;
#define RAFT_SM2_LAUNCH(G, A) \
    smooth2_loss_kernel<G, A><<<grid, kThreads, 0, s>>>(image1, pr, stride2, n_predictions, B, H, W, pw, k, dp, workspace)
    if (d_preds != nullptr) {
        if (accumulate) RAFT_SM2_LAUNCH(true, true); else RAFT_SM2_LAUNCH(true, false);
    } else {
        RAFT_SM2_LAUNCH(false, false);
    }
#undef RAFT_SM2_LAUNCH
    RAFT_TRY(raft_launch_status());
    smooth2_final_kernel<<<1, 64, 0, s>>>(workspace, (int)(grid.x * grid.y), inv2, (double)smooth2_weight, add_to, out2);
    return raft_launch_status();
}

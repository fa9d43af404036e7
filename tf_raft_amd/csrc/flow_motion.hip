// The camera's motion from a flow (no reference counterpart): one parametric motion per slice fitted to the
// vectors of a flow by iteratively reweighted least squares, on the device, and the flow that is left when it is taken away.
//
//   raft_flow_fit_motion_f32   flow (N, H, W, 2) [, mask] -> motion (N, 2, 3), stats (N, 4)
//   raft_flow_residual_f32     flow, motion -> residual (N, H, W, 2) [, moving (N, H, W)]
//   raft_motion_flow_f32       motion -> its dense flow (N, H, W, 2)
//
// The fit.  A pixel is USED iff both components of its vector are finite and its mask byte admits it (mask NULL; or
// mask_invert == 0 and the byte nonzero; or mask_invert == 1 and the byte zero).  With the centred coordinates
// X = x - (W - 1) / 2, Y = y - (H - 1) / 2 the model is d(X, Y) = L (X, Y) + t, L = (l00 l01; l10 l11).  Everything behind the
// load is float64 and contraction is off: every product, sum and quotient below is rounded on its own, in the order written.
//
// Solve k = 1 .. iterations:
//   moments kernel, per used pixel with vector (u, v):
//       k == 1:  w = 1
//       k  > 1:  ru = u - ((l00 * X + l01 * Y) + tx),  rv = v - ((l10 * X + l11 * Y) + ty),  r2 = ru * ru + rv * rv,
//                w = s2 / (s2 + r2)   with s2 = double(scale) * double(scale) and (L, t) the float64 estimate of solve k - 1: the
//                Cauchy weight 1 / (1 + r2 / scale^2) with ONE division (the kernel trace in docs/NOTEBOOK.md section 39 is why)
//       wX = w * X, wY = w * Y, and the twelve sums
//       Sw += w, SwX += wX, SwY += wY, SwXX += wX * X, SwXY += wX * Y, SwYY += wY * Y,
//       Swu += w * u, SwXu += wX * u, SwYu += wY * u, Swv += w * v, SwXv += wX * v, SwYv += wY * v
//     per thread over its grid-stride share, then raft_block_sum_store into record blockIdx.y * gridDim.x + blockIdx.x: the
//     records of slice n are the gridDim.x consecutive ones from n * gridDim.x, no record is shared between slices.
//   solve kernel, one workgroup per slice: the records, read as rows of kMotionColumns records, are added column by column in
//     index order (raft_sum_records) and the kMotionColumns partial totals of a sum in index order behind it.  Then
//       !(Sw > 0) (or the solve before gave status 2):  L = 0, t = 0, status 2
//       mX = SwX / Sw, mY = SwY / Sw, mu = Swu / Sw, mv = Swv / Sw,  pX = Sw * mX, pY = Sw * mY
//       cxx = SwXX - pX * mX, cxy = SwXY - pX * mY, cyy = SwYY - pY * mY
//       bxu = SwXu - pX * mu, byu = SwYu - pY * mu, bxv = SwXv - pX * mv, byv = SwYv - pY * mv
//       affine,     iff D > 1e-12 * (m * m) with D = cxx * cyy - cxy * cxy, m = max(cxx, cyy):
//           l00 = (bxu * cyy - byu * cxy) / D, l01 = (byu * cxx - bxu * cxy) / D,
//           l10 = (bxv * cyy - byv * cxy) / D, l11 = (byv * cxx - bxv * cxy) / D
//       similarity, iff q > 0 with q = cxx + cyy:
//           a = (bxu + byv) / q, b = (bxv - byu) / q,  L = (a  -b; b  a)
//       translation: L = 0
//       the full model: status 0, tx = mu - (l00 * mX + l01 * mY), ty = mv - (l10 * mX + l11 * mY)
//       otherwise (affine or similarity without the rank; a NaN takes this branch): L = 0, t = (mu, mv), status 1
//     and the estimate (l00, l01, l10, l11, tx, ty, status) goes back to the workspace as float64.
// After the last solve:
//   statistics kernel: per used pixel, under the final estimate, w as for k > 1, and the sums used += 1, Sw += w, Swr2 += w * r2
//   final kernel, one workgroup per slice: stats = (used / (H * W), Sw / used, sqrt(Swr2 / Sw), status), every quotient a
//     float64 one rounded to float32 once, the first three 0 where !(used > 0); and with cx = (W - 1) / 2, cy = (H - 1) / 2
//       motion = (1 + l00, l01, tx - (l00 * cx + l01 * cy);  l10, 1 + l11, ty - (l10 * cx + l11 * cy))
//     each entry rounded to float32 once: the map p2 = M (x, y, 1) in plain pixel coordinates.  Zero flow gives the identity.
//
// 2 * iterations + 2 launches, enqueued by the one call; no atomics, no memset, no host synchronisation, no grid-wide barrier:
// every record and estimate that a launch reads was written by a launch before it (workgroups without pixels store zero records,
// which is how the number of records of a slice is kept a multiple of kMotionColumns).
//
// The moments pass reads 8 bytes of flow and 1 of mask per pixel.  Two pixels per thread come as one 16-byte and one 2-byte load
// where the flow is 16-byte aligned, the mask 2-byte aligned and H * W even; the pixel's (x, y) is carried along the
// grid-stride loop by addition, not by division.  Twelve float64 accumulators and one float64 division per pixel are the
// arithmetic; docs/NOTEBOOK.md section 39 has what was measured.
#include "common.h"

#pragma clang fp contract(off)

#include "loss_common.h"

namespace {

constexpr int kMotionThreads = 256;
constexpr int kMotionRecords = 256;        // cap on the records of a slice (512 was measured and is slower: NOTEBOOK section 39)
constexpr int kMotionColumns = 64;         // records added side by side by the solve: kMotionRecords / kMotionColumns behind one another
constexpr int kSolveThreads = 768;         // of the solve and the final kernel: one per column of a row of moment records
constexpr int kMomentValues = 12;
constexpr int kStatValues = 3;
constexpr int kEstimateDoubles = 8;        // l00 l01 l10 l11 tx ty status (spare)
constexpr int kMotionMaxSlices = 65535;    // blockIdx.y walks the slices
static_assert(kMotionRecords % kMotionColumns == 0, "rows of records");
static_assert(kMomentValues * kMotionColumns <= kSolveThreads, "one thread per column of a row");

struct Estimate {
    double l00, l01, l10, l11, tx, ty;
};

__device__ __forceinline__ Estimate load_estimate(const double *__restrict__ est) {
    return Estimate{est[0], est[1], est[2], est[3], est[4], est[5]};
}

__device__ __forceinline__ bool pixel_used(float u, float v, unsigned mask_byte, int mask_mode) {
    // mask_mode: 0 no mask, 1 used where nonzero, 2 used where zero.  (|x| <= FLT_MAX: false for a NaN and an infinity)
    const bool finite = fabsf(u) <= 3.402823466e38f && fabsf(v) <= 3.402823466e38f;
    return finite && (mask_mode == 0 || (mask_mode == 1) == (mask_byte != 0u));
}

// the squared residual of (u, v) at (X, Y) under e
__device__ __forceinline__ double residual2(const Estimate &e, double X, double Y, double u, double v) {
    const double ru = u - ((e.l00 * X + e.l01 * Y) + e.tx);
    const double rv = v - ((e.l10 * X + e.l11 * Y) + e.ty);
    return ru * ru + rv * rv;
}

template <bool FIRST>
__device__ __forceinline__ void add_moments(double (&acc)[kMomentValues], const Estimate &e, double s2, double X, double Y, float uf,
                                            float vf) {
    const double u = (double)uf, v = (double)vf;
    double w = 1.0;
    if (!FIRST) w = s2 / (s2 + residual2(e, X, Y, u, v));
    const double wX = w * X, wY = w * Y;
    acc[0] += w;
    acc[1] += wX;
    acc[2] += wY;
    acc[3] += wX * X;
    acc[4] += wX * Y;
    acc[5] += wY * Y;
    acc[6] += w * u;
    acc[7] += wX * u;
    acc[8] += wY * u;
    acc[9] += w * v;
    acc[10] += wX * v;
    acc[11] += wY * v;
}

__device__ __forceinline__ void add_stats(double (&acc)[kStatValues], const Estimate &e, double s2, double X, double Y, float uf, float vf) {
    const double r2 = residual2(e, X, Y, (double)uf, (double)vf);
    const double w = s2 / (s2 + r2);
    acc[0] += 1.0;
    acc[1] += w;
    acc[2] += w * r2;
}

template <int PASS, int NV>
__device__ __forceinline__ void add_pixel(double (&acc)[NV], const Estimate &e, double s2, double X, double Y, float u, float v) {
    if constexpr (PASS == 2)
        add_stats(acc, e, s2, X, Y, u, v);
    else
        add_moments<PASS == 0>(acc, e, s2, X, Y, u, v);
}

// PASS 0: the moments of solve 1 (w = 1), 1: the moments of a later solve, 2: the statistics.  PIX pixels per thread and trip.
// (dy, dx) = divmod(gridDim.x * kMotionThreads * PIX, W), the step of the grid-stride loop in rows and columns.
template <int PASS, int PIX>
__global__ void __launch_bounds__(kMotionThreads) motion_sums_kernel(const float *__restrict__ flow, const uint8_t *__restrict__ mask,
                                                                     int mask_mode, const double *__restrict__ estimates, double s2,
                                                                     int H, int W, int dy, int dx, double *__restrict__ records) {
    constexpr int NV = PASS == 2 ? kStatValues : kMomentValues;
    const int n = blockIdx.y, HW = H * W;
    const float *f = flow + (int64_t)n * HW * 2;
    const uint8_t *m = mask_mode != 0 ? mask + (int64_t)n * HW : nullptr;
    Estimate e = {};
    if (PASS != 0) e = load_estimate(estimates + (int64_t)n * kEstimateDoubles);
    const double cx = (double)(W - 1) * 0.5, cy = (double)(H - 1) * 0.5;
    double acc[NV] = {};
    const int stride = (int)gridDim.x * kMotionThreads * PIX;          // (at most kMotionRecords * 256 * 2 = 2^17)
    int64_t p = ((int64_t)blockIdx.x * kMotionThreads + threadIdx.x) * PIX;
    int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    for (; p < HW; p += stride) {
        float u0, v0, u1 = 0.f, v1 = 0.f;
        unsigned b0 = 1u, b1 = 1u;
        if (PIX == 2) {
            const float4 q = *(const float4 *)(f + p * 2);
            u0 = q.x, v0 = q.y, u1 = q.z, v1 = q.w;
            if (m != nullptr) {
                const uchar2 b = *(const uchar2 *)(m + p);
                b0 = b.x, b1 = b.y;
            }
        } else {
            const float2 q = *(const float2 *)(f + p * 2);
            u0 = q.x, v0 = q.y;
            if (m != nullptr) b0 = m[p];
        }
        if (pixel_used(u0, v0, b0, mask_mode)) {
            const double X = (double)x - cx, Y = (double)y - cy;
            add_pixel<PASS>(acc, e, s2, X, Y, u0, v0);
        }
        if (PIX == 2 && pixel_used(u1, v1, b1, mask_mode)) {
            const bool wrap = x + 1 >= W;                               // (H * W is even, W need not be)
            const double X = (double)(wrap ? 0 : x + 1) - cx, Y = (double)(wrap ? y + 1 : y) - cy;
            add_pixel<PASS>(acc, e, s2, X, Y, u1, v1);
        }
        x += dx;
        y += dy;
        if (x >= W) {
            x -= W;
            ++y;
        }
    }
    raft_block_sum_store(acc, records);
}

// The NV sums of slice blockIdx.x from its `rows` rows of kMotionColumns records, in tot[0 .. NV), seen by every thread.
template <int NV>
__device__ __forceinline__ void slice_totals(const double *__restrict__ records, int rows, double (&cols)[NV * kMotionColumns],
                                             double (&tot)[NV]) {
    raft_sum_records(records + (int64_t)blockIdx.x * rows * (NV * kMotionColumns), rows, cols);
    if (threadIdx.x < NV) {
        double s = 0.0;
        for (int c = 0; c < kMotionColumns; ++c) s += cols[c * NV + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

template <bool FIRST>
__global__ void __launch_bounds__(kSolveThreads) motion_solve_kernel(const double *__restrict__ records, int rows, int model,
                                                                      double *__restrict__ estimates) {
    __shared__ double cols[kMomentValues * kMotionColumns];
    __shared__ double S[kMomentValues];
    slice_totals(records, rows, cols, S);
    if (threadIdx.x != 0) return;
    double *est = estimates + (int64_t)blockIdx.x * kEstimateDoubles;
    const double Sw = S[0];
    double l00 = 0.0, l01 = 0.0, l10 = 0.0, l11 = 0.0, tx = 0.0, ty = 0.0, status = 2.0;
    const bool stuck = !FIRST && est[6] == 2.0;
    if (!stuck && Sw > 0.0) {
        const double mX = S[1] / Sw, mY = S[2] / Sw, mu = S[6] / Sw, mv = S[9] / Sw;
        const double pX = Sw * mX, pY = Sw * mY;
        const double cxx = S[3] - pX * mX, cxy = S[4] - pX * mY, cyy = S[5] - pY * mY;
        const double bxu = S[7] - pX * mu, byu = S[8] - pY * mu, bxv = S[10] - pX * mv, byv = S[11] - pY * mv;
        bool full = model == 0;
        if (model == 2) {
            const double D = cxx * cyy - cxy * cxy, mx = fmax(cxx, cyy);
            if (D > 1e-12 * (mx * mx)) {
                full = true;
                l00 = (bxu * cyy - byu * cxy) / D;
                l01 = (byu * cxx - bxu * cxy) / D;
                l10 = (bxv * cyy - byv * cxy) / D;
                l11 = (byv * cxx - bxv * cxy) / D;
            }
        } else if (model == 1) {
            const double q = cxx + cyy;
            if (q > 0.0) {
                full = true;
                const double a = (bxu + byv) / q, b = (bxv - byu) / q;
                l00 = a, l01 = -b, l10 = b, l11 = a;
            }
        }
        if (full) {
            status = 0.0;
            tx = mu - (l00 * mX + l01 * mY);
            ty = mv - (l10 * mX + l11 * mY);
        } else {
            status = 1.0;
            tx = mu, ty = mv;
        }
    }
    est[0] = l00, est[1] = l01, est[2] = l10, est[3] = l11, est[4] = tx, est[5] = ty, est[6] = status, est[7] = 0.0;
}

__global__ void __launch_bounds__(kSolveThreads) motion_final_kernel(const double *__restrict__ records, int rows,
                                                                      const double *__restrict__ estimates, int H, int W,
                                                                      float *__restrict__ motion, float *__restrict__ stats) {
    __shared__ double cols[kStatValues * kMotionColumns];
    __shared__ double S[kStatValues];
    slice_totals(records, rows, cols, S);
    if (threadIdx.x != 0) return;
    const double *est = estimates + (int64_t)blockIdx.x * kEstimateDoubles;
    const Estimate e = load_estimate(est);
    const double cx = (double)(W - 1) * 0.5, cy = (double)(H - 1) * 0.5;
    float *M = motion + (int64_t)blockIdx.x * 6;
    M[0] = (float)(1.0 + e.l00);
    M[1] = (float)e.l01;
    M[2] = (float)(e.tx - (e.l00 * cx + e.l01 * cy));
    M[3] = (float)e.l10;
    M[4] = (float)(1.0 + e.l11);
    M[5] = (float)(e.ty - (e.l10 * cx + e.l11 * cy));
    float *st = stats + (int64_t)blockIdx.x * 4;
    const double used = S[0];
    const bool any = used > 0.0;
    st[0] = any ? (float)(used / ((double)H * (double)W)) : 0.f;
    st[1] = any ? (float)(S[1] / used) : 0.f;
    st[2] = any ? (float)sqrt(S[2] / S[1]) : 0.f;
    st[3] = (float)est[6];
}

// the displacement the motion gives pixel (x, y): ((m0 * x + m1 * y) + m2) - x, likewise for y, in float64
__device__ __forceinline__ void motion_vector(const float *__restrict__ M, int x, int y, double *gu, double *gv) {
    const double xd = (double)x, yd = (double)y;
    *gu = (((double)M[0] * xd + (double)M[1] * yd) + (double)M[2]) - xd;
    *gv = (((double)M[3] * xd + (double)M[4] * yd) + (double)M[5]) - yd;
}

// FLOW = true: residual = flow - g [, moving]; false: residual = g (the dense flow of the motion).  One thread per pixel.
template <bool FLOW>
__global__ void __launch_bounds__(kMotionThreads) motion_residual_kernel(const float2 *__restrict__ flow, const float *__restrict__ motion,
                                                                         float2 *__restrict__ residual, uint8_t *__restrict__ moving,
                                                                         int N, int H, int W, double threshold2) {
    const int HW = H * W;
    const int i = (int)(blockIdx.x * kMotionThreads + threadIdx.x);
    if (i >= HW) return;
    const int y = i / W, x = i - y * W;
    for (int n = blockIdx.y; n < N; n += (int)gridDim.y) {
        const int64_t at = (int64_t)n * HW + i;
        double gu, gv;
        motion_vector(motion + (int64_t)n * 6, x, y, &gu, &gv);
        if (!FLOW) {
            residual[at] = make_float2((float)gu, (float)gv);
            continue;
        }
        const float2 f = flow[at];
        const double rx = (double)f.x - gu, ry = (double)f.y - gv;
        if (residual != nullptr) residual[at] = make_float2((float)rx, (float)ry);
        if (moving != nullptr) moving[at] = !(rx * rx + ry * ry <= threshold2) ? 1 : 0;
    }
}

// (N, H, W) of flows (N, H, W, 2) whose elements an int counts, with blockIdx.y able to walk the slices of the fit
bool motion_shape_ok(int N, int H, int W, bool fit) {
    if (!(N > 0 && H > 0 && W > 0)) return false;
    const int64_t limit = ((int64_t)1 << 31) - 1;
    return (int64_t)N <= limit / H && (int64_t)N * H <= limit / W && (int64_t)N * H * W <= limit / 2 && (!fit || N <= kMotionMaxSlices);
}

int motion_record_count(int64_t HW, int pix) {
    const int64_t blocks = (HW + kMotionThreads * pix - 1) / (kMotionThreads * pix);
    const int r = (int)(blocks < kMotionRecords ? blocks : kMotionRecords);
    return (r + kMotionColumns - 1) / kMotionColumns * kMotionColumns;
}

template <int PASS>
void launch_sums(bool pair, dim3 grid, hipStream_t st, const float *flow, const uint8_t *mask, int mask_mode, const double *est, double s2,
                 int H, int W, double *records) {
    const int stride = (int)grid.x * kMotionThreads * (pair ? 2 : 1);
    if (pair)
        motion_sums_kernel<PASS, 2><<<grid, kMotionThreads, 0, st>>>(flow, mask, mask_mode, est, s2, H, W, stride / W, stride % W, records);
    else
        motion_sums_kernel<PASS, 1><<<grid, kMotionThreads, 0, st>>>(flow, mask, mask_mode, est, s2, H, W, stride / W, stride % W, records);
}

}   // namespace

extern "C" int64_t raft_flow_motion_workspace_doubles(int N, int H, int W) {
    if (!motion_shape_ok(N, H, W, true)) return 0;
    return (int64_t)N * (kEstimateDoubles + (int64_t)kMotionRecords * kMomentValues);
}

extern "C" int raft_flow_fit_motion_f32(const float *flow, const uint8_t *mask, int mask_invert, float *motion, float *stats, int N, int H,
                                        int W, int model, int iterations, float scale, double *workspace, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(motion);
    RAFT_REQUIRE_PTR(stats);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(motion_shape_ok(N, H, W, true), RAFT_E_SHAPE);
    RAFT_REQUIRE(model >= 0 && model <= 2 && iterations >= 1 && iterations <= 32 && (mask_invert == 0 || mask_invert == 1), RAFT_E_SHAPE);
    RAFT_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, RAFT_E_SHAPE);                      // (a NaN fails)
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)workspace)) & 7u) == 0, RAFT_E_ALIGN);     // read as float2; doubles
    const int64_t HW = (int64_t)H * W;
    const int mask_mode = mask == nullptr ? 0 : (mask_invert ? 2 : 1);
    const bool pair = (HW & 1) == 0 && raft_aligned16(flow) && (((uintptr_t)mask) & 1u) == 0;
    const int r = motion_record_count(HW, pair ? 2 : 1), rows = r / kMotionColumns;
    const dim3 grid((unsigned)r, (unsigned)N);
    const double s2 = (double)scale * (double)scale;
    double *est = workspace, *records = workspace + (int64_t)N * kEstimateDoubles;
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < iterations; ++k) {
        if (k == 0) {
            launch_sums<0>(pair, grid, st, flow, mask, mask_mode, est, s2, H, W, records);
            RAFT_TRY(raft_launch_status());
            motion_solve_kernel<true><<<N, kSolveThreads, 0, st>>>(records, rows, model, est);
        } else {
            launch_sums<1>(pair, grid, st, flow, mask, mask_mode, est, s2, H, W, records);
            RAFT_TRY(raft_launch_status());
            motion_solve_kernel<false><<<N, kSolveThreads, 0, st>>>(records, rows, model, est);
        }
        RAFT_TRY(raft_launch_status());
    }
    launch_sums<2>(pair, grid, st, flow, mask, mask_mode, est, s2, H, W, records);
    RAFT_TRY(raft_launch_status());
    motion_final_kernel<<<N, kSolveThreads, 0, st>>>(records, rows, est, H, W, motion, stats);
    return raft_launch_status();
}

extern "C" int raft_flow_residual_f32(const float *flow, const float *motion, float *residual, uint8_t *moving, int N, int H, int W,
                                      float threshold, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(motion);
    RAFT_REQUIRE(residual != nullptr || moving != nullptr, RAFT_E_NULL);
    RAFT_REQUIRE(motion_shape_ok(N, H, W, false), RAFT_E_SHAPE);
    RAFT_REQUIRE(threshold >= 0.f && threshold <= 3.402823466e38f, RAFT_E_SHAPE);             // (a NaN fails)
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)residual)) & 7u) == 0, RAFT_E_ALIGN);      // read and written as float2
    const dim3 grid((unsigned)raft_ceil_div((int64_t)H * W, kMotionThreads), (unsigned)(N < kMotionMaxSlices ? N : kMotionMaxSlices));
    motion_residual_kernel<true><<<grid, kMotionThreads, 0, (hipStream_t)stream>>>((const float2 *)flow, motion, (float2 *)residual, moving,
                                                                                  N, H, W, (double)threshold * (double)threshold);
    return raft_launch_status();
}

extern "C" int raft_motion_flow_f32(const float *motion, float *flow, int N, int H, int W, void *stream) {
    RAFT_REQUIRE_PTR(motion);
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE(motion_shape_ok(N, H, W, false), RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)flow) & 7u) == 0, RAFT_E_ALIGN);                                // written as float2
    const dim3 grid((unsigned)raft_ceil_div((int64_t)H * W, kMotionThreads), (unsigned)(N < kMotionMaxSlices ? N : kMotionMaxSlices));
    motion_residual_kernel<false><<<grid, kMotionThreads, 0, (hipStream_t)stream>>>(nullptr, motion, (float2 *)flow, nullptr, N, H, W, 0.0);
    return raft_launch_status();
}

// The student's view of a self-supervised step (no reference counterpart): frames, and the teacher's flow
// with its trust mask, gathered under one affine map per slice.
//
//   raft_view_frames_f32   dst[b, y, x, c] = src[b, :, :, c] sampled at p = M q + o, zero out of frame, optional gain / bias / clamp
//   raft_view_flow_f32     target[b, y, x] = Minv f, f the teacher flow sampled at p; target_visible = in frame && every tap of
//                          nonzero weight trusted && target finite; (0, 0) where it is not
//
// The record of slice b (RaftViewParams, device memory) maps the student's pixel indices q = (x, y) to the teacher's:
//     px = (m[0] * float(x) + m[1] * float(y)) + o[0],   py = (m[2] * float(x) + m[3] * float(y)) + o[1]
// every operation rounded on its own (contraction is switched off for this file).  In frame iff 0 <= px <= Wt - 1 and
// 0 <= py <= Ht - 1 (a NaN fails); the sample at (px, py) is the one of flow_sample.h, what raft_warp_f32 computes.
// A tap's weight is the product of its factor along x (1 - a or a) and along y (1 - b or b); 1 - a and 1 - b are never zero, so a
// weight is exactly zero iff the tap lies on the x1 side with a == 0 or on the y1 side with b == 0.  The flow entry reads such a
// tap as 0 and does not ask its trust: the identity view then copies the window, and a vector that is not finite clears exactly
// the pixels that weigh it.
//
// Both are gathers bound by memory, like raft_warp_f32, but the footprint of a row of student pixels is a slanted line in the
// teacher, so the workgroup is a 2-D tile of 32 x 8 student pixels (a wave: 32 x 2) whose footprint stays a compact patch in
// cache, whatever the rotation.  One thread per student pixel, the slice in blockIdx.z (the record is uniform per workgroup and
// comes through scalar loads), float2 flow accesses.  The flow entry reads the two taps of a row, neighbours in memory, as ONE
// 16-byte load and their trust bytes as ONE 2-byte load, as flow_check.hip's consistency test does: 6.2 / 6.5 us against
// 7.5 / 8.3 us with a load per tap (8 x 304 x 432 out of 368 x 496, identity / generic view, side by side in one job;
// docs/NOTEBOOK.md section 33).  No atomics, no memset, every output element is written exactly once; tap indices are clamped
// into the teacher whatever a record holds.
#include "common.h"

#pragma clang fp contract(off)

#include "flow_sample.h"      // Taps, sample_taps, bilinear: shared with flow_check.hip and photometric_loss.hip

namespace {

constexpr int kTileW = 32, kTileH = 8;

__device__ __forceinline__ Taps view_taps(const RaftViewParams &p, int x, int y, int Ht, int Wt) {
    const float fx = (float)x, fy = (float)y;
    const float px = (p.m[0] * fx + p.m[1] * fy) + p.o[0], py = (p.m[2] * fx + p.m[3] * fy) + p.o[1];
    return sample_taps(px, py, Ht, Wt);
}

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.402823466e38f; }      // (a NaN fails)

// CT > 0: the channel count at compile time (the taps of all channels are issued together); CT == 0: any C
template <int CT>
__global__ void __launch_bounds__(kTileW *kTileH) view_frames_kernel(const float *__restrict__ src,
                                                                     const RaftViewParams *__restrict__ params,
                                                                     float *__restrict__ dst, int B, int Ht, int Wt, int H, int W,
                                                                     int C) {
    const int x = (int)blockIdx.x * kTileW + (int)threadIdx.x, y = (int)blockIdx.y * kTileH + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const int Cn = CT > 0 ? CT : C;
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const RaftViewParams &p = params[b];
        const Taps t = view_taps(p, x, y, Ht, Wt);
        const float *g = src + (int64_t)b * Ht * Wt * Cn;
        float *out = dst + (((int64_t)b * H + y) * W + x) * Cn;
        const bool colour = p.colour != 0;
        if (CT > 0) {
            float v[CT > 0 ? CT : 1][4];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                v[c][0] = g[(int64_t)t.o00 * CT + c];
                v[c][1] = g[(int64_t)t.o01 * CT + c];
                v[c][2] = g[(int64_t)t.o10 * CT + c];
                v[c][3] = g[(int64_t)t.o11 * CT + c];
            }
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                float r = t.in ? bilinear(t, v[c][0], v[c][1], v[c][2], v[c][3]) : 0.f;
                if (colour) r = fminf(fmaxf(r * p.gain[c < 2 ? c : 2] + p.bias[c < 2 ? c : 2], 0.f), 255.f);
                out[c] = r;
            }
        } else {
            for (int c = 0; c < Cn; ++c) {
                const float g00 = g[(int64_t)t.o00 * Cn + c], g01 = g[(int64_t)t.o01 * Cn + c];
                const float g10 = g[(int64_t)t.o10 * Cn + c], g11 = g[(int64_t)t.o11 * Cn + c];
                float r = t.in ? bilinear(t, g00, g01, g10, g11) : 0.f;
                if (colour) r = fminf(fmaxf(r * p.gain[c < 2 ? c : 2] + p.bias[c < 2 ? c : 2], 0.f), 255.f);
                out[c] = r;
            }
        }
    }
}

// (FlowPair, two neighbouring vectors of a row read as one 16-byte load: flow_sample.h)
struct MaskPair {
    uint8_t lo, hi;              // their trust bytes, read as one 2-byte load
};

// PAIR: the two taps of a row are neighbours in memory and come as ONE load from the first of them (from the one before where the
// first is the row's last pixel, whose right neighbour is itself); needs Wt >= 2.
template <bool TVIS, bool PAIR>
__global__ void __launch_bounds__(kTileW *kTileH) view_flow_kernel(const float2 *__restrict__ flow, const uint8_t *__restrict__ tvis,
                                                                   const RaftViewParams *__restrict__ params,
                                                                   float2 *__restrict__ target, uint8_t *__restrict__ visible,
                                                                   int B, int Ht, int Wt, int H, int W) {
    const int x = (int)blockIdx.x * kTileW + (int)threadIdx.x, y = (int)blockIdx.y * kTileH + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const RaftViewParams &p = params[b];
        const Taps t = view_taps(p, x, y, Ht, Wt);
        const int64_t tbase = (int64_t)b * Ht * Wt;
        const float2 *g = flow + tbase;
        // all loads are issued together (the indices are clamped: every one is safe), the choice follows
        float2 g00, g01, g10, g11;
        uint8_t m00 = 1, m01 = 1, m10 = 1, m11 = 1;
        if (PAIR) {
            const int col = t.o01 - t.o00;               // 1, or 0 where x0 is the row's last pixel
            const int r0 = t.o00 + col - 1, r1 = t.o10 + col - 1;
            const FlowPair p0 = *(const FlowPair *)(g + r0), p1 = *(const FlowPair *)(g + r1);
            g00 = col ? p0.lo : p0.hi, g01 = p0.hi, g10 = col ? p1.lo : p1.hi, g11 = p1.hi;
            if (TVIS) {
                MaskPair q0, q1;
                __builtin_memcpy(&q0, tvis + tbase + r0, 2);
                __builtin_memcpy(&q1, tvis + tbase + r1, 2);
                m00 = col ? q0.lo : q0.hi, m01 = q0.hi, m10 = col ? q1.lo : q1.hi, m11 = q1.hi;
            }
        } else {
            g00 = g[t.o00], g01 = g[t.o01], g10 = g[t.o10], g11 = g[t.o11];
            if (TVIS) {
                const uint8_t *m = tvis + tbase;
                m00 = m[t.o00], m01 = m[t.o01], m10 = m[t.o10], m11 = m[t.o11];
            }
        }
        const bool wx = t.a != 0.f, wy = t.b != 0.f;                   // the x1 / y1 side has weight
        const bool trusted = m00 != 0 && (!wx || m01 != 0) && (!wy || m10 != 0) && (!(wx && wy) || m11 != 0);
        const float2 zero = make_float2(0.f, 0.f);
        g01 = wx ? g01 : zero, g10 = wy ? g10 : zero, g11 = (wx && wy) ? g11 : zero;
        const float u = bilinear(t, g00.x, g01.x, g10.x, g11.x), v = bilinear(t, g00.y, g01.y, g10.y, g11.y);
        const float tx = p.inv[0] * u + p.inv[1] * v, ty = p.inv[2] * u + p.inv[3] * v;
        const bool ok = t.in && trusted && finite_f32(tx) && finite_f32(ty);
        const int64_t q = ((int64_t)b * H + y) * W + x;
        target[q] = ok ? make_float2(tx, ty) : zero;
        visible[q] = ok ? 1 : 0;
    }
}

// what both entries ask of their sizes: positive, fewer than 2^31 elements in either tensor (per = elements per pixel)
int view_sizes(int B, int Ht, int Wt, int H, int W, int per) {
    RAFT_REQUIRE(B > 0 && Ht > 0 && Wt > 0 && H > 0 && W > 0 && per > 0, RAFT_E_SHAPE);
    const int64_t limit = ((int64_t)1 << 31) - 1;
    RAFT_REQUIRE((int64_t)B <= limit / Ht && (int64_t)B * Ht <= limit / Wt && (int64_t)B * Ht * Wt <= limit / per, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)B <= limit / H && (int64_t)B * H <= limit / W && (int64_t)B * H * W <= limit / per, RAFT_E_SHAPE);
    return RAFT_OK;
}

dim3 view_grid(int B, int H, int W) {
    return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)(B < 65535 ? B : 65535));
}

}   // namespace

extern "C" int raft_view_params_bytes(void) { return (int)sizeof(RaftViewParams); }

extern "C" int raft_view_frames_f32(const float *src, const RaftViewParams *params, float *dst, int B, int Ht, int Wt, int H, int W,
                                    int C, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(params);
    RAFT_REQUIRE_PTR(dst);
    RAFT_TRY(view_sizes(B, Ht, Wt, H, W, C));
    RAFT_REQUIRE((H + kTileH - 1) / kTileH <= 65535, RAFT_E_SHAPE);                         // (rows of tiles: one grid axis)
    const dim3 grid = view_grid(B, H, W), block(kTileW, kTileH);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: view_frames_kernel<1><<<grid, block, 0, s>>>(src, params, dst, B, Ht, Wt, H, W, C); break;
        case 2: view_frames_kernel<2><<<grid, block, 0, s>>>(src, params, dst, B, Ht, Wt, H, W, C); break;
        case 3: view_frames_kernel<3><<<grid, block, 0, s>>>(src, params, dst, B, Ht, Wt, H, W, C); break;
        default: view_frames_kernel<0><<<grid, block, 0, s>>>(src, params, dst, B, Ht, Wt, H, W, C); break;
    }
    return raft_launch_status();
}

extern "C" int raft_view_flow_f32(const float *flow, const uint8_t *teacher_visible, const RaftViewParams *params, float *target,
                                  uint8_t *target_visible, int B, int Ht, int Wt, int H, int W, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(params);
    RAFT_REQUIRE_PTR(target);
    RAFT_REQUIRE_PTR(target_visible);
    RAFT_TRY(view_sizes(B, Ht, Wt, H, W, 2));
    RAFT_REQUIRE((H + kTileH - 1) / kTileH <= 65535, RAFT_E_SHAPE);                         // (rows of tiles: one grid axis)
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)target)) & 7u) == 0, RAFT_E_ALIGN);      // float2
    const dim3 grid = view_grid(B, H, W), block(kTileW, kTileH);
    hipStream_t s = (hipStream_t)stream;
    const float2 *f = (const float2 *)flow;
    float2 *tg = (float2 *)target;
#define RAFT_VIEW_FLOW(T, P) view_flow_kernel<T, P><<<grid, block, 0, s>>>(f, teacher_visible, params, tg, target_visible, B, Ht, Wt, H, W)
    if (teacher_visible != nullptr) {
        if (Wt >= 2) RAFT_VIEW_FLOW(true, true); else RAFT_VIEW_FLOW(true, false);
    } else {
        if (Wt >= 2) RAFT_VIEW_FLOW(false, true); else RAFT_VIEW_FLOW(false, false);
    }
#undef RAFT_VIEW_FLOW
    return raft_launch_status();
}

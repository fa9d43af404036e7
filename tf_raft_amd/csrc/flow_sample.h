// The one definition of "the sample of a map under a flow vector" (DESIGN.md sections 15 and 17), shared by flow_check.hip (warp,
// forward-backward consistency), photometric_loss.hip (the self-supervised loss and its gradient), warped_gray.h (the warped gray
// of the census and SSIM terms), student_view.hip (the same sample at a position that an affine map gives)
// and flow_track.hip (a flow sampled at a tracked point, and flow_check.hip's forward-backward comparison).
//
// For the pixel at integer (x, y) with vector (u, v): sx = float(x) + u and sy = float(y) + v, ONE float32 addition each; the
// pixel is in frame iff 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails); x0 = floor(sx), x1 = min(x0 + 1, W - 1),
// a = sx - x0 (exact), likewise y0, y1, b, and the value is
//     (1 - b) * ((1 - a) * g[y0, x0] + a * g[y0, x1]) + b * ((1 - a) * g[y1, x0] + a * g[y1, x1])
// with every product and sum rounded on its own: a file that includes this header switches contraction off
// (#pragma clang fp contract(off) at file scope, before its first function).  Tap indices are clamped into the frame whatever
// the flow holds.
#pragma once

#include "common.h"

namespace {

struct Taps {
    int o00, o01, o10, o11;      // pixel offsets inside one image
    float a, b;
    bool in;
};

// the taps of the sample position (sx, sy) itself (student_view.hip arrives at it by an affine map, not by a flow vector)
__device__ __forceinline__ Taps sample_taps(float sx, float sy, int H, int W) {
#pragma clang fp contract(off)
    Taps t;
    t.in = sx >= 0.f && sx <= (float)(W - 1) && sy >= 0.f && sy <= (float)(H - 1);
    const float px = t.in ? sx : 0.f, py = t.in ? sy : 0.f;
    const float fx = floorf(px), fy = floorf(py);
    const int x0 = min(max((int)fx, 0), W - 1), y0 = min(max((int)fy, 0), H - 1);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    t.a = px - fx, t.b = py - fy;
    t.o00 = y0 * W + x0, t.o01 = y0 * W + x1, t.o10 = y1 * W + x0, t.o11 = y1 * W + x1;
    return t;
}

__device__ __forceinline__ Taps flow_taps(int x, int y, float2 f, int H, int W) {
#pragma clang fp contract(off)
    return sample_taps((float)x + f.x, (float)y + f.y, H, W);
}

__device__ __forceinline__ float bilinear(const Taps &t, float g00, float g01, float g10, float g11) {
#pragma clang fp contract(off)
    const float na = 1.f - t.a, nb = 1.f - t.b;
    return nb * (na * g00 + t.a * g01) + t.b * (na * g10 + t.a * g11);
}

struct alignas(8) FlowPair {
    float2 lo, hi;               // two neighbouring vectors of a row, read as one 16-byte load
};

// Both components of a flow `g` (one image, H x W vectors) sampled at the taps `t`.  PAIR: the two taps of a row are neighbours
// in memory and come as ONE 16-byte load from the first of them (from the one before where the first is the row's last pixel,
// whose right neighbour is itself); needs W >= 2.  (docs/NOTEBOOK.md section 21: faster than four 8-byte loads.)
template <bool PAIR>
__device__ __forceinline__ float2 sample_flow(const float2 *__restrict__ g, const Taps &t) {
#pragma clang fp contract(off)
    float2 g00, g01, g10, g11;
    if (PAIR) {
        const int col = t.o01 - t.o00;               // 1, or 0 where x0 is the row's last pixel
        const FlowPair r0 = *(const FlowPair *)(g + t.o00 + col - 1), r1 = *(const FlowPair *)(g + t.o10 + col - 1);
        g00 = col ? r0.lo : r0.hi, g01 = r0.hi, g10 = col ? r1.lo : r1.hi, g11 = r1.hi;
    } else {
        g00 = g[t.o00], g01 = g[t.o01], g10 = g[t.o10], g11 = g[t.o11];
    }
    return make_float2(bilinear(t, g00.x, g01.x, g10.x, g11.x), bilinear(t, g00.y, g01.y, g10.y, g11.y));
}

// The forward-backward comparison (Meister et al. 2018, UnFlow): a vector f and the other direction's vector s at f's end point
// disagree unless |f + s|^2 <= alpha * (|f|^2 + |s|^2) + beta, in exactly this operation order (a NaN anywhere: they disagree).
__device__ __forceinline__ bool flows_disagree(float2 f, float2 s, float alpha, float beta) {
#pragma clang fp contract(off)
    const float dx = f.x + s.x, dy = f.y + s.y;
    const float lhs = dx * dx + dy * dy;
    const float rhs = alpha * ((f.x * f.x + f.y * f.y) + (s.x * s.x + s.y * s.y)) + beta;
    return !(lhs <= rhs);
}

// The one-sided derivatives of that value by u and by v inside the cell the taps come from (zero where x1 == x0 or y1 == y0):
// dW/du = (1-b)*(g01-g00) + b*(g11-g10),  dW/dv = (1-a)*(g10-g00) + a*(g11-g01).  The caller drops them where !t.in.
__device__ __forceinline__ float bilinear_du(const Taps &t, float g00, float g01, float g10, float g11) {
#pragma clang fp contract(off)
    return (1.f - t.b) * (g01 - g00) + t.b * (g11 - g10);
}

__device__ __forceinline__ float bilinear_dv(const Taps &t, float g00, float g01, float g10, float g11) {
#pragma clang fp contract(off)
    return (1.f - t.a) * (g10 - g00) + t.a * (g11 - g01);
}

}   // namespace

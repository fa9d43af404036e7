// The one definition of "the sample of a map under a flow vector" (DESIGN.md sections 15 and 17), shared by flow_check.hip (warp,
// forward-backward consistency), photometric_loss.hip (the self-supervised loss and its gradient), warped_gray.h (the warped gray
// of the census and SSIM terms) and student_view.hip (the same sample at a position that an affine map gives).
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

// The one definition of "where a forward-splatted source pixel lands and with which weights" (DESIGN.md sections 21 and 25),
// shared by flow_splat.hip (the range map: a splat of the flow itself) and frame_splat.hip (the splat of frames).
//
// For the landing position (sx, sy), float32: the pixel contributes iff -1 < sx < float(W) and -1 < sy < float(H), compared on
// the floats (a NaN, an infinity or 1e30 fails before any conversion to an integer).  x0 = floor(sx), a = sx - x0 in float32,
// qa = (int)rintf(a * 4096) in 0 .. 4096, likewise y0, b, qb; the corner (x0 + dx, y0 + dy) receives the INTEGER weight
// wx[dx] * wy[dy] = (dx ? qa : 4096 - qa) * (dy ? qb : 4096 - qb), the four of which sum to exactly 2^24.  The caller drops a
// corner outside the frame or of weight 0.  A file that includes this header switches contraction off at file scope.
#pragma once

#include "common.h"

namespace {

constexpr int kSplatShift = 12;                              // a bilinear weight per axis in 1 / 4096
constexpr int kSplatOne = 1 << kSplatShift;

struct SplatTaps {
    int x0, y0;                  // -1 .. W - 1, -1 .. H - 1 (where `in`)
    unsigned wx[2], wy[2];       // the per-axis integer weights of the near and the far corner
    bool in;
};

__device__ __forceinline__ SplatTaps splat_taps(float sx, float sy, float fW, float fH) {
#pragma clang fp contract(off)
    SplatTaps t;
    t.in = sx > -1.f && sx < fW && sy > -1.f && sy < fH;                  // (a NaN fails)
    const float px = t.in ? sx : 0.f, py = t.in ? sy : 0.f;
    const float fx = floorf(px), fy = floorf(py);
    t.x0 = (int)fx, t.y0 = (int)fy;
    const int qa = (int)rintf((px - fx) * (float)kSplatOne), qb = (int)rintf((py - fy) * (float)kSplatOne);
    t.wx[0] = (unsigned)(kSplatOne - qa), t.wx[1] = (unsigned)qa;
    t.wy[0] = (unsigned)(kSplatOne - qb), t.wy[1] = (unsigned)qb;
    return t;
}

}   // namespace

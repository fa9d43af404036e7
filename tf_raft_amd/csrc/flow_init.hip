// A recurrence that does not start from zero: RAFT's video protocol starts pair t + 1 from the flow of pair t
// projected forward along itself at 1/8 resolution (`forward_interpolate` of the authors' evaluation code, which scatters the
// vectors to their end points and fills the grid with scipy's griddata(method='nearest')).
//
//   raft_forward_interpolate_f32   out[b, ty, tx] = flow[b, source] of the valid source whose end point is nearest to (tx, ty)
//   raft_warm_start_f32 / _small   coords1 = grid + flow_init, flow = flow_init, the GRU input's flow slot = flow_init
//
// The projection rule, fixed so that float32 NumPy restates it bit for bit.  Source j = y0 * w + x0 with vector (dx, dy) ends at
// x1 = x0 + dx, y1 = y0 + dy (ONE float32 addition each) and is VALID iff 0 < x1 < w and 0 < y1 < h, strictly, as in the authors'
// code (a NaN fails).  Target (tx, ty) takes the vector of the valid source that minimises
//     d = (tx - x1) * (tx - x1) + (ty - y1) * (ty - y1)
// every operation rounded on its own (the intrinsics below: never a fused multiply-add), ties to the lowest j; an image without a
// valid source gives zeros.
//
// The search is exhaustive: a frame of 448 x 1024 has M = 7168 cells, M^2 = 51 M candidates of eight VALU operations, beside a
// loop of ~10 ms.  One thread per target, grid (ceil(M / 256), images).  A workgroup walks the image's sources in chunks of
// kChunk end points staged in LDS (an invalid source is staged at infinity: its d is +inf, which the strict `<` never accepts),
// in ascending j with a strict `<`: the first minimum is kept, so the tie rule needs no cross-lane step.  Every lane of a wave
// reads the SAME LDS address per candidate -- a broadcast, no bank conflict.  Only the winner's vector is fetched from memory.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kInitThreads = 256;
constexpr int kChunk = 1024;          // end points per LDS stage: 8 KB

__global__ void __launch_bounds__(kInitThreads) forward_interpolate_kernel(const float2 *__restrict__ flow, float2 *__restrict__ out,
                                                                          int B, int h, int w) {
    __shared__ float2 ends[kChunk];
    const int M = h * w;
    const int p = (int)blockIdx.x * kInitThreads + (int)threadIdx.x;
    const int ty = p / w, tx = p - ty * w;                    // (a lane past the image computes along and stores nothing)
    const float fx = (float)tx, fy = (float)ty;
    const float fw = (float)w, fh = (float)h;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float2 *src = flow + (int64_t)b * M;
        float best = INFINITY;
        int winner = -1;
        for (int c0 = 0; c0 < M; c0 += kChunk) {
            const int n = min(kChunk, M - c0);
            __syncthreads();                                   // the previous chunk has been read by every wave
            for (int k = threadIdx.x; k < n; k += kInitThreads) {
                const int j = c0 + k;
                const int y0 = j / w, x0 = j - y0 * w;
                const float2 v = src[j];
                const float x1 = __fadd_rn((float)x0, v.x), y1 = __fadd_rn((float)y0, v.y);
                const bool valid = x1 > 0.f && x1 < fw && y1 > 0.f && y1 < fh;
                ends[k] = valid ? make_float2(x1, y1) : make_float2(INFINITY, INFINITY);
            }
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < n; ++k) {
                const float2 e = ends[k];
                const float ex = __fsub_rn(fx, e.x), ey = __fsub_rn(fy, e.y);
                const float d = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                if (d < best) {
                    best = d;
                    winner = c0 + k;
                }
            }
        }
        if (p < M) out[(int64_t)b * M + p] = winner >= 0 ? src[winner] : make_float2(0.f, 0.f);
    }
}

// coords1 = grid + init (ONE float32 addition per component), flow = init and, where the state has one, the third copy of the
// flow: the last two channels of the GRU input x, which the motion encoder's concat([out, flow]) (update.py:106 / 84) reads in the
// first iteration and flow_head.conv2 rewrites in every iteration.  One thread per cell, float2 stores.
__global__ void __launch_bounds__(kInitThreads) warm_start_kernel(const float2 *__restrict__ init, float2 *__restrict__ coords1,
                                                                 float2 *__restrict__ flow, float *__restrict__ x, int ldx,
                                                                 int flow_slot, int64_t cells, int h, int w) {
    const int64_t m = (int64_t)blockIdx.x * kInitThreads + threadIdx.x;
    if (m >= cells) return;
    const int px = (int)(m % w), py = (int)((m / w) % h);
    const float2 f = init[m];
    coords1[m] = make_float2(__fadd_rn((float)px, f.x), __fadd_rn((float)py, f.y));
    flow[m] = f;
    *(float2 *)(x + m * ldx + flow_slot) = f;                 // (ldx and flow_slot are even: 8-byte aligned with x)
}

// what both entries ask of their sizes: positive, and the (B, h, w, 2) tensor below 2^31 elements
int flow_init_sizes(int B, int h, int w) {
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    const int64_t limit = ((int64_t)1 << 31) - 1;
    RAFT_REQUIRE((int64_t)h <= limit / w && (int64_t)B <= limit / ((int64_t)h * w) && (int64_t)B * h * w <= limit / 2, RAFT_E_SHAPE);
    return RAFT_OK;
}

int warm_start(const float *flow_init, int B, int h, int w, const raft_state *st, int ldx, int flow_slot, void *stream) {
    RAFT_REQUIRE_PTR(flow_init);
    RAFT_REQUIRE_PTR(st);
    RAFT_REQUIRE_PTR(st->x);
    RAFT_REQUIRE_PTR(st->coords1);
    RAFT_REQUIRE_PTR(st->flow);
    RAFT_TRY(flow_init_sizes(B, h, w));
    RAFT_REQUIRE(((((uintptr_t)flow_init) | ((uintptr_t)st->coords1) | ((uintptr_t)st->flow) | ((uintptr_t)st->x)) & 7u) == 0, RAFT_E_ALIGN);
    const int64_t cells = (int64_t)B * h * w;
    warm_start_kernel<<<raft_ceil_div(cells, kInitThreads), kInitThreads, 0, (hipStream_t)stream>>>(
        (const float2 *)flow_init, (float2 *)st->coords1, (float2 *)st->flow, st->x, ldx, flow_slot, cells, h, w);
    return raft_launch_status();
}

}   // namespace

extern "C" int raft_forward_interpolate_f32(const float *flow, int B, int h, int w, float *out, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(out);
    RAFT_TRY(flow_init_sizes(B, h, w));
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)out)) & 7u) == 0, RAFT_E_ALIGN);          // read and written as float2
    const uintptr_t bytes = (uintptr_t)B * h * w * 2 * sizeof(float), a = (uintptr_t)flow, o = (uintptr_t)out;
    RAFT_REQUIRE(a + bytes <= o || o + bytes <= a, RAFT_E_UNSUPPORTED);                       // a target reads every source: not in place
    const dim3 grid((unsigned)raft_ceil_div((int64_t)h * w, kInitThreads), (unsigned)(B < 65535 ? B : 65535));
    forward_interpolate_kernel<<<grid, kInitThreads, 0, (hipStream_t)stream>>>((const float2 *)flow, (float2 *)out, B, h, w);
    return raft_launch_status();
}

// x (M, 256) = [inp 128 | motion 126 | flow 2]
extern "C" int raft_warm_start_f32(const float *flow_init, int B, int h, int w, const raft_state *st, void *stream) {
    return warm_start(flow_init, B, h, w, st, 256, 254, stream);
}

// x (M, 160) = [inp 64 | motion 80 | flow 2 | 14 zero pad]
extern "C" int raft_warm_start_small_f32(const float *flow_init, int B, int h, int w, const raft_state *st, void *stream) {
    return warm_start(flow_init, B, h, w, st, 160, 144, stream);
}

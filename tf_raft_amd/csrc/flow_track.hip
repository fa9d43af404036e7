// Following points through a video (no reference counterpart): the flows frame t -> t + 1 of S consecutive
// pairs chained at sub-pixel positions, with the forward-backward test of flow_check.hip at every step, in ONE launch.
//
//   raft_track_points_f32   pos_out[s], lost_out[s] = the state of every point after step s, s = 0 .. S - 1
//
// One step for a point that is tracked (code 0) at (x, y):
//     t1 = sample_taps(x, y)          not in frame (a NaN is not): code 1
//     f  = the forward flow at t1     (bilinear, both components)
//     q  = (x + f.x, y + f.y)         ONE float32 addition each
//     t2 = sample_taps(q)             not in frame: code 1
//     b  = the backward flow at t2    flows_disagree(f, b, alpha, beta): code 2   (only with a backward flow)
//     otherwise the point moves to q
// A nonzero code is sticky: the point keeps the position it was last tracked at and its code, bit for bit, in every later row
// (a position is only ever copied or replaced by q, never recomputed).  A point whose `start` lies beyond the frame a step
// begins at is copied through that step.  Contraction is switched off for this file: every product and sum is rounded on its
// own, so the kernel equals its float32 NumPy restatement (tests/test_flow_track.py) bit for bit.
//
// A pure gather bound by memory latency: the second sample's address depends on the first sample's value, so a step is two
// dependent round trips however it is written, and S steps are 2 S of them.  One thread per point, points numbered n * P + p, so
// a wave reads and writes 64 consecutive positions and codes as runs (512 and 64 bytes) and, for a dense grid under a smooth
// flow, gathers neighbouring vectors; the two taps of a row come as one 16-byte load where W >= 2.  No atomics, no LDS, no
// memset; a thread reads its own point before it writes anything and touches no other point, which is what allows the last row
// of the outputs to BE the inputs (the streaming step, S = 1).
#include "common.h"

#pragma clang fp contract(off)

#include "flow_sample.h"      // Taps, sample_taps, sample_flow, flows_disagree: shared with flow_check.hip

namespace {

constexpr int kTrackThreads = 256;

// (pos_in / pos_out and lost_in / lost_out may alias as described above: no __restrict__ on them)
template <bool PAIR>
__global__ void __launch_bounds__(kTrackThreads) track_points_kernel(const float2 *pos_in, const uint8_t *lost_in,
                                                                     const int32_t *__restrict__ start, int t0,
                                                                     const float2 *__restrict__ flow_forward,
                                                                     const float2 *__restrict__ flow_backward, float2 *pos_out,
                                                                     uint8_t *lost_out, int S, int N, int64_t P, int H, int W,
                                                                     float alpha, float beta) {
    const int64_t NP = (int64_t)N * P;
    const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
    if (i >= NP) return;
    const int64_t HW = (int64_t)H * W, step = (int64_t)N * HW;
    const int64_t image = (int64_t)((int)i / (int)P) * HW;             // the point's video inside one step's flows (N * P < 2^30)
    float2 pos = pos_in[i];
    uint32_t code = lost_in != nullptr ? lost_in[i] : 0u;
    const int64_t first = start != nullptr ? (int64_t)start[i] : 0;    // (t0 >= 0: a point without a start is active at once)
    for (int s = 0; s < S; ++s) {
        if (code == 0u && first <= (int64_t)t0 + s) {
            const Taps t1 = sample_taps(pos.x, pos.y, H, W);
            if (!t1.in) {
                code = 1u;
            } else {
                const float2 f = sample_flow<PAIR>(flow_forward + s * step + image, t1);
                const float qx = pos.x + f.x, qy = pos.y + f.y;
                const Taps t2 = sample_taps(qx, qy, H, W);
                if (!t2.in)
                    code = 1u;
                else if (flow_backward != nullptr && flows_disagree(f, sample_flow<PAIR>(flow_backward + s * step + image, t2), alpha, beta))
                    code = 2u;
                else
                    pos = make_float2(qx, qy);
            }
        }
        pos_out[s * NP + i] = pos;
        lost_out[s * NP + i] = (uint8_t)code;
    }
}

}   // namespace

extern "C" int raft_track_points_f32(const float *pos_in, const uint8_t *lost_in, const int32_t *start, int t0,
                                     const float *flow_forward, const float *flow_backward, float *pos_out, uint8_t *lost_out, int S,
                                     int N, int64_t P, int H, int W, float alpha, float beta, void *stream) {
    RAFT_REQUIRE_PTR(pos_in);
    RAFT_REQUIRE_PTR(flow_forward);
    RAFT_REQUIRE_PTR(pos_out);
    RAFT_REQUIRE_PTR(lost_out);
    RAFT_REQUIRE(S > 0 && N > 0 && P > 0 && H > 0 && W > 0 && t0 >= 0, RAFT_E_SHAPE);
    // fewer than 2^31 elements in the flows (S * N * H * W * 2) and in the positions (S * N * P * 2)
    const int64_t limit = ((int64_t)1 << 31) - 1;
    RAFT_REQUIRE((int64_t)S <= limit / N && (int64_t)S * N <= limit / H && (int64_t)S * N * H <= limit / W &&
                     (int64_t)S * N * H * W <= limit / 2 && P <= limit / 2 / ((int64_t)S * N),
                 RAFT_E_SHAPE);
    RAFT_REQUIRE(alpha >= 0.f && alpha <= 3.402823466e38f && beta >= 0.f && beta <= 3.402823466e38f, RAFT_E_SHAPE);   // (a NaN fails)
    RAFT_REQUIRE(((((uintptr_t)pos_in) | ((uintptr_t)flow_forward) | ((uintptr_t)flow_backward) | ((uintptr_t)pos_out)) & 7u) == 0,
                 RAFT_E_ALIGN);                                        // read and written as float2
    const unsigned grid = (unsigned)(((int64_t)N * P + kTrackThreads - 1) / kTrackThreads);
    hipStream_t st = (hipStream_t)stream;
    const float2 *pi = (const float2 *)pos_in, *ff = (const float2 *)flow_forward, *fb = (const float2 *)flow_backward;
    if (W >= 2)
        track_points_kernel<true><<<grid, kTrackThreads, 0, st>>>(pi, lost_in, start, t0, ff, fb, (float2 *)pos_out, lost_out, S, N, P, H, W, alpha, beta);
    else
        track_points_kernel<false><<<grid, kTrackThreads, 0, st>>>(pi, lost_in, start, t0, ff, fb, (float2 *)pos_out, lost_out, S, N, P, H, W, alpha, beta);
    return raft_launch_status();
}

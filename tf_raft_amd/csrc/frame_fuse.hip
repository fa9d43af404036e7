// Motion-compensated temporal filtering (no reference counterpart): a centre frame fused with K neighbours
// that are aligned onto it along flows and averaged robustly -- video denoising, burst fusion -- in ONE launch.
//
//   raft_fuse_frames_f32      float32 frames -> float32
//   raft_fuse_frames_u8_f32   uint8 frames   -> float32
//   raft_fuse_frames_u8       uint8 frames   -> uint8 (rintf, half to even, then clamped to 0 .. 255)
//
// Per pixel p = (x, y) of slice n and neighbour k, in float32, every product, sum and quotient rounded on its own:
//     t        = absolute ? sample_taps(vector) : flow_taps(x, y, vector)           (flow_sample.h; a NaN is not in frame)
//     vis_k(p) = t.in && (skip == NULL || skip[k, n, p] == 0)
//     c_k[ch]  = bilinear(t, the four taps of neighbour k, channel ch)             (uint8 taps converted to float first)
//     q_k(p)   = sum over ch = 0 .. C - 1, in order, of d * d, d = center[ch] - c_k[ch];  0.f where !vis_k(p)
//     D, cnt   = sum of q_k(p') and count of p' over the window p' = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r inner,
//                over the p' that are in the frame and have vis_k(p')
//     m        = D / (float)(cnt * C)
//     w_k(p)   = vis_k(p) ? s2 / (s2 + m) : 0.f,   s2 = sigma * sigma               (Cauchy, one division)
//   num[ch] = center_weight * center[ch], den = center_weight;  for k = 0 .. K - 1 in order: num[ch] = num[ch] + w_k * c_k[ch],
//   den = den + w_k;  dst[ch] = num[ch] / den, weight = den.
// q_k is a sum of squares, so it is +0 or larger (or a NaN): adding the 0.f of a window entry that does not count changes no bit,
// and the kernel adds ALL (2r + 1)^2 entries of a window in the order above.  No transcendental function appears and contraction
// is switched off for this file, so the kernel equals its float32 NumPy restatement (tests/test_frame_fuse.py) bit for bit.
//
// Structure.  One workgroup of 256 threads owns a 32 x 8 tile of output pixels of one slice, one thread per pixel, and walks the
// K neighbours in order.  For neighbour k every thread gathers its OWN pixel (vector, skip byte, 4 taps x C channels), keeps c_k in
// registers and puts (q_k, vis_k) into LDS; the ring of r pixels around the tile ((32 + 2r)(8 + 2r) - 256 positions: 84, 176, 276
// for r = 1, 2, 3) is gathered by the first threads of the workgroup, q and vis only.  After ONE barrier every thread adds the
// (2r + 1)^2 entries of its window from LDS (8-byte entries: q and vis as 1.f / 0.f, so cnt is an exact float sum), forms w_k and
// accumulates.  The LDS tile is double-buffered over (slice, neighbour) steps, so a step's writes can only meet the reads of the
// step before the previous barrier: one barrier per neighbour.  r == 0 is a template case without LDS and without a barrier.
// Two things the measurements paid for (docs/NOTEBOOK.md section 40): a position's vector and skip byte of neighbour k + 1 are
// read while neighbour k is gathered, so a step waits for one round trip, not two; and the two taps of a row come as one read of
// 2 C elements (PAIR, as sample_flow<PAIR> reads flows; W >= 2), unaligned for uint8 pixels.  A thread's ring positions do not
// depend on the slice or the neighbour and are worked out once.
// No workspace, no atomics, no memset; every output element is written exactly once; neighbours are addressed by element offsets
// that travel by value in the kernel arguments, so a window of a device video is fused where it lies.
#include "common.h"

#pragma clang fp contract(off)

#include "flow_sample.h"      // Taps, sample_taps, flow_taps, bilinear

namespace {

constexpr int kFuseTileW = 32, kFuseTileH = 8, kFuseThreads = kFuseTileW * kFuseTileH;
constexpr int kFuseMaxNeighbours = 16, kFuseMaxRadius = 3, kFuseMaxChannels = 4;

struct FuseOffsets {
    int64_t off[kFuseMaxNeighbours];      // element offset of neighbour k's (N, H, W, C) block from the base pointer
};

// What a pixel knows of neighbour k before it gathers: its vector and whether it is skipped.  The kernel reads neighbour k + 1's
// while it works on neighbour k, so that the taps, whose addresses depend on the vector, are the only round trip of a step.
struct FuseVector {
    float2 f;
    bool skipped;
};

__device__ __forceinline__ FuseVector fuse_vector(const float2 *__restrict__ vectors, const uint8_t *__restrict__ skip, int64_t i) {
    FuseVector v;
    v.f = vectors[i];
    v.skipped = skip != nullptr && skip[i] != 0;
    return v;
}

// The gather of one pixel for one neighbour: c[ch], q and vis of the definition above.  `nb` points at slice n of neighbour k,
// `cen` holds the centre's pixel, (x, y) lies in the frame.
// two neighbouring pixels of a row, read together (PAIR)
template <typename S, int C>
struct alignas(alignof(S)) FusePixels {
    S v[2 * C];
};

// PAIR: the two taps of a row are neighbours in memory and come as ONE read of 2 C elements from the first of them (from the
// pixel before where the first is the row's last pixel, whose right neighbour is itself), as sample_flow<PAIR> reads flows;
// needs W >= 2.  uint8 pixels lie at any address: the read is then an unaligned one.
template <typename S, int C, bool PAIR>
__device__ __forceinline__ void fuse_gather(const S *__restrict__ nb, const FuseVector &vk, const float (&cen)[C], int absolute, int x,
                                            int y, int H, int W, float (&c)[C], float &q, bool &vis) {
    const Taps t = absolute ? sample_taps(vk.f.x, vk.f.y, H, W) : flow_taps(x, y, vk.f, H, W);
    float v[C][4];
    if (PAIR) {
        const int col = t.o01 - t.o00;                   // 1, or 0 where x0 is the row's last pixel
        FusePixels<S, C> r0, r1;
        __builtin_memcpy(&r0, nb + (t.o00 + col - 1) * C, sizeof(r0));
        __builtin_memcpy(&r1, nb + (t.o10 + col - 1) * C, sizeof(r1));
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            v[ch][0] = (float)(col ? r0.v[ch] : r0.v[C + ch]);
            v[ch][1] = (float)r0.v[C + ch];
            v[ch][2] = (float)(col ? r1.v[ch] : r1.v[C + ch]);
            v[ch][3] = (float)r1.v[C + ch];
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            v[ch][0] = (float)nb[t.o00 * C + ch];
            v[ch][1] = (float)nb[t.o01 * C + ch];
            v[ch][2] = (float)nb[t.o10 * C + ch];
            v[ch][3] = (float)nb[t.o11 * C + ch];
        }
    }
    vis = t.in && !vk.skipped;
    float sum = 0.f;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        c[ch] = bilinear(t, v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
        const float d = cen[ch] - c[ch];
        sum = ch == 0 ? d * d : sum + d * d;
    }
    q = vis ? sum : 0.f;
}

__device__ __forceinline__ void fuse_store(float *out, float v) { *out = v; }
__device__ __forceinline__ void fuse_store(uint8_t *out, float v) { *out = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f); }

template <typename S, typename D, int C, int R, bool PAIR>
__global__ void __launch_bounds__(kFuseThreads) fuse_frames_kernel(const S *__restrict__ center, const S *__restrict__ neighbours,
                                                                   const FuseOffsets index, const float2 *__restrict__ vectors,
                                                                   const uint8_t *__restrict__ skip, D *__restrict__ dst,
                                                                   float *__restrict__ weight, int K, int N, int H, int W, int absolute,
                                                                   float s2, float center_weight) {
    constexpr int LW = kFuseTileW + 2 * R, LH = kFuseTileH + 2 * R, RING = LW * LH - kFuseThreads;
    constexpr int NR = (RING + kFuseThreads - 1) / kFuseThreads;      // ring positions of a thread: 0 (R == 0), 1 or 2
    constexpr int NRA = NR > 0 ? NR : 1;
    __shared__ float2 tile[R > 0 ? 2 : 1][R > 0 ? LW * LH : 1];       // (q, vis as 1.f / 0.f) of the tile and its ring
    const int tid = (int)threadIdx.x, tx = tid & (kFuseTileW - 1), ty = tid / kFuseTileW;
    const int x0 = (int)blockIdx.x * kFuseTileW, y0 = (int)blockIdx.y * kFuseTileH;
    const int x = x0 + tx, y = y0 + ty, HW = H * W, p = y * W + x;
    const bool inside = x < W && y < H;
    // the thread's ring positions, the same for every slice and neighbour: R rows above the tile, R below, then R columns each side
    int ring_l[NRA], ring_x[NRA], ring_y[NRA];                        // LDS entry (-1: none) and frame coordinates
    bool ring_in[NRA];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int i = tid + j * kFuseThreads;
        int ly = 0, lx = 0;
        if (i < 2 * R * LW) {
            const int row = i / LW;
            lx = i - row * LW, ly = row < R ? row : row + kFuseTileH;
        } else {
            const int r2 = R > 0 ? 2 * R : 1, e = i - 2 * R * LW, row = e / r2, col = e - row * r2;
            ly = row + R, lx = col < R ? col : col + kFuseTileW;
        }
        ring_l[j] = i < RING ? ly * LW + lx : -1;
        ring_x[j] = x0 + lx - R, ring_y[j] = y0 + ly - R;
        ring_in[j] = i < RING && ring_x[j] >= 0 && ring_x[j] < W && ring_y[j] >= 0 && ring_y[j] < H;
    }
    unsigned step = 0;                                                // which LDS buffer: counts (slice, neighbour) steps
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const int64_t image = (int64_t)n * HW;
        const S *centre = center + image * C;
        float cen[C], ring_cen[NRA][C], num[C], den = center_weight;
        FuseVector next, ring_next[NRA];
        next.f = make_float2(0.f, 0.f), next.skipped = true;
        if (inside) next = fuse_vector(vectors, skip, image + p);     // (neighbour 0's plane of slice n starts at n * HW)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            ring_next[j] = next;
            if (ring_in[j]) ring_next[j] = fuse_vector(vectors, skip, image + ring_y[j] * W + ring_x[j]);
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            cen[ch] = inside ? (float)centre[p * C + ch] : 0.f;
            num[ch] = center_weight * cen[ch];
#pragma unroll
            for (int j = 0; j < NR; ++j) ring_cen[j][ch] = ring_in[j] ? (float)centre[(ring_y[j] * W + ring_x[j]) * C + ch] : 0.f;
        }
        for (int k = 0; k < K; ++k, ++step) {
            const S *nb = neighbours + index.off[k] + image * C;
            const FuseVector cur = next;
            FuseVector ring_cur[NRA];
#pragma unroll
            for (int j = 0; j < NR; ++j) ring_cur[j] = ring_next[j];
            if (k + 1 < K) {                                          // neighbour k + 1's vectors travel while k is gathered
                const int64_t plane = ((int64_t)(k + 1) * N + n) * HW;
                if (inside) next = fuse_vector(vectors, skip, plane + p);
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (ring_in[j]) ring_next[j] = fuse_vector(vectors, skip, plane + ring_y[j] * W + ring_x[j]);
            }
            float c[C], q = 0.f, m;
            bool vis = false;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) c[ch] = 0.f;
            if (inside) fuse_gather<S, C, PAIR>(nb, cur, cen, absolute, x, y, H, W, c, q, vis);
            if constexpr (R > 0) {
                float2 *buf = tile[step & 1u];
                buf[(ty + R) * LW + tx + R] = make_float2(q, vis ? 1.f : 0.f);
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    float hq = 0.f;
                    bool hv = false;
                    if (ring_in[j]) {
                        float hc[C];
                        fuse_gather<S, C, PAIR>(nb, ring_cur[j], ring_cen[j], absolute, ring_x[j], ring_y[j], H, W, hc, hq, hv);
                    }
                    if (ring_l[j] >= 0) buf[ring_l[j]] = make_float2(hq, hv ? 1.f : 0.f);
                }
                __syncthreads();
                float sum = 0.f, cnt = 0.f;
#pragma unroll
                for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; ++dx) {
                        const float2 e = buf[(ty + dy) * LW + tx + dx];
                        sum = sum + e.x, cnt = cnt + e.y;
                    }
                m = sum / (cnt * (float)C);
            } else {
                m = q / (float)C;
            }
            const float w = vis ? s2 / (s2 + m) : 0.f;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) num[ch] = num[ch] + w * c[ch];
            den = den + w;
        }
        if (inside) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) fuse_store(dst + (image + p) * C + ch, num[ch] / den);
            if (weight != nullptr) weight[image + p] = den;
        }
    }
}

bool fuse_overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

template <typename S, typename D, int C, bool PAIR>
void fuse_launch_radius(dim3 grid, hipStream_t st, int R, const S *center, const S *neighbours, const FuseOffsets &index,
                        const float2 *vectors, const uint8_t *skip, D *dst, float *weight, int K, int N, int H, int W, int absolute,
                        float s2, float cw) {
    switch (R) {
        case 0: fuse_frames_kernel<S, D, C, 0, PAIR><<<grid, kFuseThreads, 0, st>>>(center, neighbours, index, vectors, skip, dst, weight, K, N, H, W, absolute, s2, cw); break;
        case 1: fuse_frames_kernel<S, D, C, 1, PAIR><<<grid, kFuseThreads, 0, st>>>(center, neighbours, index, vectors, skip, dst, weight, K, N, H, W, absolute, s2, cw); break;
        case 2: fuse_frames_kernel<S, D, C, 2, PAIR><<<grid, kFuseThreads, 0, st>>>(center, neighbours, index, vectors, skip, dst, weight, K, N, H, W, absolute, s2, cw); break;
        default: fuse_frames_kernel<S, D, C, 3, PAIR><<<grid, kFuseThreads, 0, st>>>(center, neighbours, index, vectors, skip, dst, weight, K, N, H, W, absolute, s2, cw); break;
    }
}

template <typename S, typename D, int C>
void fuse_launch_pair(dim3 grid, hipStream_t st, int R, const S *center, const S *neighbours, const FuseOffsets &index,
                      const float2 *vectors, const uint8_t *skip, D *dst, float *weight, int K, int N, int H, int W, int absolute,
                      float s2, float cw) {
    if (W >= 2)
        fuse_launch_radius<S, D, C, true>(grid, st, R, center, neighbours, index, vectors, skip, dst, weight, K, N, H, W, absolute, s2, cw);
    else
        fuse_launch_radius<S, D, C, false>(grid, st, R, center, neighbours, index, vectors, skip, dst, weight, K, N, H, W, absolute, s2, cw);
}

template <typename S, typename D>
int fuse_frames(const S *center, const S *neighbours, const int64_t *index, const float *vectors, const uint8_t *skip, int absolute,
                float sigma, float center_weight, int patch_radius, D *dst, float *weight, int K, int N, int H, int W, int C,
                void *stream) {
    RAFT_REQUIRE_PTR(center);
    RAFT_REQUIRE_PTR(neighbours);
    RAFT_REQUIRE_PTR(vectors);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE(K >= 1 && K <= kFuseMaxNeighbours && N > 0 && H > 0 && W > 0 && C >= 1 && C <= kFuseMaxChannels, RAFT_E_SHAPE);
    RAFT_REQUIRE(patch_radius >= 0 && patch_radius <= kFuseMaxRadius && (absolute == 0 || absolute == 1), RAFT_E_SHAPE);
    // fewer than 2^31 elements in one frame batch (N * H * W * 4) and in the vectors (K * N * H * W * 2)
    const int64_t limit = ((int64_t)1 << 31) - 1;
    RAFT_REQUIRE((int64_t)N <= limit / H && (int64_t)N * H <= limit / W && (int64_t)N * H * W <= limit / (2 * kFuseMaxNeighbours), RAFT_E_SHAPE);
    const float s2 = sigma * sigma;
    RAFT_REQUIRE(sigma > 0.f && s2 > 0.f && s2 <= 3.402823466e38f, RAFT_E_SHAPE);                       // (a NaN fails)
    RAFT_REQUIRE(center_weight > 0.f && center_weight <= 3.402823466e38f, RAFT_E_SHAPE);
    const int64_t frame = (int64_t)N * H * W * C;                      // elements of one (N, H, W, C) block
    FuseOffsets offsets;
    for (int k = 0; k < kFuseMaxNeighbours; ++k) {
        const int64_t i = k >= K ? 0 : index != nullptr ? index[k] : (int64_t)k;
        RAFT_REQUIRE(i >= 0 && i <= (((int64_t)1 << 60) / frame), RAFT_E_SHAPE);
        offsets.off[k] = i * frame;
    }
    RAFT_REQUIRE((((uintptr_t)vectors) & 7u) == 0, RAFT_E_ALIGN);      // read as float2
    RAFT_REQUIRE((((uintptr_t)center) | ((uintptr_t)neighbours)) % sizeof(S) == 0 && ((uintptr_t)dst) % sizeof(D) == 0 &&
                     (((uintptr_t)weight) & 3u) == 0,
                 RAFT_E_ALIGN);
    // windows read neighbouring pixels: an output may not lie on any input
    const int64_t planes = (int64_t)K * N * H * W;
    const void *outs[2] = {dst, weight};
    const int64_t out_bytes[2] = {frame * (int64_t)sizeof(D), (int64_t)N * H * W * 4};
    for (int o = 0; o < 2; ++o) {
        if (outs[o] == nullptr) continue;
        bool hit = fuse_overlap(outs[o], out_bytes[o], center, frame * (int64_t)sizeof(S)) ||
                   fuse_overlap(outs[o], out_bytes[o], vectors, planes * 8) ||
                   (skip != nullptr && fuse_overlap(outs[o], out_bytes[o], skip, planes));
        for (int k = 0; k < K; ++k) hit = hit || fuse_overlap(outs[o], out_bytes[o], neighbours + offsets.off[k], frame * (int64_t)sizeof(S));
        RAFT_REQUIRE(!hit, RAFT_E_SHAPE);
    }
    RAFT_REQUIRE(weight == nullptr || !fuse_overlap(dst, out_bytes[0], weight, out_bytes[1]), RAFT_E_SHAPE);
    const dim3 grid((unsigned)raft_ceil_div(W, kFuseTileW), (unsigned)raft_ceil_div(H, kFuseTileH), (unsigned)(N < 65535 ? N : 65535));
    RAFT_REQUIRE(grid.y <= 65535u, RAFT_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    const float2 *v = (const float2 *)vectors;
    switch (C) {
        case 1: fuse_launch_pair<S, D, 1>(grid, st, patch_radius, center, neighbours, offsets, v, skip, dst, weight, K, N, H, W, absolute, s2, center_weight); break;
        case 2: fuse_launch_pair<S, D, 2>(grid, st, patch_radius, center, neighbours, offsets, v, skip, dst, weight, K, N, H, W, absolute, s2, center_weight); break;
        case 3: fuse_launch_pair<S, D, 3>(grid, st, patch_radius, center, neighbours, offsets, v, skip, dst, weight, K, N, H, W, absolute, s2, center_weight); break;
        default: fuse_launch_pair<S, D, 4>(grid, st, patch_radius, center, neighbours, offsets, v, skip, dst, weight, K, N, H, W, absolute, s2, center_weight); break;
    }
    return raft_launch_status();
}

}   // namespace

extern "C" int raft_fuse_frames_f32(const float *center, const float *neighbours, const int64_t *index, const float *vectors,
                                    const uint8_t *skip, int absolute, float sigma, float center_weight, int patch_radius, float *dst,
                                    float *weight, int K, int N, int H, int W, int C, void *stream) {
    return fuse_frames<float, float>(center, neighbours, index, vectors, skip, absolute, sigma, center_weight, patch_radius, dst, weight, K, N, H, W, C, stream);
}

extern "C" int raft_fuse_frames_u8_f32(const uint8_t *center, const uint8_t *neighbours, const int64_t *index, const float *vectors,
                                       const uint8_t *skip, int absolute, float sigma, float center_weight, int patch_radius, float *dst,
                                       float *weight, int K, int N, int H, int W, int C, void *stream) {
    return fuse_frames<uint8_t, float>(center, neighbours, index, vectors, skip, absolute, sigma, center_weight, patch_radius, dst, weight, K, N, H, W, C, stream);
}

extern "C" int raft_fuse_frames_u8(const uint8_t *center, const uint8_t *neighbours, const int64_t *index, const float *vectors,
                                   const uint8_t *skip, int absolute, float sigma, float center_weight, int patch_radius, uint8_t *dst,
                                   float *weight, int K, int N, int H, int W, int C, void *stream) {
    return fuse_frames<uint8_t, uint8_t>(center, neighbours, index, vectors, skip, absolute, sigma, center_weight, patch_radius, dst, weight, K, N, H, W, C, stream);
}

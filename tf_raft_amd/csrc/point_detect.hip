// Corner detection and re-seeding for the point tracker (no reference counterpart): "good features to
// track" on the device, so that a tracker can start on its own and fill the slots it loses.
//
//   raft_corner_score_f32 / _u8_f32   the score map (N, H, W) and its per-image maximum
//   raft_detect_points                score, non-maximum suppression, candidates, top-K: points strongest first
//   raft_refill_points                new points into the lost slots of a tracker's state, ids and birth frames kept
//
// The arithmetic is written down once in include/raft_hip.h and restated in float32 NumPy in tests/test_point_detect.py.
// Contraction is switched off for this file: every product, sum and the square root are rounded on their own, so the score map
// equals the restatement bit for bit, and everything behind it works on the score's BITS (a non-negative float orders like its
// bit pattern), which has no rounding at all.
//
// Launches of raft_detect_points, all on `stream`:
//   0. the counters (and, with `avoid`, the occupancy map) are zeroed (hipMemsetAsync);
//   1. corner_score_kernel: a 32 x 16 tile per workgroup.  The gray tile with a ring of block_radius + 1 goes to LDS once, the
//      Sobel products gx gx, gx gy, gy gy with a ring of block_radius next to it, then the HORIZONTAL window sums (each window row
//      left to right) are formed once and shared between the vertically adjacent pixels, which add them top to bottom.  The
//      per-image maximum is an atomicMax over the score's bits: a maximum does not depend on the order.
//   2. stamp_kernel (only with `avoid`): every live point that lies in the frame writes the constant 1 over its
//      (2 min_distance + 1)^2 window of the occupancy map.  Every writer writes the same value: the scatter is deterministic.
//   3. nms_candidates_kernel: a 32 x 16 tile of 64-bit keys (score bits << 32 | 0xFFFFFFFF - raster index) with a ring of
//      min_distance in LDS, the window maximum taken separably (row maxima, then column maxima).  A pixel is a local maximum iff
//      the window's maximum is its own key; keys are unique within an image, so ties need no rule beyond the key itself.  Threshold,
//      mask and occupancy are applied AFTER the suppression.  Candidates are appended through an atomic slot counter (a workgroup
//      reserves the slots of its tile with one atomic), so their order in the list differs from run to run -- and that is
//      allowed, because
//   4. select_kernel takes the max_points LARGEST keys and SORTS them: keys are unique, the candidates of an image are a SET, and
//      the sorted top-K of a set is the same bits whatever order the set was gathered in.  One workgroup per image: with more
//      candidates than K a radix select over the keys (eight 8-bit digits, LDS histograms of integer counts) finds the K-th
//      largest key, the keys at or above it are gathered into LDS (again in any order), and one bitonic sort orders them.
//      Any two local maxima are more than min_distance apart (Chebyshev), so an image has at most
//      ceil(H / (m + 1)) * ceil(W / (m + 1)) of them: the candidate list has exactly that many slots and cannot overflow.
//
// raft_refill_points is one launch, one workgroup per video: an ordered prefix scan over the slots ranks the lost ones, rank r
// takes new point r.  No atomics; a thread reads its own slot before it writes it, so it may run in place.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 16;                  // pixels of a workgroup (two per thread)
constexpr int kMaxBlockRadius = 3;
constexpr int kMaxMinDistance = RAFT_DETECT_MAX_MIN_DISTANCE;
constexpr int kMaxPoints = RAFT_DETECT_MAX_POINTS;
constexpr int kSelectThreads = 1024;
constexpr int kMaxGridZ = 65535;

// Element i = tid, tid + kThreads, ... of a row-major region `w` wide as (y, x), without a division per element.
struct Walk {
    int y, x, w, dq, dr;
    __device__ __forceinline__ Walk(int tid, int width) : y(tid / width), x(tid - (tid / width) * width), w(width), dq(kThreads / width),
                                                          dr(kThreads - (kThreads / width) * width) {}
    __device__ __forceinline__ void next() {
        x += dr, y += dq;
        if (x >= w) x -= w, ++y;
    }
};

template <int C>
__device__ __forceinline__ float gray_at(const float *__restrict__ p) {
    return C == 1 ? p[0] : (0.299f * p[0] + 0.587f * p[1]) + 0.114f * p[2];      // warped_gray.h's formula
}
template <int C>
__device__ __forceinline__ float gray_at(const uint8_t *__restrict__ p) {
    return C == 1 ? (float)p[0] : (0.299f * (float)p[0] + 0.587f * (float)p[1]) + 0.114f * (float)p[2];
}

// ---------------------------------------------------------------- launch 1: the score map
template <typename T, int C>
__global__ void __launch_bounds__(kThreads) corner_score_kernel(const T *__restrict__ frames, float *__restrict__ score,
                                                                uint32_t *__restrict__ smax, int N, int H, int W, int r,
                                                                int harris, float k, int border) {
    constexpr int GW = kTileW + 2 * kMaxBlockRadius + 2, GH = kTileH + 2 * kMaxBlockRadius + 2;
    constexpr int DW = kTileW + 2 * kMaxBlockRadius, DH = kTileH + 2 * kMaxBlockRadius;
    __shared__ float g[GH * GW];
    __shared__ float pxx[DH * DW], pxy[DH * DW], pyy[DH * DW];
    __shared__ float hxx[DH * kTileW], hxy[DH * kTileW], hyy[DH * kTileW];
    __shared__ uint32_t bmax;
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int gw = kTileW + 2 * r + 2, gh = kTileH + 2 * r + 2, dw = kTileW + 2 * r, dh = kTileH + 2 * r, n_win = 2 * r + 1;
    const int64_t HW = (int64_t)H * W;
    for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
        const T *img = frames + (int64_t)n * HW * C;
        if (tid == 0) bmax = 0u;
        // the gray tile with its ring; outside the frame 0 (no scored pixel's stencil reaches there)
        Walk wg(tid, gw);
        for (int i = tid; i < gw * gh; i += kThreads, wg.next()) {
            const int ly = wg.y, lx = wg.x;
            const int y = y0 - r - 1 + ly, x = x0 - r - 1 + lx;
            g[ly * GW + lx] = (y >= 0 && y < H && x >= 0 && x < W) ? gray_at<C>(img + ((int64_t)y * W + x) * C) : 0.f;
        }
        __syncthreads();
        // Sobel derivatives and their three products
        Walk wd(tid, dw);
        for (int i = tid; i < dw * dh; i += kThreads, wd.next()) {
            const int ly = wd.y, lx = wd.x;
            const float *q = g + ly * GW + lx;
            const float tl = q[0], tm = q[1], tr = q[2], ml = q[GW], mr = q[GW + 2], bl = q[2 * GW], bm = q[2 * GW + 1], br = q[2 * GW + 2];
            const float gx = ((tr - tl) + 2.f * (mr - ml)) + (br - bl);
            const float gy = ((bl - tl) + 2.f * (bm - tm)) + (br - tr);
            pxx[ly * DW + lx] = gx * gx;
            pxy[ly * DW + lx] = gx * gy;
            pyy[ly * DW + lx] = gy * gy;
        }
        __syncthreads();
        // each window row left to right, once per row of the tile and its ring
        for (int i = tid; i < kTileW * dh; i += kThreads) {
            const int ly = i / kTileW, lx = i - ly * kTileW;
            const int at = ly * DW + lx;
            float a = pxx[at], b = pxy[at], c = pyy[at];
            for (int j = 1; j < n_win; ++j) {
                a = a + pxx[at + j];
                b = b + pxy[at + j];
                c = c + pyy[at + j];
            }
            hxx[i] = a, hxy[i] = b, hyy[i] = c;
        }
        __syncthreads();
        // the rows' sums top to bottom, the response, the score
        uint32_t best = 0u;
        for (int i = tid; i < kTileW * kTileH; i += kThreads) {
            const int ly = i / kTileW, lx = i - ly * kTileW;
            const int y = y0 + ly, x = x0 + lx;
            if (y >= H || x >= W) continue;
            float out = 0.f;
            if (x >= border && x < W - border && y >= border && y < H - border) {
                float a = hxx[i], b = hxy[i], c = hyy[i];
                for (int j = 1; j < n_win; ++j) {
                    a = a + hxx[i + j * kTileW];
                    b = b + hxy[i + j * kTileW];
                    c = c + hyy[i + j * kTileW];
                }
                float s;
                if (harris) {
                    const float tr = a + c;
                    s = (a * c - b * b) - k * (tr * tr);
                } else {
                    const float d = a - c;
                    s = ((a + c) - sqrtf(d * d + 4.f * (b * b))) * 0.5f;       // (a division by 2, exactly)
                }
                out = s > 0.f ? s : 0.f;                                        // a NaN or a negative response is 0
            }
            score[(int64_t)n * HW + (int64_t)y * W + x] = out;
            const uint32_t bits = __float_as_uint(out);
            best = bits > best ? bits : best;
        }
        if (smax != nullptr) {
            if (best != 0u) atomicMax(&bmax, best);
            __syncthreads();
            if (tid == 0 && bmax != 0u) atomicMax(smax + n, bmax);
        }
        __syncthreads();                                  // (the tiles and bmax are rewritten for the next image)
    }
}

// ---------------------------------------------------------------- launch 2: the occupancy map of `avoid`
__global__ void __launch_bounds__(kThreads) stamp_kernel(const float *__restrict__ pts, const uint8_t *__restrict__ lost,
                                                         uint8_t *__restrict__ occ, int N, int64_t P, int H, int W, int m) {
    const int rows = 2 * m + 1;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)N * P * rows) return;
    const int64_t pt = i / rows;
    const int row = (int)(i - pt * rows);
    if (lost[pt] != 0) return;
    const float px = pts[2 * pt], py = pts[2 * pt + 1];
    if (!(px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1))) return;      // (a NaN stamps nothing)
    const float fm = (float)m;
    const int xa = (int)ceilf(px - fm), xb = (int)floorf(px + fm), ya = (int)ceilf(py - fm), yb = (int)floorf(py + fm);
    const int y = ya + row;
    if (y < 0 || y > yb || y >= H) return;
    const int xs = xa < 0 ? 0 : xa, xe = xb > W - 1 ? W - 1 : xb;
    uint8_t *dst = occ + (pt / P) * ((int64_t)H * W) + (int64_t)y * W;
    for (int x = xs; x <= xe; ++x) dst[x] = 1;
}

// ---------------------------------------------------------------- launch 3: suppression and candidates
__global__ void __launch_bounds__(kThreads) nms_candidates_kernel(const float *__restrict__ score, const uint32_t *__restrict__ smax,
                                                                  const uint8_t *__restrict__ mask, const uint8_t *__restrict__ occ,
                                                                  u64 *__restrict__ cand, uint32_t *__restrict__ cand_count, int N,
                                                                  int H, int W, int m, float quality, uint32_t bound) {
    constexpr int KW = kTileW + 2 * kMaxMinDistance, KH = kTileH + 2 * kMaxMinDistance;
    __shared__ u64 key[KH * KW];
    __shared__ u64 rowmax[KH * kTileW];
    __shared__ uint32_t s_n, s_base;
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int kw = kTileW + 2 * m, kh = kTileH + 2 * m, n_win = 2 * m + 1;
    const int64_t HW = (int64_t)H * W;
    for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
        const float *sc = score + (int64_t)n * HW;
        // outside the frame the key is 0, below every key of a pixel: the window is clipped to the frame
        if (tid == 0) s_n = 0u;
        Walk wk(tid, kw);
        for (int i = tid; i < kw * kh; i += kThreads, wk.next()) {
            const int ly = wk.y, lx = wk.x;
            const int y = y0 - m + ly, x = x0 - m + lx;
            u64 v = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const uint32_t idx = (uint32_t)((int64_t)y * W + x);
                v = ((u64)__float_as_uint(sc[idx]) << 32) | (u64)(0xFFFFFFFFu - idx);
            }
            key[ly * KW + lx] = v;
        }
        __syncthreads();
        for (int i = tid; i < kTileW * kh; i += kThreads) {
            const int ly = i / kTileW, lx = i - ly * kTileW;
            const u64 *q = key + ly * KW + lx;
            u64 v = q[0];
            for (int j = 1; j < n_win; ++j) v = q[j] > v ? q[j] : v;
            rowmax[i] = v;
        }
        __syncthreads();
        const float thr = quality * __uint_as_float(smax[n]);
        constexpr int kMine = kTileW * kTileH / kThreads;                      // pixels of a thread
        u64 mine[kMine];                                                        // its candidates' keys (0: none; a key is never 0)
        uint32_t n_mine = 0u;
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int i = tid + k * kThreads;
            const int ly = i / kTileW, lx = i - ly * kTileW;
            const int y = y0 + ly, x = x0 + lx;
            mine[k] = 0;
            if (y >= H || x >= W) continue;
            const u64 own = key[(ly + m) * KW + lx + m];
            const float s = __uint_as_float((uint32_t)(own >> 32));
            if (!(s > 0.f && s >= thr)) continue;
            u64 v = rowmax[i];
            for (int j = 1; j < n_win; ++j) v = rowmax[i + j * kTileW] > v ? rowmax[i + j * kTileW] : v;
            if (v != own) continue;                                             // suppressed
            const int64_t at = (int64_t)n * HW + (int64_t)y * W + x;
            if (mask != nullptr && mask[at] == 0) continue;
            if (occ != nullptr && occ[at] != 0) continue;
            mine[k] = own;
            ++n_mine;
        }
        // ONE global atomic per workgroup reserves the slots of its candidates (an atomic per candidate on the image's one
        // counter serialises: docs/NOTEBOOK.md section 42)
        const uint32_t first = n_mine != 0u ? atomicAdd(&s_n, n_mine) : 0u;
        __syncthreads();
        if (tid == 0 && s_n != 0u) s_base = atomicAdd(cand_count + n, s_n);
        __syncthreads();
        uint32_t slot = s_base + first;
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            if (mine[k] == 0) continue;
            if (slot < bound) cand[(int64_t)n * bound + slot] = mine[k];       // (always: the bound is exact)
            ++slot;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- launch 4: the K largest keys, sorted
__global__ void __launch_bounds__(kSelectThreads) select_kernel(const u64 *__restrict__ cand, const uint32_t *__restrict__ cand_count,
                                                                uint32_t bound, int K, int W, float *__restrict__ points,
                                                                float *__restrict__ scores, int32_t *__restrict__ count,
                                                                uint8_t *__restrict__ lost) {
    __shared__ u64 keys[kMaxPoints];
    __shared__ uint32_t hist[256];
    __shared__ u64 s_prefix;
    __shared__ uint32_t s_remaining, s_fill;
    const int tid = (int)threadIdx.x;
    const int n = (int)blockIdx.x;
    const u64 *src = cand + (int64_t)n * bound;
    uint32_t c = cand_count[n];
    c = c < bound ? c : bound;
    const int kept = c < (uint32_t)K ? (int)c : K;
    int n2 = 1;
    while (n2 < kept) n2 <<= 1;                                                 // (<= kMaxPoints)
    if (c <= (uint32_t)K) {
        for (int i = tid; i < n2; i += kSelectThreads) keys[i] = (uint32_t)i < c ? src[i] : 0;
    } else {
        // the K-th largest key, digit by digit from the top: `prefix` holds the digits found so far, `remaining` the rank asked
        // for among the keys that share them
        u64 prefix = 0, known = 0;
        uint32_t remaining = (uint32_t)K;
        for (int d = 7; d >= 0; --d) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            for (uint32_t i = (uint32_t)tid; i < c; i += kSelectThreads) {
                const u64 v = src[i];
                if ((v & known) == prefix) atomicAdd(&hist[(uint32_t)(v >> (8 * d)) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t above = 0u;
                int b = 255;
                while (b > 0 && above + hist[b] < remaining) above += hist[b--];
                s_prefix = prefix | ((u64)b << (8 * d));
                s_remaining = remaining - above;
            }
            __syncthreads();
            prefix = s_prefix, remaining = s_remaining;
            known |= (u64)255 << (8 * d);
        }
        if (tid == 0) s_fill = 0u;
        __syncthreads();
        for (uint32_t i = (uint32_t)tid; i < c; i += kSelectThreads) {
            const u64 v = src[i];
            if (v >= prefix) {
                const uint32_t slot = atomicAdd(&s_fill, 1u);                   // (any order: the sort below decides)
                if (slot < (uint32_t)kMaxPoints) keys[slot] = v;
            }
        }
        for (int i = K + tid; i < n2; i += kSelectThreads) keys[i] = 0;
    }
    __syncthreads();
    // bitonic sort, largest first
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += kSelectThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 a = keys[i], b = keys[l];
                    if (((i & k) == 0) ? a < b : a > b) keys[i] = b, keys[l] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < K; i += kSelectThreads) {
        float x = -1.f, y = -1.f, s = 0.f;
        if (i < kept) {
            const u64 v = keys[i];
            const uint32_t idx = 0xFFFFFFFFu - (uint32_t)v;
            const uint32_t yy = idx / (uint32_t)W;
            x = (float)(idx - yy * (uint32_t)W), y = (float)yy, s = __uint_as_float((uint32_t)(v >> 32));
        }
        const int64_t at = (int64_t)n * K + i;
        points[2 * at] = x, points[2 * at + 1] = y;
        scores[at] = s;
        if (lost != nullptr) lost[at] = i < kept ? 0 : 3;
    }
    if (tid == 0) count[n] = kept;
}

// ---------------------------------------------------------------- re-seeding
// (pos_in / pos_out and lost_in / lost_out may be the same arrays: no __restrict__ on them)
__global__ void __launch_bounds__(kThreads) refill_kernel(const float *pos_in, const uint8_t *lost_in, const float *__restrict__ new_points,
                                                          const int32_t *__restrict__ new_count, int t, float *pos_out, uint8_t *lost_out,
                                                          int32_t *__restrict__ born, int32_t *__restrict__ ids,
                                                          int32_t *__restrict__ next_id, int64_t P, int K) {
    __shared__ int scan[kThreads];
    const int tid = (int)threadIdx.x;
    const int64_t n = blockIdx.x;
    int avail = new_count[n];
    avail = avail < 0 ? 0 : (avail > K ? K : avail);
    const int32_t first_id = next_id[n];
    int64_t base = 0;                                                           // lost slots in front of this chunk
    for (int64_t p0 = 0; p0 < P; p0 += kThreads) {
        const int64_t p = p0 + tid, at = n * P + p;
        const bool in = p < P;
        const uint32_t code = in ? lost_in[at] : 0u;
        const float px = in ? pos_in[2 * at] : 0.f, py = in ? pos_in[2 * at + 1] : 0.f;
        const int flag = code != 0u ? 1 : 0;
        scan[tid] = flag;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int64_t rank = base + scan[tid] - flag;
        base += scan[kThreads - 1];
        if (in) {
            if (flag && rank < avail) {
                const int64_t from = n * K + rank;
                pos_out[2 * at] = new_points[2 * from], pos_out[2 * at + 1] = new_points[2 * from + 1];
                lost_out[at] = 0;
                born[at] = t;
                ids[at] = first_id + (int32_t)rank;
            } else {
                pos_out[2 * at] = px, pos_out[2 * at + 1] = py;
                lost_out[at] = (uint8_t)code;
            }
        }
        __syncthreads();                                                        // (scan is rewritten by the next chunk)
    }
    if (tid == 0) next_id[n] = first_id + (int32_t)(base < avail ? base : avail);
}

// ---------------------------------------------------------------- host side
static inline bool finite_f32(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }      // (a NaN fails)

static inline bool sizes_ok(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return false;
    if ((int64_t)H * W >= ((int64_t)1 << 32)) return false;
    return (int64_t)H * W <= (((int64_t)1 << 31) - 1) / N;                      // N * H * W < 2^31
}

static inline bool score_args_ok(int N, int H, int W, int C, int block_radius, int method, float harris_k, int border) {
    if (!sizes_ok(N, H, W) || (C != 1 && C != 3)) return false;
    if (block_radius < 1 || block_radius > kMaxBlockRadius || (method != 0 && method != 1)) return false;
    if (!finite_f32(harris_k) || harris_k < 0.f) return false;
    if (border < block_radius + 1 || border > (1 << 29)) return false;
    return H > 2 * border && W > 2 * border;
}

struct Workspace {
    u64 *cand;
    float *score;
    uint32_t *smax, *cand_count;      // (adjacent: one memset zeroes both)
    uint8_t *occ;
    int64_t bound;
};

static inline int64_t up8(int64_t v) { return (v + 7) & ~(int64_t)7; }

// keys: N * bound * 8 | score: N*H*W * 4 | smax, cand_count: N * 4 each | occupancy: N*H*W   (every part padded to 8 bytes)
// Returns the size in bytes (0: the sizes are refused); with a `base`, the parts.
static inline int64_t workspace_layout(void *base, int N, int H, int W, int m, Workspace *w) {
    if (!sizes_ok(N, H, W) || m < 1 || m > kMaxMinDistance) return 0;
    const int64_t npix = (int64_t)N * H * W;
    const int64_t bound = (int64_t)((H + m) / (m + 1)) * ((W + m) / (m + 1));
    const int64_t o_score = (int64_t)N * bound * 8, o_smax = o_score + up8(npix * 4), o_occ = o_smax + up8((int64_t)N * 8);
    if (base != nullptr) {
        char *p = (char *)base;
        w->cand = (u64 *)p, w->score = (float *)(p + o_score), w->smax = (uint32_t *)(p + o_smax), w->cand_count = w->smax + N;
        w->occ = (uint8_t *)(p + o_occ), w->bound = bound;
    }
    return o_occ + up8(npix);
}

static inline dim3 tile_grid(int N, int H, int W) {
    return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)(N < kMaxGridZ ? N : kMaxGridZ));
}

template <typename T>
static inline void launch_score(const T *frames, float *score, uint32_t *smax, int N, int H, int W, int C, int block_radius, int method,
                                float harris_k, int border, hipStream_t st) {
    const dim3 grid = tile_grid(N, H, W);
    if (C == 1)
        corner_score_kernel<T, 1><<<grid, kThreads, 0, st>>>(frames, score, smax, N, H, W, block_radius, method, harris_k, border);
    else
        corner_score_kernel<T, 3><<<grid, kThreads, 0, st>>>(frames, score, smax, N, H, W, block_radius, method, harris_k, border);
}

template <typename T>
static inline int corner_score_entry(const T *frames, float *score, float *smax, int N, int H, int W, int C, int block_radius, int method,
                                     float harris_k, int border, void *stream) {
    RAFT_REQUIRE_PTR(frames);
    RAFT_REQUIRE_PTR(score);
    RAFT_REQUIRE(score_args_ok(N, H, W, C, block_radius, method, harris_k, border), RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)score) | ((uintptr_t)smax) | (sizeof(T) == 4 ? (uintptr_t)frames : 0)) & 3u) == 0, RAFT_E_ALIGN);
    hipStream_t st = (hipStream_t)stream;
    if (smax != nullptr) RAFT_TRY((int)hipMemsetAsync(smax, 0, (size_t)N * 4, st));
    launch_score(frames, score, (uint32_t *)smax, N, H, W, C, block_radius, method, harris_k, border, st);
    return raft_launch_status();
}

}   // namespace

extern "C" int raft_corner_score_f32(const float *frames, float *score, float *smax, int N, int H, int W, int C, int block_radius,
                                     int method, float harris_k, int border, void *stream) {
    return corner_score_entry(frames, score, smax, N, H, W, C, block_radius, method, harris_k, border, stream);
}

extern "C" int raft_corner_score_u8_f32(const uint8_t *frames, float *score, float *smax, int N, int H, int W, int C, int block_radius,
                                        int method, float harris_k, int border, void *stream) {
    return corner_score_entry(frames, score, smax, N, H, W, C, block_radius, method, harris_k, border, stream);
}

extern "C" int64_t raft_detect_points_workspace_bytes(int N, int H, int W, int min_distance) {
    return workspace_layout(nullptr, N, H, W, min_distance, nullptr);
}

extern "C" int raft_detect_points(const void *frames, int frames_u8, const uint8_t *mask, const float *avoid_points,
                                  const uint8_t *avoid_lost, int64_t avoid_P, float *points, float *scores, int32_t *count, uint8_t *lost,
                                  int N, int H, int W, int C, int max_points, int min_distance, float quality_level, int block_radius,
                                  int method, float harris_k, int border, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(frames);
    RAFT_REQUIRE_PTR(points);
    RAFT_REQUIRE_PTR(scores);
    RAFT_REQUIRE_PTR(count);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE((avoid_points == nullptr) == (avoid_lost == nullptr), RAFT_E_NULL);
    RAFT_REQUIRE(frames_u8 == 0 || frames_u8 == 1, RAFT_E_SHAPE);
    RAFT_REQUIRE(score_args_ok(N, H, W, C, block_radius, method, harris_k, border), RAFT_E_SHAPE);
    RAFT_REQUIRE(max_points >= 1 && max_points <= kMaxPoints && min_distance >= 1 && min_distance <= kMaxMinDistance, RAFT_E_SHAPE);
    RAFT_REQUIRE(quality_level >= 0.f && quality_level < 1.f, RAFT_E_SHAPE);                     // (a NaN fails)
    if (avoid_points != nullptr)
        RAFT_REQUIRE(avoid_P > 0 && avoid_P <= ((((int64_t)1 << 31) - 1) / 2) / N, RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)workspace) & 7u) == 0, RAFT_E_ALIGN);
    RAFT_REQUIRE(((((uintptr_t)points) | ((uintptr_t)scores) | ((uintptr_t)count) | ((uintptr_t)avoid_points) |
                   (frames_u8 ? 0 : (uintptr_t)frames)) & 3u) == 0, RAFT_E_ALIGN);
    Workspace w;
    RAFT_REQUIRE(workspace_layout(workspace, N, H, W, min_distance, &w) > 0, RAFT_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    RAFT_TRY((int)hipMemsetAsync(w.smax, 0, (size_t)N * 8, st));
    if (avoid_points != nullptr) RAFT_TRY((int)hipMemsetAsync(w.occ, 0, (size_t)N * H * W, st));
    if (frames_u8)
        launch_score((const uint8_t *)frames, w.score, w.smax, N, H, W, C, block_radius, method, harris_k, border, st);
    else
        launch_score((const float *)frames, w.score, w.smax, N, H, W, C, block_radius, method, harris_k, border, st);
    RAFT_TRY(raft_launch_status());
    if (avoid_points != nullptr) {
        const int64_t threads = (int64_t)N * avoid_P * (2 * min_distance + 1);
        stamp_kernel<<<(unsigned)((threads + kThreads - 1) / kThreads), kThreads, 0, st>>>(avoid_points, avoid_lost, w.occ, N, avoid_P, H, W,
                                                                                         min_distance);
        RAFT_TRY(raft_launch_status());
    }
    nms_candidates_kernel<<<tile_grid(N, H, W), kThreads, 0, st>>>(w.score, w.smax, mask, avoid_points != nullptr ? w.occ : nullptr, w.cand,
                                                                  w.cand_count, N, H, W, min_distance, quality_level, (uint32_t)w.bound);
    RAFT_TRY(raft_launch_status());
    select_kernel<<<(unsigned)N, kSelectThreads, 0, st>>>(w.cand, w.cand_count, (uint32_t)w.bound, max_points, W, points, scores, count, lost);
    return raft_launch_status();
}

extern "C" int raft_refill_points(const float *pos_in, const uint8_t *lost_in, const float *new_points, const int32_t *new_count, int t,
                                  float *pos_out, uint8_t *lost_out, int32_t *born, int32_t *ids, int32_t *next_id, int N, int64_t P,
                                  int K, void *stream) {
    RAFT_REQUIRE_PTR(pos_in);
    RAFT_REQUIRE_PTR(lost_in);
    RAFT_REQUIRE_PTR(new_points);
    RAFT_REQUIRE_PTR(new_count);
    RAFT_REQUIRE_PTR(pos_out);
    RAFT_REQUIRE_PTR(lost_out);
    RAFT_REQUIRE_PTR(born);
    RAFT_REQUIRE_PTR(ids);
    RAFT_REQUIRE_PTR(next_id);
    RAFT_REQUIRE(N > 0 && P > 0 && K >= 1 && K <= kMaxPoints && t >= 0, RAFT_E_SHAPE);
    RAFT_REQUIRE(P <= ((((int64_t)1 << 31) - 1) / 2) / N, RAFT_E_SHAPE);                         // N * P * 2 < 2^31
    RAFT_REQUIRE(((((uintptr_t)pos_in) | ((uintptr_t)new_points) | ((uintptr_t)new_count) | ((uintptr_t)pos_out) | ((uintptr_t)born) |
                   ((uintptr_t)ids) | ((uintptr_t)next_id)) & 3u) == 0, RAFT_E_ALIGN);
    refill_kernel<<<(unsigned)N, kThreads, 0, (hipStream_t)stream>>>(pos_in, lost_in, new_points, new_count, t, pos_out, lost_out, born, ids,
                                                                     next_id, P, K);
    return raft_launch_status();
}

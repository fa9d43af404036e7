// Image-sized copies between a frame of any size and the model's input size: the window copy of
// tf.image.resize_with_crop_or_pad (below) and the table-driven bilinear resize (further down).
//
// tf.image.resize_with_crop_or_pad on (N, H, W, C) images: one window-copy kernel between a frame of any size and the model's
// input size (reference tf_raft/datasets/dataset.py:323-334 CropOrPadder, tf_raft/training.py:72-84 VisFlowCallback).
//
// Per axis, with d = target - source: the source window starts at max(-d // 2, 0), lands at max(d // 2, 0) in the target and
// is min(source, target) long (floor division: an odd surplus goes to the bottom / right).  Everything outside the window is
// zero in the input's own scale.  Every destination element is written exactly once, so the destination needs no memset.
//
// A pure streaming kernel.  One wave owns one destination row at a time (rows of all images in a grid-stride loop: one 64-bit
// division per row, none per element) and walks it in chunks of V elements = 16 bytes of the destination; a chunk that lies
// wholly inside the window and whose source address is aligned is one wide load and one 16-byte store, four of them in flight
// per lane; the chunks on the window's edges (and rows whose source is misaligned, e.g. 1242 x 3 bytes) fall back to per-element
// loads.  A destination whose rows are not whole 16-byte chunks runs the same kernel with V = 1.
#include "common.h"

namespace {

template <typename T, int V>
struct alignas(sizeof(T) * V) Chunk {
    T v[V];
};

struct WindowGeom {
    int64_t rows;             // N * Ht
    int Hs, Ht;
    int crop_y, pad_y, ext_y;
    int64_t src_row, dst_row; // elements per source / destination row (W * C)
    int64_t lo, hi;           // window of a destination row, in elements
    int64_t shift;            // source element of a row = destination element + shift (within the rows' own bases)
    int c0, c1;               // the V-element chunks of a destination row that lie wholly inside [lo, hi): set per launch
};

constexpr int kRowsPerBlock = 4;      // one wave per row
constexpr int kMaxBlocks = 4096;

template <typename S, typename D, int V>
__device__ __forceinline__ Chunk<D, V> convert_chunk(const Chunk<S, V> &a) {
    Chunk<D, V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = (D)a.v[j];
    return o;
}

constexpr int kUnroll = 4;            // wide loads a wave keeps in flight

template <typename S, typename D, int V>
__global__ void __launch_bounds__(64 * kRowsPerBlock) window_copy_kernel(const S *__restrict__ src, D *__restrict__ dst,
                                                                           WindowGeom g) {
    const int lane = threadIdx.x & 63;
    const int chunks = (int)(g.dst_row / V);
    for (int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6); r < g.rows; r += (int64_t)gridDim.x * kRowsPerBlock) {
        const int64_t n = r / g.Ht;
        const int y = (int)(r - n * g.Ht) - g.pad_y;
        Chunk<D, V> *out = (Chunk<D, V> *)(dst + r * g.dst_row);
        if (y < 0 || y >= g.ext_y) {
            Chunk<D, V> z;
#pragma unroll
            for (int j = 0; j < V; ++j) z.v[j] = (D)0;
            for (int c = lane; c < chunks; c += 64) out[c] = z;
            continue;
        }
        // element e of this destination row comes from in[e] for lo <= e < hi
        const S *in = src + ((n * g.Hs + g.crop_y + y) * g.src_row + g.shift);
        // chunks [c0, c1) lie wholly inside the window; they are wide loads when this row's source is aligned for them
        const bool wide = (((uintptr_t)in) & (sizeof(S) * V - 1)) == 0;
        const int c0 = wide ? g.c0 : 0, c1 = wide ? g.c1 : 0;
        const Chunk<S, V> *in_chunks = (const Chunk<S, V> *)in;
        for (int c = c0 + lane; c < c1; c += 64 * kUnroll) {     // all loads of a trip are issued before its first store
            Chunk<S, V> a[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (c + 64 * u < c1) a[u] = in_chunks[c + 64 * u];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (c + 64 * u < c1) out[c + 64 * u] = convert_chunk<S, D, V>(a[u]);
        }
        // the chunks on the window's edges and outside it (every chunk of a row whose source is not aligned)
        for (int c = lane; c < chunks; c += 64) {
            if (c >= c0 && c < c1) {
                c += (c1 - 1 - c) / 64 * 64;                     // to this lane's last chunk inside [c0, c1)
                continue;
            }
            const int64_t e = (int64_t)c * V;
            Chunk<D, V> o;
#pragma unroll
            for (int j = 0; j < V; ++j) o.v[j] = (e + j >= g.lo && e + j < g.hi) ? (D)in[e + j] : (D)0;
            out[c] = o;
        }
    }
}

template <typename S, typename D>
int window_copy(const S *src, D *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ht > 0 && Wt > 0 && C > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)Ws * C <= 0x7fffffff && (int64_t)Wt * C <= 0x7fffffff, RAFT_E_SHAPE);
    WindowGeom g;
    int crop_x, pad_x, ext_x;
    raft_axis_window(Hs, Ht, &g.crop_y, &g.pad_y, &g.ext_y);
    raft_axis_window(Ws, Wt, &crop_x, &pad_x, &ext_x);
    g.rows = (int64_t)N * Ht;
    g.Hs = Hs;
    g.Ht = Ht;
    g.src_row = (int64_t)Ws * C;
    g.dst_row = (int64_t)Wt * C;
    g.lo = (int64_t)pad_x * C;
    g.hi = (int64_t)(pad_x + ext_x) * C;
    g.shift = (int64_t)(crop_x - pad_x) * C;
    const int64_t blocks = (g.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(64 * kRowsPerBlock);
    constexpr int V = 16 / (int)sizeof(D);
    if (g.dst_row % V == 0 && raft_aligned16(dst)) {
        g.c0 = (int)((g.lo + V - 1) / V);
        g.c1 = (int)(g.hi / V) > g.c0 ? (int)(g.hi / V) : g.c0;
        window_copy_kernel<S, D, V><<<grid, block, 0, (hipStream_t)stream>>>(src, dst, g);
    } else {
        g.c0 = (int)g.lo;
        g.c1 = (int)g.hi;
        window_copy_kernel<S, D, 1><<<grid, block, 0, (hipStream_t)stream>>>(src, dst, g);
    }
    return raft_launch_status();
}


// ---------------------------------------------------------------------------------------------------------------- resize
// Separable table-driven resize (bilinear with half-pixel centres, optionally widened to an antialiasing triangle on a shrinking
// axis; the tables are made on the host in float64, tf_raft_amd/image_ops.py resize_taps):
//
//     dst[n, y, x, c] = chan_scale[c] * sum_b wx[x][b] * ( sum_a wy[y][a] * src[n, y0[y] + a, x0[x] + b, c] )
//
// One wave owns one destination row at a time, as in the window copy, and walks it in segments of `seg` destination pixels.
// Per segment it (1) reduces the row's ny[y] source rows over the segment's source span into its own slice of LDS -- every
// lane reads 16 bytes of each source row (4 floats / 16 bytes of uint8) where that row is aligned for it, element by element
// where it is not (603-byte rows) and in the last, partial group of a row -- and (2) forms each destination element from the
// nx[x] LDS values of its channel, 16 bytes of destination per lane.  So a source row is read once per destination row that
// uses it (from L2 after the first), every global access of the image data is a whole-wave contiguous one, and no image-sized
// intermediate exists.  Waves never share LDS: the phases are ordered by wave barriers only.
//
// Whatever the tables hold, indices are clamped to the source before they are used as addresses.
constexpr int kResizeCap = 2048;      // floats of LDS per wave (8 KB; five 4-wave workgroups per CU)

struct ResizeGeom {
    int64_t rows;             // N * Ht
    int Hs, Ws, Ht, Wt, C;
    int src_row, dst_row;     // elements per source / destination row (W * C)
    int seg;                  // destination pixels per segment (a multiple of 4 in the vector kernel unless there is one segment)
    int my, mx;               // stride of the weight tables = largest tap count
    const int *y0, *ny, *x0, *nx;
    const float *wy, *wx, *cs;
};

__device__ __forceinline__ int resize_div(int e, int C) {     // e / C, the common channel counts without a division
    return C == 2 ? e >> 1 : C == 1 ? e : C == 3 ? (int)((unsigned)e / 3u) : (int)((unsigned)e / (unsigned)C);
}

template <typename S, int V>
__global__ void __launch_bounds__(64 * kRowsPerBlock) resize_kernel(const S *__restrict__ src, float *__restrict__ dst, ResizeGeom g) {
    constexpr int G = 16 / (int)sizeof(S);       // source elements of one 16-byte load
    __shared__ __attribute__((aligned(16))) float lds_all[kRowsPerBlock][kResizeCap];
    float *lds = lds_all[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const int C = g.C;
    for (int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6); r < g.rows; r += (int64_t)gridDim.x * kRowsPerBlock) {
        const int64_t n = r / g.Ht;
        const int y = (int)(r - n * g.Ht);
        const int fy = min(max(g.y0[y], 0), g.Hs - 1);
        const int cy = min(min(g.ny[y], g.my), g.Hs - fy);
        const float *wy = g.wy + (int64_t)y * g.my;
        const S *rows = src + (n * g.Hs + fy) * g.src_row;
        float *out = dst + r * g.dst_row;
        for (int xa = 0; xa < g.Wt; xa += g.seg) {
            const int xb = min(xa + g.seg, g.Wt);
            const int lo = min(max(g.x0[xa], 0), g.Ws - 1);
            const int hi = min(max(g.x0[xb - 1] + g.nx[xb - 1], lo + 1), g.Ws);
            const int start = lo * C / G * G;                    // the element of a source row that LDS slot 0 holds
            const int groups = (min(hi * C - start, kResizeCap) + G - 1) / G;
            __builtin_amdgcn_wave_barrier();                     // the previous segment's reads of the LDS slice are done
            for (int q = lane; q < groups; q += 64) {
                const int e = start + q * G;
                const bool whole = e + G <= g.src_row;
                float acc[G];
#pragma unroll
                for (int j = 0; j < G; ++j) acc[j] = 0.f;
                for (int a = 0; a < cy; ++a) {
                    const S *p = rows + (int64_t)a * g.src_row + e;
                    const float w = wy[a];
                    // (the test on the row's first group is the same for all lanes; only `whole` differs, in a row's last group)
                    if (whole && (((uintptr_t)(p - q * G)) & 15u) == 0) {
                        const Chunk<S, G> v = *(const Chunk<S, G> *)p;
#pragma unroll
                        for (int j = 0; j < G; ++j) acc[j] += w * (float)v.v[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < G; ++j)
                            if (e + j < g.src_row) acc[j] += w * (float)p[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < G; j += 4) {
                    f32x4 v = {acc[j], acc[j + 1], acc[j + 2], acc[j + 3]};
                    *(f32x4 *)(lds + q * G + j) = v;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int e1 = xb * C;
            for (int e = xa * C + lane * V; e < e1; e += 64 * V) {
                Chunk<float, V> o;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int x = resize_div(e + j, C), c = e + j - x * C;
                    const int fx = min(max(g.x0[x], 0), g.Ws - 1);
                    const int cx = min(min(g.nx[x], g.mx), g.Ws - fx);
                    const float *w = g.wx + (int64_t)x * g.mx;
                    const int slot = fx * C + c - start;
                    float s = 0.f;
                    for (int b = 0; b < cx; ++b) {
                        const int i = slot + b * C;
                        s += w[b] * lds[min(max(i, 0), kResizeCap - 1)];
                    }
                    o.v[j] = g.cs ? g.cs[c] * s : s;
                }
                *(Chunk<float, V> *)(out + e) = o;
            }
        }
    }
}

constexpr int kResizeMaxTaps = 64;    // per axis: shrink ratios up to 31 with the antialiasing triangle

// Destination pixels per segment such that the segment's source span fits the LDS slice.  With non-decreasing first indices
// that advance by at most ceil(Ws / Wt) per pixel plus one (every table of the rule does), k pixels span at most
// ceil((k - 1) * Ws / Wt) + 1 + max_taps source pixels; the slice also holds up to G - 1 elements in front (the span starts on
// a 16-byte group) and behind (its last group is whole).  0: not even one pixel fits.
inline int resize_segment(int Ws, int Wt, int C, int max_taps, int G) {
    const int64_t avail = (int64_t)(kResizeCap - 2 * (G - 1)) / C - max_taps - 1;
    if (avail < 0) return 0;
    const int64_t k = avail * Wt / Ws + 1;
    return (int)(k < Wt ? k : Wt);
}

template <typename S>
int resize(const S *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, const int *y_first, const int *y_count,
           const float *y_weights, int y_max_taps, const int *x_first, const int *x_count, const float *x_weights, int x_max_taps,
           const float *chan_scale, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE_PTR(y_first);
    RAFT_REQUIRE_PTR(y_count);
    RAFT_REQUIRE_PTR(y_weights);
    RAFT_REQUIRE_PTR(x_first);
    RAFT_REQUIRE_PTR(x_count);
    RAFT_REQUIRE_PTR(x_weights);
    RAFT_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ht > 0 && Wt > 0 && C > 0, RAFT_E_SHAPE);
    // (an int, with room for the last stride of a wave's walk along a row)
    RAFT_REQUIRE((int64_t)Ws * C <= 0x7fffffff - 1024 && (int64_t)Wt * C <= 0x7fffffff - 1024, RAFT_E_SHAPE);
    RAFT_REQUIRE(y_max_taps >= 1 && y_max_taps <= kResizeMaxTaps && x_max_taps >= 1 && x_max_taps <= kResizeMaxTaps, RAFT_E_SHAPE);
    constexpr int G = 16 / (int)sizeof(S);
    int seg = resize_segment(Ws, Wt, C, x_max_taps, G);
    RAFT_REQUIRE(seg >= 1, RAFT_E_SHAPE);           // this many taps of this many channels do not fit a wave's LDS slice
    ResizeGeom g;
    g.rows = (int64_t)N * Ht;
    g.Hs = Hs, g.Ws = Ws, g.Ht = Ht, g.Wt = Wt, g.C = C;
    g.src_row = Ws * C;
    g.dst_row = Wt * C;
    g.my = y_max_taps, g.mx = x_max_taps;
    g.y0 = y_first, g.ny = y_count, g.x0 = x_first, g.nx = x_count;
    g.wy = y_weights, g.wx = x_weights, g.cs = chan_scale;
    const int64_t blocks = (g.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(64 * kRowsPerBlock);
    // 16-byte stores need whole chunks per row and per segment: segments of a multiple of 4 pixels, evened out over the row
    const bool vec = g.dst_row % 4 == 0 && raft_aligned16(dst) && (seg >= Wt || seg >= 4);
    if (seg < Wt) {
        const int step = vec ? 4 : 1, fit = seg / step * step, count = (Wt + fit - 1) / fit;
        seg = ((Wt + count - 1) / count + step - 1) / step * step;
    }
    g.seg = seg;
    if (vec)
        resize_kernel<S, 4><<<grid, block, 0, (hipStream_t)stream>>>(src, dst, g);
    else
        resize_kernel<S, 1><<<grid, block, 0, (hipStream_t)stream>>>(src, dst, g);
    return raft_launch_status();
}

}   // namespace

extern "C" int raft_crop_or_pad_f32(const float *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream) {
    return window_copy<float, float>(src, dst, N, Hs, Ws, Ht, Wt, C, stream);
}

extern "C" int raft_crop_or_pad_u8_f32(const uint8_t *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream) {
    return window_copy<uint8_t, float>(src, dst, N, Hs, Ws, Ht, Wt, C, stream);
}

extern "C" int raft_crop_or_pad_u8(const uint8_t *src, uint8_t *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream) {
    return window_copy<uint8_t, uint8_t>(src, dst, N, Hs, Ws, Ht, Wt, C, stream);
}

extern "C" int raft_resize_f32(const float *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, const int *y_first,
                               const int *y_count, const float *y_weights, int y_max_taps, const int *x_first, const int *x_count,
                               const float *x_weights, int x_max_taps, const float *chan_scale, void *stream) {
    return resize<float>(src, dst, N, Hs, Ws, Ht, Wt, C, y_first, y_count, y_weights, y_max_taps, x_first, x_count, x_weights,
                         x_max_taps, chan_scale, stream);
}

extern "C" int raft_resize_u8_f32(const uint8_t *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, const int *y_first,
                                  const int *y_count, const float *y_weights, int y_max_taps, const int *x_first, const int *x_count,
                                  const float *x_weights, int x_max_taps, const float *chan_scale, void *stream) {
    return resize<uint8_t>(src, dst, N, Hs, Ws, Ht, Wt, C, y_first, y_count, y_weights, y_max_taps, x_first, x_count, x_weights,
                           x_max_taps, chan_scale, stream);
}

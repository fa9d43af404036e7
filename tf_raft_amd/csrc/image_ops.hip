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

inline void axis_window(int source, int target, int *crop, int *pad, int *ext) {
    const int d = target - source;
    *crop = d < 0 ? (-d) / 2 : 0;     // max(-d // 2, 0)
    *pad = d > 0 ? d / 2 : 0;         // max( d // 2, 0)
    *ext = source < target ? source : target;
}

template <typename S, typename D>
int window_copy(const S *src, D *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ht > 0 && Wt > 0 && C > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)Ws * C <= 0x7fffffff && (int64_t)Wt * C <= 0x7fffffff, RAFT_E_SHAPE);
    WindowGeom g;
    int crop_x, pad_x, ext_x;
    axis_window(Hs, Ht, &g.crop_y, &g.pad_y, &g.ext_y);
    axis_window(Ws, Wt, &crop_x, &pad_x, &ext_x);
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

// Image-sized copies between a frame of any size and the model's input size: the window copy of
// tf.image.resize_with_crop_or_pad (below), the table-driven bilinear resize (further down) and the tile gather / weighted blend
// of tiled inference (at the end).
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

// One destination row of `chunks` V-element chunks by one wave: element e comes from in[e] for lo <= e < hi and is zero
// elsewhere; chunks [c0, c1) lie wholly inside [lo, hi).  `in` is only dereferenced inside the window.
template <typename S, typename D, int V>
__device__ __forceinline__ void window_row(const S *__restrict__ in, Chunk<D, V> *__restrict__ out, int lane, int chunks, int64_t lo,
                                           int64_t hi, int gc0, int gc1) {
    // chunks [c0, c1) are wide loads when this row's source is aligned for them
    const bool wide = (((uintptr_t)in) & (sizeof(S) * V - 1)) == 0;
    const int c0 = wide ? gc0 : 0, c1 = wide ? gc1 : 0;
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
        for (int j = 0; j < V; ++j) o.v[j] = (e + j >= lo && e + j < hi) ? (D)in[e + j] : (D)0;
        out[c] = o;
    }
}

template <typename D, int V>
__device__ __forceinline__ void zero_row(Chunk<D, V> *__restrict__ out, int lane, int chunks) {
    Chunk<D, V> z;
#pragma unroll
    for (int j = 0; j < V; ++j) z.v[j] = (D)0;
    for (int c = lane; c < chunks; c += 64) out[c] = z;
}

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
            zero_row<D, V>(out, lane, chunks);
            continue;
        }
        // element e of this destination row comes from in[e] for lo <= e < hi
        const S *in = src + ((n * g.Hs + g.crop_y + y) * g.src_row + g.shift);
        window_row<S, D, V>(in, out, lane, chunks, g.lo, g.hi, g.c0, g.c1);
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


// ------------------------------------------------------------------------------------------------------------------ tiles
// Tiled inference: a frame larger than the model's size is covered by a product grid of ny x nx
// overlapping model-sized tiles (origins from tf_raft_amd/image_ops.py tile_origins), every tile is predicted on its own and the
// predictions are cross-faded where tiles overlap.
//
// The gather in front of the model is the window copy with a window per tile: one wave owns one row of one tile, its source is
// the frame's row oy[ky] + y shifted by ox[kx] pixels, zero outside the frame.  The origins travel by value (a wave reads its
// own two through scalar loads: the wave's row is made uniform first).
template <typename S, int V>
__global__ void __launch_bounds__(64 * kRowsPerBlock) tile_gather_kernel(const S *__restrict__ src, float *__restrict__ dst, int64_t rows,
                                                                           int Hs, int Ws, int Ht, int Wt, int C, RaftTileOrigins o) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t dst_row = (int64_t)Wt * C, src_row = (int64_t)Ws * C;
    const int chunks = (int)(dst_row / V);
    for (int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + wave; r < rows; r += (int64_t)gridDim.x * kRowsPerBlock) {
        const int64_t k = r / Ht;                                // tile (n * ny + ky) * nx + kx
        const int y = (int)(r - k * Ht);
        const int64_t nk = k / o.nx;
        const int kx = (int)(k - nk * o.nx);
        const int64_t n = nk / o.ny;
        const int ky = (int)(nk - n * o.ny);
        const int sy = o.oy[ky] + y, ox = o.ox[kx];
        Chunk<float, V> *out = (Chunk<float, V> *)(dst + r * dst_row);
        if (sy < 0 || sy >= Hs) {
            zero_row<float, V>(out, lane, chunks);
            continue;
        }
        // element e of this destination row comes from in[e] for lo <= e < hi: the tile's columns that lie inside the frame
        const int64_t lo = (int64_t)max(-ox, 0) * C, hi = (int64_t)max(min(Wt, Ws - ox), max(-ox, 0)) * C;
        const S *in = src + ((n * Hs + sy) * src_row + (int64_t)ox * C);
        const int c0 = (int)((lo + V - 1) / V);
        window_row<S, float, V>(in, out, lane, chunks, lo, hi, c0, max((int)(hi / V), c0));
    }
}

template <typename S>
int tile_gather(const S *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, const RaftTileOrigins &o, void *stream) {
    RAFT_REQUIRE_PTR(src);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ht > 0 && Wt > 0 && C > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)Ws * C <= 0x7fffffff && (int64_t)Wt * C <= 0x7fffffff, RAFT_E_SHAPE);
    RAFT_REQUIRE(o.ny >= 1 && o.ny <= RAFT_TILE_MAX_PER_AXIS && o.nx >= 1 && o.nx <= RAFT_TILE_MAX_PER_AXIS, RAFT_E_SHAPE);
    for (int i = 0; i < o.ny; ++i) RAFT_REQUIRE(o.oy[i] > -Ht && o.oy[i] < Hs, RAFT_E_SHAPE);     // every tile meets the frame
    for (int i = 0; i < o.nx; ++i) RAFT_REQUIRE(o.ox[i] > -Wt && o.ox[i] < Ws, RAFT_E_SHAPE);
    const int64_t rows = (int64_t)N * o.ny * o.nx * Ht;
    const int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(64 * kRowsPerBlock);
    if (((int64_t)Wt * C) % 4 == 0 && raft_aligned16(dst))
        tile_gather_kernel<S, 4><<<grid, block, 0, (hipStream_t)stream>>>(src, dst, rows, Hs, Ws, Ht, Wt, C, o);
    else
        tile_gather_kernel<S, 1><<<grid, block, 0, (hipStream_t)stream>>>(src, dst, rows, Hs, Ws, Ht, Wt, C, o);
    return raft_launch_status();
}

// The blend behind the model: with separable tent weights on a product grid the normalised weight of tile (ky, kx) at frame
// pixel (y, x) is a[y][ky] * b[x][kx], so
//
//     dst[m, n, y, x] = sum_kx b[x][kx] * ( sum_ky a[y][ky] * tiles[m, (n * ny + ky) * nx + kx, y - oy[ky], x - ox[kx]] )
//
// with both sums in this order.  An axis is described like an axis of the resize: per frame coordinate the first tile index, the
// number of tiles and their weights (derived in float64 on the host, each rounded once).  One wave owns kTileBlendSpan
// consecutive pixels of one destination row, kTileBlendPerLane pixels per lane, one pixel (a float2) per lane and access: a
// wave-wide access is 512 contiguous bytes of a tile row or of the destination, whatever the parity of an origin.  The row's
// taps are wave-uniform, and so is the loop over the tile columns that reach the span (from the table at the span's two ends:
// first indices and ends of runs do not decrease along an axis): a tile's origin is a scalar, the tile loads of a lane's pixels
// depend on nothing but it and are issued together, and only the weight of a pixel waits for the pixel's table entry.  A lane
// outside the tile column at hand loads from a clamped address and drops the value.  Every tile element is read by the one
// pixel it contributes to and every destination element is written once, so there is no memset, no atomic and no intermediate.
// Whatever the tables hold, tile indices and tile coordinates are clamped into the tiles.
constexpr int kTileBlendPerLane = 4;
constexpr int kTileBlendSpan = 64 * kTileBlendPerLane;

struct TileBlendGeom {
    int64_t frames;           // M * N
    int items;                // H * segs: the waves of one frame
    int H, W, Ht, Wt;
    int segs;                 // ceil(W / kTileBlendSpan)
    int my, mx;               // stride of the weight tables
    const int *y0, *ny, *x0, *nx;
    const float *wy, *wx;
};

__global__ void __launch_bounds__(64 * kRowsPerBlock) tile_blend_kernel(const float2 *__restrict__ tiles, float2 *__restrict__ dst,
                                                                          TileBlendGeom g, RaftTileOrigins o) {
    constexpr int P = kTileBlendPerLane, T = RAFT_TILE_MAX_TAPS;
    const int lane = threadIdx.x & 63;
    const int item = (int)blockIdx.x * kRowsPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= g.items) return;
    const int y = item / g.segs;
    const int xa = (item - y * g.segs) * kTileBlendSpan, xb = min(xa + kTileBlendSpan, g.W);
    // the row's taps
    const int fy = min(max(g.y0[y], 0), o.ny - 1);
    const int cy = min(min(g.ny[y], min(g.my, T)), o.ny - fy);
    float a[T];
    int row[T];                                                  // pixel offset of the row of this y inside tile (fy + i, 0)
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int ky = min(fy + i, o.ny - 1);
        a[i] = i < cy ? g.wy[(int64_t)y * g.my + i] : 0.f;
        row[i] = min(max(y - o.oy[ky], 0), g.Ht - 1) * g.Wt;
    }
    // the tile columns that reach the span
    const int k_lo = min(max(g.x0[xa], 0), o.nx - 1);
    const int k_hi = min(max(g.x0[xb - 1] + g.nx[xb - 1], k_lo + 1), o.nx);
    // the pixels of this lane (a lane past the row's end works on the row's last pixel and stores nothing)
    int x[P], fx[P], cx[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
        x[u] = min(xa + u * 64 + lane, g.W - 1);
        fx[u] = min(max(g.x0[x[u]], 0), o.nx - 1);
        cx[u] = min(min(g.nx[x[u]], min(g.mx, T)), o.nx - fx[u]);
    }
    const int64_t tile_px = (int64_t)g.Ht * g.Wt;
    for (int64_t mn = blockIdx.y; mn < g.frames; mn += gridDim.y) {
        float2 acc[P];
#pragma unroll
        for (int u = 0; u < P; ++u) acc[u] = make_float2(0.f, 0.f);
        for (int kx = k_lo; kx < k_hi; ++kx) {
            const int ox = o.ox[kx];
            int t[P];
#pragma unroll
            for (int u = 0; u < P; ++u) t[u] = min(max(x[u] - ox, 0), g.Wt - 1);
            float2 s[P];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                if (i >= cy) break;
                const float2 *in = tiles + (((mn * o.ny + fy + i) * o.nx + kx) * tile_px + row[i]);
                float2 v[P];
#pragma unroll
                for (int u = 0; u < P; ++u) v[u] = in[t[u]];
#pragma unroll
                for (int u = 0; u < P; ++u) {
                    if (i == 0)
                        s[u] = make_float2(a[0] * v[u].x, a[0] * v[u].y);
                    else
                        s[u].x += a[i] * v[u].x, s[u].y += a[i] * v[u].y;
                }
            }
            if (cy < 1) {
#pragma unroll
                for (int u = 0; u < P; ++u) s[u] = make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < P; ++u) {
                const int j = kx - fx[u];
                const bool in_run = j >= 0 && j < cx[u];
                const float b = g.wx[(int64_t)x[u] * g.mx + min(max(j, 0), g.mx - 1)];
                const float2 first = make_float2(b * s[u].x, b * s[u].y);
                const float2 next = make_float2(acc[u].x + b * s[u].x, acc[u].y + b * s[u].y);
                acc[u] = !in_run ? acc[u] : j == 0 ? first : next;
            }
        }
        float2 *out = dst + (mn * g.H + y) * g.W;
#pragma unroll
        for (int u = 0; u < P; ++u)
            if (xa + u * 64 + lane < g.W) out[x[u]] = acc[u];
    }
}

}   // namespace

extern "C" int raft_tile_gather_f32(const float *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, RaftTileOrigins origins,
                                    void *stream) {
    return tile_gather<float>(src, dst, N, Hs, Ws, Ht, Wt, C, origins, stream);
}

extern "C" int raft_tile_gather_u8_f32(const uint8_t *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C,
                                       RaftTileOrigins origins, void *stream) {
    return tile_gather<uint8_t>(src, dst, N, Hs, Ws, Ht, Wt, C, origins, stream);
}

extern "C" int raft_tile_blend_f32(const float *tiles, float *dst, int64_t M, int N, int H, int W, int Ht, int Wt, RaftTileOrigins origins,
                                   const int *y_first, const int *y_count, const float *y_weights, int y_max_taps, const int *x_first,
                                   const int *x_count, const float *x_weights, int x_max_taps, void *stream) {
    RAFT_REQUIRE_PTR(tiles);
    RAFT_REQUIRE_PTR(dst);
    RAFT_REQUIRE_PTR(y_first);
    RAFT_REQUIRE_PTR(y_count);
    RAFT_REQUIRE_PTR(y_weights);
    RAFT_REQUIRE_PTR(x_first);
    RAFT_REQUIRE_PTR(x_count);
    RAFT_REQUIRE_PTR(x_weights);
    RAFT_REQUIRE(M > 0 && N > 0 && H > 0 && W > 0 && Ht > 0 && Wt > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE(origins.ny >= 1 && origins.ny <= RAFT_TILE_MAX_PER_AXIS && origins.nx >= 1 && origins.nx <= RAFT_TILE_MAX_PER_AXIS, RAFT_E_SHAPE);
    RAFT_REQUIRE(y_max_taps >= 1 && y_max_taps <= RAFT_TILE_MAX_TAPS && x_max_taps >= 1 && x_max_taps <= RAFT_TILE_MAX_TAPS, RAFT_E_SHAPE);
    RAFT_REQUIRE(W <= 0x7fffffff - kTileBlendSpan && (int64_t)Ht * Wt <= 0x7fffffff, RAFT_E_SHAPE);
    RAFT_REQUIRE(M <= ((int64_t)1 << 40) / N, RAFT_E_SHAPE);
    RAFT_REQUIRE(((((uintptr_t)tiles) | ((uintptr_t)dst)) & 7u) == 0, RAFT_E_ALIGN);
    TileBlendGeom g;
    g.H = H, g.W = W, g.Ht = Ht, g.Wt = Wt;
    g.segs = (W + kTileBlendSpan - 1) / kTileBlendSpan;
    RAFT_REQUIRE((int64_t)H * g.segs <= 0x7fffffff - kRowsPerBlock, RAFT_E_SHAPE);
    g.items = H * g.segs;
    g.frames = M * N;
    g.my = y_max_taps, g.mx = x_max_taps;
    g.y0 = y_first, g.ny = y_count, g.x0 = x_first, g.nx = x_count;
    g.wy = y_weights, g.wx = x_weights;
    // one grid row per frame of a prediction; beyond the grid's y extent a workgroup walks several
    const dim3 grid((unsigned)((g.items + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)(g.frames < 65535 ? g.frames : 65535));
    tile_blend_kernel<<<grid, dim3(64 * kRowsPerBlock), 0, (hipStream_t)stream>>>((const float2 *)tiles, (float2 *)dst, g, origins);
    return raft_launch_status();
}

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

// Connected components of a mask and their statistics (no reference counterpart): the list behind a map.
//
//   raft_label_components            labels (N, H, W): 0 for background, 1 + the component's smallest raster index
//   raft_find_objects                the max_objects largest components of at least min_area pixels, largest first: area, box,
//                                    centroid, mean flow, and the map of their slots
//   raft_remove_small_components     the mask without the components of fewer than min_area pixels
//
// The definition is written down once in include/raft_hip.h and restated in NumPy (a breadth-first fill) in
// tests/test_components.py.  Everything here is an integer: a label is a minimum of raster indices, every statistic an integer sum,
// minimum or maximum, taken with integer atomics, which do not depend on the order they arrive in; the two divisions behind a
// centroid and a mean flow are one float64 division of exact integers each.  So the result is a function of the input alone and
// repeats bit for bit.
//
// The forest.  `parent` (int32 per pixel, index within the image) holds -1 for background and for a foreground pixel a pixel of
// its own component with parent[i] <= i; a ROOT points at itself.  A `find` from pixel i follows strictly decreasing indices, so it
// ends after at most i steps.  `unite(a, b)` finds both roots and hangs the LARGER under the smaller with atomicMin(&parent[a], b):
// it returns the value it met; if that is `a` itself the link is made, otherwise somebody else lowered parent[a] in between, and
// the loop goes on with that smaller value in a's place.  Labels only ever decrease and are bounded below by 0, so they are lowered
// finitely often and a retry happens finitely often: no thread ever waits for another, there is no flag, no barrier across
// workgroups and no ticket.  The root of a finished tree is the smallest index of its component, because every member reaches it
// over decreasing indices.
//
// Launches, all on `stream` (T = a 32 x 16 tile, one workgroup of 256 threads, two pixels per thread):
//   1. tile_label_kernel: the foreground of a tile goes to LDS, every pixel unites with its W, N (and NW, NE) neighbours INSIDE the
//      tile by the union above on LDS, then finds its root: parent[i] = the smallest raster index of its piece of the tile.  Global
//      traffic: the tile's loads and one store per pixel.
//   2. border_merge_kernel: one wave per tile walks the tile's top row and left column and unites every pixel there with its
//      foreground neighbours across the border.  WITHIN THIS LAUNCH every value of `parent` reaches a thread only as the return
//      value of an agent-scope atomic read-modify-write -- atomicMin(p, 0x7FFFFFFF) is the read -- never through a plain or an sc1
//      load: the L2s of the chip's dies are not coherent with each other and a CU's L1 is never refreshed by another CU's stores,
//      an atomic executes at the one place that is.  Only pixels that were roots after launch 1 are ever re-linked, so every
//      other pixel still points at a pixel of its own tile.
//   3. resolve_kernel, behind the kernel boundary (plain loads from here on): the pixels of a tile are binned in LDS by the pixel
//      they point at (all pixels of a bin share their root), ONE thread per non-empty bin walks to the root, and the pixels read it
//      back from LDS.  raft_label_components writes 1 + root and is done.  The other two entries store the root per pixel and add
//      the pixel counts to area[root] (uint32 at the root's own pixel slot): the bins of one root are first added up in a small
//      direct-mapped LDS table, so a tile sends one global atomic per root it met (a root that finds its entry taken sends its own).
//   raft_remove_small_components: 4. keep_kernel: out = foreground and area[root] >= min_area.
//   raft_find_objects:
//   4. candidates_kernel: every root with area >= min_area appends the key (uint64)area << 32 | (0xFFFFFFFF - root index) to the
//      image's list; a workgroup reserves its slots with one atomic.  The list's order differs from run to run, and that is allowed:
//   5. select_kernel, one workgroup per image: keys are unique, the candidates of an image are a SET, and the sorted top-K of a set
//      is the same bits whatever order the set was gathered in (radix select over eight 8-bit digits when there are more than K,
//      then one bitonic sort: csrc/point_detect.hip's, restated here so that file stays as it is).  It writes count and area,
//      clears the slots' records and marks area[root] = 0x80000000 | slot for the chosen roots (an area is below 2^31).
//   6. stats_kernel: one pass over the pixels writes `labels` and accumulates box, coordinate sums and quantised flow sums per bin
//      in LDS (integer LDS atomics), the bins of one slot are put together in a direct-mapped LDS table, and one thread per slot
//      the tile met sends them to one of the slot's 8 records (tile index mod 8: the tiles of one large object do not all queue
//      at one address): atomicMin / atomicMax on int32, atomicAdd on uint64.  No float atomic anywhere.
//   7. finish_kernel: one thread per slot joins the 8 records (integer sums, minima, maxima: any order) and makes box, centroid
//      and mean flow, one float64 division and one rounding each.
// Memsets: one (area, with the candidate counters next to it) in the two entries that count; none in raft_label_components.
#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 16, kTile = kTileW * kTileH;      // pixels of a workgroup (two per thread)
constexpr int kMine = kTile / kThreads;
constexpr int kMergeThreads = 64;
constexpr int kMaxObjects = RAFT_OBJECTS_MAX;
constexpr int kSelectThreads = 1024;
constexpr int kMaxGridY = 65535;
constexpr int kNoLabel = 0x7FFFFFFF;                                   // above every index: atomicMin with it changes nothing
constexpr uint32_t kChosen = 0x80000000u;
constexpr int kCache = 64;                                             // a workgroup's direct-mapped LDS table of roots / of slots
constexpr int kCopies = 8;                                             // records per slot: tiles spread their atomics over them
constexpr float kFlowLimit = 1048576.f;                                // 2^20

struct Tiles {
    int nx;            // tiles per row of tiles
    int64_t count;     // tiles per image
};

static inline Tiles tiles_of(int H, int W) {
    Tiles t;
    t.nx = (W + kTileW - 1) / kTileW;
    t.count = (int64_t)t.nx * ((H + kTileH - 1) / kTileH);
    return t;
}

__device__ __forceinline__ bool foreground(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ exclude, int64_t at) {
    return mask[at] != 0 && (exclude == nullptr || exclude[at] == 0);
}

// ---------------------------------------------------------------- the forest in LDS (launch 1)
// at most `a` steps: every step goes to a strictly smaller index
__device__ __forceinline__ int lds_find(const volatile int *lab, int a) {
    int p;
    while ((p = lab[a]) != a) a = p;
    return a;
}

// a retry follows only a lowering of lab[a] by another thread; labels are lowered finitely often
__device__ __forceinline__ void lds_unite(int *lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(kThreads) tile_label_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ exclude,
                                                              int32_t *__restrict__ parent, int N, int H, int W, int tiles_x,
                                                              int eight) {
    __shared__ int lab[kTile];
    const int tid = (int)threadIdx.x;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int64_t HW = (int64_t)H * W;
    for (int n = (int)blockIdx.y; n < N; n += (int)gridDim.y) {
        const int64_t base = (int64_t)n * HW;
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int y = y0 + l / kTileW, x = x0 + l % kTileW;
            lab[l] = (y < H && x < W && foreground(mask, exclude, base + (int64_t)y * W + x)) ? l : -1;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int ly = l / kTileW, lx = l % kTileW;
            if (((const volatile int *)lab)[l] < 0) continue;
            // (a label never becomes or stops being -1: the test of a neighbour needs no care)
            if (lx > 0 && ((const volatile int *)lab)[l - 1] >= 0) lds_unite(lab, l, l - 1);
            if (ly > 0) {
                if (((const volatile int *)lab)[l - kTileW] >= 0) lds_unite(lab, l, l - kTileW);
                if (eight) {
                    if (lx > 0 && ((const volatile int *)lab)[l - kTileW - 1] >= 0) lds_unite(lab, l, l - kTileW - 1);
                    if (lx < kTileW - 1 && ((const volatile int *)lab)[l - kTileW + 1] >= 0) lds_unite(lab, l, l - kTileW + 1);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int y = y0 + l / kTileW, x = x0 + l % kTileW;
            if (y >= H || x >= W) continue;
            int out = -1;
            if (lab[l] >= 0) {
                const int r = lds_find(lab, l);
                out = (int)((int64_t)(y0 + r / kTileW) * W + (x0 + r % kTileW));
            }
            parent[base + (int64_t)y * W + x] = out;
        }
        __syncthreads();                                  // (lab is rewritten for the next image)
    }
}

// ---------------------------------------------------------------- the forest in global memory (launch 2)
// the only way a value of `parent` is read in this launch
__device__ __forceinline__ int peek(int32_t *p) { return atomicMin(p, kNoLabel); }

// at most `a` steps: every step goes to a strictly smaller index
__device__ __forceinline__ int global_find(int32_t *par, int a) {
    int p;
    while ((p = peek(par + a)) != a) a = p;
    return a;
}

// a retry follows only a lowering of par[a] by another thread; labels are lowered finitely often
__device__ __forceinline__ void global_unite(int32_t *par, int a, int b) {
    for (;;) {
        a = global_find(par, a);
        b = global_find(par, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ void unite_across(int32_t *par, int p, int y, int x, int H, int W) {
    if (y < 0 || y >= H || x < 0 || x >= W) return;
    const int q = (int)((int64_t)y * W + x);
    if (peek(par + q) >= 0) global_unite(par, p, q);
}

// (no __restrict__ on parent: other workgroups write it while this one reads, through atomics on both sides)
__global__ void __launch_bounds__(kMergeThreads) border_merge_kernel(int32_t *parent, int N, int H, int W, int tiles_x, int eight) {
    const int tid = (int)threadIdx.x;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    if (tid >= kTileW + kTileH) return;
    const bool top = tid < kTileW;
    const int x = top ? x0 + tid : x0, y = top ? y0 : y0 + (tid - kTileW);
    if (y >= H || x >= W || (top ? y0 == 0 : x0 == 0)) return;
    const int64_t HW = (int64_t)H * W;
    const int p = (int)((int64_t)y * W + x);
    for (int n = (int)blockIdx.y; n < N; n += (int)gridDim.y) {
        int32_t *par = parent + (int64_t)n * HW;
        if (peek(par + p) < 0) continue;
        if (top) {                                        // the row above: N, and the two diagonals (also into the corner tiles)
            unite_across(par, p, y - 1, x, H, W);
            if (eight) {
                unite_across(par, p, y - 1, x - 1, H, W);
                unite_across(par, p, y - 1, x + 1, H, W);
            }
        } else {                                          // the column to the left: W, and the two diagonals
            unite_across(par, p, y, x - 1, H, W);
            if (eight) {
                unite_across(par, p, y - 1, x - 1, H, W);
                unite_across(par, p, y + 1, x - 1, H, W);
            }
        }
    }
}

// ---------------------------------------------------------------- launch 3: every pixel to its root
// The bin of a pixel: the pixel it points at if that lies in its own tile, else (a root of launch 1 that was hung under another
// tile's) the pixel itself.  A bin is keyed by a foreground pixel of the component, so all its pixels share their root.
__device__ __forceinline__ int bin_of(int par, int l, int y0, int x0, int W) {
    const int py = par / W, px = par - py * W;
    const int by = py - y0, bx = px - x0;
    return (by >= 0 && by < kTileH && bx >= 0 && bx < kTileW) ? by * kTileW + bx : l;
}

template <bool kLabels>
__global__ void __launch_bounds__(kThreads) resolve_kernel(const int32_t *__restrict__ parent, int32_t *__restrict__ out,
                                                           uint32_t *__restrict__ area, int N, int H, int W, int tiles_x) {
    __shared__ uint32_t cnt[kTile];
    __shared__ int root_of[kTile];
    __shared__ int hkey[kCache];                          // the roots this tile met (direct-mapped; a root that finds its entry taken
    __shared__ uint32_t hcnt[kCache];                     // goes to global memory on its own) and their pixel counts
    const int tid = (int)threadIdx.x;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int64_t HW = (int64_t)H * W;
    for (int n = (int)blockIdx.y; n < N; n += (int)gridDim.y) {
        const int32_t *par = parent + (int64_t)n * HW;
#pragma unroll
        for (int k = 0; k < kMine; ++k) cnt[tid + k * kThreads] = 0u;
        if (tid < kCache) hkey[tid] = -1, hcnt[tid] = 0u;
        __syncthreads();
        int bin[kMine];
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int y = y0 + l / kTileW, x = x0 + l % kTileW;
            bin[k] = -1;
            if (y >= H || x >= W) continue;
            const int p = par[(int64_t)y * W + x];
            if (p < 0) continue;
            bin[k] = bin_of(p, l, y0, x0, W);
            atomicAdd(&cnt[bin[k]], 1u);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            if (cnt[l] == 0u) continue;
            int r = (int)((int64_t)(y0 + l / kTileW) * W + (x0 + l % kTileW));
            for (int p = par[r]; p != r; p = par[r]) r = p;                     // at most r steps: strictly decreasing
            root_of[l] = r;
            if (!kLabels) {                               // the bins of one root are added up in LDS first: a large component has many
                const uint32_t e = ((uint32_t)r * 2654435761u) >> 26;
                const int old = atomicCAS(&hkey[e], -1, r);
                if (old == -1 || old == r)
                    atomicAdd(&hcnt[e], cnt[l]);
                else
                    atomicAdd(area + (int64_t)n * HW + r, cnt[l]);
            }
        }
        __syncthreads();
        if (!kLabels && tid < kCache && hkey[tid] >= 0) atomicAdd(area + (int64_t)n * HW + hkey[tid], hcnt[tid]);
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int y = y0 + l / kTileW, x = x0 + l % kTileW;
            if (y >= H || x >= W) continue;
            const int r = bin[k] >= 0 ? root_of[bin[k]] : -1;
            out[(int64_t)n * HW + (int64_t)y * W + x] = kLabels ? r + 1 : r;
        }
        __syncthreads();                                  // (cnt and root_of are rewritten for the next image)
    }
}

// ---------------------------------------------------------------- raft_remove_small_components, launch 4
__global__ void __launch_bounds__(kThreads) keep_kernel(const int32_t *__restrict__ root, const uint32_t *__restrict__ area,
                                                        uint8_t *__restrict__ out, int N, int64_t HW, uint32_t min_area) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= HW) return;
    for (int n = (int)blockIdx.y; n < N; n += (int)gridDim.y) {
        const int64_t at = (int64_t)n * HW + i;
        const int r = root[at];
        out[at] = (r >= 0 && area[(int64_t)n * HW + r] >= min_area) ? 1 : 0;
    }
}

// ---------------------------------------------------------------- raft_find_objects, launch 4: the candidates
__global__ void __launch_bounds__(kThreads) candidates_kernel(const int32_t *__restrict__ root, const uint32_t *__restrict__ area,
                                                              u64 *__restrict__ cand, uint32_t *__restrict__ cand_count, int N,
                                                              int64_t HW, uint32_t min_area, uint32_t bound) {
    __shared__ uint32_t s_n, s_base;
    const int tid = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
    for (int n = (int)blockIdx.y; n < N; n += (int)gridDim.y) {
        if (tid == 0) s_n = 0u;
        __syncthreads();
        u64 key = 0;                                      // (0: none; a key is never 0)
        if (i < HW && root[(int64_t)n * HW + i] == (int)i) {
            const uint32_t a = area[(int64_t)n * HW + i];
            if (a >= min_area) key = ((u64)a << 32) | (u64)(0xFFFFFFFFu - (uint32_t)i);
        }
        // ONE global atomic per workgroup reserves the slots of its candidates (docs/NOTEBOOK.md section 42)
        const uint32_t first = key != 0 ? atomicAdd(&s_n, 1u) : 0u;
        __syncthreads();
        if (tid == 0 && s_n != 0u) s_base = atomicAdd(cand_count + n, s_n);
        __syncthreads();
        if (key != 0 && s_base + first < bound) cand[(int64_t)n * bound + s_base + first] = key;      // (always: the bound is exact)
        __syncthreads();
    }
}

// ---------------------------------------------------------------- launch 5: the K largest keys, sorted (point_detect.hip's select)
struct Sums {
    u64 sx, sy, su, sv, cnt;      // su, sv: two's complement
    int x0, y0, x1, y1;
};
static_assert(sizeof(Sums) == 56, "include/raft_hip.h states the record's size");

__device__ __forceinline__ void send(Sums *rec, int x0, int y0, int x1, int y1, u64 sx, u64 sy, u64 su, u64 sv, uint32_t cnt) {
    atomicMin(&rec->x0, x0), atomicMin(&rec->y0, y0), atomicMax(&rec->x1, x1), atomicMax(&rec->y1, y1);
    atomicAdd(&rec->sx, sx), atomicAdd(&rec->sy, sy);
    if (cnt != 0u) atomicAdd(&rec->su, su), atomicAdd(&rec->sv, sv), atomicAdd(&rec->cnt, (u64)cnt);
}

__global__ void __launch_bounds__(kSelectThreads) select_kernel(const u64 *__restrict__ cand, const uint32_t *__restrict__ cand_count,
                                                                uint32_t bound, int K, int64_t HW, uint32_t *__restrict__ area_map,
                                                                int32_t *__restrict__ count, int32_t *__restrict__ area,
                                                                Sums *__restrict__ sums) {
    __shared__ u64 keys[kMaxObjects];
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
    while (n2 < kept) n2 <<= 1;                                                 // (<= kMaxObjects)
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
                if (slot < (uint32_t)kMaxObjects) keys[slot] = v;
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
        const int64_t at = (int64_t)n * K + i;
        int32_t a = 0;
        if (i < kept) {
            const u64 v = keys[i];
            a = (int32_t)(uint32_t)(v >> 32);
            area_map[(int64_t)n * HW + (0xFFFFFFFFu - (uint32_t)v)] = kChosen | (uint32_t)i;
        }
        area[at] = a;
        for (int c = 0; c < kCopies; ++c) {
            Sums *rec = sums + at * kCopies + c;
            rec->sx = 0, rec->sy = 0, rec->su = 0, rec->sv = 0, rec->cnt = 0;
            rec->x0 = kNoLabel, rec->y0 = kNoLabel, rec->x1 = -1, rec->y1 = -1;
        }
    }
    if (tid == 0) count[n] = kept;
}

// ---------------------------------------------------------------- launch 6: slot labels, boxes and sums
__device__ __forceinline__ bool flow_counts(float u) { return u >= -kFlowLimit && u <= kFlowLimit; }      // (a NaN fails)

__global__ void __launch_bounds__(kThreads) stats_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ root,
                                                         const uint32_t *__restrict__ area_map, const float *__restrict__ flow,
                                                         int32_t *__restrict__ labels, Sums *__restrict__ sums, int N, int H, int W,
                                                         int K, int tiles_x) {
    __shared__ int bx0[kTile], by0[kTile], bx1[kTile], by1[kTile], bslot[kTile];
    __shared__ u64 bsx[kTile], bsy[kTile], bsu[kTile], bsv[kTile];
    __shared__ uint32_t bcnt[kTile];
    // the slots this tile met (direct-mapped by slot; a slot that finds its entry taken goes to global memory bin by bin)
    __shared__ int ckey[kCache], cx0[kCache], cy0[kCache], cx1[kCache], cy1[kCache];
    __shared__ u64 csx[kCache], csy[kCache], csu[kCache], csv[kCache];
    __shared__ uint32_t ccnt[kCache];
    const int copy = (int)(blockIdx.x & (unsigned)(kCopies - 1));
    const int tid = (int)threadIdx.x;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int64_t HW = (int64_t)H * W;
    for (int n = (int)blockIdx.y; n < N; n += (int)gridDim.y) {
        const int64_t base = (int64_t)n * HW;
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            bx0[l] = kNoLabel, by0[l] = kNoLabel, bx1[l] = -1, by1[l] = -1, bslot[l] = -1;
            bsx[l] = 0, bsy[l] = 0, bsu[l] = 0, bsv[l] = 0, bcnt[l] = 0u;
        }
        if (tid < kCache) {
            ckey[tid] = -1, cx0[tid] = kNoLabel, cy0[tid] = kNoLabel, cx1[tid] = -1, cy1[tid] = -1;
            csx[tid] = 0, csy[tid] = 0, csu[tid] = 0, csv[tid] = 0, ccnt[tid] = 0u;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int y = y0 + l / kTileW, x = x0 + l % kTileW;
            if (y >= H || x >= W) continue;
            const int64_t at = base + (int64_t)y * W + x;
            const int r = root[at];
            int slot = -1;
            if (r >= 0) {
                const uint32_t a = area_map[base + r];
                if (a & kChosen) slot = (int)(a & ~kChosen);
            }
            if (labels != nullptr) labels[at] = slot + 1;
            if (slot < 0) continue;
            const int b = bin_of(parent[at], l, y0, x0, W);
            bslot[b] = slot;                              // (every pixel of a bin writes the same value)
            atomicMin(&bx0[b], x), atomicMin(&by0[b], y), atomicMax(&bx1[b], x), atomicMax(&by1[b], y);
            atomicAdd(&bsx[b], (u64)x), atomicAdd(&bsy[b], (u64)y);
            if (flow != nullptr) {
                const float u = flow[2 * at], v = flow[2 * at + 1];
                if (flow_counts(u) && flow_counts(v)) {
                    atomicAdd(&bsu[b], (u64)(long long)rintf(u * 256.f));
                    atomicAdd(&bsv[b], (u64)(long long)rintf(v * 256.f));
                    atomicAdd(&bcnt[b], 1u);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int l = tid + k * kThreads;
            const int slot = bslot[l];
            if (slot < 0) continue;
            const int e = slot & (kCache - 1);
            const int old = atomicCAS(&ckey[e], -1, slot);
            if (old == -1 || old == slot) {               // the bins of one slot are put together in LDS first
                atomicMin(&cx0[e], bx0[l]), atomicMin(&cy0[e], by0[l]), atomicMax(&cx1[e], bx1[l]), atomicMax(&cy1[e], by1[l]);
                atomicAdd(&csx[e], bsx[l]), atomicAdd(&csy[e], bsy[l]);
                if (bcnt[l] != 0u) atomicAdd(&csu[e], bsu[l]), atomicAdd(&csv[e], bsv[l]), atomicAdd(&ccnt[e], bcnt[l]);
            } else {
                send(sums + ((int64_t)n * K + slot) * kCopies + copy, bx0[l], by0[l], bx1[l], by1[l], bsx[l], bsy[l], bsu[l], bsv[l], bcnt[l]);
            }
        }
        __syncthreads();
        if (tid < kCache && ckey[tid] >= 0)
            send(sums + ((int64_t)n * K + ckey[tid]) * kCopies + copy, cx0[tid], cy0[tid], cx1[tid], cy1[tid], csx[tid], csy[tid], csu[tid],
                 csv[tid], ccnt[tid]);
        __syncthreads();                                  // (the bins and the table are rewritten for the next image)
    }
}

// ---------------------------------------------------------------- launch 7: the two divisions
__global__ void __launch_bounds__(kThreads) finish_kernel(const Sums *__restrict__ sums, const int32_t *__restrict__ count,
                                                          const int32_t *__restrict__ area, int32_t *__restrict__ boxes,
                                                          float *__restrict__ centroid, float *__restrict__ mean_flow, int N, int K) {
    const int64_t at = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= (int64_t)N * K) return;
    const int n = (int)(at / K), slot = (int)(at - (int64_t)n * K);
    float cx = -1.f, cy = -1.f, mu = 0.f, mv = 0.f;
    int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
    if (slot < count[n]) {
        u64 sx = 0, sy = 0, su = 0, sv = 0, cnt = 0;
        x0 = kNoLabel, y0 = kNoLabel;
        for (int c = 0; c < kCopies; ++c) {               // integer sums, minima and maxima: any order
            const Sums *rec = sums + at * kCopies + c;
            sx += rec->sx, sy += rec->sy, su += rec->su, sv += rec->sv, cnt += rec->cnt;
            x0 = rec->x0 < x0 ? rec->x0 : x0, y0 = rec->y0 < y0 ? rec->y0 : y0;
            x1 = rec->x1 > x1 ? rec->x1 : x1, y1 = rec->y1 > y1 ? rec->y1 : y1;
        }
        const double a = (double)area[at];
        cx = (float)((double)sx / a), cy = (float)((double)sy / a);
        if (cnt != 0) {
            const double d = 256.0 * (double)cnt;
            mu = (float)((double)(long long)su / d), mv = (float)((double)(long long)sv / d);
        }
    }
    boxes[4 * at] = x0, boxes[4 * at + 1] = y0, boxes[4 * at + 2] = x1, boxes[4 * at + 3] = y1;
    centroid[2 * at] = cx, centroid[2 * at + 1] = cy;
    if (mean_flow != nullptr) mean_flow[2 * at] = mu, mean_flow[2 * at + 1] = mv;
}

// ---------------------------------------------------------------- host side
static inline bool sizes_ok(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return false;
    if ((int64_t)H * W > (((int64_t)1 << 31) - 2)) return false;
    return (int64_t)H * W <= (((int64_t)1 << 31) - 1) / N;                      // N * H * W < 2^31
}

static inline int64_t up8(int64_t v) { return (v + 7) & ~(int64_t)7; }

// No image holds more components of at least min_area pixels than this: components are disjoint, so floor(H W / min_area); under
// 8-connectivity no two of the four pixels of a 2 x 2 cell lie in different components, so ceil(H / 2) * ceil(W / 2); under
// 4-connectivity no two horizontal neighbours of a row, nor vertical ones, so at most the larger colour class of a checkerboard.
static inline int64_t candidate_bound(int H, int W, int connectivity, int min_area) {
    const int64_t HW = (int64_t)H * W;
    const int64_t by_shape = connectivity == 8 ? (int64_t)((H + 1) / 2) * ((W + 1) / 2) : (HW + 1) / 2;
    const int64_t by_area = HW / min_area;
    return by_area < by_shape ? by_area : by_shape;
}

struct Workspace {
    int32_t *parent, *root;
    uint32_t *area, *cand_count;      // (adjacent: one memset zeroes both)
    u64 *cand;
    Sums *sums;
    int64_t bound;
};

// parent: N*H*W * 4 | root: N*H*W * 4 | area: N*H*W * 4, cand_count: N * 4 | keys: N * bound * 8 | records: N * RAFT_OBJECTS_MAX * 8 * 56
// (every part padded to 8 bytes): 12 bytes per pixel and the lists.  Returns the size in bytes (0: refused); with a `base`, the parts.
static inline int64_t workspace_layout(void *base, int N, int H, int W, int connectivity, int min_area, Workspace *w) {
    if (!sizes_ok(N, H, W) || (connectivity != 4 && connectivity != 8) || min_area < 1) return 0;
    const int64_t npix = (int64_t)N * H * W;
    const int64_t bound = candidate_bound(H, W, connectivity, min_area);
    const int64_t o_root = up8(npix * 4), o_area = o_root + up8(npix * 4), o_cand = o_area + up8((npix + N) * 4);
    const int64_t o_sums = o_cand + (int64_t)N * bound * 8;
    if (base != nullptr) {
        char *p = (char *)base;
        w->parent = (int32_t *)p, w->root = (int32_t *)(p + o_root), w->area = (uint32_t *)(p + o_area), w->cand_count = w->area + npix;
        w->cand = (u64 *)(p + o_cand), w->sums = (Sums *)(p + o_sums), w->bound = bound;
    }
    return o_sums + (int64_t)N * kMaxObjects * kCopies * (int64_t)sizeof(Sums);
}

static inline unsigned grid_y(int N) { return (unsigned)(N < kMaxGridY ? N : kMaxGridY); }

// launches 1 and 2
static inline int build_forest(const uint8_t *mask, const uint8_t *exclude, int32_t *parent, int N, int H, int W, int connectivity,
                               hipStream_t st) {
    const Tiles t = tiles_of(H, W);
    const dim3 grid((unsigned)t.count, grid_y(N));
    tile_label_kernel<<<grid, kThreads, 0, st>>>(mask, exclude, parent, N, H, W, t.nx, connectivity == 8);
    RAFT_TRY(raft_launch_status());
    border_merge_kernel<<<grid, kMergeThreads, 0, st>>>(parent, N, H, W, t.nx, connectivity == 8);
    return raft_launch_status();
}

// launches 1 to 3 of the two entries that count, with their memset
static inline int build_areas(const uint8_t *mask, const uint8_t *exclude, const Workspace &w, int N, int H, int W, int connectivity,
                              hipStream_t st) {
    const Tiles t = tiles_of(H, W);
    RAFT_TRY((int)hipMemsetAsync(w.area, 0, ((size_t)N * H * W + (size_t)N) * 4, st));
    RAFT_TRY(build_forest(mask, exclude, w.parent, N, H, W, connectivity, st));
    resolve_kernel<false><<<dim3((unsigned)t.count, grid_y(N)), kThreads, 0, st>>>(w.parent, w.root, w.area, N, H, W, t.nx);
    return raft_launch_status();
}

static inline bool shape_ok(int N, int H, int W, int connectivity, int min_area) {
    return sizes_ok(N, H, W) && (connectivity == 4 || connectivity == 8) && min_area >= 1;
}

}   // namespace

extern "C" int64_t raft_components_workspace_bytes(int N, int H, int W, int connectivity, int min_area) {
    return workspace_layout(nullptr, N, H, W, connectivity, min_area, nullptr);
}

extern "C" int raft_label_components(const uint8_t *mask, const uint8_t *exclude, int32_t *labels, int N, int H, int W,
                                     int connectivity, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(mask);
    RAFT_REQUIRE_PTR(labels);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(shape_ok(N, H, W, connectivity, 1), RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)labels) & 3u) == 0, RAFT_E_ALIGN);
    Workspace w;
    RAFT_REQUIRE(workspace_layout(workspace, N, H, W, connectivity, 1, &w) > 0, RAFT_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    RAFT_TRY(build_forest(mask, exclude, w.parent, N, H, W, connectivity, st));
    const Tiles t = tiles_of(H, W);
    resolve_kernel<true><<<dim3((unsigned)t.count, grid_y(N)), kThreads, 0, st>>>(w.parent, labels, nullptr, N, H, W, t.nx);
    return raft_launch_status();
}

extern "C" int raft_remove_small_components(const uint8_t *mask, const uint8_t *exclude, uint8_t *out, int N, int H, int W,
                                            int connectivity, int min_area, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(mask);
    RAFT_REQUIRE_PTR(out);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(shape_ok(N, H, W, connectivity, min_area), RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)workspace) & 7u) == 0, RAFT_E_ALIGN);
    Workspace w;
    RAFT_REQUIRE(workspace_layout(workspace, N, H, W, connectivity, min_area, &w) > 0, RAFT_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    RAFT_TRY(build_areas(mask, exclude, w, N, H, W, connectivity, st));
    const int64_t HW = (int64_t)H * W;
    keep_kernel<<<dim3((unsigned)((HW + kThreads - 1) / kThreads), grid_y(N)), kThreads, 0, st>>>(w.root, w.area, out, N, HW,
                                                                                                (uint32_t)min_area);
    return raft_launch_status();
}

extern "C" int raft_find_objects(const uint8_t *mask, const uint8_t *exclude, const float *flow, int32_t *labels, int32_t *count,
                                 int32_t *area, int32_t *boxes, float *centroid, float *mean_flow, int N, int H, int W, int connectivity,
                                 int min_area, int max_objects, void *workspace, void *stream) {
    RAFT_REQUIRE_PTR(mask);
    RAFT_REQUIRE_PTR(count);
    RAFT_REQUIRE_PTR(area);
    RAFT_REQUIRE_PTR(boxes);
    RAFT_REQUIRE_PTR(centroid);
    RAFT_REQUIRE_PTR(workspace);
    RAFT_REQUIRE(shape_ok(N, H, W, connectivity, min_area), RAFT_E_SHAPE);
    RAFT_REQUIRE(max_objects >= 1 && max_objects <= kMaxObjects, RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)workspace) & 7u) == 0, RAFT_E_ALIGN);
    RAFT_REQUIRE(((((uintptr_t)flow) | ((uintptr_t)labels) | ((uintptr_t)count) | ((uintptr_t)area) | ((uintptr_t)boxes) |
                   ((uintptr_t)centroid) | ((uintptr_t)mean_flow)) & 3u) == 0, RAFT_E_ALIGN);
    Workspace w;
    RAFT_REQUIRE(workspace_layout(workspace, N, H, W, connectivity, min_area, &w) > 0, RAFT_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    RAFT_TRY(build_areas(mask, exclude, w, N, H, W, connectivity, st));
    const int64_t HW = (int64_t)H * W;
    const Tiles t = tiles_of(H, W);
    const int K = max_objects;
    if (mean_flow == nullptr) flow = nullptr;
    if (flow == nullptr) mean_flow = nullptr;
    candidates_kernel<<<dim3((unsigned)((HW + kThreads - 1) / kThreads), grid_y(N)), kThreads, 0, st>>>(w.root, w.area, w.cand, w.cand_count,
                                                                                                      N, HW, (uint32_t)min_area,
                                                                                                      (uint32_t)w.bound);
    RAFT_TRY(raft_launch_status());
    select_kernel<<<(unsigned)N, kSelectThreads, 0, st>>>(w.cand, w.cand_count, (uint32_t)w.bound, K, HW, w.area, count, area, w.sums);
    RAFT_TRY(raft_launch_status());
    stats_kernel<<<dim3((unsigned)t.count, grid_y(N)), kThreads, 0, st>>>(w.parent, w.root, w.area, flow, labels, w.sums, N, H, W, K, t.nx);
    RAFT_TRY(raft_launch_status());
    finish_kernel<<<(unsigned)(((int64_t)N * K + kThreads - 1) / kThreads), kThreads, 0, st>>>(w.sums, count, area, boxes, centroid, mean_flow, N, K);
    return raft_launch_status();
}

// FlowAugmentor on the device (reference tf_raft/datasets/augmentor.py:9-129, dataset.py:87-102): colour jitter, the occlusion
// eraser on frame 2, random rescale / stretch, flips and the random crop, composed into ONE gather.  The host draws a record of
// parameters per sample (tf_raft_amd/augment.py); a thread of the gather owns one pixel of the crop, walks back through crop,
// flips and resize to its four source taps, passes the taps of both frames through the colour map (frame 2: through the
// rectangle test first), blends them with cv2.resize's INTER_LINEAR arithmetic and writes both uint8 crops, the rescaled flow and
// `valid`.  The eraser's fill colour is the truncated mean of colour-mapped frame 2: a first kernel leaves 64 partial channel
// sums per erased sample in a small buffer and the gather's workgroups add them up; nothing returns to the host.
//
// SparseFlowAugmentor (augmentor.py:132-267) is the second gather of this file: the same frames, and the reference's scatter of the
// sparse flow restated per output pixel.
//
// DESIGN.md section 10 states every formula.  They are written so that a host can reproduce each result bit for bit (the test
// stand-ins tests/augstub do): integer arithmetic where OpenCV uses fixed point, and individually rounded IEEE operations
// elsewhere -- contraction into fused multiply-adds is switched off for this file, and the roundings that matter are spelled
// with the __f*_rn / __d*_rn intrinsics as well.
#include "loss_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSumBlocks = RAFT_AUGMENT_SUM_BLOCKS;
constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = kThreads / kTileW;

struct Rgb {
    int r, g, b;
};

// OpenCV's 8-bit RGB -> HSV division tables: sdiv[i] = round((255 << 12) / i), hdiv[i] = round((180 << 12) / (6 i)), [0] = 0
__device__ __forceinline__ void fill_hsv_tables(int *sdiv, int *hdiv) {
    for (int i = threadIdx.x; i < 256; i += kThreads) {
        sdiv[i] = i ? (int)rint((double)(255 << 12) / (double)i) : 0;
        hdiv[i] = i ? (int)rint((double)(180 << 12) / __dmul_rn(6.0, (double)i)) : 0;
    }
}

__device__ __forceinline__ int round_u8(float x) {   // saturate_cast<uchar>(float): round half to even, then clamp
    const int i = (int)rintf(x);
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}

struct ColorMap {
    int flags;          // bit 0 brightness / contrast, bit 1 hue / saturation / value
    float alpha, beta;
    double hue, sat, val;
};

__device__ __forceinline__ ColorMap color_map_of(const RaftAugmentParams &p, int frame) {
    return {p.color[frame], p.alpha[frame], p.beta[frame], p.hue[frame], p.sat[frame], p.val[frame]};
}

__device__ __forceinline__ int brightness_contrast(int v, float alpha, float beta) {
    float t = __fadd_rn(__fmul_rn((float)v, alpha), beta);
    t = fminf(fmaxf(t, 0.f), 255.f);
    return (int)t;                                   // truncation, as numpy's astype(uint8)
}

__device__ __forceinline__ int shift_clip(int v, double shift) {
    double t = __dadd_rn((double)v, shift);
    t = fmin(fmax(t, 0.0), 255.0);
    return (int)t;
}

__device__ __forceinline__ Rgb apply_color(Rgb c, const ColorMap &m, const int *sdiv, const int *hdiv) {
    if (m.flags & 1) {
        c.r = brightness_contrast(c.r, m.alpha, m.beta);
        c.g = brightness_contrast(c.g, m.alpha, m.beta);
        c.b = brightness_contrast(c.b, m.alpha, m.beta);
    }
    if (m.flags & 2) {
        // RGB -> HSV, 8 bit, H in [0, 180)
        const int v0 = max(c.r, max(c.g, c.b)), vmin = min(c.r, min(c.g, c.b)), diff = v0 - vmin;
        int s = (diff * sdiv[v0] + (1 << 11)) >> 12;
        int h = v0 == c.r ? c.g - c.b : (v0 == c.g ? c.b - c.r + 2 * diff : c.r - c.g + 4 * diff);
        h = (h * hdiv[diff] + (1 << 11)) >> 12;
        if (h < 0) h += 180;
        // the shifts: np.mod(h + hue, 180), np.clip(s + sat, 0, 255), np.clip(v + val, 0, 255) in double, truncated
        double a = __dadd_rn((double)h, m.hue);
        if (a >= 180.0)
            a = __dsub_rn(a, 180.0);
        else if (a < 0.0)
            a = __dadd_rn(a, 180.0);
        h = (int)a;
        s = shift_clip(s, m.sat);
        const int v = shift_clip(v0, m.val);
        // HSV -> RGB in float
        const float hf = __fmul_rn((float)h, (float)(1.0 / 30.0));
        int sector = (int)floorf(hf);
        const float f = __fsub_rn(hf, (float)sector);
        if (sector >= 6) sector -= 6;
        const float sf = __fmul_rn((float)s, (float)(1.0 / 255.0)), vf = __fmul_rn((float)v, (float)(1.0 / 255.0));
        const float p = __fmul_rn(vf, __fsub_rn(1.f, sf));
        const float q = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, f)));
        const float t = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, __fsub_rn(1.f, f))));
        float r, g, b;
        switch (sector) {
            case 0: r = vf, g = t, b = p; break;
            case 1: r = q, g = vf, b = p; break;
            case 2: r = p, g = vf, b = t; break;
            case 3: r = p, g = q, b = vf; break;
            case 4: r = t, g = p, b = vf; break;
            default: r = vf, g = p, b = q; break;
        }
        c.r = round_u8(__fmul_rn(r, 255.f));
        c.g = round_u8(__fmul_rn(g, 255.f));
        c.b = round_u8(__fmul_rn(b, 255.f));
    }
    return c;
}

__device__ __forceinline__ Rgb load_rgb(const uint8_t *img, int64_t pixel) {
    const uint8_t *p = img + pixel * 3;
    return {p[0], p[1], p[2]};
}

// ------------------------------------------------------------------ channel sums of colour-mapped frame 2
__global__ void __launch_bounds__(kThreads) augment_sums_kernel(const uint8_t *__restrict__ img2, const RaftAugmentParams *__restrict__ params,
                                                                unsigned *__restrict__ partial, int HW) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ unsigned wsum[kThreads / 64][3];
    const int n = blockIdx.y;
    const RaftAugmentParams &p = params[n];
    if (p.n_rect <= 0) return;                       // uniform over the workgroup
    const ColorMap m = color_map_of(p, 1);
    if (m.flags & 2) {
        fill_hsv_tables(sdiv, hdiv);
        __syncthreads();
    }
    const uint8_t *img = img2 + (int64_t)n * HW * 3;
    unsigned sr = 0, sg = 0, sb = 0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < HW; i += kSumBlocks * kThreads) {
        const Rgb c = apply_color(load_rgb(img, i), m, sdiv, hdiv);
        sr += c.r;
        sg += c.g;
        sb += c.b;
    }
    sr = raft_wave_sum(sr);
    sg = raft_wave_sum(sg);
    sb = raft_wave_sum(sb);
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6][0] = sr;
        wsum[threadIdx.x >> 6][1] = sg;
        wsum[threadIdx.x >> 6][2] = sb;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned t = 0;
        for (int k = 0; k < kThreads / 64; ++k) t += wsum[k][threadIdx.x];
        partial[((int64_t)n * kSumBlocks + blockIdx.x) * 4 + threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------ the gather
struct Axis {           // one axis of cv2.resize INTER_LINEAR for one destination index
    int s0, s1;         // the two source indices
    float w0, w1;       // float weights (1 - f, f)
    int i0, i1;         // 11-bit fixed-point weights
};

__device__ __forceinline__ Axis resize_axis(int d, double inv, int size) {
    const float c = (float)__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), inv), 0.5);
    int s = (int)floorf(c);
    float f = __fsub_rn(c, (float)s);
    if (s < 0) s = 0, f = 0.f;
    if (s >= size - 1) s = size - 1, f = 0.f;
    Axis a;
    a.s0 = s;
    a.s1 = min(s + 1, size - 1);
    a.w0 = __fsub_rn(1.f, f);
    a.w1 = f;
    a.i0 = (int)rintf(__fmul_rn(a.w0, 2048.f));
    a.i1 = (int)rintf(__fmul_rn(a.w1, 2048.f));
    return a;
}

__device__ __forceinline__ int blend_u8(int v00, int v01, int v10, int v11, const Axis &x, const Axis &y) {
    const int top = v00 * x.i0 + v01 * x.i1, bot = v10 * x.i0 + v11 * x.i1;          // HResizeLinear
    const int v = (((y.i0 * (top >> 4)) >> 16) + ((y.i1 * (bot >> 4)) >> 16) + 2) >> 2;    // VResizeLinear
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ float blend_f32(float v00, float v01, float v10, float v11, const Axis &x, const Axis &y) {
    const float top = __fadd_rn(__fmul_rn(v00, x.w0), __fmul_rn(v01, x.w1));
    const float bot = __fadd_rn(__fmul_rn(v10, x.w0), __fmul_rn(v11, x.w1));
    return __fadd_rn(__fmul_rn(top, y.w0), __fmul_rn(bot, y.w1));
}

__device__ __forceinline__ Rgb blend_rgb(const Rgb &a, const Rgb &b, const Rgb &c, const Rgb &d, const Axis &x, const Axis &y) {
    return {blend_u8(a.r, b.r, c.r, d.r, x, y), blend_u8(a.g, b.g, c.g, d.g, x, y), blend_u8(a.b, b.b, c.b, d.b, x, y)};
}

__device__ __forceinline__ void store_rgb(uint8_t *out, int64_t pixel, const Rgb &c) {
    uint8_t *o = out + pixel * 3;
    o[0] = (uint8_t)c.r;
    o[1] = (uint8_t)c.g;
    o[2] = (uint8_t)c.b;
}

// What the dense and the sparse gather share: the colour tables and the eraser's mean in LDS, then per thread the walk from a pixel
// of the crop back to its taps in the source and the two blended frames.
struct Shared {
    int sdiv[256], hdiv[256];
    int mean[3];
};

__device__ __forceinline__ void gather_prologue(Shared &sh, const RaftAugmentParams &p, const unsigned *__restrict__ partial, int n, int HW) {
    if ((p.color[0] | p.color[1]) & 2) fill_hsv_tables(sh.sdiv, sh.hdiv);
    if (p.n_rect > 0 && threadIdx.x < 64) {         // the first wave adds the partial sums up
        const unsigned *ps = partial + ((int64_t)n * kSumBlocks + threadIdx.x) * 4;
        const unsigned sr = raft_wave_sum(ps[0]), sg = raft_wave_sum(ps[1]), sb = raft_wave_sum(ps[2]);
        if (threadIdx.x == 0) {
            const unsigned hw = (unsigned)HW;
            sh.mean[0] = (int)(sr / hw);
            sh.mean[1] = (int)(sg / hw);
            sh.mean[2] = (int)(sb / hw);
        }
    }
    __syncthreads();
}

struct Taps {
    int x, y;           // without resize: the one source pixel
    Axis ax, ay;        // with resize: the four taps and their weights
};

__device__ __forceinline__ Taps taps_of(const RaftAugmentParams &p, int xr, int yr, int H, int W) {
    Taps t;
    if (!p.resize) {
        t.x = min(max(xr, 0), W - 1);
        t.y = min(max(yr, 0), H - 1);
    } else {
        t.ax = resize_axis(xr, p.inv_fx, W);
        t.ay = resize_axis(yr, p.inv_fy, H);
    }
    return t;
}

__device__ __forceinline__ void gather_frames(const Shared &sh, const RaftAugmentParams &p, const Taps &t, const uint8_t *__restrict__ f1,
                                              const uint8_t *__restrict__ f2, int W, Rgb &c1, Rgb &c2) {
    const ColorMap m1 = color_map_of(p, 0), m2 = color_map_of(p, 1);
    const int n_rect = min(max(p.n_rect, 0), 2);
    auto tap2 = [&](int y, int x) -> Rgb {         // frame 2: rectangle test, then the colour map
        for (int r = 0; r < n_rect; ++r)
            if (x >= p.rect[r][0] && y >= p.rect[r][1] && x < p.rect[r][2] && y < p.rect[r][3]) return {sh.mean[0], sh.mean[1], sh.mean[2]};
        return apply_color(load_rgb(f2, (int64_t)y * W + x), m2, sh.sdiv, sh.hdiv);
    };
    if (!p.resize) {
        c1 = apply_color(load_rgb(f1, (int64_t)t.y * W + t.x), m1, sh.sdiv, sh.hdiv);
        c2 = tap2(t.y, t.x);
    } else {
        const Axis &ax = t.ax, &ay = t.ay;
        const int64_t r0 = (int64_t)ay.s0 * W, r1 = (int64_t)ay.s1 * W;
        c1 = blend_rgb(apply_color(load_rgb(f1, r0 + ax.s0), m1, sh.sdiv, sh.hdiv), apply_color(load_rgb(f1, r0 + ax.s1), m1, sh.sdiv, sh.hdiv),
                       apply_color(load_rgb(f1, r1 + ax.s0), m1, sh.sdiv, sh.hdiv), apply_color(load_rgb(f1, r1 + ax.s1), m1, sh.sdiv, sh.hdiv), ax, ay);
        c2 = blend_rgb(tap2(ay.s0, ax.s0), tap2(ay.s0, ax.s1), tap2(ay.s1, ax.s0), tap2(ay.s1, ax.s1), ax, ay);
    }
}

__global__ void __launch_bounds__(kThreads) augment_gather_kernel(const uint8_t *__restrict__ img1, const uint8_t *__restrict__ img2,
                                                                  const float *__restrict__ flow, const RaftAugmentParams *__restrict__ params,
                                                                  const unsigned *__restrict__ partial, uint8_t *__restrict__ out1,
                                                                  uint8_t *__restrict__ out2, float *__restrict__ out_flow,
                                                                  float *__restrict__ valid, int H, int W, int h, int w) {
    __shared__ Shared sh;
    const int n = blockIdx.z;
    const RaftAugmentParams &p = params[n];
    gather_prologue(sh, p, partial, n, H * W);
    const int j = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), i = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i >= h || j >= w) return;
    int xr = p.x0 + j, yr = p.y0 + i;               // in the resized frame, flips undone
    if (p.flip_h) xr = p.W1 - 1 - xr;
    if (p.flip_v) yr = p.H1 - 1 - yr;
    const int64_t base = (int64_t)n * H * W;
    const float *fl = flow + base * 2;
    const Taps t = taps_of(p, xr, yr, H, W);
    Rgb c1, c2;
    gather_frames(sh, p, t, img1 + base * 3, img2 + base * 3, W, c1, c2);
    float u, v;
    if (!p.resize) {
        u = fl[((int64_t)t.y * W + t.x) * 2];
        v = fl[((int64_t)t.y * W + t.x) * 2 + 1];
    } else {
        const Axis &ax = t.ax, &ay = t.ay;
        const int64_t r0 = (int64_t)ay.s0 * W, r1 = (int64_t)ay.s1 * W;
        const float2 a = ((const float2 *)fl)[r0 + ax.s0], b = ((const float2 *)fl)[r0 + ax.s1];
        const float2 c = ((const float2 *)fl)[r1 + ax.s0], d = ((const float2 *)fl)[r1 + ax.s1];
        u = blend_f32(a.x, b.x, c.x, d.x, ax, ay);
        v = blend_f32(a.y, b.y, c.y, d.y, ax, ay);
    }
    // flow * [fx, fy] is a double product in the reference (float32 array times a list), the flips change signs
    double du = p.resize ? __dmul_rn((double)u, p.fx) : (double)u, dv = p.resize ? __dmul_rn((double)v, p.fy) : (double)v;
    if (p.flip_h) du = -du;
    if (p.flip_v) dv = -dv;
    const int64_t o = ((int64_t)n * h + i) * w + j;
    store_rgb(out1, o, c1);
    store_rgb(out2, o, c2);
    out_flow[o * 2] = (float)du;
    out_flow[o * 2 + 1] = (float)dv;
    valid[o] = (fabs(du) < 1000.0 && fabs(dv) < 1000.0) ? 1.f : 0.f;
}

// ------------------------------------------------------------------ the sparse gather
// SparseFlowAugmentor (reference augmentor.py:132-267).  The frames go the dense way.  The reference resizes flow and validity with a
// scatter (resize_sparse_flow_map, augmentor.py:183-215): a valid source (x, y) lands on (rint(x f), rint(y f)), and of the sources that
// land on one target the last in row-major order stays.  The forward map is separable and monotone per axis, so the sources of a
// target form a small rectangle and the scatter is this gather: find the rectangle with the forward formula itself, scan it from the
// highest row and the highest column, and take the first source with valid >= 1.  DESIGN.md section 11.
constexpr int kSparseMaxReach = 5;      // the host refuses factors below 1 / 8: ceil(0.5 / f) + 1 <= 5

// Source indices s in [0, size) with rint(double(s) * f) == target: [lo, hi], empty when lo > hi.  Such a source lies within
// 0.5 / f of target / f; the candidates are floor(q) - reach .. ceil(q) + reach with q = target * (1 / f) and reach = ceil(0.5 / f) + 1,
// where the + 1 also covers the last-place error of multiplying by the inverse instead of dividing.
__device__ __forceinline__ void sparse_sources(int target, double f, double inv, int size, int &lo, int &hi) {
    const int reach = min(max((int)ceil(__dmul_rn(0.5, inv)) + 1, 1), kSparseMaxReach);
    const double q = __dmul_rn((double)target, inv);
    const int first = max((int)floor(q) - reach, 0), last = min((int)ceil(q) + reach, size - 1);
    lo = size;
    hi = -1;
    // last - first <= 2 * reach + 1 already; the second condition only gives the compiler a static trip count
    for (int s = first; s <= last && s - first < 2 * kSparseMaxReach + 2; ++s)
        if ((int)rint(__dmul_rn((double)s, f)) == target) {
            lo = min(lo, s);
            hi = s;
        }
}

__global__ void __launch_bounds__(kThreads) augment_gather_sparse_kernel(const uint8_t *__restrict__ img1, const uint8_t *__restrict__ img2,
                                                                         const float *__restrict__ flow, const float *__restrict__ valid_in,
                                                                         const RaftAugmentParams *__restrict__ params,
                                                                         const unsigned *__restrict__ partial, uint8_t *__restrict__ out1,
                                                                         uint8_t *__restrict__ out2, float *__restrict__ out_flow,
                                                                         float *__restrict__ valid_out, int H, int W, int h, int w) {
    __shared__ Shared sh;
    const int n = blockIdx.z;
    const RaftAugmentParams &p = params[n];
    gather_prologue(sh, p, partial, n, H * W);
    const int j = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), i = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i >= h || j >= w) return;
    int xr = p.x0 + j;                              // in the resized frame, the flip undone (there is no vertical flip)
    const int yr = p.y0 + i;
    if (p.flip_h) xr = p.W1 - 1 - xr;
    const int64_t base = (int64_t)n * H * W;
    const float2 *fl = (const float2 *)flow + base;
    const float *va = valid_in + base;
    const Taps t = taps_of(p, xr, yr, H, W);
    Rgb c1, c2;
    gather_frames(sh, p, t, img1 + base * 3, img2 + base * 3, W, c1, c2);
    float u = 0.f, v = 0.f, ok = 0.f;
    if (!p.resize) {                                // plain copies, of invalid pixels too, validity with whatever value it holds
        const int64_t s = (int64_t)t.y * W + t.x;
        const float2 a = fl[s];
        u = a.x;
        v = a.y;
        ok = va[s];
    } else if (xr > 0 && yr > 0) {                  // the reference keeps targets with xx > 0 and yy > 0, strictly
        int x_lo, x_hi, y_lo, y_hi;
        sparse_sources(xr, p.fx, p.inv_fx, W, x_lo, x_hi);
        sparse_sources(yr, p.fx, p.inv_fx, H, y_lo, y_hi);
        for (int y = y_hi; y >= y_lo && ok == 0.f; --y)
            for (int x = x_hi; x >= x_lo; --x)
                if (va[(int64_t)y * W + x] >= 1.f) {
                    const float2 a = fl[(int64_t)y * W + x];
                    u = (float)__dmul_rn((double)a.x, p.fx);        // float32 array times a list: a double product, narrowed on assignment
                    v = (float)__dmul_rn((double)a.y, p.fx);
                    ok = 1.f;
                    break;
                }
    }
    if (p.flip_h) u = -u;
    const int64_t o = ((int64_t)n * h + i) * w + j;
    store_rgb(out1, o, c1);
    store_rgb(out2, o, c2);
    out_flow[o * 2] = u;
    out_flow[o * 2 + 1] = v;
    valid_out[o] = ok;
}

}   // namespace

extern "C" int raft_augment_params_bytes(void) { return (int)sizeof(RaftAugmentParams); }

extern "C" int raft_augment_sums_u8(const uint8_t *img2, const RaftAugmentParams *params, uint32_t *partial, int N, int H, int W, void *stream) {
    RAFT_REQUIRE_PTR(img2);
    RAFT_REQUIRE_PTR(params);
    RAFT_REQUIRE_PTR(partial);
    RAFT_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)H * W <= ((int64_t)1 << 24), RAFT_E_SHAPE);
    augment_sums_kernel<<<dim3(kSumBlocks, N), kThreads, 0, (hipStream_t)stream>>>(img2, params, partial, H * W);
    return raft_launch_status();
}

extern "C" int raft_augment_gather_u8(const uint8_t *img1, const uint8_t *img2, const float *flow, const RaftAugmentParams *params,
                                      const uint32_t *partial, uint8_t *out1, uint8_t *out2, float *out_flow, float *valid,
                                      int N, int H, int W, int h, int w, void *stream) {
    RAFT_REQUIRE_PTR(img1);
    RAFT_REQUIRE_PTR(img2);
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(params);
    RAFT_REQUIRE_PTR(partial);
    RAFT_REQUIRE_PTR(out1);
    RAFT_REQUIRE_PTR(out2);
    RAFT_REQUIRE_PTR(out_flow);
    RAFT_REQUIRE_PTR(valid);
    RAFT_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)H * W <= ((int64_t)1 << 24) && (int64_t)h * w <= ((int64_t)1 << 24), RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_ceil_div(h, kTileH) <= 65535, RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)flow) & 7) == 0, RAFT_E_ALIGN);
    const dim3 grid(raft_ceil_div(w, kTileW), raft_ceil_div(h, kTileH), N);
    augment_gather_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(img1, img2, flow, params, partial, out1, out2, out_flow, valid, H, W, h, w);
    return raft_launch_status();
}

extern "C" int raft_augment_gather_sparse_u8(const uint8_t *img1, const uint8_t *img2, const float *flow, const float *valid_in,
                                             const RaftAugmentParams *params, const uint32_t *partial, uint8_t *out1, uint8_t *out2,
                                             float *out_flow, float *valid_out, int N, int H, int W, int h, int w, void *stream) {
    RAFT_REQUIRE_PTR(img1);
    RAFT_REQUIRE_PTR(img2);
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(valid_in);
    RAFT_REQUIRE_PTR(params);
    RAFT_REQUIRE_PTR(partial);
    RAFT_REQUIRE_PTR(out1);
    RAFT_REQUIRE_PTR(out2);
    RAFT_REQUIRE_PTR(out_flow);
    RAFT_REQUIRE_PTR(valid_out);
    RAFT_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)H * W <= ((int64_t)1 << 24) && (int64_t)h * w <= ((int64_t)1 << 24), RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_ceil_div(h, kTileH) <= 65535, RAFT_E_SHAPE);
    RAFT_REQUIRE((((uintptr_t)flow) & 7) == 0, RAFT_E_ALIGN);
    const dim3 grid(raft_ceil_div(w, kTileW), raft_ceil_div(h, kTileH), N);
    augment_gather_sparse_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(img1, img2, flow, valid_in, params, partial, out1, out2, out_flow,
                                                                             valid_out, H, W, h, w);
    return raft_launch_status();
}

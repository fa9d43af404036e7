// Flow colour coding on the device: the Middlebury colour wheel of the reference's tf_raft/datasets/flow_viz.py:20-132
// (flow_to_image, the call that follows model([image1, image2]) in tf_raft/training.py:82), two launches per call:
//
//   raft_flow_rad_max_f32   per image, partial maxima of sqrt(u*u + v*v)       (flow_viz.py:124-128)
//   raft_flow_to_image_u8   per pixel, the colour of (u, v) / (rad_max + 1e-5)  (flow_viz.py:129-131 and 85-105)
//
// Both see the flow through the crop-or-pad window of image_ops.hip (raft_axis_window): a source (N, Hs, Ws, 2) at a destination
// size (Ht, Wt); destination pixels outside the window are zero flow, source pixels outside it do not exist.
//
// The arithmetic is the reference's, operation by operation, in the types NumPy 2 gives each of them: float32 up to the wheel
// position fk, float64 from `f = fk - k0` on (float32 minus int32 is float64 there, and the wheel is float64).  Every product
// and sum is rounded on its own -- contraction is switched off for this file, the library's -ffp-contract=on would fuse
// u*u + v*v and (1 - f) * c0 + f * c1 -- and float32 division and square root are the correctly rounded ones hipcc emits by
// default.  The one step that is NOT NumPy's is atan2: NumPy's float32 arctan2 is not correctly rounded, so there is nothing
// to reproduce bit by bit; it is computed in double and rounded once (DESIGN.md section 13 has the consequence: a channel value
// can differ by one level where 255 * col lies within 1e-4 of an integer).
//
// No atomics, no memset, no host synchronisation: the first kernel writes every one of its kFlowVizPartials partial maxima per
// image, the second folds them in its prologue (a maximum of non-negative floats is exact in any order).
#include "loss_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kFlowVizPartials = 128;      // partial maxima per image = workgroups per image of the first kernel
constexpr int kWheelCols = 55;

struct Wheel {
    double v[kWheelCols][3];               // colour wheel / 255.0, as `tmp[k0] / 255.0` gives it (flow_viz.py:97-98)
};

// flow_viz.py:20-67: six hue segments, each with one channel at 255 and one ramping by floor(255 * i / n) up or down.
// (255 * i / n in float64 and floored equals the integer quotient: an inexact quotient is at least 1 / 15 from an integer.)
constexpr Wheel make_wheel() {
    constexpr int seg[6][4] = {{15, 0, 1, +1}, {6, 1, 0, -1}, {4, 1, 2, +1}, {11, 2, 1, -1}, {13, 2, 0, +1}, {6, 0, 2, -1}};
    Wheel w{};
    int col = 0;
    for (int s = 0; s < 6; ++s) {
        for (int i = 0; i < seg[s][0]; ++i) {
            const int step = 255 * i / seg[s][0];
            w.v[col + i][seg[s][1]] = 255 / 255.0;
            w.v[col + i][seg[s][2]] = (seg[s][3] > 0 ? step : 255 - step) / 255.0;
        }
        col += seg[s][0];
    }
    return w;
}

__constant__ const Wheel kWheel = make_wheel();

struct VizGeom {
    int N, Hs, Ws, Ht, Wt;
    int crop_y, pad_y, ext_y, crop_x, pad_x, ext_x;
    float clip;                            // >= 0: np.clip(flow, 0, clip) first; anything else: none
};

// np.clip(x, 0, clip) as NumPy 2.2 evaluates it: a negative value becomes +0, -0.0 stays -0.0, NaN stays
__device__ __forceinline__ float viz_clip(float x, float clip) {
    x = x < 0.f ? 0.f : x;
    return x > clip ? clip : x;
}

// One wave owns one source row of the window at a time; blockIdx.y walks the images.  partial[n * kFlowVizPartials + blockIdx.x].
__global__ void __launch_bounds__(256) flow_rad_max_kernel(const float2 *__restrict__ flow, float *__restrict__ partial, VizGeom g) {
    __shared__ float wave_part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool clipped = g.clip >= 0.f;
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float m = 0.f;
        for (int r = blockIdx.x * 4 + wave; r < g.ext_y; r += kFlowVizPartials * 4) {
            const float2 *row = flow + (((int64_t)n * g.Hs + g.crop_y + r) * g.Ws + g.crop_x);
            for (int x = lane; x < g.ext_x; x += 64) {
                float2 f = row[x];
                if (clipped) {
                    f.x = viz_clip(f.x, g.clip);
                    f.y = viz_clip(f.y, g.clip);
                }
                m = fmaxf(m, sqrtf(f.x * f.x + f.y * f.y));      // flow_viz.py:127 (fmaxf: a NaN magnitude does not count)
            }
        }
        m = raft_wave_max(m);
        __syncthreads();                                          // the previous image's wave_part has been read
        if (lane == 0) wave_part[wave] = m;
        __syncthreads();
        if (threadIdx.x == 0)
            partial[(int64_t)n * kFlowVizPartials + blockIdx.x] = fmaxf(fmaxf(wave_part[0], wave_part[1]), fmaxf(wave_part[2], wave_part[3]));
    }
}

// flow_viz.py:129-131 and 88-105 for one pixel: the three channel values in bits 0-7, 8-15, 16-23, in the order they are stored.
__device__ __forceinline__ uint32_t flow_colour(float u, float v, const VizGeom &g, float d, bool bgr, const double (*wheel)[3]) {
    if (g.clip >= 0.f) {
        u = viz_clip(u, g.clip);
        v = viz_clip(v, g.clip);
    }
    u = u / d;
    v = v / d;
    const float rad = sqrtf(u * u + v * v);
    const float a = (float)atan2((double)-v, (double)-u) / 3.14159274101257324f;     // float32(np.pi)
    const float fk = (a + 1.f) / 2.f * (float)(kWheelCols - 1);
    const float fl = floorf(fk);
    // inside the wheel whatever the flow holds (a NaN compares false and lands on 0)
    const int k0 = fl >= 0.f ? (fl <= (float)(kWheelCols - 1) ? (int)fl : kWheelCols - 1) : 0;
    const int k1 = k0 + 1 == kWheelCols ? 0 : k0 + 1;
    const double f = (double)fk - (double)k0;
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double col = (1.0 - f) * wheel[k0][i] + f * wheel[k1][i];
        col = rad <= 1.f ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
        const double level = floor(255.0 * col);
        const uint32_t byte = level >= 0.0 ? (level <= 255.0 ? (uint32_t)level : 255u) : 0u;
        packed |= byte << (8 * (bgr ? 2 - i : i));
    }
    return packed;
}

// pixel r of image n's destination -> its flow (zero outside the window)
__device__ __forceinline__ float2 viz_fetch(const float2 *__restrict__ flow, const VizGeom &g, int64_t n, int y, int x) {
    const int sy = y - g.pad_y, sx = x - g.pad_x;
    if (sy < 0 || sy >= g.ext_y || sx < 0 || sx >= g.ext_x) return make_float2(0.f, 0.f);
    return flow[((n * g.Hs + g.crop_y + sy) * g.Ws + g.crop_x + sx)];
}

struct alignas(4) Quad {
    uint32_t w[3];                         // four pixels = 12 bytes
};

// The picture of image n is the HW * 3 bytes from image + n * HW * 3.  `head` pixels in front bring the address to a multiple
// of 4 (3 * head = -head mod 4, so head = address & 3); from there a lane owns 4 consecutive pixels = three whole dwords;
// the up to 3 pixels in front and up to 3 behind are stored byte by byte by the first workgroup of the image.
__global__ void __launch_bounds__(256) flow_to_image_kernel(const float2 *__restrict__ flow, const float *__restrict__ partial,
                                                            uint8_t *__restrict__ image, VizGeom g, int bgr, float fixed_rad_max) {
    __shared__ double wheel[kWheelCols][3];
    for (int i = threadIdx.x; i < kWheelCols * 3; i += 256) wheel[i / 3][i % 3] = kWheel.v[i / 3][i % 3];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int HW = g.Ht * g.Wt;
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float rad_max = fixed_rad_max;
        if (!(fixed_rad_max > 0.f)) {
            const float *p = partial + (int64_t)n * kFlowVizPartials;
            rad_max = raft_wave_max(fmaxf(p[lane], p[lane + 64]));
        }
        const float d = rad_max + 1e-5f;                          // flow_viz.py:130: float32 + float32(1e-5)
        uint8_t *out = image + (int64_t)n * HW * 3;
        const int head = min((int)((uintptr_t)out & 3u), HW);
        const int quads = (HW - head) >> 2;
        for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
            const int r = head + 4 * q;
            int y = (int)((unsigned)r / (unsigned)g.Wt), x = r - y * g.Wt;
            float2 f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f[j] = viz_fetch(flow, g, n, y, x);
                if (++x == g.Wt) x = 0, ++y;
            }
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = flow_colour(f[j].x, f[j].y, g, d, bgr != 0, wheel);
            Quad o;
            o.w[0] = c[0] | (c[1] << 24);
            o.w[1] = (c[1] >> 8) | (c[2] << 16);
            o.w[2] = (c[2] >> 16) | (c[3] << 8);
            *(Quad *)(out + (int64_t)3 * r) = o;
        }
        const int edge = HW - 4 * quads;                          // head + tail pixels, at most 6
        if (blockIdx.x == 0 && (int)threadIdx.x < edge) {
            const int t = threadIdx.x;
            const int r = t < head ? t : t + 4 * quads;
            const int y = (int)((unsigned)r / (unsigned)g.Wt), x = r - y * g.Wt;
            const float2 f = viz_fetch(flow, g, n, y, x);
            const uint32_t c = flow_colour(f.x, f.y, g, d, bgr != 0, wheel);
            out[(int64_t)3 * r] = (uint8_t)c;
            out[(int64_t)3 * r + 1] = (uint8_t)(c >> 8);
            out[(int64_t)3 * r + 2] = (uint8_t)(c >> 16);
        }
    }
}

int viz_geom(const float *flow, int N, int Hs, int Ws, int Ht, int Wt, float clip, VizGeom *g) {
    RAFT_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ht > 0 && Wt > 0, RAFT_E_SHAPE);
    // a row's elements, and the pixels of one picture, are counted in ints
    RAFT_REQUIRE((int64_t)Ws * 2 <= 0x7fffffff && (int64_t)Wt * 3 <= 0x7fffffff, RAFT_E_SHAPE);
    RAFT_REQUIRE((int64_t)Ht * Wt <= 0x7fffffff - 1024 * 1024, RAFT_E_SHAPE);      // (with room for a last grid stride)
    RAFT_REQUIRE((((uintptr_t)flow) & 7u) == 0, RAFT_E_ALIGN);                     // read as float2
    g->N = N, g->Hs = Hs, g->Ws = Ws, g->Ht = Ht, g->Wt = Wt;
    raft_axis_window(Hs, Ht, &g->crop_y, &g->pad_y, &g->ext_y);
    raft_axis_window(Ws, Wt, &g->crop_x, &g->pad_x, &g->ext_x);
    g->clip = clip >= 0.f ? clip : -1.f;
    return RAFT_OK;
}

}   // namespace

extern "C" int64_t raft_flow_to_image_workspace_floats(int N) { return N > 0 ? (int64_t)N * kFlowVizPartials : 0; }

extern "C" int raft_flow_rad_max_f32(const float *flow, float *partial, int N, int Hs, int Ws, int Ht, int Wt, float clip, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(partial);
    VizGeom g;
    RAFT_TRY(viz_geom(flow, N, Hs, Ws, Ht, Wt, clip, &g));
    const dim3 grid(kFlowVizPartials, (unsigned)(N < 65535 ? N : 65535));
    flow_rad_max_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const float2 *)flow, partial, g);
    return raft_launch_status();
}

extern "C" int raft_flow_to_image_u8(const float *flow, const float *partial, uint8_t *image, int N, int Hs, int Ws, int Ht, int Wt,
                                     float clip, int bgr, float fixed_rad_max, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(image);
    if (!(fixed_rad_max > 0.f)) RAFT_REQUIRE_PTR(partial);
    VizGeom g;
    RAFT_TRY(viz_geom(flow, N, Hs, Ws, Ht, Wt, clip, &g));
    const int64_t blocks = ((int64_t)Ht * Wt / 4 + 255) / 256;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks < 1024 ? blocks : 1024), (unsigned)(N < 65535 ? N : 65535));
    flow_to_image_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const float2 *)flow, partial, image, g, bgr, fixed_rad_max);
    return raft_launch_status();
}

// Convolution launchers, the single-convolution entry points and the two small special convolutions of the update blocks
// (reference tf_raft/layers/update.py:14, 93) for gfx950.  The update blocks and the loops that sequence them: update_block.hip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_halo.h"
#include "conv_wino.h"
#include "conv_wino1d.h"
#include "conv_wino4.h"

// ------------------------------------------------------------------------------------------------
// dispatch of the direct (halo-tiled) convolution kernel (tile: launch_plan.h raft_halo_plan)
// ------------------------------------------------------------------------------------------------
int raft_launch_conv(const ConvArgs &a_in, int kh, int kw, int epi, hipStream_t s, HaloPlan p) {
    ConvArgs a = a_in;
    if (a.Hi == 0) {   // plain stride-1 'same' convolution
        a.Hi = a.H;
        a.Wi = a.W;
        a.pt = (kh - 1) / 2;
        a.pl = (kw - 1) / 2;
    }
    if (a.c0 <= 0 || a.c0 % 32 || a.c1 < 0 || a.c1 % 32 || a.npad <= 0 || a.npad % 64) return RAFT_E_UNSUPPORTED;
    RAFT_TRY(raft_check_operands(a, kh * kw, RAFT_CHECK_ALL));
    if (!raft_halo_code_valid(100 + 10 * p.th + p.tn, a.npad)) return RAFT_E_UNSUPPORTED;
    if (kh == 1 && kw == 1) return raft_launch_conv_halo_1x1(a, p.th, p.tn, epi, s);
    if (kh == 3 && kw == 3) return raft_launch_conv_halo_3x3(a, p.th, p.tn, epi, s);
    if (kh == 1 && kw == 5) return raft_launch_conv_halo_1x5(a, p.th, p.tn, epi, s);
    if (kh == 5 && kw == 1) return raft_launch_conv_halo_5x1(a, p.th, p.tn, epi, s);
    return RAFT_E_UNSUPPORTED;
}

// The single-convolution entry points: one validation, one argument block, the family's default plan under the caller's hint.
static int single_conv(int family, int kh, int kw, int mo, const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                       const float *wp, const float *bias, int B, int H, int W, int npad, int nvalid, int act, float scale,
                       float *out, int ldo, void *stream, int hint) {
    RAFT_REQUIRE_PTR(a0);
    RAFT_REQUIRE_PTR(wp);
    RAFT_REQUIRE_PTR(bias);
    RAFT_REQUIRE_PTR(out);
    RAFT_REQUIRE(c1 == 0 || a1 != nullptr, RAFT_E_NULL);
    RAFT_REQUIRE(B > 0 && H > 0 && W > 0 && nvalid > 0 && nvalid <= npad && ldo >= nvalid, RAFT_E_SHAPE);
    RAFT_REQUIRE(lda0 >= c0 && (c1 == 0 || lda1 >= c1), RAFT_E_SHAPE);
    RAFT_REQUIRE(act == RAFT_ACT_NONE || act == RAFT_ACT_RELU, RAFT_E_UNSUPPORTED);
    ConvArgs a = {};
    a.a0 = a0; a.a1 = a1; a.lda0 = lda0; a.lda1 = lda1; a.c0 = c0; a.c1 = c1;
    a.wp = wp; a.bias = bias; a.B = B; a.H = H; a.W = W;
    a.npad = npad; a.nvalid = nvalid; a.hid = 0; a.scale = scale;
    a.o0 = out; a.ldo0 = ldo;
    const int epi = act == RAFT_ACT_RELU ? EPI_RELU : EPI_LINEAR;
    hipStream_t s = (hipStream_t)stream;
    switch (family) {
        case RAFT_FAM_WINO: return raft_launch_conv_wino(a, epi, s, raft_wino_plan(B, H, W, c0, c1, npad, true, hint));
        case RAFT_FAM_WINO4: return raft_launch_conv_wino4(a, epi, s, raft_wino4_plan(B, H, W, c0, c1, npad, true, hint));
        case RAFT_FAM_WINO1D: return raft_launch_conv_wino1d(a, kh, kw, epi, s, raft_wino1d_plan(B, H, W, c0, c1, npad, kh, mo, hint));
    }
    return raft_launch_conv(a, kh, kw, epi, s, raft_halo_plan(B, H, W, npad, kh, kw, hint));
}

extern "C" int raft_conv2d_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                               const float *wp, const float *bias, int B, int H, int W, int kh, int kw, int npad,
                               int nvalid, int act, float scale, float *out, int ldo, void *stream) {
    return single_conv(RAFT_FAM_HALO, kh, kw, 0, a0, lda0, c0, a1, lda1, c1, wp, bias, B, H, W, npad, nvalid, act, scale, out, ldo,
                       stream, raft_concurrency());
}

extern "C" int raft_conv2d_winograd_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                                        const float *wp, const float *bias, int B, int H, int W, int npad, int nvalid,
                                        int act, float scale, float *out, int ldo, void *stream) {
    return single_conv(RAFT_FAM_WINO, 3, 3, 0, a0, lda0, c0, a1, lda1, c1, wp, bias, B, H, W, npad, nvalid, act, scale, out, ldo,
                       stream, raft_concurrency());
}

extern "C" int raft_conv2d_winograd4_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                                         const float *wp, const float *bias, int B, int H, int W, int npad, int nvalid,
                                         int act, float scale, float *out, int ldo, void *stream) {
    return single_conv(RAFT_FAM_WINO4, 3, 3, 0, a0, lda0, c0, a1, lda1, c1, wp, bias, B, H, W, npad, nvalid, act, scale, out, ldo,
                       stream, raft_concurrency());
}

extern "C" int raft_conv1d_winograd_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                                        const float *wp, const float *bias, int B, int H, int W, int kh, int kw,
                                        int npad, int nvalid, int act, float scale, float *out, int ldo, void *stream) {
    return single_conv(RAFT_FAM_WINO1D, kh, kw, 2, a0, lda0, c0, a1, lda1, c1, wp, bias, B, H, W, npad, nvalid, act, scale, out, ldo,
                       stream, raft_concurrency());
}

extern "C" int raft_conv1d_winograd4_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                                         const float *wp, const float *bias, int B, int H, int W, int kh, int kw,
                                         int npad, int nvalid, int act, float scale, float *out, int ldo, void *stream) {
    return single_conv(RAFT_FAM_WINO1D, kh, kw, 4, a0, lda0, c0, a1, lda1, c1, wp, bias, B, H, W, npad, nvalid, act, scale, out, ldo,
                       stream, raft_concurrency());
}

// ------------------------------------------------------------------------------------------------
// convf1: 7x7, Cin = 2 (flow), relu -- a GEMM [pixels x 98] . [98 x COUT] on fp32 MFMA 16x16x4.  [reference update.py:93]
// A workgroup owns 4 rows x 16 columns of pixels; wave w takes row w (one MFMA row block) and all COUT channels.  The
// (4 + 6) x (16 + 6) x 2 flow halo tile lives in LDS (zeros outside the image = 'same' padding); a k-step is four
// consecutive k = (ky * 7 + kx) * 2 + c of the Keras-layout kernel [k][n], so the A operand of lane (pixel r, k-group g)
// is the halo value at (row + ky, r + kx, c) and the B operand the kernel row k, both from LDS.
// K = 98 is padded to 100 with zero kernel rows.  The first version of this layer held the 98 weights of a lane's channel in
// registers and walked the pixels with wave-uniform LDS reads on the VALU: 18.9 us per launch at B = 4 for 0.36 GFLOP
// (profiles/r05b); this one is bound by its launch.
// ------------------------------------------------------------------------------------------------
template <int COUT>
__global__ void __launch_bounds__(256) conv7x7_c2_kernel(const float *__restrict__ flow, const float *__restrict__ wk,
                                                         const float *__restrict__ bias, int B, int H, int W,
                                                         float *__restrict__ out, int ldo) {
    constexpr int TH = 4, TW = 16, HW = TW + 6, NJ = COUT / 16, KQ = 25, LDW = COUT + 16;
    static_assert(COUT == 64 || COUT == 128, "conv7x7_c2: COUT must be 64 or 128");
    __shared__ float sf[(TH + 6) * HW * 2];
    // the whole kernel [k][n], rows 98 and 99 zero; row stride COUT + 16: the four k-groups of a B fragment read rows
    // k .. k + 3, 16 banks apart.  Staged with ONE round of coalesced loads per workgroup: fragments fetched from global
    // memory inside the k loop serialise on their L2 round trips (one wave per SIMD, nothing to hide them behind)
    __shared__ __attribute__((aligned(16))) float sw[4 * KQ * LDW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int xt = (W + TW - 1) / TW, yt = (H + TH - 1) / TH;
    const int x0 = (blockIdx.x % xt) * TW, y0 = ((blockIdx.x / xt) % yt) * TH, b = blockIdx.x / (xt * yt);
    {   // every load of the staging phase is issued before the first LDS write (unconditional, clamped addresses): a
        // load / wait / store loop costs one L2 round trip per iteration -- 13 of them were most of this kernel's 16 us
        constexpr int NW = (4 * KQ * (COUT / 4) + 255) / 256;
        f32x4 tw[NW];
#pragma unroll
        for (int u = 0; u < NW; ++u) {
            const int i = tid + 256 * u, k = min(i / (COUT / 4), 97), c4 = i % (COUT / 4);
            tw[u] = *(const f32x4 *)(wk + k * COUT + c4 * 4);
        }
        const int i0 = tid, i1 = min(tid + 256, (TH + 6) * HW - 1);
        const int ya = y0 - 3 + i0 / HW, xa = x0 - 3 + i0 % HW, yb = y0 - 3 + i1 / HW, xb = x0 - 3 + i1 % HW;
        const bool oka = (unsigned)ya < (unsigned)H && (unsigned)xa < (unsigned)W;
        const bool okb = (unsigned)yb < (unsigned)H && (unsigned)xb < (unsigned)W;
        const float2 fa = ((const float2 *)flow)[oka ? ((int64_t)b * H + ya) * W + xa : 0];
        const float2 fb = ((const float2 *)flow)[okb ? ((int64_t)b * H + yb) * W + xb : 0];
        static_assert((TH + 6) * HW <= 512, "two halo items per thread");
#pragma unroll
        for (int u = 0; u < NW; ++u) {
            const int i = tid + 256 * u, k = i / (COUT / 4), c4 = i % (COUT / 4);
            if (k < 4 * KQ) *(f32x4 *)(sw + k * LDW + c4 * 4) = k < 98 ? tw[u] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (i0 < (TH + 6) * HW) ((float2 *)sf)[i0] = oka ? fa : make_float2(0.f, 0.f);
        if (tid + 256 < (TH + 6) * HW) ((float2 *)sf)[tid + 256] = okb ? fb : make_float2(0.f, 0.f);
    }
    __syncthreads();
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
    for (int q = 0; q < KQ; ++q) {
        const int k = 4 * q + g;
        const int kk = k < 98 ? k : 0, ky = kk / 14, rem = kk - ky * 14;        // rem = kx * 2 + c; rows 98, 99 of sw are zero
        const float av = sf[((wv + ky) * HW + r) * 2 + rem];                   // ((row + ky) * HW + r + kx) * 2 + c
        float bv[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bv[j] = sw[k * LDW + j * 16 + r];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[j], 0, 0, 0);
    }
    // D[row = pixel 4 g + e of the wave's row][col = channel 16 j + r]
    const int y = y0 + wv;
    if (y >= H) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float bj = bias[j * 16 + r];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = x0 + 4 * g + e;
            if (x < W) out[(((int64_t)b * H + y) * W + x) * ldo + j * 16 + r] = fmaxf(acc[j][e] + bj, 0.f);
        }
    }
}

extern "C" int raft_conv7x7_c2_f32(const float *flow, const float *kernel, const float *bias, int cout, int B, int H, int W,
                                   float *out, int ldo, void *stream) {
    RAFT_REQUIRE_PTR(flow);
    RAFT_REQUIRE_PTR(kernel);
    RAFT_REQUIRE_PTR(bias);
    RAFT_REQUIRE_PTR(out);
    RAFT_REQUIRE(B > 0 && H > 0 && W > 0 && ldo >= cout, RAFT_E_SHAPE);
    RAFT_REQUIRE(raft_aligned16(kernel), RAFT_E_ALIGN);
    return raft_launch_conv7x7_c2(flow, kernel, bias, cout, B, H, W, out, ldo, (hipStream_t)stream);
}

int raft_launch_conv7x7_c2(const float *flow, const float *kernel, const float *bias, int cout, int B, int H, int W, float *out,
                           int ldo, hipStream_t s) {
    const int grid = B * ((H + 3) / 4) * ((W + 15) / 16);
    if (cout == 128)
        conv7x7_c2_kernel<128><<<grid, 256, 0, s>>>(flow, kernel, bias, B, H, W, out, ldo);
    else if (cout == 64)
        conv7x7_c2_kernel<64><<<grid, 256, 0, s>>>(flow, kernel, bias, B, H, W, out, ldo);
    else
        return RAFT_E_UNSUPPORTED;
    return raft_launch_status();
}

// ------------------------------------------------------------------------------------------------
// flow_head.conv2: 3x3, Cout = 2, fused with the coordinate update of the loop
//   delta = conv(x) + b; coords1 += delta; flow = coords1 - coords0    [update.py:14, model.py:97-102]
// One wavefront per 2 rows x 4 columns of pixels: lanes split the CIN channels (float4 / float2 per lane, the 9 x V x 2
// weights of the lane's channels in registers, one or two 16-byte loads per tap), the 4 x 6 input pixels of the eight
// windows are loaded once (24 independent loads in flight), giving 16 per-lane partial sums (8 pixels x 2 outputs).
// They are reduced across the 64 lanes by a transpose-reduction: four halving steps (xor 32, 16, 8, 4: each lane keeps
// half of its values and adds the partner's copies of them) leave one value per lane, two butterfly steps finish it.
// Lanes 0, 4, ..., 60 then own one (pixel, component) each and apply the coordinate update.
// (The first version served 1 x 4 pixels per wave and fetched its 72 weights with scalar loads: 22 load instructions
// per pixel against 5 here; 13.6 us per launch at B = 4 for a layer that reads 14.7 MB.)
// ------------------------------------------------------------------------------------------------
template <int CIN>
__global__ void __launch_bounds__(256) flowhead2_kernel(const float *__restrict__ x, int ldx,
                                                        const float *__restrict__ wk,   // [9][CIN][2]
                                                        const float *__restrict__ bias, int B, int H, int W,
                                                        float *__restrict__ delta, float *__restrict__ coords1,
                                                        float *__restrict__ flow, float *__restrict__ flow2,
                                                        int ldf2, float *__restrict__ flow3 = nullptr) {
    constexpr int V = CIN / 64;   // channels per lane (4 or 2)
    static_assert(V == 4 || V == 2, "flowhead2: CIN must be 256 or 128");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ngx = (W + 3) / 4, ngy = (H + 1) / 2;
    const int64_t g = (int64_t)blockIdx.x * 4 + wid;          // group of 2 x 4 pixels
    if (g >= (int64_t)B * ngy * ngx) return;                   // wave-uniform
    const int gx = (int)(g % ngx), gy = (int)((g / ngx) % ngy), b = (int)(g / ((int64_t)ngx * ngy));
    const int x0 = gx * 4, y0 = gy * 2;
    // per-lane weights: 9 taps x V channels x 2 outputs, contiguous as [v][o] at (t * CIN + lane * V) * 2
    float w0[9][V], w1[9][V];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float *src = wk + ((int64_t)t * CIN + lane * V) * 2;
#pragma unroll
        for (int h = 0; h < V / 2; ++h) {
            const f32x4 q = *(const f32x4 *)(src + 4 * h);
            w0[t][2 * h] = q[0]; w1[t][2 * h] = q[1]; w0[t][2 * h + 1] = q[2]; w1[t][2 * h + 1] = q[3];
        }
    }
    // the 4 x 6 input pixels (zero outside the image; the conditions are wave-uniform)
    float in[4][6][V];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int yy = y0 + r - 1, xx = x0 + c - 1;
#pragma unroll
            for (int v = 0; v < V; ++v) in[r][c][v] = 0.f;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float *src = x + (((int64_t)b * H + yy) * W + xx) * ldx + lane * V;
                if (V == 4) {
                    const f32x4 q = *(const f32x4 *)src;
                    in[r][c][0] = q[0]; in[r][c][1] = q[1]; in[r][c][2] = q[2]; in[r][c][3] = q[3];
                } else {
                    const float2 q = *(const float2 *)src;
                    in[r][c][0] = q.x; in[r][c][1] = q.y;
                }
            }
        }
    float acc[16];   // index = (row * 4 + pixel) * 2 + component
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float xv = in[r + t / 3][p + t % 3][v];
                    acc[(r * 4 + p) * 2] = fmaf(xv, w0[t][v], acc[(r * 4 + p) * 2]);
                    acc[(r * 4 + p) * 2 + 1] = fmaf(xv, w1[t][v], acc[(r * 4 + p) * 2 + 1]);
                }
    // transpose-reduction over the 64 lanes
    float a8[8], a4[4], a2[2], a1;
    {
        const bool hi = lane & 32;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float keep = hi ? acc[8 + i] : acc[i], send = hi ? acc[i] : acc[8 + i];
            a8[i] = keep + __shfl_xor(send, 32, 64);
        }
    }
    {
        const bool hi = lane & 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float keep = hi ? a8[4 + i] : a8[i], send = hi ? a8[i] : a8[4 + i];
            a4[i] = keep + __shfl_xor(send, 16, 64);
        }
    }
    {
        const bool hi = lane & 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float keep = hi ? a4[2 + i] : a4[i], send = hi ? a4[i] : a4[2 + i];
            a2[i] = keep + __shfl_xor(send, 8, 64);
        }
    }
    {
        const bool hi = lane & 4;
        const float keep = hi ? a2[1] : a2[0], send = hi ? a2[0] : a2[1];
        a1 = keep + __shfl_xor(send, 4, 64);
    }
    a1 += __shfl_xor(a1, 2, 64);
    a1 += __shfl_xor(a1, 1, 64);
    if ((lane & 3) == 0) {
        const int idx = lane >> 2;            // = (row * 4 + pixel) * 2 + component
        const int py = y0 + (idx >> 3), px = x0 + ((idx >> 1) & 3), comp = idx & 1;
        if (px < W && py < H) {
            const int64_t m = ((int64_t)b * H + py) * W + px;
            const float d = a1 + bias[comp];
            const float c = coords1[2 * m + comp] + d;
            coords1[2 * m + comp] = c;
            delta[2 * m + comp] = d;
            const float f = c - (float)(comp ? py : px);     // coords0 = (x, y) grid
            flow[2 * m + comp] = f;
            if (flow2) flow2[m * ldf2 + comp] = f;
            if (flow3) flow3[2 * m + comp] = f;       // the copy the (concurrent) mask branch of this iteration reads
        }
    }
}

int raft_launch_flowhead2(const float *x, int ldx, int cin, const float *wk, const float *bias, int B, int H, int W, float *delta,
                          float *coords1, float *flow, float *flow2, int ldf2, float *flow3, hipStream_t s) {
    const int grid = raft_ceil_div((int64_t)B * ((H + 1) / 2) * ((W + 3) / 4), 4);
    if (cin == 256)
        flowhead2_kernel<256><<<grid, 256, 0, s>>>(x, ldx, wk, bias, B, H, W, delta, coords1, flow, flow2, ldf2, flow3);
    else if (cin == 128)
        flowhead2_kernel<128><<<grid, 256, 0, s>>>(x, ldx, wk, bias, B, H, W, delta, coords1, flow, flow2, ldf2, flow3);
    else
        return RAFT_E_UNSUPPORTED;
    return raft_launch_status();
}

// ------------------------------------------------------------------------------------------------
// misc
// ------------------------------------------------------------------------------------------------
extern "C" int raft_version(void) { return RAFT_HIP_VERSION; }

extern "C" const char *raft_error_string(int rc) {
    switch (rc) {
        case RAFT_OK: return "ok";
        case RAFT_E_NULL: return "raft: required pointer is NULL";
        case RAFT_E_SHAPE: return "raft: invalid or inconsistent dimension";
        case RAFT_E_UNSUPPORTED: return "raft: configuration not instantiated (radius / channels / kernel size)";
        case RAFT_E_ALIGN: return "raft: pointer or leading dimension not 16-byte aligned";
    }
    if (rc > 0) return hipGetErrorString((hipError_t)rc);
    return "raft: unknown error";
}

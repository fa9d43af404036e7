// Convolution launchers, the two small special convolutions, and the BasicUpdateBlock sequencing
// (reference tf_raft/layers/update.py:5-153, tf_raft/model.py:84-109) for gfx950.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_halo.h"
#include "conv_wino.h"
#include "conv_wino1d.h"
#include "conv_wino4.h"

// mask.2 + RAFT.upsample_flow in one kernel (mask_upsample.hip)
int raft_launch_mask_upsample(const float *a, int lda, const float *wp, const float *bias, int npad, const float *flow, int B,
                              int h, int w, float scale, float *out, hipStream_t s, int max_wgs = 0);
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

// One layer of a loop plan: the weight copy of the chosen family, its launcher.
static int launch_layer(const ConvChoice &c, ConvArgs a, int kh, int kw, int epi, hipStream_t s) {
    a.wp = c.wt->wp;
    a.bias = c.wt->bias;
    a.npad = c.wt->npad;
    switch (c.family) {
        case RAFT_FAM_WINO: return raft_launch_conv_wino(a, epi, s, c.wino);
        case RAFT_FAM_WINO1D: return raft_launch_conv_wino1d(a, kh, kw, epi, s, c.wino1d);
        case RAFT_FAM_WINO4: return raft_launch_conv_wino4(a, epi, s, c.wino4);
    }
    return raft_launch_conv(a, kh, kw, epi, s, c.halo);
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
    const int grid = B * ((H + 3) / 4) * ((W + 15) / 16);
    if (cout == 128)
        conv7x7_c2_kernel<128><<<grid, 256, 0, (hipStream_t)stream>>>(flow, kernel, bias, B, H, W, out, ldo);
    else if (cout == 64)
        conv7x7_c2_kernel<64><<<grid, 256, 0, (hipStream_t)stream>>>(flow, kernel, bias, B, H, W, out, ldo);
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

// ------------------------------------------------------------------------------------------------
// state preparation  [model.py:84-89]
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) prepare_state_kernel(const float *__restrict__ cnet, int B, int h, int w,
                                                            int hdim, int cdim, float *__restrict__ net,
                                                            float *__restrict__ x, int ldx, int flow_slot,
                                                            float *__restrict__ corr, int ldc, int corr_used,
                                                            float *__restrict__ coords1, float *__restrict__ flow) {
    const int64_t M = (int64_t)B * h * w;
    const int per = hdim + cdim;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * per) return;
    const int64_t m = i / per;
    const int c = (int)(i - m * per);
    const float v = cnet[i];
    if (c < hdim)
        net[m * hdim + c] = tanhf(v);
    else
        x[m * ldx + (c - hdim)] = fmaxf(v, 0.f);
    if (c == 0) {
        const int px = (int)(m % w), py = (int)((m / w) % h);
        ((float2 *)coords1)[m] = make_float2((float)px, (float)py);
        ((float2 *)flow)[m] = make_float2(0.f, 0.f);
    }
    // GRU input tail [flow | zero pad]: the flow slot starts at 0 and is rewritten every iteration
    if (c < ldx - flow_slot) x[m * ldx + flow_slot + c] = 0.f;
    // zero pad channels of the lookup output (never written by the lookup, read by convc1)
    if (c < ldc - corr_used) corr[m * ldc + corr_used + c] = 0.f;
}

// ------------------------------------------------------------------------------------------------
// BasicUpdateBlock
// workspace (floats per pixel): cor1 256 | corflo 256 [cor2 192 | flo2 64] | flo1 128 | z 128 | rh 128 | fm 512
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int WS_COR1 = 0, WS_CORFLO = 256, WS_FLO1 = 512, WS_Z = 640, WS_RH = 768, WS_FM = 896;
// second [flow_head.conv1 | mask.0] buffer and two copies of the flow for the three-stream loop with the fused mask + upsampling
// kernel: iteration i uses buffer i & 1, so the mask branch of iteration i - 1 is never overwritten by the main chain of i
constexpr int WS_FM2 = 1408, WS_FLOWM = 1920, WS_PER_PIX = 1924;
constexpr int HDIM = 128, XDIM = 256, CORR_LD = 352, CORR_USED = 324;
constexpr int CDIM = 128;               // inp channels = x[:, 0:CDIM]; x[:, CDIM:XDIM] = [motion 126 | flow 2]
constexpr int CTX_LD = 6 * HDIM;        // [z1 | r1 | q1 | z2 | r2 | q2] context terms per pixel
}   // namespace

extern "C" int64_t raft_update_workspace_floats(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return (int64_t)B * h * w * WS_PER_PIX;
}

// small = true: the SmallUpdateBlock's state (no mask, no GRU context)
static int check_state(const raft_state *st, bool small = false) {
    RAFT_REQUIRE_PTR(st);
    RAFT_REQUIRE_PTR(st->net);
    RAFT_REQUIRE_PTR(st->x);
    RAFT_REQUIRE_PTR(st->corr);
    RAFT_REQUIRE_PTR(st->coords1);
    RAFT_REQUIRE_PTR(st->flow);
    RAFT_REQUIRE_PTR(st->delta);
    RAFT_REQUIRE_PTR(st->ws);
    RAFT_REQUIRE(small || (st->mask != nullptr && st->ctx != nullptr), RAFT_E_NULL);
    return RAFT_OK;
}

extern "C" int raft_prepare_state_f32(const float *cnet, int B, int h, int w, const raft_state *st, void *stream) {
    RAFT_REQUIRE_PTR(cnet);
    int rc = check_state(st);
    if (rc) return rc;
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    const int64_t total = (int64_t)B * h * w * (HDIM + 128);
    prepare_state_kernel<<<raft_ceil_div(total, 256), 256, 0, (hipStream_t)stream>>>(
        cnet, B, h, w, HDIM, 128, st->net, st->x, XDIM, XDIM - 2, st->corr, CORR_LD, CORR_USED, st->coords1, st->flow);
    return raft_launch_status();
}

static ConvArgs conv_args(const raft_conv_weights &wt, const float *a0, int lda0, int c0, const float *a1, int lda1,
                          int c1, int B, int h, int w, int nvalid, float *o0, int ldo0) {
    ConvArgs a = {};
    a.a0 = a0; a.lda0 = lda0; a.c0 = c0; a.a1 = a1; a.lda1 = lda1; a.c1 = c1;
    a.wp = wt.wp; a.bias = wt.bias; a.npad = wt.npad; a.nvalid = nvalid;
    a.B = B; a.H = h; a.W = w; a.scale = 1.0f; a.o0 = o0; a.ldo0 = ldo0;
    return a;
}

// Loop-invariant part of the SepConvGRU.  hx = [h | inp | motion | flow] and [r*h | inp | motion | flow]
// (update.py:53, 58, 63): `inp` never changes inside the prediction loop (model.py:86, 91-106), so the
// inp rows of convz / convr / convq contribute the same pre-activation term in every iteration.  It is
// computed here once per forward -- one 1x5 and one 5x1 convolution 128 -> [z | r | q] (the biases ride
// along) -- and the per-iteration GRU convolutions start their accumulators from it and walk only the
// h / motion / flow rows (K = 5 * 256 instead of 5 * 384).
extern "C" int raft_gru_context_f32(const raft_basic_update_weights *wts, int B, int h, int w,
                                    const raft_state *st, void *stream) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    const int hint = raft_concurrency();
    for (int pass = 0; pass < 2; ++pass) {
        const int kh = pass == 0 ? 1 : 5, kw = pass == 0 ? 5 : 1;
        const raft_conv_weights &wc = pass == 0 ? wts->gru_ctx1 : wts->gru_ctx2;
        ConvArgs a = conv_args(wc, st->x, XDIM, CDIM, nullptr, 0, 0, B, h, w, 3 * HDIM, st->ctx + pass * 3 * HDIM, CTX_LD);
        RAFT_TRY(launch_layer(raft_gru_ctx_plan(*wts, pass, B, h, w, hint), a, kh, kw, EPI_LINEAR, (hipStream_t)stream));
    }
    return RAFT_OK;
}

// Optional per-stage HIP-event recorder (profiling entry point only; see raft_iterate_basic_timed_f32).
struct StageTimer {
    hipEvent_t *ev;
    int n, cap;
    void mark(hipStream_t s) {
        if (n < cap) (void)hipEventRecord(ev[n++], s);
    }
};
#define RAFT_MARK()                 \
    do {                            \
        if (tm) tm->mark(s);        \
    } while (0)

// Where the loop's correlation features come from: the stored pyramid, or fmap1 + the pooled fmap2 pyramid (on demand).
struct LookupSource {
    const float *pyr;
    const int64_t *level_offsets;
    const float *fmap1, *fmap2_pyr;
    int C;
};
// Optional three-stream schedule of one loop iteration (raft_iterate_basic_overlap_f32):
//   main  lookup, convc1, convc2, [join flow branch] conv, GRU, [join previous upsample] fh1_mask0, fh2
//   s1    convf1, convf2                 (needs only the previous iteration's flow)
//   s2    mask2, upsample                (feed nothing inside the loop; must drain before the next fh1_mask0
//                                         overwrites their inputs)
// so the small / short / one-workgroup-per-CU kernels run in the shadows of the big ones.
struct Overlap {
    hipStream_t s1, s2;
    hipEvent_t e_fh, e_f, e_fm, e_up;   // after fh2, after convf2, after fh1_mask0, after upsample
    bool have_up;                       // e_up has been recorded (false in the first iteration)
    // Rotating buffers (all-predictions loop with the fused mask + upsampling kernel).  Every event operation on the MAIN
    // stream costs the dependent chain 6 - 11 us of idle time (the next kernel is not dispatched under the previous one's
    // tail: profiles/r07v_loop_gaps_b4.txt), and two of the four per iteration only protected buffers: the wait for the
    // previous mask branch before fh1_mask0 / fh2 overwrite what it reads, and the record that let mask.2 start before fh2.
    // With rot set, iteration i writes [fh1 | mask.0] and the mask branch's copy of the flow into buffer i & 1 and records
    // e_rot[i & 1] after its mask + upsampling kernel; the FLOW branch of iteration i + 2 waits for that event on its own
    // stream, and the main chain already waits for the flow branch before `conv` -- so the buffer is free before fh1_mask0
    // of i + 2 rewrites it, with no event operation added to the main stream (two per iteration are left: the flow-branch
    // join and the record after fh2).
    bool rot;
    int iter;
    hipEvent_t e_rot[2];
    // Background mask branch (rot only): every iteration but the last launches the mask + upsampling kernel with at most this
    // many workgroups (0 = one per tile).  The chain's kernels have 7 * 2^k workgroups at 448 x 512 and leave 32 CUs idle; 32
    // long-lived mask workgroups settle there (their 95 KB of LDS keep chain workgroups off those CUs) instead of competing
    // with the chain for all of them.  The last iteration's launch is a full one: nothing is left to hide behind.
    int mask_bg_wgs;
};
#define RAFT_HIP(expr)                       \
    do {                                     \
        hipError_t e__ = (expr);             \
        if (e__ != hipSuccess) return (int)e__; \
    } while (0)

// with_mask = false (final-only prediction, every iteration but the last): the mask branch -- mask.0 (the second half of
// fh1_mask0) and mask.2 -- is skipped; flow_head.conv1 alone runs from wts->fh1_w / fh1_w44 (plan.fh1).
// fused_src != NULL: st->corr is NOT read; cor1 comes from the volume through the fused kernel
static int update_basic_impl(const raft_basic_update_weights *wts, const BasicLoopPlan &plan, int B, int h, int w, const raft_state *st,
                             void *stream, StageTimer *tm, Overlap *ov = nullptr, bool with_mask = true,
                             const LookupSource *fused_src = nullptr, float *flow_up_fused = nullptr) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    hipStream_t s = (hipStream_t)stream;
    hipStream_t sf = ov ? ov->s1 : s;   // flow branch
    hipStream_t sm = ov ? ov->s2 : s;   // mask branch
    const int64_t M = (int64_t)B * h * w;
    float *ws = st->ws;
    float *cor1 = ws + M * WS_COR1, *corflo = ws + M * WS_CORFLO, *flo1 = ws + M * WS_FLO1;
    const bool rot = ov && ov->rot && with_mask && flow_up_fused != nullptr;
    float *zb = ws + M * WS_Z, *rh = ws + M * WS_RH, *fm = ws + M * ((rot && (ov->iter & 1)) ? WS_FM2 : WS_FM);
    float *flowm = rot ? ws + M * WS_FLOWM + (ov->iter & 1) * 2 * M : nullptr;

    // ---- BasicMotionEncoder (update.py:97-106)
    if (fused_src) {   // cor = relu(convc1(retrieve(coords1)))   lookup + 1x1, 324 -> 256, one kernel
        RAFT_TRY(raft_lookup_convc1_f32(fused_src->pyr, fused_src->level_offsets, st->coords1, B, h, w, wts->convc1_f.wp,
                                        wts->convc1_f.bias, wts->convc1_f.npad, 256, cor1, 256, stream));
        RAFT_MARK();
    } else {   // cor = relu(convc1(corr))            1x1, 324(+28 zero pad) -> 256
        ConvArgs a = conv_args(wts->convc1, st->corr, CORR_LD, CORR_LD, nullptr, 0, 0, B, h, w, 256, cor1, 256);
        RAFT_TRY(launch_layer(plan.convc1, a, 1, 1, EPI_RELU, s));
        RAFT_MARK();
    }
    {   // cor = relu(convc2(cor))             3x3, 256 -> 192   -> corflo[:, 0:192]
        ConvArgs a = conv_args(wts->convc2, cor1, 256, 256, nullptr, 0, 0, B, h, w, 192, corflo, 256);
        RAFT_TRY(launch_layer(plan.convc2, a, 3, 3, EPI_RELU, s));
        RAFT_MARK();
    }
    if (ov) RAFT_HIP(hipStreamWaitEvent(sf, ov->e_fh, 0));   // flow of the previous iteration is final
    if (rot && ov->iter >= 2) RAFT_HIP(hipStreamWaitEvent(sf, ov->e_rot[ov->iter & 1], 0));   // mask branch of iteration - 2: its buffers are free
    {   // flo = relu(convf1(flow))            7x7, 2 -> 128
        conv7x7_c2_kernel<128><<<B * ((h + 3) / 4) * ((w + 15) / 16), 256, 0, sf>>>(st->flow, wts->convf1.wp, wts->convf1.bias, B, h, w, flo1, 128);
        RAFT_TRY(raft_launch_status());
        RAFT_MARK();
    }
    {   // flo = relu(convf2(flo))             3x3, 128 -> 64    -> corflo[:, 192:256]
        ConvArgs a = conv_args(wts->convf2, flo1, 128, 128, nullptr, 0, 0, B, h, w, 64, corflo + 192, 256);
        RAFT_TRY(launch_layer(plan.convf2, a, 3, 3, EPI_RELU, sf));
        RAFT_MARK();
    }
    if (ov) {
        RAFT_HIP(hipEventRecord(ov->e_f, sf));
        RAFT_HIP(hipStreamWaitEvent(s, ov->e_f, 0));
    }
    {   // out = relu(conv(cat[cor, flo]))     3x3, 256 -> 126   -> x[:, 128:254]; x[:, 254:256] = flow (kept by flowhead2)
        ConvArgs a = conv_args(wts->conv, corflo, 256, 256, nullptr, 0, 0, B, h, w, 126, st->x + 128, XDIM);
        RAFT_TRY(launch_layer(plan.conv, a, 3, 3, EPI_RELU, s));
        RAFT_MARK();
    }
    // ---- SepConvGRU (update.py:51-67): hx = [h | x]; [r*h | x]
    for (int pass = 0; pass < 2; ++pass) {
        const int kh = pass == 0 ? 1 : 5, kw = pass == 0 ? 5 : 1;
        const float *xm = st->x + CDIM;                      // [motion | flow]; the inp rows live in st->ctx
        const float *ctx = st->ctx + pass * 3 * HDIM;        // [z | r | q] context of this pass
        {
            ConvArgs a = conv_args(*plan.gru[2 * pass].wt, st->net, HDIM, HDIM, xm, XDIM, XDIM - CDIM, B, h, w, 2 * HDIM, zb, HDIM);
            a.hid = HDIM; a.o1 = rh; a.ldo1 = HDIM; a.e0 = st->net; a.lde0 = HDIM;
            a.init = ctx; a.ldi = CTX_LD;
            RAFT_TRY(launch_layer(plan.gru[2 * pass], a, kh, kw, EPI_GRU_ZR, s));
            RAFT_MARK();
        }
        {
            ConvArgs a = conv_args(*plan.gru[2 * pass + 1].wt, rh, HDIM, HDIM, xm, XDIM, XDIM - CDIM, B, h, w, HDIM, st->net, HDIM);
            a.e0 = st->net; a.lde0 = HDIM; a.e1 = zb; a.lde1 = HDIM;
            a.init = ctx + 2 * HDIM; a.ldi = CTX_LD;
            RAFT_TRY(launch_layer(plan.gru[2 * pass + 1], a, kh, kw, EPI_GRU_Q, s));
            RAFT_MARK();
        }
    }
    if (ov && ov->have_up && !rot) RAFT_HIP(hipStreamWaitEvent(s, ov->e_up, 0));   // mask2 / upsample of the previous iteration
    if (with_mask) {   // relu(flow_head.conv1(net)) | relu(mask.0(net))   3x3, 128 -> 256 + 256
        ConvArgs a = conv_args(wts->fh1_mask0, st->net, HDIM, HDIM, nullptr, 0, 0, B, h, w, 512, fm, 512);
        RAFT_TRY(launch_layer(plan.fh1_mask0, a, 3, 3, EPI_RELU, s));
        RAFT_MARK();
    } else {           // relu(flow_head.conv1(net)) only            3x3, 128 -> 256        -> fm[:, 0:256]
        ConvArgs a = conv_args(wts->fh1_w, st->net, HDIM, HDIM, nullptr, 0, 0, B, h, w, 256, fm, 512);
        RAFT_TRY(launch_layer(plan.fh1, a, 3, 3, EPI_RELU, s));
    }
    if (ov && with_mask && flow_up_fused == nullptr) {   // two-kernel mask branch: mask.2 may start before fh2
        RAFT_HIP(hipEventRecord(ov->e_fm, s));
        RAFT_HIP(hipStreamWaitEvent(sm, ov->e_fm, 0));
    }
    {   // delta = flow_head.conv2(.), coords1 += delta, flow = coords1 - coords0
        flowhead2_kernel<256><<<raft_ceil_div((int64_t)B * ((h + 1) / 2) * ((w + 3) / 4), 4), 256, 0, s>>>(fm, 512, wts->fh2.wp, wts->fh2.bias, B, h, w,
                                                                   st->delta, st->coords1, st->flow, st->x + 254, XDIM, flowm);
        RAFT_TRY(raft_launch_status());
        RAFT_MARK();
    }
    if (ov) RAFT_HIP(hipEventRecord(ov->e_fh, s));
    if (with_mask && flow_up_fused != nullptr) {
        // mask.2 and the convex upsampling as ONE kernel (mask_upsample.hip): the mask is never written.  Besides fm (the mask
        // branch already waits for fh1_mask0) it needs the flow fh2 has just written.
        if (ov) RAFT_HIP(hipStreamWaitEvent(sm, ov->e_fh, 0));
        RAFT_TRY(raft_launch_mask_upsample(fm + 256, 512, wts->mask2.wp, wts->mask2.bias, wts->mask2.npad, rot ? flowm : st->flow, B, h, w,
                                           0.25f, flow_up_fused, sm, rot ? ov->mask_bg_wgs : 0));
        RAFT_MARK();
    } else if (with_mask) {   // mask = 0.25 * mask.2(.)             1x1, 256 -> 576
        ConvArgs a = conv_args(wts->mask2, fm + 256, 512, 256, nullptr, 0, 0, B, h, w, 576, st->mask, 576);
        a.scale = 0.25f;
        RAFT_TRY(launch_layer(plan.mask2, a, 1, 1, EPI_LINEAR, sm));
        RAFT_MARK();
    }
    return RAFT_OK;
}

extern "C" int raft_update_basic_f32(const raft_basic_update_weights *wts, int B, int h, int w,
                                     const raft_state *st, void *stream) {
    RAFT_REQUIRE_PTR(wts);
    return update_basic_impl(wts, raft_basic_loop_plan(*wts, B, h, w, false, raft_concurrency()), B, h, w, st, stream, nullptr);
}

extern "C" int raft_iterate_basic_f32(const raft_basic_update_weights *wts, const float *pyr,
                                      const int64_t *level_offsets, int B, int h, int w, int iters,
                                      const raft_state *st, float *flow_up, void *stream) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    RAFT_REQUIRE_PTR(flow_up);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0 && iters > 0, RAFT_E_SHAPE);
    const int64_t up = (int64_t)B * 64 * h * w * 2;
    const LookupSource src = {pyr, level_offsets, nullptr, nullptr, 0};
    const BasicLoopPlan plan = raft_basic_loop_plan(*wts, B, h, w, true, raft_concurrency());
    const bool fused = plan.lookup_fused, mf = plan.mask_fused;
    for (int i = 0; i < iters; ++i) {
        if (!fused) RAFT_TRY(raft_corr_lookup_f32(pyr, level_offsets, st->coords1, B, h, w, 4, 4, st->corr, CORR_LD, stream));
        RAFT_TRY(update_basic_impl(wts, plan, B, h, w, st, stream, nullptr, nullptr, true, fused ? &src : nullptr, mf ? flow_up + i * up : nullptr));
        if (!mf) RAFT_TRY(raft_upsample_convex_f32(st->flow, st->mask, B, h, w, flow_up + i * up, stream));
    }
    return RAFT_OK;
}

static int loop_lookup(const LookupSource &src, const raft_state *st, int B, int h, int w, void *stream) {
    if (src.pyr) return raft_corr_lookup_f32(src.pyr, src.level_offsets, st->coords1, B, h, w, 4, 4, st->corr, CORR_LD, stream);
    return raft_corr_lookup_ondemand_f32(src.fmap1, src.fmap2_pyr, st->coords1, B, h, w, src.C, 4, 4, st->corr, CORR_LD, stream);
}

// Caller-owned loop context (include/raft_hip.h): the four cross-stream events of the three-stream schedule, created
// ONCE by raft_loop_ctx_create (the only allocating entry point).
struct raft_loop_ctx {
    hipEvent_t ev[4];
    int device;
};

static int iterate_basic_overlap_impl(const raft_basic_update_weights *wts, const LookupSource &src, int B, int h, int w,
                                      int iters, const raft_state *st, float *flow_up, void *stream, void *aux0, void *aux1,
                                      raft_loop_ctx *ctx, int hint, bool final_only = false);

extern "C" int raft_loop_ctx_create(raft_loop_ctx **out) {
    RAFT_REQUIRE_PTR(out);
    raft_loop_ctx *c = (raft_loop_ctx *)calloc(1, sizeof(raft_loop_ctx));
    if (!c) return (int)hipErrorOutOfMemory;
    int rc = (int)hipGetDevice(&c->device);
    int made = 0;
    // Default HIP events (system-scope release / acquire when they complete).  The events only order streams of ONE device and
    // kernel boundaries release / acquire at agent scope anyway, so RAFT_EVENT_FENCE=0 creates them with
    // hipEventDisableSystemFence: +0.4 .. 0.9 % on the three-stream loop (329.8 against 326.3 - 327.0 pairs/s at 4 pairs, A/B/A in
    // one process, profiles/r10c_event_fence.txt), validated by the bitwise three-stream tests only -- since round 6 an opt-in:
    // the throughput schedule (several single-stream loops in flight) has no event inside the loop, so the default costs it nothing.
    // Read once, when the context is created.
    const unsigned flags = hipEventDisableTiming | (raft_opt(RAFT_OPT_EVENT_FENCE, 1) ? 0u : (unsigned)hipEventDisableSystemFence);
    for (; made < 4 && rc == RAFT_OK; ++made) rc = (int)hipEventCreateWithFlags(&c->ev[made], flags);
    if (rc != RAFT_OK) {
        for (int k = 0; k < made - 1; ++k) (void)hipEventDestroy(c->ev[k]);
        free(c);
        return rc;
    }
    *out = c;
    return RAFT_OK;
}

extern "C" int raft_loop_ctx_destroy(raft_loop_ctx *c) {
    if (!c) return RAFT_OK;
    for (int k = 0; k < 4; ++k) (void)hipEventDestroy(c->ev[k]);
    free(c);
    return RAFT_OK;
}

// raft_iterate_basic_f32 on three streams (see struct Overlap).  aux0 / aux1 are caller-owned streams
// distinct from `stream`; all work is joined back into `stream` before returning.
extern "C" int raft_iterate_basic_overlap_f32(const raft_basic_update_weights *wts, const float *pyr,
                                              const int64_t *level_offsets, int B, int h, int w, int iters,
                                              const raft_state *st, float *flow_up, void *stream, void *aux0,
                                              void *aux1, raft_loop_ctx *ctx) {
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    const LookupSource src = {pyr, level_offsets, nullptr, nullptr, 0};
    return iterate_basic_overlap_impl(wts, src, B, h, w, iters, st, flow_up, stream, aux0, aux1, ctx, raft_concurrency());
}

// The same three-stream loop with the volume-free ("alternate") correlation: every iteration's lookup computes its
// footprint correlations from fmap1 and the pooled fmap2 pyramid (raft_fmap_pyramid_f32).  BASELINE config 4.
extern "C" int raft_iterate_basic_ondemand_f32(const raft_basic_update_weights *wts, const float *fmap1,
                                               const float *fmap2_pyr, int C, int B, int h, int w, int iters,
                                               const raft_state *st, float *flow_up, void *stream, void *aux0,
                                               void *aux1, raft_loop_ctx *ctx) {
    RAFT_REQUIRE_PTR(fmap1);
    RAFT_REQUIRE_PTR(fmap2_pyr);
    const LookupSource src = {nullptr, nullptr, fmap1, fmap2_pyr, C};
    return iterate_basic_overlap_impl(wts, src, B, h, w, iters, st, flow_up, stream, aux0, aux1, ctx, raft_concurrency());
}

// The prediction loop for callers that only want flow_predictions[-1] (reference model.py:160-166, predict_step): the
// mask head and the convex upsampling run in the LAST iteration only; flow_up_last: (B, 8h, 8w, 2).  The recurrence
// (lookup, motion encoder, GRU, flow head) is launch for launch the one of raft_iterate_basic_overlap_f32, so the
// result equals its last prediction.  Needs the Winograd copy of flow_head.conv1 (wts->fh1_w).
extern "C" int raft_iterate_basic_final_f32(const raft_basic_update_weights *wts, const float *pyr,
                                            const int64_t *level_offsets, int B, int h, int w, int iters,
                                            const raft_state *st, float *flow_up_last, void *stream, void *aux0,
                                            void *aux1, raft_loop_ctx *ctx) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    RAFT_REQUIRE(wts->fh1_w.wp != nullptr, RAFT_E_NULL);
    const LookupSource src = {pyr, level_offsets, nullptr, nullptr, 0};
    return iterate_basic_overlap_impl(wts, src, B, h, w, iters, st, flow_up_last, stream, aux0, aux1, ctx, raft_concurrency(), true);
}

// Enqueue the whole loop on `stream` + the two side streams.
static int enqueue_loop(const raft_basic_update_weights *wts, const BasicLoopPlan &plan, const LookupSource &src, int B, int h,
                        int w, int iters, const raft_state *st, float *flow_up, void *stream, void *aux0, void *aux1,
                        raft_loop_ctx *ctx, bool final_only) {
    const bool fused = plan.lookup_fused;
    hipStream_t s = (hipStream_t)stream;
    if (aux0 == stream) {
        // single-stream schedule (aux0 == aux1 == stream): the launches of raft_iterate_basic_f32, for every lookup source and
        // for the final-only loop -- what several concurrent loops (one per lane of the pipelined forward) run
        const int64_t up1 = (int64_t)B * 64 * h * w * 2;
        for (int i = 0; i < iters; ++i) {
            const bool with_mask = !final_only || i == iters - 1;
            if (!fused) RAFT_TRY(loop_lookup(src, st, B, h, w, stream));
            float *up_i = flow_up + (final_only ? 0 : i * up1);
            const bool mf = with_mask && plan.mask_fused;
            RAFT_TRY(update_basic_impl(wts, plan, B, h, w, st, stream, nullptr, nullptr, with_mask, fused ? &src : nullptr, mf ? up_i : nullptr));
            if (with_mask && !mf) RAFT_TRY(raft_upsample_convex_f32(st->flow, st->mask, B, h, w, up_i, stream));
        }
        return RAFT_OK;
    }
    Overlap ov = {};
    ov.s1 = (hipStream_t)aux0;
    ov.s2 = (hipStream_t)aux1;
    ov.e_fh = ctx->ev[0];
    ov.e_f = ctx->ev[1];
    ov.e_fm = ctx->ev[2];
    ov.e_up = ctx->ev[3];
    ov.e_rot[0] = ctx->ev[2];   // e_fm is not used in that mode
    ov.e_rot[1] = ctx->ev[3];
    ov.rot = !final_only && plan.mask_fused;
    const int64_t up = (int64_t)B * 64 * h * w * 2;
    int rc = (int)hipEventRecord(ov.e_fh, s);   // state prepared on `stream`: the flow branch may start
    for (int i = 0; i < iters && rc == RAFT_OK; ++i) {
        const bool with_mask = !final_only || i == iters - 1;
        rc = fused ? RAFT_OK : loop_lookup(src, st, B, h, w, stream);
        float *up_i = flow_up + (final_only ? 0 : i * up);
        const bool mf = with_mask && plan.mask_fused;
        ov.iter = i;
        // default 32, except where the chain's launches cover the chip exactly (the flow / mask head's F(4x4) grid a multiple of
        // 256: a single 1024 x 1024 pair loses 6 % to a background branch); one process, profiles/r09d_mask_bg_shapes.txt:
        // 448 x 512 at 4 / 5 / 6 / 8 / 12 / 16 pairs +2.7 / +7.9 / +4.5 / +6.1 / +2.5 / +1.6 %, 16 or 40+ workgroups lose
        const int head_grid = B * ((h + 7) / 8) * ((w + 63) / 64) * 8;
        ov.mask_bg_wgs = (ov.rot && i + 1 < iters) ? (head_grid % 256 ? 32 : 0) : 0;
        if (rc == RAFT_OK) rc = update_basic_impl(wts, plan, B, h, w, st, stream, nullptr, &ov, with_mask, fused ? &src : nullptr, mf ? up_i : nullptr);
        if (!with_mask) continue;
        if (!mf) {
            // upsample on the mask branch: needs mask2 (same stream) and the flow written by fh2
            if (rc == RAFT_OK) rc = (int)hipStreamWaitEvent(ov.s2, ov.e_fh, 0);
            if (rc == RAFT_OK) rc = raft_upsample_convex_f32(st->flow, st->mask, B, h, w, up_i, ov.s2);
        }
        if (ov.rot) ov.e_up = ov.e_rot[i & 1];
        if (rc == RAFT_OK) rc = (int)hipEventRecord(ov.e_up, ov.s2);
        ov.have_up = true;
    }
    if (rc == RAFT_OK && ov.have_up) rc = (int)hipStreamWaitEvent(s, ov.e_up, 0);   // join
    return rc;
}

static int iterate_basic_overlap_impl(const raft_basic_update_weights *wts, const LookupSource &src, int B, int h, int w,
                                      int iters, const raft_state *st, float *flow_up, void *stream, void *aux0, void *aux1,
                                      raft_loop_ctx *ctx, int hint, bool final_only) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_REQUIRE_PTR(flow_up);
    RAFT_REQUIRE_PTR(aux0);
    RAFT_REQUIRE_PTR(aux1);
    RAFT_REQUIRE_PTR(ctx);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0 && iters > 0, RAFT_E_SHAPE);
    // three distinct streams, or all three the same one (the single-stream schedule)
    RAFT_REQUIRE((aux0 != stream && aux1 != stream && aux0 != aux1) || (aux0 == stream && aux1 == stream), RAFT_E_UNSUPPORTED);
    const BasicLoopPlan plan = raft_basic_loop_plan(*wts, B, h, w, src.pyr != nullptr, hint);
    const int rc = enqueue_loop(wts, plan, src, B, h, w, iters, st, flow_up, stream, aux0, aux1, ctx, final_only);
    if (rc != RAFT_OK) {   // never leave side streams running behind an error return
        (void)hipStreamSynchronize((hipStream_t)aux0);
        (void)hipStreamSynchronize((hipStream_t)aux1);
    }
    return rc;
}

// Profiling twin of raft_iterate_basic_f32: identical launches, plus a HIP event after every kernel
// on `stream`; synchronises and accumulates per-stage milliseconds into stage_ms[RAFT_BASIC_STAGES]
// (host array).  Used by bench.py for the live roofline numbers -- never on the product path.
extern "C" int raft_iterate_basic_timed_f32(const raft_basic_update_weights *wts, const float *pyr,
                                            const int64_t *level_offsets, int B, int h, int w, int iters,
                                            const raft_state *st, float *flow_up, void *stream,
                                            float *stage_ms) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    RAFT_REQUIRE_PTR(flow_up);
    RAFT_REQUIRE_PTR(stage_ms);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0 && iters > 0 && iters <= 64, RAFT_E_SHAPE);
    hipStream_t s = (hipStream_t)stream;
    const int per_iter = RAFT_BASIC_STAGES;
    const int nev = iters * per_iter + 1;
    hipEvent_t *ev = (hipEvent_t *)malloc(sizeof(hipEvent_t) * nev);
    if (!ev) return (int)hipErrorOutOfMemory;
    for (int i = 0; i < nev; ++i) (void)hipEventCreate(&ev[i]);
    StageTimer tm = {ev, 0, nev};
    const int64_t up = (int64_t)B * 64 * h * w * 2;
    int rc = RAFT_OK;
    const LookupSource src = {pyr, level_offsets, nullptr, nullptr, 0};
    const BasicLoopPlan plan = raft_basic_loop_plan(*wts, B, h, w, true, raft_concurrency());
    const bool fused = plan.lookup_fused, mf = plan.mask_fused;
    tm.mark(s);
    for (int i = 0; i < iters && rc == RAFT_OK; ++i) {
        // RAFT_LOOKUP_FUSED as in the product loops: fused, the lookup stage is empty and the convc1 stage is the fused kernel
        if (!fused) rc = raft_corr_lookup_f32(pyr, level_offsets, st->coords1, B, h, w, 4, 4, st->corr, CORR_LD, stream);
        tm.mark(s);
        // RAFT_MASK_FUSED likewise: fused, the mask2 stage is the fused kernel and the upsampling stage is empty
        if (rc == RAFT_OK) rc = update_basic_impl(wts, plan, B, h, w, st, stream, &tm, nullptr, true, fused ? &src : nullptr, mf ? flow_up + i * up : nullptr);
        if (rc == RAFT_OK && !mf) rc = raft_upsample_convex_f32(st->flow, st->mask, B, h, w, flow_up + i * up, stream);
        tm.mark(s);
    }
    if (rc == RAFT_OK) rc = (int)hipStreamSynchronize(s);
    if (rc == RAFT_OK && tm.n == nev) {
        for (int k = 0; k < per_iter; ++k) stage_ms[k] = 0.f;
        for (int i = 0; i < iters; ++i)
            for (int k = 0; k < per_iter; ++k) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, ev[i * per_iter + k], ev[i * per_iter + k + 1]);
                stage_ms[k] += ms;
            }
    }
    for (int i = 0; i < nev; ++i) (void)hipEventDestroy(ev[i]);
    free(ev);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// SmallUpdateBlock  (reference update.py:70-85, 17-35, 109-125; model.py:190-226)
//   net (M,96); x (M,160) = [inp 64 | motion 80 | flow 2 | 14 zero pad]; corr (M,224) = 196 + 28 pad
// workspace (floats per pixel): corflo 128 [cor 96 | flo2 32] | flo1 64 | z 96 | rh 96 | fh 128
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int SW_CORFLO = 0, SW_FLO1 = 128, SW_Z = 192, SW_RH = 288, SW_FH = 384, SW_PER_PIX = 512;
constexpr int S_HDIM = 96, S_CDIM = 64, S_XLD = 160, S_FLOW_SLOT = 144, S_CORR_LD = 224, S_CORR_USED = 196;
}   // namespace

extern "C" int64_t raft_small_update_workspace_floats(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return (int64_t)B * h * w * SW_PER_PIX;
}

extern "C" int raft_prepare_state_small_f32(const float *cnet, int B, int h, int w, const raft_state *st,
                                            void *stream) {
    RAFT_REQUIRE_PTR(cnet);
    RAFT_TRY(check_state(st, true));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    const int64_t total = (int64_t)B * h * w * (S_HDIM + S_CDIM);
    prepare_state_kernel<<<raft_ceil_div(total, 256), 256, 0, (hipStream_t)stream>>>(
        cnet, B, h, w, S_HDIM, S_CDIM, st->net, st->x, S_XLD, S_FLOW_SLOT, st->corr, S_CORR_LD, S_CORR_USED,
        st->coords1, st->flow);
    return raft_launch_status();
}

static int update_small_impl(const raft_small_update_weights *wts, const SmallLoopPlan &plan, int B, int h, int w,
                             const raft_state *st, void *stream) {
    RAFT_TRY(check_state(st, true));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = (int64_t)B * h * w;
    float *ws = st->ws;
    float *corflo = ws + M * SW_CORFLO, *flo1 = ws + M * SW_FLO1, *zb = ws + M * SW_Z, *rh = ws + M * SW_RH;
    float *fh = ws + M * SW_FH;
    {   // cor = relu(convc1(corr))      1x1, 196(+28) -> 96     -> corflo[:, 0:96]
        ConvArgs a = conv_args(wts->convc1, st->corr, S_CORR_LD, S_CORR_LD, nullptr, 0, 0, B, h, w, 96, corflo, 128);
        RAFT_TRY(launch_layer(plan.convc1, a, 1, 1, EPI_RELU, s));
    }
    {   // flo = relu(convf1(flow))      7x7, 2 -> 64
        conv7x7_c2_kernel<64><<<B * ((h + 3) / 4) * ((w + 15) / 16), 256, 0, s>>>(st->flow, wts->convf1.wp, wts->convf1.bias, B, h, w, flo1, 64);
        RAFT_TRY(raft_launch_status());
    }
    {   // flo = relu(convf2(flo))       3x3, 64 -> 32           -> corflo[:, 96:128]
        ConvArgs a = conv_args(wts->convf2, flo1, 64, 64, nullptr, 0, 0, B, h, w, 32, corflo + 96, 128);
        RAFT_TRY(launch_layer(plan.convf2, a, 3, 3, EPI_RELU, s));
    }
    {   // out = relu(conv(cat[cor, flo])) 3x3, 128 -> 80        -> x[:, 64:144]
        ConvArgs a = conv_args(wts->conv, corflo, 128, 128, nullptr, 0, 0, B, h, w, 80, st->x + 64, S_XLD);
        RAFT_TRY(launch_layer(plan.conv, a, 3, 3, EPI_RELU, s));
    }
    {   // ConvGRU (update.py:26-35), 3x3: z | r
        ConvArgs a = conv_args(wts->gru_zr, st->net, S_HDIM, S_HDIM, st->x, S_XLD, S_XLD, B, h, w, 2 * S_HDIM, zb,
                               S_HDIM);
        a.hid = S_HDIM; a.o1 = rh; a.ldo1 = S_HDIM; a.e0 = st->net; a.lde0 = S_HDIM;
        RAFT_TRY(launch_layer(plan.gru_zr, a, 3, 3, EPI_GRU_ZR, s));
    }
    {
        ConvArgs a = conv_args(wts->gru_q, rh, S_HDIM, S_HDIM, st->x, S_XLD, S_XLD, B, h, w, S_HDIM, st->net, S_HDIM);
        a.e0 = st->net; a.lde0 = S_HDIM; a.e1 = zb; a.lde1 = S_HDIM;
        RAFT_TRY(launch_layer(plan.gru_q, a, 3, 3, EPI_GRU_Q, s));
    }
    {   // relu(flow_head.conv1(net))    3x3, 96 -> 128
        ConvArgs a = conv_args(wts->fh1, st->net, S_HDIM, S_HDIM, nullptr, 0, 0, B, h, w, 128, fh, 128);
        RAFT_TRY(launch_layer(plan.fh1, a, 3, 3, EPI_RELU, s));
    }
    {   // delta = flow_head.conv2(.), coords1 += delta, flow = coords1 - coords0
        flowhead2_kernel<128><<<raft_ceil_div((int64_t)B * ((h + 1) / 2) * ((w + 3) / 4), 4), 256, 0, s>>>(fh, 128, wts->fh2.wp, wts->fh2.bias, B, h, w,
                                                                   st->delta, st->coords1, st->flow,
                                                                   st->x + S_FLOW_SLOT, S_XLD);
        RAFT_TRY(raft_launch_status());
    }
    return RAFT_OK;
}

extern "C" int raft_update_small_f32(const raft_small_update_weights *wts, int B, int h, int w,
                                     const raft_state *st, void *stream) {
    RAFT_REQUIRE_PTR(wts);
    return update_small_impl(wts, raft_small_loop_plan(*wts, B, h, w, raft_concurrency()), B, h, w, st, stream);
}

extern "C" int raft_iterate_small_f32(const raft_small_update_weights *wts, const float *pyr,
                                      const int64_t *level_offsets, int B, int h, int w, int iters,
                                      const raft_state *st, float *flow_up, void *stream) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    RAFT_REQUIRE_PTR(flow_up);
    RAFT_TRY(check_state(st, true));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0 && iters > 0, RAFT_E_SHAPE);
    const int64_t up = (int64_t)B * 64 * h * w * 2;
    const SmallLoopPlan plan = raft_small_loop_plan(*wts, B, h, w, raft_concurrency());
    for (int i = 0; i < iters; ++i) {
        RAFT_TRY(raft_corr_lookup_f32(pyr, level_offsets, st->coords1, B, h, w, 4, 3, st->corr, S_CORR_LD, stream));
        RAFT_TRY(update_small_impl(wts, plan, B, h, w, st, stream));
        RAFT_TRY(raft_upflow8_f32(st->flow, B, h, w, flow_up + i * up, stream));
    }
    return RAFT_OK;
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

// Shared definitions of the fp32-MFMA convolution kernels for gfx950 (conv_halo.h, conv_wino.h, conv_wino1d.h, conv_wino4.h):
// the argument block, the epilogue codes, gate activations, buffer-load helper, and -- in conv_epilogue.h and conv_stage.h,
// included below -- the ONE epilogue all four families share (descriptors, channel bookkeeping, value formulas, STATS tail) and
// their ONE prologue (source / weight descriptors, halo staging, weight-fragment fetch; the workgroup remap is in launch_plan.h).
//
// GEMM view of every kernel: M = B*H*W output pixels, N = output channels, K = taps x input channels; NHWC activations, weights
// packed by tf_raft_amd/packing.py into fragment-shaped k-quads (include/raft_hip.h).  Two rules shape all of them:
//   * A-tile loads are UNCONDITIONAL buffer loads: out-of-image taps get an out-of-range offset and the buffer bounds check
//     returns 0 (a per-chunk `ok ? load : 0` makes hipcc branch around every load with an s_waitcnt in between, which
//     serialises the loads and exposes their latency);
//   * the same for the epilogues: the GRU gates read h / z with unconditional (clamped) loads issued as one batch per
//     accumulator tile before any arithmetic.
#pragma once
#include <type_traits>

#include "common.h"

enum ConvEpilogue {
    EPI_LINEAR = 0,   // out = (acc + bias) * scale
    EPI_RELU = 1,     // out = relu(acc + bias) * scale
    EPI_GRU_ZR = 2,   // n <  hid: o0 = sigmoid(v)            (z)
                      // n >= hid: o1 = sigmoid(v) * e0[n-hid] (r * h)
    EPI_GRU_Q = 3,    // o0 = (1 - e1) * e0 + e1 * tanh(v)     (h <- (1-z) h + z q), e0 = h, e1 = z
    EPI_RES = 4       // o0 = relu(e0 + relu(acc + bias))     (ResBlock tail, reference extractor.py:41-49)
};

struct ConvArgs {
    const float *a0, *a1;   // input sources (NHWC); channels [0,c0) of a0 then [0,c1) of a1
    int lda0, lda1, c0, c1;
    const float *wp, *bias;
    int B, H, W;
    int npad, nvalid, hid;
    float scale;
    float *o0, *o1;
    int ldo0, ldo1;
    const float *e0, *e1;
    int lde0, lde1;
    // ---- halo-tiled kernel only (conv_halo.h); zero-initialised = plain stride-1 'same' convolution
    int Hi, Wi;                            // input height / width (0: same as the output H, W)
    int pt, pl;                            // zero padding before the first row / column (TF 'SAME')
    const float *pre_scale, *pre_shift;    // PRE: input is relu(x * scale[b][c] + shift[b][c]) (fused instance norm)
    float *stats;                          // STATS: per-tile (sum, sum of squares) of the raw output, [tile][npad][2]
    const float *init;                     // accumulators start from init[pixel * ldi + n] instead of 0 (NULL: 0):
    int ldi;                               //   a precomputed partial convolution (loop-invariant GRU context term)
};

// GRU gate functions on the transcendental unit: exp2 and rcp are each within 1 ulp, the composites within a few
// 1e-7 absolute of libm's -- three orders below the 1e-4 `net` tolerance of the parity tests (the reference's own
// gates are whatever Eigen / cuDNN approximations TensorFlow dispatches to).  libm expf + an IEEE divide cost ~32
// VALU instructions per element, 28 elements per lane per gate kernel.
__device__ __forceinline__ float raft_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ float raft_tanh(float x) {
    // 1 - 2 / (exp(2x) + 1): exp2 overflows to +inf -> 1, underflows to 0 -> -1
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(2.88539008177792681f * x) + 1.0f);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 raft_buffer_load_f4(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0));
}

constexpr unsigned RAFT_OOB = 0x80000000u;   // >= any buffer extent we accept (< 2 GiB): load returns 0

#include "conv_epilogue.h"
#include "conv_stage.h"

// (The first version of the direct kernel -- a (tap, chunk)-stepped LDS pipeline with 32x32 / 16x16 MFMA tiles, tile codes 0..5 of
// RAFT_CONV_TILE -- was kept for A/B through round 3 and removed in round 4: the halo-tiled kernel of conv_halo.h replaced it
// everywhere in round 1; its measurements stay in profiles/r01*.)

// ---- launchers: validate, then dispatch a plan (launch_plan.h); RAFT_E_UNSUPPORTED for a shape or plan not instantiated
int raft_launch_conv(const ConvArgs &a, int kh, int kw, int epi, hipStream_t s, HaloPlan p);            // conv.hip
int raft_launch_conv_wino(const ConvArgs &a, int epi, hipStream_t s, WinoPlan p);                      // conv_wino.hip
int raft_launch_conv_wino1d(const ConvArgs &a, int kh, int kw, int epi, hipStream_t s, Wino1dPlan p);   // conv_wino1d.hip
int raft_launch_conv_wino4(const ConvArgs &a, int epi, hipStream_t s, Wino4Plan p);                    // conv_wino4.hip
// the two special convolutions of the update blocks (conv.hip): 7x7 on the flow, relu, cout = 128 or 64; flow_head.conv2 from
// cin = 256 or 128 channels with the coordinate update (flow2 / flow3: optional copies of the flow, NULL = none).  Hidden: the
// library exports what it did while their only callers were part of conv.hip
__attribute__((visibility("hidden"))) int raft_launch_conv7x7_c2(const float *flow, const float *kernel, const float *bias, int cout,
                                                                 int B, int H, int W, float *out, int ldo, hipStream_t s);
__attribute__((visibility("hidden"))) int raft_launch_flowhead2(const float *x, int ldx, int cin, const float *wk, const float *bias,
                                                                int B, int H, int W, float *delta, float *coords1, float *flow,
                                                                float *flow2, int ldf2, float *flow3, hipStream_t s);

// Operand checks of every launcher: 16-byte aligned sources and weights (RAFT_E_ALIGN); each operand spans < 2 GiB (32-bit buffer
// offsets, RAFT_E_UNSUPPORTED).  wtaps: weight taps (kernel or Winograd transform); opt: optional operands checked where present.
enum { RAFT_CHECK_O1 = 1, RAFT_CHECK_E0 = 2, RAFT_CHECK_E1 = 4, RAFT_CHECK_INIT = 8, RAFT_CHECK_ALL = 15 };
static inline int raft_check_operands(const ConvArgs &a, int64_t wtaps, int opt) {
    if (a.lda0 % 4 || (a.c1 && a.lda1 % 4)) return RAFT_E_ALIGN;
    if (!raft_aligned16(a.a0) || !raft_aligned16(a.wp) || (a.c1 && !raft_aligned16(a.a1))) return RAFT_E_ALIGN;
    const int64_t M = (int64_t)a.B * a.H * a.W, lim = (int64_t)1 << 31;
    if (((M - 1) * a.lda0 + a.c0) * 4 >= lim || (a.c1 && ((M - 1) * a.lda1 + a.c1) * 4 >= lim)) return RAFT_E_UNSUPPORTED;
    if (M * a.ldo0 * 4 >= lim || wtaps * (a.c0 + a.c1) * a.npad * 4 >= lim) return RAFT_E_UNSUPPORTED;
    if (((opt & RAFT_CHECK_O1) && a.o1 && M * a.ldo1 * 4 >= lim) || ((opt & RAFT_CHECK_E0) && a.e0 && M * a.lde0 * 4 >= lim) ||
        ((opt & RAFT_CHECK_E1) && a.e1 && M * a.lde1 * 4 >= lim) || ((opt & RAFT_CHECK_INIT) && a.init && M * a.ldi * 4 >= lim))
        return RAFT_E_UNSUPPORTED;
    return RAFT_OK;
}

// Epilogue dispatch: launch(std::integral_constant<int, EPI>()) if epi is one of EPIS (a family's instantiated epilogues), else RAFT_E_UNSUPPORTED.
template <int... EPIS, class Launch>
static int raft_dispatch_epi(int epi, Launch &&launch) {
    int rc = RAFT_E_UNSUPPORTED;
    (void)((epi == EPIS && ((rc = launch(std::integral_constant<int, EPIS>())), true)) || ...);
    return rc;
}

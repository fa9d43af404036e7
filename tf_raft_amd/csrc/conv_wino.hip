// Winograd F(2x2, 3x3) convolution launcher (kernel: conv_wino.h; plan: launch_plan.h raft_wino_plan).
#include "conv_wino.h"

template <int TNW, int SB, int CK>
static int launch_wino(const ConvArgs &a, int epi, int grid, hipStream_t s) {
    if (a.pre_scale || a.stats) {   // instance-norm encoder: linear epilogue + output moments, optionally the normalised input
        if (epi != EPI_LINEAR || a.stats == nullptr) return RAFT_E_UNSUPPORTED;
        if (a.pre_scale)
            conv_wino_kernel<TNW, EPI_LINEAR, 1, 1, 0, 1><<<grid, 256, 0, s>>>(a);
        else
            conv_wino_kernel<TNW, EPI_LINEAR, 0, 1, SB, CK><<<grid, 256, 0, s>>>(a);
        return raft_launch_status();
    }
    return raft_dispatch_epi<EPI_LINEAR, EPI_RELU, EPI_RES, EPI_GRU_ZR, EPI_GRU_Q>(epi, [&](auto e) {
        conv_wino_kernel<TNW, decltype(e)::value, 0, 0, SB, CK><<<grid, 256, 0, s>>>(a);
        return raft_launch_status();
    });
}

// split-K inside the workgroup (conv_wino.h, KS = 2): 512 threads, plain epilogues only; CK = 32 or 64 channels per stage
template <int CK>
static int launch_wino_ks2(const ConvArgs &a, int epi, int grid, hipStream_t s) {
    return raft_dispatch_epi<EPI_LINEAR, EPI_RELU, EPI_RES, EPI_GRU_ZR, EPI_GRU_Q>(epi, [&](auto e) {
        conv_wino_kernel<1, decltype(e)::value, 0, 0, 1, CK, 2><<<grid, 512, 0, s>>>(a);
        return raft_launch_status();
    });
}

int raft_launch_conv_wino(const ConvArgs &a, int epi, hipStream_t s, WinoPlan p) {
    if (a.c0 <= 0 || a.c0 % 16 || a.c1 < 0 || a.c1 % 16 || a.npad <= 0 || a.npad % 32) return RAFT_E_UNSUPPORTED;
    RAFT_TRY(raft_check_operands(a, 16, epi == EPI_RES ? RAFT_CHECK_E0 : 0));
    if (a.init || (a.Hi && (a.Hi != a.H || a.Wi != a.W))) return RAFT_E_UNSUPPORTED;
    if ((epi == EPI_GRU_ZR || epi == EPI_GRU_Q) && (a.e0 == nullptr || (epi == EPI_GRU_Q && a.e1 == nullptr))) return RAFT_E_NULL;
    if (epi == EPI_RES && a.e0 == nullptr) return RAFT_E_UNSUPPORTED;
    // a plan made for another shape (the final-only flow head reuses fh1_mask0's) must still fit this one
    if (a.npad % (32 * p.tnw) || (p.ck > 1 && (a.c0 % (16 * p.ck) || a.c1 % (16 * p.ck))) ||
        (p.ks == 2 && (a.pre_scale || a.stats)))
        return RAFT_E_UNSUPPORTED;
    const int grid = a.B * ((a.H + 3) / 4) * ((a.W + 31) / 32) * (a.npad / (32 * p.tnw));
    if (p.ks == 2) return p.ck == 4 ? launch_wino_ks2<4>(a, epi, grid, s) : launch_wino_ks2<2>(a, epi, grid, s);
    if (p.tnw == 2) return p.sb ? launch_wino<2, 1, 1>(a, epi, grid, s) : launch_wino<2, 0, 1>(a, epi, grid, s);
    if (p.ck == 2) return p.sb ? launch_wino<1, 1, 2>(a, epi, grid, s) : launch_wino<1, 0, 2>(a, epi, grid, s);
    return p.sb ? launch_wino<1, 1, 1>(a, epi, grid, s) : launch_wino<1, 0, 1>(a, epi, grid, s);
}

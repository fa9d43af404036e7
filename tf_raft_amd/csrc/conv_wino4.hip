// Winograd F(4x4, 3x3) convolution launcher (kernel: conv_wino4.h; plan: launch_plan.h raft_wino4_plan).
#include "conv_wino4.h"

template <int KS>
static int launch_wino4(const ConvArgs &a, int epi, int grid, hipStream_t s) {
    return raft_dispatch_epi<EPI_LINEAR, EPI_RELU, EPI_RES>(epi, [&](auto e) {
        conv_wino4_kernel<decltype(e)::value, KS><<<grid, 256, 0, s>>>(a);
        return raft_launch_status();
    });
}

int raft_launch_conv_wino4(const ConvArgs &a, int epi, hipStream_t s, Wino4Plan p) {
    if (a.c0 <= 0 || a.c0 % 16 || a.c1 < 0 || a.c1 % 16 || a.npad <= 0 || a.npad % 64) return RAFT_E_UNSUPPORTED;
    RAFT_TRY(raft_check_operands(a, 36, epi == EPI_RES ? RAFT_CHECK_E0 : 0));
    if (a.init || (a.Hi && (a.Hi != a.H || a.Wi != a.W))) return RAFT_E_UNSUPPORTED;
    if ((a.pre_scale || a.stats) && (epi != EPI_LINEAR || a.stats == nullptr || a.c1 != 0)) return RAFT_E_UNSUPPORTED;
    if (a.pre_scale && a.pre_shift == nullptr) return RAFT_E_NULL;
    if (epi == EPI_RES && a.e0 == nullptr) return RAFT_E_NULL;
    if (p.ks == 2 && (a.c0 % 32 || a.c1 % 32 || a.stats)) return RAFT_E_UNSUPPORTED;   // the plan must fit the shape
    const int nt = a.npad / 64;
    if (a.stats) {   // instance-norm encoder: moments of the raw output, optionally the producer's normalisation + relu on the input
        const int grid1 = a.B * ((a.H + 7) / 8) * ((a.W + 63) / 64) * nt;
        if (a.pre_scale)
            conv_wino4_kernel<EPI_LINEAR, 1, 1, 1><<<grid1, 256, 0, s>>>(a);
        else
            conv_wino4_kernel<EPI_LINEAR, 1, 0, 1><<<grid1, 256, 0, s>>>(a);
        return raft_launch_status();
    }
    if (p.ks == 2) return launch_wino4<2>(a, epi, a.B * ((a.H + 3) / 4) * ((a.W + 63) / 64) * nt, s);
    return launch_wino4<1>(a, epi, a.B * ((a.H + 7) / 8) * ((a.W + 63) / 64) * nt, s);
}

// 1-D Winograd F(2, 5) / F(4, 5) convolution launcher (kernel: conv_wino1d.h; plan: launch_plan.h raft_wino1d_plan).
#include "conv_wino1d.h"

template <int AXIS, int TNW, int CK, int TM, int MO = 2>
static int launch_wino1d(const ConvArgs &a, int epi, int grid, hipStream_t s) {
    return raft_dispatch_epi<EPI_LINEAR, EPI_RELU, EPI_GRU_ZR, EPI_GRU_Q>(epi, [&](auto e) {
        conv_wino1d_kernel<AXIS, TNW, decltype(e)::value, CK, TM, MO><<<grid, 256, 0, s>>>(a);
        return raft_launch_status();
    });
}

template <int AXIS>
static int launch_wino1d_axis(const ConvArgs &a, int epi, int grid, Wino1dPlan p, hipStream_t s) {
    if (p.mo == 4) return p.tnw == 2 ? launch_wino1d<AXIS, 2, 2, 1, 4>(a, epi, grid, s) : launch_wino1d<AXIS, 1, 2, 1, 4>(a, epi, grid, s);
    if (p.tm == 2) {
        if (p.ck == 2) return p.tnw == 2 ? launch_wino1d<AXIS, 2, 2, 2>(a, epi, grid, s) : launch_wino1d<AXIS, 1, 2, 2>(a, epi, grid, s);
        return p.tnw == 2 ? launch_wino1d<AXIS, 2, 1, 2>(a, epi, grid, s) : launch_wino1d<AXIS, 1, 1, 2>(a, epi, grid, s);
    }
    if (p.ck == 2) return p.tnw == 2 ? launch_wino1d<AXIS, 2, 2, 1>(a, epi, grid, s) : launch_wino1d<AXIS, 1, 2, 1>(a, epi, grid, s);
    return p.tnw == 2 ? launch_wino1d<AXIS, 2, 1, 1>(a, epi, grid, s) : launch_wino1d<AXIS, 1, 1, 1>(a, epi, grid, s);
}

int raft_launch_conv_wino1d(const ConvArgs &a, int kh, int kw, int epi, hipStream_t s, Wino1dPlan p) {
    if (p.mo != 2 && p.mo != 4) return RAFT_E_UNSUPPORTED;
    if (p.mo == 4 && (a.c0 % 32 || a.c1 % 32)) return RAFT_E_UNSUPPORTED;
    if (!((kh == 1 && kw == 5) || (kh == 5 && kw == 1))) return RAFT_E_UNSUPPORTED;
    if (a.c0 <= 0 || a.c0 % 16 || a.c1 < 0 || a.c1 % 16 || a.npad <= 0 || a.npad % 32) return RAFT_E_UNSUPPORTED;
    RAFT_TRY(raft_check_operands(a, p.mo + 4, RAFT_CHECK_ALL));
    if (a.pre_scale || a.stats || (a.Hi && (a.Hi != a.H || a.Wi != a.W))) return RAFT_E_UNSUPPORTED;
    if (a.npad % (32 * p.tnw) || (p.ck == 2 && (a.c0 % 32 || a.c1 % 32))) return RAFT_E_UNSUPPORTED;   // the plan must fit the shape
    const int grid = raft_wino1d_tiles(a.B, a.H, a.W, kh, p.mo, p.tm) * (a.npad / (32 * p.tnw));
    return kh == 5 ? launch_wino1d_axis<1>(a, epi, grid, p, s) : launch_wino1d_axis<0>(a, epi, grid, p, s);
}

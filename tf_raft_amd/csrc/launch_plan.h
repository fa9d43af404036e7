// Launch plans: which kernel family and workgroup shape every convolution runs (internal; pure host C++ without HIP headers:
// tests/native/abi_host_check.cpp checks the plan table on the CPU).  The rules read the tuning switches and take the launch-shape
// hint as an ARGUMENT -- only the extern "C" entry points read the thread-local hint (raft_concurrency), once per call -- so every
// rule is safe to call from any thread.  The launchers (conv_mfma.h) validate their arguments and dispatch a plan.
#pragma once

#include <stdint.h>

#include "../../include/raft_hip.h"

// Tuning switches (include/raft_hip.h: raft_set_option).  Process-global, initialised ONCE from the environment when the
// library is loaded and changed only through raft_set_option afterwards: the launch path reads an atomic int, it never
// calls getenv.  raft_opt(id, dflt) = the switch's value, or dflt while it is unset.
enum RaftOptionId {
    RAFT_OPT_CONV_WINO, RAFT_OPT_SMALL_WINO, RAFT_OPT_GRU_WINO, RAFT_OPT_GRU_WINO4, RAFT_OPT_WINO_TNW, RAFT_OPT_WINO_SB,
    RAFT_OPT_WINO_CK, RAFT_OPT_WINO1D_TM,
    RAFT_OPT_LOOKUP_FUSED, RAFT_OPT_ONDEMAND_BLOCK, RAFT_OPT_ENC_WINO,
    RAFT_OPT_WINO_KS, RAFT_OPT_CONV_WINO4, RAFT_OPT_WINO4_KS, RAFT_OPT_MASK_FUSED, RAFT_OPT_ENC_WINO4, RAFT_OPT_CONVC2_KS, RAFT_OPT_CONVF2_KS,
    RAFT_OPT_EVENT_FENCE, RAFT_OPT_CORR_XCD, RAFT_OPT_CORR_POOL,
    RAFT_OPT_COUNT
};
int raft_opt(int id, int dflt);
bool raft_opt_is_set(int id);
// RAFT_CONV_TILE ("<code>" or "<npad>:<taps>:<code>,..."): the tile code forced for a convolution, or -1
int raft_opt_conv_tile(int npad, int taps, bool (*valid)(int code, int npad));

#ifdef __HIP__
#define RAFT_HOST_DEVICE __host__ __device__
#else
#define RAFT_HOST_DEVICE
#endif
// XCD-aware workgroup remap of the MFMA convolution kernels and the fused mask + upsampling kernel: the hardware places workgroup
// bid on XCD bid & 7; the logical tile it works on is chosen so that the tiles of one XCD are contiguous (the N tiles of one pixel
// tile are neighbours and share the halo tile in that XCD's L2).  A permutation of 0 .. nwg-1 for every grid size
// (tests/native/abi_host_check.cpp checks both properties).
RAFT_HOST_DEVICE static inline int raft_xcd_remap(int bid, int nwg) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// direct halo-tiled kernel (conv_halo.h), F(2x2, 3x3) (conv_wino.h), F(2, 5) / F(4, 5) by Wino1dPlan::mo (conv_wino1d.h), F(4x4, 3x3)
enum RaftConvFamily { RAFT_FAM_HALO, RAFT_FAM_WINO, RAFT_FAM_WINO1D, RAFT_FAM_WINO4 };
struct HaloPlan { int th, tn; };                // TH x 16-pixel x 64*TN-channel workgroups
struct WinoPlan { int tnw, sb, ck, ks; };       // 32*TNW channels, pinned weight prefetch, 16*CK channels per stage, K split
struct Wino1dPlan { int mo, tnw, tm, ck; };     // outputs per tile, 32*TNW channels, tile height, 16*CK channels per stage
struct Wino4Plan { int ks; };                   // 1: 8-row workgroups; 2: 4-row workgroups with K split between two wave sets
// one layer: the family, that family's plan (the other plans are unused) and, in the loop plans, the weight copy it runs
struct ConvChoice { int family; HaloPlan halo; WinoPlan wino; Wino1dPlan wino1d; Wino4Plan wino4; const raft_conv_weights *wt; };
typedef const raft_conv_weights *RaftWeights;
static inline ConvChoice raft_choice(HaloPlan p, RaftWeights wt = nullptr) { ConvChoice c = {RAFT_FAM_HALO}; c.halo = p; c.wt = wt; return c; }
static inline ConvChoice raft_choice(WinoPlan p, RaftWeights wt = nullptr) { ConvChoice c = {RAFT_FAM_WINO}; c.wino = p; c.wt = wt; return c; }
static inline ConvChoice raft_choice(Wino1dPlan p, RaftWeights wt = nullptr) { ConvChoice c = {RAFT_FAM_WINO1D}; c.wino1d = p; c.wt = wt; return c; }
static inline ConvChoice raft_choice(Wino4Plan p, RaftWeights wt = nullptr) { ConvChoice c = {RAFT_FAM_WINO4}; c.wino4 = p; c.wt = wt; return c; }

// ------------------------------------------------------------------------------------------------
// direct (halo-tiled) kernel
// ------------------------------------------------------------------------------------------------
// Tuning / test override: RAFT_CONV_TILE is either one code (applies to every convolution whose npad
// it divides) or a comma-separated list of `npad:taps:code` entries, e.g. "256:5:171,128:5:141".
// code = 100 + 10*TH + TN: TH x 16-pixel x 64*TN-channel workgroups of the halo-tiled kernel.
static inline bool raft_halo_code_valid(int code, int npad) {
    const int th = (code - 100) / 10, tn = (code - 100) % 10;
    return code >= 100 && (th == 4 || th == 7 || th == 8) && (tn == 1 || tn == 2) && npad % (64 * tn) == 0;
}

// Pick the halo tile (TH x 16 pixels, 64*TN channels) by a small cost model of MI355X (256 CUs):
//   time ~ (workgroups per CU, rounded up) x (MFMA work of one tile) x (latency-hiding penalty),
// where the penalty reflects how many workgroups (= waves per SIMD) are co-resident on a CU: one wave
// per SIMD exposes prologue / barrier / epilogue latency, three or more hide it (docs/NOTEBOOK.md section 4.1).
static inline HaloPlan raft_halo_plan(int B, int H, int W, int npad, int kh, int kw, int hint) {
    int code = raft_opt_conv_tile(npad, kh * kw, raft_halo_code_valid);
    if (code < 100) {
        static const int ths[3] = {4, 7, 8};
        double best = 1e30;
        code = 141;
        for (int ti = 0; ti < 3; ++ti)
            for (int tn = 1; tn <= 2; ++tn) {
                const int th = ths[ti];
                if (npad % (64 * tn)) continue;
                const int64_t blocks = (int64_t)B * ((H + th - 1) / th) * ((W + 15) / 16) * (npad / (64 * tn)) * hint;
                const int64_t per_cu = (blocks + 255) / 256;
                const int lds = 2 * ((th + kh - 1) * (16 + kw - 1) * 40 + 8) * 4;
                int resident = 160 * 1024 / lds;
                const int reg_limit = (tn == 2 && th >= 7) ? 1 : (th >= 7 ? 2 : 3);   // VGPR + AGPR budget per SIMD
                if (resident > reg_limit) resident = reg_limit;
                const int64_t conc = per_cu < resident ? per_cu : resident;
                const double pen = conc >= 3 ? 1.0 : (conc == 2 ? 1.05 : 1.15);
                const double eff = (th == 4 && kh * kw > 1) ? 0.88 : 1.0;   // short tiles: more halo traffic per MFMA (measured; a 1x1 kernel has no halo)
                const double cost = (double)per_cu * th * 16 * 64 * tn * pen / eff;
                if (cost < best) {
                    best = cost;
                    code = 100 + th * 10 + tn;
                }
            }
    }
    return {(code - 100) / 10, (code - 100) % 10};
}

// ------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3); plain = no fused input normalisation and no output moments (the encoder's instance norm)
// ------------------------------------------------------------------------------------------------
static inline WinoPlan raft_wino_plan(int B, int H, int W, int c0, int c1, int npad, bool plain, int hint) {
    // channel blocks of 64 per workgroup when that still leaves >= 2 workgroups per CU, else blocks of 32
    const int tiles = B * ((H + 3) / 4) * ((W + 31) / 32);
    const int forced = raft_opt(RAFT_OPT_WINO_TNW, 0);   // tuning / test override (raft_set_option)
    int tnw = (npad % 64 == 0 && (int64_t)tiles * (npad / 64) * hint >= 512) ? 2 : 1;
    if (forced == 1 || (forced == 2 && npad % 64 == 0)) tnw = forced;
    const int grid = tiles * (npad / (32 * tnw));
    // Not scaled by the hint (unlike TNW and KS), as measured so far:
    // pinned weight prefetch (SB): always at TNW = 2; at TNW = 1 only when two workgroups per CU hold the whole grid
    const int sb = raft_opt(RAFT_OPT_WINO_SB, (tnw == 2 || grid <= 512) ? 1 : 0) != 0;   // tuning override: 0 / 1
    // 32 channels per barrier at TNW = 1 when the channel counts allow it (RAFT_WINO_CK = 1 / 2 overrides)
    const bool ck2_ok = c0 % 32 == 0 && c1 % 32 == 0;
    const bool ck2 = ck2_ok && raft_opt(RAFT_OPT_WINO_CK, grid <= 512 ? 2 : 1) == 2;   // 58 KB of LDS: two workgroups per CU
    // fewer wave-tasks than SIMDs (grid * 4 < 1024): split K between two wave sets of a 512-thread workgroup
    // (RAFT_WINO_KS = 1 / 2 overrides)
    const int ks = raft_opt(RAFT_OPT_WINO_KS, (tnw == 1 && grid * hint <= 224) ? 2 : 1);
    if (ks == 2 && tnw == 1 && ck2_ok && plain) {
        // 64 channels per stage where the channel counts allow: the stages of these launches are latency, not work
        const bool ck4 = c0 % 64 == 0 && c1 % 64 == 0 && raft_opt(RAFT_OPT_WINO_CK, 4) == 4;
        return {1, 1, ck4 ? 4 : 2, 2};
    }
    return {tnw, sb, (tnw == 1 && ck2) ? 2 : 1, 1};
}

// ------------------------------------------------------------------------------------------------
// 1-D Winograd F(2, 5) (mo = 2) / F(4, 5) (mo = 4) along x (kh = 1) or y (kh = 5)
// ------------------------------------------------------------------------------------------------
constexpr bool RAFT_WINO1D_CK2_DEFAULT = true;   // 32 channels per barrier: +2-4 % on the GRU layers (profiles/r03u)

// workgroup tiles of one 32-channel column block: F(4, 5) 2 rows x 64 columns (1x5) or 8 rows x 16 columns (5x1);
// F(2, 5) 2*TM rows x 32 columns (1x5) or 4*TM rows x 16 columns (5x1)
static inline int raft_wino1d_tiles(int B, int H, int W, int kh, int mo, int tm) {
    if (mo == 4) return kh == 5 ? B * ((H + 7) / 8) * ((W + 15) / 16) : B * ((H + 1) / 2) * ((W + 63) / 64);
    return kh == 5 ? B * ((H + 4 * tm - 1) / (4 * tm)) * ((W + 15) / 16) : B * ((H + 2 * tm - 1) / (2 * tm)) * ((W + 31) / 32);
}

static inline Wino1dPlan raft_wino1d_plan(int B, int H, int W, int c0, int c1, int npad, int kh, int mo, int hint) {
    // F(4, 5): 64-channel workgroups while that leaves about two per CU (gru_q at B = 4 stand-alone: 224 workgroups of
    // 64 channels 28.3 us against 31.0 us for 448 of 32 channels, but inside the three-stream loop with the GRU epilogue
    // 34.5 / 38.6 us against 33.5 / 34.3).
    // F(2, 5): 64-channel workgroups (a transformed input feeds two column blocks) wherever the channel count allows; full-height
    // tiles (TM = 2) when they still give about two workgroups per CU, half-height tiles otherwise (gru_q at B = 4:
    // 224 -> 448 workgroups).  64-channel workgroups only where that still leaves enough of them (a single 448 x 512 pair: 112
    // against 448 workgroups for gru_zr -- 7.90 -> 7.48 ms per forward with the 32-channel ones, profiles/r06b_b1_options.txt)
    const int forced = raft_opt(RAFT_OPT_WINO_TNW, 0);   // tuning / test overrides (raft_set_option)
    const int tiles = raft_wino1d_tiles(B, H, W, kh, mo, 2);   // F(2, 5): full-height tiles
    int tnw = (npad % 64 == 0 && (int64_t)tiles * (npad / 64) * hint >= 400) ? 2 : 1;
    if (forced == 1 || (forced == 2 && npad % 64 == 0)) tnw = forced;
    if (mo == 4) return {4, tnw, 1, 2};
    const int tm_forced = raft_opt(RAFT_OPT_WINO1D_TM, 0);
    const bool ck2 = c0 % 32 == 0 && c1 % 32 == 0 && raft_opt(RAFT_OPT_WINO_CK, RAFT_WINO1D_CK2_DEFAULT ? 2 : 1) == 2;
    int tm = (int64_t)tiles * (npad / (32 * tnw)) * hint >= 400 ? 2 : 1;
    if (tm_forced == 1 || tm_forced == 2) tm = tm_forced;
    return {2, tnw, tm, ck2 ? 2 : 1};
}

// ------------------------------------------------------------------------------------------------
// Winograd F(4x4, 3x3)
// ------------------------------------------------------------------------------------------------
// Two row blocks (8 x 64 pixels) x 64 channels per workgroup; when that leaves fewer workgroups than ~3/4 of the chip's CUs
// (fewer than 128: convc2 84, conv 56, fh1 112 at 4 pairs; conv 112 at 8 -- profiles/r07i_wino4_bench.txt), one row block per workgroup with K split between two wave sets instead --
// twice the workgroups, half the K loop each (RAFT_WINO4_KS = 1 / 2 overrides).  The split needs an even number of
// 16-channel chunks in each source.  layer_ks: a layer's own choice (1 / 2) in place of the grid rule, 0 = none.
static inline Wino4Plan raft_wino4_plan(int B, int H, int W, int c0, int c1, int npad, bool plain, int hint, int layer_ks = 0) {
    const int grid1 = B * ((H + 7) / 8) * ((W + 63) / 64) * (npad / 64);
    int ks = raft_opt(RAFT_OPT_WINO4_KS, (layer_ks == 1 || layer_ks == 2) ? layer_ks : (grid1 * hint < 128 ? 2 : 1));
    if (ks != 2 || c0 % 32 || c1 % 32 || !plain) ks = 1;
    return {ks};
}

// ------------------------------------------------------------------------------------------------
// update blocks: one plan per loop call
// ------------------------------------------------------------------------------------------------
// The per-iteration SepConvGRU convolutions: direct halo kernel or 1-D Winograd F(2, 5) / F(4, 5) (conv_wino1d.h).
// RAFT_GRU_WINO and RAFT_GRU_WINO4 are bit masks over {1: gru_zr1, 2: gru_q1, 4: gru_zr2, 8: gru_q2}; a layer runs
// F(4, 5) if its WINO4 bit is set and the 8-tap weights were supplied, else F(2, 5) if its WINO bit is set and the
// 6-tap weights were supplied, else the direct kernel.  Unset = the defaults below.
constexpr int RAFT_GRU_WINO_DEFAULT = 15;
constexpr int RAFT_GRU_WINO4_DEFAULT = 15;
// The 3x3 layers of the update block run either on the direct halo kernel or on the Winograd F(2x2, 3x3) kernel
// (conv_wino.h) when the caller supplied transformed weights.  RAFT_CONV_WINO is a bit mask over
// {1: convc2, 2: convf2, 4: conv, 8: fh1_mask0}; unset = RAFT_WINO_DEFAULT (the layers where it measured faster at
// B = 4, docs/NOTEBOOK.md section 4.4).  Read per call so that tests can switch it.
constexpr int RAFT_WINO_DEFAULT = 13;
constexpr int RAFT_SMALL_WINO_DEFAULT = 15;   // SmallRAFT: {1: conv, 2: gru_zr, 4: gru_q, 8: fh1}, switch RAFT_SMALL_WINO
// F(4x4, 3x3) (conv_wino4.h), switch RAFT_CONV_WINO4 = bit mask {1: convc2, 4: conv, 8: fh1_mask0 / fh1}.  Default (us alone,
// F(4x4) against F(2x2), profiles/r07i_wino4_bench.txt): from 4 pairs on the flow / mask head (63 vs 91 at 4 pairs, 128 vs 169 at
// 8) and convc2 (61 vs 76 with the K-split workgroups, 107 vs 132); conv (N = 128) from 8 pairs on (65 vs 114; at 4 pairs its
// 112 K-split workgroups lose to F(2x2): 59 vs 49).  A single pair nothing: a launch is then one round of workgroups whose
// duration is one workgroup's K loop, and the one-wave-per-SIMD F(4x4) workgroup is the longer one (single pair: 151 pairs/s
// without, 133 with -- same-box A/B with bench.py, profiles/r07p_bench_mask_ab.txt: 4 pairs 270 -> 282, 8 pairs 285 -> 296);
// at two pairs the flow / mask head alone gains (206 -> 221 pairs/s with mask 8 on two boxes; with convc2 as well 214 and one
// outlier of 235: profiles/r08k_round3_options.txt, r08z_b2_options.txt).
// Bit 2 = convf2 (3x3, 128 -> 64), with convc2 from 3 pairs on: alone its 56 K-split workgroups (4 pairs) are slower than the direct kernel's
// 224 (42 against 27 us), but they take a quarter of the CU-time and, with 108 KB of LDS each, settle on CUs of their own: in the
// three-stream loop convc2's 168 K-split workgroups + these 56 + the 32 of the background mask branch are exactly 256 -- the flow
// branch no longer competes with convc2, which can have its faster shape back (one process, profiles/r09i_b4_options3.txt:
// 303.1 pairs/s -> 325.9 at 4 pairs; with convc2 on 8-row workgroups 303.3; 8 pairs 345.0 -> 353.3).
static inline int raft_wino4_default_mask(int64_t m) {   // m = pixels x hint: loops sharing the chip fill it like one loop of n times the batch
    return m < 2 * 3584 ? 0 : (8 | (m >= 3 * 3584 ? 1 | 2 : 0) | (m >= 8 * 3584 ? 4 : 0));   // three pairs: 250 -> 262 pairs/s with 11, two: 237 -> 231
}

struct BasicLoopPlan {
    bool lookup_fused, mask_fused;
    ConvChoice convc1, convc2, convf2, conv, gru[4], fh1_mask0, fh1, mask2;   // gru: zr1, q1, zr2, q2; fh1: final-only flow head
};

// stored_volume: the loop reads a stored correlation volume (not the on-demand lookup)
static inline BasicLoopPlan raft_basic_loop_plan(const raft_basic_update_weights &wt, int B, int h, int w, bool stored_volume, int hint) {
    BasicLoopPlan p = {};
    const int64_t m = (int64_t)B * h * w * hint;   // loops sharing the chip fill it like one loop of n times the batch
    // The loops run the lookup fused into convc1 (raft_lookup_convc1_f32) when they read a stored volume, the repacked
    // kernel was supplied and RAFT_LOOKUP_FUSED is not switched off.
    p.lookup_fused = stored_volume && wt.convc1_f.wp != nullptr && raft_opt(RAFT_OPT_LOOKUP_FUSED, 1) != 0;
    // RAFT_MASK_FUSED: the prediction loops run mask.2 and the convex upsampling as one kernel.  Default: from 2 pairs (2 x 3584
    // feature pixels) on.  Launched one workgroup per tile the fused kernel only pays from 4 pairs (single pair 152.7 pairs/s with two
    // kernels, 137.8 - 142.0 fused; two pairs 210.7 / 205.4; four 282.7 / 288.4: profiles/r08k_round3_options.txt, r07q); as the
    // 32-workgroup background branch of the three-stream loop (update_block.hip, LoopIter::mask_bg_wgs) it pays from 2 pairs: 225.5 -> 244.1 pairs/s at two,
    // 246.3 -> 256.3 at three (profiles/r09e_small_batch_mask.txt); a single pair stays on the two-kernel path (152 - 153 against
    // 148 - 155).
    p.mask_fused = raft_opt(RAFT_OPT_MASK_FUSED, m >= 2 * 3584 ? 1 : 0) != 0 && wt.mask2.wp != nullptr && wt.mask2.npad == 576;
    p.convc1 = raft_choice(raft_halo_plan(B, h, w, wt.convc1.npad, 1, 1, hint), &wt.convc1);
    p.mask2 = raft_choice(raft_halo_plan(B, h, w, wt.mask2.npad, 1, 1, hint), &wt.mask2);

    const int wino = raft_opt(RAFT_OPT_CONV_WINO, RAFT_WINO_DEFAULT), wino4 = raft_opt(RAFT_OPT_CONV_WINO4, raft_wino4_default_mask(m));
    auto conv3x3 = [&](int bit, const raft_conv_weights &direct, const raft_conv_weights &w2, const raft_conv_weights &w44, int c0,
                       int layer_ks) {
        if (w44.wp != nullptr && (wino4 & bit)) return raft_choice(raft_wino4_plan(B, h, w, c0, 0, w44.npad, true, hint, layer_ks), &w44);
        if ((wino & bit) && w2.wp != nullptr) return raft_choice(raft_wino_plan(B, h, w, c0, 0, w2.npad, true, hint), &w2);
        return raft_choice(raft_halo_plan(B, h, w, direct.npad, 3, 3, hint), &direct);
    };
    // F(4x4) workgroup shape of convc2: the grid rule (K-split 4-row workgroups while 8-row ones would be fewer than 128: 168
    // instead of 84 at 4 pairs).  While the flow branch ran the direct convf2 (224 workgroups competing for the same CUs) the
    // 8-row shape was the better one in the loop (288.7 -> 293.7 pairs/s: less CU-time, room for the side branches,
    // profiles/r08n_b4_options.txt); with convf2 on its own 56 CUs (raft_wino4_default_mask) the K-split shape wins by 7 %.
    // RAFT_CONVC2_KS = 1 / 2 forces either; every loop uses the same shape (the loops stay bit-identical to each other).
    p.convc2 = conv3x3(1, wt.convc2, wt.convc2_w, wt.convc2_w44, 256, raft_opt(RAFT_OPT_CONVC2_KS, 0));
    // F(4x4) shape of convf2: K-split workgroups up to 4 pairs (28 eight-row workgroups -> 56), eight-row ones from 56 on (8 pairs:
    // 56 of them beside convc2's 168 and the mask branch's 32: 353.4 -> 356.1 pairs/s, profiles/r09k_b8_options.txt)
    const int f2_grid1 = B * ((h + 7) / 8) * ((w + 63) / 64);
    p.convf2 = conv3x3(2, wt.convf2, wt.convf2_w, wt.convf2_w44, 128, raft_opt(RAFT_OPT_CONVF2_KS, f2_grid1 * hint >= 56 ? 1 : 0));
    p.conv = conv3x3(4, wt.conv, wt.conv_w, wt.conv_w44, 256, 0);
    p.fh1_mask0 = conv3x3(8, wt.fh1_mask0, wt.fh1_mask0_w, wt.fh1_mask0_w44, 128, 0);
    // flow_head.conv1 alone (final-only loop, every iteration but the last) must round exactly like its half of fh1_mask0
    // (RAFT.predict_step returns the bits of flow_predictions[-1]): the plan of fh1_mask0's shape.  Knowingly asymmetric: it runs
    // F(2x2) whenever its RAFT_CONV_WINO4 bit is clear, whatever RAFT_CONV_WINO says.
    const int n4 = wt.fh1_mask0_w44.npad > 0 ? wt.fh1_mask0_w44.npad : wt.fh1_w44.npad;
    const int n2 = (wt.fh1_mask0_w.npad > 0 && wt.fh1_mask0_w.npad % 32 == 0) ? wt.fh1_mask0_w.npad : wt.fh1_w.npad;
    p.fh1 = wt.fh1_w44.wp != nullptr && (wino4 & 8) ? raft_choice(raft_wino4_plan(B, h, w, 128, 0, n4, true, hint), &wt.fh1_w44)
                                                    : raft_choice(raft_wino_plan(B, h, w, 128, 0, n2, true, hint), &wt.fh1_w);

    const int gmask = raft_opt(RAFT_OPT_GRU_WINO, RAFT_GRU_WINO_DEFAULT);
    // F(4, 5) wins where the launch fills the chip; below ~2 x 3584 pixels (the reference's single 448 x 512 pair) every
    // kernel is one under-filled round of workgroups and the F(2, 5) kernel's smaller workgroups finish sooner
    // (B = 1: 8.69 -> 8.40 ms per forward, profiles/r05d_b1_probe.txt)
    const int gmask4 = raft_opt(RAFT_OPT_GRU_WINO4, m < 2 * 3584 ? 0 : RAFT_GRU_WINO4_DEFAULT);
    const raft_conv_weights *gw[4][3] = {{&wt.gru_zr1, &wt.gru_zr1_w, &wt.gru_zr1_w4}, {&wt.gru_q1, &wt.gru_q1_w, &wt.gru_q1_w4},
                                         {&wt.gru_zr2, &wt.gru_zr2_w, &wt.gru_zr2_w4}, {&wt.gru_q2, &wt.gru_q2_w, &wt.gru_q2_w4}};
    for (int l = 0; l < 4; ++l) {   // hx = [h 128 | motion + flow 128]
        const int bit = 1 << l, kh = l < 2 ? 1 : 5, kw = 6 - kh;
        if ((gmask4 & bit) && gw[l][2]->wp != nullptr)   // workgroup width by grid size (a forced 32- / 64-channel width for gru_q lost to it: profiles/r09q_gru_q_tnw.txt)
            p.gru[l] = raft_choice(raft_wino1d_plan(B, h, w, 128, 128, gw[l][2]->npad, kh, 4, hint), gw[l][2]);
        else if ((gmask & bit) && gw[l][1]->wp != nullptr)
            p.gru[l] = raft_choice(raft_wino1d_plan(B, h, w, 128, 128, gw[l][1]->npad, kh, 2, hint), gw[l][1]);
        else
            p.gru[l] = raft_choice(raft_halo_plan(B, h, w, gw[l][0]->npad, kh, kw, hint), gw[l][0]);
    }
    return p;
}

// raft_gru_context_f32, pass 0 (1x5) / 1 (5x1): F(4, 5) like the per-iteration GRU convolutions (same switch: bit 1 / 4 of
// RAFT_GRU_WINO4 = the pass).  Knowingly asymmetric: no pixel threshold on the default here.
static inline ConvChoice raft_gru_ctx_plan(const raft_basic_update_weights &wt, int pass, int B, int h, int w, int hint) {
    const raft_conv_weights &w4 = pass == 0 ? wt.gru_ctx1_w4 : wt.gru_ctx2_w4;
    const int kh = pass == 0 ? 1 : 5;
    if (w4.wp != nullptr && (raft_opt(RAFT_OPT_GRU_WINO4, RAFT_GRU_WINO4_DEFAULT) & (pass == 0 ? 1 : 4)))
        return raft_choice(raft_wino1d_plan(B, h, w, 128, 0, w4.npad, kh, 4, hint), &w4);
    const raft_conv_weights &wc = pass == 0 ? wt.gru_ctx1 : wt.gru_ctx2;
    return raft_choice(raft_halo_plan(B, h, w, wc.npad, kh, 6 - kh, hint), &wc);
}

struct SmallLoopPlan { ConvChoice convc1, convf2, conv, gru_zr, gru_q, fh1; };

static inline SmallLoopPlan raft_small_loop_plan(const raft_small_update_weights &wt, int B, int h, int w, int hint) {
    SmallLoopPlan p = {};
    const int mask = raft_opt(RAFT_OPT_SMALL_WINO, RAFT_SMALL_WINO_DEFAULT);
    auto conv3x3 = [&](int bit, const raft_conv_weights &direct, const raft_conv_weights &w2, int c0, int c1) {
        return (mask & bit) && w2.wp != nullptr ? raft_choice(raft_wino_plan(B, h, w, c0, c1, w2.npad, true, hint), &w2)
                                                : raft_choice(raft_halo_plan(B, h, w, direct.npad, 3, 3, hint), &direct);
    };
    p.convc1 = raft_choice(raft_halo_plan(B, h, w, wt.convc1.npad, 1, 1, hint), &wt.convc1);
    p.convf2 = raft_choice(raft_halo_plan(B, h, w, wt.convf2.npad, 3, 3, hint), &wt.convf2);
    p.conv = conv3x3(1, wt.conv, wt.conv_w, 128, 0);          // [cor 96 | flo 32]
    p.gru_zr = conv3x3(2, wt.gru_zr, wt.gru_zr_w, 96, 160);   // [h 96 | x 160]
    p.gru_q = conv3x3(4, wt.gru_q, wt.gru_q_w, 96, 160);
    p.fh1 = conv3x3(8, wt.fh1, wt.fh1_w, 96, 0);
    return p;
}

// ------------------------------------------------------------------------------------------------
// encoders
// ------------------------------------------------------------------------------------------------
// Stages whose stride-1 3x3 layers run the F(4x4, 3x3) kernel (stage 0 = layer1 ...; n images, Ho x Wo x F outputs).  Default:
// every layer whose launch is MORE than one round of the kernel's 8 x 64-pixel x 64-channel workgroups on the chip (> 256) -- at
// 4 pairs fnet's layer1 / layer2 (896 / 448) and cnet's layer1 (448).  Per kernel at 4 pairs (profiles/r07u_encoder_kernels_b4.txt):
// fnet's ten layers 1308 -> 1120 us, the 64-channel half-resolution layers ~190 -> ~150 us each (K = 64 is only four 16-channel
// chunks: prologue and output transform are 40 % of a workgroup); a layer3 launch with the K-split variant is slower than F(2x2)
// (41 against 28 us).  Launches of a single round gain nothing measurable (one / two pairs: 137.2 / 203.8 pairs/s without,
// 137.2 / 204.5 with every stage on it, profiles/r08k_round3_options.txt) and F(4x4) is the noisier algorithm (3.3e-6 against
// 1.9e-6 of the output scale), so they stay on F(2x2).  Loops sharing the chip: the launch counts hint times (378.7 against
// 375.6 pairs/s with every stage on F(4x4) under three lanes, profiles/r12l_*).  RAFT_ENC_WINO = 0: direct 3x3 kernels everywhere
// (A/B timing, parity tests).  Knowingly asymmetric: an explicit RAFT_ENC_WINO4 is taken as given (no grid test).
static inline bool raft_enc_wino() { return raft_opt(RAFT_OPT_ENC_WINO, 1) != 0; }
static inline bool raft_enc_stage_wino4(int stage, int n, int Ho, int Wo, int F, int hint) {
    const int mask = raft_enc_wino() ? raft_opt(RAFT_OPT_ENC_WINO4, 7) : 0;
    return ((mask >> stage) & 1) &&
           (raft_opt_is_set(RAFT_OPT_ENC_WINO4) || (int64_t)n * ((Ho + 7) / 8) * ((Wo + 63) / 64) * ((F + 63) / 64) * hint > 256);
}

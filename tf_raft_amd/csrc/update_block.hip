// State preparation, the GRU context, the BasicUpdateBlock / SmallUpdateBlock sequencing and the prediction loops
// (reference tf_raft/layers/update.py:5-153, tf_raft/model.py:84-109, 190-226) for gfx950: host code over the convolution
// launchers of conv_mfma.h, one small kernel of its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_mfma.h"

// mask.2 + RAFT.upsample_flow in one kernel (mask_upsample.hip)
int raft_launch_mask_upsample(const float *a, int lda, const float *wp, const float *bias, int npad, const float *flow, int B,
                              int h, int w, float scale, float *out, hipStream_t s, int max_wgs = 0);

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

// ------------------------------------------------------------------------------------------------
// The prediction loop of the BasicUpdateBlock: one description of a call (LoopCall), one driver (run_loop)
// ------------------------------------------------------------------------------------------------
// Optional per-stage HIP-event recorder (profiling entry point only; see raft_iterate_basic_timed_f32).
struct StageTimer {
    hipEvent_t *ev;
    int n, cap;
    void mark(hipStream_t s) {
        if (n < cap) (void)hipEventRecord(ev[n++], s);
    }
};

// Where the loop's correlation features come from: the stored pyramid, or fmap1 + the pooled fmap2 pyramid (on demand).
// Neither: no lookup, st->corr is the caller's (raft_update_basic_f32).
struct LookupSource {
    const float *pyr;
    const int64_t *level_offsets;
    const float *fmap1, *fmap2_pyr;
    int C;
};

// Caller-owned loop context (include/raft_hip.h): the four cross-stream events of the three-stream schedule, created
// ONCE by raft_loop_ctx_create (the only allocating entry point).
struct raft_loop_ctx {
    hipEvent_t ev[4];
    int device;
};
// after fh2, after convf2, after fh1_mask0, after upsample; with rotating buffers (LoopIter::rot) e_fm is not used and the last
// two are the events of buffer 0 and buffer 1
enum { EV_FH = 0, EV_F = 1, EV_FM = 2, EV_UP = 3, EV_ROT = 2 };

// The streams of a loop.  All three the same one is the single-stream schedule -- what several concurrent loops (one per lane
// of the pipelined forward) run.  Three distinct ones are the three-stream schedule of one loop iteration:
//   main  lookup, convc1, convc2, [join flow branch] conv, GRU, [join previous upsample] fh1_mask0, fh2
//   flow  convf1, convf2                 (needs only the previous iteration's flow)
//   mask  mask2, upsample                (feed nothing inside the loop; must drain before the next fh1_mask0
//                                         overwrites their inputs)
// so the small / short / one-workgroup-per-CU kernels run in the shadows of the big ones.
struct LoopStreams {
    hipStream_t main, flow, mask;
    bool split() const { return flow != main; }
};

// One loop call, fixed before its first launch.
struct LoopCall {
    const raft_basic_update_weights *wts;
    BasicLoopPlan plan;
    LookupSource src;
    int B, h, w, iters;
    const raft_state *st;
    float *flow_up;          // iters predictions (final_only: one); NULL: the mask goes to st->mask, nothing is upsampled
    bool final_only;         // the mask head and the upsampling run in the last iteration only
    LoopStreams s;
    raft_loop_ctx *ctx;      // the events of split streams (not read on one stream, may be NULL there)
    StageTimer *tm;          // optional: a mark after every stage of RAFT_BASIC_STAGES
};

// What iteration i of a call does differently from the others.
struct LoopIter {
    // with_mask = false (final-only prediction, every iteration but the last): the mask branch -- mask.0 (the second half of
    // fh1_mask0) and mask.2 -- is skipped; flow_head.conv1 alone runs from wts->fh1_w / fh1_w44 (plan.fh1).
    bool with_mask;
    bool mask_fused;         // the mask branch is the fused mask.2 + upsampling kernel (mask_upsample.hip), not two kernels
    float *up;               // this iteration's prediction (NULL with the call's flow_up)
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
    float *fm, *flowm;       // [flow_head.conv1 | mask.0] of this iteration; rot: the mask branch's copy of the flow (else NULL)
    int ev_done;             // recorded behind this iteration's mask branch: e_rot[i & 1] with rot, else e_up
    bool wait_buffer;        // rot: the flow branch waits for ev_done of iteration i - 2 (this iteration's buffer)
    bool wait_prev_mask;     // no rot: the main chain waits for the previous iteration's mask branch before it rewrites fm
    // Background mask branch (rot only): every iteration but the last launches the mask + upsampling kernel with at most this
    // many workgroups (0 = one per tile).  The chain's kernels have 7 * 2^k workgroups at 448 x 512 and leave 32 CUs idle; 32
    // long-lived mask workgroups settle there (their 95 KB of LDS keep chain workgroups off those CUs) instead of competing
    // with the chain for all of them.  The last iteration's launch is a full one: nothing is left to hide behind.
    int mask_bg_wgs;
};

static LoopIter loop_iter(const LoopCall &c, int i) {
    const int64_t M = (int64_t)c.B * c.h * c.w;
    LoopIter it = {};
    it.with_mask = !c.final_only || i == c.iters - 1;
    if (c.flow_up && it.with_mask) it.up = c.flow_up + (c.final_only ? 0 : i * (M * 64 * 2));
    it.mask_fused = it.up != nullptr && c.plan.mask_fused;
    it.rot = c.s.split() && !c.final_only && it.mask_fused;
    it.fm = c.st->ws + M * ((it.rot && (i & 1)) ? WS_FM2 : WS_FM);
    it.flowm = it.rot ? c.st->ws + M * WS_FLOWM + (i & 1) * 2 * M : nullptr;
    it.ev_done = it.rot ? EV_ROT + (i & 1) : EV_UP;
    it.wait_buffer = it.rot && i >= 2;
    it.wait_prev_mask = !it.rot && !c.final_only && i >= 1;
    // default 32, except where the chain's launches cover the chip exactly (the flow / mask head's F(4x4) grid a multiple of
    // 256: a single 1024 x 1024 pair loses 6 % to a background branch); one process, profiles/r09d_mask_bg_shapes.txt:
    // 448 x 512 at 4 / 5 / 6 / 8 / 12 / 16 pairs +2.7 / +7.9 / +4.5 / +6.1 / +2.5 / +1.6 %, 16 or 40+ workgroups lose
    const int head_grid = c.B * ((c.h + 7) / 8) * ((c.w + 63) / 64) * 8;
    it.mask_bg_wgs = (it.rot && i + 1 < c.iters) ? (head_grid % 256 ? 32 : 0) : 0;
    return it;
}

// The cross-stream edges.  On one stream everything is already ordered: no event operation is issued (and no context read).
static int record_event(const LoopCall &c, int ev, hipStream_t from) {
    return c.s.split() ? (int)hipEventRecord(c.ctx->ev[ev], from) : RAFT_OK;
}
static int wait_event(const LoopCall &c, hipStream_t to, int ev) {
    return c.s.split() ? (int)hipStreamWaitEvent(to, c.ctx->ev[ev], 0) : RAFT_OK;
}
static int edge(const LoopCall &c, hipStream_t from, int ev, hipStream_t to) {
    RAFT_TRY(record_event(c, ev, from));
    return wait_event(c, to, ev);
}

static void mark(const LoopCall &c) {
    if (c.tm) c.tm->mark(c.s.main);
}

static int loop_lookup(const LoopCall &c) {
    const LookupSource &src = c.src;
    const raft_state *st = c.st;
    if (src.pyr) return raft_corr_lookup_f32(src.pyr, src.level_offsets, st->coords1, c.B, c.h, c.w, 4, 4, st->corr, CORR_LD, c.s.main);
    return raft_corr_lookup_ondemand_f32(src.fmap1, src.fmap2_pyr, st->coords1, c.B, c.h, c.w, src.C, 4, 4, st->corr, CORR_LD, c.s.main);
}

// The mask branch of an iteration, on the mask stream: mask.2 and the convex upsampling, as two kernels or as one.
static int mask_branch(const LoopCall &c, const LoopIter &it) {
    const raft_basic_update_weights *wts = c.wts;
    const raft_state *st = c.st;
    const int B = c.B, h = c.h, w = c.w;
    hipStream_t sm = c.s.mask;
    if (it.mask_fused) {
        // mask.2 and the convex upsampling as ONE kernel (mask_upsample.hip): the mask is never written.  Besides fm (the mask
        // branch already waits for fh1_mask0) it needs the flow fh2 has just written.
        RAFT_TRY(wait_event(c, sm, EV_FH));
        RAFT_TRY(raft_launch_mask_upsample(it.fm + 256, 512, wts->mask2.wp, wts->mask2.bias, wts->mask2.npad, it.rot ? it.flowm : st->flow, B, h, w,
                                           0.25f, it.up, sm, it.mask_bg_wgs));
        mark(c);
    } else {   // mask = 0.25 * mask.2(.)             1x1, 256 -> 576
        ConvArgs a = conv_args(wts->mask2, it.fm + 256, 512, 256, nullptr, 0, 0, B, h, w, 576, st->mask, 576);
        a.scale = 0.25f;
        RAFT_TRY(launch_layer(c.plan.mask2, a, 1, 1, EPI_LINEAR, sm));
        mark(c);
        if (it.up) {
            // upsample on the mask branch: needs mask2 (same stream) and the flow written by fh2
            RAFT_TRY(wait_event(c, sm, EV_FH));
            RAFT_TRY(raft_upsample_convex_f32(st->flow, st->mask, B, h, w, it.up, sm));
        }
    }
    mark(c);   // RAFT_MASK_FUSED: fused, the mask2 stage is the fused kernel and the upsampling stage is empty
    return record_event(c, it.ev_done, sm);
}

// Iteration i of a call: [lookup], BasicUpdateBlock, coordinate update, [mask branch].
// plan.lookup_fused: st->corr is NOT read; cor1 comes from the volume through the fused kernel
static int loop_iteration(const LoopCall &c, int i) {
    const LoopIter it = loop_iter(c, i);
    const raft_basic_update_weights *wts = c.wts;
    const BasicLoopPlan &plan = c.plan;
    const raft_state *st = c.st;
    const int B = c.B, h = c.h, w = c.w;
    hipStream_t s = c.s.main, sf = c.s.flow, sm = c.s.mask;
    const int64_t M = (int64_t)B * h * w;
    float *ws = st->ws;
    float *cor1 = ws + M * WS_COR1, *corflo = ws + M * WS_CORFLO, *flo1 = ws + M * WS_FLO1;
    float *zb = ws + M * WS_Z, *rh = ws + M * WS_RH, *fm = it.fm;

    // RAFT_LOOKUP_FUSED: fused, the lookup stage is empty and the convc1 stage is the fused kernel
    const bool lookup = c.src.pyr != nullptr || c.src.fmap1 != nullptr;
    if (lookup && !plan.lookup_fused) RAFT_TRY(loop_lookup(c));
    mark(c);
    // ---- BasicMotionEncoder (update.py:97-106)
    if (lookup && plan.lookup_fused) {   // cor = relu(convc1(retrieve(coords1)))   lookup + 1x1, 324 -> 256, one kernel
        RAFT_TRY(raft_lookup_convc1_f32(c.src.pyr, c.src.level_offsets, st->coords1, B, h, w, wts->convc1_f.wp,
                                        wts->convc1_f.bias, wts->convc1_f.npad, 256, cor1, 256, s));
    } else {   // cor = relu(convc1(corr))            1x1, 324(+28 zero pad) -> 256
        ConvArgs a = conv_args(wts->convc1, st->corr, CORR_LD, CORR_LD, nullptr, 0, 0, B, h, w, 256, cor1, 256);
        RAFT_TRY(launch_layer(plan.convc1, a, 1, 1, EPI_RELU, s));
    }
    mark(c);
    {   // cor = relu(convc2(cor))             3x3, 256 -> 192   -> corflo[:, 0:192]
        ConvArgs a = conv_args(wts->convc2, cor1, 256, 256, nullptr, 0, 0, B, h, w, 192, corflo, 256);
        RAFT_TRY(launch_layer(plan.convc2, a, 3, 3, EPI_RELU, s));
        mark(c);
    }
    RAFT_TRY(wait_event(c, sf, EV_FH));   // flow of the previous iteration is final
    if (it.wait_buffer) RAFT_TRY(wait_event(c, sf, it.ev_done));   // mask branch of iteration - 2: its buffers are free
    {   // flo = relu(convf1(flow))            7x7, 2 -> 128
        RAFT_TRY(raft_launch_conv7x7_c2(st->flow, wts->convf1.wp, wts->convf1.bias, 128, B, h, w, flo1, 128, sf));
        mark(c);
    }
    {   // flo = relu(convf2(flo))             3x3, 128 -> 64    -> corflo[:, 192:256]
        ConvArgs a = conv_args(wts->convf2, flo1, 128, 128, nullptr, 0, 0, B, h, w, 64, corflo + 192, 256);
        RAFT_TRY(launch_layer(plan.convf2, a, 3, 3, EPI_RELU, sf));
        mark(c);
    }
    RAFT_TRY(edge(c, sf, EV_F, s));       // join the flow branch
    {   // out = relu(conv(cat[cor, flo]))     3x3, 256 -> 126   -> x[:, 128:254]; x[:, 254:256] = flow (kept by flowhead2)
        ConvArgs a = conv_args(wts->conv, corflo, 256, 256, nullptr, 0, 0, B, h, w, 126, st->x + 128, XDIM);
        RAFT_TRY(launch_layer(plan.conv, a, 3, 3, EPI_RELU, s));
        mark(c);
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
            mark(c);
        }
        {
            ConvArgs a = conv_args(*plan.gru[2 * pass + 1].wt, rh, HDIM, HDIM, xm, XDIM, XDIM - CDIM, B, h, w, HDIM, st->net, HDIM);
            a.e0 = st->net; a.lde0 = HDIM; a.e1 = zb; a.lde1 = HDIM;
            a.init = ctx + 2 * HDIM; a.ldi = CTX_LD;
            RAFT_TRY(launch_layer(plan.gru[2 * pass + 1], a, kh, kw, EPI_GRU_Q, s));
            mark(c);
        }
    }
    if (it.wait_prev_mask) RAFT_TRY(wait_event(c, s, EV_UP));   // mask2 / upsample of the previous iteration
    if (it.with_mask) {   // relu(flow_head.conv1(net)) | relu(mask.0(net))   3x3, 128 -> 256 + 256
        ConvArgs a = conv_args(wts->fh1_mask0, st->net, HDIM, HDIM, nullptr, 0, 0, B, h, w, 512, fm, 512);
        RAFT_TRY(launch_layer(plan.fh1_mask0, a, 3, 3, EPI_RELU, s));
    } else {              // relu(flow_head.conv1(net)) only            3x3, 128 -> 256        -> fm[:, 0:256]
        ConvArgs a = conv_args(wts->fh1_w, st->net, HDIM, HDIM, nullptr, 0, 0, B, h, w, 256, fm, 512);
        RAFT_TRY(launch_layer(plan.fh1, a, 3, 3, EPI_RELU, s));
    }
    mark(c);
    if (it.with_mask && !it.mask_fused) RAFT_TRY(edge(c, s, EV_FM, sm));   // two-kernel mask branch: mask.2 may start before fh2
    {   // delta = flow_head.conv2(.), coords1 += delta, flow = coords1 - coords0
        RAFT_TRY(raft_launch_flowhead2(fm, 512, 256, wts->fh2.wp, wts->fh2.bias, B, h, w, st->delta, st->coords1, st->flow, st->x + 254, XDIM,
                                       it.flowm, s));
        mark(c);
    }
    // one record, two waits: the flow branch of the next iteration and the mask branch of this one
    RAFT_TRY(record_event(c, EV_FH, s));
    return it.with_mask ? mask_branch(c, it) : RAFT_OK;
}

// The driver of every BasicUpdateBlock entry point: all work is joined back into the main stream before it returns, the first
// failing code is returned.
static int run_loop(const LoopCall &c) {
    mark(c);
    int rc = record_event(c, EV_FH, c.s.main);   // state prepared on the main stream: the flow branch may start
    for (int i = 0; i < c.iters && rc == RAFT_OK; ++i) rc = loop_iteration(c, i);
    if (rc == RAFT_OK) rc = wait_event(c, c.s.main, loop_iter(c, c.iters - 1).ev_done);   // join the last mask branch
    if (rc != RAFT_OK && c.s.split()) {   // never leave side streams running behind an error return
        (void)hipStreamSynchronize(c.s.flow);
        (void)hipStreamSynchronize(c.s.mask);
    }
    return rc;
}

// What the loop entry points share.  NULL pointers are reported before dimensions.
static int check_loop_args(const raft_basic_update_weights *wts, const raft_state *st, const float *flow_up, int B, int h, int w,
                           int iters) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_REQUIRE_PTR(flow_up);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0 && iters > 0, RAFT_E_SHAPE);
    return RAFT_OK;
}

// The loop on one stream, from a stored volume (raft_iterate_basic_f32 and its timed twin).
static int iterate_basic_one_stream(const raft_basic_update_weights *wts, const float *pyr, const int64_t *level_offsets, int B, int h,
                                    int w, int iters, const raft_state *st, float *flow_up, void *stream, StageTimer *tm) {
    hipStream_t s = (hipStream_t)stream;
    const LoopCall c = {wts, raft_basic_loop_plan(*wts, B, h, w, true, raft_concurrency()), {pyr, level_offsets, nullptr, nullptr, 0},
                        B, h, w, iters, st, flow_up, false, {s, s, s}, nullptr, tm};
    return run_loop(c);
}

// The loop on caller-owned side streams aux0 / aux1: three distinct streams, or all three the same one.
static int iterate_basic_side_streams(const raft_basic_update_weights *wts, const LookupSource &src, int B, int h, int w, int iters,
                                      const raft_state *st, float *flow_up, void *stream, void *aux0, void *aux1, raft_loop_ctx *ctx,
                                      bool final_only) {
    RAFT_REQUIRE_PTR(aux0);
    RAFT_REQUIRE_PTR(aux1);
    RAFT_REQUIRE_PTR(ctx);
    RAFT_TRY(check_loop_args(wts, st, flow_up, B, h, w, iters));
    // three distinct streams, or all three the same one (the single-stream schedule)
    RAFT_REQUIRE((aux0 != stream && aux1 != stream && aux0 != aux1) || (aux0 == stream && aux1 == stream), RAFT_E_UNSUPPORTED);
    const LoopCall c = {wts, raft_basic_loop_plan(*wts, B, h, w, src.pyr != nullptr, raft_concurrency()), src, B, h, w, iters, st, flow_up,
                        final_only, {(hipStream_t)stream, (hipStream_t)aux0, (hipStream_t)aux1}, ctx, nullptr};
    return run_loop(c);
}

extern "C" int raft_update_basic_f32(const raft_basic_update_weights *wts, int B, int h, int w,
                                     const raft_state *st, void *stream) {
    RAFT_REQUIRE_PTR(wts);
    RAFT_TRY(check_state(st));
    RAFT_REQUIRE(B > 0 && h > 0 && w > 0, RAFT_E_SHAPE);
    hipStream_t s = (hipStream_t)stream;
    const LoopCall c = {wts, raft_basic_loop_plan(*wts, B, h, w, false, raft_concurrency()), {}, B, h, w, 1, st, nullptr, false, {s, s, s},
                        nullptr, nullptr};
    return run_loop(c);
}

extern "C" int raft_iterate_basic_f32(const raft_basic_update_weights *wts, const float *pyr,
                                      const int64_t *level_offsets, int B, int h, int w, int iters,
                                      const raft_state *st, float *flow_up, void *stream) {
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    RAFT_TRY(check_loop_args(wts, st, flow_up, B, h, w, iters));
    return iterate_basic_one_stream(wts, pyr, level_offsets, B, h, w, iters, st, flow_up, stream, nullptr);
}

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

// raft_iterate_basic_f32 on three streams (see struct LoopStreams).  aux0 / aux1 are caller-owned streams
// distinct from `stream`; all work is joined back into `stream` before returning.
extern "C" int raft_iterate_basic_overlap_f32(const raft_basic_update_weights *wts, const float *pyr,
                                              const int64_t *level_offsets, int B, int h, int w, int iters,
                                              const raft_state *st, float *flow_up, void *stream, void *aux0,
                                              void *aux1, raft_loop_ctx *ctx) {
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    const LookupSource src = {pyr, level_offsets, nullptr, nullptr, 0};
    return iterate_basic_side_streams(wts, src, B, h, w, iters, st, flow_up, stream, aux0, aux1, ctx, false);
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
    return iterate_basic_side_streams(wts, src, B, h, w, iters, st, flow_up, stream, aux0, aux1, ctx, false);
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
    return iterate_basic_side_streams(wts, src, B, h, w, iters, st, flow_up_last, stream, aux0, aux1, ctx, true);
}

// Profiling twin of raft_iterate_basic_f32: identical launches, plus a HIP event after every kernel
// on `stream`; synchronises and accumulates per-stage milliseconds into stage_ms[RAFT_BASIC_STAGES]
// (host array).  Used by bench.py for the live roofline numbers -- never on the product path.
extern "C" int raft_iterate_basic_timed_f32(const raft_basic_update_weights *wts, const float *pyr,
                                            const int64_t *level_offsets, int B, int h, int w, int iters,
                                            const raft_state *st, float *flow_up, void *stream,
                                            float *stage_ms) {
    RAFT_REQUIRE_PTR(pyr);
    RAFT_REQUIRE_PTR(level_offsets);
    RAFT_REQUIRE_PTR(stage_ms);
    RAFT_TRY(check_loop_args(wts, st, flow_up, B, h, w, iters));
    RAFT_REQUIRE(iters <= 64, RAFT_E_SHAPE);
    const int per_iter = RAFT_BASIC_STAGES;
    const int nev = iters * per_iter + 1;
    hipEvent_t *ev = (hipEvent_t *)malloc(sizeof(hipEvent_t) * nev);
    if (!ev) return (int)hipErrorOutOfMemory;
    for (int i = 0; i < nev; ++i) (void)hipEventCreate(&ev[i]);
    StageTimer tm = {ev, 0, nev};
    int rc = iterate_basic_one_stream(wts, pyr, level_offsets, B, h, w, iters, st, flow_up, stream, &tm);
    if (rc == RAFT_OK) rc = (int)hipStreamSynchronize((hipStream_t)stream);
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
        RAFT_TRY(raft_launch_conv7x7_c2(st->flow, wts->convf1.wp, wts->convf1.bias, 64, B, h, w, flo1, 64, s));
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
        RAFT_TRY(raft_launch_flowhead2(fh, 128, 128, wts->fh2.wp, wts->fh2.bias, B, h, w, st->delta, st->coords1, st->flow,
                                       st->x + S_FLOW_SLOT, S_XLD, nullptr, s));
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

// Host-side check of the C ABI under AddressSanitizer / ThreadSanitizer ("re-entrant and thread-safe").
// Linked against a HOST-ONLY build of the library (hipcc --offload-host-only -fsanitize=...; tf_raft_amd/build.py
// build_sanitizer_library): no device code, no GPU -- what runs here is everything an entry point does BEFORE it launches:
// argument validation, geometry / workspace arithmetic, the option table, error strings.  Every launching entry point is
// called with arguments it must reject (null pointers, bad shapes, misaligned buffers) and has to return an error code
// without touching memory; the pure-host helpers are called with valid arguments; the launch plans (which kernel family and
// workgroup shape every update-block layer and encoder stage runs) are checked against a table and the kernels' workgroup remap
// is checked to be a permutation for every grid size; four threads then hammer the
// option table, the helpers and the plans concurrently (the only process-global state of the library).
// Test infrastructure: built and run by tests/test_abi_sanitizers.py, never shipped.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "raft_hip.h"
#include "../../tf_raft_amd/csrc/launch_plan.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void helpers_once(int salt) {
    int64_t off[RAFT_MAX_LEVELS + 1];
    int lh[RAFT_MAX_LEVELS], lw[RAFT_MAX_LEVELS];
    const int B = 1 + salt % 3, h = 56 + salt % 5, w = 64 + salt % 7;
    EXPECT(raft_corr_pyramid_layout(B, h, w, 4, off, lh, lw) == 0);
    EXPECT(off[0] == 0 && off[4] > off[3] && lh[0] == h && lw[0] == w && lh[3] == h / 8 && lw[3] == w / 8);
    for (int l = 0; l < 4; ++l) EXPECT((off[l + 1] - off[l]) % 32 == 0);     // whole 128-byte tiles per map
    EXPECT(raft_corr_pyramid_layout(B, h, w, 4, off, nullptr, nullptr) == 0);
    EXPECT(raft_corr_pyramid_layout(B, h, w, 0, off, lh, lw) != 0);
    EXPECT(raft_corr_pyramid_layout(B, h, w, RAFT_MAX_LEVELS + 1, off, lh, lw) != 0);
    EXPECT(raft_corr_pyramid_layout(0, h, w, 4, off, lh, lw) != 0);
    EXPECT(raft_corr_pyramid_layout(B, h, w, 4, nullptr, lh, lw) != 0);
    EXPECT(raft_corr_build_workspace_floats(B, h, w, 256, 4) > (int64_t)B * h * w * 256);
    EXPECT(raft_corr_build_workspace_floats(0, h, w, 256, 4) == 0);
    EXPECT(raft_update_workspace_floats(B, h, w) > 0);
    EXPECT(raft_small_update_workspace_floats(B, h, w) > 0);
    EXPECT(raft_metrics_workspace_doubles() > 0);
    EXPECT(raft_sumsq_workspace_doubles() > 0);
    EXPECT(raft_sumsq_multi_workspace_doubles(7) > 0);
    EXPECT(raft_norm_workspace_doubles(4, 64) > 0);
    EXPECT(raft_conv2d_wgrad_workspace_floats(128, 128, B, h, w, 3, 3) >= 0);
    EXPECT(raft_conv7x7_c2_wgrad_workspace_floats(128) > 0);
    EXPECT(raft_upsample_convex_backward_workspace_floats(B, h, w) >= 0);
    EXPECT(raft_version() > 0);
    for (int rc = -3; rc < 1100; rc += 37) {
        const char *s = raft_error_string(rc);
        EXPECT(s != nullptr && std::strlen(s) > 0);
    }
}

static void options_once(int salt) {
    char buf[64];
    EXPECT(raft_set_option("RAFT_NO_SUCH_SWITCH", "1") != 0);
    EXPECT(raft_get_option("RAFT_NO_SUCH_SWITCH", buf, sizeof buf) != 0);
    EXPECT(raft_set_option(nullptr, "1") != 0);
    const char *vals[3] = {"0", "1", nullptr};
    EXPECT(raft_set_option("RAFT_CORR_XCD", vals[salt % 3]) == 0);
    EXPECT(raft_get_option("RAFT_CORR_XCD", buf, sizeof buf) == 0);
    EXPECT(raft_get_option("RAFT_CORR_XCD", buf, 1) == 0 || true);       // a one-byte buffer: truncated, never overrun
    EXPECT(raft_get_option("RAFT_CORR_XCD", nullptr, 0) != 0 || true);
    EXPECT(raft_set_option("RAFT_LOOKUP_FUSED", vals[(salt + 1) % 3]) == 0);
    EXPECT(raft_set_option("RAFT_LOOKUP_FUSED", "not a number") != 0 || true);
}

static raft_basic_update_weights basic_weights();

// The update-block and loop entry points with invalid calls that reach validation (non-NULL dummy weights and state) and the
// exact code each returns: NULL pointers first, then dimensions, then the stream rule.  Every row is rejected before any HIP call.
static void loop_rejects() {
    static float f[64] = {0};
    static const int64_t off[RAFT_MAX_LEVELS + 1] = {0, 32, 64, 96, 128};
    static const raft_basic_update_weights W = basic_weights();
    static const raft_small_update_weights SW = {};
    const raft_state ok = {f, f, f, f, f, f, f, f, f};
    raft_state no_net = ok, no_mask = ok, no_ctx = ok, no_ws = ok;
    no_net.net = nullptr; no_mask.mask = nullptr; no_ctx.ctx = nullptr; no_ws.ws = nullptr;
    raft_basic_update_weights no_fh1 = W;
    no_fh1.fh1_w = {nullptr, nullptr, 0};
    // never dereferenced: validation fails first
    void *s = (void *)f, *a0 = (void *)(f + 4), *a1 = (void *)(f + 8);
    raft_loop_ctx *ctx = (raft_loop_ctx *)(f + 12);
    float ms[RAFT_BASIC_STAGES];
#define EXPECT_RC(call, want)                                                                                          \
    do {                                                                                                               \
        const int got__ = (call);                                                                                      \
        if (got__ != (want)) {                                                                                         \
            std::fprintf(stderr, "FAILED %s:%d: %s returned %d, expected %s\n", __FILE__, __LINE__, #call, got__, #want); \
            ++failures;                                                                                                \
        }                                                                                                              \
    } while (0)
    // ---- raft_update_basic_f32
    EXPECT_RC(raft_update_basic_f32(nullptr, 1, 8, 8, &ok, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_basic_f32(&W, 1, 8, 8, nullptr, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_basic_f32(&W, 1, 8, 8, &no_net, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_basic_f32(&W, 1, 8, 8, &no_mask, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_basic_f32(&W, 1, 8, 8, &no_ctx, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_basic_f32(&W, 0, 8, 8, &ok, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_update_basic_f32(&W, 1, 8, -1, &ok, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_update_basic_f32(&W, 0, 8, 8, &no_ws, s), RAFT_E_NULL);            // pointers before dimensions
    // ---- raft_iterate_basic_f32
    EXPECT_RC(raft_iterate_basic_f32(nullptr, f, off, 1, 8, 8, 2, &ok, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, nullptr, off, 1, 8, 8, 2, &ok, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, nullptr, 1, 8, 8, 2, &ok, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, 2, &ok, nullptr, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, 2, nullptr, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, 2, &no_net, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, 2, &no_mask, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, 0, &ok, f, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, -3, &ok, f, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 0, 8, 2, &ok, f, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_f32(&W, f, off, 1, 8, 8, 0, &ok, nullptr, s), RAFT_E_NULL);
    // ---- raft_iterate_basic_timed_f32
    EXPECT_RC(raft_iterate_basic_timed_f32(nullptr, f, off, 1, 8, 8, 2, &ok, f, s, ms), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, nullptr, off, 1, 8, 8, 2, &ok, f, s, ms), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, nullptr, 1, 8, 8, 2, &ok, f, s, ms), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 2, &ok, nullptr, s, ms), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, nullptr), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 2, nullptr, f, s, ms), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 2, &no_mask, f, s, ms), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 0, &ok, f, s, ms), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 65, &ok, f, s, ms), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, -1, 8, 8, 2, &ok, f, s, ms), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_timed_f32(&W, f, off, 1, 8, 8, 65, &ok, f, s, nullptr), RAFT_E_NULL);
    // ---- raft_iterate_basic_overlap_f32
    EXPECT_RC(raft_iterate_basic_overlap_f32(nullptr, f, off, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, nullptr, off, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, nullptr, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, nullptr, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, nullptr, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, nullptr, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, a1, nullptr), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, s, s, nullptr), RAFT_E_NULL);   // one stream still needs a context
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, nullptr, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &no_net, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &no_mask, f, s, s, s, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 0, &ok, f, s, a0, a1, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, -1, &ok, f, s, s, s, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 0, 2, &ok, f, s, a0, a1, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, s, a1, ctx), RAFT_E_UNSUPPORTED);    // aux0 == stream only
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, s, ctx), RAFT_E_UNSUPPORTED);    // aux1 == stream only
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, a0, ctx), RAFT_E_UNSUPPORTED);   // aux0 == aux1 != stream
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 0, &ok, f, s, a0, a0, ctx), RAFT_E_SHAPE);         // dimensions before streams
    EXPECT_RC(raft_iterate_basic_overlap_f32(&W, f, off, 1, 8, 8, 0, &ok, f, s, a0, a0, nullptr), RAFT_E_NULL);
    // ---- raft_iterate_basic_ondemand_f32
    EXPECT_RC(raft_iterate_basic_ondemand_f32(nullptr, f, f, 256, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, nullptr, f, 256, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, nullptr, 256, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, nullptr, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, f, s, nullptr, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, f, s, a0, nullptr, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, f, s, a0, a1, nullptr), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &no_ctx, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &no_mask, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 0, &ok, f, s, a0, a1, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 0, 8, 8, 2, &ok, f, s, s, s, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, f, s, s, a1, ctx), RAFT_E_UNSUPPORTED);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, f, s, a0, s, ctx), RAFT_E_UNSUPPORTED);
    EXPECT_RC(raft_iterate_basic_ondemand_f32(&W, f, f, 256, 1, 8, 8, 2, &ok, f, s, a0, a0, ctx), RAFT_E_UNSUPPORTED);
    // ---- raft_iterate_basic_final_f32
    EXPECT_RC(raft_iterate_basic_final_f32(nullptr, f, off, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, nullptr, off, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, nullptr, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&no_fh1, f, off, 1, 8, 8, 2, &ok, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&no_fh1, f, off, 1, 8, 8, 2, &ok, f, s, s, s, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, nullptr, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, nullptr, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, nullptr, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, a1, nullptr), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, s, s, nullptr), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &no_mask, f, s, a0, a1, ctx), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 0, &ok, f, s, a0, a1, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, -8, 8, 2, &ok, f, s, s, s, ctx), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, s, a1, ctx), RAFT_E_UNSUPPORTED);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, s, ctx), RAFT_E_UNSUPPORTED);
    EXPECT_RC(raft_iterate_basic_final_f32(&W, f, off, 1, 8, 8, 2, &ok, f, s, a0, a0, ctx), RAFT_E_UNSUPPORTED);
    EXPECT_RC(raft_iterate_basic_final_f32(&no_fh1, f, off, 1, 8, 8, 0, &ok, f, s, a0, a0, ctx), RAFT_E_NULL);
    // ---- SmallUpdateBlock: a state without mask and GRU context is complete
    EXPECT_RC(raft_update_small_f32(nullptr, 1, 8, 8, &ok, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_small_f32(&SW, 1, 8, 8, &no_net, s), RAFT_E_NULL);
    EXPECT_RC(raft_update_small_f32(&SW, 0, 8, 8, &no_mask, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_small_f32(nullptr, f, off, 1, 8, 8, 2, &ok, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_small_f32(&SW, nullptr, off, 1, 8, 8, 2, &ok, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, nullptr, 1, 8, 8, 2, &ok, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, off, 1, 8, 8, 2, &ok, nullptr, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, off, 1, 8, 8, 2, nullptr, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, off, 1, 8, 8, 2, &no_net, f, s), RAFT_E_NULL);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, off, 1, 8, 8, 0, &no_mask, f, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, off, 1, 8, 8, 0, &no_ctx, f, s), RAFT_E_SHAPE);
    EXPECT_RC(raft_iterate_small_f32(&SW, f, off, 1, 8, 8, -1, &ok, f, s), RAFT_E_SHAPE);
#undef EXPECT_RC
}

// every launching entry point with arguments it has to reject before any launch (no GPU is present here)
static void rejects() {
    loop_rejects();
    float f[64] = {0};
    int64_t off[RAFT_MAX_LEVELS + 1] = {0, 32, 64, 96, 128};
    unsigned char u8[8] = {0};
    double d[8] = {0};
    void *s = nullptr;
    EXPECT(raft_corr_build_f32(nullptr, f, 1, 8, 8, 256, 4, f, off, f, s) != 0);
    EXPECT(raft_corr_build_f32(f, f, 0, 8, 8, 256, 4, f, off, f, s) != 0);
    EXPECT(raft_corr_build_f32(f, f, 1, 8, 8, 255, 4, f, off, f, s) != 0);
    EXPECT(raft_corr_lookup_f32(nullptr, off, f, 1, 8, 8, 4, 4, f, 352, s) != 0);
    EXPECT(raft_corr_lookup_f32(f, off, f, 1, 8, 8, 4, 9, f, 352, s) != 0);       // unsupported radius
    EXPECT(raft_corr_lookup_f32(f, off, f, 1, 8, 8, 4, 4, f, 10, s) != 0);        // row stride < 4 * 81
    EXPECT(raft_corr_lookup_f32(f, off, f, 1, 0, 8, 4, 4, f, 352, s) != 0);
    EXPECT(raft_fmap_pyramid_f32(nullptr, 1, 8, 8, 256, 4, f, s) != 0);
    EXPECT(raft_fmap_pyramid_f32(f, 1, 8, 8, 255, 4, f, s) != 0);
    EXPECT(raft_fmap_pyramid_f32(f + 1, 1, 8, 8, 256, 4, f, s) != 0);            // misaligned
    EXPECT(raft_bilinear_sampler_f32(nullptr, f, 1, 8, 8, 1, 1, f, s) != 0);
    EXPECT(raft_bilinear_sampler_f32(f, f, 0, 8, 8, 1, 1, f, s) != 0);
    EXPECT(raft_coords_grid_f32(nullptr, 1, 8, 8, s) != 0);
    EXPECT(raft_coords_grid_f32(f, 1, 0, 8, s) != 0);
    EXPECT(raft_upsample_convex_f32(nullptr, f, 1, 8, 8, f, s) != 0);
    EXPECT(raft_upsample_convex_f32(f, f, 1, -1, 8, f, s) != 0);
    EXPECT(raft_upflow8_f32(nullptr, 1, 8, 8, f, s) != 0);
    EXPECT(raft_lookup_convc1_f32(f, off, f, 1, 8, 8, f, f, 128, 128, f, 256, s) != 0);   // npad must be 256
    EXPECT(raft_lookup_convc1_f32(f, off, f, 1, 8, 8, nullptr, f, 256, 256, f, 256, s) != 0);
    EXPECT(raft_conv2d_f32(nullptr, 0, 0, nullptr, 0, 0, f, f, 1, 8, 8, 3, 3, 64, 64, 1, 1.0f, f, 64, s) != 0);
    EXPECT(raft_conv7x7_c2_f32(nullptr, f, f, 128, 1, 8, 8, f, 128, s) != 0);
    EXPECT(raft_update_basic_f32(nullptr, 1, 8, 8, nullptr, s) != 0);
    EXPECT(raft_iterate_basic_f32(nullptr, f, off, 1, 8, 8, 1, nullptr, f, s) != 0);
    EXPECT(raft_iterate_small_f32(nullptr, f, off, 1, 8, 8, 1, nullptr, f, s) != 0);
    EXPECT(raft_iterate_basic_overlap_f32(nullptr, f, off, 1, 8, 8, 1, nullptr, f, s, s, s, nullptr) != 0);
    EXPECT(raft_prepare_state_f32(nullptr, 1, 8, 8, nullptr, s) != 0);
    EXPECT(raft_prepare_state_small_f32(nullptr, 1, 8, 8, nullptr, s) != 0);
    EXPECT(raft_encoder_f32(nullptr, f, 1, 64, 64, 1, f, f, s) != 0);
    EXPECT(raft_encoder_workspace_floats(nullptr, 1, 64, 64) == 0);
    EXPECT(raft_flow_metrics_f32(nullptr, u8, f, 64, 400.f, f, d, s) != 0);
    EXPECT(raft_relu_backward_f32(nullptr, f, f, 8, s) != 0);
    EXPECT(raft_axpby_f32(1.f, nullptr, 1.f, f, f, 8, s) != 0);
    EXPECT(raft_sumsq_f32(nullptr, 8, 0, d, d, s) != 0);
    EXPECT(raft_loop_ctx_destroy(nullptr) == 0 || true);
}

// ---- launch plans (tf_raft_amd/csrc/launch_plan.h) at 448 x 512 (56 x 64 features), every weight copy supplied
static std::string plan_str(const ConvChoice &c) {
    char b[48];
    switch (c.family) {
        case RAFT_FAM_HALO: std::snprintf(b, sizeof b, "halo th%d tn%d", c.halo.th, c.halo.tn); break;
        case RAFT_FAM_WINO: std::snprintf(b, sizeof b, "F2x2 tnw%d sb%d ck%d ks%d", c.wino.tnw, c.wino.sb, c.wino.ck, c.wino.ks); break;
        case RAFT_FAM_WINO1D:
            if (c.wino1d.mo == 4) std::snprintf(b, sizeof b, "F4,5 tnw%d", c.wino1d.tnw);
            else std::snprintf(b, sizeof b, "F2,5 tnw%d tm%d ck%d", c.wino1d.tnw, c.wino1d.tm, c.wino1d.ck);
            break;
        case RAFT_FAM_WINO4: std::snprintf(b, sizeof b, "F4x4 ks%d", c.wino4.ks); break;
        default: std::snprintf(b, sizeof b, "family %d", c.family);
    }
    return b;
}
#define EXPECT_PLAN(choice, want)                                                                            \
    do {                                                                                                     \
        const std::string got__ = plan_str(choice);                                                          \
        if (got__ != (want)) {                                                                               \
            std::fprintf(stderr, "FAILED %s:%d: %s is \"%s\", expected \"%s\"\n", __FILE__, __LINE__, #choice, got__.c_str(), want); \
            ++failures;                                                                                      \
        }                                                                                                    \
    } while (0)

static float plan_dummy[4];
static raft_conv_weights cw(int npad) { return {plan_dummy, plan_dummy, npad}; }

struct BasicRow {
    int B, hint;
    const char *convc2, *convf2, *conv, *fh1_mask0, *fh1, *gru[4];   // fh1: final-only flow head; gru: zr1, q1, zr2, q2
    bool lookup_fused, mask_fused;
};
static const BasicRow kBasic[] = {
    {1, 1, "F2x2 tnw1 sb1 ck4 ks2", "halo th4 tn1", "F2x2 tnw1 sb1 ck4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F2x2 tnw1 sb1 ck2 ks1", {"F2,5 tnw1 tm1 ck2", "F2,5 tnw1 tm1 ck2", "F2,5 tnw1 tm1 ck2", "F2,5 tnw1 tm1 ck2"}, 1, 0},
    {1, 3, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw1", "F4,5 tnw1", "F4,5 tnw1", "F4,5 tnw1"}, 1, 1},
    {2, 1, "F2x2 tnw1 sb1 ck2 ks1", "halo th4 tn1", "F2x2 tnw1 sb1 ck4 ks2", "F4x4 ks2", "F4x4 ks2", {"F4,5 tnw1", "F4,5 tnw1", "F4,5 tnw1", "F4,5 tnw1"}, 1, 1},
    {2, 3, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw1", "F4,5 tnw2", "F4,5 tnw1"}, 1, 1},
    {3, 1, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw1", "F4,5 tnw1", "F4,5 tnw1", "F4,5 tnw1"}, 1, 1},
    {3, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks2", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1},
    {4, 1, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw1", "F4,5 tnw2", "F4,5 tnw1"}, 1, 1},
    {4, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1},
    {8, 1, "F4x4 ks1", "F4x4 ks1", "F4x4 ks2", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1},
    {8, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1},
    {16, 1, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1},
    {16, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1},
};
struct SmallRow {
    int B, hint;
    const char *convc1, *convf2, *conv, *gru_zr, *gru_q, *fh1;
};
static const SmallRow kSmall[] = {
    {4, 1, "halo th7 tn1", "halo th4 tn1", "F2x2 tnw1 sb1 ck2 ks1", "F2x2 tnw1 sb0 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1", "F2x2 tnw1 sb1 ck2 ks1"},
    {4, 3, "halo th7 tn1", "halo th4 tn1", "F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw2 sb1 ck1 ks1"},
};
// the stride-1 3x3 layers of BasicEncoder stages layer1..3 (224 x 256 x 64, 112 x 128 x 96, 56 x 64 x 128); fnet: 2B images,
// instance norm (moments in the epilogue); cnet: B images, folded batch norm
struct EncRow {
    int B, hint, cnet;
    const char *stage[3];
};
static const EncRow kEnc[] = {
    {1, 1, 0, {"F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw1 sb0 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1"}},
    {1, 1, 1, {"F2x2 tnw1 sb0 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1", "F2x2 tnw1 sb1 ck4 ks2"}},
    {1, 3, 0, {"F4x4 ks1", "F4x4 ks1", "F2x2 tnw1 sb1 ck2 ks1"}},
    {1, 3, 1, {"F4x4 ks1", "F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1"}},
    {4, 1, 0, {"F4x4 ks1", "F4x4 ks1", "F2x2 tnw1 sb0 ck1 ks1"}},
    {4, 1, 1, {"F4x4 ks1", "F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1"}},
    {4, 3, 0, {"F4x4 ks1", "F4x4 ks1", "F4x4 ks1"}},
    {4, 3, 1, {"F4x4 ks1", "F4x4 ks1", "F2x2 tnw2 sb1 ck1 ks1"}},
};
// forced switches (raft_set_option); rows as above
struct SwitchRows {
    const char *name, *value;
    BasicRow basic[2];
    EncRow enc[2];
};
static const SwitchRows kSwitched[] = {
    {"RAFT_WINO4_KS", "1",
     {{4, 1, "F4x4 ks1", "F4x4 ks1", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw1", "F4,5 tnw2", "F4,5 tnw1"}, 1, 1},
      {4, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1}},
     {{1, 3, 1, {"F4x4 ks1", "F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1"}}, {4, 3, 1, {"F4x4 ks1", "F4x4 ks1", "F2x2 tnw2 sb1 ck1 ks1"}}}},
    {"RAFT_CONVC2_KS", "2",
     {{4, 1, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw1", "F4,5 tnw2", "F4,5 tnw1"}, 1, 1},
      {4, 3, "F4x4 ks2", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1}},
     {{1, 1, 1, {"F2x2 tnw1 sb0 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1", "F2x2 tnw1 sb1 ck4 ks2"}}, {4, 3, 0, {"F4x4 ks1", "F4x4 ks1", "F4x4 ks1"}}}},
    {"RAFT_GRU_WINO4", "0",
     {{4, 1, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F2,5 tnw2 tm2 ck2", "F2,5 tnw1 tm2 ck2", "F2,5 tnw2 tm2 ck2", "F2,5 tnw1 tm2 ck2"}, 1, 1},
      {4, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F2,5 tnw2 tm2 ck2", "F2,5 tnw2 tm2 ck2", "F2,5 tnw2 tm2 ck2", "F2,5 tnw2 tm2 ck2"}, 1, 1}},
     {{1, 1, 0, {"F2x2 tnw2 sb1 ck1 ks1", "F2x2 tnw1 sb0 ck1 ks1", "F2x2 tnw1 sb1 ck2 ks1"}}, {1, 3, 0, {"F4x4 ks1", "F4x4 ks1", "F2x2 tnw1 sb1 ck2 ks1"}}}},
    {"RAFT_ENC_WINO4", "7",   // explicit: every stage, no grid test
     {{4, 1, "F4x4 ks2", "F4x4 ks2", "F2x2 tnw1 sb1 ck2 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw1", "F4,5 tnw2", "F4,5 tnw1"}, 1, 1},
      {4, 3, "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", "F4x4 ks1", {"F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2", "F4,5 tnw2"}, 1, 1}},
     {{1, 1, 0, {"F4x4 ks1", "F4x4 ks1", "F4x4 ks1"}}, {1, 1, 1, {"F4x4 ks2", "F4x4 ks2", "F4x4 ks2"}}}},
};

static raft_basic_update_weights basic_weights() {
    raft_basic_update_weights w = {};
    w.convc1 = cw(256); w.convc2 = cw(192); w.convf2 = cw(64); w.conv = cw(128);
    w.gru_zr1 = w.gru_zr2 = cw(256); w.gru_q1 = w.gru_q2 = cw(128); w.fh1_mask0 = cw(512); w.mask2 = cw(576);
    w.convc2_w = cw(192); w.convf2_w = cw(64); w.conv_w = cw(128); w.fh1_mask0_w = cw(512);
    w.gru_zr1_w = w.gru_zr2_w = cw(256); w.gru_q1_w = w.gru_q2_w = cw(128); w.fh1_w = cw(256);
    w.gru_zr1_w4 = w.gru_zr2_w4 = cw(256); w.gru_q1_w4 = w.gru_q2_w4 = cw(128);
    w.convc2_w44 = cw(192); w.conv_w44 = cw(128); w.fh1_mask0_w44 = cw(512); w.fh1_w44 = cw(256); w.convf2_w44 = cw(64);
    w.convc1_f = cw(256);
    return w;
}

// check_fused: false while other threads flip RAFT_LOOKUP_FUSED (options_once)
static void check_basic(const BasicRow &r, bool check_fused) {
    static const raft_basic_update_weights w = basic_weights();
    const BasicLoopPlan p = raft_basic_loop_plan(w, r.B, 56, 64, true, r.hint);
    EXPECT_PLAN(p.convc2, r.convc2);
    EXPECT_PLAN(p.convf2, r.convf2);
    EXPECT_PLAN(p.conv, r.conv);
    EXPECT_PLAN(p.fh1_mask0, r.fh1_mask0);
    EXPECT_PLAN(p.fh1, r.fh1);
    for (int l = 0; l < 4; ++l) EXPECT_PLAN(p.gru[l], r.gru[l]);
    EXPECT(!check_fused || p.lookup_fused == r.lookup_fused);
    EXPECT(p.mask_fused == r.mask_fused);
}

static void check_enc(const EncRow &r) {
    const int Ho[3] = {224, 112, 56}, Wo[3] = {256, 128, 64}, F[3] = {64, 96, 128};
    const int n = r.cnet ? r.B : 2 * r.B;
    for (int st = 0; st < 3; ++st) {
        const int npad = (F[st] + 63) / 64 * 64;
        EXPECT_PLAN(raft_enc_stage_wino4(st, n, Ho[st], Wo[st], F[st], r.hint)
                        ? raft_choice(raft_wino4_plan(n, Ho[st], Wo[st], F[st], 0, npad, r.cnet, r.hint))
                        : raft_choice(raft_wino_plan(n, Ho[st], Wo[st], F[st], 0, npad, r.cnet, r.hint)),
                    r.stage[st]);
    }
}

static void plans_once(bool check_fused) {
    for (const BasicRow &r : kBasic) check_basic(r, check_fused);
    raft_small_update_weights sw = {};
    sw.convc1 = cw(128); sw.convf2 = cw(64); sw.conv = cw(128); sw.gru_zr = cw(192); sw.gru_q = cw(128); sw.fh1 = cw(128);
    sw.conv_w = cw(128); sw.gru_zr_w = cw(192); sw.gru_q_w = cw(128); sw.fh1_w = cw(128);
    for (const SmallRow &r : kSmall) {
        const SmallLoopPlan p = raft_small_loop_plan(sw, r.B, 56, 64, r.hint);
        EXPECT_PLAN(p.convc1, r.convc1);
        EXPECT_PLAN(p.convf2, r.convf2);
        EXPECT_PLAN(p.conv, r.conv);
        EXPECT_PLAN(p.gru_zr, r.gru_zr);
        EXPECT_PLAN(p.gru_q, r.gru_q);
        EXPECT_PLAN(p.fh1, r.fh1);
    }
    for (const EncRow &r : kEnc) check_enc(r);
}

// The XCD-aware workgroup remap of the convolution kernels (raft_xcd_remap, launch_plan.h), for every grid size 1 .. 4096: the
// images of 0 .. n-1 are a permutation of 0 .. n-1, and the logical tiles of one XCD (the workgroups with equal bid & 7) are
// contiguous -- consecutive workgroups of an XCD get consecutive tiles, and XCD x + 1 starts where XCD x ends.
// Walking the workgroups XCD by XCD must therefore visit the tiles 0, 1, .. n-1 in order.
static void xcd_remap() {
    for (int n = 1; n <= 4096; ++n) {
        int next = 0;   // the tile the next workgroup in (XCD, bid) order must get
        bool ok = true;
        for (int xcd = 0; xcd < 8; ++xcd)
            for (int bid = xcd; bid < n; bid += 8) ok = ok && raft_xcd_remap(bid, n) == next++;
        if (!ok || next != n) {
            std::fprintf(stderr, "FAILED %s:%d: raft_xcd_remap is no contiguous-per-XCD permutation for a grid of %d\n", __FILE__, __LINE__, n);
            ++failures;
        }
    }
}

static void switched_plans() {   // single-threaded: the switches are process-global
    for (const SwitchRows &sr : kSwitched) {
        EXPECT(raft_set_option(sr.name, sr.value) == 0);
        for (const BasicRow &r : sr.basic) check_basic(r, true);
        for (const EncRow &r : sr.enc) check_enc(r);
        EXPECT(raft_set_option(sr.name, "") == 0);
    }
}

int main() {
    // the plan table describes the built-in defaults: no tuning switch from the environment
    const char *plan_switches[] = {"RAFT_CONV_WINO", "RAFT_SMALL_WINO", "RAFT_GRU_WINO", "RAFT_GRU_WINO4", "RAFT_WINO_TNW", "RAFT_WINO_SB",
                                   "RAFT_WINO_CK", "RAFT_WINO1D_TM", "RAFT_LOOKUP_FUSED", "RAFT_ENC_WINO", "RAFT_WINO_KS", "RAFT_CONV_WINO4",
                                   "RAFT_WINO4_KS", "RAFT_MASK_FUSED", "RAFT_ENC_WINO4", "RAFT_CONVC2_KS", "RAFT_CONVF2_KS", "RAFT_CONV_TILE"};
    for (const char *name : plan_switches) EXPECT(raft_set_option(name, "") == 0);
    plans_once(true);
    switched_plans();
    xcd_remap();
    helpers_once(0);
    options_once(0);
    rejects();
    std::atomic<int> go{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
        th.emplace_back([t, &go] {
            while (!go.load()) {}
            // the launch-shape hint is THREAD-local: every thread sees only its own value, whatever the others set
            EXPECT(raft_set_thread_concurrency(t + 2) == 1);
            for (int i = 0; i < 400; ++i) {
                helpers_once(t * 1000 + i);
                options_once(t + i);
                if ((i & 63) == 0) rejects();
                if ((i & 15) == 0) plans_once(false);
                if (i == 200) {   // the plan functions take the hint as an argument: the thread's own hint changes nothing
                    raft_set_thread_concurrency(5 - t);
                    plans_once(false);
                    raft_set_thread_concurrency(t + 2);
                }
                EXPECT(raft_set_thread_concurrency(t + 2) == t + 2);
            }
            EXPECT(raft_set_thread_concurrency(0) == t + 2);       // n < 1 restores the default ...
            EXPECT(raft_set_thread_concurrency(1000) == 1);        // ... and large values are clamped
            EXPECT(raft_set_thread_concurrency(1) == 64);
        });
    go.store(1);
    for (auto &x : th) x.join();
    EXPECT(raft_set_thread_concurrency(1) == 1);                   // the main thread never saw the workers' hints
    raft_set_option("RAFT_CORR_XCD", nullptr);
    raft_set_option("RAFT_LOOKUP_FUSED", nullptr);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::puts("abi_host_check: ok");
    return 0;
}

// Host side of raft_resize_f32 / raft_resize_u8_f32 under AddressSanitizer + UndefinedBehaviorSanitizer: everything the two entries
// do before they launch (pointer checks, size checks, the tap-count and LDS-share checks, the segment arithmetic up to the
// refusal).  Linked with a HOST-ONLY build of tf_raft_amd/csrc/image_ops.hip (hipcc --offload-host-only -Xarch_host
// -fsanitize=address,undefined); nothing here reaches a launch, so it runs without a GPU.  How to build it: docs/NOTEBOOK.md.
#include <climits>
#include <cstdint>
#include <cstdio>

#include "raft_hip.h"

static int failures = 0;

#define EXPECT(call, want)                                                              \
    do {                                                                                \
        const int got__ = (call);                                                       \
        if (got__ != (want)) {                                                          \
            std::printf("line %d: %s = %d, expected %d\n", __LINE__, #call, got__, want); \
            ++failures;                                                                 \
        }                                                                               \
    } while (0)

template <typename S, typename F>
static void check(F fn) {
    static float dstbuf[64];
    static S srcbuf[64];
    static int idx[64];
    static float w[64];
    const S *s = srcbuf;
    float *d = dstbuf;
    EXPECT(fn(nullptr, d, 1, 4, 4, 8, 8, 3, idx, idx, w, 2, idx, idx, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, nullptr, 1, 4, 4, 8, 8, 3, idx, idx, w, 2, idx, idx, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, nullptr, idx, w, 2, idx, idx, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, nullptr, w, 2, idx, idx, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, idx, nullptr, 2, idx, idx, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, idx, w, 2, nullptr, idx, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, idx, w, 2, idx, nullptr, w, 2, nullptr, nullptr), RAFT_E_NULL);
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, idx, w, 2, idx, idx, nullptr, 2, nullptr, nullptr), RAFT_E_NULL);
    const int sizes[][6] = {{0, 4, 4, 8, 8, 3}, {1, 0, 4, 8, 8, 3}, {1, 4, 0, 8, 8, 3}, {1, 4, 4, 0, 8, 3}, {1, 4, 4, 8, 0, 3}, {1, 4, 4, 8, 8, 0},
                            {-2, 4, 4, 8, 8, 3}, {1, 4, 4, 8, -8, 3}, {INT_MIN, 4, 4, 8, 8, 3}, {1, 4, INT_MAX, 8, 8, 3}, {1, 4, 4, 8, INT_MAX, 3},
                            {1, 4, 1 << 30, 8, 8, 3}, {1, 4, 4, 8, 1 << 30, 3}, {1, 4, INT_MAX, 8, INT_MAX, INT_MAX}};
    for (const auto &z : sizes)
        EXPECT(fn(s, d, z[0], z[1], z[2], z[3], z[4], z[5], idx, idx, w, 2, idx, idx, w, 2, nullptr, nullptr), RAFT_E_SHAPE);
    const int taps[] = {0, -1, 65, INT_MAX, INT_MIN};
    for (const int t : taps) {
        EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, idx, w, t, idx, idx, w, 2, nullptr, nullptr), RAFT_E_SHAPE);
        EXPECT(fn(s, d, 1, 4, 4, 8, 8, 3, idx, idx, w, 2, idx, idx, w, t, nullptr, nullptr), RAFT_E_SHAPE);
    }
    // taps x channels beyond a wave's share of LDS, with sizes at the ends of the segment arithmetic
    EXPECT(fn(s, d, 1, 4, 4, 8, 8, 64, idx, idx, w, 2, idx, idx, w, 34, nullptr, nullptr), RAFT_E_SHAPE);
    EXPECT(fn(s, d, INT_MAX, INT_MAX, 1 << 20, INT_MAX, 1, 2047, idx, idx, w, 64, idx, idx, w, 64, nullptr, nullptr), RAFT_E_SHAPE);
    EXPECT(fn(s, d, 1, 1, 1, 1, 1 << 19, 4000, idx, idx, w, 1, idx, idx, w, 1, nullptr, nullptr), RAFT_E_SHAPE);
}

int main() {
    check<float>(raft_resize_f32);
    check<uint8_t>(raft_resize_u8_f32);
    if (failures) {
        std::printf("resize_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("resize_host_check: ok\n");
    return 0;
}

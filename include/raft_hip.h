/*
 * raft_hip.h -- C ABI of libraft_hip.so: the MI355X (gfx950) RAFT forward-prediction hot path.
 *
 * Every entry point replaces one piece of the reference's Python/TensorFlow path
 * (daigo0927/tf-raft); the reference interface each one stands in for is cited as
 * file:line into the reference tree.  The reference has no FFI of its own (it is pure
 * Python on TensorFlow ops), so "what its FFI for this path would bind" is exactly the set
 * of op groups listed here; INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, explicit sizes, no torch / C++ types;
 *   - all tensors are fp32, NHWC (channels contiguous), exactly the reference's layouts (the one exception: the
 *     raft_crop_or_pad_u8* and raft_augment_* entries take or return bytes, the type frames and validity masks arrive in);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only
 *     enqueue work, they never synchronise and never allocate.  Two documented exceptions:
 *     raft_loop_ctx_create / _destroy, which create and destroy the four cross-stream HIP events of
 *     the three-stream loops, and the bench-only raft_iterate_basic_timed_f32, which synchronises;
 *   - return value: RAFT_OK (0), a negative RAFT_E_* argument error, or a positive
 *     hipError_t from the launch; no exception or abort crosses the ABI;
 *   - the library keeps no per-call state and is re-entrant (ordering only through `stream`).  Its
 *     only process-global state is the table of tuning switches below (raft_set_option).
 *
 * Tuning switches (tests, A/B timing, ablation -- never needed for correct results; every setting
 * computes the same function within the per-kernel tolerances).  Each is an integer with a built-in
 * default; the table is initialised ONCE from the environment variables of the same names when the
 * library is loaded and is changed afterwards only through raft_set_option -- the launch path reads
 * an atomic, it never calls getenv:
 *   RAFT_CONV_TILE      "<code>" or "<npad>:<taps>:<code>,...": tile of the direct convolution kernels
 *                       (100 + 10*TH + TN: TH x 16-pixel x 64*TN-channel halo tiles, TH in {4,7,8}, TN in {1,2})
 *   RAFT_CONV_WINO      bit mask {1 convc2, 2 convf2, 4 conv, 8 fh1_mask0}: layers on the F(2x2,3x3) kernel (13)
 *   RAFT_CONV_WINO4     the same mask (bit 2 = convf2) for the F(4x4,3x3) kernel, preferred where its bit is set and the 6x6-tap weights
 *                       were supplied        (default by launch size: 0 for a single 448x512 pair, 8 = fh1_mask0 from 2 pairs, + 1 | 2 = convc2, convf2 from 3, + 4 = conv from 8)
 *   RAFT_WINO4_KS       1/2  F(4x4,3x3) kernel: 8 x 64-pixel workgroups / 4 x 64-pixel workgroups with K split between two
 *                            wave sets                                                        (default: by grid size)
 *   RAFT_SMALL_WINO     bit mask {1 conv, 2 gru_zr, 4 gru_q, 8 fh1} of the SmallUpdateBlock      (default 15)
 *   RAFT_GRU_WINO       bit mask {1 zr1, 2 q1, 4 zr2, 8 q2}: SepConvGRU layers on F(2,5)         (default 15)
 *   RAFT_GRU_WINO4      the same mask for F(4,5), preferred where both bits are set              (default 15)
 *   RAFT_WINO_TNW       1/2  32- or 64-channel workgroups of the Winograd kernels                (default: by grid size)
 *   RAFT_WINO_SB        0/1  pinned weight prefetch of the F(2x2,3x3) kernel                      (default: by grid size)
 *   RAFT_WINO1D_TM      1/2  half- / full-height F(2,5) tiles                                    (default: by grid size)
 *   RAFT_WINO_CK        1/2  16 or 32 channels per barrier (4: 64, split-K kernel only)          (default: by grid size)
 *   RAFT_WINO_KS        1/2  F(2x2,3x3) kernel: K split between two wave sets of a 512-thread workgroup (default: 2 for
 *                            launches of fewer wave-tasks than SIMDs, i.e. single pairs)
 *   RAFT_ENC_WINO       0/1  encoder ResBlock 3x3 layers on the F(2x2,3x3) kernel                 (default 1)
 *   RAFT_ENC_WINO4      bit mask {1 layer1, 2 layer2, 4 layer3}: stride-1 3x3 layers of those encoder stages on the
 *                       F(4x4,3x3) kernel where a transformed copy is present (block_w44)      (default: every layer whose launch has more than 256 workgroups)
 *   RAFT_LOOKUP_FUSED   0/1  prediction loops: lookup + convc1 as two kernels / fused (raft_lookup_convc1_f32)  (default 1)
 *   RAFT_MASK_FUSED     0/1  prediction loops: mask.2 + convex upsampling as two kernels / one (the mask is never stored) (default: 1 from 2 pairs at 448x512 on)
 *   RAFT_CONVC2_KS      1/2  convc2 on the F(4x4) kernel in the loops: 8-row workgroups / K-split 4-row workgroups   (default: by grid size)
 *   RAFT_CONVF2_KS      1/2  the same for convf2                             (default: K-split below 56 eight-row workgroups)
 *   RAFT_EVENT_FENCE    0/1  cross-stream events of a raft_loop_ctx without / with the system-scope fence of a default HIP event
 *                            (read when the context is created)                                    (default 1 since round 6; 0: the
 *                            events only order streams of one device, +0.4 .. 0.9 % on the three-stream loop, profiles/r10c_event_fence.txt)
 *   RAFT_CORR_XCD       0/1/n  volume build: plain (n, m, batch) tile grid / one region of the tile plane per XCD, walked in strips
 *                            of 2 (n >= 2: n) column tiles                                          (default 1)
 *   RAFT_CORR_POOL      0/1  volume build: pyramid level 1 as extra GEMM columns against the pooled fmap2 / pooled from the level-0
 *                            accumulators in the epilogue (2x2 averages by two DPP adds; 18 % fewer workgroups; the reference's own
 *                            summation order, corr.py:106-114).  1 needs even map sizes and an even number of 4x8 tiles per
 *                            row and column (448x512 and 1024x1024 frames have them), else 0 is used         (default 1)
 *   RAFT_ONDEMAND_BLOCK 0/1  on-demand lookup: wave per query / 4x8 query blocks on MFMA         (default 1)
 */
#ifndef RAFT_HIP_H_
#define RAFT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAFT_HIP_VERSION 222          /* 0.2.2: ABI stamp, checked by the Python binding -- bump on ANY struct / signature change */
#define RAFT_MAX_LEVELS 4

enum {
    RAFT_OK = 0,
    RAFT_E_NULL = -1,        /* a required pointer is NULL */
    RAFT_E_SHAPE = -2,       /* a dimension is non-positive or inconsistent */
    RAFT_E_UNSUPPORTED = -3, /* radius / channel count / kernel size not instantiated */
    RAFT_E_ALIGN = -4        /* a pointer or leading dimension is not 16-byte aligned */
};

int raft_version(void);
/* Human-readable message for a return code (RAFT_E_* or hipError_t). */
const char *raft_error_string(int rc);

/* Tuning switches (table above).  value: decimal text (RAFT_CONV_TILE: its rule list); "" = unset (built-in default);
 * NULL = back to the load-time (environment) state.  RAFT_E_UNSUPPORTED for an unknown name.  Thread-safe; takes effect
 * for launches enqueued after the call. */
int raft_set_option(const char *name, const char *value);
/* Launch-shape hint of the CALLING THREAD (thread-local, not process-global): its subsequent launches share the device with
 * n - 1 other independent launch sequences of about the same size -- the lanes of tf_raft_amd/model.py's pipelined forward,
 * several recurrent loops in flight on streams of their own.  The launchers' "does this grid fill the chip?" rules (Winograd
 * variant per layer, K-split / channel width of a workgroup, fused mask head) then count a grid n times, i.e. choose the
 * shapes of an n-times larger batch: less CU-time per launch instead of less latency.  Every shape computes the same function
 * within the per-kernel tolerances (as with the switches above).  n <= 1 restores the default.  Returns the previous value. */
int raft_set_thread_concurrency(int n);
/* Current value as text into buf ("" while unset). */
int raft_get_option(const char *name, char *buf, size_t len);

/* CRC-32C (Castagnoli, reflected 0x1EDC6F41) of `n` bytes, continuing from `crc` (0 to start).
 * Host-only.  The checksum of the TensorFlow tensor-bundle checkpoint files the reference
 * stores its weights in (README.md:66-96); used by tf_raft_amd/checkpoint.py. */
uint32_t raft_crc32c(uint32_t crc, const void *data, size_t n);

/* ------------------------------------------------------------------ correlation volume */

/* Pyramid geometry.  Level l holds, for each of the B*h*w query pixels, an (lh[l], lw[l]) map;
 * lh/lw follow tf.nn.avg_pool2d(2, 2, 'VALID') (floor).  A map is stored as 4x8 tiles of 32
 * floats (one 128-byte line each), tiles row-major, padded to whole tiles:
 *   map_floats(l) = ceil(lh/4) * ceil(lw/8) * 32,
 *   element (y, x) at ((y/4) * ceil(lw/8) + x/8) * 32 + (y%4) * 8 + x%8     (padding is zero),
 * so that the (2r+2)^2 lookup footprint pulls ~7 lines of a large map instead of ~13.
 * level_offsets[l] is the float offset of level l inside one allocation (level l = B*h*w maps
 * back to back), level_offsets[levels] the total float count.  Host-only helper (no GPU work).
 * reference corr.py:106-114. */
int raft_corr_pyramid_layout(int B, int h, int w, int levels,
                             int64_t *level_offsets /* [levels+1] */,
                             int *lh /* [levels] */, int *lw /* [levels] */);

/* Float count of the fmap2 feature-pyramid workspace raft_corr_build_f32 needs. */
int64_t raft_corr_build_workspace_floats(int B, int h, int w, int C, int levels);

/* All-pairs correlation volume + 4-level pyramid.
 * Replaces CorrBlock.__init__ / CorrBlock.correlation (reference corr.py:100-114, 154-162):
 *   corr[b, q, t] = <fmap1[b, q, :], fmap2[b, t, :]> / sqrt(C), then 3x avg_pool2d over t.
 * fmap1, fmap2: (B, h, w, C).  pyr: float[level_offsets[levels]]; level l is laid out
 * (B*h*w, map_floats(l)) in the tiled map layout above == the reference's corr_pyramid[l]
 * (B*h*w, lh[l], lw[l], 1) after un-tiling.
 * Levels > 0 are computed as <fmap1, avgpool_l(fmap2)> / sqrt(C) (average pooling over the
 * target dims commutes with the dot product); `workspace` holds the pooled fmap2 pyramid. */
int raft_corr_build_f32(const float *fmap1, const float *fmap2, int B, int h, int w, int C,
                        int levels, float *pyr, const int64_t *level_offsets,
                        float *workspace, void *stream);

/* Windowed bilinear pyramid lookup.  Replaces CorrBlock.retrieve + bilinear_sampler
 * (reference corr.py:116-152, 28-69), including its exact semantics: clamp, ceil/floor
 * weights (integer or out-of-range coordinate => 0), window axis 0 offsets x.
 * coords: (B, h, w, 2) xy.  out: (B, h, w, ld_out) with channel = lvl*(2r+1)^2 + a*(2r+1) + b
 * in the first levels*(2r+1)^2 channels; channels beyond that are left untouched.
 * radius 3 and 4 are instantiated. */
int raft_corr_lookup_f32(const float *pyr, const int64_t *level_offsets, const float *coords,
                         int B, int h, int w, int levels, int radius,
                         float *out, int ld_out, void *stream);

/* Same lookup without a stored volume ("alternate" correlation; no reference code --
 * the reference README.md:109 notes its absence): correlations of the (2r+2)^2 footprint are
 * computed on demand from fmap1 and the pooled fmap2 pyramid held in `fmap2_pyr`
 * (the workspace layout of raft_corr_build_f32, filled by raft_fmap_pyramid_f32). */
int raft_fmap_pyramid_f32(const float *fmap2, int B, int h, int w, int C, int levels,
                          float *fmap2_pyr, void *stream);
int raft_corr_lookup_ondemand_f32(const float *fmap1, const float *fmap2_pyr,
                                  const float *coords, int B, int h, int w, int C,
                                  int levels, int radius, float *out, int ld_out,
                                  void *stream);

/* bilinear_sampler (reference corr.py:28-69) as a standalone op.
 * image: (n, h, w[, 1]); coords: (n, kh, kw, 2) xy; out: (n, kh, kw[, 1]). */
int raft_bilinear_sampler_f32(const float *image, const float *coords, int64_t n, int h, int w,
                              int kh, int kw, float *out, void *stream);

/* coords_grid (reference corr.py:72-90): coords[b, y, x] = (x, y). */
int raft_coords_grid_f32(float *coords, int B, int h, int w, void *stream);

/* ------------------------------------------------------------------ upsampling */

/* RAFT.upsample_flow (reference model.py:39-66): softmax over the 9 taps of
 * mask[b, y, x, (i*8 + j)*9 + k], 3x3 zero-padded neighbourhood of 8*flow, depth_to_space(8).
 * flow: (B, h, w, 2); mask: (B, h, w, 576); out: (B, 8h, 8w, 2). */
int raft_upsample_convex_f32(const float *flow, const float *mask, int B, int h, int w,
                             float *out, void *stream);

/* upflow8 (reference corr.py:93-96): 8 * tf.image.resize(flow, (8h, 8w), 'bilinear')
 * with TF2 half-pixel centres.  flow: (B, h, w, 2); out: (B, 8h, 8w, 2). */
int raft_upflow8_f32(const float *flow, int B, int h, int w, float *out, void *stream);

/* Measurement utility (no reference counterpart): 16-byte-per-lane streaming copy of n floats
 * (n % 4 == 0, 16-byte aligned pointers).  bench.py times it to state the HBM copy bandwidth of
 * the box it runs on -- the "measured roofline" the lookup / build / upsample kernels are quoted
 * against next to the 8 TB/s datasheet figure. */
int raft_stream_copy_f32(const float *src, float *dst, int64_t n, void *stream);

/* tf.image.resize_with_crop_or_pad on NHWC images (reference tf_raft/datasets/dataset.py:323-334 CropOrPadder,
 * tf_raft/training.py:72-84 VisFlowCallback): src (N, Hs, Ws, C) -> dst (N, Ht, Wt, C), both contiguous.  Per axis, with
 * d = target - source (floor division): the source window starts at max(-d // 2, 0), lands at max(d // 2, 0) in the target
 * and is min(source, target) long, so an odd surplus goes to the bottom / right; everything outside it is zero in the
 * input's own scale.  Every element of dst is written exactly once (no memset needed).  Any sizes >= 1, any C >= 1 and any
 * alignment are accepted; destination rows that are whole 16-byte chunks of a 16-byte aligned dst (the model's targets
 * always are) take the vectorised path.  W * C of either side must fit an int.
 *   _f32    : float -> float (float images, ground-truth flow, predictions: N = iterations x batch in one launch)
 *   _u8_f32 : uint8 -> float (uint8 frames: the cast and the window in one pass)
 *   _u8     : uint8 -> uint8 (validity masks; bool tensors are bytes) */
int raft_crop_or_pad_f32(const float *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream);
int raft_crop_or_pad_u8_f32(const uint8_t *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream);
int raft_crop_or_pad_u8(const uint8_t *src, uint8_t *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, void *stream);

/* Separable resize of NHWC images by per-axis tap tables: src (N, Hs, Ws, C) uint8 or float -> dst (N, Ht, Wt, C) float, both
 * contiguous:
 *     dst[n, y, x, c] = chan_scale[c] * sum_b x_weights[x][b] * sum_a y_weights[y][a] * src[n, y_first[y] + a, x_first[x] + b, c]
 * An axis of n_out outputs is described by three DEVICE arrays: first[n_out] (first source index), count[n_out] (taps,
 * 1 <= count <= max_taps) and weights[n_out * max_taps] (row i holds output i's count[i] weights).  The tables of the project
 * are bilinear with half-pixel centres, optionally widened to an antialiasing triangle on a shrinking axis, derived in float64
 * on the host (tf_raft_amd/image_ops.py resize_taps); any table whose first indices do not decrease and
 * advance by at most ceil(n_in / n_out) + 1 per output is taken.  Indices are clamped to the source whatever a table holds.
 * chan_scale: C device floats (a flow resized from (Hs, Ws) to (Ht, Wt) has its u scaled by Wt / Ws and its v by Ht / Hs), or
 * NULL for none.  One launch over all N images on `stream`, no intermediate, nothing synchronised or copied back.  Any sizes
 * >= 1, any C >= 1 and any alignment are accepted; W * C of either side must fit an int; max_taps up to 64 per axis (shrink
 * ratios up to 31), and (x_max_taps + 2) * C + 30 must not exceed 2048: RAFT_E_SHAPE otherwise. */
int raft_resize_f32(const float *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C,
                    const int *y_first, const int *y_count, const float *y_weights, int y_max_taps,
                    const int *x_first, const int *x_count, const float *x_weights, int x_max_taps,
                    const float *chan_scale, void *stream);
int raft_resize_u8_f32(const uint8_t *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C,
                       const int *y_first, const int *y_count, const float *y_weights, int y_max_taps,
                       const int *x_first, const int *x_count, const float *x_weights, int x_max_taps,
                       const float *chan_scale, void *stream);

/* Tiled inference (no reference counterpart): a frame larger than the model's size is covered by a product
 * grid of ny x nx overlapping model-sized tiles, each tile is predicted on its own, and the predictions are cross-faded where
 * tiles overlap.  The origins of the tiles in the frame (tf_raft_amd/image_ops.py tile_origins; negative where a frame shorter
 * than the tile is centred in it by the crop-or-pad rule) travel by value: */
#define RAFT_TILE_MAX_PER_AXIS 32
#define RAFT_TILE_MAX_TAPS 4
typedef struct RaftTileOrigins {
    int32_t ny, nx;                          /* tiles per axis, 1 .. RAFT_TILE_MAX_PER_AXIS */
    int32_t oy[RAFT_TILE_MAX_PER_AXIS];      /* frame row of tile row 0, the first ny are read */
    int32_t ox[RAFT_TILE_MAX_PER_AXIS];      /* frame column of tile column 0, the first nx are read */
} RaftTileOrigins;

/* The gather in front of the model: src (N, Hs, Ws, C) uint8 or float -> dst (N * ny * nx, Ht, Wt, C) float, both contiguous,
 * tile (n * ny + ky) * nx + kx holding dst[y, x] = src[n, oy[ky] + y, ox[kx] + x] and zero outside the frame (uint8 is cast in
 * the same pass).  Every element of dst is written exactly once, in one launch on `stream`.  Any sizes >= 1, any C >= 1 and any
 * alignment are accepted, as by raft_crop_or_pad_*; W * C of either side must fit an int.  RAFT_E_SHAPE for a non-positive
 * size, for ny or nx outside 1 .. RAFT_TILE_MAX_PER_AXIS and for a tile that lies wholly outside the frame; RAFT_E_NULL for a
 * null pointer.  All checks precede the launch. */
int raft_tile_gather_f32(const float *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, RaftTileOrigins origins,
                         void *stream);
int raft_tile_gather_u8_f32(const uint8_t *src, float *dst, int N, int Hs, int Ws, int Ht, int Wt, int C, RaftTileOrigins origins,
                            void *stream);

/* The blend behind the model: tiles (M, N * ny * nx, Ht, Wt, 2) -> dst (M, N, H, W, 2), both contiguous floats, M the
 * flattened leading axes (the iterations of a call):
 *     dst[m, n, y, x] = sum_b x_weights[x][b] * sum_a y_weights[y][a] * tiles[m, (n * ny + ky) * nx + kx, y - oy[ky], x - ox[kx]]
 * with ky = y_first[y] + a and kx = x_first[x] + b, the sums in this order.  An axis of L frame coordinates is described by
 * three DEVICE arrays, as an axis of raft_resize_*: first[L] (first tile index), count[L] (tiles covering the coordinate,
 * 1 <= count <= max_taps <= RAFT_TILE_MAX_TAPS) and weights[L * max_taps] (the normalised tent weights of those tiles, derived
 * in float64 on the host and rounded once: tf_raft_amd/image_ops.py tile_taps).  Flow vectors are not scaled.  One launch on
 * `stream`; no atomics, no memset, no intermediate, nothing synchronised; every element of dst is written exactly once, and
 * element offsets are 64-bit.  Tile indices and tile coordinates are clamped into the tiles whatever the tables hold.  tiles
 * and dst must be 8-byte aligned (RAFT_E_ALIGN: they are read and written as float2).  RAFT_E_SHAPE for a non-positive size,
 * ny / nx / max_taps out of range, or Ht * Wt beyond an int; RAFT_E_NULL for a null pointer.  All checks precede the launch. */
int raft_tile_blend_f32(const float *tiles, float *dst, int64_t M, int N, int H, int W, int Ht, int Wt, RaftTileOrigins origins,
                        const int *y_first, const int *y_count, const float *y_weights, int y_max_taps,
                        const int *x_first, const int *x_count, const float *x_weights, int x_max_taps, void *stream);

/* Flow colour coding (reference tf_raft/datasets/flow_viz.py:109-132 flow_to_image, the Middlebury colour wheel): a flow
 * (N, Hs, Ws, 2) seen through the crop-or-pad window above at a destination size (Ht, Wt) -> pictures (N, Ht, Wt, 3) uint8,
 * in two launches on `stream` with no atomics, no memset and nothing synchronised.  Destination pixels outside the window are
 * zero flow (white); source pixels outside it count for nothing.  clip >= 0: np.clip(flow, 0, clip) first, as the reference
 * does it (negative components become 0); any negative clip: none.
 *   raft_flow_rad_max_f32: partial maxima of sqrt(u*u + v*v) in float32, each product and the sum rounded on its own, into
 *     partial[raft_flow_to_image_workspace_floats(N)] (every element is written; image n's maximum is the largest of its
 *     raft_flow_to_image_workspace_floats(1) consecutive elements -- exact in any order, so bit-identical to NumPy's).
 *   raft_flow_to_image_u8: the picture.  Each image is normalised by its own maximum from `partial`; fixed_rad_max > 0
 *     replaces it for every image (partial may then be NULL), and vectors beyond it take the reference's darkened
 *     out-of-range branch.  bgr != 0 stores the channels in reverse.  float32 up to the wheel position, float64 from there on,
 *     as NumPy 2 types the reference's expressions; atan2 is computed in double and rounded once.  A NaN
 *     or infinite flow is outside the contract; it never reads outside the 55-entry wheel.
 * flow must be 8-byte aligned (RAFT_E_ALIGN); image may have any alignment.  Ws * 2, Wt * 3 and Ht * Wt must fit an int
 * (RAFT_E_SHAPE, like non-positive sizes); RAFT_E_NULL for a null pointer.  All checks precede any launch. */
int64_t raft_flow_to_image_workspace_floats(int N);
int raft_flow_rad_max_f32(const float *flow, float *partial, int N, int Hs, int Ws, int Ht, int Wt, float clip, void *stream);
int raft_flow_to_image_u8(const float *flow, const float *partial, uint8_t *image, int N, int Hs, int Ws, int Ht, int Wt,
                          float clip, int bgr, float fixed_rad_max, void *stream);

/* Where a flow can be trusted (no reference counterpart): the backward warp of an image by a flow and the
 * forward-backward consistency test of two flows.  Flows are (N, H, W, 2) floats, [..., 0] = u along x, [..., 1] = v along y.
 * For the pixel at integer (x, y) with vector (u, v) the sample position is sx = float(x) + u, sy = float(y) + v, ONE float32
 * addition each; the pixel is IN FRAME iff 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails the comparison).  A map g is
 * sampled there bilinearly: x0 = floor(sx), x1 = min(x0 + 1, W - 1), a = sx - x0, likewise y0, y1, b, and
 *     (1 - b) * ((1 - a) * g[y0, x0] + a * g[y0, x1]) + b * ((1 - a) * g[y1, x0] + a * g[y1, x1])
 * every operation rounded on its own.  This is ordinary bilinear interpolation, not the reference's bilinear_sampler
 * (corr.py:28-69: its ceil / floor weights are both 0 at an integer coordinate).
 *   raft_warp_f32 / raft_warp_u8_f32: dst[n, y, x, c] = src[n, :, :, c] sampled at the pixel's sample position, 0.0f in every
 *     channel of a pixel out of frame; src (N, H, W, C) float or uint8 (cast in the same pass), C >= 1, dst (N, H, W, C) float.
 *     inside: NULL, or uint8 (N, H, W), 1 where in frame.  warp(image2, flow_forward) reconstructs frame 1 from frame 2.
 *   raft_flow_consistency_f32: with s = flow_b sampled at the pixel's sample position under flow_a (both components),
 *         occluded_a = !(in frame && |flow_a + s|^2 <= alpha * (|flow_a|^2 + |s|^2) + beta)
 *     (Meister et al. 2018, UnFlow: alpha 0.01, beta 0.5), so a non-finite vector marks its pixel.  occluded_b: NULL, or the
 *     same test with the roles of the flows swapped, produced by the SAME launch as a second grid slice.  Masks are uint8
 *     (N, H, W), 1 = occluded.
 * One launch on `stream` each, no atomics, no memset, every output element written exactly once; tap indices are clamped into
 * the frame whatever a flow holds.  RAFT_E_NULL for a NULL required pointer; RAFT_E_SHAPE for a non-positive size, a negative
 * or non-finite alpha or beta, W * C beyond an int, or N * H * W * max(C, 2) of 2^31 elements or more; RAFT_E_ALIGN for a flow
 * that is not 8-byte aligned (flows are read as float2).  All checks precede the launch. */
int raft_warp_f32(const float *src, const float *flow, float *dst, uint8_t *inside, int N, int H, int W, int C, void *stream);
int raft_warp_u8_f32(const uint8_t *src, const float *flow, float *dst, uint8_t *inside, int N, int H, int W, int C, void *stream);
int raft_flow_consistency_f32(const float *flow_a, const float *flow_b, uint8_t *occluded_a, uint8_t *occluded_b, int N, int H, int W,
                              float alpha, float beta, void *stream);

/* The consistency test inside a bidirectional training step: `flows` (2N, H, W, 2) holds N forward flows
 * and, behind them, the N backward flows of the same pairs.  Slice s < N is tested against slice s + N, slice s >= N against
 * slice s - N, by the test of raft_flow_consistency_f32 (one device function serves both entries), and
 *     visible[s, y, x] = (mask == NULL || mask[s, y, x] != 0) && (!apply || !occluded) ? 1 : 0
 * mask: NULL (all ones) or uint8 (2N, H, W); visible: uint8 (2N, H, W), or NULL when only the count is wanted; the two must not
 * overlap.  occluded_fraction[0] = float(count / (2 * N * H * W)), count the number of occluded pixels of all 2N slices whatever
 * `apply` and `mask` are; the division is done in double and rounded once.  Deterministic (no atomics, no memset): float64
 * partial records in `workspace` (raft_flow_visibility_workspace_doubles() doubles, 8-byte aligned), summed in index order by a
 * one-workgroup launch, so two launches on `stream`.  Errors, in this order: RAFT_E_NULL for a NULL flows, occluded_fraction or
 * workspace; RAFT_E_SHAPE for a non-positive size, 2N * H * W * 2 of 2^31 elements or more, a negative or non-finite alpha or
 * beta, `apply` other than 0 or 1; RAFT_E_ALIGN for flows or a workspace that is not 8-byte aligned.  All checks precede the
 * first launch. */
int64_t raft_flow_visibility_workspace_doubles(void);
int raft_flow_visibility_f32(const float *flows, const uint8_t *mask, uint8_t *visible, float *occluded_fraction, int N, int H, int W,
                             float alpha, float beta, int apply, double *workspace, void *stream);

/* The range map of a flow (Wang et al. 2018): a forward splat of the flow itself, the second occlusion test.
 * The source pixel at integer (x, y) with vector (u, v) has the sample position sx = float(x) + u, sy = float(y) + v of above.  It
 * contributes iff -1 < sx < float(W) and -1 < sy < float(H), compared on the floats (a NaN, an infinity or 1e30 fails).  Then
 * x0 = floor(sx), a = sx - x0 in float32, qa = (int)rintf(a * 4096.0f) in 0 .. 4096, likewise y0, b, qb, and the corner
 * (x0 + dx, y0 + dy) receives the integer weight (dx ? qa : 4096 - qa) * (dy ? qb : 4096 - qb); the four sum to exactly 2^24.  A
 * corner outside the frame or of weight 0 receives nothing.  acc[n, cy, cx] is the uint64 sum of the weights that land there:
 * exact in any arrival order, so every entry below repeats bit for bit.
 *   raft_flow_range_map_f32: range[n, y, x] = float(double(acc) * 2^-24), (N, H, W) floats; 1.0 under zero flow.
 *   raft_flow_range_occlusion_f32: with acc_ba the sums of flow_b (it lives on frame B's grid and lands on frame A's) and
 *         T = (uint64)ceil(double(threshold) * 2^24), compared on the integers,
 *         occluded_a = acc_ba < T || !(flow_a's pixel IN FRAME)
 *     so a mask means what raft_flow_consistency_f32's means: 1 = occluded or out of frame.  occluded_b: NULL (then only flow_b
 *     is splatted), or the same with the roles swapped.  Masks are uint8 (N, H, W).
 *   raft_flow_range_visibility_f32: raft_flow_visibility_f32 with this test: `flows` (2N, H, W, 2), slice s against the sums of
 *     slice s + N (s < N) or s - N; mask, visible, occluded_fraction and `apply` as there.  `records`:
 *     raft_flow_visibility_workspace_doubles() doubles.
 * `workspace` holds the sums: raft_flow_range_workspace_bytes(slices, H, W) bytes, 8-byte aligned, with slices = N for the map
 * and for occluded_b == NULL, else 2N (0: the sizes are refused).  Three phases on `stream`: the sums are zeroed, one thread per
 * source pixel adds up to four weights with 64-bit integer atomics, one thread per destination pixel writes the result (the
 * visibility entry adds its one-workgroup sum of the records).  Errors, in this order: RAFT_E_NULL for a NULL required pointer;
 * RAFT_E_SHAPE for a non-positive size, N * H * W * 2 (2N for the visibility entry) of 2^31 elements or more, H * W above 2^28,
 * a threshold outside (0, 1] or NaN, `apply` other than 0 or 1; RAFT_E_ALIGN for a flow, a workspace or records that are not
 * 8-byte aligned.  All checks precede the first launch. */
int64_t raft_flow_range_workspace_bytes(int slices, int H, int W);
int raft_flow_range_map_f32(const float *flow, float *range, int N, int H, int W, void *workspace, void *stream);
int raft_flow_range_occlusion_f32(const float *flow_a, const float *flow_b, uint8_t *occluded_a, uint8_t *occluded_b, int N, int H, int W,
                                  float threshold, void *workspace, void *stream);
int raft_flow_range_visibility_f32(const float *flows, const uint8_t *mask, uint8_t *visible, float *occluded_fraction, int N, int H,
                                   int W, float threshold, int apply, void *workspace, double *records, void *stream);

/* The forward splat of FRAMES along a flow, and the frame in between two frames: the accumulator above
 * carried over to colour.  Frames are (N, H, W, C) with C in 1 .. 4, uint8 or float32 on 0 .. 255; flows (N, H, W, 2) float32.
 * The source pixel at integer (x, y) of slice n with vector (u, v) and time t lands on sx = float(x) + t * u, sy = float(y) + t * v
 * (one float32 multiplication, then one float32 addition, never fused).  It contributes iff -1 < sx < float(W) and
 * -1 < sy < float(H) (a NaN, an infinity or 1e30 fails) and, with a non-NULL uint8 mask (N, H, W), mask[n, y, x] != 0.  The
 * corners and their integer weights w are the range map's.  Every destination pixel holds C + 1 uint64 sums: W += w and
 * S_c += w * q_c, with q_c the byte of a uint8 frame or (int)rintf(fminf(fmaxf(value, 0), 255) * 256) of a float32 one (a NaN
 * gives 0).  Integer sums: every entry repeats bit for bit, whatever the order of the adds.
 *   raft_splat_frames_*: dst[n, y, x, c] = float(double(S_c) / double(W)) (times 1 / 256 for float32 frames, before the cast), 0
 *     where W == 0; weight (N, H, W), if not NULL, = float(double(W) * 2^-24): at t = 1 the flow's range map.  t must be finite.
 *   raft_interpolate_frames_*: image1 is splatted to t along flow_forward (slices 0 .. N - 1 of the sums) and image2 to
 *     s = 1.0f - t along flow_backward (slices N .. 2N - 1) by ONE scatter launch; then per pixel, in float64 and never fused,
 *     td = t, a = (1 - td) * W1, b = td * W2, den = a + b and
 *         den > 0:   out_c = ((1 - td) * S1_c + td * S2_c) / den
 *         otherwise: out_c = (1 - td) * q1_c + td * q2_c on the pixel's own two quantised values, a HOLE: holes[n, y, x] = 1
 *     (holes: uint8 (N, H, W), 0 elsewhere; may be NULL).  Float32 frames are multiplied by 1 / 256 at the end; a float32 dst
 *     is the cast of out_c, a uint8 dst is (uint8)fmin(rint(out_c), 255).  0 <= t <= 1; mask1 / mask2 may each be NULL.
 * `workspace` holds the sums: raft_frame_splat_workspace_bytes(slices, H, W, C) = slices * H * W * (C + 1) * 8 bytes, 8-byte
 * aligned, zeroed by the entry itself, with slices = N for a splat and 2N for an interpolation (0: the sizes are refused).
 * Errors, in this order: RAFT_E_NULL for a NULL required pointer; RAFT_E_SHAPE for a non-positive size, C outside 1 .. 4,
 * H * W above 2^24, slices * H * W * 4 of 2^31 or more, a t that is not finite (splat) or outside [0, 1] or NaN (interpolate);
 * RAFT_E_ALIGN for a flow or a workspace that is not 8-byte aligned.  All checks precede the first launch. */
int64_t raft_frame_splat_workspace_bytes(int slices, int H, int W, int C);
int raft_splat_frames_f32(const float *src, const float *flow, const uint8_t *mask, float t, float *dst, float *weight, int N, int H,
                          int W, int C, void *workspace, void *stream);
int raft_splat_frames_u8_f32(const uint8_t *src, const float *flow, const uint8_t *mask, float t, float *dst, float *weight, int N, int H,
                             int W, int C, void *workspace, void *stream);
int raft_interpolate_frames_f32(const float *image1, const float *image2, const float *flow_forward, const float *flow_backward,
                                const uint8_t *mask1, const uint8_t *mask2, float t, float *dst, uint8_t *holes, int N, int H, int W, int C,
                                void *workspace, void *stream);
int raft_interpolate_frames_u8_f32(const uint8_t *image1, const uint8_t *image2, const float *flow_forward, const float *flow_backward,
                                   const uint8_t *mask1, const uint8_t *mask2, float t, float *dst, uint8_t *holes, int N, int H, int W,
                                   int C, void *workspace, void *stream);
int raft_interpolate_frames_u8(const uint8_t *image1, const uint8_t *image2, const float *flow_forward, const float *flow_backward,
                               const uint8_t *mask1, const uint8_t *mask2, float t, uint8_t *dst, uint8_t *holes, int N, int H, int W,
                               int C, void *workspace, void *stream);

/* Following points through a video: the flows of S consecutive frame pairs of N videos chained at
 * sub-pixel positions by ONE launch.  pos_in (N, P, 2) floats, (x, y) in pixels of the frames; lost_in uint8 (N, P) or NULL (all
 * 0); flow_forward (S, N, H, W, 2), the flows frame t0 + s -> t0 + s + 1; flow_backward the same shape for t0 + s + 1 -> t0 + s,
 * or NULL (no consistency test); pos_out (S, N, P, 2) and lost_out uint8 (S, N, P): the state after every step; start int32
 * (N, P) or NULL: a point with start > t0 + s is copied through step s untouched (a query point given at a later frame).
 * Codes in lost: 0 = tracked, 1 = left the frame, 2 = failed the consistency test (3 = an empty slot comes in from
 * raft_detect_points below and is never produced here); any nonzero code is sticky, the point keeps
 * the position it was last tracked at and its code, bit for bit.  One step of a tracked point at (x, y), with the sample of the
 * warp entries above (in frame iff 0 <= sx <= W - 1 and 0 <= sy <= H - 1, a NaN fails; bilinear, every operation rounded on its
 * own):
 *     (x, y) out of frame: code 1.  f = flow_forward[s, n] sampled at (x, y); qx = x + f.x, qy = y + f.y, ONE float32 addition
 *     each; (qx, qy) out of frame: code 1.  With a flow_backward, b = flow_backward[s, n] sampled at (qx, qy), and
 *     !(|f + b|^2 <= alpha * (|f|^2 + |b|^2) + beta), raft_flow_consistency_f32's comparison in its operation order (one device
 *     function serves both): code 2.  Otherwise the point moves to (qx, qy).
 * One thread per point and no atomics: a thread reads its own point first and touches no other, so pos_out + (S - 1) * N * P * 2
 * == pos_in and lost_out + (S - 1) * N * P == lost_in are allowed (the in-place streaming step with S = 1); no other overlap is.
 * Errors, in this order: RAFT_E_NULL for a NULL pos_in, flow_forward, pos_out or lost_out; RAFT_E_SHAPE for a non-positive size,
 * a negative t0, S * N * H * W * 2 or S * N * P * 2 of 2^31 elements or more, a negative or non-finite alpha or beta (checked
 * with and without a flow_backward); RAFT_E_ALIGN for a pos_in, pos_out or flow that is not 8-byte aligned (read and written as
 * float2).  All checks precede the launch. */
int raft_track_points_f32(const float *pos_in, const uint8_t *lost_in, const int32_t *start, int t0, const float *flow_forward,
                          const float *flow_backward, float *pos_out, uint8_t *lost_out, int S, int N, int64_t P, int H, int W,
                          float alpha, float beta, void *stream);

/* The camera's motion from a flow (csrc/flow_motion.hip has the definition in the operation order of the kernels; DESIGN.md
 * section 27).  raft_flow_fit_motion_f32 fits, per slice of flow (N, H, W, 2), the displacement field d(X, Y) = L (X, Y) + t in
 * the centred coordinates X = x - (W - 1) / 2, Y = y - (H - 1) / 2 to the USED vectors by iteratively reweighted least squares:
 * a pixel is used iff both components of its vector are finite and mask == NULL, or mask_invert == 0 and its byte of mask (uint8
 * (N, H, W)) is nonzero, or mask_invert == 1 and the byte is zero (an occluded_* mask goes in as it is).  model: 0 translation,
 * 1 similarity (rotation, uniform zoom, shift), 2 affine.  Solve 1 weights every used pixel 1; solve k > 1 weights it
 * 1 / (1 + r2 / scale^2), r2 its squared residual under the float64 estimate of solve k - 1 (Cauchy; evaluated with one division
 * as s2 / (s2 + r2), s2 = (double)scale * (double)scale); iterations in 1 .. 32, scale in pixels, positive and finite.  All arithmetic behind the load is float64, never fused; sums are per-thread float64, reduced
 * through records that belong to one slice each and added in a fixed order: the same input gives the same bits, and a slice's
 * result does not depend on the other slices.
 *   motion (N, 2, 3): the map p2 = M (x, y, 1) from frame 1 to frame 2 in plain pixel coordinates, M[:, :2] = I + L,
 *     M[:, 2] = t - L c with c the frame centre, formed in float64, each entry rounded once; zero flow gives the identity exactly.
 *   stats (N, 4): used / (H W); the inlier share Sw / used and the weighted RMS residual sqrt(Sw_r2 / Sw), both with the Cauchy
 *     weights under the FINAL estimate; the status.  The first three are 0 where no pixel is used.
 *   status: 0 the model asked for was fitted; 1 its normal equations had no rank (affine: D <= 1e-12 max(cxx, cyy)^2; similarity:
 *     cxx + cyy <= 0; or a NaN), L = 0 and t = the weighted mean vector; 2 nothing to fit (!(Sw > 0)), L = 0 and t = 0.  0 and 1
 *     refer to the last solve; 2 stays once it is met.
 * workspace: raft_flow_motion_workspace_doubles(N, H, W) doubles (0: the sizes are refused), 8-byte aligned; it need not be
 * cleared.  2 * iterations + 2 launches on `stream`, no atomics, no memset, no host synchronisation.
 * Errors, in this order: RAFT_E_NULL for a NULL flow, motion, stats or workspace; RAFT_E_SHAPE for a non-positive size,
 * N * H * W * 2 of 2^31 or more, N above 65535, a model outside 0 .. 2, iterations outside 1 .. 32, a mask_invert other than 0 or
 * 1, a scale that is not positive and finite; RAFT_E_ALIGN for a flow or a workspace that is not 8-byte aligned.  All checks
 * precede the first launch.
 *
 * raft_flow_residual_f32: residual[n, y, x] = flow[n, y, x] - g with g = (((double)m00 * x + (double)m01 * y) + (double)m02) - x
 * (likewise for the second component with row 1 and y), evaluated in float64, never fused, each component rounded to float32
 * once; moving (uint8 (N, H, W)) = 1 iff !(rx^2 + ry^2 <= threshold^2) on the float64 residual, so a vector that is not finite
 * is marked.  residual or moving may be NULL, not both.  One launch, every output element written once.  Errors: RAFT_E_NULL
 * (flow, motion, or both outputs NULL); RAFT_E_SHAPE (a non-positive size, N * H * W * 2 of 2^31 or more, a threshold that is
 * negative or not finite, checked with and without `moving`); RAFT_E_ALIGN (a flow or a residual that is not 8-byte aligned).
 * raft_motion_flow_f32: flow[n, y, x] = g, the dense flow of the motions, each component rounded once; the same errors. */
int64_t raft_flow_motion_workspace_doubles(int N, int H, int W);
int raft_flow_fit_motion_f32(const float *flow, const uint8_t *mask, int mask_invert, float *motion, float *stats,
                             int N, int H, int W, int model, int iterations, float scale, double *workspace, void *stream);
int raft_flow_residual_f32(const float *flow, const float *motion, float *residual, uint8_t *moving,
                           int N, int H, int W, float threshold, void *stream);
int raft_motion_flow_f32(const float *motion, float *flow, int N, int H, int W, void *stream);

/* Motion-compensated temporal filtering: a centre frame fused with K neighbours that are aligned onto it
 * along flows and averaged robustly, in ONE launch.  center (N, H, W, C), uint8 or float32 on 0 .. 255, C in 1 .. 4.  Neighbour k,
 * k = 0 .. K - 1 with K in 1 .. 16, is the (N, H, W, C) block of the centre's type at neighbours + index[k] * N * H * W * C
 * elements; index is a HOST array of K entries >= 0, read at call time and passed by value with the launch (NULL: 0 .. K - 1); an
 * entry may repeat, so a window frames[t - r : t + r + 1] of a device video serves as it lies, with no copies.  vectors
 * (K, N, H, W, 2) float32: with absolute == 0 the flow centre -> neighbour k, the sample position of the pixel at integer (x, y)
 * being sx = float(x) + u, sy = float(y) + v as for raft_warp_f32; with absolute == 1 the sample position (sx, sy) itself, so
 * raft_track_points_f32's positions go in as they are.  skip: NULL, or uint8 (K, N, H, W), nonzero = neighbour k is not used at this
 * pixel (an occluded_* mask or raft_track_points_f32's lost codes go in unchanged).  sigma (on the 0 .. 255 scale) and
 * center_weight are positive and finite, and s2 = sigma * sigma is positive and finite as a float32; patch_radius r in 0 .. 3.
 * Per pixel p = (x, y) of slice n and neighbour k, in float32, every product, sum and quotient rounded on its own, never fused:
 *     vis_k(p) = the sample position is IN FRAME (0 <= sx <= W - 1 and 0 <= sy <= H - 1, a NaN fails) && (skip == NULL ||
 *                skip[k, n, p] == 0)
 *     c_k[ch]  = neighbour k's channel ch sampled there by the bilinear rule of raft_warp_f32 (uint8 taps converted to float
 *                first; out of frame the taps are those of position (0, 0), the value is never weighted)
 *     q_k(p)   = sum over ch = 0 .. C - 1, in this order, of d * d with d = center[ch] - c_k[ch];  0.f where !vis_k(p)
 *     D, cnt   = the sum of q_k(p') and the count of p' over the window p' = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r
 *                inner, over the p' that are in the frame and have vis_k(p')  (q_k is +0 or larger: the kernel adds 0.f for the
 *                others, which changes no bit)
 *     m        = D / (float)(cnt * C)
 *     w_k(p)   = vis_k(p) ? s2 / (s2 + m) : 0.f                                   (Cauchy, one division, as raft_flow_fit_motion_f32)
 *   num[ch] = center_weight * center[ch], den = center_weight;  for k = 0 .. K - 1 in this order: num[ch] = num[ch] + w_k * c_k[ch],
 *   den = den + w_k;  then dst[n, y, x, ch] = num[ch] / den and weight[n, y, x] = den.
 * dst (N, H, W, C): float32 (_f32: float32 frames; _u8_f32: uint8 frames) or uint8 (_u8: uint8 frames, rintf -- half to even --
 * then clamped to 0 .. 255); weight: NULL, or float32 (N, H, W).  A pixel with no visible neighbour gets (center_weight *
 * center) / center_weight and the weight center_weight.  No transcendental function appears, so the result equals its float32
 * NumPy restatement bit for bit and repeats bit for bit.  One launch on `stream`: no workspace, no atomics, no memset, every
 * output element written exactly once; a workgroup stages (q_k, vis_k) of its 32 x 8 tile and a ring of r pixels in LDS once per
 * neighbour.  dst and weight may overlap no input and not each other (windows read the neighbours' pixels).
 * Errors, in this order: RAFT_E_NULL for a NULL center, neighbours, vectors or dst; RAFT_E_SHAPE for K outside 1 .. 16, a
 * non-positive size, C outside 1 .. 4, patch_radius outside 0 .. 3, absolute other than 0 or 1, N * H * W above 2^26, a sigma,
 * sigma * sigma or center_weight that is not positive and finite, a negative index (or one beyond 2^60 elements); RAFT_E_ALIGN for
 * vectors that are not 8-byte aligned or float32 frames, dst or weight that are not 4-byte aligned (uint8 frames may lie at any
 * address); RAFT_E_SHAPE for an output that overlaps an input or the other output.  All checks precede the launch. */
int raft_fuse_frames_f32(const float *center, const float *neighbours, const int64_t *index, const float *vectors, const uint8_t *skip,
                         int absolute, float sigma, float center_weight, int patch_radius, float *dst, float *weight, int K, int N,
                         int H, int W, int C, void *stream);
int raft_fuse_frames_u8_f32(const uint8_t *center, const uint8_t *neighbours, const int64_t *index, const float *vectors,
                            const uint8_t *skip, int absolute, float sigma, float center_weight, int patch_radius, float *dst,
                            float *weight, int K, int N, int H, int W, int C, void *stream);
int raft_fuse_frames_u8(const uint8_t *center, const uint8_t *neighbours, const int64_t *index, const float *vectors,
                        const uint8_t *skip, int absolute, float sigma, float center_weight, int patch_radius, uint8_t *dst,
                        float *weight, int K, int N, int H, int W, int C, void *stream);

/* Corner detection and re-seeding for the point tracker (csrc/point_detect.hip): "good features to track"
 * on the device.  frames (N, H, W, C), C in {1, 3}, uint8 or float32 on 0 .. 255 (float32 values are used as they are).
 *
 * The score, per pixel, all float32, every operation rounded on its own, never fused, in exactly this order:
 *     g        = C == 1 ? the value : (0.299f * R + 0.587f * G) + 0.114f * B                    (uint8 converted to float first)
 *     gx       = ((g[y-1][x+1] - g[y-1][x-1]) + 2.f * (g[y][x+1] - g[y][x-1])) + (g[y+1][x+1] - g[y+1][x-1])      (Sobel 3 x 3)
 *     gy       = ((g[y+1][x-1] - g[y-1][x-1]) + 2.f * (g[y+1][x] - g[y-1][x])) + (g[y+1][x+1] - g[y-1][x+1])
 *     a, b, c  = the sums of gx * gx, gx * gy, gy * gy over the (2 block_radius + 1)^2 window around the pixel: EACH WINDOW ROW
 *                LEFT TO RIGHT first (r = p[-R]; r = r + p[-R + 1]; ...), THEN THE ROWS' SUMS TOP TO BOTTOM in the same manner
 *     method 0 (min_eig, Shi-Tomasi):  d = a - c;  s = ((a + c) - sqrtf(d * d + 4.f * (b * b))) / 2.f      (sqrt correctly rounded)
 *     method 1 (harris):               t = a + c;  s = (a * c - b * b) - harris_k * (t * t)
 *     score    = s > 0 ? s : 0          (a NaN or a negative response is 0: every score is a non-negative float, and such floats
 *                                        order like their bit patterns)
 * A pixel closer than `border` to a frame edge (x < border or x >= W - border, likewise y) scores 0; border >= block_radius + 1, so
 * no stencil of a scored pixel leaves the frame.  block_radius in 1 .. 3; harris_k finite and >= 0 (checked under both methods).
 *   raft_corner_score_*: score (N, H, W); smax (N) or NULL: the per-image maximum of the score (an atomic maximum over the bits:
 *     order-independent), zeroed by the entry itself.  One launch.
 *
 * raft_detect_points runs the score into its workspace and selects points from it (frames_u8: 1 = uint8 frames, 0 = float32):
 *     thr[n]   = quality_level * smax[n], ONE float32 product; quality_level in [0, 1)
 *     key(p)   = (uint64)score bits << 32 | (0xFFFFFFFF - raster index y * W + x): unique within an image; of two equal scores the
 *                EARLIER pixel in raster order has the larger key
 *     p is a LOCAL MAXIMUM iff its key is the largest in its (2 min_distance + 1)^2 window, clipped to the frame (min_distance in
 *                1 .. RAFT_DETECT_MAX_MIN_DISTANCE).  Any two local maxima are more than min_distance apart in Chebyshev
 *                distance, so an image holds at most ceil(H / (m + 1)) * ceil(W / (m + 1)) of them: the workspace's bound.
 *     a local maximum is a CANDIDATE iff score > 0, score >= thr[n], mask == NULL or mask[n, y, x] != 0 (uint8 (N, H, W)), and it
 *                is not within Chebyshev distance min_distance of a live point of `avoid`: avoid_points (N, avoid_P, 2) as (x, y)
 *                with avoid_lost uint8 (N, avoid_P), code 0 = live (both NULL: none).  A live point (px, py) that is in frame
 *                (0 <= px <= W - 1 and 0 <= py <= H - 1; a NaN is not) bars the integer pixels ceilf(px - (float)m) .. floorf(px +
 *                (float)m) by the same in y; any other point bars nothing.  Mask and avoid apply AFTER the suppression: the
 *                neighbours of a barred maximum do not move up.
 *     the max_points (1 .. RAFT_DETECT_MAX_POINTS) candidates with the LARGEST KEYS per image, largest first, fill the slots:
 *                points (N, K, 2) float32 (x, y), integer-valued; scores (N, K); count (N) int32 = the number of filled slots;
 *                lost (N, K) uint8 or NULL: 0 for a filled slot, 3 for an empty one.  Empty slots hold (-1, -1) and score 0.
 * Codes in `lost` across the tracker: 0 = tracked, 1 = left the frame, 2 = failed the consistency test (raft_track_points_f32),
 * 3 = EMPTY: the slot never held a point.  raft_track_points_f32 keeps any nonzero code and its position bit for bit, so 3 rides
 * through it untouched until raft_refill_points fills the slot.
 * Candidates are gathered through an atomic slot counter, in an order that differs from run to run; keys are unique, so they are a
 * set, and the sorted top-K of a set is the same bits every run.  workspace: raft_detect_points_workspace_bytes(N, H, W,
 * min_distance) bytes (0: the sizes are refused), 8-byte aligned, need not be cleared.  Up to two memsets and four launches on
 * `stream` (score; occupancy stamp, with avoid only; suppression + candidates; one workgroup per image selects and sorts).
 * Errors, in this order: RAFT_E_NULL for a NULL frames, score / points, scores, count or workspace, or only one of the avoid pair;
 * RAFT_E_SHAPE for a non-positive size, C outside {1, 3}, H * W >= 2^32, N * H * W >= 2^31, block_radius outside 1 .. 3, a method
 * or frames_u8 other than 0 or 1, a harris_k that is negative or not finite, border < block_radius + 1, H or W <= 2 * border,
 * max_points or min_distance out of range, a quality_level outside [0, 1) or NaN, N * avoid_P * 2 >= 2^31; RAFT_E_ALIGN for a
 * workspace that is not 8-byte aligned or a float32 / int32 array that is not 4-byte aligned.  All checks precede the first launch.
 *
 * raft_refill_points puts new points into the lost slots of a tracker's state: pos_in (N, P, 2), lost_in uint8 (N, P), new_points
 * (N, K, 2) strongest first with new_count (N) int32 (clamped to 0 .. K), the frame index t >= 0.  Per video, the slots with a
 * nonzero code in ascending slot order take new points 0, 1, ... until either side runs out: the r-th such slot (r < new_count[n])
 * gets pos_out = new_points[n, r], lost_out = 0, born = t, ids = next_id[n] + r; every other slot copies pos and lost through and
 * leaves born and ids as they are; next_id[n] grows by the number of refilled slots.  born, ids (N, P) int32 and next_id (N) int32
 * are updated in place.  One launch, one workgroup per video, an ordered prefix scan over the slots, no atomics; pos_out == pos_in
 * and lost_out == lost_in are allowed (a thread reads its own slot before it writes it).  Ids never repeat within a video (up to
 * 2^31 of them).  Errors: RAFT_E_NULL for any NULL pointer; RAFT_E_SHAPE for a non-positive N or P, K outside 1 ..
 * RAFT_DETECT_MAX_POINTS, a negative t, N * P * 2 >= 2^31; RAFT_E_ALIGN for a float32 / int32 array that is not 4-byte aligned. */
#define RAFT_DETECT_MAX_POINTS 4096
#define RAFT_DETECT_MAX_MIN_DISTANCE 15
int raft_corner_score_f32(const float *frames, float *score, float *smax, int N, int H, int W, int C, int block_radius, int method,
                          float harris_k, int border, void *stream);
int raft_corner_score_u8_f32(const uint8_t *frames, float *score, float *smax, int N, int H, int W, int C, int block_radius, int method,
                             float harris_k, int border, void *stream);
int64_t raft_detect_points_workspace_bytes(int N, int H, int W, int min_distance);
int raft_detect_points(const void *frames, int frames_u8, const uint8_t *mask, const float *avoid_points, const uint8_t *avoid_lost,
                       int64_t avoid_P, float *points, float *scores, int32_t *count, uint8_t *lost, int N, int H, int W, int C,
                       int max_points, int min_distance, float quality_level, int block_radius, int method, float harris_k, int border,
                       void *workspace, void *stream);
int raft_refill_points(const float *pos_in, const uint8_t *lost_in, const float *new_points, const int32_t *new_count, int t,
                       float *pos_out, uint8_t *lost_out, int32_t *born, int32_t *ids, int32_t *next_id, int N, int64_t P, int K,
                       void *stream);

/* Connected components of a mask and their statistics (csrc/components.hip): which objects move, where they
 * are, how large they are and how fast they go.  mask and exclude are uint8 (N, H, W); exclude may be NULL.
 *     FOREGROUND   pixel (n, y, x) iff mask[n, y, x] != 0 and (exclude == NULL or exclude[n, y, x] == 0)
 *     COMPONENTS   the classes of an image's foreground under `connectivity` 4 (W, E, N, S) or 8 (and the diagonals); nothing
 *                  connects two images of a batch
 *     ROOT INDEX   of a component: min(y * W + x) over its pixels
 * Everything below is an integer -- a minimum of indices, integer sums, minima and maxima, taken with integer atomics -- up to ONE
 * float64 division of two exact integers and one rounding to float32 per centroid and mean-flow component.  So every output is a
 * function of the input alone, whatever order the merges and the atomics ran in, and repeats bit for bit.
 *
 * raft_label_components: labels (N, H, W) int32 = 0 for a background pixel, 1 + root index for a foreground pixel.
 *     Three launches, no memset: a 32 x 16 tile labelled in LDS; the tiles' borders merged; every pixel sent to its root.
 *
 * raft_find_objects selects, per image, the components with area >= min_area (min_area >= 1) and orders them by
 *     key      = (uint64)area << 32 | (0xFFFFFFFF - root index), LARGEST FIRST: larger objects first, of equal areas the one that
 *                starts earlier in raster order (keys are unique within an image).
 *     The first K = max_objects (1 .. RAFT_OBJECTS_MAX) of them fill the slots 0 .. K - 1:
 *     count     (N) int32         the number of filled slots
 *     area      (N, K) int32      pixels
 *     boxes     (N, K, 4) int32   x0, y0, x1, y1, inclusive
 *     centroid  (N, K, 2) float32 (float)((double)Sx / (double)area), likewise y, with Sx, Sy the exact integer sums of x and y
 *     mean_flow (N, K, 2) float32 or NULL; written (and flow read) only when flow (float32 (N, H, W, 2)) and mean_flow are BOTH
 *                                 non-NULL.  A pixel of the object contributes iff both components of its vector are finite and
 *                                 at most 2^20 in magnitude: q = (int64)rintf(u * 256.f) (one float32 product, round to nearest
 *                                 even) per component to an int64 sum S, and 1 to a counter cnt; the mean is (float)((double)S /
 *                                 (256.0 * (double)cnt)), or 0 where cnt == 0.  The quantum of 1/256 px is the frame splat's; the
 *                                 clamp keeps every sum below 2^63 (2^31 pixels * 2^28).
 *     labels    (N, H, W) int32 or NULL: slot + 1 for the pixels of a selected component, 0 for background and for the pixels of
 *                                 every other component.
 *     An empty slot has area 0, box (0, 0, -1, -1), centroid (-1, -1) and mean flow 0.
 *     One memset and seven launches: the three above (the third also counts areas, at the root's own pixel), the roots with area >=
 *     min_area gathered as candidates through an atomic slot counter (one reservation per workgroup; their order differs from run
 *     to run, they are a set, and the sorted top-K of a set is the same bits every run), one workgroup per image selects and
 *     sorts, one pass over the pixels writes labels and accumulates boxes and sums into the K records, one thread per slot divides.
 *
 * raft_remove_small_components: out (N, H, W) uint8 = 1 where the pixel is foreground and its component has at least min_area
 *     pixels, else 0.  out == mask IS allowed (the mask is read by the first launch only, out written by the last, which
 *     reads neither); for the same reason out == exclude is safe too.  One memset and four launches.
 *
 * workspace: raft_components_workspace_bytes(N, H, W, connectivity, min_area) bytes (0: the sizes are refused), 8-byte aligned, need
 * not be cleared: 12 bytes per pixel (parent, root, area), N counters, N * bound keys of 8 bytes and N * RAFT_OBJECTS_MAX * 8 records
 * of 56 bytes, every part padded to 8 bytes.  bound is exact: an image holds at most ceil(H / 2) * ceil(W / 2) components under
 * 8-connectivity (no two pixels of a 2 x 2 cell lie in different components), at most ceil(H W / 2) under 4-connectivity, and in
 * either case at most floor(H W / min_area) of at least min_area pixels; bound is the smaller of the two that apply, so the
 * candidate list cannot overflow.  raft_label_components uses the first 4 bytes per pixel only and takes the size of any min_area.
 * No workgroup waits for another anywhere (no flag, no grid barrier, no cooperative launch); no entry synchronises or downloads.
 * Errors, in this order: RAFT_E_NULL for a NULL mask, labels (raft_label_components), out, count, area, boxes, centroid or
 * workspace; RAFT_E_SHAPE for a non-positive size, H * W > 2^31 - 2, N * H * W >= 2^31, a connectivity other than 4 or 8,
 * min_area < 1, max_objects outside 1 .. RAFT_OBJECTS_MAX; RAFT_E_ALIGN for a workspace that is not 8-byte aligned or a float32 /
 * int32 array that is not 4-byte aligned.  All checks precede the first launch. */
#define RAFT_OBJECTS_MAX 1024
int64_t raft_components_workspace_bytes(int N, int H, int W, int connectivity, int min_area);
int raft_label_components(const uint8_t *mask, const uint8_t *exclude, int32_t *labels, int N, int H, int W, int connectivity,
                          void *workspace, void *stream);
int raft_find_objects(const uint8_t *mask, const uint8_t *exclude, const float *flow, int32_t *labels, int32_t *count, int32_t *area,
                      int32_t *boxes, float *centroid, float *mean_flow, int N, int H, int W, int connectivity, int min_area,
                      int max_objects, void *workspace, void *stream);
int raft_remove_small_components(const uint8_t *mask, const uint8_t *exclude, uint8_t *out, int N, int H, int W, int connectivity,
                                 int min_area, void *workspace, void *stream);

/* Object identity through a video (csrc/object_track.hip): which object of one frame pair is which object
 * of the next.  Two consecutive raft_find_objects results deal their slots independently; these three entries carry the labels of
 * the first along the flow into the frame of the second, count what lands on what, match the slots one to one and hand
 * identities on.  Integer sums, integer maxima and one float64 comparison per pair: every output is a function of the input alone
 * and repeats bit for bit.  K = the number of slots, 1 .. RAFT_TRACK_OBJECTS_MAX (128, a choice: the K x K table of one image is
 * then 64 KiB).  There is no workspace, no entry synchronises or downloads, and no workgroup waits for another.
 *
 * raft_object_overlap: labels_prev, labels_next int32 (M, H, W) as raft_find_objects writes them (slot + 1, 0 = background; a
 * value outside 0 .. K counts as background on either side and never indexes anything); flow float32 (M, H, W, 2) from the frame of
 * labels_prev into the frame of labels_next.  Outputs overlap int32 (M, K, K) and landed int32 (M, K), both zeroed by the entry
 * itself (memsets on `stream`).  Per pixel (m, y, x) with a = labels_prev - 1 in 0 .. K - 1 and (u, v) its vector:
 *     skipped unless u and v are both finite;
 *     fx = (float)x + u, fy = (float)y + v, ONE float32 addition each; qx = rintf(fx), qy = rintf(fy) (ties to even);
 *     IN FRAME iff 0 <= qx <= W - 1 and 0 <= qy <= H - 1, compared before any conversion to an integer (the comparison is exact:
 *     against the largest float32 that is <= W - 1, which for an integer-valued qx says the same; an infinite sum fails);
 *     in frame: landed[m, a] += 1, and with b = labels_next[m, qy, qx] - 1 in 0 .. K - 1 also overlap[m, a, b] += 1.
 * All sums are int32 and cannot overflow (M * H * W < 2^31).  One pass over the pixels in 32 x 16 tiles; a tile's counts are put
 * together in LDS (a direct-mapped table of pairs, as raft_find_objects' statistics) before one integer atomic per pair the tile
 * met goes to global memory.  No float atomic.
 *
 * raft_match_objects: overlap (M, K, K), landed (M, K) as above, area_next int32 (M, K) the areas of the next side's slots,
 * min_overlap a float32 in (0, 1].  Per image:
 *     a pair (a, b) is ADMISSIBLE iff overlap[a, b] >= 1 and (double)overlap[a, b] >= (double)min_overlap *
 *         (double)min(landed[a], area_next[b]): one float64 product, one comparison;
 *     key(a, b) = (uint64)overlap[a, b] << 32 | (uint32)(0xFFFF - a) << 16 | (0xFFFF - b): unique; of equal counts the smaller
 *         previous slot wins, then the smaller next slot (smaller slots are larger objects);
 *     THE MATCHING: walk the admissible pairs by key, largest first, and take a pair iff both its slots are still free.
 *   match         (M, K) int32          for next slot b the previous slot it took, or -1
 *   match_overlap (M, K) int32 or NULL  that pair's count, 0 where unmatched
 *   origin        (M, K) int32 or NULL  the previous slot of the largest key in column b over ALL pairs with overlap >= 1, whatever
 *                                       the threshold and whoever was matched; -1 for an all-zero column (after a split it names
 *                                       the object that was divided)
 * One launch, one workgroup per image.  The kernel does not sort: it repeats "every free a picks its best free admissible b, every
 * free b its best free a, pairs that picked each other are matched" until a round matches nothing, at most K rounds, which gives
 * the walk's matching because keys are unique and the largest remaining pair is always mutual.
 *
 * raft_chain_object_ids: identities through S consecutive steps of N videos in ONE launch, one workgroup per video.  match int32
 * (S, N, K) (a value outside -1 .. K - 1 is treated as -1); count int32 (S, N), the filled slots of each step's objects (clamped to
 * 0 .. K); ids_in, born_in int32 (N, K) the state before step 0; next_id int32 (N), updated in place once, at the end; ids, born
 * int32 (S, N, K) the state after every step.  Step s reads the state of step s - 1 (ids_in / born_in for s == 0).  A filled slot
 * b < count[s, n] with a = match[s, n, b] >= 0 gets the id and born of previous slot a; an unmatched filled slot gets ids =
 * next_id[n] + r and born = t0 + s, r its rank among the unmatched filled slots of that step in ascending slot order
 * (raft_refill_points' ordered scan), and next_id[n] grows by their number; an empty slot gets -1 / -1.  ids == ids_in and born ==
 * born_in are allowed when S == 1 (every thread reads the previous state before any thread writes, behind a barrier).  The first
 * objects of a video get 0 .. count - 1 from this entry too: match all -1 and next_id = 0.
 *
 * Errors, in this order, all before any launch: RAFT_E_NULL for a NULL pointer other than match_overlap and origin; RAFT_E_SHAPE
 * for a non-positive size, K outside 1 .. RAFT_TRACK_OBJECTS_MAX, M * H * W >= 2^31, a min_overlap outside (0, 1] or NaN, a negative
 * t0 (or t0 + S >= 2^31), S * N * K >= 2^31; RAFT_E_ALIGN for an array that is not 4-byte aligned. */
#define RAFT_TRACK_OBJECTS_MAX 128
int raft_object_overlap(const int32_t *labels_prev, const float *flow, const int32_t *labels_next, int32_t *overlap, int32_t *landed,
                        int M, int H, int W, int K, void *stream);
int raft_match_objects(const int32_t *overlap, const int32_t *landed, const int32_t *area_next, float min_overlap, int32_t *match,
                       int32_t *match_overlap, int32_t *origin, int M, int K, void *stream);
int raft_chain_object_ids(const int32_t *match, const int32_t *count, int t0, const int32_t *ids_in, const int32_t *born_in,
                          int32_t *next_id, int32_t *ids, int32_t *born, int S, int N, int K, void *stream);

/* ------------------------------------------------------------------ training augmentation */

/* FlowAugmentor (reference tf_raft/datasets/augmentor.py:9-129, used at dataset.py:87-91) composed into one gather (the sparse
 * augmentor shares the record and the frame path, see raft_augment_gather_sparse_u8): every pixel
 * of the crop is a bilinear blend of four source pixels (cv2.resize INTER_LINEAR as restated in DESIGN.md section 10), the colour
 * map and the eraser rectangles of frame 2 are applied to the taps, the flow is rescaled and flipped on the way.  The host draws
 * one record per sample (tf_raft_amd/augment.py) and uploads the records; no image-sized intermediate exists.
 * Every operation is individually rounded (no fused multiply-add), so the results are reproducible bit for bit on the host. */
typedef struct {
    double inv_fx, inv_fy;   /* 1 / fx, 1 / fy: source coordinate of resized index d is (float)((d + 0.5) * inv - 0.5) */
    double fx, fy;           /* flow factors (the resize factors) */
    double hue[2], sat[2], val[2];   /* HueSaturationValue shifts of frame 1, frame 2 */
    float alpha[2], beta[2]; /* RandomBrightnessContrast: v * alpha + beta (beta already times 255) */
    int32_t W1, H1;          /* size after the resize (the source size when resize == 0) */
    int32_t x0, y0;          /* origin of the crop in the resized, flipped frame */
    int32_t resize;          /* 0: the taps are plain copies (the reference skips cv2.resize) */
    int32_t flip_h, flip_v;
    int32_t color[2];        /* per frame: bit 0 brightness / contrast on, bit 1 hue / saturation / value on */
    int32_t n_rect;          /* 0..2 eraser rectangles */
    int32_t rect[2][4];      /* x0, y0, x1, y1 (exclusive) in SOURCE coordinates of frame 2, clipped to the frame */
} RaftAugmentParams;

#define RAFT_AUGMENT_SUM_BLOCKS 64   /* partial sums per sample */

/* sizeof(RaftAugmentParams): the binding checks its mirror against it.  Host-only. */
int raft_augment_params_bytes(void);

/* Per-sample channel sums of colour-mapped frame 2 (the eraser's fill is their truncated mean): img2 (N, H, W, 3) uint8,
 * params: N records in DEVICE memory, partial: uint32[N][RAFT_AUGMENT_SUM_BLOCKS][4], written (not accumulated) for every sample
 * whose n_rect > 0 and left untouched for the others.  H * W <= 2^24 so that 32 bits hold a channel's sum. */
int raft_augment_sums_u8(const uint8_t *img2, const RaftAugmentParams *params, uint32_t *partial, int N, int H, int W, void *stream);

/* The gather: img1, img2 (N, H, W, 3) uint8 and flow (N, H, W, 2) float -> out1, out2 (N, h, w, 3) uint8, out_flow (N, h, w, 2)
 * float and valid (N, h, w) float = |u| < 1000 & |v| < 1000 (dataset.py:102).  params / partial as above (partial is read only
 * for samples whose n_rect > 0).  The records are trusted to keep every tap inside the source (tf_raft_amd/augment.py draws
 * them so); the kernel clamps tap indices to the frame regardless.  Every output element is written exactly once. */
int raft_augment_gather_u8(const uint8_t *img1, const uint8_t *img2, const float *flow, const RaftAugmentParams *params,
                           const uint32_t *partial, uint8_t *out1, uint8_t *out2, float *out_flow, float *valid,
                           int N, int H, int W, int h, int w, void *stream);

/* SparseFlowAugmentor (reference tf_raft/datasets/augmentor.py:132-267, used at dataset.py:88-89): the frames as above; flow and
 * validity of a resized sample by the reference's scatter (resize_sparse_flow_map) restated as a gather.  A
 * valid source (x, y) lands on (rint(x f), rint(y f)) in double, halves to even, with f = params.fx for both axes; output pixel
 * (X, Y) of the resized frame takes, of the sources with valid_in >= 1 that land on it, the last in row-major order: flow
 * (float)((double)flow * f) and valid 1; without such a source, or with X == 0 or Y == 0, flow 0 and valid 0.  A sample that is not
 * resized copies flow and valid_in as they are.  The horizontal flip negates u; flip_v is not read.  valid_in (N, H, W) float,
 * valid_out (N, h, w) float; the rest as for raft_augment_gather_u8.  f >= 1/8 is the caller's promise (tf_raft_amd/augment.py
 * checks it): the kernel looks no further than 5 sources beyond X / f.  No atomics, no intermediate; every output element is
 * written exactly once.  Argument errors as for the dense entry: RAFT_E_NULL (-1) for a null pointer, RAFT_E_SHAPE (-2) for a
 * bad size, H * W or h * w > 2^24, or N > 65535, and RAFT_E_ALIGN when flow is not 8-byte aligned (it is read as float2). */
int raft_augment_gather_sparse_u8(const uint8_t *img1, const uint8_t *img2, const float *flow, const float *valid_in,
                                  const RaftAugmentParams *params, const uint32_t *partial, uint8_t *out1, uint8_t *out2,
                                  float *out_flow, float *valid_out, int N, int H, int W, int h, int w, void *stream);

/* Measurement utility (no reference counterpart): `blocks` workgroups of 256 threads, every wave issuing `iters` x 8
 * independent v_mfma_f32_16x16x4_f32 (nothing else in the loop; non-zero lane-varying operands); out: blocks * 256
 * floats (written so that the loop cannot be optimised away).  FLOPs = blocks * 4 * iters * 8 * 2048.  bench.py times it
 * to state the fp32-MFMA rate the box SUSTAINS (power-limited clock) next to the 157.3 TFLOP/s datasheet figure every
 * `roofline.frac` is quoted against. */
int raft_mfma_probe_f32(float *out, int blocks, int iters, void *stream);

/* ------------------------------------------------------------------ convolutions */

/* Packed weight layout of the implicit-GEMM convolution: for a Keras kernel (kh, kw, Cin, Cout)
 *   wp[((t * (Kpad/4) + k/4) * npad + n) * 4 + k%4] = kernel[t / kw, t % kw, k, n]
 * with Kpad = Cin rounded up per input source to a multiple of 32 and npad = Cout rounded up
 * to a multiple of 64; padding is zero.  bias is float[npad].  The host mirror
 * (tf_raft_amd/packing.py) produces these once per model. */

enum { RAFT_ACT_NONE = 0, RAFT_ACT_RELU = 1 };

/* One stride-1 'same' Keras Conv2D (+ optional relu, + scale) on fp32 MFMA.
 * Replaces a layers.Conv2D call (reference update.py:10-11, 91-95, 138-140).
 * The input is the channel concatenation of up to two NHWC sources: channels [0, c0) of a0
 * (pixel stride lda0 floats) followed by [0, c1) of a1 (c1 may be 0, a1 NULL); c0 and c1 must be
 * multiples of 32 (pad with zero channels).  out[pixel * ldo + n] for n < nvalid.
 * (kh, kw) in {(1,1), (3,3), (1,5), (5,1)}. */
int raft_conv2d_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                    const float *wp, const float *bias, int B, int H, int W, int kh, int kw,
                    int npad, int nvalid, int act, float scale, float *out, int ldo,
                    void *stream);

/* The same convolution for 3x3 kernels by Winograd F(2x2, 3x3) (fp32 arithmetic, 2.25x fewer multiplies; what
 * cuDNN runs under the reference's Conv2D on a GPU; not bit-identical to the direct kernel).  `wp` = the
 * transformed kernel G g G^T packed as a 4x4-tap kernel; c0, c1 multiples of 16, npad a multiple of 32. */
int raft_conv2d_winograd_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                             const float *wp, const float *bias, int B, int H, int W, int npad,
                             int nvalid, int act, float scale, float *out, int ldo, void *stream);

/* The same by Winograd F(4x4, 3x3) (36 multiplies per 16 outputs: 4x fewer than the direct kernel, 1.78x fewer than
 * F(2x2, 3x3); fp32, points {0, +-5/8, +-3/2, inf}; deviation from the float64 convolution ~3x that of F(2x2, 3x3)).
 * `wp` = the transformed kernel in the consumption order of the kernel, (Cin/16, 72, 4, npad/32, 16, 2, 2) -- packing.py
 * pack_conv_winograd4; c0, c1 multiples of 16, npad a multiple of 64. */
int raft_conv2d_winograd4_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                              const float *wp, const float *bias, int B, int H, int W, int npad,
                              int nvalid, int act, float scale, float *out, int ldo, void *stream);

/* 1x5 (kh = 1, kw = 5) or 5x1 convolution by 1-D Winograd F(2, 5) (6 multiplies per output pair instead of 10;
 * fp32, points {0, +-1, +-1/2, inf}).  `wp` = the transformed kernel packed with 6 taps; c0, c1 multiples of 16. */
int raft_conv1d_winograd_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                             const float *wp, const float *bias, int B, int H, int W, int kh, int kw,
                             int npad, int nvalid, int act, float scale, float *out, int ldo, void *stream);

/* The same by 1-D Winograd F(4, 5) (8 multiplies per 4 outputs; points {0, +-1, +-1/2, +-2, inf}).  `wp` = the
 * transformed kernel packed with 8 taps (packing.py pack_conv_winograd1d(..., m=4)); c0, c1 multiples of 32. */
int raft_conv1d_winograd4_f32(const float *a0, int lda0, int c0, const float *a1, int lda1, int c1,
                              const float *wp, const float *bias, int B, int H, int W, int kh, int kw,
                              int npad, int nvalid, int act, float scale, float *out, int ldo, void *stream);

/* cor1 = relu(convc1(CorrBlock.retrieve(coords))) in ONE kernel (reference corr.py:116-152 + update.py:91, 98): the
 * window values are those of raft_corr_lookup_f32 bit for bit, but they live only in LDS as the A operand of the 1x1
 * convolution -- the (B, h, w, 324) lookup output is neither written nor re-read.  levels = 4, radius = 4, npad = 256.
 * wp / bias: packing.py pack_convc1_fused.  out: (B*h*w, ldo), first nvalid channels written. */
int raft_lookup_convc1_f32(const float *pyr, const int64_t *level_offsets, const float *coords, int B, int h, int w,
                           const float *wp, const float *bias, int npad, int nvalid, float *out, int ldo, void *stream);

/* ------------------------------------------------------------------ update block */

typedef struct raft_conv_weights {
    const float *wp;     /* packed kernel (see above) or a layer-specific layout */
    const float *bias;
    int npad;
} raft_conv_weights;

/* BasicUpdateBlock weights (reference update.py:128-153).  z and r convolutions of each GRU
 * half are fused along N (npad 256 = [z | r]); flow_head.conv1 and mask[0] are fused along N
 * (npad 512 = [flow_head.conv1 | mask.0]).
 * convf1: (7,7,2,128) kept in Keras layout [t][c][n] (98 x 128 floats).
 * fh2: flow_head.conv2 (3,3,256,2) kept in Keras layout [t][c][2].
 * SepConvGRU (update.py:38-67), input order hx = [h(128) | inp(128) | motion(126) | flow(2)]: the rows of
 * convz / convr / convq that multiply `inp` are split off into gru_ctx1 (1x5) / gru_ctx2 (5x1), each
 * (kh,kw,128,384) = [z | r | q] WITH the three biases; gru_zr{1,2} / gru_q{1,2} keep the h rows and the
 * [motion | flow] rows (K = 256 per tap) and carry ZERO bias.  `inp` is constant over the prediction
 * loop, so its contribution is evaluated once per forward (raft_gru_context_f32). */
typedef struct raft_basic_update_weights {
    raft_conv_weights convc1, convc2, convf1, convf2, conv;
    raft_conv_weights gru_zr1, gru_q1, gru_zr2, gru_q2;
    raft_conv_weights fh1_mask0, fh2, mask2;
    raft_conv_weights gru_ctx1, gru_ctx2;
    /* optional (wp == NULL: not supplied): Winograd F(2x2, 3x3) transformed copies of the 3x3 layers, U = G g G^T
     * packed as a 4x4-tap kernel (16, Cin/4, npad, 4) -- tf_raft_amd/packing.py pack_conv_winograd */
    raft_conv_weights convc2_w, convf2_w, conv_w, fh1_mask0_w;
    /* optional: 1-D Winograd F(2, 5) transformed copies of gru_zr{1,2} / gru_q{1,2}: U = G' g packed as a 6-tap
     * kernel (6, Cin/4, npad, 4) -- tf_raft_amd/packing.py pack_conv_winograd1d */
    raft_conv_weights gru_zr1_w, gru_q1_w, gru_zr2_w, gru_q2_w;
    /* optional: Winograd F(2x2, 3x3) copy of flow_head.conv1 ALONE (3,3,128,256), for raft_iterate_basic_final_f32 */
    raft_conv_weights fh1_w;
    /* optional: 1-D Winograd F(4, 5) transformed copies of gru_zr{1,2} / gru_q{1,2}, packed as 8-tap kernels
     * (8, Cin/4, npad, 4) -- pack_conv_winograd1d(..., m=4); preferred over the F(2, 5) copies when supplied */
    raft_conv_weights gru_zr1_w4, gru_q1_w4, gru_zr2_w4, gru_q2_w4;
    /* optional: convc1 repacked for raft_lookup_convc1_f32 (K = 4 levels x 84: each level's 81 channels + 3 zero rows;
     * (84, 256, 4) -- packing.py pack_convc1_fused).  When supplied, the raft_iterate_basic_* loops on a STORED volume
     * run the lookup fused into convc1 (RAFT_LOOKUP_FUSED = 0 keeps the two kernels). */
    raft_conv_weights convc1_f;
    /* optional: 1-D Winograd F(4, 5) transformed copies of gru_ctx1 / gru_ctx2 (8-tap kernels, with the biases) */
    raft_conv_weights gru_ctx1_w4, gru_ctx2_w4;
    /* optional: Winograd F(4x4, 3x3) transformed copies of convc2 / conv / fh1_mask0 and of flow_head.conv1 alone
     * (packing.py pack_conv_winograd4); preferred over the F(2x2, 3x3) copies where RAFT_CONV_WINO4 has the layer's bit */
    raft_conv_weights convc2_w44, conv_w44, fh1_mask0_w44, fh1_w44;
    /* optional: the same for convf2 (RAFT_CONV_WINO4 bit 2) */
    raft_conv_weights convf2_w44;
} raft_basic_update_weights;

/* Device state of the recurrent loop (all caller-owned, (B*h*w) pixels, NHWC):
 *   net    (M,128)  hidden state h, updated in place
 *   x      (M,256)  GRU input [inp(128) | motion(126) | flow(2)]; inp is written once by
 *                   raft_prepare_state_f32, the rest every iteration
 *   corr   (M,352)  lookup output, 324 used + 28 zero pad channels
 *   coords1(M,2), flow (M,2), delta (M,2), mask (M,576)
 *   ws              scratch, raft_update_workspace_floats() floats
 *   ctx    (M,768)  loop-invariant GRU pre-activation terms [z1 | r1 | q1 | z2 | r2 | q2] of `inp`,
 *                   written by raft_gru_context_f32 (BasicUpdateBlock only; SmallRAFT ignores it) */
typedef struct raft_state {
    float *net, *x, *corr, *coords1, *flow, *delta, *mask, *ws, *ctx;
} raft_state;

int64_t raft_update_workspace_floats(int B, int h, int w);

/* model.py:84-89 -- net = tanh(cnet[..., :128]); inp = relu(cnet[..., 128:]); coords1 = grid;
 * flow = 0; zero the pad channels of corr.  cnet: (B, h, w, 256). */
int raft_prepare_state_f32(const float *cnet, int B, int h, int w, const raft_state *st,
                           void *stream);

/* conv{z,r,q}{1,2} restricted to the `inp` rows of the GRU input, plus their biases -> st->ctx.
 * Must run after raft_prepare_state_f32 (or any other write of x[:, 0:128]) and before
 * raft_update_basic_f32 / raft_iterate_basic_*; reference update.py:51-67 evaluates these rows inside
 * every SepConvGRU call, model.py:86 shows `inp` is fixed for the whole loop. */
int raft_gru_context_f32(const raft_basic_update_weights *wts, int B, int h, int w,
                         const raft_state *st, void *stream);

/* One BasicUpdateBlock call + the coordinate update (reference update.py:143-153 and
 * model.py:97-102): reads st->corr, st->flow, st->net, st->x, st->ctx; writes st->net, st->mask
 * (already scaled by 0.25), st->delta, st->coords1 (+= delta), st->flow (coords1 - coords0). */
int raft_update_basic_f32(const raft_basic_update_weights *wts, int B, int h, int w,
                          const raft_state *st, void *stream);

/* The whole prediction loop of RAFT.call (reference model.py:91-109), `iters` times:
 * lookup -> update -> coords1 += delta -> convex upsample.  flow_up: (iters, B, 8h, 8w, 2);
 * prediction i is written to flow_up + i * B*8h*8w*2. */
int raft_iterate_basic_f32(const raft_basic_update_weights *wts, const float *pyr,
                           const int64_t *level_offsets, int B, int h, int w, int iters,
                           const raft_state *st, float *flow_up, void *stream);

/* Caller-owned context of the three-stream loops below: the four cross-stream events of the schedule.  Create once per
 * model / thread on the device the loops run on (the only entry point that allocates), pass to every
 * raft_iterate_basic_{overlap,ondemand,final}_f32 call, destroy after the last loop has drained.  Not thread-safe: one
 * context per launching thread. */
typedef struct raft_loop_ctx raft_loop_ctx;
int raft_loop_ctx_create(raft_loop_ctx **ctx);
int raft_loop_ctx_destroy(raft_loop_ctx *ctx);

/* The same loop scheduled on three streams: the flow branch (convf1, convf2) and the mask branch (mask2,
 * convex upsample) run on the caller-owned side streams aux0 / aux1 next to the main chain on `stream`,
 * ordered by events; everything is joined back into `stream` before the call returns (it still only
 * enqueues).  Results are identical to raft_iterate_basic_f32.
 * aux0 == aux1 == stream selects the SINGLE-STREAM schedule (the launches of raft_iterate_basic_f32, no events) for
 * this and the two entry points below: what a caller that keeps several loops in flight on streams of their own
 * (tf_raft_amd/model.py, lanes of the pipelined forward) runs on each.  Any other coincidence of the three streams is
 * RAFT_E_UNSUPPORTED. */
int raft_iterate_basic_overlap_f32(const raft_basic_update_weights *wts, const float *pyr,
                                   const int64_t *level_offsets, int B, int h, int w, int iters,
                                   const raft_state *st, float *flow_up, void *stream, void *aux0, void *aux1,
                                   raft_loop_ctx *ctx);

/* The three-stream loop with the volume-free correlation (BASELINE config 4, no reference code: README.md:109):
 * fmap1 (B, h, w, C) and fmap2_pyr (raft_fmap_pyramid_f32) replace the stored pyramid. */
int raft_iterate_basic_ondemand_f32(const raft_basic_update_weights *wts, const float *fmap1,
                                    const float *fmap2_pyr, int C, int B, int h, int w, int iters,
                                    const raft_state *st, float *flow_up, void *stream, void *aux0, void *aux1,
                                    raft_loop_ctx *ctx);

/* The three-stream loop for callers that want flow_predictions[-1] only (reference model.py:160-166, predict_step):
 * mask head + convex upsampling run in the last iteration only; flow_up_last: (B, 8h, 8w, 2).  The recurrence is launch
 * for launch that of raft_iterate_basic_overlap_f32, so the result equals its last prediction.  Needs wts->fh1_w. */
int raft_iterate_basic_final_f32(const raft_basic_update_weights *wts, const float *pyr,
                                 const int64_t *level_offsets, int B, int h, int w, int iters,
                                 const raft_state *st, float *flow_up_last, void *stream, void *aux0, void *aux1,
                                 raft_loop_ctx *ctx);

/* Profiling twin of raft_iterate_basic_f32 (bench.py only): the same launches with a HIP event
 * recorded on `stream` after every kernel; synchronises the stream and accumulates the elapsed
 * milliseconds of each stage over all iterations into the HOST array stage_ms.  Stage order:
 * lookup, convc1, convc2, convf1, convf2, conv, gru_zr1, gru_q1, gru_zr2, gru_q2, fh1_mask0, fh2,
 * mask2, upsample. */
#define RAFT_BASIC_STAGES 14
int raft_iterate_basic_timed_f32(const raft_basic_update_weights *wts, const float *pyr,
                                 const int64_t *level_offsets, int B, int h, int w, int iters,
                                 const raft_state *st, float *flow_up, void *stream,
                                 float *stage_ms /* host, [RAFT_BASIC_STAGES] */);

/* ------------------------------------------------------------------ encoders */

/* BasicEncoder / SmallEncoder forward (reference extractor.py:88-130, 133-175; ResBlock 19-49;
 * Normalization 6-16), inference mode.  Channel widths: stem c0, layer1..3 c1..c3 (multiples of 32),
 * output cout.  norm:
 *   RAFT_NORM_NONE      no normalisation (SmallRAFT cnet)
 *   RAFT_NORM_INSTANCE  tfa InstanceNormalization, eps 1e-3, biased variance, affine in_gamma / in_beta
 *   RAFT_NORM_FOLDED    Keras BatchNormalization in inference mode, folded into kernels and biases by the
 *                       host packer (tf_raft_amd/packing.py): the device sees plain convolutions
 * Convolution kernels use the packed layout above; the 7x7 stem is packed as 7 K-chunks (one per kernel
 * row) of k = kx * 4 + ch over the 4-channel padded image.  block[i][2] (down-sampling 1x1) has wp == NULL
 * for stride-1 blocks.  in_gamma / in_beta index: 0 = stem norm1, 1 + 3*i + {0, 1, 2} = block i norm1,
 * norm2, downsample norm. */
enum { RAFT_NORM_NONE = 0, RAFT_NORM_INSTANCE = 1, RAFT_NORM_FOLDED = 2 };

typedef struct raft_encoder_weights {
    int c0, c1, c2, c3, cout, norm;
    raft_conv_weights conv1;
    raft_conv_weights block[6][3];
    raft_conv_weights conv2;
    const float *in_gamma[19];
    const float *in_beta[19];
    /* optional (wp == NULL: absent): Winograd F(2x2, 3x3) transformed copies of block[i][0] (when it has
     * stride 1) and block[i][1], packed as 4x4-tap kernels (see raft_conv2d_winograd_f32) */
    raft_conv_weights block_w[6][2];
    /* optional: Winograd F(4x4, 3x3) transformed copies of the same layers in the consumption order of
     * raft_conv2d_winograd4_f32 (used for the stages RAFT_ENC_WINO4 selects) */
    raft_conv_weights block_w44[6][2];
} raft_encoder_weights;

int64_t raft_encoder_workspace_floats(const raft_encoder_weights *w, int n, int H, int W);

/* images: (n, H, W, 3); out: (n, ceil(H/8), ceil(W/8), cout).  input_affine != 0 applies the model's
 * 2 * (image / 255) - 1 (reference model.py:70-71) while the image is staged. */
int raft_encoder_f32(const raft_encoder_weights *w, const float *images, int n, int H, int W,
                     int input_affine, float *out, float *workspace, void *stream);
/* The feature encoder's call on [image1, image2] (reference extractor.py:114-116 concatenates along the batch, 128-130 splits
 * again): images_a / images_b: (n_each, H, W, 3) each, staged from where they lie; out: (2 * n_each, ...), the first n_each
 * maps belong to images_a.  Workspace = raft_encoder_workspace_floats(w, 2 * n_each, H, W). */
int raft_encoder_pair_f32(const raft_encoder_weights *w, const float *images_a, const float *images_b, int n_each, int H, int W,
                          int input_affine, float *out, float *workspace, void *stream);

/* ------------------------------------------------------------------ SmallRAFT update block */

/* SmallUpdateBlock weights (reference update.py:109-125): z and r of the 3x3 ConvGRU fused along N
 * (npad 192 = [z 96 | r 96]); convf1 (7,7,2,64) and fh2 = flow_head.conv2 (3,3,128,2) in Keras layout.
 * State: net (M,96); x (M,160) = [inp 64 | motion 80 | flow 2 | 14 zero pad]; corr (M,224) = 196 used
 * + 28 zero pad; mask is unused (SmallUpdateBlock returns None). */
typedef struct raft_small_update_weights {
    raft_conv_weights convc1, convf1, convf2, conv, gru_zr, gru_q, fh1, fh2;
    /* optional: Winograd F(2x2, 3x3) transformed copies of the 3x3 layers (see raft_basic_update_weights) */
    raft_conv_weights conv_w, gru_zr_w, gru_q_w, fh1_w;
} raft_small_update_weights;

int64_t raft_small_update_workspace_floats(int B, int h, int w);
/* cnet: (B, h, w, 160) -> net = tanh(cnet[..., :96]), inp = relu(cnet[..., 96:]).  model.py:206-211 */
int raft_prepare_state_small_f32(const float *cnet, int B, int h, int w, const raft_state *st,
                                 void *stream);
/* One SmallUpdateBlock call + coordinate update (update.py:118-125, model.py:216-220). */
int raft_update_small_f32(const raft_small_update_weights *wts, int B, int h, int w,
                          const raft_state *st, void *stream);
/* The prediction loop of SmallRAFT.call (model.py:213-226): lookup (radius 3) -> update -> upflow8. */
int raft_iterate_small_f32(const raft_small_update_weights *wts, const float *pyr,
                           const int64_t *level_offsets, int B, int h, int w, int iters,
                           const raft_state *st, float *flow_up, void *stream);

/* ------------------------------------------------------------------ a recurrence that does not start from zero */

/* RAFT's video protocol: the loop of pair t + 1 starts from the low-resolution flow of pair t projected
 * forward along itself.  flow, out: (B, h, w, 2) floats, [..., 0] = u along x, [..., 1] = v along y, each image on its own.
 *   raft_forward_interpolate_f32: source j = y0 * w + x0 with vector (dx, dy) ends at x1 = float(x0) + dx, y1 = float(y0) + dy,
 *     ONE float32 addition each, and is valid iff 0 < x1 < w and 0 < y1 < h (strict; a NaN fails).  out[b, ty, tx] is the vector
 *     of the valid source that minimises d = (tx - x1) * (tx - x1) + (ty - y1) * (ty - y1), every float32 operation rounded on
 *     its own (no fused multiply-add), ties to the lowest j; an image without a valid source gives zeros.  Exhaustive search, one
 *     launch on `stream`, every output element written exactly once.  out must not overlap flow (RAFT_E_UNSUPPORTED).
 *   raft_warm_start_f32 / raft_warm_start_small_f32: after raft_prepare_state_f32 / raft_prepare_state_small_f32 (and in front of
 *     the loop), on the state of that variant: coords1 = grid + flow_init (one float32 addition per component), flow =
 *     flow_init, and the flow channels of the GRU input x (the last two of the 256; channels 144 and 145 of the 160) =
 *     flow_init -- the three places the loop's first iteration reads a flow from.  One launch; nothing else is written.
 * RAFT_E_NULL for a NULL pointer (st, st->x, st->coords1, st->flow included); RAFT_E_SHAPE for a non-positive size or B * h * w * 2
 * of 2^31 or more; RAFT_E_ALIGN for a flow, out, coords1, flow or x that is not 8-byte aligned (float2 accesses).  All checks
 * precede the launch. */
int raft_forward_interpolate_f32(const float *flow, int B, int h, int w, float *out, void *stream);
int raft_warm_start_f32(const float *flow_init, int B, int h, int w, const raft_state *st, void *stream);
int raft_warm_start_small_f32(const float *flow_init, int B, int h, int w, const raft_state *st, void *stream);

/* ------------------------------------------------------------------ evaluation metrics / loss */

/* Reductions over flow predictions (reference tf_raft/losses/losses.py; the caller side of the forward pass:
 * model.py:146-158 test_step, 126-144 train_step).  flow_gt / predictions: (npix, 2) fp32 with npix = B*H*W;
 * valid: npix bytes (0 = invalid).  valid' = valid & (|flow_gt|_2 < max_flow).  Deterministic (no atomics);
 * `workspace` = raft_metrics_workspace_doubles() doubles, 8-byte aligned; results are written to device memory. */
int64_t raft_metrics_workspace_doubles(void);
/* end_point_error (losses.py:24-43): out5 = {mean EPE over valid', rate EPE < 1, rate EPE < 3, rate EPE < 5,
 * number of valid' pixels}; the means are NaN when no pixel is valid' (as tf.reduce_mean of an empty tensor). */
int raft_flow_metrics_f32(const float *flow_gt, const unsigned char *valid, const float *flow_pred,
                          int64_t npix, float max_flow, float *out5, double *workspace, void *stream);
/* sequence_loss (losses.py:4-21): loss = sum_i gamma^(n-i-1) * mean over ALL 2*npix elements of valid' * |pred_i - gt|.
 * Prediction i starts at preds + i * pred_stride floats (the flow_up buffer of raft_iterate_*: stride 2*npix);
 * n_predictions <= 64. */
int raft_sequence_loss_f32(const float *flow_gt, const unsigned char *valid, const float *preds,
                           int64_t pred_stride, int n_predictions, int64_t npix, double gamma, float max_flow,
                           float *loss_out, double *workspace, void *stream);

/* ------------------------------------------------------------------ training step, first slice (backward kernels) */

/* The reference's train_step (model.py:126-144) differentiates the forward pass with tf.GradientTape.  These entry points
 * are the backward of the path-specific ops, deterministic (no atomics).  BASELINE config 5; see DESIGN.md section 9 for
 * what is and is not built yet. */

/* d sequence_loss / d prediction_i for all n predictions (losses.py:4-21):
 *   d_preds[i][e] = upstream * gamma^(n-i-1) * valid'[pixel(e)] * sign(pred_i[e] - flow_gt[e]) / (2 * npix),  sign(0) = 0.
 * d_preds has the layout of preds (prediction i at d_preds + i * pred_stride). */
int raft_sequence_loss_grad_f32(const float *flow_gt, const unsigned char *valid, const float *preds,
                                int64_t pred_stride, int n_predictions, int64_t npix, double gamma, float max_flow,
                                float upstream, float *d_preds, void *stream);

/* Self-supervised sequence loss and its gradient in ONE launch (no reference counterpart).
 *   image1, image2 (B, H, W, 3) float in 0..255; mask NULL (all ones) or uint8 (B, H, W), nonzero = use the pixel;
 *   preds: n_predictions flows (B, H, W, 2), prediction i at preds + i * pred_stride (floats).
 * With s = 1/255, rho(d) = sqrtf(d*d + eps*eps) (eps*eps rounded once to float32), w_i = (float)gamma^(n-i-1) built on the host
 * as raft_sequence_loss_f32 builds it, W2 = image2 sampled at the pixel's sample position under p_i exactly as raft_warp_f32
 * samples (same position, in-frame test `inside`, taps and weights a, b):
 *   ph_i = sum mask * inside * rho(s * (W2_c - image1_c)) / (B*H*W*3)          (the divisor counts ALL elements)
 *   wx(x,y) = expf(-edge_weight * mean_c |s * (image1(x+1,y)_c - image1(x,y)_c)|) for x < W-1, wy likewise along y
 *   sm_i = [sum wx * rho(p(x+1,y)_k - p(x,y)_k) + sum wy * rho(p(x,y+1)_k - p(x,y)_k)] / (B*H*W*2), k in {u, v}
 *   loss = sum_i w_i * (ph_i + smooth_weight * sm_i);      out3 = {loss, ph_{n-1}, sm_{n-1}}
 * d_preds: NULL (value only), or the layout of preds; d_preds_i = upstream * w_i * (d ph_i + smooth_weight * d sm_i), every
 * element written exactly once (gaps of a pred_stride larger than 2*B*H*W are not touched).  mask and inside are constants of
 * the gradient; dW2_c/du = (1-b)*(g01-g00) + b*(g11-g10), dW2_c/dv = (1-a)*(g10-g00) + a*(g11-g01), the one-sided derivative of
 * the cell the taps come from; the smoothness gradient is the adjoint as a gather, missing neighbours dropped.
 * Deterministic (no atomics, no memset): float64 partial records in `workspace` (raft_photometric_loss_workspace_doubles()
 * doubles), added in index order by a second one-workgroup launch.
 * RAFT_E_NULL: image1, image2, preds, out3 or workspace NULL.  RAFT_E_SHAPE: a non-positive size, pred_stride < 2*B*H*W,
 * B*H*W*3 of 2^31 or more, eps or eps*eps (in float32) not positive and finite, gamma / smooth_weight / edge_weight negative or not finite, upstream
 * not finite.  RAFT_E_UNSUPPORTED: n_predictions > 64 or an odd pred_stride.  RAFT_E_ALIGN: preds, d_preds or workspace not
 * 8-byte aligned.  All checks precede the first launch. */
int64_t raft_photometric_loss_workspace_doubles(void);
int raft_photometric_loss_f32(const float *image1, const float *image2, const uint8_t *mask, const float *preds,
                              int64_t pred_stride, int n_predictions, int B, int H, int W, double gamma, float smooth_weight,
                              float edge_weight, float eps, float upstream, float *out3, float *d_preds, double *workspace,
                              void *stream);

/* Soft census term of the self-supervised loss and its gradient (csrc/census_loss.hip).  Inputs as for
 * raft_photometric_loss_f32.  With gray(c) = (0.299f*R + 0.587f*G) + 0.114f*B on 0..255, g1 = gray(image1), w_i the bilinear sample
 * of gray(image2) under p_i (0 out of frame), f(d) = d / sqrtf(0.81f + d*d), h(e) = e*e / (0.1f + e*e),
 * interior(x, y) = 3 <= x <= W-4 && 3 <= y <= H-4, M_i = mask && inside_i && interior:
 *   D(y) = (1/48) * sum over the 48 neighbours z of y in a 7x7 patch of h(f(w_i(z) - w_i(y)) - f(g1(z) - g1(y)))
 *   cen_i = sum_y M_i(y) * D(y) / (B*H*W),     w_i = (float)gamma^(n-i-1)
 *   out2[0] = (add_to ? *add_to : 0) + census_weight * sum_i w_i * cen_i  (formed in double, rounded once; add_to may be out2);
 *   out2[1] = cen_{n-1}
 * d_preds: NULL (value only), or the layout of preds; every element is touched exactly once with
 * upstream * census_weight * w_i * d cen_i -- stored (accumulate == 0) or added to what is there with one float32 addition
 * (accumulate == 1); gaps of a pred_stride larger than 2*B*H*W are not touched.  mask and inside are constants of the gradient;
 * the derivatives of w_i are the one-sided ones of raft_photometric_loss_f32.
 * Deterministic (no atomics, no memset).  `workspace`: raft_census_loss_workspace_bytes(n_predictions, B, H, W) bytes (float64
 * partial records, g1, and per prediction the planes w_i and M_i; 0 for sizes the entry refuses).
 * RAFT_E_NULL: image1, image2, preds, out2 or workspace NULL.  RAFT_E_SHAPE: a non-positive size, pred_stride < 2*B*H*W,
 * B*H*W*3 of 2^31 or more, gamma / census_weight negative or not finite, upstream not finite, accumulate not 0 or 1.
 * RAFT_E_UNSUPPORTED: n_predictions > 64 or an odd pred_stride.  RAFT_E_ALIGN: preds, d_preds or workspace not 8-byte aligned.
 * All checks precede the first launch. */
int64_t raft_census_loss_workspace_bytes(int n_predictions, int B, int H, int W);
int raft_census_loss_f32(const float *image1, const float *image2, const uint8_t *mask, const float *preds, int64_t pred_stride,
                         int n_predictions, int B, int H, int W, double gamma, float census_weight, float upstream,
                         const float *add_to, float *out2, float *d_preds, int accumulate, void *workspace, void *stream);

/* SSIM term of the self-supervised loss and its gradient (csrc/ssim_loss.hip).  Arguments, checks, error
 * codes and their precedence are raft_census_loss_f32's, with ssim_weight in the place of census_weight.  g1 and w_i as there; over
 * the 3x3 window of z (rows first, x = g1), with C1 = (0.01f*255.f)^2, C2 = (0.03f*255.f)^2,
 * interior(z) = 1 <= zx <= W-2 && 1 <= zy <= H-2 and M_i = mask && inside_i && interior:
 *   mx = (sum x) / 9.f, mw = (sum w_i) / 9.f, sxx = (sum (x-mx)^2) / 9.f, sww = (sum (w_i-mw)^2) / 9.f, sxw = (sum (x-mx)*(w_i-mw)) / 9.f
 *   S(z) = ((2*mx*mw + C1) * (2*sxw + C2)) / ((mx*mx + mw*mw + C1) * (sxx + sww + C2)),      D(z) = (1 - S(z)) / 2
 *   ssim_i = sum_z M_i(z) * D(z) / (B*H*W),     w_i = (float)gamma^(n-i-1)
 *   out2[0] = (add_to ? *add_to : 0) + ssim_weight * sum_i w_i * ssim_i  (formed in double, rounded once; add_to may be out2);
 *   out2[1] = ssim_{n-1}
 * d_preds: NULL (value only), or the layout of preds; every element is touched exactly once with
 * upstream * ssim_weight * w_i * d ssim_i -- stored (accumulate == 0) or added to what is there with one float32 addition
 * (accumulate == 1); gaps of a pred_stride larger than 2*B*H*W are not touched.  mask and inside are constants of the gradient; a
 * pixel outside the interior receives gradient from the interior windows that contain it.
 * Deterministic (no atomics, no memset).  `workspace`: raft_ssim_loss_workspace_bytes(n_predictions, B, H, W) bytes (the census
 * entry's layout and size; 0 for sizes the entry refuses).
 * RAFT_E_NULL: image1, image2, preds, out2 or workspace NULL.  RAFT_E_SHAPE: a non-positive size, pred_stride < 2*B*H*W,
 * B*H*W*3 of 2^31 or more, gamma / ssim_weight negative or not finite, upstream not finite, accumulate not 0 or 1.
 * RAFT_E_UNSUPPORTED: n_predictions > 64 or an odd pred_stride.  RAFT_E_ALIGN: preds, d_preds or workspace not 8-byte aligned.
 * All checks precede the first launch. */
int64_t raft_ssim_loss_workspace_bytes(int n_predictions, int B, int H, int W);
int raft_ssim_loss_f32(const float *image1, const float *image2, const uint8_t *mask, const float *preds, int64_t pred_stride,
                       int n_predictions, int B, int H, int W, double gamma, float ssim_weight, float upstream,
                       const float *add_to, float *out2, float *d_preds, int accumulate, void *workspace, void *stream);

/* Self-supervision term and its gradient (csrc/selfsup_loss.hip): the predictions of a student pass over a
 * crop against the flow of a teacher pass over the full frames, held constant.
 *   teacher (B, Ht, Wt, 2) float; teacher_visible NULL or uint8 (B, Ht, Wt), nonzero = the teacher is trusted there.  Both are read
 *   IN PLACE through the window: student pixel (y, x) of slice b faces teacher pixel (y + oy, x + ox).
 *   student_visible NULL or uint8 (B, H, W), nonzero = the student sees the pixel itself: it is left out.
 *   preds: n_predictions flows (B, H, W, 2), prediction i at preds + i * pred_stride (floats).
 * With eps2 = eps*eps rounded once to float32, rho(d) = sqrtf(d*d + eps2), w_i = (float)gamma^(n-i-1) as raft_sequence_loss_f32
 * builds it, t the teacher vector a pixel faces:
 *   used = (teacher_visible == NULL || teacher_visible != 0 there) && (student_visible == NULL || student_visible == 0 there)
 *          && both components of t finite
 *   dist_i  = sum_used sum_k rho(p_i[k] - t[k]) / (B*H*W*2)                     (the divisor counts ALL elements)
 *   out3[0] = (add_to ? *add_to : 0) + weight * sum_i w_i * dist_i  (formed in double, rounded once; add_to may be out3);
 *   out3[1] = dist_{n-1};      out3[2] = (float)(#used / (B*H*W))  (an exact count, divided in double)
 * d_preds: NULL (value only), or the layout of preds; every element is touched exactly once with
 * ((upstream * weight) * w_i) * ((d / rho(d)) * (float)(1 / (B*H*W*2))) where used, else 0 -- stored (accumulate == 0) or added to
 * what is there with one float32 addition (accumulate == 1); gaps of a pred_stride larger than 2*B*H*W are not touched.  The
 * teacher and both masks are constants of the gradient.
 * Deterministic (no atomics, no memset): float64 partial records in `workspace` (raft_selfsup_loss_workspace_doubles()
 * doubles), added in index order by a second one-workgroup launch; the count of used pixels goes through the same records.
 * In this order: RAFT_E_NULL: teacher, preds, out3 or workspace NULL.  RAFT_E_SHAPE: a non-positive size, a window that does not
 * lie inside the teacher (oy < 0, ox < 0, oy + H > Ht, ox + W > Wt), B*Ht*Wt*3 of 2^31 or more, pred_stride < 2*B*H*W, gamma /
 * weight negative or not finite, eps or eps*eps (in float32) not positive and finite, upstream not finite, accumulate not 0 or 1.
 * RAFT_E_UNSUPPORTED: n_predictions > 64 or an odd pred_stride.  RAFT_E_ALIGN: teacher, preds, d_preds or workspace not 8-byte
 * aligned.  All checks precede the first launch. */
int64_t raft_selfsup_loss_workspace_doubles(void);
int raft_selfsup_loss_f32(const float *teacher, const uint8_t *teacher_visible, int Ht, int Wt, int oy, int ox,
                          const uint8_t *student_visible, const float *preds, int64_t pred_stride, int n_predictions, int B, int H,
                          int W, double gamma, float weight, float eps, float upstream, const float *add_to, float *out3,
                          float *d_preds, int accumulate, double *workspace, void *stream);

/* Second-order, edge-aware smoothness of the self-supervised loss and its gradient in ONE launch (csrc/smooth2_loss.hip; DESIGN.md
 * section 24).  image1 and preds as for raft_photometric_loss_f32; image2 and the mask play no part.  s = 1/255,
 * eps2 = eps*eps rounded once to float32, rho(d) = sqrtf(d*d + eps2) and w_i = (float)gamma^(n-i-1) are that entry's, and
 * edge_weight and eps are the first-order term's own parameters.  For image b, prediction p = p_i, component k in {u, v}:
 *   cx(x,y) = expf(-edge_weight * mean_c |s * (image1(x+1,y)_c - image1(x-1,y)_c)|)   for 1 <= x <= W-2 (no term otherwise)
 *   cy(x,y) = the same along y                                                         for 1 <= y <= H-2
 *   Dx_k(x,y) = (p(x+1,y)_k - 2*p(x,y)_k) + p(x-1,y)_k,     Dy_k likewise
 *   sm2_i = [sum cx * rho(Dx_k) + sum cy * rho(Dy_k)] / (B*H*W*2)                      (the divisor counts ALL elements)
 *   out2[0] = (add_to ? *add_to : 0) + smooth2_weight * sum_i w_i * sm2_i  (formed in double, rounded once; add_to may be out2);
 *   out2[1] = sm2_{n-1}
 * The edge weight is the central difference over two pixels (mean over the channels: ((|.| + |.|) + |.|) / 3.f).
 * d_preds: NULL (value only), or the layout of preds.  The gradient is the adjoint written as a gather: with
 * qx_k(x,y) = cx * (Dx_k / rho(Dx_k)), qy_k likewise, both +0 where no stencil is centred,
 *   g_k(x,y) = ((qx_k(x-1,y) - 2*qx_k(x,y)) + qx_k(x+1,y)) + ((qy_k(x,y-1) - 2*qy_k(x,y)) + qy_k(x,y+1))
 *   d_preds_i(x,y)_k  (= or +=)  ((upstream * smooth2_weight) * w_i) * (g_k * (float)(1.0 / (B*H*W*2)))
 * every element touched exactly once -- stored (accumulate == 0) or added to what is there with one float32 addition
 * (accumulate == 1); gaps of a pred_stride larger than 2*B*H*W are not touched.  Where W < 3 and H < 3 the value is add_to (or 0)
 * and the gradient exactly zero; an affine flow has D == 0 everywhere, hence a gradient of exactly zero.
 * Deterministic (no atomics, no memset): float64 partial records in `workspace` (raft_smooth2_loss_workspace_doubles()
 * doubles), added in index order by a second one-workgroup launch.
 * In this order: RAFT_E_NULL: image1, preds, out2 or workspace NULL.  RAFT_E_SHAPE: a non-positive size, B*H*W*3 of 2^31 or
 * more, pred_stride < 2*B*H*W, gamma / smooth2_weight / edge_weight negative or not finite, eps or eps*eps (in float32) not
 * positive and finite, upstream not finite, accumulate not 0 or 1.  RAFT_E_UNSUPPORTED: n_predictions > 64 or an odd pred_stride.
 * RAFT_E_ALIGN: preds, d_preds or workspace not 8-byte aligned.  All checks precede the first launch. */
int64_t raft_smooth2_loss_workspace_doubles(void);
int raft_smooth2_loss_f32(const float *image1, const float *preds, int64_t pred_stride, int n_predictions, int B, int H, int W,
                          double gamma, float smooth2_weight, float edge_weight, float eps, float upstream,
                          const float *add_to, float *out2, float *d_preds, int accumulate, double *workspace, void *stream);

/* The student's view (csrc/student_view.hip): the frames of a self-supervised step, and the teacher's flow
 * with its trust mask, seen through one affine map per slice.  The record of slice b maps the student's pixel indices q = (x, y)
 * to the teacher's, p = M q + o:
 *     px = (m[0] * float(x) + m[1] * float(y)) + o[0],     py = (m[2] * float(x) + m[3] * float(y)) + o[1]
 * every operation rounded on its own.  The student pixel is IN FRAME iff 0 <= px <= Wt - 1 and 0 <= py <= Ht - 1 (a NaN fails), and
 * a map is sampled at (px, py) by the bilinear rule of raft_warp_f32 above.  The host inverts M in double and rounds each
 * element of both once (tf_raft_amd/augment.py). */
typedef struct {
    float m[4];              /* M, row-major: student index -> teacher position */
    float o[2];              /* o = (ox, oy) */
    float inv[4];            /* M^-1, row-major: a teacher vector seen by the student */
    float gain[3], bias[3];  /* per channel (channels beyond the third take the third's), read when colour != 0 */
    int32_t colour;          /* nonzero: v -> min(max(v * gain + bias, 0), 255) */
} RaftViewParams;

/* sizeof(RaftViewParams): the binding checks its mirror against it.  Host-only. */
int raft_view_params_bytes(void);

/*   raft_view_frames_f32: dst[b, y, x, c] = src[b, :, :, c] sampled at the pixel's position, 0.0f in every channel of a pixel out
 *     of frame; then, where the record's colour != 0, min(max(v * gain[c] + bias[c], 0), 255) as two rounded operations and the
 *     clamp (out-of-frame pixels included); with colour == 0 the value is stored as sampled.  src (B, Ht, Wt, C), dst (B, H, W, C).
 *   raft_view_flow_f32: with f = (u, v) the flow (B, Ht, Wt, 2) sampled at the pixel's position,
 *         target[b, y, x] = (inv[0] * u + inv[1] * v, inv[2] * u + inv[3] * v)
 *     (a point the student sees at q lies at p, moves to p + f and is seen at q + M^-1 f).  A tap's weight is the product of its
 *     factors (1 - a or a, 1 - b or b); a tap of weight exactly zero (the x1 side with a == 0, the y1 side with b == 0) counts as
 *     0 and its trust is not asked.  target_visible[b, y, x] (uint8, (B, H, W)) = 1 iff the pixel is in frame, every tap of
 *     nonzero weight has teacher_visible != 0 (uint8 (B, Ht, Wt); NULL = all ones) and both components of the target are finite;
 *     where it is 0 the target is (0, 0).  Under M = I with an integer o both entries copy the window at o.
 * params: B records in DEVICE memory.  The student may be larger than the teacher.  One launch on `stream` each, no atomics, no
 * memset, every output element written exactly once; tap indices are clamped into the teacher whatever a record holds.
 * Errors, in this order: RAFT_E_NULL for a NULL src / flow, params, dst / target or target_visible; RAFT_E_SHAPE for a
 * non-positive size, B * Ht * Wt * C or B * H * W * C (C = 2 for the flow) of 2^31 elements or more, or H above 8 * 65535;
 * RAFT_E_ALIGN for a flow or target that is not 8-byte aligned (read and written as float2).  All checks precede the launch. */
int raft_view_frames_f32(const float *src, const RaftViewParams *params, float *dst, int B, int Ht, int Wt, int H, int W, int C,
                         void *stream);
int raft_view_flow_f32(const float *flow, const uint8_t *teacher_visible, const RaftViewParams *params, float *target,
                       uint8_t *target_visible, int B, int Ht, int Wt, int H, int W, void *stream);

/* Backward of raft_corr_lookup_f32 (CorrBlock.retrieve + bilinear_sampler, corr.py:116-152, 28-69), with TensorFlow's
 * gradient conventions: floor / ceil contribute nothing, clip_by_value passes the gradient on [0, size - 1].
 * d_out: (B, h, w, ld_out) upstream gradient of the lookup output (first levels*(2r+1)^2 channels used).
 * d_coords: (B, h, w, 2), overwritten.  d_pyr: gradient w.r.t. the correlation pyramid in the layout of `pyr`
 * (raft_corr_pyramid_layout), ACCUMULATED (+=) so that the iterations of the loop add up -- zero it before the first
 * call; NULL skips it. */
int raft_corr_lookup_backward_f32(const float *pyr, const int64_t *level_offsets, const float *coords,
                                  const float *d_out, int ld_out, int B, int h, int w, int levels, int radius,
                                  float *d_coords, float *d_pyr, void *stream);

/* dx = dy where y > 0 else 0 (the relu between the convolutions of the update block), n elements. */
int raft_relu_backward_f32(const float *y, const float *dy, float *dx, int64_t n, void *stream);

/* Training-time weight packing on the device (train_step's master weights change every step: reference model.py:134-136), one
 * launch per (kernel, use).  kernel: (kh, kw, cin, cout) Keras layout.  dgrad != 0 packs the kernel of the INPUT gradient
 * K'[ky][kx][co][ci] = K[kh-1-ky][kw-1-kx][ci][co] instead.  mode 0: the kh * kw taps as they are; mode 1 (3x3): the 16 taps
 * G g G^T of F(2x2, 3x3), g = (4, 3) row-major doubles; mode 2 (1x5 / 5x1): the gt taps G' g of F(gt - 4, 5), g = (gt, 5) doubles;
 * float64 accumulation, one rounding.  wp: [taps][kpad / 4][npad][4] as raft_conv2d_f32 / raft_conv2d_winograd_f32 /
 * raft_conv1d_winograd{,4}_f32 consume it (zero beyond the kernel's channels); bias_out: npad floats (bias, or zeros when bias is
 * NULL or dgrad is set). */
int raft_pack_train_conv_f32(const float *kernel, const float *bias, int kh, int kw, int cin, int cout, int dgrad, int mode,
                             const double *g, int gt, int kpad, int npad, float *wp, float *bias_out, void *stream);

/* Keras Conv2D (stride 1, 'same'; kh x kw in {1x1, 3x3, 1x5, 5x1}) backward w.r.t. kernel and bias:
 *   d_kernel[ky][kx][ci][co] = sum_pixels x[b, y + ky - (kh-1)/2, x + kx - (kw-1)/2, ci] * dy[b, y, x, co]   (Keras layout)
 *   d_bias[co] = sum_pixels dy[b, y, x, co]                                                       (NULL skips it)
 * x: (B, H, W, ldx) with cin channels used, dy: (B, H, W, ldy) with cout channels used; cin, cout, ldx, ldy multiples
 * of 4.  fp32 MFMA over pixel slices + an ordered second-stage sum (deterministic); workspace:
 * raft_conv2d_wgrad_workspace_floats() floats.  The gradient w.r.t. the INPUT is raft_conv2d_f32 of dy with the flipped,
 * transposed kernel (tf_raft_amd/packing.py pack_conv_dgrad). */
int64_t raft_conv2d_wgrad_workspace_floats(int cin, int cout, int B, int H, int W, int kh, int kw);
int raft_conv2d_wgrad_f32(const float *x, int ldx, int cin, const float *dy, int ldy, int cout, int B, int H, int W,
                          int kh, int kw, float *d_kernel, float *d_bias, float *workspace, void *stream);
/* The same gradient summed over nseg (1..32) pairs (xs[i], dys[i]) of identical geometry in ONE pixel reduction; xs / dys are
 * HOST arrays of device pointers (copied into the kernel arguments).  The iterations of a training step share the update
 * block's weights (reference model.py:91-109): one launch over all of them replaces nseg launches, nseg second-stage sums and
 * nseg - 1 accumulations per layer.  Workspace: raft_conv2d_wgrad_workspace_floats(cin, cout, B * nseg, H, W, kh, kw). */
int raft_conv2d_wgrad_multi_f32(const float *const *xs, const float *const *dys, int nseg, int ldx, int cin, int ldy, int cout,
                                int B, int H, int W, int kh, int kw, float *d_kernel, float *d_bias, float *workspace, void *stream);

/* ---- second slice: everything one BasicUpdateBlock call needs (tf_raft_amd/grad.py basic_update_block_backward) */

/* relu(Conv2D(7, 7, Cin = 2 -> cout)) of the flow (update.py:93, 76): kernel (98, cout) = Keras (7,7,2,cout) flattened,
 * cout in {64, 128}; out (B, H, W, ldo).  The inference loop runs this kernel inside raft_update_*_f32. */
int raft_conv7x7_c2_f32(const float *flow, const float *kernel, const float *bias, int cout, int B, int H, int W,
                        float *out, int ldo, void *stream);
/* Its backward for an upstream gradient dy that already carries the relu mask: d_flow (B, H, W, 2), d_kernel (98, cout),
 * d_bias (cout).  Deterministic; workspace raft_conv7x7_c2_wgrad_workspace_floats(cout) floats. */
int64_t raft_conv7x7_c2_wgrad_workspace_floats(int cout);
int raft_conv7x7_c2_backward_f32(const float *flow, const float *dy, int ldy, const float *kernel, int cout, int B, int H,
                                 int W, float *d_flow, float *d_kernel, float *d_bias, float *workspace, void *stream);

/* SepConvGRU gates (update.py:51-67) as separate kernels, so that the training forward keeps z, r, q:
 *   zr: a_zr (M, 2C) = [convz | convr] pre-activations -> z = sigmoid, r = sigmoid, rh = r * h        (all (M, C))
 *   q : a_q (n) -> q = tanh(a_q), h_new = (1 - z) h + z q
 * and their backward:
 *   q_backward: d_h_new -> dz_pre = d (q - h) z (1 - z), dq_pre = d z (1 - q^2), dh = d (1 - z)      (dh overwritten)
 *   r_backward: d_rh -> dr_pre = d h r (1 - r), dh += d r                                           (dh accumulated) */
int raft_gru_gate_zr_f32(const float *a_zr, const float *h, int C, int64_t M, float *z, float *r, float *rh, void *stream);
int raft_gru_gate_q_f32(const float *a_q, const float *z, const float *h, int64_t n, float *q, float *h_new, void *stream);
int raft_gru_gate_q_backward_f32(const float *d_h_new, const float *z, const float *q, const float *h, int64_t n,
                                 float *dz_pre, float *dq_pre, float *dh, void *stream);
int raft_gru_gate_r_backward_f32(const float *d_rh, const float *r, const float *h, int64_t n, float *dr_pre, float *dh,
                                 void *stream);
/* out = alpha * a + beta * b (b may be NULL): gradient accumulation where two branches meet, the 0.25 of the mask head. */
int raft_axpby_f32(float alpha, const float *a, float beta, const float *b, float *out, int64_t n, void *stream);

/* Backward of raft_upsample_convex_f32 (RAFT.upsample_flow, model.py:39-66): d_up (B, 8h, 8w, 2) -> d_flow (B, h, w, 2)
 * and d_mask (B, h, w, 576), both overwritten.  Deterministic (the scatter into the 3x3 neighbours is a gather over a
 * per-pixel, per-tap scratch); workspace raft_upsample_convex_backward_workspace_floats() floats. */
int64_t raft_upsample_convex_backward_workspace_floats(int B, int h, int w);
int raft_upsample_convex_backward_f32(const float *flow, const float *mask, const float *d_up, int B, int h, int w,
                                      float *d_flow, float *d_mask, float *workspace, void *stream);

/* ---- optimizer side of train_step (model.py:131-136): tf.clip_by_global_norm + tfa.optimizers.AdamW (tfa 0.11.1) */

/* *out (+)= sum of x[i]^2 in float64, deterministic; accumulate != 0 adds to the value already in *out (the global norm
 * runs over every gradient tensor).  workspace: raft_sumsq_workspace_doubles() doubles. */
int64_t raft_sumsq_workspace_doubles(void);
int raft_sumsq_f32(const float *x, int64_t n, int accumulate, double *out, double *workspace, void *stream);
/* One AdamW step on one tensor, tensorflow-addons 0.11.1 semantics: var -= weight_decay * var (decoupled, not scaled by
 * the learning rate); g = grad * clip_norm / max(sqrt(*global_norm_sq), clip_norm) (global_norm_sq NULL: no clipping);
 * m, v Adam moments; var -= lr_t * m / (sqrt(v) + epsilon) with lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) from the caller. */
int raft_adamw_step_f32(float *var, const float *grad, float *m, float *v, int64_t n, float lr_t, float beta1, float beta2,
                        float epsilon, float weight_decay, const double *global_norm_sq, float clip_norm, void *stream);
/* The same two steps over MANY tensors per launch (host arrays of device pointers and element counts, copied into the kernel
 * arguments in chunks of 64): a RAFT model has 154 trainable tensors, i.e. 154 x 3 launches per training step otherwise.
 * raft_sumsq_multi_f32: *out = sum over all tensors of the sum of squares (float64, ordered: deterministic), workspace
 * raft_sumsq_multi_workspace_doubles(count) doubles.  raft_adamw_step_multi_f32: raft_adamw_step_f32's arithmetic per element. */
int64_t raft_sumsq_multi_workspace_doubles(int count);
int raft_sumsq_multi_f32(const float *const *xs, const int64_t *ns, int count, double *out, double *workspace, void *stream);
int raft_adamw_step_multi_f32(float *const *vars, const float *const *grads, float *const *ms, float *const *vs, const int64_t *ns,
                              int count, float lr_t, float beta1, float beta2, float epsilon, float weight_decay,
                              const double *global_norm_sq, float clip_norm, void *stream);

/* ---- backward of the volume build and of the state preparation */

/* Generic strided batched GEMM on fp32 MFMA: C[b][m][n] = alpha * sum_k A(b,m,k) B(b,k,n) + beta * C[b][m][n] with
 * A(b,m,k) = a[b*sab + m*sam + k*sak], B(b,k,n) = b[b*sbb + k*sbk + n*sbn], C row-major (ldc) with batch stride scb. */
int raft_gemm_f32(const float *a, int64_t sab, int64_t sam, int64_t sak, const float *b, int64_t sbb, int64_t sbk, int64_t sbn,
                  float *c, int64_t scb, int ldc, int batch, int M, int N, int K, float alpha, float beta, void *stream);
/* Backward of raft_corr_build_f32 (CorrBlock.__init__, corr.py:100-114, 154-162): d_pyr (layout of the pyramid) ->
 * d_fmap1, d_fmap2 (B, h, w, C), overwritten.  fmap2_pyr: the pooled-fmap2 workspace the forward filled; workspace: as
 * many floats again (raft_corr_build_workspace_floats). */
int raft_corr_build_backward_f32(const float *fmap1, const float *fmap2_pyr, const float *d_pyr, const int64_t *level_offsets,
                                 int B, int h, int w, int C, int levels, float *d_fmap1, float *d_fmap2, float *workspace,
                                 void *stream);
/* model.py:84-86 backward: d_cnet (M, hdim + cdim) = [d_net0 * (1 - net0^2) | d_inp where inp > 0]. */
int raft_prepare_state_backward_f32(const float *net0, const float *inp, const float *d_net0, const float *d_inp, int hdim,
                                    int cdim, int64_t M, float *d_cnet, void *stream);

/* ---- normalisation layers of the encoders in training form (extractor.py:6-16) */

/* x viewed as (G groups, P pixels, C channels): tfa InstanceNormalization = (G = B, P = H*W), Keras BatchNormalization with
 * batch statistics = (G = 1, P = B*H*W); biased variance, y = (x - mean) * rstd * gamma + beta [relu], rstd = 1/sqrt(var + eps).
 * mean, rstd (and var when non-NULL): (G, C), kept for the backward / the moving statistics.  Deterministic float64 sums.
 * workspace: raft_norm_workspace_doubles(G, C) doubles. */
int64_t raft_norm_workspace_doubles(int G, int C);
int raft_norm_forward_f32(const float *x, int G, int64_t P, int C, const float *gamma, const float *beta, float eps, int relu,
                          float *y, float *mean, float *rstd, float *var, double *workspace, void *stream);
/* dy is the gradient at the norm's linear output (apply raft_relu_backward_f32 first when relu was fused). */
int raft_norm_backward_f32(const float *x, const float *dy, const float *mean, const float *rstd, const float *gamma, int G,
                           int64_t P, int C, float *dx, float *dgamma, float *dbeta, double *workspace, void *stream);
/* out = relu(alpha * a + beta * b): the residual join of a ResBlock (extractor.py:49). */
int raft_axpby_relu_f32(float alpha, const float *a, float beta, const float *b, float *out, int64_t n, void *stream);

/* bf16 storage of the training tape (BASELINE configs[4]: "bf16" = bf16 storage, fp32 arithmetic): round-to-nearest-even
 * narrowing of n floats into n 16-bit words and the exact widening back. */
int raft_f32_to_bf16(const float *x, void *y, int64_t n, void *stream);
int raft_bf16_to_f32(const void *x, float *y, int64_t n, void *stream);

/* Keras Dropout in training mode (reference extractor.py:109-111, 127-128): y = x * keep / (1 - rate) with keep ~
 * Bernoulli(1 - rate) from a counter-based generator of (seed, element index); mask[i] = keep (bytes).  The backward is
 * dx = dy * mask / (1 - rate).  TensorFlow's random stream is not reproduced: parity of this layer is distributional. */
int raft_dropout_f32(const float *x, int64_t n, float rate, uint64_t seed, float *y, unsigned char *mask, void *stream);
int raft_dropout_backward_f32(const float *dy, const unsigned char *mask, int64_t n, float rate, float *dx, void *stream);

/* Backward of raft_upflow8_f32 (corr.py:93-96): d_up (B, 8h, 8w, 2) -> d_flow (B, h, w, 2), a deterministic gather. */
int raft_upflow8_backward_f32(const float *d_up, int B, int h, int w, float *d_flow, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RAFT_HIP_H_ */

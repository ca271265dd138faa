/*
 * libhulkkp — C ABI of the MI355X-native keypoint-heatmap CNN hot path.
 *
 * Replaces the device work the reference hands to PyTorch/cuDNN implicitly
 * (reference: vainaviv/hulk-keypoints, Python only, no FFI of its own —
 * SURVEY §8(b)).  Each entry point cites the reference code whose device work
 * it performs.  The Python host layer (hulk-keypoints_amd/hkp/) binds these
 * with ctypes and re-exposes the reference's own call surface
 * (KeypointsGauss, gauss_2d_batch, Prediction, train.py forward/fit).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch or C++ types cross it.
 *   - Activations are NHWC fp32, conv weights KRSC ([Cout][R][S][Cin]) fp32,
 *     except the stem, which reads the reference's NCHW image and OIHW weight.
 *   - The caller owns and allocates every buffer (device pointers).  The
 *     library never allocates, never synchronises; every launch goes on the
 *     stream argument (a hipStream_t; NULL = legacy default stream).
 *   - Return: 0 ok; <0 bad argument (see hkp_last_error()); >0 a hipError_t.
 *   - All reductions are deterministic (fixed order, no float atomics), so
 *     results are bitwise reproducible run to run.
 */
#ifndef HULKKP_H
#define HULKKP_H

#include <stddef.h>
#include <stdint.h>

#include "hkp_jpeg.h"   /* hkpj_geom: the host half of the hybrid JPEG decode */

#ifdef __cplusplus
extern "C" {
#endif

#define HKP_OK 0
#define HKP_ERR_BAD_ARG (-1)
#define HKP_ERR_UNSUPPORTED (-2)

#define HKP_LAYOUT_NHWC 0
#define HKP_LAYOUT_NCHW 1

#define HKP_LOSS_BCE 0
#define HKP_LOSS_MSE 1

typedef void* hkp_stream_t;

/* thread-local message of the last failing call on this thread */
const char* hkp_last_error(void);
/* "hulkkp <version> gfx950" */
const char* hkp_version(void);

/* ---------------------------------------------------------------- conv ---- */
typedef struct hkp_conv_desc {
    int32_t n, h, w, c;             /* input batch, height, width, channels            */
    int32_t k, r, s;                /* output channels, filter height, filter width    */
    int32_t stride, pad, dilation;  /* symmetric                                        */
    int32_t in_layout;              /* HKP_LAYOUT_NHWC, or HKP_LAYOUT_NCHW (stem only)  */
    int32_t tile;                   /* x3 / fp16 conv tile policy, HKP_TILE_* (0: the
                                       planner).  Per call — no process-global state */
} hkp_conv_desc;

/* Tile policies of the packed-operand convs (hkp_conv2d_fwd_x3 / _fwd_f16 /
 * _bwd_data_x3 / _bwd_data_x3_strided).  AUTO: fewest rounds of blocks over the
 * CUs weighted by the measured per-column cost of each tile width (256x256,
 * 256x128, 256x64), data-parallel or stream-K (with a workspace).  The others
 * force one kernel body (for tests and tuning; outputs agree to fp32 summation
 * order): NO_SK never stream-K; SK stream-K wherever a tile split helps;
 * 256 = 256x256 16x16x32 (Cout % 256 == 0); 128_MF16 / 128_MF32 = 256x128 with
 * 16x16x32 / 32x32x16 MFMAs; 64_PAIR = 256x64, two blocks per CU. */
#define HKP_TILE_AUTO 0
#define HKP_TILE_NO_SK 1
#define HKP_TILE_SK 2
#define HKP_TILE_256 3
#define HKP_TILE_128_MF16 4
#define HKP_TILE_128_MF32 5
#define HKP_TILE_64_PAIR 6
#define HKP_TILE_RESERVED_7 7         /* retired: the persistent conv (measured slower */
#define HKP_TILE_RESERVED_8 8         /* than the one-tile grid); rejected with HKP_ERR_ARG */
#define HKP_TILE_256_TAIL 9           /* 256x256; tiles past the last full round as split-K segments */
#define HKP_TILE_HALO 10              /* 8x32-pixel halo tiles (stride-1 3x3, pad = dil = 1, Ho%8 = Wo%32 = 0;
                                         the default there under AUTO and 256_TAIL when the
                                         input has 64 channels) */
#define HKP_TILE_AUTO_A3 12           /* the round-4 planner: AUTO without its plain-fp16 DUO
                                         choices (K-depth 64, 128-wide outputs) */
#define HKP_TILE_256_A3 11            /* 256x256 on the A3 body (A ring 3 stages deep, B ring 2: an A
                                         line has two K-steps to land) + the split-K tail of 9 */
#define HKP_TILE_DUO 13               /* plain fp16 (hkp_conv2d_fwd_f16 / _f16_bn) only: 256x128 tiles,
                                         two 4-wave blocks per CU (one block's fill and epilogue
                                         beside the other's K loop); Cout % 128 == 0; other
                                         operand layouts plan as AUTO */
#define HKP_TILE_RESERVED_14 14      /* retired: the persistent A3 body (measured slower on every shape,
                                         round 5); rejected with HKP_ERR_BAD_ARG */
#define HKP_TILE_192_A3 15            /* packed operands (x3 forward / dgrad), Cout % 256 == 0: the A3
                                         body on 192 x 256 tiles (one partial round of 256-row
                                         tiles on many fewer tiles than CUs); its BN partials are
                                         per 96-row tile: hkp_bn_finalize(..., tile_rows = 96, ...)
                                         over ceil(M / 96) tiles.  Other shapes plan as AUTO */
#define HKP_TILE_160_A3 16            /* the same on 160 x 256 tiles (waves 2 x 4; 160 x 128 where
                                         Cout % 256 != 0, Cout % 128 == 0), BN partials per 80-row
                                         tile (tile_rows = 80) */
#define HKP_TILE_MIX_A3 17            /* the same operands, Cout % 256 == 0, more than one round of 256 x 256
                                         tiles: one launch whose blocks run 256-, then 192-, then
                                         160-row A3 tiles (conv_x3_a3_mix_kernel), every CU tall
                                         tiles first and one shorter tile last, so that the last
                                         round is filled — hkp_conv_x3_mix_plan has the regions.  The
                                         output bits are HKP_TILE_256_A3's; the BN partial list is
                                         segmented (128-, 96-, 80-row tiles: hkp_conv_x3_stat_layout,
                                         hkp_bn_finalize_seg).  No tail, no workspace.  Never AUTO's
                                         own choice; other shapes plan as AUTO */

/* output spatial size: (h + 2*pad - dilation*(r-1) - 1)/stride + 1 */
int hkp_conv_out_hw(const hkp_conv_desc* d, int32_t* ho, int32_t* wo);

/* number of BatchNorm statistic tiles the conv epilogue emits; the
 * stat_partials buffer holds tiles * k * 2 floats */
int64_t hkp_conv_stat_tiles(const hkp_conv_desc* d);

/* y[n,ho,wo,k] = sum_{r,s,c} x[n, ho*st-pad+r*dil, wo*st-pad+s*dil, c] * w[k,r,s,c]
 * (zero padding, no bias) on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces: conv3x3 src/resnet.py:20-37 (BasicBlock :45,48; Bottleneck :80),
 *           1x1 convs src/resnet.py:77,86 and downsample :184-188,
 *           stem conv src/resnet.py:137,199 (in_layout NCHW, w OIHW).
 * If stat_partials != NULL the epilogue also writes per-tile per-channel
 * (sum, sum of squared deviations from the tile mean) for train-mode BN. */
int hkp_conv2d_fwd(const hkp_conv_desc* d, const float* x, const float* w, float* y,
                   float* stat_partials, hkp_stream_t stream);

/* The f16x3 conv of the main path (same conv and epilogue as hkp_conv2d_fwd;
 * fp32-class accuracy) on operands pre-split into the "packed split" layout:
 * per pixel (weights: per output channel and filter tap) and per 32-channel
 * group one 128-B line [hi 32 | lo 32] (fp16 bit patterns), hi = f16(v),
 * lo = f16(v - hi); the conv sums hi*hi + hi*lo + lo*hi in fp32.
 *   x_split[n*h*w][c/32][64]   written by hkp_bn_apply / hkp_bn_relu_maxpool with
 *                              split_passes = 3 (v = the activation),
 *   w_split[k][r*s][c/32][64]  written by hkp_weight_pack_x3 from KRSC fp32, each
 *                              output channel scaled by a power of two (max|w| ->
 *                              [2^13, 2^14)); w_inv_scale[k] = the inverse, which
 *                              the conv applies to its output.
 * Needs c % 32 == 0 and k % 64 == 0.  Replaces the same convs as hkp_conv2d_fwd. */
int hkp_weight_pack_x3(int32_t k, int32_t rsc, int32_t c, const float* w, uint16_t* w_split, float* w_inv_scale,
                       hkp_stream_t stream);
int hkp_conv2d_fwd_x3(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* w_split,
                      const float* w_inv_scale, float* y, float* stat_partials, void* sk_workspace,
                      int64_t sk_ws_bytes, hkp_stream_t stream);
/* Stream-K workspace of the x3 convs (hkp_conv2d_fwd_x3, hkp_conv2d_bwd_data_x3,
 * hkp_conv2d_bwd_data_x3_strided; nullable: then every launch is one tile per
 * block).  With it, a launch whose tiles fill the CUs poorly (e.g. 300 tiles on
 * 256 CUs) splits tiles x K-steps evenly over one block per CU and sums each split
 * tile's fp32 segments in fixed segment order (deterministic).  Its first 64 KiB
 * are arrival counters that must be ZERO before the first call; every call
 * leaves them zero (allocate once, zeroed, per stream: calls on one workspace
 * must not run concurrently).  Size: hkp_conv_x3_sk_workspace_bytes(). */
int64_t hkp_conv_x3_sk_workspace_bytes(void);
/* hkp_conv2d_fwd_x3 with a chosen subset of the three f16x3 products (inference
 * precision modes between config C4's plain fp16 and f16x3; same operands,
 * outputs and workspace).  products: HKP_X3_ALL = hkp_conv2d_fwd_x3;
 * HKP_X3_W16 = hi_x*hi_w + lo_x*hi_w (the weights rounded to fp16 after their
 * per-channel power-of-two scale, the activation kept to ~2^-22); HKP_X3_X16 =
 * hi_x*hi_w + hi_x*lo_w (the activation rounded to fp16, the weights kept).
 * Two fp16 MFMAs per 32 channels instead of three.  Replaces the same convs as
 * hkp_conv2d_fwd_x3 (src/resnet.py:20-37,77,86,184-188). */
#define HKP_X3_ALL 3
#define HKP_X3_W16 2
#define HKP_X3_X16 4
int hkp_conv2d_fwd_x3_products(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* w_split,
                               const float* w_inv_scale, int32_t products, float* y, float* stat_partials,
                               void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream);
/* Inference: hkp_conv2d_fwd_x3 whose input is the producer conv's raw output,
 * with the producer's train-mode BN + ReLU applied in the conv itself — the
 * bn_apply pass between a BasicBlock's / Bottleneck's inner convs
 * (src/resnet.py:46-48 / 80-86: relu(bn1(conv1 x)) feeding conv2) disappears.
 * x_raw: fp32 NHWC [n][h][w][c]; in_scale_shift: [2c] scale | shift from
 * hkp_bn_finalize (or hkp_bn_finalize_ranks) of that output; the A operand is
 * relu(x * scale + shift) with bn_apply's arithmetic (two roundings), split as
 * hkp_bn_apply(split = 3) would write it — so y is bit-identical to hkp_bn_apply
 * followed by hkp_conv2d_fwd_x3 with the same d->tile and workspace.  Runs
 * where that unfused launch runs the halo-tile body (stride-1 3x3, pad = dil =
 * 1, Ho % 8 == 0, Wo % 32 == 0) — the kernel hkp_conv_kernel_name names for
 * HKP_KOP_FWD_X3, with "_bnin" before "_kernel"; other launches return
 * HKP_ERR_BAD_ARG. */
int hkp_conv2d_fwd_x3_bnin(const hkp_conv_desc* d, const float* x_raw, const float* in_scale_shift,
                           const uint16_t* w_split, const float* w_inv_scale, float* y, float* stat_partials,
                           void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream);
/* The plain-fp16 form (config C4): x_raw_f16 is the producer's fp16 output,
 * relu(x * scale + shift) rounded to fp16 as hkp_bn_apply_f16 writes it; the
 * halo-tile body only. */
int hkp_conv2d_fwd_f16_bnin(const hkp_conv_desc* d, const uint16_t* x_raw_f16, const float* in_scale_shift,
                            const uint16_t* w_f16, const float* w_inv_scale, uint16_t* y_f16, float* stat_partials,
                            void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream);
/* Plain-fp16 conv (BASELINE config C4, "fp16 with MFMA"): the same LDS-DMA
 * kernel family as hkp_conv2d_fwd_x3 with one fp16 product per MAC (fp32
 * accumulation).  x_f16: NHWC fp16 [n][h][w][c] (a producer's split_passes = 1
 * output); w_f16: KRSC fp16 written by hkp_weight_pack_f16 (each output channel
 * scaled by a power of two, max|w| -> [2^13, 2^14); w_inv_scale[k] the inverse).
 * Output y_f16: fp16 NHWC (autocast semantics; the tile is staged in LDS and
 * written as whole 16-B row chunks); BN partials from the fp32 accumulators.
 * Needs c % 64 == 0 and k % 64 == 0.  Stream-K workspace as hkp_conv2d_fwd_x3. */
int hkp_weight_pack_f16(int32_t k, int32_t rsc, const float* w, uint16_t* w_f16, float* w_inv_scale,
                        hkp_stream_t stream);
int hkp_conv2d_fwd_f16(const hkp_conv_desc* d, const uint16_t* x_f16, const uint16_t* w_f16,
                       const float* w_inv_scale, uint16_t* y_f16, float* stat_partials, void* sk_workspace,
                       int64_t sk_ws_bytes, hkp_stream_t stream);
/* The plain-fp16 conv with the output's train-mode BN apply fused into its
 * epilogue (config C4's Bottleneck tail, src/resnet.py:106-110: bn3, + residual,
 * ReLU): out_f16 = [relu](y*scale + shift [+ res | + res*rscale + rshift]) on the
 * fp16-rounded conv output y — hkp_bn_apply_f16's arithmetic, so the result is
 * what hkp_conv2d_fwd_f16 + hkp_bn_apply_f16 give with the same scale_shift [2k].
 * y is never written.  res_f16 [n*ho*wo][k] (nullable), res_scale_shift [2k]
 * (nullable: raw residual).  The scale/shift must be known before the conv:
 * eval-mode BN, or train-mode statistics from the input's second moments
 * (hkp_gram_f16 + hkp_bn_from_gram, 1x1 convs).  Stream-K workspace as
 * hkp_conv2d_fwd_x3. */
int hkp_conv2d_fwd_f16_bn(const hkp_conv_desc* d, const uint16_t* x_f16, const uint16_t* w_f16,
                          const float* w_inv_scale, const float* scale_shift, const uint16_t* res_f16,
                          const float* res_scale_shift, int32_t relu, uint16_t* out_f16, void* sk_workspace,
                          int64_t sk_ws_bytes, hkp_stream_t stream);
/* Train-mode BN statistics of a 1x1 conv's output y = W a without a pass over y
 * (replaces the batch statistics of bn3, src/resnet.py:106-108, for
 * hkp_conv2d_fwd_f16_bn): hkp_gram_f16 reduces the fp16 input a [m][c] (c % 64
 * == 0, c <= 2048) to its mean mu [c] and second moments E = a^T a / m [c][c]
 * (fp64; fp32 MFMA partials over row splits of <= 16 k rows, merged in fp64 in
 * fixed order; workspace hkp_gram_f16_workspace_bytes(m, c)); hkp_bn_from_gram
 * takes, per output channel k of the packed fp16 weight w_f16 [k][c] (x
 * w_inv_scale[k], hkp_weight_pack_f16 — the weights the conv multiplies with),
 * mean = w.mu and var = w^T E w - mean^2 (fp64), and writes hkp_bn_finalize's
 * outputs from them
 * (scale_shift, mean_invstd (nullable), running stats with the unbiased
 * variance, num_batches_tracked += 1); workspace hkp_bn_from_gram_workspace_bytes(k,
 * c) (per-column-block partial sums, merged in fixed order). */
int64_t hkp_gram_f16_workspace_bytes(int64_t m, int32_t c);
int hkp_gram_f16(int64_t m, int32_t c, const uint16_t* a, double* mean, double* second, void* workspace,
                 int64_t ws_bytes, hkp_stream_t stream);
int64_t hkp_bn_from_gram_workspace_bytes(int32_t k, int32_t c);
int hkp_bn_from_gram(int32_t k, int32_t c, int64_t count, const double* mean, const double* second,
                     const uint16_t* w_f16, const float* w_inv_scale, const float* gamma, const float* beta,
                     float momentum, float eps, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float* scale_shift, float* mean_invstd, void* workspace,
                     int64_t ws_bytes, hkp_stream_t stream);
/* The kernel a launch with descriptor d runs — its template name as rocprofv3
 * reports it (e.g. "conv_x3_kernel<256, false, false, 16, false, 3>"), for
 * profiling / roofline attribution — the first launch of hkp_conv_x3_launch_plan.
 * op: HKP_KOP_*; stream_k_ok: whether the call passes a stream-K workspace.  Writes at most len bytes (NUL-terminated);
 * returns the name's length, or < 0 on bad args. */
#define HKP_KOP_FWD_X3 0
#define HKP_KOP_DGRAD_X3 1
#define HKP_KOP_FWD_F16 2
#define HKP_KOP_STEM_X3 3
#define HKP_KOP_WGRAD_X3 4
#define HKP_KOP_FWD_X3_W16 5   /* hkp_conv2d_fwd_x3_products(HKP_X3_W16) */
#define HKP_KOP_FWD_X3_X16 6   /* hkp_conv2d_fwd_x3_products(HKP_X3_X16) */
#define HKP_KOP_STEM_X3_IMAGE 7     /* hkp_conv2d_fwd_stem_x3_image, fp32 NCHW image */
#define HKP_KOP_STEM_X3_IMAGE_U8 8  /* hkp_conv2d_fwd_stem_x3_image, uint8 NHWC batch */
#define HKP_KOP_FWD_F16_BN 9        /* hkp_conv2d_fwd_f16_bn: its fused output BN rules the halo-tile body out */
int32_t hkp_conv_kernel_name(const hkp_conv_desc* d, int32_t op, int32_t stream_k_ok, char* buf, int32_t len);
/* Rows per BN statistic tile of a forward conv (op HKP_KOP_FWD_X3 / _W16 / _X16 /
 * _F16) with this descriptor, from the body the launcher picks for it: 96 on the
 * 192-row A3 tiles (HKP_TILE_192_A3), 80 on the 160-row ones (HKP_TILE_160_A3), else
 * 128 (hkp_conv_stat_tiles' tiles) — also where such a policy is routed to another
 * body (the halo-tile body writes 128-row partials).  stat_partials then holds
 * ceil(M / rows) * k * 2 floats, and hkp_bn_finalize / _ws / hkp_bn_stats take
 * tile_rows = rows (src/resnet.py:46,49: the statistics are the same).  For a
 * HKP_TILE_MIX_A3 launch this is the first segment's rows: use the layout below.  Any other
 * op answers 128 (a dgrad, and HKP_KOP_FWD_F16_BN, whose launch writes no partials); the
 * layout query rejects them. */
int32_t hkp_conv_x3_stat_tile_rows(const hkp_conv_desc* d, int32_t op);
/* The BN partial list of that conv as segments: segments[2i] = rows per statistic
 * tile of segment i, segments[2i + 1] = its tiles (room for 3 segments: 6 values);
 * returns the segment count (1 for every body but the mixed-height launch, whose
 * regions write ceil(region rows / (tile height / 2)) tiles each, in region
 * order), or a negative HKP_ERR_*.  stat_partials holds sum(tiles) * k * 2
 * floats; hkp_bn_finalize_seg / hkp_bn_stats_seg take the table as it is. */
int32_t hkp_conv_x3_stat_layout(const hkp_conv_desc* d, int32_t op, int32_t* segments);
/* The regions of a HKP_TILE_MIX_A3 launch over m output rows and n_tiles column tiles
 * on cus CUs (host arithmetic only; the launcher uses the device's CU count): a, b, c
 * rounds of 256-, 192-, 160-row tiles, cus / n_tiles m-tiles to a round, minimising
 * 16 a + 12 b + 10 c subject to (cus / n_tiles) (256 a + 192 b + 160 c) >= m (ties:
 * most 256-row rounds, then most 192-row ones); every region but the last
 * non-empty one holds whole rounds, the last the tiles the rows left need.
 * out[HKP_MIX_PLAN_LEN] = cost | rounds[3] | m-tiles[3] | first row[3] | first BN
 * partial tile[3] | BN partial tiles in all.  Returns the non-empty regions (0: no
 * plan, n_tiles > cus) or a negative HKP_ERR_*. */
#define HKP_MIX_PLAN_LEN 14
int32_t hkp_conv_x3_mix_plan(int64_t m, int32_t n_tiles, int32_t cus, int32_t* out);
/* The launches of the conv entry point op (HKP_KOP_*) for descriptor d on cus CUs (0: the
 * device's, or 256 without a device), with (stream_k_ok) or without a stream-K workspace:
 * the plan the launcher itself runs (host arithmetic only).  Returns the number of
 * launches — 1; 2 for the HKP_TILE_256_TAIL form, the full rounds (no blocks, and not
 * started, where the grid is less than a round) and then conv_x3_tail_kernel; 0 where the
 * entry point rejects the shape (Cout % 64, no whole line of input channels), launch 0 then
 * holding only the planner's kernel — or a negative HKP_ERR_*.  For launch launch_index it
 * writes the kernel's name as hkp_conv_kernel_name does (which names launch 0) and
 * out[HKP_X3_LAUNCH_PLAN_LEN] = kernel id (HKP_X3K_*; -1: a wgrad kernel) | blocks |
 * threads | n_tiles (column tiles) | nks (K-steps per tile) | sk_units | sk_one | mt0 |
 * main_blocks | tail_groups | tail_mt0 | tail_units | mix_b1 | mix_b2 | mix_m1 | mix_m2 |
 * mix_p1 | mix_p2 | stagger_blocks | DUO stagger in ns (-1: not a DUO launch) | uses the
 * workspace | workspace bytes it uses | then, the same for every launch: the BN partial
 * segments (rows, tiles) x 3 | their count | the CU count used | M | 256-row m-tiles | tile
 * width | tile height.  A strided dgrad runs one such plan per output phase and has no
 * descriptor here; HKP_KOP_WGRAD_X3 fills the name, blocks, threads and M only.  The BN
 * partial segments are hkp_conv_x3_stat_layout's when stream_k_ok is set. */
#define HKP_X3_LAUNCH_PLAN_LEN 34
#define HKP_X3K_TILE_256 0           /* conv_x3_kernel<256, false, false, 16, false, P> */
#define HKP_X3K_TILE_128_MF16 1      /* conv_x3_kernel<128, false, false, 16, false, P> */
#define HKP_X3K_TILE_128_MF32 2      /* conv_x3_kernel<128, false, false, 32, false, P> */
#define HKP_X3K_PAIR_64 3            /* conv_x3_kernel<64, false, true, 16, false, P> */
#define HKP_X3K_SK_128 4             /* conv_x3_kernel<128, false, false, 16, true, P> */
#define HKP_X3K_SK_64 5              /* conv_x3_kernel<64, false, false, 32, true, P> */
#define HKP_X3K_A3 6                 /* conv_x3_a3_kernel<P> */
#define HKP_X3K_A3_192 7             /* conv_x3_a3_192_kernel<P> */
#define HKP_X3K_A3_160 8             /* conv_x3_a3_160_kernel<P> */
#define HKP_X3K_A3_160X128 9         /* conv_x3_a3_160x128_kernel<P> */
#define HKP_X3K_A3_MIX 10            /* conv_x3_a3_mix_kernel<P> */
#define HKP_X3K_TAIL 11              /* conv_x3_tail_kernel<256, P> */
#define HKP_X3K_HALO 12              /* conv_x3_halo_kernel<P> */
#define HKP_X3K_HALO_BNIN 13         /* conv_x3_halo_bnin_kernel<P> (hkp_conv2d_fwd_x3_bnin / _f16_bnin) */
#define HKP_X3K_DUO 14               /* conv_x3_duo_kernel<1> */
#define HKP_X3K_STEM_PAIR 15         /* conv_x3_kernel<64, true, true, 16, false, 3> */
#define HKP_X3K_STEM_PATCH 16        /* conv_x3_stem_patch_kernel<0> */
#define HKP_X3K_STEM_PATCH_IMAGE 17  /* conv_x3_stem_patch_kernel<1> */
#define HKP_X3K_STEM_PATCH_U8 18     /* conv_x3_stem_patch_kernel<2> */
#define HKP_X3K_COUNT 19
int32_t hkp_conv_x3_launch_plan(const hkp_conv_desc* d, int32_t op, int32_t stream_k_ok, int32_t cus,
                                int32_t launch_index, char* name_buf, int32_t len, int64_t* out);

/* (The A/B instruments — hkp_debug_* — are not part of this library: they exist only
 * in the tools build, include/hulkkp_ab.h.) */

/* ----------------------------------------------------------- batchnorm ---- */
/* Train-mode BatchNorm2d statistics (src/resnet.py:46,49,78,85,87,139,187;
 * nn.BatchNorm2d defaults eps=1e-5, momentum=0.1): merges the conv's tile
 * partials in fp64 (Chan), writes scale_shift = [gamma*invstd | beta - mean*scale],
 * mean_invstd = [mean | invstd] (nullable), and updates the running stats
 * (unbiased variance; nullable) and num_batches_tracked (nullable, +1). */
int hkp_bn_finalize(int32_t c, int64_t count, int64_t tiles, int32_t tile_rows, const float* partials,
                    const float* gamma, const float* beta, float momentum, float eps,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* scale_shift, float* mean_invstd, hkp_stream_t stream);

/* The same statistics in two levels for long tile lists (tiles > 128): chunks of
 * 128 tiles reduced by [C/64][chunks] blocks into a caller-allocated fp64
 * workspace of hkp_bn_finalize_workspace_bytes(c, tiles) bytes, then merged per
 * channel in fixed order (Chan at both levels).  Same outputs and argument
 * meaning as hkp_bn_finalize (src/resnet.py:46,49,78,85,87,139,187); the two
 * forms agree to fp64 summation order. */
int64_t hkp_bn_finalize_workspace_bytes(int32_t c, int64_t tiles);
int hkp_bn_finalize_ws(int32_t c, int64_t count, int64_t tiles, int32_t tile_rows, const float* partials,
                       const float* gamma, const float* beta, float momentum, float eps,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked,
                       float* scale_shift, float* mean_invstd, void* workspace, int64_t ws_bytes,
                       hkp_stream_t stream);

/* The same merges over a segmented tile list (a HKP_TILE_MIX_A3 conv's partials:
 * hkp_conv_x3_stat_layout): segments[2i] = rows per tile, segments[2i + 1] = tiles of
 * segment i, 1 <= nseg <= 3, a host table.  Every segment but the last is whole
 * full tiles; the last segment's last tile holds the rows left of count.  Tiles
 * merge in list order.  workspace == NULL: the one-kernel merge (hkp_bn_finalize),
 * else the two-level one (hkp_bn_finalize_ws; hkp_bn_finalize_workspace_bytes(c,
 * sum of tiles)).  nseg == 1 is hkp_bn_finalize / _ws / hkp_bn_stats itself: the
 * same kernels, the same bits. */
int hkp_bn_finalize_seg(int32_t c, int64_t count, int32_t nseg, const int32_t* segments, const float* partials,
                        const float* gamma, const float* beta, float momentum, float eps,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked,
                        float* scale_shift, float* mean_invstd, void* workspace, int64_t ws_bytes,
                        hkp_stream_t stream);
int hkp_bn_stats_seg(int32_t c, int64_t count, int32_t nseg, const int32_t* segments, const float* partials,
                     double* stats, void* workspace, int64_t ws_bytes, hkp_stream_t stream);

/* SyncBN for data-parallel ranks (caveat D5: train-mode BN makes a
 * shard's outputs depend on the shard; torch.nn.SyncBatchNorm's forward
 * statistics).  hkp_bn_stats: this rank's per-channel statistics from its conv
 * tile partials, written as stats = [mean[c] | M2[c] | count] (2c+1 fp64) —
 * the merge of hkp_bn_finalize (workspace == NULL) or hkp_bn_finalize_ws
 * (workspace of hkp_bn_finalize_workspace_bytes) without the scale/shift.  The
 * caller all-gathers the blocks in rank order into stats[nranks][2c+1], and
 * hkp_bn_finalize_ranks merges them in fixed rank order (Chan:
 * mean = sum n_r mean_r / N, M2 = sum M2_r + n_r (mean_r - mean)^2) into the same
 * outputs as hkp_bn_finalize over the global batch (running stats with the global
 * count's unbiased variance, num_batches_tracked += 1).  Identical bytes on every
 * rank.  Replaces the batch statistics of nn.BatchNorm2d.forward
 * (src/resnet.py:46,49,78,85,87,139,187) for a batch sharded over ranks. */
int hkp_bn_stats(int32_t c, int64_t count, int64_t tiles, int32_t tile_rows, const float* partials,
                 double* stats, void* workspace, int64_t ws_bytes, hkp_stream_t stream);
int hkp_bn_finalize_ranks(int32_t c, int32_t nranks, const double* stats, const float* gamma, const float* beta,
                          float momentum, float eps, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float* scale_shift, float* mean_invstd,
                          hkp_stream_t stream);

/* Eval-mode BN parameters from running statistics (the reference never uses
 * them; offered as an option). */
int hkp_bn_eval_params(int32_t c, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale_shift, float* mean_invstd,
                       hkp_stream_t stream);

/* out = [relu]( y*scale + shift  [+ res | + res*rscale + rshift] ), NHWC [m][c].
 * Replaces the bn→relu / bn→(+residual)→relu tails of BasicBlock
 * (src/resnet.py:57-67) and Bottleneck (:96-110). res may be NULL;
 * res_scale_shift NULL means the residual is added raw.  res_split (instead of res;
 * c % 32 == 0): the raw residual read from its packed split, hi + lo (the block
 * input a producer wrote split-only: inference keeps the residual stream as an
 * fp16 pair with a 22-bit significand instead of fp32).
 * out_split (nullable; needs c % 32 == 0): the same values also written as the
 * next conv's operand — split_passes = 1: fp16 plane [m][c] for
 * hkp_conv2d_fwd_f16; split_passes = 3: the packed split layout
 * [m][c/32][hi32|lo32] (hi = f16(out), lo = f16(out-hi)) for
 * hkp_conv2d_fwd_x3.  out may be NULL when out_split is given (an activation
 * only a conv consumes).  hkp_bn_relu_maxpool takes the same optional split. */
int hkp_bn_apply(int64_t m, int32_t c, const float* y, const float* scale_shift, const float* res,
                 const float* res_scale_shift, const uint16_t* res_split, int32_t relu, float* out,
                 uint16_t* out_split, int32_t split_passes, hkp_stream_t stream);

/* Plain-fp16 path (BASELINE config C4; autocast semantics): out (fp16) =
 * [relu](y*scale + shift [+ res | + res*rscale + rshift]) for an fp16 conv output
 * y [m][c] (hkp_conv2d_fwd_f16), fp16 residual res (the block input, or with
 * res_scale_shift the downsample conv's fp16 y); the arithmetic is fp32.  out32
 * (nullable): the same values in fp32 (the block feeding the head).  c % 8 == 0. */
int hkp_bn_apply_f16(int64_t m, int32_t c, const uint16_t* y, const float* scale_shift, const uint16_t* res,
                     const float* res_scale_shift, int32_t relu, uint16_t* out, float* out32, hkp_stream_t stream);

/* Stem tail: maxpool3x3/s2/p1( relu( y*scale + shift ) ), NHWC
 * (src/resnet.py:139-141, 200-202). Output [n, (h-1)/2+1, (w-1)/2+1, c].
 * route (nullable; training): per output element the window tap 0..8 (r*3+s)
 * of its first maximum — the pixel max_pool2d's backward routes the gradient
 * to — or 255 when the maximum is <= 0 (the ReLU derivative there is 0). */
int hkp_bn_relu_maxpool(int32_t n, int32_t h, int32_t w, int32_t c, const float* y,
                        const float* scale_shift, float* out, uint16_t* out_split, int32_t split_passes,
                        uint8_t* route, hkp_stream_t stream);

/* ---------------------------------------------------------------- head ---- */
/* K-channel 1x1 scoring conv + bias (src/resnet_dilated.py:16 sliced to the K
 * rows src/model.py:21 keeps): feat NHWC [n,hw,c] → lowres [n,k,hw]. */
int hkp_head_fc(int32_t n, int32_t hw, int32_t c, int32_t k, const float* feat, const float* w,
                const float* bias, float* lowres, hkp_stream_t stream);

/* Inference tail: the last block's BN apply (+ residual, ReLU — hkp_bn_apply /
 * hkp_bn_apply_f16's arithmetic) fused with hkp_head_fc, so the final feature
 * map is never written (src/resnet.py:110-112 / :68-69 of the last block, then
 * src/resnet_dilated.py:16 sliced to the K rows src/model.py:21 keeps).
 * y [n*hw][c] fp32 (y_f16 = 0) or fp16 (y_f16 = 1); res_kind 0: none, 1: raw
 * residual of y's dtype, 2: residual * rscale + rshift (res_scale_shift [2c]),
 * 3: packed split raw residual (fp32 y only); w [k][c], bias [k] →
 * lowres [n][k][hw].  Needs c % 512 == 0, c <= 2048, k <= 16.  fp16 y with
 * k <= 8 (config C4): the fp32 apply's result enters the head rounded to fp16,
 * against fp16-rounded head rows, fp32 accumulation (autocast's ReLU output and
 * 1x1 conv; MFMA). */
int hkp_bn_apply_head(int32_t n, int32_t hw, int32_t c, int32_t k, int32_t y_f16, const void* y,
                      const float* scale_shift, const void* res, const float* res_scale_shift, int32_t res_kind,
                      const float* w, const float* bias, float* lowres, hkp_stream_t stream);

/* bilinear align_corners=True upsample [n,k,h,w] → [n,k,H,W]
 * (src/resnet_dilated.py:27) + sigmoid (src/model.py:21; skipped when
 * apply_sigmoid == 0, the raw Resnet34_8s.forward output), NCHW output (nullable),
 * and the per-(n,k) argmax (src/prediction.py:46, first index wins) as
 * int32 (y, x) pairs in argmax_yx [n*k*2] (nullable).  argmax_ws: workspace of
 * hkp_upsample_argmax_ws_bytes(n,k,H,W) bytes (one key per 1024-pixel block per
 * plane; reduced in fixed order, no atomics), required when argmax_yx != NULL. */
int64_t hkp_upsample_argmax_ws_bytes(int32_t n, int32_t k, int32_t H, int32_t W);
int hkp_upsample_sigmoid(int32_t n, int32_t k, int32_t h, int32_t w, int32_t H, int32_t W,
                         int32_t apply_sigmoid, const float* lowres, float* heat, uint64_t* argmax_ws, int32_t* argmax_yx,
                         hkp_stream_t stream);

/* On-GPU visualisation (Prediction.plot, src/prediction.py:40-66):
 * per heatmap plane cv2.normalize NORM_MINMAX → .astype(uint8) (double scale /
 * shift, truncation), JET colour map (BGR; analytic — OpenCV's LUT is not in
 * this image, so cv2-pixel parity is unpinned), cv2.addWeighted(img, 0.65, map,
 * 0.35, 0) (rounded, saturated), a black filled radius-4 disc at argmax_yx as
 * cv2.circle's midpoint rasteriser draws it, tiled into the reference's grid:
 * planes k < K/2 stacked in column 0, the rest in column 1 — out
 * [n][H*K/2][2W][3] uint8 (K = 1: [n][H][W][3]; other odd K rejected, as the
 * reference's hconcat of unequal columns fails).  heat NCHW [n,k,H,W] fp32,
 * img_nhwc [n,H,W,3] uint8 BGR, argmax_yx [n,k,2] int32 (hkp_upsample_sigmoid),
 * minmax_ws [n*k*2] floats of workspace. */
int hkp_heat_overlay(int32_t n, int32_t k, int32_t H, int32_t W, const float* heat, const uint8_t* img_nhwc,
                     const int32_t* argmax_yx, float* minmax_ws, uint8_t* out, hkp_stream_t stream);

/* Soft-argmax per heatmap plane, the reference's Prediction.expectation
 * (src/prediction.py:31-38) with its axis mix-up fixed: p = softmax(beta * h)
 * over the plane (beta = 1: the reference's softmax), out_xy[n][k] = (sum p*x,
 * sum p*y) as fp32 from fp64 sums in fixed order (deterministic). */
int hkp_soft_argmax(int32_t n, int32_t k, int32_t H, int32_t W, float beta, const float* heat, float* out_xy,
                    hkp_stream_t stream);

/* Multi-peak decode of the low-res logits (not in the reference): per plane of
 * lowres [n,k,h,w] (fp32, what enters the upsample kernel; the full-resolution
 * heatmap is neither read nor written) the up to max_peaks best local maxima,
 * each as (x, y, score) — the order of soft_argmax and the labels, not the
 * (y, x) of the argmax — in peaks [n][k][max_peaks][3] fp32, and their number
 * in counts [n][k] int32; unused slots hold (-1, -1, 0).
 *  order:     a NaN logit counts as -inf and -0 as +0; node a beats node b if
 *             z[a] > z[b], or z[a] == z[b] and a has the smaller index i*w + j
 *             (first max wins, as the argmax).
 *  candidate: z > -inf, score = sigmoid(z) (fp32, the upsample kernel's own
 *             function) >= threshold, and the node beats every other node of its
 *             (2 radius + 1)^2 window clipped to the plane — the window is the
 *             non-maximum suppression: two peaks of a plane are never within
 *             Chebyshev distance radius.  The max_peaks best candidates are
 *             written, best first.
 *  position:  per axis, in fp64 from the fp32 logits, with g(z) = min(z, 0) -
 *             log1p(exp(-|z|)) (log sigmoid: -d^2 / 2 sigma^2 for a Gaussian
 *             target): if both neighbours lie in the plane, the three g are
 *             finite and den = 2 g0 - g- - g+ > 1e-6, the offset is
 *             clamp(0.5 (g+ - g-) / den, -0.5, 0.5), else 0;
 *             x = (j + dx) (W - 1) / (w - 1) (0 when w == 1), y likewise: the
 *             align_corners node coordinates in pixels of the H x W output, the
 *             frame of the labels and the argmax; rounded once to fp32.
 * One block per plane, the plane in LDS; no atomics, fixed reduction order: the
 * same input gives the same bits.  Limits: 1 <= radius <= 8,
 * 1 <= max_peaks <= 16, 0 <= threshold <= 1, h * w <= 32768 (128 KiB of LDS;
 * 120 x 160 is 19200); anything else is HKP_ERR_BAD_ARG. */
int hkp_heat_peaks(int32_t n, int32_t k, int32_t h, int32_t w, int32_t H, int32_t W, int32_t radius,
                   int32_t max_peaks, float threshold, const float* lowres, float* peaks, int32_t* counts,
                   hkp_stream_t stream);

/* Gaussian target (src/dataset.py:36-44): out[n,k,H,W] (fp64) =
 * (double) expf( -((x-u)^2 + (y-v)^2) / (2 sigma^2) ) computed in fp32;
 * uv [n,k,2] fp32 (u = column, v = row). */
int hkp_gauss_target(int32_t n, int32_t k, int32_t H, int32_t W, float sigma, const float* uv,
                     double* out, hkp_stream_t stream);

/* ============================================================ backward ==== */
/* Everything loss.backward() (train.py:35) runs through the reference's
 * modules, as hand-written kernels.  d = the FORWARD conv descriptor. */

/* w_flip[c][r][s][k] = w[k][R-1-r][S-1-s][c]: the dgrad weight (KRSC in → CRSK-flipped out). */
int hkp_conv_weight_flip(const hkp_conv_desc* d, const float* w, float* w_flip, hkp_stream_t stream);

/* dx[n,h,w,c] = sum over taps/k of dy * w (+ add[n,h,w,c], nullable: fuses the
 * residual-branch gradient sum): backward-data of hkp_conv2d_fwd (NHWC convs;
 * strided convs take the transposed-loader path).  w_flip from hkp_conv_weight_flip. */
int hkp_conv2d_bwd_data(const hkp_conv_desc* d, const float* dy, const float* w_flip, const float* add, float* dx,
                        hkp_stream_t stream);

/* max |x| as an IEEE bit pattern in amax_bits[0] (non-negative floats order like
 * their bits): the power-of-two gradient scale of the f16x3 backward convs
 * (dy_amax_bits of hkp_conv2d_bwd_data_x3 / _filter_x3 and hkp_split_pack_x3)
 * when no BN backward bound is at hand.  n % 4 == 0. */
int hkp_absmax(int64_t n, const float* x, uint32_t* amax_bits, hkp_stream_t stream);

/* The stem conv (7x7, stride 2, pad 3, NCHW input with C <= 4; src/resnet.py:137,199)
 * on the f16x3 path: hkp_stem_pack_x3 writes the image as zero-padded NHWC4 fp16
 * planes [2][n][2*ho+6][2*wo+6][4] (hi, then lo; hkp_stem_pack_x3_elems halves),
 * hkp_stem_weight_pack_x3 the OIHW weight as [k][7][hi32|lo32] (k*7*64 halves,
 * per-output-channel power-of-two scale, inverse in w_inv_scale[k]),
 * hkp_conv2d_fwd_stem_x3 = hkp_conv2d_fwd on them (NHWC fp32 y + BN partials). */
int64_t hkp_stem_pack_x3_elems(const hkp_conv_desc* d);
int hkp_stem_pack_x3(const hkp_conv_desc* d, const float* x_nchw, uint16_t* x_split, hkp_stream_t stream);
/* Device data path: the same planes straight from the uint8 batch
 * cv2.imread gives — img_nhwc [n][h][w][c] (BGR, c = d->c = 3), x = u8 / 255 in
 * fp32 exactly as ToTensor (src/dataset.py:16,71): 3 B per pixel read instead of
 * 12, and no fp32 image in HBM or over PCIe. */
int hkp_stem_pack_x3_u8(const hkp_conv_desc* d, const uint8_t* img_nhwc, uint16_t* x_split, hkp_stream_t stream);
/* ToTensor on the device: uint8 [n][h][w][c] → fp32 NCHW / 255 (the training path's
 * stem wgrad operand, and any consumer that wants the reference's tensor). */
int hkp_images_u8_to_nchw(int32_t n, int32_t h, int32_t w, int32_t c, const uint8_t* img_nhwc, float* x_nchw,
                          hkp_stream_t stream);
int hkp_stem_weight_pack_x3(int32_t k, int32_t c, const float* w_oihw, uint16_t* w_split, float* w_inv_scale,
                            hkp_stream_t stream);
int hkp_conv2d_fwd_stem_x3(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* w_split,
                           const float* w_inv_scale, float* y, float* stat_partials, hkp_stream_t stream);
/* The stem straight from the image where the patch body takes the shape (output
 * height % 8 == 0, width % 32 == 0, d->tile != HKP_TILE_64_PAIR: hkp_stem_x3_image_ok
 * returns 1): the fp32 NCHW image (image_u8 = 0) or the uint8 NHWC batch (1), split
 * in LDS per 8x32-pixel tile with hkp_stem_pack_x3's arithmetic — the same y and
 * partials bit for bit, without writing or reading the packed planes. */
int32_t hkp_stem_x3_image_ok(const hkp_conv_desc* d);
int hkp_conv2d_fwd_stem_x3_image(const hkp_conv_desc* d, const void* image, int32_t image_u8, const uint16_t* w_split,
                                 const float* w_inv_scale, float* y, float* stat_partials, hkp_stream_t stream);

/* f16x3 backward on packed split operands (the layout of hkp_conv2d_fwd_x3):
 *   hkp_split_pack_x3:       x * 2^e → packed split [n/c][c/32][64]; 2^e from
 *                            amax_bits (max|x| as from hkp_absmax; NULL: 2^0) puts
 *                            max|x|*2^e in [2^13, 2^14) — gradients far below
 *                            fp16's normal range keep fp32-class accuracy.
 *   hkp_weight_flip_pack_x3: KRSC w → packed flipped [c][r][s][k/32][64] (dgrad
 *                            operand), per-row power-of-two scale, inverse in
 *                            wf_inv_scale[c].
 *   hkp_conv2d_bwd_data_x3:  dx = conv(dy, flipped w) + add for stride-1 convs,
 *                            dy_split packed with the scale of dy_amax_bits;
 *                            needs Cin % 64 == 0, Cout % 32 == 0.
 *   hkp_conv2d_bwd_filter_x3: dw (KRSC) from x_split (forward operand) and dy_split;
 *                            split-K over output pixels into `workspace`
 *                            (hkp_conv_bwd_filter_x3_workspace bytes), fixed-order
 *                            reduce; needs Cout % 64 == 0, Cin % 32 == 0.  Here
 *                            d->tile is the number of CUs the grid should occupy
 *                            (0: the planner's split count, which fills whole
 *                            rounds of all CUs; a wgrad sharing the GPU with a
 *                            dgrad may take fewer): splits = max(1, tile / tiles).
 *                            3x3 stride-1 pad-1 convs with Cin, Cout in {64, 128},
 *                            Ho % 4 == 0 and Wo % 16 == 0 run the halo body
 *                            (wgrad_x3_halo_kernel: 64 Cout x 9 taps x 64 Cin per
 *                            block, 4x16-pixel patches staged once for every tap);
 *                            tile == -1 keeps the tiled body for them.
 * Replace the same cuDNN backward calls as hkp_conv2d_bwd_data / _filter. */
int hkp_split_pack_x3(int64_t n, int32_t c, const float* x, const uint32_t* amax_bits, uint16_t* x_split,
                      hkp_stream_t stream);
int hkp_weight_flip_pack_x3(const hkp_conv_desc* d, const float* w, uint16_t* wf_split, float* wf_inv_scale,
                            hkp_stream_t stream);
int hkp_conv2d_bwd_data_x3(const hkp_conv_desc* d, const uint16_t* dy_split, const uint16_t* wf_split,
                           const float* wf_inv_scale, const uint32_t* dy_amax_bits, const float* add, float* dx,
                           void* sk_workspace, int64_t sk_ws_bytes, hkp_stream_t stream);
/* Strided (stride 2, dilation 1) backward-data on the f16x3 path: dx is computed
 * per output phase (py, px) as a stride-1 conv of dy with that phase's taps
 * (phase_split[py*2+px] = kind-2 packs of hkp_weight_pack_x3_batch, inverse
 * scales phase_inv_scale[..]) written to dx pixels (2a+py, 2b+px); a phase no tap
 * reaches (NULL entry; e.g. the odd pixels of a 1x1 stride-2 downsample) gets
 * dx = add (or 0).  d = the forward descriptor; needs Cin % 64 == 0, Cout % 32 == 0.
 * hkp_phase_taps: taps of phase `phase` along an axis of r taps (0: none, -1: bad args). */
int32_t hkp_phase_taps(int32_t r, int32_t pad, int32_t stride, int32_t phase);
int hkp_conv2d_bwd_data_x3_strided(const hkp_conv_desc* d, const uint16_t* dy_split,
                                   const uint16_t* const* phase_split, const float* const* phase_inv_scale,
                                   const uint32_t* dy_amax_bits, const float* add, float* dx, void* sk_workspace,
                                   int64_t sk_ws_bytes, hkp_stream_t stream);
/* Batched weight packing for a training step (one launch pair for a whole
 * network instead of one hkp_weight_pack_x3 / hkp_weight_flip_pack_x3 per conv;
 * outputs bit-identical to those).  jobs: host array; kind 0 = forward pack
 * (out = w_split [k][rs][c/32][64], inv_scale [k]; needs c % 32 == 0), kind 1 =
 * flipped dgrad pack (out = wf_split [c][rs][k/32][64], inv_scale [c]; needs
 * c % 64 == 0, k % 32 == 0), kind 2 = output phase `phase` (= py*2 + px) of a
 * stride-2 conv's dgrad operand (fields r, s, pad; out = [c][R2][S2][k/32][64]
 * with R2/S2 = hkp_phase_taps(r|s, pad, 2, py|px); inv_scale [c] = kind 1's) for
 * hkp_conv2d_bwd_data_x3_strided; w is KRSC fp32 [k][rs][c].  workspace:
 * hkp_weight_pack_x3_batch_ws_bytes(njobs, jobs) bytes (per-channel column
 * maxima of the flip jobs). */
typedef struct hkp_pack_job {
    const float* w;
    uint16_t* out;
    float* inv_scale;
    int32_t kind, k, rs, c;
    int32_t r, s, pad, phase;   /* kind 2 only */
} hkp_pack_job;
int64_t hkp_weight_pack_x3_batch_ws_bytes(int32_t njobs, const hkp_pack_job* jobs);
int hkp_weight_pack_x3_batch(int32_t njobs, const hkp_pack_job* jobs, void* workspace, int64_t ws_bytes,
                             hkp_stream_t stream);
int64_t hkp_conv_bwd_filter_x3_workspace(const hkp_conv_desc* d);
int hkp_conv2d_bwd_filter_x3(const hkp_conv_desc* d, const uint16_t* x_split, const uint16_t* dy_split,
                             const uint32_t* dy_amax_bits, float* dw, void* workspace, int64_t ws_bytes,
                             hkp_stream_t stream);

/* dw (KRSC, or OIHW for the stem) = sum over pixels of dy x im2col(x); split-K over
 * pixels into `workspace`, reduced in fixed order.  accumulate != 0 adds into dw. */
int64_t hkp_conv_bwd_filter_workspace(const hkp_conv_desc* d);
int hkp_conv2d_bwd_filter(const hkp_conv_desc* d, const float* x, const float* dy, float* dw, int32_t accumulate,
                          void* workspace, int64_t ws_bytes, hkp_stream_t stream);

/* Train-mode BatchNorm backward, three launches:
 *   reduce:   dz = g * (out_mask > 0) (out_mask NULL: dz = g), optionally stored to dz;
 *             partials[tiles][c][2] = (sum dz, sum dz*(y-mean)); tiles = hkp_bn_bwd_tiles(m);
 *             maxima (nullable) [tiles][c][2] = (max|dz|, max|y-mean|), and then
 *             dy_bound_bits (nullable) is zeroed for finalize
 *   finalize: dgamma = invstd*sum dz*(y-mean), dbeta = sum dz (nullable), coef[3c];
 *             with maxima: dy_amax_bits receives an upper bound of max|dy|,
 *             (max|dz| + |mean dz| + max|y-mean|*|k|) * |invstd*gamma|; without:
 *             dy_amax_bits (nullable) is reset to 0 for apply's exact max
 *   apply:    dy = ((dz - sum dz/m) - (y-mean)*invstd^2*sum dz*(y-mean)/m) * invstd*gamma
 *             dy_split (nullable): dy written as the packed f16x3 split of dy*2^e,
 *             2^e = the power of two of the bound in dy_amax_bits — the gradient
 *             operand of the x3 backward convs, with no hkp_split_pack_x3 pass and
 *             dy (fp32) optional; else dy_amax_bits (nullable) gets the exact max|dy|.
 * mean_invstd is what hkp_bn_finalize produced in the forward. */
/* The ReLU mask: out_mask (the BN+ReLU output, > 0), or relu_ss = the forward's
 * [scale | shift] of this BN — the mask is then recomputed from y exactly as
 * hkp_bn_apply made it (round(round(y*scale) + shift) > 0), so an inner BN's fp32
 * activation is not read back; both NULL: no ReLU. */
int64_t hkp_bn_bwd_tiles(int64_t m);
int hkp_bn_bwd_reduce(int64_t m, int32_t c, const float* g, const float* out_mask, const float* relu_ss,
                      const float* y, const float* mean_invstd, float* dz, float* partials, float* maxima,
                      uint32_t* dy_bound_bits, hkp_stream_t stream);
int hkp_bn_bwd_finalize(int32_t c, int64_t m, const float* partials, const float* maxima, const float* mean_invstd,
                        const float* gamma, float* dgamma, float* dbeta, float* coef, uint32_t* dy_amax_bits,
                        hkp_stream_t stream);
/* SyncBN backward (torch SyncBatchNorm: sum_dy and sum_dy_xmu over all ranks).
 * hkp_bn_bwd_stats: in place of hkp_bn_bwd_finalize's outputs, this rank's
 * per-channel [S = sum dz | D = sum dz*(y-mean) | max|dz| | max|y-mean| | m]
 * (4c+1 fp64; the maxima are 0 when maxima == NULL).  The caller all-gathers the
 * blocks in rank order into stats[nranks][4c+1]; hkp_bn_bwd_finalize_ranks sums
 * them in fixed rank order and writes hkp_bn_bwd_finalize's outputs: coef from
 * the global sums and count, dgamma/dbeta from this rank's block `own`, the
 * dy-split scale bound (has_maxima) from own maxima.  One rank: the same bits as
 * hkp_bn_bwd_finalize.  Replaces the backward of nn.BatchNorm2d in train mode
 * (src/resnet.py:46,49,78,85,87,139,187) for a batch sharded over ranks. */
int hkp_bn_bwd_stats(int32_t c, int64_t m, const float* partials, const float* maxima, const float* mean_invstd,
                     double* stats, hkp_stream_t stream);
int hkp_bn_bwd_finalize_ranks(int32_t c, int32_t nranks, const double* stats, const double* own, int32_t has_maxima,
                              const float* mean_invstd, const float* gamma, float* dgamma, float* dbeta, float* coef,
                              uint32_t* dy_amax_bits, hkp_stream_t stream);
int hkp_bn_bwd_apply(int64_t m, int32_t c, const float* g, const float* out_mask, const float* relu_ss,
                     const float* y, const float* mean_invstd, const float* coef, float* dy, uint32_t* dy_amax_bits,
                     uint16_t* dy_split, hkp_stream_t stream);

/* ----------------------------------------------------------- optimizer ---- */
/* Fused multi-tensor Adam with L2 weight decay (replaces the
 * optim.Adam(lr, weight_decay) step of train.py:36,79 — torch/optim/adam.py's
 * multi-tensor path, amsgrad/maximize off): for every element of every tensor
 *   g = g + wd*p;  m = m + (1-b1)*(g-m);  v = v*b2 + (1-b2)*g*g;
 *   p = p + neg_step_size * m / (sqrt(v)/bias_correction2_sqrt + eps)
 * with one_minus_beta1/2 = 1-b1, 1-b2, neg_step_size = -lr/(1-b1^step) and
 * bias_correction2_sqrt = sqrt(1-b2^step) computed by the caller in double (as
 * torch does with its Python-float scalars).  p, m, v updated in place; g read only. */
typedef struct hkp_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
} hkp_adam_tensor;
int hkp_adam_step(int32_t ntensors, const hkp_adam_tensor* tensors, float beta2, float one_minus_beta1,
                  float one_minus_beta2, float eps, float weight_decay, float neg_step_size,
                  float bias_correction2_sqrt, hkp_stream_t stream);

/* Global L2 norm of every gradient of a tensor table and the clip coefficient of
 * clip_grad_norm_ (torch/nn/utils/clip_grad.py), both left on the device:
 *   out[0] = norm = (float)sqrt(sum g^2),  c = max_norm / (norm + 1e-6f) in fp32,
 *   out[1] = coef = c < 1 ? c : (c != c ? c : 1)        (torch.clamp(c, max=1.0): NaN stays NaN)
 * Only `grad` and `n` of each entry are read.  One block per 4096-element unit
 * squares in fp64 (exact for fp32) and sums in a fixed order (thread, wave64, the
 * four waves) into one fp64 partial in `partials` (device, partials_len doubles,
 * at least hkp_grad_norm_partials(ntensors, tensors)); a single block sums the
 * partials in a fixed order.  No atomics, no host read: the same bits on every run.
 * max_norm > 0; +inf gives the norm alone (coef = 1 for a finite norm). */
int64_t hkp_grad_norm_partials(int32_t ntensors, const hkp_adam_tensor* tensors);
int hkp_grad_norm(int32_t ntensors, const hkp_adam_tensor* tensors, float max_norm, double* partials,
                  int64_t partials_len, float* out, hkp_stream_t stream);

/* hkp_adam_step with two optional extras in the same pass (both NULL: hkp_adam_step):
 *   coef (device float, e.g. out + 1 of hkp_grad_norm): g = g * coef before the
 *     update — _foreach_mul_(grads, clip_coef) followed by Adam; g is not written;
 *   ema ([ntensors] device pointers, one per entry of `tensors`) with
 *     one_minus_decay in (0, 0.5): after the update e = e + one_minus_decay * (p - e),
 *     torch._foreach_lerp_(ema, params, 1 - decay) (torch/optim/swa_utils.py). */
int hkp_adam_step_ex(int32_t ntensors, const hkp_adam_tensor* tensors, float* const* ema, float one_minus_decay,
                     const float* coef, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                     float weight_decay, float neg_step_size, float bias_correction2_sqrt, hkp_stream_t stream);

/* Stem: backward of maxpool3x3/s2/p1(relu(y*scale+shift)) → dz = dL/d(BN output)
 * [n,h,w,c], ReLU mask applied (src/resnet.py:200-202; ATen's first-max window
 * rule): each window's dpool goes to the tap the forward recorded in `route`
 * (hkp_bn_relu_maxpool), summed per pixel over its windows in (ho, wo) order. */
int hkp_maxpool_bwd(int32_t n, int32_t h, int32_t w, int32_t c, const float* dpool, const uint8_t* route, float* dz,
                    hkp_stream_t stream);

/* Loss over the heatmaps (train.py:21,25; MSE train.py:13) in fp64: loss (device
 * double), dheat = dL/dheat as fp32 (nullable).  Target: dense fp64 `target`
 * [n,k,H,W], or NULL to recompute the Gaussian from uv/sigma (dataset.py:36-44).
 * BCE clamps as ATen does: the logs at -100, and the gradient's denominator
 * (1-p)*p at ATen's `constexpr float EPSILON = 1e-12` widened to double
 * ((double)1e-12f = 9.99999996e-13, not the double 1e-12), so dheat keeps
 * nn.BCELoss's bits on saturated pixels (p of 0, 1 or within 1e-12 of either).
 * workspace: hkp_heat_loss_workspace() bytes. */
int64_t hkp_heat_loss_workspace(void);
int hkp_heat_loss(int32_t n, int32_t k, int32_t H, int32_t W, int32_t loss_kind, const float* heat,
                  const double* target, const float* uv, float sigma, double* loss, float* dheat, void* workspace,
                  hkp_stream_t stream);

/* Multi-instance labels: pts [n,k,m,3] fp32, last axis (u, v, flag), 1 <= m <= 16
 * (the max_peaks limit of hkp_heat_peaks).  flag > 0: the slot holds an instance at
 * (u, v) (u = column, v = row, integers are pixel centres; finite, may lie outside
 * the image).  Anything else: the slot is empty, and its u, v (NaN included) are
 * never read into the result; slots need not be packed.  A plane without a present
 * slot is an absent keypoint.
 *
 * Target (src/dataset.py:36-44 per instance): out[n,k,H,W] (fp64) =
 * max over the present slots of (double) expf( -((x-u)^2 + (y-v)^2) / (2 sigma^2) ),
 * each term in hkp_gauss_target's fp32 operation order (m = 1: its bits), 0 for an
 * absent plane.  The maximum, not the sum: every instance keeps a peak of 1, and
 * near a peak log t is the parabola hkp_heat_peaks refines on. */
int hkp_gauss_target_multi(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, float sigma, const float* pts,
                           double* out, hkp_stream_t stream);

/* hkp_heat_loss (train.py:21,25; MSE train.py:13) against that target, recomputed
 * in registers (dataset.py:36-44): the same per-element formulas, clamps and fp64
 * arithmetic; dheat fp32 (nullable).  absent_mode: HKP_ABSENT_ZERO trains an absent
 * plane against the all-zero target (divisor n*k*H*W, as hkp_heat_loss);
 * HKP_ABSENT_IGNORE leaves it out: its dheat is +0.0f and the divisor is H*W*A, A =
 * the planes with a present slot, counted on the device (no host synchronisation);
 * A = 0 gives loss 0 and dheat 0.  One partial per block summed in index order, no
 * atomics: the same input gives the same bits.  Limits: 1 <= m <= 16,
 * H*W <= 2^30; anything else is HKP_ERR_BAD_ARG.
 * workspace: hkp_heat_loss_multi_workspace(n, k, H, W) bytes. */
#define HKP_ABSENT_ZERO 0
#define HKP_ABSENT_IGNORE 1
int64_t hkp_heat_loss_multi_workspace(int32_t n, int32_t k, int32_t H, int32_t W);
int hkp_heat_loss_multi(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind, int32_t absent_mode,
                        const float* heat, const float* pts, float sigma, double* loss, float* dheat, void* workspace,
                        hkp_stream_t stream);

/* hkp_heat_loss_multi with a third loss kind and a choice of divisor (not in the
 * reference; hkp_heat_loss_multi itself is unchanged).  Same labels, target,
 * absent_mode, workspace, limits and launch scheme: fixed-order partials, no atomics,
 * the same input gives the same bits.
 * loss_kind: HKP_LOSS_BCE, HKP_LOSS_MSE (beta is not read; with HKP_NORM_ELEMENTS the
 *   bits of hkp_heat_loss_multi) or HKP_LOSS_QFL, the quality focal loss (Li et al.,
 *   "Generalized Focal Loss", 2020) against the soft target: per element in fp64, with
 *   x = (double)heat, y = (double)t, d = x - y and
 *   bce = (y-1) * max(log1p(-x), -100) - y * max(log(x), -100)  (hkp_heat_loss's clamps),
 *     l = |d|^beta * bce
 *     g = (beta * |d|^(beta-1) * sgn(d) * bce + |d|^beta * d / max((1-x)*x, 1e-12f)) / divisor
 *   — float64 autograd of binary_cross_entropy(x, y, "none") * |x - y|^beta, cast to
 *   fp32.  d == 0 gives l = 0 and g = +0 exactly, for every beta and also at x = y = 0
 *   or 1: the minimum is at heat == target in every pixel.  beta in [1, 8] (finite; it
 *   is a float: what the kernel raises to is that float); 2 takes a path of its own
 *   without pow.  Anything else is HKP_ERR_BAD_ARG and nothing is written.
 * norm_mode: HKP_NORM_ELEMENTS: hkp_heat_loss_multi's divisors (n*k*H*W, or H*W*A under
 *   HKP_ABSENT_IGNORE); HKP_NORM_INSTANCES: max(P, 1), P = the present slots (flag > 0)
 *   of the whole batch, counted on the device (no host synchronisation).  Under
 *   HKP_ABSENT_IGNORE an absent plane's dheat is +0.0f and it adds nothing, in either
 *   norm mode. */
#define HKP_LOSS_QFL 2
#define HKP_NORM_ELEMENTS 0
#define HKP_NORM_INSTANCES 1
int hkp_heat_loss_multi_ex(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                           int32_t absent_mode, int32_t norm_mode, float beta, const float* heat, const float* pts,
                           float sigma, double* loss, float* dheat, void* workspace, hkp_stream_t stream);

/* hkp_heat_loss_multi_ex with a weight per (image, class) plane, the per-plane loss
 * values and online hard keypoint mining (OHKM: Chen et al., "Cascaded Pyramid
 * Network", 2018); not in the reference, and the entries above are unchanged.  Same
 * labels, target, loss kinds (beta as there), absent_mode, per-element formulas, clamps
 * and fp64 arithmetic, the 16-byte and the scalar path, fixed-order sums, no atomics:
 * the same input gives the same bits.  Every decision is taken on the device, with no
 * host synchronisation.
 * eligible:  a plane (b, c) is eligible unless it has no present slot under
 *            HKP_ABSENT_IGNORE, or weights is given and !(weights[b][c] > 0): zero,
 *            negative and NaN all mean "not labelled" (the instance flag's rule).  The
 *            heat of a plane that is not eligible is never read into the result; its
 *            dheat is +0.0f, its plane_loss -1.0 (every kind is >= 0) and plane_used 0.
 * S[b][c]:   the fp64 sum of the unweighted per-element losses of an eligible plane: its
 *            block partials added in chunk order.  plane_loss[b][c] = S / (H*W); two
 *            planes with the same heat and labels get the same bits.
 * topk = T:  0: every eligible plane is counted.  1 <= T <= k <= 64: per image the
 *            eligible planes are ranked by r = (double)w * S (w = 1 without weights) and
 *            the T largest are counted; equal r goes to the lower class, a NaN r ranks
 *            above everything, fewer than T eligible planes are all counted.
 *            plane_used is 1 for a counted plane; an eligible plane that is not counted
 *            keeps its plane_loss and gets dheat +0.0f.
 * divisor D: HKP_NORM_ELEMENTS: H*W*C, C = the counted planes of the batch (C = 0: loss 0,
 *            dheat 0); HKP_NORM_INSTANCES: max(P, 1), P = the present slots of the
 *            counted planes.  Weights never enter the divisor.
 * values:    loss = (sum over the counted planes, in plane order, of (double)w * S) / D;
 *            dheat = (float)(g * (double)w), g the fp64 value hkp_heat_loss_multi_ex
 *            forms for that element with divisor D.  With w == 1 (or no weights) the
 *            product is exact: the bits of hkp_heat_loss_multi_ex.
 * launches:  topk == 0: one pass over the planes between a small pre- and post-kernel.
 *            topk > 0: a first pass that reads the heat and writes only the partials, a
 *            one-block kernel that ranks and counts, and a second pass that writes dheat
 *            and reads the heat of the counted planes only.  The loss comes from the
 *            stored S either way, so topk == k gives the bits of topk == 0.
 * weights [n][k] fp32, plane_loss [n][k] fp64 and plane_used [n][k] int32 are nullable,
 * as is dheat.  Limits as hkp_heat_loss_multi_ex, and 0 <= topk <= k, k <= 64 when
 * topk > 0; anything else is HKP_ERR_BAD_ARG and nothing is launched or written.
 * workspace: hkp_heat_loss_planes_workspace(n, k, H, W) bytes. */
int64_t hkp_heat_loss_planes_workspace(int32_t n, int32_t k, int32_t H, int32_t W);
int hkp_heat_loss_planes(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                         int32_t absent_mode, int32_t norm_mode, float beta, int32_t topk, const float* heat,
                         const float* pts, const float* weights, float sigma, double* loss, float* dheat,
                         double* plane_loss, int32_t* plane_used, void* workspace, hkp_stream_t stream);

/* hkp_heat_loss_planes with a per-pixel ignore mask; not in the reference, and the entries
 * above are unchanged.  mask uint8 [n][H][W], in the frame of the heatmaps and labels, one
 * byte per pixel holding class bits: bit c set takes the pixel out for class c (0xFF: for
 * every class), so k <= 8.  The k planes of an image read the same bytes.  Everything the
 * planes entry defines holds, with these changes:
 * keep:      keep(b,c,y,x) = !((mask[b][y][x] >> c) & 1); n_bc = the kept pixels of plane
 *            (b, c), an exact integer counted on the device.
 * eligible:  under the planes entry's rules AND n_bc > 0: a fully masked plane is "not
 *            labelled", exactly as a weight of 0 is (dheat +0.0f, plane_loss -1.0, not in
 *            the divisor).
 * S[b][c]:   the fp64 sum of the unweighted per-element losses over the KEPT pixels, as
 *            block partials in chunk order.  A masked pixel adds +0.0 and gets dheat +0.0f
 *            by a select, not a product: whatever its heat holds (NaN included) changes no
 *            output bit.  plane_loss = S / n_bc; plane_pixels = n_bc, 0 for a plane that is
 *            not eligible.
 * topk = T:  the eligible planes of an image are ranked by r = (double)w * (S / n_bc), the
 *            weighted mean (what OHKM ranks on when planes differ in size); ties and NaN
 *            as in the planes entry.
 * divisor D: HKP_NORM_ELEMENTS: the sum of n_bc over the counted planes, exact, converted
 *            to double (D = 0: loss 0, dheat 0); HKP_NORM_INSTANCES: max(P, 1), unchanged.
 * values:    loss = (sum over the counted planes, in plane order, of (double)w * S) / D; on
 *            kept pixels dheat = (float)(g * (double)w), g the fp64 gradient under D.  With
 *            an all-zero mask every output has the bits of hkp_heat_loss_planes.
 * launches:  a count pass over the mask (integers: any order), then the planes entry's
 *            pre-kernel, pass, one-block finish and, with topk > 0, second pass.  No atomics
 *            on floating values, no host synchronisation.
 * mask is required (null: HKP_ERR_BAD_ARG; callers without a mask use the planes entry);
 * it is read bytewise, or as 32-bit words where W % 4 == 0 and it is 4-byte aligned.
 * plane_pixels [n][k] int32 is nullable like the other plane outputs.  k > 8 and every
 * argument the planes entry refuses is HKP_ERR_BAD_ARG, and nothing is launched or written.
 * workspace: hkp_heat_loss_masked_workspace(n, k, H, W) bytes. */
int64_t hkp_heat_loss_masked_workspace(int32_t n, int32_t k, int32_t H, int32_t W);
int hkp_heat_loss_masked(int32_t n, int32_t k, int32_t m, int32_t H, int32_t W, int32_t loss_kind,
                         int32_t absent_mode, int32_t norm_mode, float beta, int32_t topk, const float* heat,
                         const float* pts, const float* weights, const uint8_t* mask, float sigma, double* loss,
                         float* dheat, double* plane_loss, int32_t* plane_used, int32_t* plane_pixels,
                         void* workspace, hkp_stream_t stream);

/* Keypoint evaluation (not in the reference): the peaks and counts of
 * hkp_heat_peaks, peaks [n][k][p][3] (x, y, score) and counts [n][k], matched
 * plane by plane to the labels of hkp_heat_loss_multi, pts [n][k][m][3] (u, v,
 * flag), at t distance thresholds at once, and ADDED into two int64 accumulators
 * that stay on the device: hist [k][t][2][bins] and totals [k][8].  One launch,
 * no host synchronisation.  thresholds_host [t] is host memory and is passed to
 * the kernel by value; thresholds are in pixels of the frame of peaks and labels.
 * Per plane (b, c):
 *  slots:     cnt = clamp(counts[b][c], 0, p); peak slots at index cnt and above
 *             are never read, whatever they hold.  A label slot is present iff
 *             flag > 0 (hkp_heat_loss_multi's rule); the (u, v) of an empty slot
 *             are never read into the result.
 *  distance:  dx = (double)x - (double)u, dy likewise, d2 = dx*dx + dy*dy in fp64
 *             without fused multiply-add.  Every decision is made on d2: within
 *             threshold tau means d2 <= (double)tau * (double)tau, inclusive, so a
 *             NaN coordinate never matches (such a peak is a false positive, such
 *             a present instance a miss).  No square root takes part in a decision.
 *  matching:  independently per threshold index ti, COCO's greedy rule: the peaks
 *             in slot order 0 .. cnt-1 (best first, as hkp_heat_peaks writes them)
 *             each take the nearest present instance that is not yet taken at this
 *             threshold and lies within tau[ti]; equal d2 goes to the lower label
 *             slot.  A peak that takes one is a true positive, else a false
 *             positive.
 *  score bin: in fp32, bin = s >= 1 ? bins-1 : !(s > 0) ? 0 :
 *             min(bins-1, (int)(s * (float)bins)); NaN goes to bin 0.
 *             hist[c][ti][0][bin] += 1 for a true positive, hist[c][ti][1][bin] += 1
 *             for a false positive.
 *  totals[c]: [0] planes seen, [1] planes without a present slot (absent
 *             keypoints), [2] present instances, [3] peaks (sum of cnt),
 *             [4] instances matched at the loosest threshold t-1, [5] the sum over
 *             those matches of (int64)floor((double)dist32 * 65536.0 + 0.5) with
 *             dist32 = (float)sqrt(d2), the very value written to gt_dist,
 *             [6] peaks on absent planes, [7] is never touched.
 *  per batch (each skipped when NULL):
 *             peak_match [n][k][t][p] int32: the label slot taken, -1 for an
 *             unmatched peak, -2 for a slot j >= cnt;
 *             gt_match [n][k][m] int32: at the loosest threshold the peak slot that
 *             took instance i, -1 for a present but missed instance, -2 for an
 *             empty slot; gt_dist [n][k][m] fp32: the distance of that match,
 *             else -1.
 * Everything accumulated is an integer (64-bit integer atomic adds, the totals
 * combined per block first), so the result does not depend on the order of the
 * additions: the same inputs give the same bits.  Limits: n, k >= 1,
 * 1 <= p, m <= 16, 1 <= t <= 8, 1 <= bins <= 4096, thresholds finite, > 0 and
 * strictly ascending; anything else is HKP_ERR_BAD_ARG with no launch. */
int hkp_peaks_match(int32_t n, int32_t k, int32_t p, int32_t m, int32_t t, int32_t bins,
                    const float* thresholds_host, const float* peaks, const int32_t* counts, const float* pts,
                    int64_t* hist, int64_t* totals, int32_t* peak_match, int32_t* gt_match, float* gt_dist,
                    hkp_stream_t stream);

/* dlow = upsample-adjoint( dheat * (1-heat) * heat ) (sigmoid backward fused;
 * heat NULL = dheat is already the pre-sigmoid gradient): a row gather into
 * `workspace` (hkp_head_bwd_workspace bytes: [n*k][H][w] floats), then a column
 * gather — the direct double sum's loop order, so the same bits.  Needs H >= h
 * and W >= w; h or w of 1 is fine (that one node takes every output's gradient). */
int64_t hkp_head_bwd_workspace(int32_t n, int32_t k, int32_t w, int32_t H);
int hkp_head_bwd(int32_t n, int32_t k, int32_t h, int32_t w, int32_t H, int32_t W, const float* dheat,
                 const float* heat, float* dlow, void* workspace, int64_t ws_bytes, hkp_stream_t stream);

/* fc (K used rows) backward: dfeat NHWC [n,hw,c], dw [k][c], db [k]. */
int64_t hkp_head_fc_bwd_workspace(int32_t n, int32_t hw, int32_t c, int32_t k);
int hkp_head_fc_bwd(int32_t n, int32_t hw, int32_t c, int32_t k, const float* dlow, const float* feat,
                    const float* w, float* dfeat, float* dw, float* db, void* workspace, int64_t ws_bytes,
                    hkp_stream_t stream);

/* ----------------------------------------------------------- JPEG ---- */
/* Device half of the hybrid JPEG decode (hkp_jpeg.h; replaces cv2.imread,
 * src/dataset.py:71): n images of one geometry g (hkpj_probe), coefs = int16
 * [n][g->nblocks][64] and qt = uint16 [n][g->ncomp][64] from hkpj_decode, on
 * the device → out_bgr = uint8 [n][H][W][3] BGR, bit-identical to
 * libjpeg-turbo's default decode (islow IDCT, fancy upsampling).  planes:
 * workspace of n * hkp_jpeg_planes_bytes(g) bytes (the IDCT'd component
 * planes).  hkp_jpeg_planes_bytes returns -1 for a geometry the kernels do not
 * take. */
int64_t hkp_jpeg_planes_bytes(const hkpj_geom* g);
int hkp_jpeg_reconstruct(int32_t n, const hkpj_geom* g, const int16_t* coefs, const uint16_t* qt, uint8_t* planes,
                         int64_t planes_bytes, uint8_t* out_bgr, hkp_stream_t stream);

/* ---------------------------------------------- domain randomisation ---- */
/* The reference's commented-out imgaug pipeline (src/dataset.py:18-31) on uint8
 * [n][h][w][3] BGR batches.  One image's augmentation is a program: an ordered
 * list of stages; after every stage the image is uint8 again (rint, half to
 * even, then clamp to [0,255]).  All arithmetic is fp32 with every operation
 * rounded on its own; transcendentals live in host-built tables (the LUTs, the
 * blur weights, the Gaussian quantile table), so a numpy float32 restatement in
 * the same order gives the same bits.
 *
 *   HKP_AUG_LUT    out_c = lut[c][v_c]; the stage in slot i of image b reads
 *                  luts[b][i][c][256] (c in memory order B, G, R).  LinearContrast
 *                  (:22), Add (:23), GammaContrast (:24), ChangeColorTemperature (:26).
 *   HKP_AUG_HSV    one float RGB→HSV→RGB round trip: f[0] = hue shift in sectors
 *                  (hue in [0,6)), S' = clamp(S * f[2] + f[1], 0, 255).
 *                  AddToHueAndSaturation (:21), MultiplySaturation (:27).
 *   HKP_AUG_BLUR   separable 5-tap blur, f[0..2] = w0, w1, w2 (w0 + 2 w1 + 2 w2 = 1),
 *                  reflect-101 borders; at most one per program.  GaussianBlur (:25).
 *   HKP_AUG_NOISE  n = gauss_table[x0 >> 20] * f[0], x0 = first word of
 *                  Philox4x32-10(counter (y*w + x, 0, 0, 0), key), added to the
 *                  three channels.  AdditiveGaussianNoise (:28).
 */
#define HKP_AUG_LUT 1
#define HKP_AUG_HSV 2
#define HKP_AUG_BLUR 3
#define HKP_AUG_NOISE 4
#define HKP_AUG_MAX_STAGES 8
#define HKP_AUG_GAUSS_TABLE 4096   /* entries of gauss_table: fp32 quantiles of N(0,1) at (i + 0.5) / 4096 */
#define HKP_AUG_TILE_H 16          /* one block's tile of one image (pixels) */
#define HKP_AUG_TILE_W 64

typedef struct hkp_aug_stage {
    int32_t kind;        /* HKP_AUG_*                                   */
    int32_t reserved0;
    float f[3];          /* HSV: dh, add, mul; BLUR: w0, w1, w2; NOISE: scale */
    uint32_t key[2];     /* NOISE: the Philox key                        */
    int32_t reserved1;
} hkp_aug_stage;         /* 32 bytes */

typedef struct hkp_aug_program {
    int32_t nstages;     /* 0 .. HKP_AUG_MAX_STAGES (0: copy)           */
    int32_t reserved[7];
    hkp_aug_stage stages[HKP_AUG_MAX_STAGES];
} hkp_aug_program;       /* 288 bytes */

/* img_out = programs applied to img_in, one launch for the batch.  programs_host
 * and programs hold the same n programs: the host copy is validated here (stage
 * counts, stage kinds, at most one BLUR) before anything is launched, the device
 * copy is what the kernel reads.  luts: device uint8 [n][HKP_AUG_MAX_STAGES][3][256]
 * (only the slots of LUT stages are read); gauss_table: device fp32
 * [HKP_AUG_GAUSS_TABLE].  h, w >= 3 (reflect-101); img_out must not overlap img_in
 * (the blur reads neighbours). */
int hkp_augment_u8(int32_t n, int32_t h, int32_t w, const uint8_t* img_in, uint8_t* img_out,
                   const hkp_aug_program* programs_host, const hkp_aug_program* programs, const uint8_t* luts,
                   const float* gauss_table, hkp_stream_t stream);

/* ------------------------------------------------------- affine warp ---- */
/* Batched per-image affine warp of uint8 [n][hs][ws][3] into [n][h][w][3]: the
 * geometric augmentation (rotation, scale, translation, shear, flips) and the
 * resize are host-side matrix builders over it (hkp/geometry.py).  Integer pixel
 * coordinates are pixel centres (as for the labels and hkp_gauss_target).  The
 * arithmetic is integer only and part of the contract (tests/_warp_ref.py restates
 * it in numpy), per output pixel (x, y):
 *
 *   sx = m0*x + m1*y + m2,  sy = m3*x + m4*y + m5        (int64, Q16)
 *   BILINEAR  qx = (sx + 128) >> 8 (arithmetic shift: floor), ix = qx >> 8,
 *             fx = qx & 255; the same for y; per channel
 *               top = p00*(256-fx) + p01*fx,  bot = p10*(256-fx) + p11*fx
 *               out = (top*(256-fy) + bot*fy + 32768) >> 16
 *             with p00 = src[iy][ix], p01 = src[iy][ix+1], p10 = src[iy+1][ix],
 *             p11 = src[iy+1][ix+1]  (fx = fy = 0 returns p00 exactly)
 *   NEAREST   ix = (sx + 32768) >> 16, iy likewise, out = src[iy][ix]
 *
 * ix and iy are clamped into [-2, dim + 1] first (no visible effect in CONSTANT
 * and REPLICATE mode; in REFLECT101 mode the image does not repeat further out),
 * then every tap index (ix, ix+1, iy, iy+1) goes through the border rule on its
 * own; the kernel forms addresses from in-range indices only. */
#define HKP_WARP_BILINEAR 0
#define HKP_WARP_NEAREST  1
#define HKP_WARP_BORDER_CONSTANT   0   /* a tap outside the source takes fill[c] (each tap on its own) */
#define HKP_WARP_BORDER_REPLICATE  1   /* tap indices clamped */
#define HKP_WARP_BORDER_REFLECT101 2   /* tap indices reflected without repeating the edge (-1 -> 1, dim -> dim-2,
                                          once, then clamped); hs, ws >= 2 */
#define HKP_WARP_MAX_DIM 16384

typedef struct hkp_warp_xform {   /* 32 bytes */
    int32_t m[6];      /* inverse map, dest -> source, Q16: sx = m0*x + m1*y + m2, sy = m3*x + m4*y + m5 */
    uint8_t fill[4];   /* B, G, R, unused */
    int32_t reserved;  /* 0 */
} hkp_warp_xform;

/* One launch for the batch.  xforms_host and xforms hold the same n records: the
 * host copy is validated here before anything is launched (device memory is not
 * read), the device copy is what the kernel reads.  All dimensions in
 * [1, HKP_WARP_MAX_DIM]; img_out must not overlap img_in.  Rows leave as dwords
 * when w % 4 == 0 and img_out is 4-byte aligned, as bytes otherwise. */
int hkp_warp_affine_u8(int32_t n, int32_t hs, int32_t ws, const uint8_t* img_in, int32_t h, int32_t w,
                       uint8_t* img_out, const hkp_warp_xform* xforms_host, const hkp_warp_xform* xforms,
                       int32_t interp, int32_t border, hkp_stream_t stream);

/* The ignore masks of hkp_heat_loss_masked through the images' transforms: a one-channel
 * warp of uint8 [n][hs][ws] into [n][h][w] with the records of hkp_warp_affine_u8 (their
 * fill colours are not read) and exactly its HKP_WARP_NEAREST rule: Q16 coordinates,
 * ix = (sx + 32768) >> 16, indices clamped into [-2, dim + 1] and then through the border
 * rule, addresses from in-range indices only, in all three border modes.  The source byte
 * goes through lut [n][256] (device, nullable: the identity) — how a flipped image
 * exchanges the class bits of its flip pairs — and under HKP_WARP_BORDER_CONSTANT a pixel
 * outside the source gets `fill` (0..255) as given, not through the table: 0 leaves the
 * outside trained, 255 ignores it.  Rows leave as dwords when w % 4 == 0 and mask_out is
 * 4-byte aligned, as bytes otherwise.  Limits and checks as hkp_warp_affine_u8. */
int hkp_warp_mask_u8(int32_t n, int32_t hs, int32_t ws, const uint8_t* mask_in, int32_t h, int32_t w,
                     uint8_t* mask_out, const hkp_warp_xform* xforms_host, const hkp_warp_xform* xforms,
                     int32_t border, int32_t fill, const uint8_t* lut, hkp_stream_t stream);

/* Ignore masks from region records: regions fp32 [n][r][6] = (kind, a, b, c, d, bits) in
 * device memory, 1 <= r <= HKP_MASK_MAX_REGIONS, into out uint8 [n][H][W], every byte
 * written in one launch (no memset).  Integer pixel coordinates are pixel centres; pixel
 * (x, y) is inside
 *   kind == 1 (box)   iff a <= x <= c and b <= y <= d
 *   kind == 2 (disc)  iff (x-a)*(x-a) + (y-b)*(y-b) <= c*c, in fp32 with every product and
 *                     sum rounded on its own (no contraction); d is not used
 * and any other kind (NaN included) is an empty slot whose other fields are never read
 * into the result.  A NaN bound is never inside.  bits is an integer 0..255 held in a
 * float (anything else counts as 0).  out = the OR of the bits of the regions that hold
 * the pixel.  H, W in [1, HKP_MASK_MAX_DIM], n in [1, 65535]; rows leave as dwords when
 * W % 4 == 0 and out is 4-byte aligned, as bytes otherwise. */
#define HKP_MASK_BOX 1
#define HKP_MASK_DISC 2
#define HKP_MASK_MAX_REGIONS 64
#define HKP_MASK_MAX_DIM 4096
int hkp_mask_regions_u8(int32_t n, int32_t r, int32_t H, int32_t W, const float* regions, uint8_t* out,
                        hkp_stream_t stream);

/* ------------------------------------------------- antialiased resize ---- */
/* Batched antialiased resize of uint8 BGR images of ANY size (each image of the
 * batch has its own) into uint8 [n][h][w][3]: the first stage of the data path,
 * decoded frame -> network-size frame.  The result equals Pillow's
 * Image.resize((wd, hd), filter, reducing_gap=None) of an RGB image bit for bit
 * (tests/_resample_ref.py restates it in numpy; tests pin both).  The resampler is
 * separable, horizontal pass first; the filter lives in host-built axis tables
 * (hkp/resample.py) and the device arithmetic is integer only.  Per image, with
 * its x table (ws -> wd) and its y table (hs -> hd), for every pixel (xx, yy) of
 * the destination rectangle and every channel:
 *
 *   mid[sy][xx] = clip((2^21 + sum_{t < xcnt[xx]} src[sy][xmin[xx] + t] * kx[xx][t]) >> 22, 0, 255)
 *   out[y0 + yy][x0 + xx] = clip((2^21 + sum_{t < ycnt[yy]} mid[ymin[yy] + t][xx] * ky[yy][t]) >> 22, 0, 255)
 *
 * (>> is an arithmetic shift; int32 accumulators suffice: the coefficients of a
 * row sum to 2^22 and the negative lobes of the filters fit the two spare bits).
 * mid is Pillow's uint8 intermediate image; the kernel keeps it in registers, one
 * pixel at a time, and never writes it to memory.  An axis that keeps its size
 * takes the identity table (cnt = 1, k = 2^22), which returns the pixel exactly.
 * Output pixels outside the destination rectangle take the fill colour.
 *
 * Axis table, int32 words at a word offset into `tables`:
 *   [0] ksize   [1] out   then out x (xmin, cnt)   then out x ksize coefficients
 * (row xx's coefficients start at word 2 + 2*out + xx*ksize; cnt of them are read).
 * Built on the host in float64 as Pillow builds them: scale = in/out,
 * fs = max(scale, 1), support = filter_support * fs, ksize = ceil(support)*2 + 1,
 * center = (xx + 0.5)*scale, xmin = max(int(center - support + 0.5), 0),
 * cnt = min(int(center + support + 0.5), in) - xmin,
 * w[t] = filter((t + xmin - center + 0.5) * (1/fs)), divided by their sum (index
 * order) unless it is 0, k[t] = int(w*2^22 + 0.5) (w >= 0) or int(w*2^22 - 0.5)
 * (w < 0), both truncating. */
typedef struct hkp_resample_image {   /* 64 bytes */
    int64_t offset;      /* byte offset of the image (uint8 [hs][ws][3]) inside img_in */
    int32_t hs, ws;      /* source size                                                */
    int64_t xtab, ytab;  /* word offsets of the x (ws -> wd) and y (hs -> hd) tables   */
    int32_t x0, y0;      /* destination rectangle inside the h x w output ...          */
    int32_t wd, hd;      /* ... and its size                                           */
    uint8_t fill[4];     /* B, G, R, unused: the colour outside the rectangle          */
    int32_t reserved[3]; /* 0 */
} hkp_resample_image;

/* One launch for the batch, no workspace.  records_host / records hold the same n
 * records and tables_host / tables the same table_words int32 words: the host
 * copies are validated here before anything is launched (device memory is not
 * read), the device copies are what the kernel reads.  Checked: every image lies
 * inside in_bytes; table offsets and sizes lie inside table_words; a table's `out`
 * equals wd / hd; xmin >= 0, cnt >= 0, xmin + cnt <= the source extent and
 * cnt <= ksize for every output index; the rectangle lies inside h x w; all
 * dimensions in [1, HKP_WARP_MAX_DIM]; reserved == 0; img_out does not overlap
 * img_in.  Coefficients are not checked (they cannot form an address).  Rows
 * leave as dwords when w % 4 == 0 and img_out is 4-byte aligned, as bytes
 * otherwise. */
int hkp_resample_u8(int32_t n, const uint8_t* img_in, int64_t in_bytes, const hkp_resample_image* records_host,
                    const hkp_resample_image* records, const int32_t* tables_host, const int32_t* tables,
                    int64_t table_words, int32_t h, int32_t w, uint8_t* img_out, hkp_stream_t stream);

/* ------------------------------------------- procedural cable scenes ---- */
/* Renders uint8 [n][h][w][3] BGR pictures of cables from a scene description
 * (hkp/synth.py samples it and makes the labels): a value-noise background, then
 * the scene's pieces composited in index order.  Every piece is a capsule (a disc
 * is a capsule of length 0).  Integer pixel coordinates are pixel centres.  The
 * arithmetic is integer only and part of the contract (tests/_synth_ref.py restates
 * it in numpy); >> is an arithmetic shift (floor).
 *
 * Background of pixel (x, y), scene key (k0, k1), cell_log2 = L; octave o = 0, 1
 * has shift sh = L - o:
 *   ix = x >> sh,  fx = ((x & ((1 << sh) - 1)) << 8) >> sh      (Q8; the same for y)
 *   v(i, j) = low 8 bits of the first word of Philox4x32-10(counter (i, j, o, 0), key)
 *   top = v(ix, iy)*(256 - fx) + v(ix+1, iy)*fx,  bot = v(ix, iy+1)*(256 - fx) + v(ix+1, iy+1)*fx
 *   n_o = (top*(256 - fy) + bot*fy + 32768) >> 16
 *   n = (3*n_0 + n_1 + 2) >> 2,   bg_c = bg0_c + (((bg1_c - bg0_c)*n + 128) >> 8)
 *
 * Piece, with P = (16 x, 16 y) the pixel in Q4:
 *   a  = P - (x0, y0)
 *   s  = clamp((ax*ux + ay*uy) >> 14, 0, len)                    Q4 along the axis
 *   c  = a - ((s*ux) >> 14, (s*uy) >> 14)
 *   d2 = cx*cx + cy*cy                                            Q8
 *   alpha = 256 if d2 <= r_in2;  0 if d2 >= r_out2;  else ((r_out2 - d2)*inv) >> 24
 *   lum   = 256 - ((shade * ((min(d2, r2)*inv_r2) >> 24)) >> 8)
 *   colour_c = (bgr_c*lum + 128) >> 8
 * with r the radius in Q4, r_in2 = (r - 8)^2, r_out2 = (r + 8)^2 (half a pixel either
 * side), r2 = r*r, inv = floor(2^32 / (r_out2 - r_in2)), inv_r2 = floor(2^32 / r2).
 *
 * Word widths, at the validated limits (|x0|, |y0| <= 2^17, P < 2^16, |ux|, |uy| <= 2^14,
 * len <= 2^18, 16 <= r <= 512):
 *   a.u        |a| < 2^18 per axis, so |ax*ux + ay*uy| < 2*2^18*2^14 = 2^33: 64 bits.
 *   s*u        s <= 2^18, |u| <= 2^14: up to 2^32: 64 bits.
 *   c.c        |c| <= |a| + 2^18 < 2^19 per axis, d2 < 2^39: 64 bits.  Only d2 < r_out2
 *              <= 520^2 < 2^19 is used after the comparison, so all that follows is narrow.
 *   (r_out2 - d2)*inv   in the ramp r_in2 < d2, so the factor is at most D - 1 with
 *              D = r_out2 - r_in2 = 32 r <= 2^14, and (D - 1)*floor(2^32 / D) < 2^32: 32 bits
 *              unsigned, and alpha <= 255 there.
 *   min(d2, r2)*inv_r2  reaches r2*floor(2^32 / r2), which is 2^32 exactly when r2 is a
 *              power of two (r = 16, 32, ... 512): 64 bits (33 would do).  The quotient is <= 256.
 *   everything else (the bilinear noise < 2^24, the blends < 2^17) fits 32 bits.
 *
 * Compositing: the pieces with alpha > 0 at the pixel are walked in ascending index.
 * A piece continues the current run when its arc id equals the run's and its index is
 * the run's last index + 1; otherwise the run ends and a new one starts.  A run keeps
 * the piece with the largest alpha, then the smallest d2, then the later index; when
 * it ends it is blended over what lies below:
 *   out_c = (run_c*alpha + out_c*(256 - alpha) + 128) >> 8
 * so a joint is not blended twice and a later strand's rim lies over an earlier one. */
#define HKP_SYNTH_MAX_DIM 4096
#define HKP_SYNTH_MAX_SEGS 512     /* pieces per image */
#define HKP_SYNTH_TILE_H 16        /* one block's tile of one image (pixels) */
#define HKP_SYNTH_TILE_W 64

typedef struct hkp_synth_seg {    /* 64 bytes */
    int32_t x0, y0;        /* start vertex, Q4, |.| <= 2^17                      */
    int32_t ux, uy;        /* unit direction, Q14, |.| <= 2^14                   */
    int32_t len;           /* length, Q4, 0 .. 2^18                              */
    int32_t r;             /* radius, Q4, 16 .. 512 (1 .. 32 px)                 */
    int32_t r_in2, r_out2; /* (r - 8)^2, (r + 8)^2                               */
    int32_t r2;            /* r*r                                                */
    uint32_t inv, inv_r2;  /* floor(2^32 / (r_out2 - r_in2)), floor(2^32 / r2)   */
    uint8_t bgr[4];        /* B, G, R, unused                                    */
    int32_t shade;         /* 0 .. 256: how much darker the rim is               */
    int32_t arc;           /* run id: consecutive pieces of one arc form a run   */
    int32_t reserved[2];   /* 0 */
} hkp_synth_seg;

typedef struct hkp_synth_scene {  /* 64 bytes */
    int32_t seg_off;       /* first piece of the image in the table              */
    int32_t seg_cnt;       /* 0 .. HKP_SYNTH_MAX_SEGS                            */
    uint32_t key[2];       /* Philox key of the background                       */
    uint8_t bg0[4], bg1[4];/* the two background colours: B, G, R, unused        */
    int32_t cell_log2;     /* 4 .. 12: octave 0's lattice cell is 1 << cell_log2 px */
    int32_t reserved[9];   /* 0 */
} hkp_synth_scene;

/* One launch for the batch, no workspace, no input image: img_out is written whole.
 * scenes_host / scenes hold the same n records and segs_host / segs the same nsegs
 * pieces: the host copies are validated here before anything is launched or written
 * (device memory is not read), the device copies are what the kernel reads.  Checked:
 * 1 <= h, w <= HKP_SYNTH_MAX_DIM; seg_off >= 0, 0 <= seg_cnt <= HKP_SYNTH_MAX_SEGS and
 * seg_off + seg_cnt <= nsegs; every piece of every image within the limits above with
 * r_in2, r_out2, r2, inv and inv_r2 equal to what r gives; 4 <= cell_log2 <= 12;
 * reserved == 0.  Rows leave as dwords when w % 4 == 0 and img_out is 4-byte aligned,
 * as bytes otherwise. */
int hkp_synth_cables_u8(int32_t n, int32_t h, int32_t w, uint8_t* img_out, const hkp_synth_scene* scenes_host,
                        const hkp_synth_scene* scenes, const hkp_synth_seg* segs_host, const hkp_synth_seg* segs,
                        int32_t nsegs, hkp_stream_t stream);

/* ==================================== test-time augmentation: view merge ==== */
/* The low-res logits of several views of one batch (the input as it is, flipped,
 * rescaled: one forward each) merged into logits on the base view's stride-8
 * lattice, in one launch (csrc/tta.hip); hkp_heat_peaks reads the result as it
 * reads one forward's.  Not in the reference.
 *
 *  packed  the views' logits, one after the other in one flat fp32 buffer: view v
 *          is [n][k][h_v][w_v], contiguous, at element offset off_v.
 *  table   `views` hkp_merge_view records in device memory (below).
 *  perm    int32 [views][k] in device memory: the channel of view v that feeds
 *          output channel c is perm[v][c] (the flip pairs).
 *  out     [n][k][h][w] fp32; must not overlap packed.
 *
 * For output node (i, j) of plane (b, c) and view v, all in fp64, no fused
 * multiply-add, the views in table order (tests/_tta_ref.py restates it in numpy):
 *  coordinates  cy = ay*i + by (one multiply, then one add), clamped to
 *               [0, h_v - 1]; i0 = floor(cy), fy = cy - i0, i1 = min(i0 + 1, h_v - 1);
 *               the same along x with (ax, bx), j and w_v.
 *  sample       with z the fp32 logits of view v, image b, channel perm[v][c]:
 *                 top = z[i0][j0] + fx*(z[i0][j1] - z[i0][j0])
 *                 bot = z[i1][j0] + fx*(z[i1][j1] - z[i1][j0])
 *                 z_v = top + fy*(bot - top)
 *               A tap whose weight is exactly 0 is not read: fx == 0 gives
 *               top = z[i0][j0] and bot = z[i1][j0], fy == 0 gives z_v = top.  A flip
 *               (a = -1, b = dim - 1) is therefore an exact copy, even beside a NaN or
 *               an infinity.  (An infinity in a tap that IS read with a fractional
 *               weight follows the formula: inf - inf is NaN.)
 *  HKP_MERGE_LOGIT  out = (float) sum_v weight_v * z_v; the sum starts with view 0's
 *                   term, not with +0, so one identity view returns its input's bits
 *                   (-0 included)
 *  HKP_MERGE_PROB   zc = min(max(z_v, -700), 700), a NaN stays NaN;
 *                   p = sum_v weight_v / (1 + exp(-zc)),  q = sum_v weight_v / (1 + exp(zc));
 *                   out = (float)(log p - log q): the logit of the weighted mean
 *                   probability, both tails summed so that scores near 1 keep
 *                   their precision.
 * One thread per output element (per 4 of a row, stored as 16 bytes, where
 * w % 4 == 0 and out is 16-byte aligned), grid-stride over a capped grid; no LDS, no
 * atomics, no workspace: the same input gives the same bits.
 * Checked on the host arguments alone, before anything is written: n, k, h, w >= 1,
 * 1 <= views <= HKP_MERGE_MAX_VIEWS, mode, non-null pointers, packed / perm / out
 * 4-byte and table 8-byte aligned; anything else is HKP_ERR_BAD_ARG.  The table's
 * contents (off, 1 <= h_v, w_v, finite coefficients, 0 <= perm < k, every view inside
 * packed) are the caller's contract, as for the warp and resample plans; tap indices
 * and the channel are clamped into range before an address is formed. */
#define HKP_MERGE_LOGIT 0
#define HKP_MERGE_PROB 1
#define HKP_MERGE_MAX_VIEWS 8

typedef struct hkp_merge_view {   /* 64 bytes */
    int64_t off;           /* element offset of the view's [n][k][h][w] logits in packed */
    int32_t h, w;          /* the view's lattice                                         */
    double ay, by;         /* base row i    -> view row    ay*i + by                     */
    double ax, bx;         /* base column j -> view column ax*j + bx                     */
    double weight;         /* the view's share of the sum                                */
    int64_t reserved;      /* 0 */
} hkp_merge_view;

int hkp_logits_merge(int32_t n, int32_t k, int32_t h, int32_t w, int32_t views, int32_t mode,
                     const float* packed, const void* table, const int32_t* perm,
                     float* out, hkp_stream_t stream);

/* ============================ associative-embedding tags: loss and grouping ==== */
/* Which cap belongs to which tail (Newell et al., 2017; the grouping of
 * HigherHRNet): one scalar tag map per keypoint class on the stride-8 lattice,
 * trained so that the tags of one instance agree and those of different instances
 * differ, and a decode that groups the peaks of hkp_heat_peaks by tag
 * (csrc/tags.hip; tests/_tags_ref.py restates all of it in numpy).  Neither entry
 * has a counterpart in the reference.
 *
 *  tag map      the tag map of class c is row k + c of the scoring conv, so tags need
 *               2k <= 16 rows of the head: the low-res tensor with tags is
 *               low_all [n][2k][h][w] fp32, heat logits in channels 0..k-1, tags in
 *               channels k..2k-1.
 *  in place     `tags` points at channel k of image 0 and batch_stride is the distance
 *               in ELEMENTS between two images (2k*h*w for low_all; >= k*h*w); tags
 *               needs 4-byte alignment only.  No copy of the tag planes is made.
 *  frame        the frame of hkp_heat_peaks: pixel (u, v) of the H x W picture lies at
 *               x = (double)u * (w-1) / (W-1) (0 when W == 1 or w == 1), y likewise,
 *               each clamped to the lattice (x > 0 ? x : 0, then x < w-1 ? x : w-1: a
 *               NaN goes to 0); x0 = min(floor(x), w-2) (0 when w == 1), fx = x - x0,
 *               x1 = min(x0 + 1, w-1), and the same along y.
 *  sample       the fp64 bilinear value of the fp32 map, without fused multiply-add:
 *               top = (1-fx)*t[y0][x0] + fx*t[y0][x1], bot likewise on row y1,
 *               t = (1-fy)*top + fy*bot.
 *
 * hkp_tag_loss: pts [n][k][m][3] (u, v, flag) as hkp_heat_loss_multi takes them and
 * gid int32 [n][k][m], the group (cable) of each slot.  A slot takes part when its
 * flag > 0 and 0 <= gid < 32; the (u, v) of any other slot are never read.  Per
 * image, with t_i the samples of the participating points, G distinct groups, n_g
 * members and mu_g their mean:
 *    pull_b = (1/G) sum_g (1/n_g) sum_{i in g} (t_i - mu_g)^2
 *    push_b = (1/(G(G-1))) sum_{g != g'} exp(-(mu_g - mu_g')^2 / 2),  0 for G < 2
 * and an image without a group adds 0.  out[3] (fp64) = (total, mean pull, mean
 * push) with total = (1/n) sum_b (pull_w*pull_b + push_w*push_b): the divisor is the
 * constant n.  dtag [n][k][h][w] fp32 (NULL: no gradient) is WRITTEN WHOLE, +0 where
 * no point reaches, and needs no memset: dtag = (float)(scale * d total / d map),
 * formed in fp64 from the closed form
 *    d pull_b / d t_i  = 2 (t_i - mu_g) / (G n_g)
 *    d push_b / d mu_g = -(2/(G(G-1))) sum_{g' != g} (mu_g - mu_g') exp(-(mu_g - mu_g')^2 / 2)
 *    d mu_g / d t_i    = 1 / n_g
 * each point's gradient spread to its four taps by the bilinear weights.  A gather:
 * every node sums, in slot order and tap order 00, 01, 10, 11, the taps that fall
 * on it — no atomics, so the same input gives the same bits.  scale (the loss
 * weight), pull_w and push_w travel as floats and must be finite and >= 0.
 * workspace: hkp_tag_loss_workspace(n) bytes (the per-image pull and push).
 * Limits: n >= 1, 1 <= k <= 8, 1 <= m <= 16, 1 <= h, w <= 32767, H, W >= 1;
 * anything else is HKP_ERR_BAD_ARG and nothing is launched or written. */
int64_t hkp_tag_loss_workspace(int32_t n);
int hkp_tag_loss(int32_t n, int32_t k, int32_t m, int32_t h, int32_t w, int32_t H, int32_t W,
                 const float* tags, int64_t batch_stride, const float* pts, const int32_t* gid,
                 float scale, float pull_w, float push_w, double* out, float* dtag, void* workspace,
                 hkp_stream_t stream);

/* hkp_peaks_group: peaks [n][k][p][3] (x, y, score) and counts [n][k] of
 * hkp_heat_peaks, the tag planes as above, and order_host, q distinct class ids
 * (host memory, passed to the kernel by value), 1 <= q <= k.  Written whole:
 *    tag     [n][k][p] fp32   the sample (rounded once to fp32) at every peak slot
 *                             below min(max(count, 0), p), of every class; 0 elsewhere
 *    group   [n][k][p] int32  the group of the peak; -1 for unused slots and for
 *                             classes not in order
 *    ngroups [n] int32
 * Per image the classes are taken in `order` and the peaks in slot order (best
 * first).  Each peak looks at the groups that do not yet hold a member of its
 * class, with d_g = |t - mean_g| in fp64, mean_g the fp64 sum of the members' fp32
 * tags divided by their count; the smallest d_g wins, equal values go to the lower
 * group id; if that d_g <= (double)max_dist the peak joins the group, else it opens
 * group ngroups++.  A NaN tag fails every comparison and opens a group.  A greedy
 * rule, not HigherHRNet's per-class Hungarian assignment.  One wavefront per image,
 * no atomics.  Limits: 1 <= k <= 8, 1 <= p <= 16, lattice as above, max_dist finite
 * and > 0, order within 0..k-1 without repeats; anything else is HKP_ERR_BAD_ARG
 * and nothing is launched or written. */
int hkp_peaks_group(int32_t n, int32_t k, int32_t p, int32_t h, int32_t w, int32_t H, int32_t W, int32_t q,
                    const int32_t* order_host, float max_dist, const float* peaks, const int32_t* counts,
                    const float* tags, int64_t batch_stride, float* tag, int32_t* group, int32_t* ngroups,
                    hkp_stream_t stream);

/* ============================ line labels: the centreline target ================ */
/* A heatmap class trained against a polyline (a cable's centreline) instead of
 * points: the Gaussian of the distance to the nearest segment, and that distance
 * (csrc/lines.hip; tests/_lines_ref.py restates it in numpy).  The reference has no
 * counterpart; its path from here on is dense target -> BCE (hkp_heat_loss).
 *
 * lines float32 [n][k][s][5], last axis (x0, y0, x1, y1, flag), 1 <= s <= HKP_LINE_MAX_S.
 *   frame   that of pts: x is the column, y the row, integers are pixel centres;
 *           coordinates may lie outside the picture.
 *   flag    > 0 marks a present segment; anything else (NaN included) is an empty
 *           slot whose coordinates are never read into a result.  Slots need not be
 *           packed.  Present coordinates are finite with |.| <= 32768: the caller's
 *           duty, not checked (there is no host read).
 * Per plane and pixel (x, y), all in fp32 without contraction or fused multiply-add,
 * over the present slots in slot order:
 *    dx = x1 - x0;  dy = y1 - y0;  l2 = dx*dx + dy*dy;              (per segment, once)
 *    inv = 1.0f / l2                                (IEEE division; only when l2 > 0)
 *    px = (float)x - x0;  py = (float)y - y0;
 *    t  = l2 > 0 ? fminf(fmaxf((px*dx + py*dy) * inv, 0.f), 1.f) : 0.f
 *                                   (fmaxf / fminf's NaN rule: a NaN product gives t = 0)
 *    cx = px - t*dx;  cy = py - t*dy;
 *    d2 = fminf(d2, cx*cx + cy*cy)                                  (starts at +inf)
 * Outputs, each nullable, at least one given:
 *    d2     float32 [n][k][H][W]  the minimum above; +inf for a plane without a
 *                                 present slot
 *    target float64 [n][k][H][W]  (double)expf(-d2 / den), den as in hkp_gauss_target,
 *                                 (float)(2.0 * (double)sigma * (double)sigma); +0.0
 *                                 for a plane without a present slot
 * A zero-length segment gives t = 0, cx = px, cy = py: hkp_gauss_target's
 * (x-u)^2 + (y-v)^2 in its operation order, so a plane of points has the bits of
 * hkp_gauss_target_multi at m = 1 (and at m > 1 as far as expf is monotone).
 * One launch, no atomics, no workspace, no host synchronisation: the same input gives
 * the same bits.  The kernel drops, per tile, the segments that cannot be nearest to
 * any of its pixels; the outputs are the bits of the definition above regardless.
 * n, k, H, W >= 1, 1 <= s <= HKP_LINE_MAX_S, H*W <= 2^30, sigma finite and > 0 (checked
 * even when target is NULL, where it is not read), lines and at least one output
 * non-null; anything else is HKP_ERR_BAD_ARG and nothing is launched or written. */
#define HKP_LINE_MAX_S 128
int hkp_line_target(int32_t n, int32_t k, int32_t s, int32_t H, int32_t W, float sigma,
                    const float* lines, double* target, float* d2, hkp_stream_t stream);

/* The plane loss against line labels, the target recomputed in registers: the contract
 * of hkp_heat_loss_masked (and, without a mask, of hkp_heat_loss_planes) with lines
 * [n][k][s][5] in place of pts; not in the reference, and the entries above are
 * unchanged.  Two definitions above are composed and nothing is added to either:
 * target:    per pixel t is the fp32 value hkp_line_target defines, with its flag rule, its
 *            operation order, den = (float)(2.0 * (double)sigma * (double)sigma), d2 over the
 *            present slots in slot order, t = expf(-d2 / den), +0.0f for a plane without a
 *            present slot; no contraction.  An empty slot is never read into a result, a
 *            point is a zero-length segment.  The dense target is never stored.
 * element:   loss and gradient are hkp_heat_loss_planes' per-element formulas on
 *            ((double)heat, (double)t) under the divisor D; dheat = (float)(g * (double)w).
 *            With a mask, a masked pixel is selected out of the sum and gets dheat +0.0f.
 * rules:     eligibility, S, plane_loss (S / (H*W), or S / n_bc with a mask; -1.0 where not
 *            eligible), plane_used, plane_pixels, the topk ranking with its tie and NaN
 *            rules, D and the loss are those of hkp_heat_loss_planes (mask == NULL) and of
 *            hkp_heat_loss_masked (mask given), word for word, with one reading:
 * P:         "present slots" are present SEGMENT slots: a plane's P is the number of its
 *            slots with flag > 0, points and pieces alike, so a polyline of 12 pieces counts
 *            12 under HKP_NORM_INSTANCES.
 * S[b][c]:   a block owns one chunk of a plane's 32 x 32 tiles (chunk, chunk + chunks, ...);
 *            every thread adds its elements into one fp64 accumulator over all its tiles,
 *            the block's sum is one partial, and S is the partials in chunk order.  The
 *            order differs from the other entries': S agrees with theirs to rounding, dheat
 *            (which depends on S only through topk) bit for bit where the targets do.
 * A plane that takes no part gets dheat +0.0f; its heat, its mask and its records beyond
 * the flags are never read.  Per tile the kernel drops the segments that cannot be nearest
 * to any of its pixels, as hkp_line_target does: the outputs are the bits of the definition.
 * launches:  the mask's count pass (with a mask), a pre-kernel, the pass, the one-block
 *            finish and, with topk > 0 and dheat, the second pass.  No atomics on floating
 *            values, no host synchronisation: the same input gives the same bits.
 * weights, mask, dheat, plane_loss, plane_used and plane_pixels are nullable; plane_pixels
 * is written only when a mask is given.  n, k, H, W >= 1, H*W <= 2^30, 1 <= s <=
 * HKP_LINE_MAX_S, sigma finite and > 0, heat, lines, loss and workspace non-null, the
 * kind / absent / norm codes of hkp_heat_loss_planes, beta in [1, 8] for HKP_LOSS_QFL (NaN
 * refused), 0 <= topk <= k and k <= 64 when topk > 0, k <= 8 with a mask; anything else is
 * HKP_ERR_BAD_ARG and nothing is launched or written.
 * workspace: hkp_heat_loss_lines_workspace(n, k, H, W) bytes. */
int64_t hkp_heat_loss_lines_workspace(int32_t n, int32_t k, int32_t H, int32_t W);
int hkp_heat_loss_lines(int32_t n, int32_t k, int32_t s, int32_t H, int32_t W, int32_t loss_kind,
                        int32_t absent_mode, int32_t norm_mode, float beta, int32_t topk, const float* heat,
                        const float* lines, const float* weights, const uint8_t* mask, float sigma, double* loss,
                        float* dheat, double* plane_loss, int32_t* plane_used, int32_t* plane_pixels,
                        void* workspace, hkp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HULKKP_H */

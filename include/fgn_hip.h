/* libfgn_hip.so -- C-ABI of the MI355X (gfx950) FGN inference kernels.
 *
 * The reference (tooHotSpot/FGN) has no native/FFI layer: its hot path is Python
 * (subprojects/sp02_omniiseg_fgn_mmdet/fgn.py:187-303) calling CUDA kernels inside the
 * mmdet / mmcv / torchvision / torch wheels.  Each entry point below replaces one of
 * those third-party kernel families at the call site cited; a maintainer binds them
 * with ctypes or any other FFI: plain pointers and sizes only, no
 * torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; tensors are fp32, NHWC
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); nothing here
 *     allocates, frees or synchronises: the caller owns workspaces, calls are
 *     asynchronous and safe to capture in a hipGraph
 *   - `n_*_dev` arguments are optional device int32 counters: when non-NULL the kernel
 *     processes min(*n_dev, n) items, so data-dependent counts (proposals, detections)
 *     never round-trip through the host
 *   - return value: 0 on success, <0 for FGN_ERR_* (bad argument / unsupported shape),
 *     >0 for a hipError_t from the launch
 */
#ifndef FGN_HIP_H
#define FGN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGN_OK 0
#define FGN_ERR_SHAPE (-1)
#define FGN_ERR_ARG (-2)

int fgn_abi_version(void);

/* Profiler hook (no reference counterpart): arm the calling thread so that the NEXT convolution-family kernel it
 * launches stamps the two HIP events (hipEvent_t, created by the caller) with that kernel's own start and end -
 * the duration a rocprofv3 kernel trace reports.  NULL, NULL disarms. */
int fgn_profile_next_launch(void* start_event, void* stop_event);
/* Launch records that work inside a replayed hipGraph (no reference counterpart): while the calling thread is armed,
 * every launch of the dominant kernel (conv_pw_persist_kernel) is handed the next record of `records` (device memory,
 * `capacity` records of fgn_profile_stamp_words() x uint64, all zero except word 4 = ~0); each execution of such a
 * launch - every replay of a graph it was captured into - adds its span (first workgroup start -> last workgroup end,
 * 10 ns ticks of the constant 100 MHz clock) to the record: [1] sum, [3] executions, [4] shortest, [5] longest.  A
 * recorded launch pays one returning atomic per workgroup at its exit (~1 us at the end of the launch).  NULL disarms.
 * Returns the number of records handed out since the previous call (= launches recorded, in launch order). */
int fgn_profile_stamp_words(void);
int fgn_profile_stamps(void* records, int capacity);
/* Phase marks between streams that replay captured graphs (no reference counterpart; the pipelined serving loop of
 * INTEGRATION.md): fgn_phase_signal bumps *counter (device memory, int32) from inside an episode - captured into its
 * graph like any kernel; fgn_phase_wait holds `stream` until *counter - target >= 0 or timeout_us (<= 1 s) have passed. */
int fgn_phase_signal(int32_t* counter, void* stream);
int fgn_phase_wait(const int32_t* counter, int32_t target, int timeout_us, void* stream);

/* Implicit-GEMM convolution on the fp32 MFMA pipe with fused epilogue
 *   y = conv(x * in_scale?, w) * scale[c] + shift[c] (+ residual) (ReLU)
 * Replaces cuDNN conv + BN(eval) + ReLU of mmdet ResNet (fgn.py:212,215), RPNHead
 * (fgn_ag_rpn_head.py:48), shared_head ResLayer (fgn_roi_head.py:236,369,436), the two
 * halves of cls_reg_shared_conv (fgn_roi_head.py:270), FCNMaskHead convs and the 2x2
 * deconv (fgn_roi_head.py:380); in_scale fuses the guidance multiplies at
 * fgn_ag_rpn_head.py:44 and fgn_roi_head.py:379.
 *   x [n_img/a_img_div, H, W, Cin]   w_packed [cout_pad, KH, KW, Cin] (K padded to x32,
 *   cout_pad multiple of 128, zero rows)   y [n_img, Ho, Wo, Cout]
 *   scale/shift [Cout] or NULL; residual like y or NULL; in_scale [n_img, Cin] or NULL
 *   Cin must be a multiple of 32, or exactly 4 = the stem's NHWC4 image: three channels and a ZERO fourth one, in x
 *   (fgn_nchw3_to_nhwc4_f32) and in w_packed alike - the kernel does not multiply the fourth channel
 *   tile_hint 0 = auto, 1..4 = force a tile configuration, negative = no split-K,
 *   +100 = register-staged loader instead of LDS-DMA (tests)
 *   splitk_ws: optional workspace of fgn_conv2d_workspace_bytes() bytes; when given and the plain
 *   grid would under-fill the GPU, K is split over blockIdx.y into partial-tile slabs that are
 *   summed in slab order (bit-reproducible) before the epilogue.  NULL = never split.
 *   (The kernels behind this entry point that were measured and not adopted - Stream-K, a tile scheduler, other
 *   tile shapes - are not part of this library: tools/micro/conv_pw_experiments.inc.) */
size_t fgn_conv2d_workspace_bytes(int n_img, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                  int pad, int tile_hint);
/* Which kernel the dispatcher launches for a layer (tile*10 + mode; 41 = conv_igemm_dma_kernel<64,64,32,32,2,4,1>):
 * lets a profiler attribute a launch to the kernel name rocprofv3 reports.  It is the decision of the launch itself (one
 * plan serves both, given the workspace fgn_conv2d_workspace_bytes asks for): arguments fgn_conv2d_nhwc_f32 refuses on
 * shape or hint return that refusal's code (FGN_ERR_SHAPE / FGN_ERR_ARG, negative), not an id.  fgn_conv2d_workspace_bytes
 * is 0 for them.  No reference counterpart. */
int fgn_conv2d_kernel_id(int n_img, int H, int W, int Cin, int Cout, int cout_pad, int KH, int KW, int stride,
                         int pad, int a_img_div, int has_in_scale, int has_residual, int tile_hint);
int fgn_conv2d_nhwc_f32(const float* x, const float* w_packed, float* y, const float* scale,
                        const float* shift, const float* residual, const float* in_scale,
                        const int32_t* n_img_dev, int n_img, int H, int W, int Cin, int Cout,
                        int cout_pad, int KH, int KW, int stride, int pad, int a_img_div, int relu,
                        int tile_hint, float* splitk_ws, size_t splitk_ws_bytes, void* stream);

/* Two 1x1 / stride 1 convolutions on the same rows summed in one K loop: y = x W1^T + x2 W2^T + shift (ReLU), w_packed
 * [cout_pad][Cin1 + Cin2] with both BatchNorm scales folded into its rows.  Replaces conv3 + bn3 and the shortcut
 * conv + bn + add + ReLU of the first Bottleneck of a stride-1 stage (mmdet ResNet layer1.0 under fgn.py:212,215):
 * no launch and no [rows, Cout] round trip for the shortcut.  x [rows,Cin1], y [rows,Cout]; x2 [x2_total_rows,Cin2]:
 * output row m reads row x2_rows[m] of it (device int32: the 1x1 / stride 2 shortcut of layer2.0 / layer3.0), or row m
 * when x2_rows is NULL (x2_total_rows = rows).  Cin1, Cin2 multiples of 32, Cout % 4 == 0. */
int fgn_conv1x1_dual_nhwc_f32(const float* x, const float* x2, const int32_t* x2_rows, int x2_total_rows,
                              const float* w_packed, float* y, const float* shift, int rows, int Cin1, int Cin2, int Cout,
                              int cout_pad, int relu, void* stream);

/* The GEMM-shaped launches of the path with their PRODUCTS on the bf16 matrix pipe (conv_pw_x3_kernel, csrc/conv_pw_x3.h;
 * gfx950's f32-input MFMA runs at 1/16 of the bf16 MFMA's rate and has no xf32 / TF32 form).  An f32 value is the exact
 * sum of three bf16 values (8 significant bits each); a product of two such sums is nine exact bf16 products, of which
 * the six that reach 2^-23 of |a b| are issued as bf16 MFMAs and accumulated in f32 - the operands, the accumulation,
 * the epilogue and the results are f32, and the error against fp64 is that of the f32 MFMA kernels
 * (tests/test_hip_conv.py::test_x3_*).  The same call sites as their f32 counterparts (fgn_conv2d_nhwc_f32 with a 1x1 /
 * stride 1 / unpadded kernel, fgn_conv1x1_dual_nhwc_f32, fgn_winograd_gemm_f32), same arguments, except that the weights
 * are given as their bf16-plane IMAGE (host-packed once: fgn_amd/ops.py::pack_x3):
 *   w_x3 [groups][K / 32][3 planes][cout_pad][32] bf16, plane 0 = w with the low 16 bits cleared, plane 1 the same of
 *   w - plane 0, plane 2 = w - plane 0 - plane 1; inside a K-tile chunk g (8 values) holds k = 4g..4g+3, 16+4g..16+4g+3 -
 *   the operand order of v_mfma_f32_16x16x32_bf16 under which ds_read_b128's lane groups read both operands without bank
 *   conflicts -, and the four 16-byte chunks of a 64-byte row are XOR-ed with tau[(n >> 2) & 3], tau = (0, 3, 2, 1).
 * fgn_x3_image_bytes = its size.  K >= 64, K % 32 == 0, Cout % 4 == 0, cout_pad % 128 == 0.
 * fgn_gemm_x3_f32: y[rows, Cout] = relu?(x[rows, K] W^T + shift + residual) directly (grouped: rows = n_groups *
 * grp_rows, image g for group g, first grp_valid rows of a group computed); bm 0 (= fgn_x3_row_tile) / 64 / 128 and
 * nterms 6 / 9 choose the kernel instance (tests, tools/x3_probe.py). */
size_t fgn_x3_image_bytes(int K, int npad, int n_groups);
int fgn_x3_row_tile(long long M, int Cout, int K, int grp_rows, int grp_valid);   /* 64 / 128: the kernel instance a launch of this shape runs on; 0: use the f32 entry point */
int fgn_gemm_x3_f32(const float* x, const void* w_x3, float* y, const float* shift, const float* residual, int rows, int K,
                    int Cout, int npad, int relu, int grp_rows, int grp_valid, int n_groups, int bm, int nterms,
                    void* stream);
int fgn_conv1x1_x3_nhwc_f32(const float* x, const void* w_x3, float* y, const float* scale, const float* shift,
                            const float* residual, const int32_t* n_img_dev, int n_img, int H, int W, int Cin, int Cout,
                            int cout_pad, int relu, void* stream);
int fgn_conv1x1_dual_x3_nhwc_f32(const float* x, const float* x2, const int32_t* x2_rows, int x2_total_rows,
                                 const void* w_x3, float* y, const float* shift, int rows, int Cin1, int Cin2, int Cout,
                                 int cout_pad, int relu, void* stream);
/* rows written, device count, untouched rows: as stated at fgn_winograd_gemm_f32, with the row tile of fgn_x3_row_tile(
 * n_groups * t_pad, Cout, Cin, t_pad, n_img * tiles_per_img); where that is 0 the call returns FGN_ERR_SHAPE and writes nothing */
int fgn_winograd_gemm_x3_f32(const float* V, const void* U_x3, float* Mo, const int32_t* n_img_dev, int n_img,
                             int tiles_per_img, int t_pad, int Cin, int Cout, int cout_pad, int n_groups, void* stream);
/* The same GEMMs with THREE f16 MFMA products per f32 product (conv_pw_h2_kernel, csrc/conv_pw_h2.h; the default of the
 * host wrappers): an f32 value scaled by a power of two into the f16 range is h + l to within 2^-23 of itself (h = f16(x),
 * l = f16(x - h), round to nearest), products of f16 values are exact in f32, and h_a h_b + h_a l_b + l_a h_b leaves out
 * only l_a l_b <= 2^-22 |a b| (per product ~2^-24 |a b| rms: the order of an f32 FMA chain's own rounding); f32 accumulation, f32 in / out, the f32 kernels' error against fp64
 * (tests/test_hip_conv.py::test_h2_*).  The scales are powers of two (exact) and taken out again inside the kernel: the
 * weights' per output column at pack time (fgn_amd/ops.py::pack_h2), the activations' found by the kernel itself per wave
 * and output tile (the first non-zero K-tile of a tile sets it; a later K-tile that would leave the f16 range picks a
 * new one and the accumulators follow by the exact ratio).  Same call sites and arguments as the x3 entry points, with
 *   w_h2: [groups][K / 32][2 planes][cout_pad][32] f16 of the column-scaled weights (k order and chunk swizzle of w_x3),
 *         then [groups][cout_pad] f32 inverse column scales.  fgn_h2_image_bytes = the size of both.
 * Shapes: as the x3 entry points, and Cout 48..64 on a 64-column tile (fgn_h2_row_tile decides).  fgn_gemm_h2_f32: the direct entry (tests, tools);
 * bm 0 (= fgn_h2_row_tile, fgn_h2_k_groups) / 64 / 128 / 264 force the tile on one K-group; 1064 = 64 rows on two K-groups
 * (K / 32 even and >= 4).  fgn_h2_k_groups: 2 = the launch runs its 64-row tiles on two sets of four waves, each on every
 * other K-tile (ungrouped launches of at most 256 tiles, one per CU, with an even and long enough K-tile count); 1 = one set.
 * ACCURACY CONTRACT of every entry point on conv_pw_h2_kernel (fgn_gemm_h2_f32, fgn_conv1x1_h2_nhwc_f32,
 * fgn_conv1x1_dual_h2_nhwc_f32, fgn_conv2d_pair_h2[_bm]_nhwc_f32, fgn_winograd_gemm_h2_f32).  It is PER WAVE: the 32 rows
 * (64 on the 128-row x 128-column tile) of an output tile that one wave holds share one activation scale S, chosen for the largest
 * finite |x| of those rows in the K-tile that set it.
 *   (1) Exactly summable operands give the exact result, whatever the tile, the K-groups or the order of the sum: when
 *       the activations have at most 22 and the weights at most 11 significant bits (or the other way round: the dropped
 *       l_a l_b is then zero), every element lies within 2^15 of its wave's maximum, and for every output element
 *       sum |a||w| + |shift| + |residual| is at most 2^22 times a power of two that divides each of its terms, y is the
 *       exact sum - bit for bit, with shift, residual and ReLU.  (f32 holds 2^24; the two spare bits are a margin for the
 *       matrix pipe's alignment inside a 32-deep dot product.)
 *   (2) An element within 2^15 of the maximum S was chosen for keeps both planes at full precision (22 bits).
 *   (3) A smaller element loses low bits of its l plane to the f16 subnormals: an absolute error of at most 2^-38 of that
 *       maximum per element, i.e. at most 2^-38 max|x| sum_k |w[n, k]| per output - a row far below its wave's largest
 *       row is right to that absolute bound only, not relative to itself; outputs stay finite.
 * tests/test_hip_conv_exact.py pins all three ((1), (2) by equality against integer arithmetic; (3) as a bound with rows
 * 2^30 and 2^40 below their wave's maximum); the operand classes are in tests/_exact_ref.py, DESIGN 7.6. */
size_t fgn_h2_image_bytes(int K, int npad, int n_groups);
int fgn_h2_k_groups(long long M, int Cout, int K, int grp_rows, int grp_valid);
int fgn_h2_row_tile(long long M, int Cout, int K, int grp_rows, int grp_valid);   /* 64 / 128: rows of a 128-column tile; 264: 128 rows x 64 columns (Cout 48..64); 0: use the f32 entry point */
/* A 3x3 or 1x1 convolution of any stride / padding with folded scale / shift / ReLU on ONE or TWO NHWC tensors that share
 * the weights (x1 == NULL: one; two: the query map and the support maps of a backbone layer, fgn_conv2d_pair_nhwc_f32's
 * call sites) as an implicit GEMM on conv_pw_h2_kernel.  w_h2 = the f16-plane image of the packed weights
 * [cout_pad][KH KW Cin] (K order tap, channel: fgn_amd/ops.py::pack_conv, pack_h2); Cin / 32 a power of two; the two
 * inputs within 2 GiB of each other. */
int fgn_conv2d_pair_h2_nhwc_f32(const float* x0, int n_img0, int H0, int W0, const float* x1, int n_img1, int H1, int W1,
                                const void* w_h2, float* y0, float* y1, const float* scale, const float* shift, int Cin,
                                int Cout, int cout_pad, int KH, int KW, int stride, int pad, int relu, void* stream);
/* the same with the tile code forced (bm as for fgn_gemm_h2_f32; tests, tools) */
int fgn_conv2d_pair_h2_bm_nhwc_f32(const float* x0, int n_img0, int H0, int W0, const float* x1, int n_img1, int H1, int W1,
                                   const void* w_h2, float* y0, float* y1, const float* scale, const float* shift, int Cin,
                                   int Cout, int cout_pad, int KH, int KW, int stride, int pad, int relu, int bm, void* stream);
int fgn_gemm_h2_f32(const float* x, const void* w_h2, float* y, const float* shift, const float* residual, int rows, int K,
                    int Cout, int npad, int relu, int grp_rows, int grp_valid, int n_groups, int bm, void* stream);
int fgn_conv1x1_h2_nhwc_f32(const float* x, const void* w_h2, float* y, const float* scale, const float* shift,
                            const float* residual, const int32_t* n_img_dev, int n_img, int H, int W, int Cin, int Cout,
                            int cout_pad, int relu, void* stream);
int fgn_conv1x1_dual_h2_nhwc_f32(const float* x, const float* x2, const int32_t* x2_rows, int x2_total_rows,
                                 const void* w_h2, float* y, const float* shift, int rows, int Cin1, int Cin2, int Cout,
                                 int cout_pad, int relu, void* stream);
/* the same with the tile code forced (bm as for fgn_gemm_h2_f32; tests, tools).  Launches with a second operand run on
 * conv_pw_h2_kernel_dual<waves along M, waves along N, row blocks, stages, K-groups>, every other launch on
 * conv_pw_h2_kernel<..., implicit-GEMM loader, K-groups>, which holds no second descriptor and no operand select - with one
 * exception: conv_pw_h2_kernel<2, 2, 1, 2, false, 2> (two K-groups, no implicit-GEMM loader) keeps the look at x2 at run
 * time (as a one-operand instance it measured slower), though launch_h2 never hands it a second operand. */
int fgn_conv1x1_dual_h2_bm_nhwc_f32(const float* x, const float* x2, const int32_t* x2_rows, int x2_total_rows,
                                    const void* w_h2, float* y, const float* shift, int rows, int Cin1, int Cin2, int Cout,
                                    int cout_pad, int relu, int bm, void* stream);
/* rows written, device count, untouched rows: as stated at fgn_winograd_gemm_f32, with the row tile of fgn_h2_row_tile(
 * n_groups * t_pad, Cout, Cin, t_pad, n_img * tiles_per_img) (64 / 128, 264 = 128 rows; rows of V past the valid ones reach neither a
 * wave's scale nor a valid row); where that is 0 the call returns FGN_ERR_SHAPE and writes nothing */
int fgn_winograd_gemm_h2_f32(const float* V, const void* U_h2, float* Mo, const int32_t* n_img_dev, int n_img,
                             int tiles_per_img, int t_pad, int Cin, int Cout, int cout_pad, int n_groups, void* stream);

/* The same convolution (w_packed, scale, shift, relu as in fgn_conv2d_nhwc_f32) on TWO NHWC tensors of different
 * geometry in one launch: x0 [n_img0,H0,W0,Cin] -> y0, x1 [n_img1,H1,W1,Cin] -> y1.  For the backbone layers that
 * stride over the spatial structure when the query image and the support crops go through the backbone together
 * (fgn.py:212,215: the 3x3 / stride 2 conv2 and the 1x1 / stride 2 shortcut of a stage's first block, the stem) -
 * the other layers of the two passes already share launches by sharing rows.  Per tensor the arithmetic of
 * fgn_conv2d_nhwc_f32 without split-K; no residual / in_scale / device-side count; Cout % 4 == 0. */
int fgn_conv2d_pair_nhwc_f32(const float* x0, float* y0, int n_img0, int H0, int W0, const float* x1, float* y1,
                             int n_img1, int H1, int W1, const float* w_packed, const float* scale, const float* shift,
                             int Cin, int Cout, int cout_pad, int KH, int KW, int stride, int pad, int relu,
                             void* stream);

/* Winograd F(2x2,3x3) form of a 3x3 / stride 1 / pad 1 convolution (same call sites as
 * fgn_conv2d_nhwc_f32: fgn_ag_rpn_head.py:48 rpn_conv, fgn_roi_head.py:236 shared_head conv2):
 *   fgn_winograd_input_f32   V[16][t_pad][C]   = B^T (x * in_scale?) B per 4x4 input tile
 *   fgn_winograd_gemm_f32    Mo[g] = V[g] U[g]^T for the 16 tile positions, one MFMA launch (64x64 kernel,
 *                            per-group weights); U [16][cout_pad][Cin] = G w G^T (host-packed, BN scale folded)
 *   fgn_winograd_output_f32  y = A^T Mo A + shift (ReLU), y [n_img,H,W,Cout]
 * tiles per image = ceil(H/2)*ceil(W/2); t_pad = fgn_winograd_t_pad(n_img*tiles) (a multiple of 128 rows: whole GEMM tiles per group).
 * Image i reads x[i / a_img_div]; in_scale [n_img][C] optional (AG-RPN guidance, fgn_ag_rpn_head.py:44; mask
 * guidance, fgn_roi_head.py:379). */
int fgn_winograd_input_f32(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev, int n_img,
                           int a_img_div, int H, int W, int C, int t_pad, void* stream);
int fgn_winograd_t_pad(int tiles_total);
/* WHAT A LAUNCH WRITES (all three fgn_winograd_gemm_* entries; tests/test_hip_wg_exact.py holds them to it): per group the
 * first min(n_img, *n_img_dev) * tiles_per_img rows of Mo (n_img_dev NULL: n_img * tiles_per_img) are the products; a launch
 * writes whole row tiles, so the rows from there up to the next multiple of the row tile (64 here; 64 / 128 on the image
 * entries: fgn_x3_row_tile / fgn_h2_row_tile) are unspecified, and every row behind that up to t_pad keeps its bytes.  A
 * count above n_img is clamped to n_img; a count of 0 writes nothing.  Columns [0, Cout) only: Mo is [n_groups][t_pad][Cout].
 * Group g reads U[g] alone.  On exactly summable operands (fgn_gemm_h2_f32's contract (1)) the products are exact. */
int fgn_winograd_gemm_f32(const float* V, const float* U, float* Mo, const int32_t* n_img_dev, int n_img,
                          int tiles_per_img, int t_pad, int Cin, int Cout, int cout_pad, int n_groups, void* stream);
int fgn_winograd_output_f32(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev, int n_img,
                            int H, int W, int C, int t_pad, int relu, void* stream);
/* F(4x4,3x3) form of the same convolutions (the default): 36 tile positions (n_groups = 36 in
 * fgn_winograd_gemm_f32), V / Mo [36][t_pad][C], tiles per image = ceil(H/4)*ceil(W/4); interpolation points
 * {0, 1, -1, 1/2, -2, inf} (winograd.hip).  4x fewer multiply-adds than the direct form, 1.78x fewer than F(2x2). */
int fgn_winograd4_input_f32(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev, int n_img,
                            int a_img_div, int H, int W, int C, int t_pad, void* stream);
int fgn_winograd4_output_f32(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev, int n_img,
                             int H, int W, int C, int t_pad, int relu, void* stream);
/* The F(4x4) transforms of TWO tensors of one layer (the query map and the support maps of a backbone layer, each with
 * its own image count and size) in one launch: tensor 0 fills tiles [0, n0*tiles(H0,W0)) of V / reads them from Mo,
 * tensor 1 the tiles behind them; no input scale, no device-side count.  t_pad >= all tiles. */
int fgn_winograd4_input2_f32(const float* x0, int n_img0, int H0, int W0, const float* x1, int n_img1, int H1, int W1,
                             float* V, int C, int t_pad, void* stream);
int fgn_winograd4_output2_f32(const float* Mo, const float* shift, float* y0, int n_img0, int H0, int W0, float* y1,
                              int n_img1, int H1, int W1, int C, int t_pad, int relu, void* stream);
/* Index width of the F(4x4) transforms.  The transforms above choose between two instances of each kernel from the sizes
 * alone: the NARROW one (32-bit byte offsets, a short prologue) when every tensor of the launch - x / y of both tensors,
 * in_scale, V / Mo [36][t_pad][C] - ends below 2 GiB, else the WIDE one (64-bit indices).  Both give the same bytes.
 * fgn_winograd4_index_bits -> 32 / 64, the choice for these sizes (n_img1 = 0: one tensor; with_scale: in_scale is read;
 * is_output: the output transform, else the input transform) - the launchers' own rule, one function;
 * nothing is allocated or launched.  32: the device kernels are wg4_input_narrow_kernel<V> / wg4_output_narrow_kernel<V>,
 * 64: wg4_input_kernel<V, eager> / wg4_output_kernel<V> (V, eager: fgn_winograd4_variant).
 * WHAT A DEVICE COUNT BELOW n_img LEAVES READABLE: the narrow instances load the patches of EVERY tile below the capacity
 * n_img and compare against *n_img_dev only before the stores, so with any of the F(4x4) entry points x must be readable
 * for all ceil(n_img / a_img_div) images, in_scale for all n_img rows and Mo for all n_img * tiles rows of each position,
 * whatever the count is (their values past the count reach no output); V and y past the count are not touched.  The _ix entries (tests, tools) run either form of the transform - x1 / y1 == NULL:
 * one tensor, else the two-tensor form - with index_bits 0 (by the sizes), 32 or 64 forced; 32 on sizes the narrow
 * instance cannot address is FGN_ERR_SHAPE.  vec: 0 = the channel vector width of fgn_winograd4_variant, 1 / 2 / 4 = that
 * many floats per thread (tools/wg4_ab.py measures the rule with it). */
int fgn_winograd4_index_bits(int n_img, int a_img_div, int H, int W, int n_img1, int H1, int W1, int C, int t_pad,
                             int with_scale, int is_output);
int fgn_winograd4_input_ix_f32(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev, int n_img,
                               int a_img_div, int H, int W, int C, int t_pad, const float* x1, int n_img1, int H1, int W1,
                               int index_bits, int vec, void* stream);
int fgn_winograd4_output_ix_f32(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev, int n_img, int H,
                                int W, int C, int t_pad, int relu, float* y1, int n_img1, int H1, int W1, int index_bits,
                                int vec, void* stream);
/* Which instance of the F(4x4) transform kernels a layer with `tiles_total` tiles and C channels launches: the
 * channel vector width of a thread (1, 2 or 4 floats) * 10 + 1 when the input transform issues all 36 loads up front.
 * Informational (lets a profiler name the kernel of a launch); the transforms choose it themselves. */
int fgn_winograd4_variant(int tiles_total, int C, int is_output);
/* Weight side of both Winograd forms on the device: U[(a*R+b)][co][ci] = sum_ij G[a][i] w[co][ci][i][j] G[b][j] (R = m + 2,
 * fp64 arithmetic, one rounding), written IN PLACE into U [R*R][cout_pad][Cin] (rows past cout untouched).  w is the
 * torch-layout weight [Cout][Cin][3][3], G the [R][3] fp64 table of the interpolation points.  What mmcv's optimizer
 * step + the next forward need between two training steps (no reference counterpart: cuDNN picks its own algorithm). */
int fgn_winograd_pack_weights_f32(const float* w, const double* G, float* U, int cout, int cin, int cout_pad, int m,
                                  void* stream);

/* NCHW [n,3,H,W] -> NHWC4 [n,H,W,4] (input side of fgn.py:212,215) */
int fgn_nchw3_to_nhwc4_f32(const float* x, float* y, int n_img, int H, int W, void* stream);

/* uint8 channels-last [n,H,W,3] -> the same NHWC4 [n,H,W,4] fp32 stem input, normalised on the way: y[..,c] =
 * lut[c][x[..,c]] for c < 3, y[..,3] = +0.0f.  lut: [3][256] fp32 in device memory, built by the host in the data
 * loader's own arithmetic ((v / scale - mean[c]) / std[c], fgn_amd.ops.input_lut), so y is bit-identical to
 * fgn_nchw3_to_nhwc4_f32 of the host-normalised image by construction - no device division is involved.  x needs no
 * alignment (a pointer that is not dword-aligned takes a pixel-per-lane path).  An empty tensor is FGN_OK. */
int fgn_u8hwc3_to_nhwc4_f32(const unsigned char* x, const float* lut, float* y, int n_img, int H, int W, void* stream);

/* Query resize behind the upload (BaseFewShotISEG.get_query, base_fst.py:876-887).  Both entries compute the integer
 * bilinear rule of fgn_amd.fewshot_ds (resize_taps: half-pixel centres, clamped edges, 11-bit weights, round half up; a
 * restatement of cv2.resize's design that no reference golden pins) and agree with resize_image_u8 / resize_masks bit for
 * bit.  Every dimension is at most 16384 (int32 arithmetic); larger or negative ones are FGN_ERR_SHAPE, a null pointer
 * FGN_ERR_ARG, an empty output FGN_OK with no launch.
 *
 * fgn_resize_u8hwc3_to_nhwc4_f32: image b is [h_b][w_b][3] bytes at src + b * src_stride_bytes (no alignment needed),
 * {h_b, w_b} = src_hw[b] is read ON THE DEVICE (int32 [n_img][2]) - the launch does not depend on the source sizes, so
 * one captured launch serves all of them.  y [n_img][H][W][4] fp32 = fgn_u8hwc3_to_nhwc4_f32 of the resized images.
 * An image with h_b or w_b outside 1..16384 or h_b * w_b * 3 > src_stride_bytes is written as +0.0f and not read. */
int fgn_resize_u8hwc3_to_nhwc4_f32(const unsigned char* src, long long src_stride_bytes, const int* src_hw,
                                   const float* lut, float* y, int n_img, int H, int W, void* stream);
/* fgn_resize_mask_u8: src [G][h][w] bytes (nonzero = set; bool storage) -> dst [G][H][W] 0 / 1 bytes, set where the
 * weighted sum of the four taps reaches half (cv2.resize(m.astype(uint8)).astype(bool)). */
int fgn_resize_mask_u8(const unsigned char* src, unsigned char* dst, int G, int h, int w, int H, int W, void* stream);

/* Query augmentation behind the upload (BaseFewShotISEG.augment_with_imgaug, base_fst.py:735-770: flip, affine warp and
 * channel order of natural_fst.py:18-35), composed with the resize above into one bilinear gather from the source image.
 * Both entries compute the integer rule of fgn_amd.fewshot_ds (query_augment_record; a restatement of imgaug's operators
 * that no reference golden pins) and agree with augment_image_u8 / augment_masks bit for bit.  Return codes as above.
 *   record, int32 [16]: {h, w, kind, flip, border, perm, c00, c01, c10, c11, c02 lo, c02 hi, c12 lo, c12 hi, -, -}
 *     kind 0: the taps of the resize, of column W-1-ox under flip.
 *     kind 1: source coordinate (U, V) = c (ox, oy, 1) in int64, units of 2^-20 samples; i0 = U >> 20, w1 =
 *             ((U & (2^20-1)) + 256) >> 9, w0 = 2048 - w1, taps i0 and i0 + 1; a tap outside the image reads the
 *             symmetric extension (border 1: r = k mod 2n, r < n ? r : 2n-1-r) or 0 (border 0).
 *     perm: index into itertools.permutations(range(3)); output channel c is table c of blended byte p[c].
 *   A record is out of range when h or w is outside 1..16384, kind, flip, border or perm outside its set, a linear
 *   coefficient beyond +-2^26 or an offset beyond +-2^40.
 *
 * fgn_augment_u8hwc3_to_nhwc4_f32: the contract of fgn_resize_u8hwc3_to_nhwc4_f32 with recs int32 [n_img][16] read ON THE
 * DEVICE in place of src_hw: no launch argument depends on a source size or on the augmentation.  An image whose record
 * is out of range or with h * w * 3 > src_stride_bytes is written as +0.0f and not read. */
int fgn_augment_u8hwc3_to_nhwc4_f32(const unsigned char* src, long long src_stride_bytes, const int* recs,
                                    const float* lut, float* y, int n_img, int H, int W, void* stream);
/* fgn_augment_mask_u8: the contract of fgn_resize_mask_u8 with one record (device, int32 [16]) for the G masks of an
 * image; taps outside the image are 0 whatever the border.  A record out of range, or one whose (h, w) is not the
 * launch's, gives empty masks and src is not read. */
int fgn_augment_mask_u8(const unsigned char* src, unsigned char* dst, const int* rec, int G, int h, int w, int H, int W,
                        void* stream);

/* Photometric query augmentation on the source bytes, ahead of the two gathers above (the other six operators of
 * augs_seq, natural_fst.py:18-35: Gaussian noise, impulse noise, Gaussian blur, hue, saturation, brightness): one
 * out-of-place pass src -> dst, both [n_img][stride_bytes] with image b as [h_b, w_b, 3] bytes at the start of slot b
 * (any byte alignment).  It computes the integer rule of fgn_amd.fewshot_ds (query_photometric_record; a restatement of
 * imgaug's operators that no reference golden pins) and agrees with photometric_image_u8 bit for bit.
 *   recs int32 [n_img][64], read ON THE DEVICE (no launch argument depends on a source size or on an operator):
 *     {h, w, op, seed, a0, a1, rx, ry, payload ...}
 *     op 0: copy.
 *     op 1: Gaussian noise.  u = word 0 of Philox4x32-10 at counter (y * w + x, 0, 0, op), key (seed, 0); payload 12
 *           thresholds L; k = #{L[j] <= u} - 12 + #{~u < L[j]}; the pixel's three bytes become clip(byte + k, 0, 255).
 *     op 2: impulse noise.  Byte c is replaced where word c < a1 * 2^32 + a0, by 255 where bit c of word 3 is set, else 0.
 *     op 3: Gaussian blur.  Radii rx, ry in 1..16; weights of offset |k|: w[0..rx] at 8, w[0..ry] at 25, each axis summing
 *           to 2048; byte = (sum of byte * wy * wx + 2^21) >> 22; reflect-101 border.
 *     op 4 / 5 / 6: hue / saturation / brightness with a0 = the amount as rint(a * 3 / 255 * 2^16) mod 6 * 2^16 /
 *           rint(a / 255 * 2^23) / rint(a * 2^7) (DESIGN.md 4.4.6 for the fixed-point rule).
 *   Bytes [0, 3 h w) of a slot are written.  A record out of range (size outside 1..16384, operator, radius, weights not
 *   summing to 2048, amount outside its set) or with h * w * 3 > stride_bytes gets its whole slot written as zeros and none
 *   of its source bytes are read.  src and dst must not overlap (FGN_ERR_ARG): the blur reads neighbours. */
int fgn_photometric_u8hwc3(const unsigned char* src, unsigned char* dst, long long stride_bytes, const int* recs,
                           int n_img, void* stream);

/* A chain of the operators above in ONE pass over the same slots (COCODS.augs_seq, coco_ds.py:45-59: one of AddToHue /
 * AddToSaturation / AddToBrightness, then GaussianBlur): image b has n_ops records, recs int32 [n_img][n_ops][64] read ON
 * THE DEVICE, applied in order.  The rule is the left fold of photometric_image_u8 over the records
 * (fgn_amd.fewshot_ds.photometric_chain_u8) and the kernel agrees with it bit for bit; the point operators run on a pixel
 * in registers, where the chain ends in a blur while its tile and halo are staged (each staged pixel with its own flat
 * index y * w + x as the noise counter), so the image is read once and written once.
 *   A chain is point operators, then at most one blur: every record must pass the checks above, all records of an image
 *   carry the same (h, w), and a blur record has only operator-0 records behind it (operator-0 records may stand
 *   anywhere).  An image that fails gets its whole slot written as zeros and none of its source bytes are read.
 *   n_ops outside 1..3: FGN_ERR_SHAPE.  src and dst must not overlap (FGN_ERR_ARG).  Other return codes as above. */
int fgn_photometric_chain_u8hwc3(const unsigned char* src, unsigned char* dst, long long stride_bytes, const int* recs,
                                 int n_ops, int n_img, void* stream);

/* Supports from the source image behind the upload (BaseFewShotISEG.get_support, base_fst.py:1043-1167: get_crop with
 * reflected context, bicubic resize of the longer side to S, centre pad): one launch for all n = B * N * K instances of
 * a batch.  The arithmetic is the integer rule of fgn_amd.fewshot_ds (cubic_taps: cubic convolution A = -3/4, half-pixel
 * centres, 10-bit fraction, 11-bit weights, taps clamped into the crop; support_geometry; a restatement of imgaug's
 * bicubic that no reference golden pins) and the outputs agree with support_from_source bit for bit.
 *   src  instance i's image window [wh_i][ww_i][3] bytes at src + i * src_stride_bytes (no alignment needed)
 *   msk  its mask window [wh_i][ww_i] bytes (nonzero = set) at msk + i * msk_stride_bytes
 *   recs int32 [n][16], read ON THE DEVICE: {H, W, y0, x0, ch, cw, nh, nw, top, left, reflect, wy, wx, wh, ww, -} =
 *        source size, crop origin in the source frame (may be negative) and crop size, resized size and its place in
 *        the S x S support, border mode (1: periodic reflection of period 2 (n - 1), 0: zeros), and the window - the rows
 *        [wy, wy + wh) and columns [wx, wx + ww) of the source that were uploaded.  No launch argument depends on a
 *        source, window or crop size: one captured launch serves every support set.
 *   y    [n][S][S][4] fp32 = fgn_u8hwc3_to_nhwc4_f32 of the support crops (the padding is byte 0 through the table)
 *   m    [n][S][S] 0 / 1 bytes: the support masks (always zero outside the image and in the padding)
 * Every source index is clamped into the window.  An instance whose record is out of range - a size outside 1..16384,
 * nh / nw / top / left that do not fit S, an origin beyond +-2 * 16384, a window outside its image or larger than its
 * slot (wh * ww * 3 > src_stride_bytes or wh * ww > msk_stride_bytes) - is written as padding with an empty mask and
 * none of its slot is read.  A null pointer is FGN_ERR_ARG; negative n, S or strides, or S > 16384, FGN_ERR_SHAPE; an
 * empty output FGN_OK with no launch. */
int fgn_support_from_source_f32(const unsigned char* src, long long src_stride_bytes, const unsigned char* msk,
                                long long msk_stride_bytes, const int* recs, const float* lut, float* y,
                                unsigned char* m, int n, int S, void* stream);

/* The byte-output form of fgn_support_from_source_f32 (the same kernel body: record, taps, window reads, validity rule
 * and mask are those above): crop [n][S][S][3] uint8 = fewshot_ds.support_from_source's crop itself, bit for bit - the
 * clamped bytes, byte 0 in the padding and for an instance whose record is out of range - and m as above.  No table.
 * It feeds fgn_photometric_u8hwc3 (n slots of stride 3 * S * S) and fgn_support_augment_f32.  Return codes as above. */
int fgn_support_from_source_u8(const unsigned char* src, long long src_stride_bytes, const unsigned char* msk,
                               long long msk_stride_bytes, const int* recs, unsigned char* crop, unsigned char* m,
                               int n, int S, void* stream);

/* Support augmentation behind the cut (get_support with augment_spp, base_fst.py:1151-1153: per instance, on the S x S
 * crop after resize and pad), ONE launch for all n instances: fewshot_ds.augment_image_u8 / augment_masks at S -> S
 * followed by the table, bit for bit.
 *   crop [n][S][S][3] uint8, msk [n][S][S] bytes (nonzero = set): what fgn_support_from_source_u8 makes
 *   recs int32 [n][16], read ON THE DEVICE: the records of fgn_augment_u8hwc3_to_nhwc4_f32 with h = w = S.  No launch
 *        argument depends on an augmentation.
 *   lut  [3][256] fp32;  y [n][S][S][4] fp32: channel c = table c of byte order[c] of the gathered pixel;  m [n][S][S]
 *        0 / 1 bytes: the mask by the image's taps, a tap outside the frame reading 0 whatever the border, set where
 *        acc >= 2^21.
 * Kind 0 copies column ox (S-1-ox under flip); kind 1 is the bilinear gather, whose symmetric border reflects the S x S
 * frame, pad bands included.  An instance whose record is out of range, or whose h or w is not S, is written as the
 * table's byte-0 pixel with an empty mask and none of its bytes are read; its neighbours are untouched.  A null pointer,
 * or crop / y or msk / m overlapping, is FGN_ERR_ARG; n < 0 or S outside 0..16384 FGN_ERR_SHAPE; n * S == 0 FGN_OK with
 * no launch. */
int fgn_support_augment_f32(const unsigned char* crop, const unsigned char* msk, const int* recs, const float* lut,
                            float* y, unsigned char* m, int n, int S, void* stream);

/* 3x3/2 pad 1 max-pool of the ResNet stem */
int fgn_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n_img, int H, int W, int C, void* stream);

/* GroupNorm over NHWC (+ residual) (+ ReLU): the norm layers of the from-scratch backbone variant
 * (fgn_r50_c4_scratch.py:16-23, norm_cfg GN(32); torch.nn.GroupNorm inside mmdet ResNet at
 * fgn.py:71-73).  y = (x - mean_g) * rstd_g * gamma[c] + beta[c] per (image, group);
 * ws from fgn_group_norm_workspace_bytes.  x == y (in place) is allowed.  Mean and variance are fp64 sums of the
 * values shifted by the group's first one (fixed order, no atomics): accurate whatever mean / std is. */
size_t fgn_group_norm_workspace_bytes(int n_img, int HW, int C, int groups);
int fgn_group_norm_nhwc_f32(const float* x, float* y, const float* gamma, const float* beta,
                            const float* residual, void* ws, size_t ws_bytes, int n_img, int HW, int C,
                            int groups, float eps, int relu, void* stream);

/* AvgPool2d(2, stride 2, ceil_mode, count_include_pad=False): shortcut of a strided bottleneck
 * under avg_down (fgn_r50_c4_scratch.py:18-19); out [n, ceil(H/2), ceil(W/2), C] */
int fgn_avgpool2x2_nhwc_f32(const float* x, float* y, int n_img, int H, int W, int C, void* stream);

/* RoIAlign (avg), rois [R,5] = (batch_idx,x1,y1,x2,y2), out [R,P,P,C].
 * aligned=1,sampling_ratio=0 : mmcv.ops.RoIAlign (fgn_roi_head.py:331,366)
 * aligned=0,sampling_ratio=-1: torchvision.ops.roi_align (fgn_roi_head.py:429,432)
 * post_shift [C] (optional) is added and ReLU applied after the average: RoIAlign is linear per channel, so
 * the first 1x1 conv of the shared_head (fgn_roi_head.py:236) is applied to the feature map once and its
 * BN shift + ReLU here, instead of a conv over every RoI's 49 pixels. */
int fgn_roi_align_nhwc_f32(const float* fmap, const float* rois, float* out, const int32_t* n_rois_dev,
                           int n_rois, int n_img, int H, int W, int C, int out_size, float spatial_scale,
                           int sampling_ratio, int aligned, const float* post_shift, int relu, void* stream);
/* The same pooling of TWO maps of one spatial size at the same RoIs in one launch: out [R,P,P,C] from fmap, out2
 * [R,P,P,C2] from fmap2 (+ post_shift2 [C2], ReLU) - the C4 map and the map of the shared head's first 1x1 conv taken
 * in front of the pooling (fgn_roi_head.py:331-336, 366-369).  Identical bytes to two single-map calls. */
int fgn_roi_align2_nhwc_f32(const float* fmap, const float* fmap2, const float* rois, float* out, float* out2,
                            const int32_t* n_rois_dev, int n_rois, int n_img, int H, int W, int C, int C2,
                            int out_size, float spatial_scale, int sampling_ratio, int aligned,
                            const float* post_shift2, int relu2, void* stream);
/* same for a single-channel uint8/bool map [n_img,H,W] -> [R,P,P] (support masks,
 * fgn_roi_head.py:429) */
int fgn_roi_align_mask_u8(const uint8_t* mask, const float* rois, float* out, int n_rois, int n_img, int H,
                          int W, int out_size, float spatial_scale, int sampling_ratio, int aligned,
                          void* stream);

/* out[g][c] = mean_{k<K,p<P} x[g*K+k][p][c] * (weights ? weights[g*K+k][p] : 1)
 * (fgn_ag_rpn_head.py:38-41 with weights=NULL; fgn_roi_head.py:444-447 with the pooled masks) */
int fgn_support_class_vectors_f32(const float* x, const float* weights, float* out, int n_groups, int K,
                                  int P, int C, void* stream);
/* out[g][p][c] = mean_k x[g*K+k][p][c]   (fgn_roi_head.py:439-442) */
int fgn_support_kmean_f32(const float* x, float* out, int n_groups, int K, int P, int C, void* stream);
/* out[i][:] = table[labels[i] + n_ways*img(i)][:]  (fgn_roi_head.py:707-714); rois may be NULL (img 0) */
int fgn_gather_support_vectors_f32(const float* table, const int64_t* labels, const float* rois, float* out,
                                   const int32_t* n_dev, int n, int n_ways, int C, void* stream);

/* out[n][p][c] = x[n / div][p][c] * v[n][c]  (guidance multiply, fgn_ag_rpn_head.py:44-46, materialised
 * for the LDS-DMA conv kernel where a layer does not take the Winograd form); x [n_out/div, P, C], v [n_out, C], out [n_out, P, C] */
int fgn_scale_channels_f32(const float* x, const float* v, float* out, int n_out, int div, int P, int C,
                           void* stream);

/* Fused tail of count_one_roi_by_n_spp + BBoxHead.forward (fgn_roi_head.py:253-279,338):
 * x = Q[r] + S[img*N+n]; GroupNorm(32)+ReLU; 7x7 avg-pool; fc_cls/fc_reg.
 * Q [R,49,C], S [B*N,49,C] (bias included), fc_weight [6,C] (2 cls rows then 4 reg rows) */
int fgn_relation_gn_head_f32(const float* Q, const float* S, const float* rois, const float* gn_weight,
                             const float* gn_bias, const float* fc_weight, const float* fc_bias, float* cls_out,
                             float* reg_out, const int32_t* n_rois_dev, int n_rois, int n_ways, int C,
                             int gn_groups, int roi_size, float eps, float* rel_out_debug, float* scratch, void* stream);
/* scratch of fgn_relation_gn_head_f32: per (RoI, 256-channel chunk, class) partial fc products, summed in chunk order */
size_t fgn_relation_gn_head_scratch_bytes(int n_rois, int n_ways, int C);

/* AG-RPN merge: per-anchor arg-max over the N guided passes (fgn_ag_rpn_head.py:81-113) + sigmoid.
 * head [B*N,HW,head_channels]: channels [0,A) objectness, [A,5A) deltas. Outputs in (y,x,a) order. */
int fgn_rpn_merge_f32(const float* head, float* logits, float* scores, float* deltas, int batch, int n_ways,
                      int HW, int n_anchors, int head_channels, void* stream);

/* Proposals (mmdet RPNHead._get_bboxes_single/_bbox_post_process via fgn.py:229-235):
 * top nms_pre -> delta2bbox -> min size -> NMS -> max_per_img.  proposals [B,max_per_img,5],
 * n_props [B]. scratch: fgn_rpn_proposals_scratch_bytes(). dbg_topk_idx optional [B,cap]. */
size_t fgn_rpn_proposals_scratch_bytes(int batch, int n_total, int nms_pre);
/* rois_out (optional) [B*max_per_img,5]: the same boxes as (image index, x1, y1, x2, y2) = bbox2roi (fgn_roi_head.py:556) */
/* pre_zeroed (optional): fgn_rpn_proposals_zeroed_bytes(batch) bytes of ZERO-FILLED device memory (fresh per call);
 * when given, the top-k selection of the ~63 000 scores runs as multi-workgroup kernels in front of the proposal
 * kernel (same result, bit for bit) */
size_t fgn_rpn_proposals_zeroed_bytes(int batch);
int fgn_rpn_proposals_f32(const float* scores, const float* deltas, const float* base_anchors, void* scratch,
                          void* pre_zeroed, float* proposals, float* rois_out, int32_t* n_props, int32_t* dbg_topk_idx, int batch, int feat_h,
                          int feat_w, int n_anchors, int stride, float img_h, float img_w,
                          const float* host_means4, const float* host_stds4, float max_ratio, int nms_pre,
                          float min_bbox_size, float iou_thr, int max_per_img, void* stream);

/* count_modified_cls_bbox + BBoxHead.get_bboxes + multiclass_nms, one workgroup per image
 * (fgn_roi_head.py:302-326, 606-613).  `batch` images with n_rois RoIs each, stacked: rois [batch*n_rois,5],
 * cls_raw [batch*n_rois*n_ways,2], reg_raw [batch*n_rois*n_ways,4], n_rois_dev (optional) [batch];
 * det_bboxes [batch*max_per_img,5], det_labels int64 [batch*max_per_img], n_dets [batch]; image i carries
 * image index img_index + i in mask_rois_out.  scratch: batch * fgn_det_post_scratch_bytes() bytes. */
size_t fgn_det_post_scratch_bytes(int max_rois, int n_ways);   /* per image */
int fgn_det_post_f32(const float* rois, const float* cls_raw, const float* reg_raw, const int32_t* n_rois_dev,
                     void* scratch, float* det_bboxes, float* mask_rois_out /* optional [max_per_img,5]: (img_index, box),
                     the mask branch's bbox2roi, fgn_roi_head.py:654 */, int img_index, int64_t* det_labels, int32_t* n_dets,
                     float* dbg_scores /* optional, tests / diagnostics: n_rois*(n_ways+1) softmax scores of the first image
                     + 16 words of phase stamps */,
                     int batch, int n_rois, int n_ways, float img_h, float img_w, const float* host_means4,
                     const float* host_stds4, float max_ratio, float score_thr, float iou_thr, int max_per_img,
                     void* stream);

/* conv_logits (1x1, one class) + sigmoid on the un-shuffled deconv output [D,P*P,4,C];
 * logits/prob [D,2P,2P] (FCNMaskHead, fgn_roi_head.py:380; sigmoid of get_seg_masks).  bias_dev (optional): the bias
 * as one float in device memory, read by the kernel instead of `bias` (a training loop updates it on the device). */
int fgn_mask_logits_f32(const float* x, const float* w, float bias, const float* bias_dev, float* logits, float* prob,
                        const int32_t* n_dev, int n_det, int roi_size, int C, void* stream);

/* _do_paste_mask + threshold (fgn_roi_head.py:668-671): out uint8 [D,H,W].
 * skip_empty = 1: mmdet's CPU path (paste inside the integer-expanded box only - the CPU reference of north_star);
 * skip_empty = 0: its CUDA path (the grid spans the whole image; the reference runs on cuda:0, main.py:365).  The two
 * agree for thr >= 0.5 (the configured 0.5, fgn_r50_c4_densecl.py:186) on boxes of positive width and height, and
 * differ below it (and on degenerate boxes, whose grid coordinate mmdet sets to 0: the mask's centre line everywhere). */
int fgn_mask_paste_u8(const float* prob, const float* boxes, int box_stride, uint8_t* out, const int32_t* n_dev,
                      int n_det, int img_h, int img_w, int mask_size, float thr, int skip_empty, void* stream);

/* Fused paste + threshold + COCO RLE (replaces get_seg_masks -> .cpu() -> pycocotools encode,
 * fgn_roi_head.py:668-671 + fgn.py:267,281): out_bytes [D,byte_cap] holds the COCO "counts"
 * string of detection d in its first out_len[d] bytes.  trans_scratch uint32 [D,trans_cap].
 * overflow[d] != 0: a cap was too small, use fgn_mask_paste_u8 + host RLE for that detection. */
int fgn_mask_rle(const float* prob, const float* boxes, int box_stride, uint32_t* trans_scratch,
                 uint8_t* out_bytes, int32_t* out_len, int32_t* overflow, const int32_t* n_dev, int n_det,
                 int img_h, int img_w, int mask_size, float thr, int trans_cap, int byte_cap, int skip_empty,
                 void* stream);

/* fgn_mask_rle for a batch whose results are wanted at SOURCE size, one launch: row r = b * n_det + d of
 * prob / boxes / out_* / trans_scratch is detection d of image b.  src_hw int32 [batch][2] = (h_b, w_b) IN DEVICE
 * MEMORY, read by the kernel (the launch is the same for every source size); n_dev int32 [batch] (or null: n_det each).
 * The boxes are network-frame boxes of a (net_h, net_w) network; each is divided by the image's scale
 * s_x = (float)((double)net_w / w_b), s_y = (float)((double)net_h / h_b) (correctly rounded f32 division, no clipping)
 * and pasted into h_b x w_b.  boxes_src (optional) float [batch * n_det][4]: the divided boxes.  An image whose size is
 * outside 1..16384 yields out_len = 0, overflow = 0 and zero boxes_src rows. */
int fgn_mask_rle_src(const float* prob, const float* boxes, int box_stride, const int32_t* src_hw,
                     uint32_t* trans_scratch, uint8_t* out_bytes, int32_t* out_len, int32_t* overflow, float* boxes_src,
                     const int32_t* n_dev, int batch, int n_det, int net_h, int net_w, int mask_size, float thr,
                     int trans_cap, int byte_cap, int skip_empty, void* stream);

/* COCO RLE of dense binary masks on the device: the query's ground-truth masks, which the reference copies to
 * the GPU with the batch (fgn.py:92-99) and encodes on the host with pycocotools (fgn.py:298, `qry_isegmaps_rle`).
 * masks [n][H][W] bytes (non-zero = set); out_bytes [n][byte_cap], out_len [n], overflow [n] (a cap was exceeded:
 * the caller encodes that mask on the host).  scratch: fgn_dense_rle_scratch_bytes(). */
size_t fgn_dense_rle_scratch_bytes(int n_masks, int img_h, int img_w, int trans_cap);
int fgn_dense_mask_rle(const uint8_t* masks, void* scratch, size_t scratch_bytes, uint8_t* out_bytes,
                       int32_t* out_len, int32_t* overflow, int n_masks, int img_h, int img_w, int trans_cap,
                       int byte_cap, void* stream);

/* COCO RLE as an INPUT, decoded on the device: the masks the reference's COCO dataset keeps as [size, counts]
 * (coco_ds.py:195-207) and decodes on the host for every sample (maskUtils.decode in get_isegmap, coco_ds.py:265-278).
 * n masks, or windows of them, in ONE launch; output i is exactly the bytes a dense upload of that window would hold.
 *   ends uint32 [n_ends]: the cumulative run ends of all masks concatenated, each mask counted from its own 0
 *        (fgn_amd.rle.RleMasks; a repeated end is a zero-length run)
 *   recs int32 [n][8], read ON THE DEVICE: {h, w, wy, wx, wh, ww, run0, n_runs} = the mask size, the window of it to
 *        produce (rows [wy, wy + wh), columns [wx, wx + ww)) and its slice ends[run0, run0 + n_runs)
 *   out  output i is [wh][ww] bytes, each 0 or 1, row-major, at out + i * out_stride_bytes; no alignment is assumed, and
 *        the bytes behind the window in its row of the slot are not written
 * Pixel (y, x) of a mask sits at column-major position p = x * h + y (< 2^28) and its value is r & 1, r = the number
 * of entries of the slice that are <= p.  The kernel is safe for ANY contents of ends: every index it forms lies in
 * [run0, run0 + n_runs); a slice that is not monotone gives garbage bits, never a read outside it.
 * A record is out of range when a size is outside 1..16384, the window is empty or leaves the mask, wh > max_wh or
 * ww > max_ww, wh * ww > out_stride_bytes, n_runs < 1, or the slice leaves [0, n_ends): none of its runs is read, and
 * its window is written as zeros where wh >= 1, ww >= 1 and wh * ww <= out_stride_bytes, and not at all otherwise.
 * A null pointer is FGN_ERR_ARG; negative n, stride or n_ends, max_wh / max_ww above 16384, or
 * n * ceil(max_ww / 256) >= 2^24 (the grid), FGN_ERR_SHAPE; n == 0 or
 * an empty maximum window FGN_OK with no launch (pointers are not looked at). */
int fgn_rle_decode_u8(const uint32_t* ends, long long n_ends, const int32_t* recs, unsigned char* out,
                      long long out_stride_bytes, int n, int max_wh, int max_ww, void* stream);

/* Box + colour as an INPUT, made into masks on the device: the reference's character datasets (MNISTISEG, OMNIISEG)
 * store a box and an RGB colour per instance and derive the mask from the image on the host for every sample
 * (get_char_mask_by_color, create_img_from_chars.py:136-158).  n masks in ONE launch, from image bytes that are on the
 * device already; output i is exactly the bytes a dense upload of that mask would hold.
 *   src  uint8, the image slot: row r starts at src + r * src_stride_bytes and holds an image [h][w][3] (RGB bytes,
 *        packed, no padding) at its front; src_cap_bytes of every row may be read; src_rows rows.  No alignment is
 *        assumed: src and the stride may be any byte count.
 *   recs int32 [n][16], read ON THE DEVICE: {row, h, w, y0, x0, y1, x1, lo_r, lo_g, lo_b, hi_r, hi_g, hi_b, out, 0, 0}
 *        = the slot row the mask reads and the size of the image in it, the box (rows [y0, y1), columns [x0, x1)) in
 *        that frame, the inclusive colour window (the host forms lo = max(c - shift, 0), hi = min(c + shift, 255)) and
 *        the index of the output
 *   out  output `out` of a record is [h][w] bytes, each 0 or 1, row-major, at out + out * out_stride_bytes; n_out
 *        outputs exist.  It is written IN FULL, zeros outside the box included (no memset is needed); the bytes behind
 *        h * w in its stride are not written.  No alignment is assumed.
 * p(y, x) = all_c(lo_c <= img[y][x][c] <= hi_c) for (y, x) inside the box and 0 outside it; the mask is the OR of p
 * over the 3x3 neighbourhood for (y, x) inside the box and 0 outside: a pixel outside the box never dilates in, even
 * where it matches the colour, and no pixel outside the image is read (OpenCV's dilate on the ROI array: the border
 * does not contribute).  An empty box gives a mask of zeros.
 * The kernel is safe for ANY contents of recs: every address it reads lies inside 3 * h * w <= src_cap_bytes of a row
 * below src_rows, every address it writes inside h * w <= out_stride_bytes of an output below n_out.  A record is out
 * of range when a size is outside 1..16384, h > max_h or w > max_w, row is outside [0, src_rows), 3 * h * w >
 * src_cap_bytes, or the box is not 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w: none of its pixels is read and its output
 * is written as zeros where 0 <= out < n_out, h >= 1, w >= 1 and h * w <= out_stride_bytes, and not at all otherwise.
 * Two records naming the same output race (whole bytes, 0 or 1): the caller gives every record its own.
 * Negative n, src_rows, n_out, strides or capacity, max_h / max_w outside 0..16384, or n * ceil(max_w / 64) >= 2^24
 * (the grid) is FGN_ERR_SHAPE; n == 0 or an empty maximum size FGN_OK with no launch (pointers are not looked at);
 * a null pointer otherwise FGN_ERR_ARG. */
int fgn_color_mask_u8(const unsigned char* src, long long src_stride_bytes, long long src_cap_bytes, int src_rows,
                      const int32_t* recs, int n, unsigned char* out, long long out_stride_bytes, int n_out, int max_h,
                      int max_w, void* stream);

/* COCO polygons as an INPUT, rasterised on the device (fgn_amd/polygon.py states the rule: pycocotools' rleFrPoly and
 * merge, which the reference runs once at dataset build, coco_ds.py:246-263).  n masks, or windows of them, from ONE
 * blob in TWO launches; output i is exactly the bytes a dense upload of that window would hold.
 *   blob int32, read ON THE DEVICE, three tables of 8 ints per record, back to back:
 *        masks [n]       {h, w, wy, wx, wh, ww, part0, n_parts}: the mask size, the window of it to produce (rows
 *                        [wy, wy + wh), columns [wx, wx + ww)) and its parts [part0, part0 + n_parts), ORed
 *        parts [n_parts] {edge0, n_edges, points, ends0, cap, h, w, 0}: its edges [edge0, edge0 + n_edges), the length
 *                        of its path, its slice scratch[ends0, ends0 + cap) with cap a power of two within 1..8192 that
 *                        is at least the number of positions the part toggles, and the size of its mask
 *        edges [n_edges] {xs, ys, steps, major | flip << 1, s lo, s hi, first, 0}: on the 5x grid, the start after the
 *                        flip, max(dx, dy), whether x is the major axis, whether the edge is walked from its far end,
 *                        the slope as the two halves of a double, and the index of its first point in its part's path
 *        blob_ints >= 8 * (n + n_parts + n_edges) ints can be read.
 *   scratch uint32 [scratch_len]: every part's sorted positions, padded with 0xFFFFFFFF to cap; written by the first
 *        launch, read by the second; its contents before the call do not matter
 *   out  output i is [wh][ww] bytes, each 0 or 1, row-major, at out + i * out_stride_bytes; no alignment is assumed, and
 *        the bytes behind the window in its row of the slot are not written
 * Point d of an edge is t = flip ? steps - d : d, (major + t, (int)(minor + s * t + .5)) - a product rounded, then two
 * sums rounded, never an fma.  Where u changes between neighbours of the path, m = u[j] < u[j-1] ? u[j] : u[j] - 1 toggles
 * position cx * h + cy, cx = (m - 2) / 5, cy = clamp(floor((min(v[j], v[j-1]) + 2) / 5), 0, h), iff m >= 2, m % 5 == 2
 * and cx <= w - 1.  Pixel (y, x) of a part is set where an odd number of its positions are <= x * h + y.
 * The kernels are safe for ANY contents of the blob: every index they form lies inside the blob's tables, a part's
 * slice or a mask's window; edge contents give garbage bits at worst.  A part is out of range when its edges leave
 * [0, n_edges), points is outside 1..2^20, cap is no power of two within 1..8192, its slice leaves the scratch or a
 * size is outside 1..16384: it writes nothing and no mask reads it (nor one whose size differs from the mask's).  A mask
 * is out of range when a size is outside 1..16384, the window is empty or leaves the mask, wh > max_wh or ww > max_ww,
 * wh * ww > out_stride_bytes, n_parts < 1 or its parts leave [0, n_parts): its window is written as zeros where
 * wh >= 1, ww >= 1 and wh * ww <= out_stride_bytes, and not at all otherwise.
 * Negative counts, lengths or stride, max_wh / max_ww above 16384, scratch_len >= 2^31, a blob shorter than its three
 * tables, or n * ceil(max_ww / 256) >= 2^24 (the grid) is FGN_ERR_SHAPE; n == 0 or an empty maximum window FGN_OK with
 * no launch (pointers are not looked at); a null blob or out, or a null scratch with n_parts > 0, FGN_ERR_ARG.  No
 * allocation, no synchronisation, no environment variable. */
int fgn_poly_masks_u8(const int32_t* blob, long long blob_ints, int n, int n_parts, int n_edges, uint32_t* scratch,
                      long long scratch_len, unsigned char* out, long long out_stride_bytes, int max_wh, int max_ww,
                      void* stream);

/* Matching on the device: the exact pixel counts the evaluator needs from the masks, so that no RLE is decoded on the
 * host.  Step 1, bit planes of the ground-truth masks: masks [n][H][W] bytes (non-zero = set) -> bits, one 64-bit word
 * per 64 consecutive x of a row (bit b of word xw = pixel x = 64 xw + b; bits of x >= W are zero), laid out
 * [H][ceil(W/64)][n] (the words of all masks for one row segment are contiguous); area [n] = pixel count of each mask.
 * H*W < 2^31 (counts are int32).  n_masks == 0 launches nothing. */
int fgn_mask_bits_u64(const uint8_t* masks, uint64_t* bits, int32_t* area, int n_masks, int img_h, int img_w,
                      void* stream);

/* Step 2: inter [D][n_gt] = pixels set in both the pasted, thresholded mask of detection d and ground-truth mask g;
 * det_area [D] = pixels of the pasted mask.  prob / boxes / n_dev / thr / skip_empty as for fgn_mask_rle: the pasted bits
 * are those of fgn_mask_paste_u8, and the masks are never written.  gt_bits: from fgn_mask_bits_u64 for the same image
 * size.  Both outputs are fully written: rows at or beyond the device count are zero.  mask_size <= 32, H*W < 2^31.
 * n_det == 0 or n_gt == 0 launches nothing and leaves the outputs as they are. */
int fgn_mask_overlap_i32(const float* prob, const float* boxes, int box_stride, const uint64_t* gt_bits, int32_t* inter,
                         int32_t* det_area, const int32_t* n_dev, int n_det, int n_gt, int img_h, int img_w,
                         int mask_size, float thr, int skip_empty, void* stream);

/* Step 2 at source size: the boxes are network-frame boxes of a (net_h, net_w) network, divided by the scale of the
 * src_h x src_w image exactly as fgn_mask_rle_src divides them, and pasted into src_h x src_w, the size of gt_bits.
 * Sizes within 1..16384. */
int fgn_mask_overlap_src_i32(const float* prob, const float* boxes, int box_stride, const uint64_t* gt_bits,
                             int32_t* inter, int32_t* det_area, const int32_t* n_dev, int n_det, int n_gt, int src_h,
                             int src_w, int net_h, int net_w, int mask_size, float thr, int skip_empty, void* stream);

/* Step 3: the evaluator's greedy matching of one image (fgn_amd/fsiseg_eval.py: match_flags, bit for bit).  Per IoU type
 * and category 0..n_ways-1: the detections of the category in descending score order (ties in index order), cut at
 * max_dets; each in turn takes the still unmatched ground truth of its category with the largest IoU >= thr (among equal
 * IoUs the largest index).  boxes [n_det][box_stride >= 5] = x1, y1, x2, y2, score (no NaN scores); labels [n_det]
 * int64; n_dev (optional) the device-side detection count.  inter [n_det][n_gt] / det_area [n_det] / gt_area [n_gt]: the
 * counts of step 2 - segm IoU = inter / (|d| + |g| - inter) in float64, 0 where the union is 0; det_area == NULL = no
 * segm row is computed (inter and gt_area are then not read).  gt_xywh [n_gt][4] float64 = x, y, max(w,1), max(h,1) of
 * the ground-truth boxes, gt_cat [n_gt] int32 - bbox IoU as pycocotools' bbIou in float64, the detections' width and
 * height being float32 differences clamped to >= 1.  thr [n_thr] float64 on the device, each already min(thr, 1 - 1e-10).
 * src_h / src_w != 0: the boxes are network-frame boxes of a (net_h, net_w) network and are divided by the scale of the
 * src_h x src_w image exactly as fgn_mask_rle_src divides them (sizes within 1..16384); both 0: as given.
 * flags [2][n_det] int32, row 0 bbox, row 1 segm, fully written (row 1 is zero without det_area): bit t = matched at
 * thr[t]; -1 = beyond max_dets of its category; 0 = label outside 0..n_ways-1, or row at / beyond the device count.
 * n_thr in 1..16, n_ways >= 1, max_dets >= 1, counts >= 0, n_det <= 2048, min(n_det, max_dets) <= 1024, n_gt <= 4096, else
 * FGN_ERR_SHAPE.  n_det == 0 launches nothing.  n_gt == 0: 0 for every evaluated detection. */
int fgn_eval_match_i32(const float* boxes, int box_stride, const int64_t* labels, const int32_t* n_dev,
                       const int32_t* inter, const int32_t* det_area, const int32_t* gt_area, const double* gt_xywh,
                       const int32_t* gt_cat, const double* thr, int32_t* flags, int n_det, int n_gt, int n_thr,
                       int n_ways, int max_dets, int src_h, int src_w, int net_h, int net_w, void* stream);

/* ---- forward_train (fgn.py:125-185) ----------------------------------------------------- */

/* The proposal stage at training sizes (train_cfg.rpn_proposal, fgn_r50_c4_densecl.py:153-157: nms_pre 12000,
 * max_per_img 2000 - any nms_pre, max_per_img <= 4096): global bitonic sort of all anchor keys, then one workgroup
 * per image decodes the best nms_pre and runs the greedy NMS.  Same outputs as fgn_rpn_proposals_f32. */
size_t fgn_rpn_proposals_large_scratch_bytes(int batch, int n_total, int nms_pre);
int fgn_rpn_proposals_large_f32(const float* scores, const float* deltas, const float* base_anchors, void* scratch,
                                float* proposals, float* rois_out, int32_t* n_props, int batch, int feat_h, int feat_w,
                                int n_anchors, int stride, float img_h, float img_w, const float* host_means4,
                                const float* host_stds4, float max_ratio, int nms_pre, float min_bbox_size,
                                float iou_thr, int max_per_img, void* stream);

/* MaxIoUAssigner.assign (my_max_iou_assigner.py:60-213 on mmdet's bbox_overlaps): boxes [n, box_stride >= 4],
 * inside (optional) [n] bytes: 0 = not a candidate (anchor outside the image, my_anchor_head.py:233-239),
 * gts [k,4], k <= 256.  gt_inds [n] int32: -2 not a candidate, -1 ignored, 0 negative, i+1 = positive of GT i;
 * max_overlaps (optional) [n].  scratch: fgn_box_assign_scratch_bytes(n, k), uninitialised. */
size_t fgn_box_assign_scratch_bytes(int n, int k);
int fgn_box_assign_f32(const float* boxes, int box_stride, const uint8_t* inside, const float* gts, int n, int k,
                       float pos_iou_thr, float neg_iou_thr, float min_pos_iou, int match_low_quality, void* scratch,
                       int32_t* gt_inds, float* max_overlaps, void* stream);

/* DeltaXYWHBBoxCoder.encode (bbox_coder.encode at my_anchor_head.py:256, fgn_roi_head.py:141): [n,4] x [n,4] -> [n,4] */
int fgn_bbox2delta_f32(const float* proposals, const float* gts, float* out, int n, const float* host_means4,
                       const float* host_stds4, void* stream);

/* Weighted loss sums, out[0] = sum_i w_i * loss_i / avg_factor (mmdet weight_reduce_loss; w optional):
 * sigmoid CE (F.binary_cross_entropy_with_logits; y >= y_threshold is the target when y_threshold >= 0 - the mask
 * targets of mask_target_single), smooth L1, softmax CE (labels int64, outside [0, n_classes) ignored). */
int fgn_bce_logits_sum_f32(const float* x, const float* y, const float* w, long long n, float y_threshold,
                           double avg_factor, float* out, void* stream);
int fgn_smooth_l1_sum_f32(const float* pred, const float* target, const float* w, long long n, float beta,
                          double avg_factor, float* out, void* stream);
int fgn_softmax_ce_sum_f32(const float* logits, const int64_t* labels, const float* w, int n, int n_classes,
                           double avg_factor, float* out, void* stream);

/* BatchNorm2d in training mode (the shared head's BN layers during forward_train, fgn_roi_head.py:202-238) on
 * NHWC rows x [P,C]: batch mean / biased variance -> mean, var; y = (x-mean)/sqrt(var+eps)*gamma+beta (+residual)
 * (ReLU) -> out (may alias x); running_mean / running_var (optional) updated with `momentum` (unbiased variance). */
size_t fgn_bn_train_scratch_bytes(int C);
int fgn_bn_train_f32(const float* x, int P, int C, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, const float* residual, int relu, void* scratch,
                     float* mean, float* var, float* out, void* stream);

/* ---- backward of the trainable heads (the reference: torch.autograd under fgn.py:125-185) ---------------- */

/* d(sum_i w_i loss_i / avg_factor)/d(prediction) * scale for the three loss forms above (scale carries 1/avg_factor
 * and any upstream factor such as the 1/N balancer of fgn_ag_rpn_head.py:77-78) */
int fgn_bce_logits_grad_f32(const float* x, const float* y, const float* w, long long n, float y_threshold, float scale,
                            float* dx, void* stream);
int fgn_smooth_l1_grad_f32(const float* pred, const float* target, const float* w, long long n, float beta, float scale,
                           float* dpred, void* stream);
int fgn_softmax_ce_grad_f32(const float* logits, const int64_t* labels, const float* w, int n, int n_classes,
                            float scale, float* dlogits, void* stream);

/* ReLU backward: out = dy * [y > 0], y = the ReLU's output; n % 4 == 0 (mask convs, rpn_conv) */
int fgn_relu_backward_f32(const float* dy, const float* y, float* out, long long n, void* stream);

/* out[c] (+)= sum_r x[r][c]: bias gradients and reductions over RoIs; fp64 partials in a fixed order */
size_t fgn_colsum_scratch_bytes(int C);
int fgn_colsum_f32(const float* x, long long R, int C, void* scratch, float* out, int accumulate, void* stream);

/* BatchNorm2d(train) backward on NHWC rows [P,C]: g = dy * [y_post > 0] (y_post optional: the ReLU after the norm);
 * dx, dgamma, dbeta; g_out (optional) = g, the gradient of the identity branch of relu(bn3(conv3) + identity) */
size_t fgn_bn_train_backward_scratch_bytes(int C);
int fgn_bn_train_backward_f32(const float* x_pre, const float* y_post, const float* dy, const float* mean,
                              const float* var, const float* gamma, float eps, int P, int C, void* scratch, float* dx,
                              float* g_out, float* dgamma, float* dbeta, void* stream);

/* Backward of fgn_relation_gn_head_f32 (fc_cls|fc_reg -> avg-pool -> ReLU -> GroupNorm -> Q + S): d_out6 [R*N,6] =
 * (d cls_raw | d reg_raw); dQ [R,49,C]; dZ [R*N,49,C] (summed over the RoIs of an image it is dS); pooled [R*N,C]
 * (forward value, for the fc weight gradient); dgamma_part / dbeta_part [R,C] (column-summed by the caller) */
int fgn_relation_gn_head_backward_f32(const float* Q, const float* S, const float* rois, const float* gn_weight,
                                      const float* gn_bias, const float* fc_weight, const float* d_out6, float* dQ,
                                      float* dZ, float* pooled, float* dgamma_part, float* dbeta_part, int n_rois,
                                      int n_ways, int C, int gn_groups, int roi_size, float eps, void* stream);

/* Backward of fgn_mask_logits_f32 (ReLU(deconv) -> conv_logits): up [D,P*P,4,C], dlogit [D,2P,2P] ->
 * d_up (through the ReLU) and dw_part [D,C] (column-summed by the caller); roi_size > 0 and C > 0 */
int fgn_mask_logits_backward_f32(const float* up, const float* dlogit, const float* w, float* d_up, float* dw_part,
                                 int n_det, int roi_size, int C, void* stream);

/* im2col of a 3x3 / stride 1 / pad 1 input, NHWC: out [n*H*W, 9*C], column (ky*3+kx)*C + ci (weight gradients) */
int fgn_im2col3x3_f32(const float* x, float* out, int n, int H, int W, int C, void* stream);

/* Weight-gradient GEMM C [M,N] = A [R,M]^T . B [R,N] (A = dY, B = X or im2col(X); reduction over the rows) on fp32
 * MFMA; M % 4 == 0, N % 4 == 0; slabs of rows reduced in a fixed order.  workspace: fgn_gemm_tn_workspace_bytes() */
size_t fgn_gemm_tn_workspace_bytes(int R, int M, int N);
int fgn_gemm_tn_f32(const float* A, const float* B, float* C, int R, int M, int N, void* workspace, void* stream);

/* Products too narrow for the MFMA kernels (a dimension that is not a multiple of 4 / 32): C[M,N] = A[M,K] B[K,N]
 * (trans_a = 0) or A[K,M]^T B[K,N] (trans_a = 1), one thread per output element, reduction in index order.  Training
 * only: the 6-row fc weight / data gradients and the 75-channel AG-RPN head (torch.matmul in round 2). */
int fgn_gemm_small_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                       int trans_a, void* stream);

/* torch.optim.Adagrad step (fgn_train_schedule.py:5-13): g += wd*p; state += g*g; p -= lr*g/(sqrt(state)+eps) */
/* the same update for `count` parameter tensors (each with its own learning rate) in one launch; element-wise, so
 * bit-identical to `count` calls of fgn_adagrad_step_f32 (Trainer.step: ~40 tensors of the heads) */
int fgn_adagrad_multi_f32(float* const* params, const float* const* grads, float* const* state_sums, const long long* n,
                          const float* lr, int count, float weight_decay, float eps, void* stream);
int fgn_adagrad_step_f32(float* param, const float* grad, float* state_sum, long long n, float lr, float weight_decay,
                         float eps, void* stream);

/* Optimiser step for `count` parameter tensors in one launch per 64 non-empty tensors (csrc/optim.hip, compiled with
 * contraction off).  rule 0: Adagrad (state1 = sum); 1: Adam, L2 decay, no amsgrad (state1 = exp_avg, state2 = exp_avg_sq,
 * h0 / h1 = beta1 / beta2, bc1 / bc2 = 1 - beta^t formed by the caller in double); 2: SGD, dampening 0 (h0 = momentum,
 * state1 = momentum_buffer, may be null when h0 == 0; flags bit 0 = Nesterov).  g' = g * mul + weight_decay * p with
 * mul = (coef ? *coef * grad_scale : grad_scale); coef (device, nullable) is the clip coefficient of
 * fgn_grad_sqnorm_multi_f32; with coef null and grad_scale == 1 the gradient is used bit for bit. */
int fgn_optim_multi_f32(int rule, float* const* params, const float* const* grads, float* const* state1,
                        float* const* state2, const long long* n, const float* lr, int count, float weight_decay, float eps,
                        float h0, float h1, double bc1, double bc2, int flags, const float* coef, float grad_scale,
                        void* stream);

/* torch.nn.utils.clip_grad_norm_(max_norm, norm_type=2) without the host: out[0] = grad_scale x the L2 norm of all
 * gradients (the norm of the gradients scaled by the host scalar fgn_optim_multi_f32 takes),
 * out[1] = min(1, max_norm / (out[0] + 1e-6)).  Squares summed in fp64, one partial per 4096-element chunk in a fixed
 * order, the partials in a fixed second stage: no atomics, the same bits on every run.  partials: fp64 scratch of
 * partials_capacity >= sum ceil(n_i / 4096) entries.  Non-finite gradients give a NaN coefficient. */
int fgn_grad_sqnorm_multi_f32(const float* const* grads, const long long* n, int count, float max_norm, float grad_scale,
                              double* partials, long long partials_capacity, float* out, void* stream);

/* accs[i] = (first ? 0 : accs[i]) + a * grads[i] (gradient accumulation; `first` saves the zero fill) */
int fgn_grad_accumulate_multi_f32(float* const* accs, const float* const* grads, const long long* n, int count, float a,
                                  int first, void* stream);

/* ---- feature gradients: the gradient of the summed losses at the two C4 feature tensors ---------------------- */

/* Adjoint of fgn_roi_align_nhwc_f32 (both flavours; no post_shift, no ReLU): dy [R,P,P,C], rois [R,5] -> dx
 * [n_img,H,W,C]; accumulate = 0 overwrites dx (R = 0: zero fill), 1 adds onto it.  Same box transform, sampling grid,
 * sample coordinates and validity as the forward kernel (csrc/roi_geom.h).  Gather form, no atomics: every dx element
 * is owned by one thread, which adds its terms in (RoI index, bin row, bin column) order - the same bits on every
 * run.  RoIs of other images (batch index != the image), with an empty sampling grid or wholly outside the map
 * contribute nothing.  C % 4 == 0, 0 < out_size <= 32, n_img <= 65535, else FGN_ERR_SHAPE. */
int fgn_roi_align_backward_nhwc_f32(const float* dy, const float* rois, float* dx, int n_rois, int n_img, int H, int W,
                                    int C, int out_size, float spatial_scale, int sampling_ratio, int aligned,
                                    int accumulate, void* stream);

/* Backward of the AG-RPN guidance G[bN+n,y,x,c] = qry_fmap[b,y,x,c] * vec[bN+n,c] from the sparse gradient of rpn_conv's
 * input: T [rows,9,C] = the nine taps each active (pass, pixel) row sends to its 3x3 neighbourhood, and a CSR index
 * built on the host: pix [n_touched] flat pixels b*hw + y*w + x in ascending order, seg [n_touched*N + 1] the entry range
 * of every (touched pixel, pass), ent [nnz] = row*9 + tap, img_seg [B + 1] the touched-pixel range of every image.
 * d_qry [B,hw,C] (accumulate = 0: zero-filled first, untouched pixels stay zero; 1: added onto) receives
 * sum_n vec[bN+n,c] dG_n[c], dG_n = the taps of pass n in list order; slab [n_touched,N,C] (scratch) = qry_fmap dG_n;
 * d_vec [B*N,C] = the sum of slab over the image's touched pixels in ascending order.  No atomics.  The index is
 * trusted (the caller validates it on the host).  C % 4 == 0. */
int fgn_guidance_backward_f32(const float* T, const int32_t* pix, const int32_t* seg, const int32_t* ent,
                              const int32_t* img_seg, const float* qry_fmap, const float* vec, float* d_qry, float* slab,
                              float* d_vec, int n_touched, int B, int N, int hw, int C, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif

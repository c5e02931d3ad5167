/*
 * gtsfm_amd.h -- C ABI of libgtsfm_amd.so: the MI355X (gfx950) deep front-end of GTSfM.
 *
 * This is the drop-in boundary for ONE hot path of borglab/gtsfm: the SuperPoint detector/descriptor and the
 * SuperGlue / LightGlue matchers behind gtsfm/frontend's DetectorDescriptorBase / MatcherBase plugins. The reference
 * has no native code on this path (it calls ATen ops from Python); each entry point below names the reference
 * Python it replaces (paths relative to the reference repository root, abbreviated
 *   SP = thirdparty/SuperGluePretrainedNetwork/models/superpoint.py
 *   SG = thirdparty/SuperGluePretrainedNetwork/models/superglue.py
 *   LG = thirdparty/LightGlue/lightglue/lightglue.py (un-vendored submodule; call sites in
 *        gtsfm/frontend/matcher/lightglue_matcher.py:37-110)).
 *
 * Conventions
 *   - plain C: pointers and sizes only; no torch types. "_dev" pointers are device (HBM) addresses, e.g.
 *     torch.Tensor.data_ptr(); "_host" pointers are host addresses. `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success, a negative GTSFM_ERR_* code otherwise, and never throws across the ABI;
 *     gtsfm_last_error() returns a thread-local message for the last failure.
 *   - no hidden device allocations: callers pass workspaces sized by the *_workspace_bytes() queries.
 *   - no global mutable state besides the thread-local error string: any number of callers (one per GPU / process)
 *     may coexist. Kernels are enqueued on `stream` and are asynchronous with respect to the host.
 *   - activations are fp32, channels-last (NHWC for images, [tokens][channels] for keypoint sets).
 */
#ifndef GTSFM_AMD_H
#define GTSFM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTSFM_OK 0
#define GTSFM_ERR_INVALID -1
#define GTSFM_ERR_HIP -2
#define GTSFM_ERR_WORKSPACE -3

/* ABI version of this header; bumped on incompatible changes. */
int gtsfm_abi_version(void);
/* Thread-local description of the last error returned on this thread ("" if none). */
const char* gtsfm_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Generic fp32 dense ops (exact-fp32 MFMA). Exposed so that callers and parity tests can exercise each kernel
 * in isolation against the reference's ATen op.
 * ---------------------------------------------------------------------------------------------------------- */

/* Packed-weight sizes (floats) and host-side packers.
 * conv3x3: w_host is torch Conv2d layout [cout][cin][3][3], cin % 64 == 0.
 * linear : w_host is [n][k_real] row-major (nn.Linear / Conv1d(k=1)); k_pad = k_real rounded up to 8.
 * bias (if any) must be passed to the ops as a device array padded with zeros to a multiple of 64 entries. */
size_t gtsfm_packed_conv3x3_floats(int cin, int cout);
size_t gtsfm_packed_linear_floats(int k_pad, int n);
int gtsfm_pack_conv3x3(const float* w_host, int cin, int cout, float* packed_host);
int gtsfm_pack_linear(const float* w_host, int k_real, int k_pad, int n, float* packed_host);

/* y = [maxpool2x2](relu?(conv3x3(x) + bias)), stride 1, zero pad 1, NHWC.            replaces SP:148-161,190
 * in : [batch][h][w][in_stride], channels in_coff .. in_coff+cin-1
 * out: [batch][ho][wo][out_stride], channels out_coff .. out_coff+cout-1; (ho,wo) = (h,w) or (h/2,w/2) if pool */
int gtsfm_conv3x3_f32(const float* in_dev, int in_stride, int in_coff, float* out_dev, int out_stride, int out_coff,
                      const float* packed_w_dev, const float* bias_dev, int batch, int h, int w, int cin, int cout,
                      int relu, int pool, void* stream);

/* SuperPoint's first two layers as gtsfm_sp_forward runs them: y = [maxpool2x2] relu(conv1b(relu(conv1a(image)))), conv1a
 * recomputed inside conv1b's halo staging (its 64-channel output never reaches HBM).            replaces SP:148-150
 * image: [batch][h][w] uint8 (read as x / 255) or float32; w1a: [9 taps][64] (tap = 3 ky + kx), b1a: [64];
 * packed_w1b: gtsfm_pack_conv3x3(conv1b.weight, 64, 64); bias1b: [64]; out: [batch][ho][wo][64] */
int gtsfm_conv1_fused_f32(const void* image_dev, int image_is_u8, const float* w1a_dev, const float* b1a_dev,
                          const float* packed_w1b_dev, const float* bias1b_dev, int batch, int h, int w, int pool,
                          float* out_dev, void* stream);

/* C[:, c_coff:c_coff+n] = (res +) relu?(alpha * (A[:, :k] W^T + bias))              replaces SP:162,191, SG:49-60,
 * A: [m][lda]; C: [m][ldc]; res (optional): [m][ldres]; m_dev (optional): row count in device memory (<= m).
 * nn.Linear / Conv1d(kernel_size=1) / Conv2d(kernel_size=1).                                     98-119,254 */
int gtsfm_linear_f32(const float* a_dev, int lda, int m, const int32_t* m_dev, int k, const float* packed_w_dev,
                     const float* bias_dev, int n, float* c_dev, int ldc, int c_coff, const float* res_dev, int ldres,
                     float alpha, int relu, void* stream);

/* Same operation with the weights (or a second activation matrix) given row-major, W[n][ldw] as nn.Linear stores them:
 * both operands then travel by LDS-DMA (k % 32 == 0 and ldw % 4 == 0 required). n_dev (optional): column count in
 * device memory (<= n).                                                        same reference lines as gtsfm_linear_f32
 * Environment (read per launch): GTSFM_GEMM_MATH=bf16x3 runs the product (either tiling) in the opt-in arithmetic of
 * gtsfm_attention_math_f32 (operands split exactly into three bf16 pieces, six bf16 MFMA products per block, fp32 accumulation:
 * fp32-class error, NOT the default's bits); GTSFM_GEMM_MATH=f16x2 runs it in the second opt-in arithmetic (two fp16 pieces per operand,
 * three fp16 MFMA products per block; operands beyond +-65504 give NaN); the default is exact fp32 and every parity statement is made
 * with it. */
int gtsfm_linear_rowmajor_f32(const float* a_dev, int lda, int m, const int32_t* m_dev, int k, const float* w_dev, int ldw,
                              const float* bias_dev, int n, const int32_t* n_dev, float* c_dev, int ldc, int c_coff,
                              const float* res_dev, int ldres, float alpha, int relu, void* stream);

/* Pack a device activation matrix B[n][k] (row stride ldb) as the "weight" operand of gtsfm_linear_f32, so that
 * A B^T products of two activation matrices (score matrices, SG:257) use the same kernel. */
int gtsfm_pack_rows_f32(const float* b_dev, int ldb, int n, const int32_t* n_dev, int k, float* packed_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SuperPoint
 * ---------------------------------------------------------------------------------------------------------- */

/* Number of floats of the packed SuperPoint weight blob, and the packer. `tensors_host` are the 24 state_dict
 * tensors in checkpoint order: conv1a.weight, conv1a.bias, conv1b.weight, ..., convDb.weight, convDb.bias
 * (SP:119-134; torch layouts). */
size_t gtsfm_sp_packed_weight_floats(void);
int gtsfm_sp_pack_weights(const float* const* tensors_host, float* packed_host);

/* Bytes of device workspace gtsfm_sp_forward needs for `batch` images of height x width. */
size_t gtsfm_sp_workspace_bytes(int batch, int height, int width);

/* SuperPoint.forward for a batch of equally-sized gray images.                              replaces SP:145-202
 * image_dev       : [batch][height][width], fp32 in [0,1] (image_is_u8 = 0) or uint8 (image_is_u8 = 1; converted as
 *                   astype(float32) / 255.0 like gtsfm/frontend/detector_descriptor/superpoint.py:73-75)
 * capacity        : rows available per image in the output arrays; keypoints beyond it are dropped (row-major
 *                   order), kp_count_raw_dev still reports the true count
 * kp_count_dev    : [batch] int32, min(count, capacity)
 * kp_count_raw_dev: [batch] int32, true keypoint count (may be NULL)
 * kp_xy_dev       : [batch][capacity][2] fp32 (x, y) pixel coordinates, row-major (y, x) detection order = the order
 *                   of torch.nonzero (SP:170-173,187)
 * kp_score_dev    : [batch][capacity] fp32
 * desc_dev        : [batch][capacity][256] fp32, row i <-> keypoint i (the transposed layout the wrapper builds at
 *                   gtsfm/frontend/detector_descriptor/superpoint.py:84)
 * top_k           : <= 0 returns every keypoint (what SP returns with max_keypoints = -1, as GTSfM runs it). > 0 (then
 *                   capacity must equal top_k) keeps the top_k responses on the device, in detection order, and
 *                   describes only those -- the selection gtsfm/common/keypoints.py:89-110 (get_top_k) makes on
 *                   the host; used by the GPU-resident detect+match pipeline.
 * Optional taps for parity tests (NULL to skip): dense_scores_dev [batch][8*(h/8)][8*(w/8)] (pre-NMS, SP:163-166),
 * nms_scores_dev same shape (SP:167). */
int gtsfm_sp_forward(const float* packed_weights_dev, const void* image_dev, int image_is_u8, int batch, int height,
                     int width, float keypoint_threshold, int nms_radius, int remove_borders, int capacity, int top_k,
                     void* workspace_dev, size_t workspace_bytes, int32_t* kp_count_dev, int32_t* kp_count_raw_dev,
                     float* kp_xy_dev, float* kp_score_dev, float* desc_dev, float* dense_scores_dev,
                     float* nms_scores_dev, void* stream);

/* The same with the image masks GTSfM attaches to images (gtsfm/common/image.py `mask`): valid_mask_dev [batch][height][width]
 * uint8, 1 = valid (NULL = no mask). A keypoint at pixel (x, y) is kept iff valid_mask[y][x] == 1 -- Keypoints.filter_by_mask,
 * gtsfm/common/keypoints.py:112-127 -- applied BEFORE the top-k, as gtsfm/frontend/detector_descriptor/superpoint.py:76-91
 * orders them. (With a mask the nms_scores_dev tap shows the masked scores; keypoint_threshold must be positive.) */
int gtsfm_sp_forward_masked(const float* packed_weights_dev, const void* image_dev, int image_is_u8, int batch, int height,
                            int width, float keypoint_threshold, int nms_radius, int remove_borders, int capacity, int top_k,
                            void* workspace_dev, size_t workspace_bytes, int32_t* kp_count_dev, int32_t* kp_count_raw_dev,
                            float* kp_xy_dev, float* kp_score_dev, float* desc_dev, float* dense_scores_dev,
                            float* nms_scores_dev, const uint8_t* valid_mask_dev, void* stream);

/* The individual SuperPoint stages (same kernels gtsfm_sp_forward launches), for stage-wise parity tests. */

/* softmax over 65 logits per cell, drop dustbin, depth-to-space 8x8.                           replaces SP:163-166
 * logits: [batch][hc][wc][ld] (ld >= 65); scores: [batch][8*hc][8*wc] */
int gtsfm_sp_softmax_d2s(const float* logits_dev, int ld, int batch, int hc, int wc, float* scores_dev, void* stream);
/* simple_nms. scratch: 2*n bytes + n floats where n = batch*h*w (gtsfm_sp_nms_scratch_bytes).    replaces SP:47-62 */
size_t gtsfm_sp_nms_scratch_bytes(int batch, int h, int w);
int gtsfm_sp_simple_nms(const float* scores_dev, int batch, int h, int w, int radius, void* scratch_dev, float* out_dev,
                        void* stream);
/* nonzero(score > thr) + remove_borders + flip. scratch: 2*batch*h int32.            replaces SP:170-178,187 */
int gtsfm_sp_extract_keypoints(const float* nms_dev, int batch, int h, int w, float threshold, int border, int capacity,
                               int32_t* scratch_dev, int32_t* kp_count_dev, int32_t* kp_count_raw_dev, float* kp_xy_dev,
                               float* kp_score_dev, void* stream);
/* Top-k by response, survivors in detection order (host analogue: Keypoints.get_top_k,   gtsfm/common/keypoints.py:89-110).
 * in: kp_score [batch][capacity], kp_xy [batch][capacity][2], kp_count [batch]; out arrays have top_k rows per image. */
int gtsfm_sp_select_topk(const float* kp_score_dev, const float* kp_xy_dev, const int32_t* kp_count_dev, int batch,
                         int capacity, int top_k, float* out_xy_dev, float* out_score_dev, int32_t* out_count_dev,
                         void* stream);
/* L2-normalise dense descriptors, bilinear sample (align_corners=True), L2-normalise.   replaces SP:80-92,192-196
 * dense: [batch][hc*wc][ld] raw convDb output (256 channels). */
int gtsfm_sp_sample_descriptors(const float* dense_dev, int ld, int batch, int hc, int wc, const float* kp_xy_dev,
                                const int32_t* kp_count_dev, int capacity, float* desc_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Matchers (SuperGlue / LightGlue): ragged batches of image pairs, token-major activations
 * ---------------------------------------------------------------------------------------------------------- */

/* Weight blobs. A blob is a sequence of 64-float-aligned entries: kind 0 = linear (W [n][k] row-major + optional
 * bias [n], stored packed for gtsfm_linear_f32), kind 1 = raw vector of n floats. The entry sequences of the two
 * matchers are documented in gtsfm_amd/runtime/matcher_engine.py (BatchNorm folded, attention heads made
 * contiguous); the forward passes walk the same sequence. */
size_t gtsfm_blob_floats(int count, const int32_t* kinds, const int32_t* n, const int32_t* k);
int gtsfm_pack_blob(int count, const int32_t* kinds, const int32_t* n, const int32_t* k, const float* const* w_host,
                    const float* const* b_host, float* packed_host);

/* Batch descriptors. A batch is `npairs` image pairs; pair p has n0[p] / n1[p] keypoints (all > 0; n1[p] == 0 is accepted for
 * the per-image phase 1 of gtsfm_{sg,lg}_forward_phase only: an odd number of images leaves the last second slot empty) and image shapes
 * hw[p] = {H0, W0, H1, W1}. Token-major inputs concatenate the keypoint sets in the order pair0/img0, pair0/img1,
 * pair1/img0, ... (T = sum of all counts rows). The int32 descriptor block (counts, per-set row offsets / image
 * shapes, per-pair score-matrix offsets, attention problem lists) is built on the host and uploaded by the caller;
 * LightGlue's point pruning rewrites the counts section on the device. */
size_t gtsfm_match_desc_ints(int superglue, int npairs, const int32_t* n0_host, const int32_t* n1_host);
int gtsfm_match_build_desc(int superglue, int npairs, const int32_t* n0_host, const int32_t* n1_host,
                           const int32_t* hw_host, int32_t* desc_host);

/* Block moves inside device memory: dst block b <- src block src_index[b] (src_index_dev == NULL: b), written at dst block
 * dst_index[b] (dst_index_dev == NULL: b); a block is block_floats contiguous floats (even).    replaces the per-pair numpy -> torch
 * marshalling of gtsfm/frontend/matcher/{superglue,lightglue}_matcher.py:75-102 in the batched pipeline: the keypoint sets of a
 * pair chunk are gathered from the resident feature table [images][max_keypoints][2 | 1 | 256] by image index. */
int gtsfm_move_blocks_f32(const float* src_dev, const int32_t* src_index_dev, float* dst_dev, const int32_t* dst_index_dev,
                          int nblocks, int64_t block_floats, void* stream);

/* out = softmax(scale * q k^T) v per head (head h = columns [64h, 64h+64)).          replaces SG:85-89,98-106
 * problems_dev: [nproblems][4] int32 {q_row_off, q_count_idx, k_row_off, k_count_idx}; counts_dev: int32 array the
 * *_count_idx fields index; max_q: upper bound of the query counts (grid sizing). */
int gtsfm_attention_f32(const float* q_dev, int ldq, const float* k_dev, int ldk, const float* v_dev, int ldv,
                        float* out_dev, int ldo, const int32_t* problems_dev, const int32_t* counts_dev, int nproblems,
                        int max_q, int heads, float scale, void* stream);
/* The same attention with its two SCHEDULES selectable (results are bit-identical): mode -1 = fused (one workgroup walks all keys of
 * its 128 queries; what gtsfm_attention_f32 runs), 1 = split (one workgroup per query tile and 1024-key segment writes an
 * unnormalised partial (O, m, l) to the workspace, a second kernel merges the segments in ascending order -- fills the chip for a
 * single pair, the per-call plugin API), 0 = chosen from the launch geometry as the matchers do. max_k: upper bound of the key
 * counts (0: unknown); rows: rows of the q / out arrays; workspace_dev: gtsfm_attention_split_workspace_bytes(...) bytes -- the
 * split schedule's partial states or, for the fused schedule, parking space for the merged state between key segments (NULL with
 * mode -1: parked in LDS, one workgroup per CU instead of two). */
size_t gtsfm_attention_split_workspace_bytes(int nproblems, int max_q, int max_k, int heads, size_t rows);
int gtsfm_attention_split_f32(const float* q_dev, int ldq, const float* k_dev, int ldk, const float* v_dev, int ldv,
                              float* out_dev, int ldo, const int32_t* problems_dev, const int32_t* counts_dev, int nproblems,
                              int max_q, int max_k, int heads, float scale, int mode, size_t rows, void* workspace_dev,
                              size_t workspace_bytes, void* stream);
/* The same attention with its ARITHMETIC selectable as well. math 0 = exact fp32 (v_mfma_f32_32x32x2_f32, bit-for-bit an fmaf chain:
 * the default everywhere and the arithmetic every parity statement of this package is made with). math 1 = "bf16x3": both products
 * (K Q^T and P V) on v_mfma_f32_32x32x16_bf16 with each fp32 operand split EXACTLY into three bf16 pieces (8 + 8 + 8 significand
 * bits) and six of the nine piece products executed, fp32 accumulation -- fp32-class error per product term (the dropped terms are
 * ~2^-24 of it, below 2^-21 in the worst case), NOT the same bits as math 0, 3/8 of its matrix-pipe time. Opt-in: the matchers take it from the environment
 * variable GTSFM_ATTENTION_MATH=bf16x3 (read per call). math 2 = "f16x2" (GTSFM_ATTENTION_MATH=f16x2): each operand carried as TWO fp16
 * pieces (hi = RN16(x), lo = RN16(x - hi)) and three products (lo hi, hi lo, hi hi) on v_mfma_f32_32x32x16_f16, fp32 accumulation --
 * per product term < 2^-20.9 |x y| worst case, 2^-24 on average (the class of math 1), 3/16 of math 0's matrix-pipe time; fp16 has no
 * exponent headroom: the softmax weights are kept <= 2^15 by the kernel itself, and a q / k / v value beyond +-65504 gives NaN output rows
 * (never a clamped value). max_k must be given (> 0) for math 1 and 2; the workspace additionally holds the split K / V tiles
 * (6 resp. 4 x heads x nproblems x ceil(max_k / 64) x 8 KiB). */
size_t gtsfm_attention_math_workspace_bytes(int nproblems, int max_q, int max_k, int heads, size_t rows, int math);
int gtsfm_attention_math_f32(const float* q_dev, int ldq, const float* k_dev, int ldk, const float* v_dev, int ldv,
                             float* out_dev, int ldo, const int32_t* problems_dev, const int32_t* counts_dev, int nproblems,
                             int max_q, int max_k, int heads, float scale, int mode, int math, size_t rows, void* workspace_dev,
                             size_t workspace_bytes, void* stream);

/* ---- input step in front of SuperPoint (uint8, OpenCV's 8-bit fixed-point arithmetic) ----
 * RGB(A) -> gray.          replaces gtsfm/utils/images.py:15-42 (cv.cvtColor COLOR_RGB2GRAY / COLOR_RGBA2GRAY), called from
 * gtsfm/frontend/detector_descriptor/superpoint.py:73. rgb_dev [H][W][channels], gray_dev [H][W]. */
int gtsfm_prep_rgb_to_gray_u8(const uint8_t* rgb_dev, int height, int width, int channels, uint8_t* gray_dev, void* stream);
/* INTER_CUBIC resize.      replaces gtsfm/utils/images.py:102-129 (cv.resize), called from gtsfm/loader/loader_base.py:160-200.
 * gtsfm_prep_cubic_taps (host): per destination index the source index of the second of the four taps and the four 11-bit
 * integer weights (float32 cubic weights, A = -0.75, rounded half to even); the caller uploads the tables of both axes.
 * src_dev [src_h][src_w][channels] -> dst_dev [dst_h][dst_w][channels], taps clamped to the image. */
int gtsfm_prep_cubic_taps(int dst_size, int src_size, int32_t* first_src_host, int16_t* weights_host);
int gtsfm_prep_resize_cubic_u8(const uint8_t* src_dev, int src_h, int src_w, int channels, const int32_t* xofs_dev, const int16_t* xw_dev,
                               const int32_t* yofs_dev, const int16_t* yw_dev, uint8_t* dst_dev, int dst_h, int dst_w, void* stream);

/* SuperGlue.forward for a batch of pairs.                                                    replaces SG:228-283
 * kpts_dev [T][2] (x, y) pixels, scores_dev [T], descriptors_dev [T][256] (the wrapper's (N, 256) layout,
 * gtsfm/frontend/matcher/superglue_matcher.py:94-99 without the transposes).
 * matches_dev [T] int32: for a keypoint of image i1 the matched index in image i2 (matches0), for a keypoint of
 * image i2 the matched index in image i1 (matches1), -1 if unmatched; mscores_dev [T]: matching_scores0/1.
 * ot_dev (optional, parity tests): final log optimal-transport matrices, pair p at the offset / row stride of the
 * descriptor block ((n0+1) x (n1+1), SG:263). Pairs with an empty keypoint set must be handled by the caller
 * (SG:233-240). */
size_t gtsfm_sg_workspace_bytes(int npairs, const int32_t* n0_host, const int32_t* n1_host);
int gtsfm_sg_forward(const float* blob_dev, int num_layers, float bin_score, int npairs, const int32_t* n0_host,
                     const int32_t* n1_host, const int32_t* desc_dev, const float* kpts_dev, const float* scores_dev,
                     const float* descriptors_dev, int sinkhorn_iters, float match_threshold, void* workspace_dev,
                     size_t workspace_bytes, int32_t* matches_dev, float* mscores_dev, float* ot_dev, void* stream);

/* Log-space Sinkhorn iterations on their own (parity tests, roofline measurement).        replaces SG:141-147,150-170
 * z_dev: couplings matrices back to back, pair p is (m[p]+1) x (n[p]+1) with row stride ld = (n[p]+1 rounded up to 4); the
 * inner m x n block holds the scores, the dustbin row / column are filled with bin_score here (SG:156-160). After `iters`
 * iterations u_dev [npairs][max(m)+1] and v_dev [npairs][max(n)+1] hold SG:143-146's u and v (Z + u + v - norm is the
 * log optimal-transport matrix). Builds and uploads its own batch descriptor: synchronises `stream` once. */
size_t gtsfm_sinkhorn_workspace_bytes(int npairs, const int32_t* m_host, const int32_t* n_host);
int gtsfm_sinkhorn_f32(float* z_dev, int npairs, const int32_t* m_host, const int32_t* n_host, float bin_score, int iters,
                       void* workspace_dev, size_t workspace_bytes, float* u_dev, float* v_dev, void* stream);

/* The score matrices of a batch of pairs in ONE ragged launch of the LDS-DMA GEMM, as gtsfm_sg_forward issues them (SG:257-258:
 * scores = einsum('bdn,bdm->bnm', mdesc0, mdesc1) / 256^.5): pair p's image-0 descriptor rows times its image-1 rows, image 1's rows
 * standing in for the weights as they lie (no packing pass). mdesc_dev: [sum(m) + sum(n)][256], pair p's m[p] image-0 rows followed by
 * its n[p] image-1 rows, pairs back to back. z_dev: couplings matrices in gtsfm_sinkhorn_f32's layout (pair p: (m[p]+1) rows of stride
 * ld = (n[p]+1 rounded up to 4)); only the inner m x n block is written: alpha * <mdesc0[i], mdesc1[j]>. Parity tests of the batched
 * product against per-pair matmuls; bench.py's roofline of the launch. Builds and uploads its own batch descriptor: synchronises
 * `stream` once. */
size_t gtsfm_score_matrices_workspace_bytes(int npairs);
int gtsfm_score_matrices_f32(const float* mdesc_dev, int npairs, const int32_t* m_host, const int32_t* n_host, float alpha, float* z_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same, split at the point where a pair's two images first see each other (for callers that match one image against
 * many: the per-image part runs once per image instead of once per pair; results are bit-identical to gtsfm_sg_forward).
 * phase 1: keypoint encoder + the first (self) GNN layer of every keypoint set of the batch (superglue.py:243-248, first
 * iteration of :126-137) -> x_out_dev [T][256] in the input's row order; matches / scores outputs unused (may be NULL);
 * the keypoint sets are independent here, so an odd number of images is passed with n1 = 0 in the last slot.
 * phase 2: descriptors_dev holds that x; kpts_dev / scores_dev unused; the rest of the forward. phase 0 = gtsfm_sg_forward. */
int gtsfm_sg_forward_phase(const float* blob_dev, int num_layers, float bin_score, int npairs, const int32_t* n0_host,
                           const int32_t* n1_host, const int32_t* desc_dev, const float* kpts_dev, const float* scores_dev,
                           const float* descriptors_dev, int sinkhorn_iterations, float match_threshold, void* workspace_dev,
                           size_t workspace_bytes, int32_t* matches_dev, float* mscores_dev, float* ot_dev, int phase, float* x_out_dev,
                           void* stream);

/* LightGlue(features="superpoint").forward for a batch of pairs.          replaces LG (upstream LightGlue._forward;
 * reference call site gtsfm/frontend/matcher/lightglue_matcher.py:88-110). PARITY UNPINNED: the reference does not
 * vendor LightGlue's source; this follows the published upstream algorithm (see oracle/lightglue_oracle.py).
 * kpts_dev [T][2], descriptors_dev [T][256] as above. match_bias_host [num_layers] / conf_bias_host [num_layers-1]:
 * the scalar biases of the matchability / token-confidence heads. desc_dev is READ-WRITE (live counts, stop layers).
 * depth_confidence <= 0 disables early stopping; pruning_threshold = INT32_MAX disables point pruning (upstream:
 * -1 on CPU = always prune, 1024 / 1536 on CUDA without / with flash attention).
 * matches_dev [T] int32 / mscores_dev [T] as for SuperGlue (indices refer to the ORIGINAL keypoint order).
 * sim_dev (optional, parity tests): raw similarity matrices over the kept keypoints. After the call the descriptor
 * block holds the per-pair stop layer and the final (kept) keypoint counts. */
size_t gtsfm_lg_workspace_bytes(int npairs, const int32_t* n0_host, const int32_t* n1_host);
int gtsfm_lg_forward(const float* blob_dev, int num_layers, const float* match_bias_host, const float* conf_bias_host,
                     int npairs, const int32_t* n0_host, const int32_t* n1_host, int32_t* desc_dev,
                     const float* kpts_dev, const float* descriptors_dev, float depth_confidence,
                     float width_confidence, float filter_threshold, int pruning_threshold, void* workspace_dev,
                     size_t workspace_bytes, int32_t* matches_dev, float* mscores_dev, float* sim_dev, void* stream);

/* gtsfm_lg_forward_phase with ONE pair's launch sequence split over two streams (round 5; the per-call plugin path, where a caller
 * hands over one pair at a time as gtsfm/frontend/matcher/lightglue_matcher.py:75-112 does): everything LightGlue computes per image is
 * enqueued per keypoint set -- image 0's on `stream`, image 1's on `side_stream` -- with event waits where a set needs the other's keys /
 * values and once per layer for the pair-level part; all work is joined back into `stream` before the call returns (the caller
 * synchronises `stream` only). Bit-identical to the one-stream form. Taken for npairs == 1, phase 0 / 2, exact-fp32 attention; in every
 * other case (and with side_stream == NULL) it IS gtsfm_lg_forward_phase. */
int gtsfm_lg_forward_streams(const float* blob_dev, int num_layers, const float* match_bias_host, const float* conf_bias_host,
                             int npairs, const int32_t* n0_host, const int32_t* n1_host, int32_t* desc_dev,
                             const float* kpts_dev, const float* descriptors_dev, float depth_confidence,
                             float width_confidence, float filter_threshold, int pruning_threshold, void* workspace_dev,
                             size_t workspace_bytes, int32_t* matches_dev, float* mscores_dev, float* sim_dev, int phase,
                             float* x_out_dev, void* stream, void* side_stream);

/* LightGlue's assignment stage alone, on given similarity matrices (parity tests; bench.py's rooflines of the sweep kernels the forward
 * launches).                                  replaces upstream sigmoid_log_double_softmax + filter_matches (call site
 *                                             gtsfm/frontend/matcher/lightglue_matcher.py:104-110)
 * sim_dev    : pair p's m[p] x n[p] similarities at float offset sum_{q<p} m[q] * ld[q], row stride ld[p] = n[p] rounded up to 4
 * zlogit_dev : matchability logits, token-major with every keypoint set aligned to 128 rows (pair0/img0, pair0/img1, pair1/img0, ...:
 *              set s starts at row sum of the previous sets' counts each rounded up to 128); matches_dev / mscores_dev: same layout,
 *              match index within the other set or -1, exp(score) as upstream's matching_scores
 * stages     : 1 = the two log-softmax sweeps (row / column log-sum-exp into the workspace), 2 = mutual arg-max extraction + filter
 *              (needs the workspace of a call with 1 on the same inputs), 3 = both. Builds and uploads its own batch descriptor:
 *              synchronises `stream` once -- unless 4 is added: the workspace then still holds the descriptor of an earlier call with
 *              the same shapes (timing loops: launches only). */
size_t gtsfm_lg_assignment_workspace_bytes(int npairs, const int32_t* m_host, const int32_t* n_host);
int gtsfm_lg_assignment_f32(const float* sim_dev, int npairs, const int32_t* m_host, const int32_t* n_host, const float* zlogit_dev,
                            float filter_threshold, int stages, void* workspace_dev, size_t workspace_bytes, int32_t* matches_dev,
                            float* mscores_dev, void* stream);

/* x = gelu(layer_norm(x) * gamma + beta) in place over rows of 512 columns (row stride ld >= 512): the FFN's normalisation /
 * activation of a LightGlue block (upstream nn.LayerNorm(512) + nn.GELU between ffn.0 and ffn.3), stand-alone for parity tests and
 * bench.py's roofline. scratch_dev: 64 bytes of device memory; synchronises `stream` once. */
int gtsfm_layernorm_gelu_f32(float* x_dev, int ld, int rows, const float* gamma_dev, const float* beta_dev, void* scratch_dev, void* stream);

/* LightGlue split the same way: phase 1 = the first layer's SELF block (rotary self-attention + FFN of one image) -> x_out_dev;
 * phase 2 = descriptors_dev holds that x, the first self block is skipped. Bit-identical to gtsfm_lg_forward (phase 0). */
int gtsfm_lg_forward_phase(const float* blob_dev, int num_layers, const float* match_bias_host, const float* conf_bias_host,
                           int npairs, const int32_t* n0_host, const int32_t* n1_host, int32_t* desc_dev, const float* kpts_dev,
                           const float* descriptors_dev, float depth_confidence, float width_confidence, float filter_threshold,
                           int pruning_threshold, void* workspace_dev, size_t workspace_bytes, int32_t* matches_dev,
                           float* mscores_dev, float* sim_dev, int phase, float* x_out_dev, void* stream);

/* ---- verifier stage behind the matcher (float64) ----
 * OpencvVerifierBase.verify with use_intrinsics_in_verification=True for a batch of pairs.
 *                                  replaces gtsfm/frontend/verifier/opencv_verifier_base.py:47-111 + ransac.py:52-84
 *                                  (cv2.findEssentialMat) + gtsfm/utils/verification.py:54-96 (cv.recoverPose),
 *                                  called from gtsfm/two_view_estimator.py:391-397.
 * PARITY UNPINNED (OpenCV absent, its sampler not reproducible): Nister's five-point solver, squared Sampson error
 * (gtsfm/utils/verification.py:172-220), RANSAC with a counter-based sampler (splitmix64 of seed / hypothesis / attempt),
 * 256 hypotheses per round scored by MSAC, at most 4 rounds, stop when (1 - w^5)^n <= 1e-6, then one round of 256 samples
 * drawn from the winner's inliers (LO-RANSAC inner sampling), cheirality choice, and six Gauss-Newton steps on the inliers'
 * Sampson error over the pose (kept when the MSAC cost drops); see oracle/verifier_oracle.py.
 * kp_xy_dev [*][2] float32 pixel coordinates of all keypoint tables; pair p uses the tables starting at rows kp_off1_dev[p]
 * (image i1) and kp_off2_dev[p] (image i2). match_idx_dev [total_matches][2] int32 (row in i1's table, row in i2's table),
 * pair p owning rows match_off_dev[p] .. match_off_dev[p+1], or only the first match_count_dev[p] of them when match_count_dev
 * is given (capacity layout, filled by gtsfm_verify_compact_matches; total_matches = match_off_dev[num_pairs]). intrinsics_dev [num_pairs][8] = fx, fy, cx, cy of i1 then i2
 * (pinhole; lens distortion is the caller's to remove). threshold_px is divided by max(fx1, fx2) as the reference does.
 * Outputs per pair: essential_dev [9] i2Ei1 (unnormalised), rotation_dev [9] i2Ri1 row-major, translation_dev [3] unit i2Ui1,
 * inlier_mask_dev [total_matches] (1 = verified), stats_dev [8] int32 = inliers, hypotheses drawn, winning hypothesis,
 * winning root, cheirality counts of (R1,t) (R2,t) (R1,-t) (R2,-t). Pairs with fewer than 6 matches or no model: inliers = 0,
 * NaN matrices (the reference's failure tuple is built by the caller). */
size_t gtsfm_verify_workspace_bytes(long long total_matches);
int gtsfm_verify_essential_f64(const float* kp_xy_dev, const long long* kp_off1_dev, const long long* kp_off2_dev,
                               const int32_t* match_idx_dev, const long long* match_off_dev, const int32_t* match_count_dev,
                               long long total_matches, const double* intrinsics_dev, const unsigned long long* seeds_dev, double threshold_px,
                               int num_pairs, void* workspace_dev, size_t workspace_bytes, double* essential_dev,
                               double* rotation_dev, double* translation_dev, uint8_t* inlier_mask_dev, int32_t* stats_dev,
                               void* stream);

/* The same with use_intrinsics_in_verification=False: fundamental matrix from pixel coordinates, then E = K2^T F K1.
 *                                  replaces opencv_verifier_base.py:91-97 + ransac.py:86-112 (cv2.findFundamentalMat(FM_RANSAC),
 *                                  seven-point samples) + gtsfm/utils/verification.py:99-112 (fundamental_to_essential_matrix).
 * Residual = OpenCV's for this estimator, the larger squared point-to-epipolar-line distance, against threshold_px^2 (not
 * divided by a focal length); minimal sample 7, at least 8 matches (NUM_MATCHES_REQ_F_MATRIX). fundamental_dev [9] = i2Fi1;
 * essential_dev [9] = K2^T F K1; pose and cheirality on the normalised coordinates as above. PARITY UNPINNED as above. */
int gtsfm_verify_fundamental_f64(const float* kp_xy_dev, const long long* kp_off1_dev, const long long* kp_off2_dev,
                                 const int32_t* match_idx_dev, const long long* match_off_dev, const int32_t* match_count_dev,
                                 long long total_matches, const double* intrinsics_dev, const unsigned long long* seeds_dev,
                                 double threshold_px, int num_pairs, void* workspace_dev, size_t workspace_bytes, double* fundamental_dev,
                                 double* essential_dev, double* rotation_dev, double* translation_dev, uint8_t* inlier_mask_dev,
                                 int32_t* stats_dev, void* stream);

/* Matcher output -> the verifier's match lists on the device.   replaces the host marshalling of
 * gtsfm/frontend/matcher/superglue_matcher.py:100-102 / lightglue_matcher.py:104-110 ((K, 2) arrays per pair) between the
 * matcher and the verifier. matches_dev: gtsfm_sg_forward / gtsfm_lg_forward output; pair p's matches0 block starts at row
 * row_off_dev[p] and has n0_dev[p] rows. Writes the (row, matches0[row]) pairs with matches0[row] > -1, in row order, at
 * match_idx_dev + 2 * match_off_dev[p] (capacity n0_dev[p]) and their number to match_count_dev[p]. */
int gtsfm_verify_compact_matches(const int32_t* matches_dev, const long long* row_off_dev, const int32_t* n0_dev,
                                 const long long* match_off_dev, int num_pairs, int32_t* match_idx_dev, int32_t* match_count_dev,
                                 void* stream);

/* ---- TwoWayMatcher: brute-force mutual nearest neighbour with an optional ratio test ----
 *                                  replaces gtsfm/frontend/matcher/twoway_matcher.py:40-147 (cv.BFMatcher match / knnMatch(k=2),
 *                                  run 1->2 and 2->1, then the mutual check).
 * desc_dev: one descriptor table, row r at desc_dev + r * row_stride elements; float32 (desc_is_u8 = 0) or uint8 (1).
 * metric: 1 = HAMMING (popcount of a XOR b over the bytes; uint8 only), 2 = EUCLIDEAN (sqrtf of the sum of squares).
 * pairs_host [npairs][4] int32 = (first row of side 1, n1, first row of side 2, n2); n1, n2 >= 1; rows 0 .. max(first + n) - 1
 * of the table must be readable. Side 1 row i's nearest side-2 row j (ties -> lower j) is kept iff, with use_ratio,
 * (double)d1st <= ratio * (double)d2nd (second entry of the top-2, duplicates counted), and side 2 row j's nearest side-1 row,
 * under the same test, is i. Outputs, pair p's block starting at the sum of the n1 of the pairs before it:
 * matches0_dev [sum n1] int32 = j or -1; dist0_dev [sum n1] float32 = the distance of row i to its nearest side-2 row.
 * The product is computed once per pair in exact fp32 (v_mfma_f32_32x32x2_f32) and never stored; integer descriptors with
 * max|a|^2 + max|b|^2 < 2^24 give the reference's distances bit for bit. At most 65535 pairs per call; partial offsets are 64-bit, so
 * the workspace (gtsfm_twoway_workspace_bytes, ~3.3 MB per 5000 x 5000 pair) is the only bound. Copies the batch descriptor into the workspace and
 * synchronises `stream` once. */
size_t gtsfm_twoway_workspace_bytes(int desc_is_u8, int metric, int dim, int row_stride, int npairs, const int32_t* pairs_host);
int gtsfm_twoway_match(const void* desc_dev, int desc_is_u8, int metric, int dim, int row_stride, int npairs, const int32_t* pairs_host,
                       int use_ratio, double ratio, void* workspace_dev, size_t workspace_bytes, int32_t* matches0_dev, float* dist0_dev,
                       void* stream);

/* gtsfm_twoway_match output -> the verifier's match lists, in the TwoWayMatcher contract's order, on the device.
 *                                  replaces the stable sort by distance of gtsfm/frontend/matcher/twoway_matcher.py:117-147 and the
 *                                  host marshalling between the matcher and the verifier.
 * Pair p owns rows blk_off_dev[p] .. blk_off_dev[p+1] of matches0_dev / dist0_dev (n1 of the pair) and the same rows of
 * match_idx_dev (capacity layout, as gtsfm_verify_compact_matches fills it). Writes the K_p pairs (i, matches0[i]) with
 * matches0[i] >= 0, ordered by (dist0[i] ascending as float32, i ascending), to match_idx_dev + 2 * blk_off_dev[p], and K_p to
 * match_count_dev[p]. Rows beyond K_p are not written. Kept rows must hold a distance >= 0 that is not NaN (what gtsfm_twoway_match
 * writes). Rank by counting over 64-bit integer keys: no workspace, no host synchronisation, no floating-point reduction, the
 * same bytes on every run; any n1 (the cost grows with n1^2). At most 65535 pairs per call. */
int gtsfm_twoway_order_matches(const int32_t* matches0_dev, const float* dist0_dev, const long long* blk_off_dev, int num_pairs,
                               int32_t* match_idx_dev, int32_t* match_count_dev, void* stream);

/* float32 rows holding integers 0 .. 255 (SIFT descriptors as OpenCV emits them) -> uint8 rows, for a device-resident descriptor
 * table that gtsfm_twoway_match reads with desc_is_u8 = 1. Row r: src_dev + r * src_stride floats -> dst_dev + r * dst_stride bytes,
 * `dim` values each. A value that is not an integer in 0 .. 255 (NaN included) is written as 0 and sets *flag_dev to 1; the call
 * never clears the flag, and nothing is clamped or rounded. */
int gtsfm_pack_rows_f32_to_u8(const float* src_dev, long long rows, int dim, int src_stride, uint8_t* dst_dev, int dst_stride,
                              int32_t* flag_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * NetVLAD global descriptor and similarity retrieval
 *   NV = thirdparty/hloc/netvlad.py, SR = gtsfm/retriever/similarity_retriever.py
 * ---------------------------------------------------------------------------------------------------------- */

/* Packed NetVLAD weights (floats) and the packer. tensors_host, torch layouts, in this order: the 13 backbone convolutions
 * conv1_1 .. conv5_3 as (weight [out][in][3][3], bias [out]) pairs (26 tensors), score_proj.weight [64][512], centers [512][64],
 * mean [3]; with whiten also whiten.weight [4096][32768] and whiten.bias [4096] (31 tensors). The whitening matrix is 512 MB.
 *                                                                                                        replaces NV:103-163 */
size_t gtsfm_netvlad_packed_weight_floats(int whiten);
int gtsfm_netvlad_pack_weights(const float* const* tensors_host, int whiten, float* packed_host);

/* Bytes of device workspace a forward / stage call needs for `batch` images of height x width (0 for an invalid shape:
 * batch >= 1, height, width >= 16). Indexing is 64-bit throughout; the workspace (~320 bytes per pixel) is the only bound. */
size_t gtsfm_netvlad_workspace_bytes(int batch, int height, int width);

/* NetVLAD.forward for a batch of equally-sized RGB images, exact fp32.                                  replaces NV:166-202
 * layout 0: image_dev [batch][3][height][width] float32 in [0, 1] (the loader's batch transform output); the reference's
 *           preprocessing clamp(x * 255, 0, 255) - mean is applied as it does.
 * layout 1: image_dev [batch][height][width][3] uint8; equals layout 0 fed with float(u8) / 255, bit for bit.
 * whiten: 1 -> out_dev [batch][4096] (packed weights must include the whitening), 0 -> out_dev [batch][32768].
 * range_flag_dev (optional, int32, not cleared here): bit 0 is set when a layout-0 value is NaN or outside [-1e-6, 1 + 1e-6]
 * (the reference's assert, NV:177); the caller reads it after the call. Per image, the result does not depend on the batch. */
int gtsfm_netvlad_forward(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int whiten,
                          float* out_dev, int32_t* range_flag_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The stages of gtsfm_netvlad_forward (same kernels), for stage-wise tests. stage 0: relu(conv1_1(preprocessed image)),
 * [batch][height][width][64] NHWC; 1: conv5_3 (no ReLU), [batch][height / 16][width / 16][512] NHWC (floor at every pool);
 * 2: the NetVLAD layer's output before whitening, [batch][32768], index d * 64 + k. */
int gtsfm_netvlad_stage(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int stage, float* out_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* Bytes of device workspace gtsfm_retrieval_topk needs for n descriptors of dimension d (with_sim_out: whether the caller
 * passes sim_out_dev; without it the workspace holds the n x n product). */
size_t gtsfm_retrieval_workspace_bytes(int n, int d, int with_sim_out);

/* Similarity retrieval: S = D D^T (exact fp32, v_mfma_f32_32x32x2_f32; only row strips from their diagonal block on are
 * computed), then per row i the kk = min(k, n) best columns j > i with S[i][j] >= min_score (float compare; pass -INFINITY for
 * no threshold) and S[i][j] finite, in descending score order; EQUAL SCORES ARE BROKEN BY THE LOWER j (torch.topk makes no
 * promise). idx_out_dev / score_out_dev [n][kk]: column index or -1 (score -inf) for an empty rank.   replaces SR:98-245
 * sim_out_dev (optional, [n][n]): S in the reference's block layout: (i, j) holds D_i . D_j iff j / blocksize >= i / blocksize,
 * else 0 (n <= 65535). */
int gtsfm_retrieval_topk(const float* desc_dev, int n, int d, int k, float min_score, int blocksize, int32_t* idx_out_dev, float* score_out_dev,
                         float* sim_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MegaLoc global descriptor (DINOv2 ViT-B/14 + SALAD + linear)
 *   ML = thirdparty/megaloc/megaloc.py, MG = gtsfm/frontend/global_descriptor/megaloc_global_descriptor.py,
 *   HF = transformers.models.dinov2.modeling_dinov2 (the backbone's pin: torch.hub's DINOv2 is not in the reference checkout)
 * Fixed: hidden size 768, 12 heads, patch 14, MLP ratio 4, 64 clusters x 256 channels, token part 256, SALAD MLP width 512.
 * From the weights: depth (transformer blocks; 12 in the published model) and feat_dim (8448; a multiple of 64).
 * ---------------------------------------------------------------------------------------------------------- */

/* Packed MegaLoc weights (floats) and the packer (0 for an invalid depth / feat_dim). tensors_host, torch layouts, 20 + 14 * depth
 * tensors in this order: patch_embed.proj.weight [768][3][14][14], its bias, cls_token [768]; per block norm1.weight, norm1.bias,
 * attn.qkv.weight [2304][768] (rows q | k | v), attn.qkv.bias, attn.proj.weight, attn.proj.bias, ls1.gamma, norm2.weight, norm2.bias,
 * mlp.fc1.weight [3072][768], mlp.fc1.bias, mlp.fc2.weight [768][3072], mlp.fc2.bias, ls2.gamma; norm.weight, norm.bias; SALAD
 * token_features.{0,2} (weight, bias) x 2, cluster_features.{0,3} x 2, score.{0,3} x 2 (1 x 1 convolutions as [out][in]), dust_bin [1];
 * linear.weight [feat_dim][16640], linear.bias. The LayerScale vectors are folded into attn.proj and mlp.fc2 (weight rows and
 * bias times gamma, in float32). The position table is not packed: it depends on the image size (see gtsfm_megaloc_forward).
 *                                                                                                replaces ML:19-46, 85-93, 233-263 */
size_t gtsfm_megaloc_packed_weight_floats(int depth, int feat_dim);
int gtsfm_megaloc_pack_weights(const float* const* tensors_host, int depth, int feat_dim, float* packed_host);

/* Bytes of device workspace a forward / stage call needs (0 for an invalid shape: batch >= 1, height and width multiples of 14,
 * more than 64 patches). A batch runs in chunks of at most 64 images through one workspace, so the size stops growing there. */
size_t gtsfm_megaloc_workspace_bytes(int batch, int height, int width, int feat_dim);

/* MegaLocModel.forward for a batch of equally-sized RGB images, exact fp32.                   replaces ML:62-71, 104-120, 144-283 and HF's
 * Dinov2Embeddings / Dinov2Layer / layernorm.
 * pos_dev: the position table [1 + n][768] for THIS grid, n = (height / 14) (width / 14): row 0 the class position, rows 1 .. n the
 *          patch positions interpolated by the caller (HF: bicubic, align_corners = False); weight preparation, not hot path.
 * layout 0: image_dev [batch][3][height][width] float32, already normalised (MG:52-57: x / 255, ImageNet mean / std).
 * layout 1: image_dev [batch][3][height][width] uint8; ((float)u8 / 255 - mean[c]) / std[c] is applied while the patches are read:
 *           equals layout 0 fed with that arithmetic in float32, bit for bit.
 * out_dev [batch][feat_dim], unit rows. flag_dev (optional, int32, not cleared here): bit 0 is set when a layout-0 value is not finite;
 * the caller reads it after the call. Height or width not a multiple of 14 (ML:64-67 resizes) and n <= 64 (NaN in ML:170) are refused.
 * Per image, the result does not depend on the batch. */
int gtsfm_megaloc_forward(const float* packed_weights_dev, int depth, int feat_dim, const float* pos_dev, const void* image_dev, int layout, int batch,
                          int height, int width, float* out_dev, int32_t* flag_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The stages of gtsfm_megaloc_forward (same kernels), for stage-wise tests. stage 0: the tokens after patch embedding, class token and
 * position table, [batch][1 + n][768]; 1: the output of block 0, same shape; 2: the final LayerNorm's tokens (row 0 x_norm_clstoken, rows
 * 1 .. n x_norm_patchtokens), same shape; 3: the SALAD vector before the linear layer, [batch][16640] (token part, then l * 64 + m). */
int gtsfm_megaloc_stage(const float* packed_weights_dev, int depth, int feat_dim, const float* pos_dev, const void* image_dev, int layout, int batch, int height,
                        int width, int stage, float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * D2-Net detector-descriptor, single scale
 *   DM = thirdparty/d2net/lib/model_test.py, DP = thirdparty/d2net/lib/pyramid.py, DU = thirdparty/d2net/lib/utils.py,
 *   DG = gtsfm/frontend/detector_descriptor/d2net.py
 * The dense map of a height x width image is [(height / 2) / 2 - 1][(width / 2) / 2 - 1][512] (floor at both max-pools, then the
 * stride-1 average pool). A candidate record is six 32-bit words: int32 channel, i, j; float step_i, step_j, score.
 * ---------------------------------------------------------------------------------------------------------- */

/* gtsfm_conv3x3_f32 with dilation 2 and zero pad 2 (DM:34-38): out = relu?(conv(in) + bias), same NHWC layouts and the same packed
 * weights (gtsfm_pack_conv3x3; the packing does not depend on the dilation); no pool; cout, out_stride and out_coff multiples of 4; bias_dev holds ceil(cout / 64) * 64 floats (padded, as for gtsfm_conv3x3_f32).
 * Every 64-channel chunk of the input is summed on its own and the chunk sums are added in order, starting from the bias. */
int gtsfm_conv3x3_dil2_f32(const float* in_dev, int in_stride, int in_coff, float* out_dev, int out_stride, int out_coff, const float* packed_w_dev,
                           const float* bias_dev, int batch, int h, int w, int cin, int cout, int relu, void* stream);

/* Packed D2-Net weights (floats) and the packer. tensors_host, torch layouts, 21 tensors in this order: the ten convolutions
 * conv1_1 .. conv3_3, conv4_1 .. conv4_3 (DM:17-38) as (weight [out][in][3][3], bias [out]) pairs, then the uint8 normalisation
 * table [3][256] float32: entry [c][v] = float32(((float32(v) / 255) - mean[c]) / std[c]) evaluated as DU:23-38 does (the division
 * by 255 in float32, the rest in float64).                                                                   replaces DM:16-40 */
size_t gtsfm_d2net_packed_weight_floats(void);
int gtsfm_d2net_pack_weights(const float* const* tensors_host, float* packed_host);

/* Bytes of device workspace a forward / stage call needs (0 for a shape the calls refuse, with the reason in gtsfm_last_error: batch >= 1,
 * height, width >= 8, cand_capacity >= 1, batch * cand_capacity <= 2^28, batch * ceil(height / 8) * ceil(width / 16) < 2^31). cand_capacity: the number of candidate records per image the call can hold. */
size_t gtsfm_d2net_workspace_bytes(int batch, int height, int width, int cand_capacity);

/* D2Net.dense_feature_extraction + process_multiscale(scales = [1]) + the top-k of DG:84-87 for a batch of equally-sized images,
 * exact fp32.                                                                 replaces DM:47-58,110-200, DP:48-128, DU:89-177, DG:84-95
 * layout 0: image_dev [batch][3][height][width] float32, already normalised (DU:35-38).
 * layout 1: image_dev [batch][height][width][3] uint8, normalised through the packed table: equals the reference's input bit for bit.
 * layout 2: image_dev [batch][height][width] uint8, a gray image: the same value in the three channels (DG:113-116).
 * A detection is a (pixel, channel) whose value equals the pixel's channel maximum and the 3 x 3 maximum of its channel (-inf
 * outside the map), with det > 0 and tr * tr / det <= 7.2f of the Hessian (zeros outside the map), whose Newton step -H^-1 g is
 * below 0.5 in both components and whose four bilinear corners lie inside the map. Arithmetic, in this order:
 *   dii = (up - 2 x) + down, djj = (left - 2 x) + right, dij = 0.25 (((x[-1,-1] - x[-1,+1]) - x[+1,-1]) + x[+1,+1]),
 *   det = dii djj - dij dij, di = 0.5 down - 0.5 up, dj = 0.5 right - 0.5 left,
 *   step_i = -((djj / det) di + (-dij / det) dj), step_j = -((-dij / det) di + (dii / det) dj).
 * The candidates are sorted by score descending, EQUAL SCORES BY (channel, i, j) ASCENDING (np.argsort in DG:84 is not stable and
 * makes no promise); the first min(count, max_keypoints) are kept.
 * counts_dev [batch] int32: the number of candidates FOUND per image. When one exceeds cand_capacity that image's outputs are
 *   incomplete and the call has to be repeated with at least that capacity; nothing is truncated silently. The number of
 *   keypoints of an image is min(counts_dev[b], max_keypoints).
 * keypoints_dev [batch][max_keypoints][2] (x, y) = ((p * 2 + 0.5) * 2 + 0.5 of (j, i) + step), scores_dev [batch][max_keypoints],
 * desc_dev [batch][max_keypoints][512] unit rows (bilinear interpolation DU:149-164 left to right, x / max(||x||, 1e-12)).
 * Per image, the result does not depend on the batch. */
int gtsfm_d2net_forward(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int max_keypoints,
                        int cand_capacity, int32_t* counts_dev, float* keypoints_dev, float* scores_dev, float* desc_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream);

/* The stages of gtsfm_d2net_forward (same kernels), for stage-wise tests. stage 0: relu(conv1_1(normalised image)),
 * [batch][height][width][64] NHWC; 1: relu(conv3_3), [batch][height / 4][width / 4][256]; 2: the dense map, [batch][H2][W2][512];
 * 3: the sorted candidate list, out_dev [batch][cand_capacity] records of which the first min(counts_dev[b], cand_capacity) are
 * written, and counts_dev [batch] (used by stage 3 only). */
int gtsfm_d2net_stage(const float* packed_weights_dev, const void* image_dev, int layout, int batch, int height, int width, int stage, int cand_capacity,
                      void* out_dev, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The detection head alone on a caller's dense map map_dev [batch][map_height][map_width][512]: counts_dev as above,
 * candidates_dev (optional) [batch][cand_capacity] sorted records, and for max_keypoints > 0 the three keypoint outputs. */
size_t gtsfm_d2net_detect_workspace_bytes(int batch, int cand_capacity);
int gtsfm_d2net_detect(const float* map_dev, int batch, int map_height, int map_width, int max_keypoints, int cand_capacity, int32_t* counts_dev,
                       void* candidates_dev, float* keypoints_dev, float* scores_dev, float* desc_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SIFT detector-descriptor, OpenCV's SIFT_create() defaults
 *   SG = gtsfm/frontend/detector_descriptor/sift.py (cv.SIFT_create().detectAndCompute + Keypoints.get_top_k)
 * nOctaveLayers 3, contrastThreshold 0.04, edgeThreshold 10, sigma 1.6, float32 pyramid, first octave -1 (the image is doubled).
 * The pyramid of a height x width image has n = round(log2(min(2 height, 2 width))) - 2 octaves; octave o is (2 height >> o) x
 * (2 width >> o). Its layout in floats: the six Gaussian images of octave 0, of octave 1, ..., then the five DoG images of octave 0, ...
 * Records (32-bit words): a candidate is int32 octave, layer, row, column; a keypoint is those four, then float x = column + X0,
 * y = row + X1 (octave coordinates), scl = 1.6 * 2^((layer + X2) / 3), response; an oriented keypoint is a keypoint followed by float
 * angle (degrees) and a zero word. Final coordinates: (x, y) * 2^(octave - 1), size = scl * 2^octave.
 * tests/sift_reference.py restates every stage in numpy in the same operation order; the device equals it bit for bit.
 * ---------------------------------------------------------------------------------------------------------- */

/* Octaves and floats of the pyramid (0 for a shape the calls refuse). */
int gtsfm_sift_num_octaves(int height, int width);
size_t gtsfm_sift_pyramid_floats(int height, int width);

/* Bytes of device workspace a call needs (0 for a shape the calls refuse, with the reason in gtsfm_last_error: batch >= 1, both
 * edges in 1 .. 16383, cand_capacity in 1 .. 2^26, kp_capacity in 1 .. 2^24). The workspace holds ONE image's pyramid: a batch runs
 * image after image on the stream. cand_capacity: candidate records; kp_capacity: keypoint and oriented-keypoint records. */
size_t gtsfm_sift_workspace_bytes(int batch, int height, int width, int cand_capacity, int kp_capacity);

/* detectAndCompute + top-k for a batch of equally-sized gray images.                                         replaces SG:41-54
 * gray_dev [batch][height][width] uint8; mask_dev the same shape or NULL: a keypoint whose mask[round(y)][round(x)] is 0 is dropped
 * before the top-k. The first min(counts_dev[4 b + 2], max_keypoints) rows of image b are written, ordered by response descending,
 * equal responses by (octave, layer, row, column, angle) ascending (OpenCV and get_top_k promise no order):
 * keypoints_dev [batch][max_keypoints][4] = x, y, size, response; desc_dev [batch][max_keypoints][128] float32 holding the integers
 * 0 .. 255 that cv2 returns.
 * counts_dev [batch][4] int32: candidates, keypoints and oriented keypoints FOUND, and 0. The call waits for the stream; when a
 * count exceeds its capacity it returns GTSFM_ERR_WORKSPACE with the counts in gtsfm_last_error and that image's outputs are
 * incomplete: repeat with at least those capacities. Per image, the result does not depend on the batch or on the run. */
int gtsfm_sift_detect_and_describe(const uint8_t* gray_dev, const uint8_t* mask_dev, int batch, int height, int width, int max_keypoints, int cand_capacity,
                                   int kp_capacity, int32_t* counts_dev, float* keypoints_dev, float* desc_dev, void* workspace_dev, size_t workspace_bytes,
                                   void* stream);

/* The stages of one image (same kernels), for stage-wise tests and timing; the call does not wait. stage 0: the pyramid,
 * out_dev [gtsfm_sift_pyramid_floats] float32; 1: candidates, out_dev [cand_capacity] records in any order; 2: keypoints,
 * out_dev [kp_capacity] records in any order; 3: oriented keypoints after the mask, out_dev [kp_capacity] records in the output
 * order. counts_dev [4] as above (stages >= 1); of every list the first min(count, capacity) records are written. */
int gtsfm_sift_stage(const uint8_t* gray_dev, const uint8_t* mask_dev, int height, int width, int stage, int cand_capacity, int kp_capacity, void* out_dev,
                     int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The explicit float32 functions behind the byte-identity contract, element-wise on n (1 .. 2^24) elements, for tests: one small
 * kernel that calls the __device__ functions the pipeline calls; the call does not wait. All arrays hold 32-bit words.
 *   EXP2, EXP     in [n] float t                      -> out [n] float
 *   ATAN2_DEG     in [n][2] float y, x                -> out [n] float degrees in [0, 360]
 *   SINCOS_DEG    in [n] float degrees                -> out [n][2] float cos, sin
 *   SOLVE3        in [n][12] float A (row-major), b   -> out [n][3] float X with A X = b (a singular system gives 0)
 *   REFLECT101    in [n][2] int32 index, length       -> out [n] int32 (-1 unless 1 <= length <= 2^24 and |index| <= 2^24)
 *   PEAK_ANGLE    in [n][4] int32 bin j, float h[j - 1], h[j], h[j + 1] of the smoothed orientation histogram -> out [n] float degrees */
enum {
    GTSFM_SIFT_FN_EXP2 = 0,
    GTSFM_SIFT_FN_EXP = 1,
    GTSFM_SIFT_FN_ATAN2_DEG = 2,
    GTSFM_SIFT_FN_SINCOS_DEG = 3,
    GTSFM_SIFT_FN_SOLVE3 = 4,
    GTSFM_SIFT_FN_REFLECT101 = 5,
    GTSFM_SIFT_FN_PEAK_ANGLE = 6
};
int gtsfm_sift_math(int fn, const void* in_dev, void* out_dev, int n, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Feature tracks: union-find over verified matches
 *   replaces gtsfm/data_association/dsf_tracks_estimator.py:51-85, cpp_dsf_tracks_estimator.py:63-84 (gtsam's DSFMapIndexPair /
 *   tracksFromPairwiseMatches), called twice per scene from gtsfm/multi_view_optimizer.py:185,199,266-268.
 * A node is a keypoint: node = node_off[image] + k (in the generators' capacity layout node_off[image] = image * capacity). An edge is
 * a match row (k1, k2) of pair (i1, i2); i1 == i2 is legal. A row is ACTIVE when its pair is enabled, it lies below match_count[p]
 * (when counts are given) and mask[row] != 0 (when a mask is given). Every connected component of the active edges is a track, unless
 * it holds two keypoints of one image: those are counted as discarded (the reference's validate_unique_cameras).
 * The result depends on the SET of active edges only: not on the order of pairs or rows, on duplicates, or on the run.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace for num_nodes keypoints (0 for a negative size or num_nodes >= 2^31). The match rows are read where they
 * lie, so the size (about 50 bytes per node) does not grow with total_matches. */
size_t gtsfm_tracks_workspace_bytes(long long num_nodes, long long total_matches);

/* match_idx_dev [total_matches][2] int32, pair p owning rows match_off_dev[p] .. match_off_dev[p+1] (the verifier's layout, see
 * gtsfm_verify_essential_f64); match_count_dev [num_pairs], inlier_mask_dev [total_matches] and pair_enable_dev [num_pairs] are optional
 * (NULL: every row / every pair). pair_images_dev [num_pairs][2] = (i1, i2); node_off_dev [num_images + 1], ascending, with
 * num_nodes = node_off_dev[num_images] < 2^31. kp_xy_dev (optional) [num_nodes][2] float32.
 * Outputs, capacities in entries with C = min(num_nodes, 2 * total_matches): track_image_dev [C], track_kp_dev [C], track_uv_dev [C][2]
 * (optional; kp_xy_dev[node] bit for bit), track_off_dev [C + 1] (a track has at least two measurements, so C / 2 + 1 entries are enough
 * unless a row matches a keypoint to itself, which makes a track of one). Track t owns measurements track_off_dev[t] ..
 * track_off_dev[t+1]. Tracks are ordered by their smallest (image, keypoint) member, the measurements of a track by image ascending.
 * counts_dev [8] int32: tracks, measurements, discarded tracks, components (tracks + discarded), rounds, 0, 0, 0.
 * The labelling runs in rounds of two launches (hook, compress) and the call reads a 4-byte flag from `stream` after each; a round
 * that hooks nothing ends it, rounds counts that one too. After 64 rounds without a fixed point the call fails with the sizes in
 * gtsfm_last_error and writes no result. An active row that names an image or a keypoint outside the tables is refused the same way.
 * num_pairs == 0 or total_matches == 0: zero counts and track_off_dev[0] = 0, nothing else is touched. */
int gtsfm_tracks_from_matches(const int32_t* match_idx_dev, const long long* match_off_dev, const int32_t* match_count_dev,
                              const uint8_t* inlier_mask_dev, const uint8_t* pair_enable_dev, const int32_t* pair_images_dev, int num_pairs,
                              long long total_matches, const long long* node_off_dev, int num_images, const float* kp_xy_dev, void* workspace_dev,
                              size_t workspace_bytes, long long* track_off_dev, int32_t* track_image_dev, int32_t* track_kp_dev, float* track_uv_dev,
                              int32_t* counts_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Triangulation of feature tracks (float64)
 *   replaces gtsfm/data_association/point3d_initializer.py:139-295 per track, called from data_assoc.py:205-273.
 * PARITY UNPINNED towards gtsam: triangulatePoint3(rank_tol = 1e-9, optimize = true) is restated as DLT + 8 damped Gauss-Newton steps
 * + cheirality, and np.random.choice by a counter-based sampler; the specification is tests/triangulation_reference.py.
 * mode: 0 NO_RANSAC, 1 RANSAC_SAMPLE_UNIFORM, 2 RANSAC_SAMPLE_BIASED_BASELINE, 3 RANSAC_TOPK_BASELINES. A track of n measurements has
 * C(n,2) measurement pairs in itertools.combinations order; min(num_hypotheses, C(n,2)) of them are evaluated: all of them, or those
 * with the smallest sampling keys (splitmix64 of seed, the track's first measurement and the pair index; see the specification).
 * exit codes: 0 SUCCESS, 1 CHEIRALITY_FAILURE, 2 INLIERS_UNDERCONSTRAINED, 3 POSES_UNDERCONSTRAINED, 4 EXCEEDS_REPROJ_THRESH,
 * 5 LOW_TRIANGULATION_ANGLE. A track's outputs depend on its own measurements, the cameras and the options only.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace (0 for sizes out of range): 8 per track plus 20 per hypothesis record, of which there are at most
 * min(num_tracks * max_hypotheses, total_measurements * sqrt(max_hypotheses / 2) + num_tracks). max_hypotheses = 0 for NO_RANSAC. */
size_t gtsfm_triangulate_workspace_bytes(long long num_tracks, long long total_measurements, long long max_hypotheses);

/* The CSR arrays gtsfm_tracks_from_matches writes: track_off_dev [num_tracks + 1] ascending within 0 .. total_measurements,
 * track_image_dev [total_measurements], track_uv_dev [total_measurements][2] float32 (pixels). cameras_dev [num_images][17] float64:
 * valid (0: not estimated), fx, fy, cx, cy, wRc row-major, wtc; an image index outside the table counts as not estimated.
 * reproj_error_threshold > 0, infinity allowed; min_triangulation_angle_deg <= 0 switches the angle test off.
 * Outputs: point_dev [num_tracks][3] (NaN unless SUCCESS), avg_error_dev [num_tracks] (NaN where the reference returns None),
 * exit_code_dev [num_tracks], inlier_mask_dev [total_measurements] uint8, stats_dev [num_tracks][4] int32: hypotheses evaluated,
 * of those skipped (camera missing, underconstrained, cheirality), winning pair index or -1, its votes.
 * A track with fewer than two measurements gets INLIERS_UNDERCONSTRAINED. The call waits for the stream once, to report offsets that are
 * not ascending or a track longer than 65535 as GTSFM_ERR_INVALID. */
int gtsfm_triangulate_tracks_f64(const long long* track_off_dev, const int32_t* track_image_dev, const float* track_uv_dev, long long num_tracks,
                                 long long total_measurements, const double* cameras_dev, int num_images, int mode, double reproj_error_threshold,
                                 double min_triangulation_angle_deg, long long num_hypotheses, unsigned long long seed, void* workspace_dev,
                                 size_t workspace_bytes, double* point_dev, double* avg_error_dev, int32_t* exit_code_dev, uint8_t* inlier_mask_dev,
                                 int32_t* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Two-view bundle adjustment (float64)
 *   replaces gtsfm/two_view_estimator.py:212-288 (TwoViewEstimator.bundle_adjust: triangulate_two_view_correspondences :165-210, the
 *   factor graph and Levenberg-Marquardt of gtsfm/bundle/two_view_ba.py / bundle_adjustment.py, the reprojection-error filter of
 *   gtsfm/common/gtsfm_data.py:839-852), called per pair from run_2view :411-426.
 * PARITY UNPINNED towards gtsam: its Levenberg-Marquardt path and retraction, the cheirality convention, the pivot thresholds of the
 * indeterminate-system test, calibrations held fixed (the reference's priors on them have sigma 1e-5) and no pose priors; the
 * specification is tests/two_view_ba_reference.py.
 * status: 0 OK, 1 SKIPPED (fewer verified correspondences than min_verified: the verifier's result passes through), 2 NO_INITIAL_POSE
 * (NaN pose: NaN out, the verifier's mask passes through), 3 NONE_TRIANGULATED (the initial pose, an empty mask), 4 INDETERMINATE
 * (NaN pose and an empty mask unless allow_indeterminate). A pair's outputs depend on its own data (the places of its verified rows within
 * its slice included) and the options only, byte for byte.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace (0 for sizes out of range): about 120 per match row, the two-measurement tracks and their triangulation. */
size_t gtsfm_two_view_ba_workspace_bytes(long long num_pairs, long long total_matches);

/* The verifier's arrays where they lie (see gtsfm_verify_essential_f64): kp_xy_dev, kp_off1_dev / kp_off2_dev [num_pairs], match_idx_dev
 * [total_matches][2], match_off_dev [num_pairs + 1], match_count_dev [num_pairs] (optional, capacity layout), inlier_mask_dev
 * [total_matches], intrinsics_dev [num_pairs][8], rotation_dev [num_pairs][9] i2Ri1 and translation_dev [num_pairs][3] i2Ui1.
 * PRECONDITION, as for the verifier: a verified row below match_count_dev names keypoints inside the tables (the call has no table sizes
 * to check them against; a negative index leaves the row without cameras, rows at or past match_count_dev are never read).
 * Options: max_iterations accepted steps at most; reproj_error_threshold of the filter in pixels; huber_k (infinity: no robust loss);
 * the sigmas of the measurements (pixels), the pose prior on the pair's first camera and the point prior on its first point; min_verified
 * (InlierSupportProcessor's min_num_inliers_est_model); triangulation_threshold / triangulation_min_angle_deg: the TriangulationOptions
 * of the two-view triangulation (NO_RANSAC), done by gtsfm_triangulate_tracks_f64 itself on two-measurement tracks.
 * Outputs per pair: rotation_out_dev [9] and unit translation_out_dev [3]; cost_dev [2] (initial, final; NaN unless adjusted);
 * stats_dev [8] int32 = status, verified, triangulated, valid, accepted steps, linear solves tried, 0, 0. Per match row of a pair's
 * slice: valid_mask_dev (1 = verified, triangulated and both reprojection errors under the threshold; the verifier's rows, so that
 * gtsfm_tracks_from_matches takes it in place of inlier_mask_dev) and point_dev [3] (NaN unless triangulated). Rows outside every
 * pair's slice are not written. The call waits for the stream; match_off_dev not ascending within 0 .. total_matches is
 * GTSFM_ERR_INVALID. */
int gtsfm_two_view_ba_f64(const float* kp_xy_dev, const long long* kp_off1_dev, const long long* kp_off2_dev, const int32_t* match_idx_dev,
                          const long long* match_off_dev, const int32_t* match_count_dev, long long total_matches, const uint8_t* inlier_mask_dev,
                          const double* intrinsics_dev, const double* rotation_dev, const double* translation_dev, int num_pairs, int max_iterations,
                          double reproj_error_threshold, double huber_k, double measurement_sigma, double pose_prior_sigma, double point_prior_sigma,
                          int min_verified, int allow_indeterminate, double triangulation_threshold, double triangulation_min_angle_deg,
                          void* workspace_dev, size_t workspace_bytes, double* rotation_out_dev, double* translation_out_dev, uint8_t* valid_mask_dev,
                          double* point_dev, double* cost_dev, int32_t* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * View-graph estimation: rotation cycle consistency and the largest connected component (float64)
 *   replaces gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:80-157,224-240 (run, the per-edge aggregate),
 *   gtsfm/utils/graph.py:92-149 (create_adjacency_list, extract_cyclic_triplets_from_edges), gtsfm/utils/geometry_comparisons.py:137-159,
 *   226-241 (the cycle error) and gtsfm/utils/graph.py:24-89 (the largest component), called from gtsfm/multi_view_optimizer.py:82-84,
 *   130-164,175: the configured estimator, once more with MEDIAN_EDGE_ERROR, then prune_to_largest_connected_component.
 * A vertex is an image; an edge is a row: pair_images_dev [E][2] int32 = (i1, i2), rotation_dev [E][9] float64 = i2Ri1 row-major (what the
 * verifier and gtsfm_two_view_ba_f64 write), pair_enable_dev [E] uint8 optional (NULL: every row). An edge is an INPUT EDGE when it is
 * enabled and its nine numbers are finite (the device form of _get_valid_input_edges). An enabled edge with i1 >= i2, an index outside
 * 0 .. num_images - 1, or the pair of another enabled edge makes the call fail (GTSFM_ERR_INVALID, gtsfm_last_error) with no output written.
 * For every input edge (a, b), each common neighbour c of a and b over the input edges is a triplet. Its error is the angle in degrees of
 * M = i2Ri0^T . i2Ri1 . i1Ri0 over the sorted triplet i0 < i1 < i2 (products in that order), found as scipy's
 * Rotation.from_matrix(M).as_rotvec() norm finds it: matrix -> quaternion by the largest of trace and diagonal, normalised, then
 * 2 atan2(|q_xyz|, |q_w|). The error of a triplet is the same bytes on its three edges. criterion 0 = MIN_EDGE_ERROR, 1 = MEDIAN_EDGE_ERROR
 * (numpy's median: the middle element, or (lo + hi) / 2 of the two middle ones); keep = aggregate < error_threshold, strict; an input edge
 * without a triplet is kept. Every output depends on the SET of input edges and their rotations only: permuting the rows permutes the
 * per-edge outputs byte for byte and leaves the triplet list unchanged.
 * PARITY UNPINNED towards the reference: gtsam's Rot3.between / compose arithmetic, restated as float64 matrix products in the stated order;
 * rotations that are not orthonormal: scipy's from_matrix re-orthogonalises M and this routine takes it as it is, as stated above. With
 * every entry off by a factor 1 + N(0, 1e-6) (M M^T off the identity by 7.5e-6) scipy 1.15.3 differs from this routine by 9.7e-5 degrees
 * (tests/view_graph_scenes.py, hard_cycles_skewed), for 30 degrees scaled by 1.01 it returns 30.000 where the definition gives 30.076, and
 * it raises on a non-positive determinant where this routine answers; the device is held to the definition. An edge whose aggregate lies
 * within the measured tolerance of the threshold (profiles/view_graph_gpu_tests.txt) is kept or dropped by the last bits, and NaN or a
 * threshold no aggregate is below (NaN, 0) keeps only the input edges without a triplet. The specification is tests/view_graph_reference.py.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace for either call below (0 for sizes out of range: a negative one, 2^28 edges or images, 2^31 / 3 triplets):
 * about 60 per edge, 12 per image and 24 per triplet of capacity. */
size_t gtsfm_view_graph_workspace_bytes(long long num_edges, long long num_images, long long triplet_capacity);

/* Per edge row: num_triplets_dev [E] int32, aggregate_error_dev [E] float64 (NaN without a triplet or when not an input edge), keep_dev [E]
 * uint8 (0 when not an input edge). counts_dev [8] int32: input edges, kept edges, distinct triplets, the largest per-edge triplet count,
 * 0, 0, 0, 0. triplets_dev [triplet_capacity][3] int32 and cycle_error_dev [triplet_capacity] (both optional, together): each distinct
 * triplet once, sorted nodes, in lexicographic order; the first counts_dev[2] rows are written.
 * The call waits for the stream twice: for the two input flags, and for the triplet count T, which it also stores in *num_triplets_host
 * (optional host pointer; -1 until known). T > triplet_capacity is GTSFM_ERR_WORKSPACE with no output written: repeat with a workspace and
 * outputs for at least T. num_edges == 0: zero counts, nothing else is touched. */
int gtsfm_view_graph_cycle_filter_f64(const int32_t* pair_images_dev, const double* rotation_dev, const uint8_t* pair_enable_dev, long long num_edges,
                                      int num_images, int criterion, double error_threshold, long long triplet_capacity, void* workspace_dev,
                                      size_t workspace_bytes, int32_t* num_triplets_dev, double* aggregate_error_dev, uint8_t* keep_dev, int32_t* counts_dev,
                                      int32_t* triplets_dev, double* cycle_error_dev, long long* num_triplets_host, void* stream);

/* The largest connected component of the enabled edges (any order of i1 and i2; i1 == i2 is legal). node_mask_dev [num_images] uint8;
 * pair_keep_dev [E] uint8: enabled and both endpoints in the component; counts_dev [8] int32: nodes and edges of the component, components
 * with at least one edge, 0, .... Of components of equal size the one that owns the enabled edge with the smallest row wins, as
 * max(nx.connected_components(g), key=len) decides after add_edges_from in row order. The labelling runs in rounds of two launches and
 * reads a 4-byte flag after each, as gtsfm_tracks_from_matches does, and refuses after 64 rounds; an enabled edge that names an image
 * outside 0 .. num_images - 1 is refused the same way, with no output written. */
int gtsfm_largest_component(const int32_t* pair_images_dev, const uint8_t* pair_enable_dev, long long num_edges, int num_images, void* workspace_dev,
                            size_t workspace_bytes, uint8_t* node_mask_dev, uint8_t* pair_keep_dev, int32_t* counts_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Translation averaging, first half: 1DSfM outlier rejection (float64)
 *   replaces gtsfm/averaging/translation/averaging_1dsfm.py:234-315 (compute_inliers, with gtsam's MFAS per projection direction), :403-437
 *   (_get_landmark_directions) and :684-707 (get_valid_measurements_in_world_frame), called from gtsfm/multi_view_optimizer.py:175-199.
 * Camera i is node i, track j is node num_images + j. A pair row (i1, i2, i2Ui1) is the measurement (key1, key2) = (i2, i1) with the world
 * direction unit(wRi2 . i2Ui1); it is VALID when it is enabled (pair_enable_dev, NULL: every row), rotation_valid_dev[i2] is set (i1's
 * rotation is not looked at, as in the reference) and the three numbers are finite. A track measurement s of track j (track_off_dev [T + 1],
 * image_dev [S], uv_dev [S][2]: the track builder's CSR) is the measurement (camera, num_images + j) with the direction
 * unit(wRi . unit(((u - cx) / fx, (v - cy) / fy, 1))) for intrinsics_dev [N][4] = fx, fy, cx, cy; it is valid when track_enable_dev[j] and
 * meas_enable_dev[s] (NULL: all) are set and the direction is finite. unit(v) = v / sqrt((x x + y y) + z z); a matrix row is summed as
 * (r0 x + r1 y) + r2 z. With directions_given != 0 the world directions are INPUTS in world_pair_dev / world_meas_dev (valid: enabled and
 * finite) and rotation, intrinsics, pair_direction and uv are not read.
 * Per projection direction d (directions_dev [D][3], unit vectors) an edge has w = (mx dx + my dy) + mz dz and runs key1 -> key2 unless
 * w < 0. MFAS: inW / outW per node are the sums of |w| over its edges in ascending (key1, key2) order; then, one node per step: the
 * smallest id with inW < 1e-8 if there is one, else the largest (outW + 1) / (inW + 1), ties to the smallest id; the chosen node's |w| is
 * subtracted from outW of its remaining in-neighbours and inW of its remaining out-neighbours. An edge whose source was chosen after its
 * destination weighs |w|, else 0; the weights are added over the directions in order and divided by D; inlier = mean < threshold. A pair's
 * cameras become inlier cameras; a measurement stays an inlier only when its camera is one. Every byte is fixed by the inputs: not by the
 * grid, the row order of the lists, the storage tier or timing (tests/translation_inliers_reference.py is the specification).
 * Refused (GTSFM_ERR_INVALID, gtsfm_last_error): an enabled pair row with i1 >= i2 or an id out of range, a measurement listed twice, an
 * enabled measurement whose camera is out of range or has no valid rotation, D <= 0 with rows present.
 * PARITY UNPINNED towards the reference: gtsam's MFAS picks among several roots or tied scores in the order of an unordered_map; Unit3's
 * normalisation in the last bits; calibrations with distortion (not handled). TranslationRecovery is the next call, gtsfm_translation_recovery_f64.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace (0 for sizes out of range). node_capacity: the most nodes that may have an edge (at most num_images +
 * num_tracks; the host knows num_images + the enabled tracks). lds_node_limit: up to this many graph nodes the MFAS state is kept in LDS,
 * beyond it in a slice of the workspace per workgroup; negative or more than 2048: 2048. Both tiers give the same bytes. */
size_t gtsfm_translation_inliers_workspace_bytes(long long num_pairs, long long num_meas, long long num_images, long long num_tracks,
                                                 long long num_directions, long long node_capacity, int lds_node_limit);

/* Outputs: world_pair_dev [E][3], world_meas_dev [S][3] (NaN rows where not valid), pair_weight_dev [E], meas_weight_dev [S] (the mean
 * outlier weight, NaN where not valid), pair_inlier_dev [E], meas_inlier_dev [S], camera_inlier_dev [N] uint8, position_dev [D][N + T] int32
 * (optional: each node's place in the ordering of each direction, -1 for a node without an edge), counts_dev [8] int32: valid pair rows,
 * valid measurements, nodes with an edge, inlier pairs, inlier measurements, inlier cameras, 0, 0. The call waits for the stream once, for
 * the refusal flags and the node count; more nodes than node_capacity is GTSFM_ERR_WORKSPACE. */
int gtsfm_translation_inliers_f64(const int32_t* pair_images_dev, const double* pair_direction_dev, const uint8_t* pair_enable_dev, long long num_pairs,
                                  const double* rotation_dev, const uint8_t* rotation_valid_dev, const double* intrinsics_dev, int num_images,
                                  const long long* track_off_dev, const int32_t* image_dev, const float* uv_dev, const uint8_t* track_enable_dev,
                                  const uint8_t* meas_enable_dev, long long num_tracks, long long num_meas, const double* directions_dev,
                                  long long num_directions, double threshold, int directions_given, long long node_capacity, int lds_node_limit,
                                  void* workspace_dev, size_t workspace_bytes, double* world_pair_dev, double* world_meas_dev, double* pair_weight_dev,
                                  double* meas_weight_dev, uint8_t* pair_inlier_dev, uint8_t* meas_inlier_dev, uint8_t* camera_inlier_dev,
                                  int32_t* position_dev, int32_t* counts_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Rotation averaging (float64)
 *   replaces gtsfm/averaging/rotation/shonan.py:122-168,185-204 (ShonanRotationAveraging._run_with_consecutive_ordering and
 *   chordal_initialize: gtsam's InitializePose3::initializeOrientations and ShonanAveraging3 at p = 3), called from
 *   gtsfm/multi_view_optimizer.py between the view graph and 1DSfM.
 * A node is an image, R_k = wRk. A row is pair_images_dev [E][2] int32 = (i1, i2), rotation_dev [E][9] float64 = M = i2Ri1 row-major (what
 * the verifier and gtsfm_two_view_ba_f64 write; the model is wRi1 = wRi2 . M), weight_dev [E] float64 = kappa = 1 / sigma^2, pair_enable_dev
 * [E] uint8 optional (NULL: every row). Either orientation of a pair and the same pair several times are legal (priors are further rows).
 * A row is VALID when it is enabled, its nine numbers and its weight are finite and kappa > 0. An enabled row with i1 == i2 or an index
 * outside 0 .. num_images - 1 makes the call fail (GTSFM_ERR_INVALID, gtsfm_last_error) with no output written.
 * The cost is f(R) = sum_e kappa_e |R_i2 M_e - R_i1|_F^2 over SO(3)^n: Shonan's chordal cost at p = 3 up to gtsam's factor 1/2. anchor = -1
 * takes the i2 of the valid row with the smallest row index (measurements[0].key1()). Only the anchor's connected component over the valid
 * rows is solved; every other image gets a NaN rotation and node_valid 0; the output gauge is R_anchor = I exactly.
 * A. Chordal initialisation: min sum_e |X_i2 M_e - X_i1|_F^2 over 3 x 3 matrices, unweighted, X_anchor = I, by conjugate gradients from X = 0
 * (one step length for the nine columns) to |r| <= chordal_tol |r0| or chordal_max_iterations; every X_k is projected onto SO(3) by a
 * one-sided Jacobi SVD. B. Riemannian trust region with Steihaug-Toint truncated CG and the exact Hessian (as SE-Sync at fixed rank), the
 * Cayley retraction, rho regularised as Manopt does; accept at rho > 0.1, Delta / 4 under 0.25, Delta * 2 above 0.75 on the boundary; the
 * inner loop ends at |r| <= |r0| min(kappa_cg, |r0|^theta) (theta one of 0, 0.5, 1, 2: there is no libm call in the stage), on the boundary,
 * on negative curvature or after max_inner steps (0: three per node); the outer loop ends at |g|_inf <= gradient_tol * max kappa or after
 * max_outer iterations. Sums run over a node's rows in ascending (neighbour, row) order and over the nodes by a fixed pairwise tree, so
 * every byte is fixed by the inputs: not by the lane count, the run, or the problem's place in a batch. The specification is
 * tests/rotation_averaging_reference.py, operation for operation.
 * Batch: problem_row_off_dev [P + 1] int64 (NULL with num_problems 1: one problem over every row) gives each problem a row range of the same
 * arrays; one workgroup solves one problem. Offsets not ascending within 0 .. num_rows are refused like a bad row.
 * PARITY UNPINNED towards the reference (nothing of gtsam was observed running): its Levenberg-Marquardt path, the soft anchor and the
 * Karcher / gauge terms, Rot3::ClosestTo in the last bits, its output gauge. NOT DONE HERE: Shonan's optimality certificate and the rank
 * staircase p > 3 -- the point returned is a critical point reached from the chordal start, which on graphs with outliers may not be the
 * global minimum (tests/rotation_averaging_scenes.py holds one such scene); Huber weighting; the random start.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace (0 for sizes out of range: negative, 2^28 rows, 2^24 images, 2^28 images over all problems): 33 per row and about
 * 570 per image and problem. One workgroup solves one problem, start to end: a node's list is ranked in O(degree^2) and every pass walks
 * the lists with 256 lanes, so a call's time grows with rows x steps on ONE CU (163 ms at 48 725 rows and 1000 images, measured). The size
 * limits above are those of the index arithmetic, not a promise of speed: beyond about 10^5 rows or a degree of a few thousand split the
 * graph into problems (clusters) of a batch. */
size_t gtsfm_rotation_averaging_workspace_bytes(long long num_rows, long long num_images, long long num_problems);

/* Outputs per problem: rotation_out_dev [P][num_images][9] wRi (NaN outside the component), node_valid_dev [P][num_images] uint8,
 * counters_dev [P][8] int32 = status (0 CONVERGED, 1 MAX_ITERATIONS, 2 NO_VALID_ROW: all outputs NaN / 0, 3 NON_FINITE: a NaN met inside,
 * outputs NaN, mask 0), outer iterations, accepted steps, Hessian applications, chordal CG steps, component size, anchor, valid rows;
 * costs_dev [P][4] float64 = the cost with every rotation the identity, after the chordal initialisation, at the end, and the final
 * |g|_inf. The call waits for the stream once, for the two refusal flags; the inputs are not changed. */
int gtsfm_rotation_averaging_f64(const int32_t* pair_images_dev, const double* rotation_dev, const double* weight_dev, const uint8_t* pair_enable_dev,
                                 long long num_rows, int num_images, const long long* problem_row_off_dev, int num_problems, int anchor,
                                 double chordal_tol, int chordal_max_iterations, double delta0, double kappa_cg, double theta, double gradient_tol,
                                 int max_outer, int max_inner, void* workspace_dev, size_t workspace_bytes, double* rotation_out_dev,
                                 uint8_t* node_valid_dev, int32_t* counters_dev, double* costs_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Translation averaging, second half: translation recovery (float64)
 *   replaces gtsfm/averaging/translation/averaging_1dsfm.py:439-495 (__run_averaging: gtsam's TranslationRecovery over the inlier
 *   measurements, sigma 0.01, Huber k = 1.3), called from gtsfm/multi_view_optimizer.py right after the outlier rejection.
 * The inputs are the arrays gtsfm_translation_inliers_f64 takes and leaves on the device. Camera i is node i, track j of a problem whose
 * first track is t0 is node num_images + (j - t0) (num_images + j for a single problem). A pair row (i1, i2) with the world direction z =
 * w_i2Ui1 (world_pair_dev [E][3]) is the measurement a = i2, b = i1; measurement s of track j (track_off_dev [T + 1], image_dev [S],
 * world_meas_dev [S][3]) is a = image[s], b = the track's node; the model is unit(x_b - x_a) = z. A row is VALID when it is enabled
 * (pair_enable_dev / meas_enable_dev, normally the 1DSfM inlier masks; NULL: every row) and its three numbers are finite. Refused
 * (GTSFM_ERR_INVALID, gtsfm_last_error, no output written): an enabled pair with i1 >= i2, an enabled row with an image outside
 * 0 .. num_images - 1, track or problem offsets that are not ascending within their range, a problem with more than max_problem_tracks tracks.
 * The cost is f(x) = sum_e rho(|unit(x_b - x_a) - z_e| / sigma) with Huber's rho (huber_k <= 0 or inf: the half square), plus one SCALE ROW
 * rho(|(x_b - x_a) - scale_factor z| / sigma) on the first valid row of the solved component. The gauge is hard: x_anchor = 0 exactly, the
 * anchor is not an unknown; anchor = -1 takes the a of the first valid row (measurements[0].key1()). Only the anchor's connected component
 * over the valid rows is solved; every other node gets NaN and node_valid 0.
 * A. Initialisation: min sum_e |x_b - x_a - scale_factor z_e|^2, x_anchor = 0: the scalar graph Laplacian with three right-hand sides, by
 * conjugate gradients from x = 0 (one step length) to |r| <= init_tol |r0| or init_max_iterations. B. Trust region on the Gauss-Newton
 * model with the Huber weights w = min(1, k sigma / |r|): gradient sum +- w P_u r / (|d| sigma^2), Hessian sum +- w P_u (v_b - v_a) /
 * (|d| sigma)^2, P_u = I - u u^T, plus the scale row's w / sigma^2; Steihaug-Toint truncated CG preconditioned by the scalar per-node
 * Jacobi weight m_i = (2 sum w / (|d| sigma)^2 + 3 w_scale / sigma^2) / 3, the radius delta0 measured in that M-norm; the inner loop ends at
 * |r|_M^-1 <= kappa_cg |r0|_M^-1, on the boundary or after max_inner steps (0: three per node); accept at rho > 0.1, Delta / 4 under 0.25,
 * Delta * 2 above 0.75 on the boundary, rho regularised as in the rotation call. The outer loop ends when an accepted step lowers the cost
 * by at most rel_tol * f or abs_tol, at |g|_inf <= gradient_tol / sigma^2 (both CONVERGED), or after max_outer iterations. A row with
 * |x_b - x_a| = 0 at the point held gives NaN and the problem ends NON_FINITE. Sums run over a node's rows in ascending (neighbour, row)
 * order (a problem's rows: its pairs, then its measurements) and over the nodes by a fixed pairwise tree, so every byte is fixed by the
 * inputs: not by the lane count, the run, or the problem's place in a batch. The specification is
 * tests/translation_recovery_reference.py, operation for operation.
 * Batch: problem_row_off_dev [P + 1][2] int64 = (first pair row, first track) per problem (NULL with num_problems 1 and max_problem_tracks
 * = num_tracks: one problem over everything); one workgroup solves one problem.
 * PARITY UNPINNED towards the reference (nothing of gtsam was observed running): gtsam's Levenberg-Marquardt path and its seeded random
 * start (here a deterministic linear start); its soft prior on the first key (here a hard anchor); Unit3 and the 2-dimensional noise model
 * of the reference's gtsam version (here the 3-vector chordal residual with the same sigma); relative and absolute pose priors;
 * rig_1dsfm.py; the metrics group. The point returned is a critical point reached from the linear start: no local-minimum guarantee.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace (0 for sizes out of range: negative, 2^28 rows, 2^24 nodes, 2^28 nodes over all problems, max_problem_tracks >
 * num_tracks): about 105 per row and 300 per node and problem, nodes = num_images + max_problem_tracks. One workgroup solves one problem,
 * start to end, as in the rotation call: a call's time grows with rows x steps on ONE CU. */
size_t gtsfm_translation_recovery_workspace_bytes(long long num_pairs, long long num_meas, long long num_images, long long num_tracks,
                                                  long long max_problem_tracks, long long num_problems);

/* Outputs per problem, M = num_images + max_problem_tracks: translation_out_dev [P][M][3] (NaN outside the component), node_valid_dev [P][M]
 * uint8, counters_dev [P][8] int32 = status (0 CONVERGED, 1 MAX_ITERATIONS, 2 NO_VALID_ROW: all outputs NaN / 0, 3 NON_FINITE: outputs NaN,
 * mask 0), outer iterations, accepted steps, Hessian applications, initialisation CG steps, component size, anchor, valid rows; costs_dev
 * [P][4] float64 = the cost at the initialisation, the final cost, the final |g|_inf, the trust radius at exit. The call waits for the
 * stream once, for the two refusal flags; the inputs are not changed. */
int gtsfm_translation_recovery_f64(const int32_t* pair_images_dev, const double* world_pair_dev, const uint8_t* pair_enable_dev, long long num_pairs,
                                   const long long* track_off_dev, const int32_t* image_dev, const double* world_meas_dev, const uint8_t* meas_enable_dev,
                                   long long num_tracks, long long num_meas, int num_images, const long long* problem_row_off_dev, int num_problems,
                                   long long max_problem_tracks, int anchor, double scale_factor, double sigma, double huber_k, double init_tol,
                                   int init_max_iterations, double delta0, double kappa_cg, double gradient_tol, double rel_tol, double abs_tol, int max_outer,
                                   int max_inner, void* workspace_dev, size_t workspace_bytes, double* translation_out_dev, uint8_t* node_valid_dev,
                                   int32_t* counters_dev, double* costs_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Global bundle adjustment (float64)
 *   replaces gtsfm/bundle/bundle_adjustment.py (BundleAdjustmentOptimizer.run_ba: the factor graph, Levenberg-Marquardt and the
 *   reprojection-error filter of gtsfm/common/gtsfm_data.py), called from gtsfm/multi_view_optimizer.py:215-221 after the triangulation.
 * The inputs are the arrays gtsfm_triangulate_tracks_f64 reads and writes: cameras_dev [num_images][17] (valid, fx, fy, cx, cy, wRc
 * row-major, wtc), the track CSR (track_off_dev [T + 1], image_dev [S], uv_dev [S][2] float32), point_dev [T][3]; track_enable_dev [T] and
 * meas_enable_dev [S] uint8 (NULL: every one; in the chain exit_code == SUCCESS and the triangulation's inlier_mask). A measurement is VALID
 * when it is enabled, its camera id lies in the table with valid != 0 and its pixel is finite; a track when it is enabled, its point is
 * finite and it has at least min_track_length valid measurements; a measurement counts only in a valid track. A camera id outside the
 * table counts as not estimated, it is no refusal. Refused (GTSFM_ERR_INVALID, gtsfm_last_error, no output written): track or problem
 * offsets that are not ascending over their whole range, a problem with more than max_problem_tracks tracks.
 * Camera i is node i, track j of a problem whose first track is t0 is node num_images + (j - t0). The problem is the connected component
 * of `anchor` (a camera; -1: the smallest camera id with a valid measurement) over the valid measurements; every camera and point outside it
 * is copied through unchanged with node_valid 0. The cost is f = sum_m rho_k(|proj(cam_i, p_j) - uv_m| / measurement_sigma) with gtsam's
 * Huber on the norm (huber_k <= 0 or inf: the half square); a measurement whose point has depth <= 0 contributes zero residual and Jacobian.
 * Calibrations are held fixed, the anchor's pose is held fixed exactly, the scale is left to the damping. A pose moves by (R Cay(omega),
 * t + R v), a point by its 3-vector. Levenberg-Marquardt with the two-view call's scalar rules: lambda from 1e-5 by factors of 10 up to 1e5
 * (beyond: LAMBDA_BOUND), a trial accepted when its cost is finite, the model decrease positive and the gain ratio > 1e-3; CONVERGED when an
 * accepted step lowers the cost by less than abs_tol or relatively by less than rel_tol; at most max_iterations accepted steps. The linear
 * step: every point's damped 3 x 3 block eliminated, the reduced camera system applied matrix-free and solved by conjugate gradients
 * preconditioned by the cameras' damped 6 x 6 blocks, to |r| <= cg_forcing |r0|, r.M^-1 r <= 0 or max_inner iterations (0: six per camera); the points by
 * back-substitution; the model decrease of the step actually taken by one more pass. Sums run over a node's measurements in ascending
 * (neighbour, measurement) order and over the nodes by a fixed pairwise tree, so every byte is fixed by the inputs: not by the lane count,
 * the run, or the problem's place in a batch. The specification is tests/global_ba_reference.py, operation for operation.
 * Batch: problem_off_dev [P + 1] int64 over the tracks, from 0 to num_tracks (NULL with num_problems 1 and max_problem_tracks = num_tracks);
 * the problems share the camera table and each refines a copy of its own; one workgroup solves one problem.
 * PARITY UNPINNED towards the reference (nothing of gtsam was observed running): gtsam's Levenberg-Marquardt path, elimination ordering and
 * retraction; the Karcher-mean factor and the soft prior (sigma 0.1) in place of the hard anchor; calibration variables, their priors and
 * shared_calib; GNC / GMC / TLS; relative and absolute pose priors; the marginals check; select_largest_connected_component (here: the
 * anchor's component); the metrics group.
 * ---------------------------------------------------------------------------------------------------------- */

/* Bytes of device workspace (0 for sizes out of range: negative, 2^28 measurements, 2^24 nodes, 2^28 nodes over all problems,
 * max_problem_tracks > num_tracks): about 377 per measurement and 900 per node and problem, nodes = num_images + max_problem_tracks. One
 * workgroup solves one problem, start to end: a call's time grows with measurements x CG iterations on ONE CU. */
size_t gtsfm_global_ba_workspace_bytes(long long num_meas, long long num_images, long long num_tracks, long long max_problem_tracks, long long num_problems);

/* Outputs, M = num_images + max_problem_tracks: cameras_out_dev [P][num_images][17], point_out_dev [T][3], reproj_error_dev [S] (pixels at
 * the final values; NaN where the measurement is not a valid one of the problem or the point is behind the camera), track_valid_dev [T]
 * uint8 (in the problem and every valid measurement's error finite and < reproj_error_threshold), camera_kept_dev [P][num_images] uint8 (a
 * valid measurement in a kept track), node_valid_dev [P][M] uint8, counters_dev [P][8] int32 = status (0 CONVERGED, 1 MAX_ITERATIONS,
 * 2 NO_VALID_ROW, 3 NON_FINITE: a first cost that is NaN, 4 LAMBDA_BOUND; on 2 and 3 the outputs are the inputs and the masks zero), anchor,
 * cameras and points in the problem, valid measurements, accepted steps, linear solves tried, CG iterations; costs_dev [P][4] float64 = the
 * initial cost, the final cost, the final |g|_inf, the final lambda. The call waits for the stream once, for the two refusal flags; the
 * inputs are not changed. */
int gtsfm_global_ba_f64(const double* cameras_dev, int num_images, const long long* track_off_dev, const int32_t* image_dev, const float* uv_dev,
                        const double* point_dev, const uint8_t* track_enable_dev, const uint8_t* meas_enable_dev, long long num_tracks, long long num_meas,
                        const long long* problem_off_dev, int num_problems, long long max_problem_tracks, int anchor, int min_track_length,
                        double measurement_sigma, double huber_k, double reproj_error_threshold, double rel_tol, double abs_tol, double cg_forcing,
                        int max_iterations, int max_inner, void* workspace_dev, size_t workspace_bytes, double* cameras_out_dev, double* point_out_dev,
                        double* reproj_error_dev, uint8_t* track_valid_dev, uint8_t* camera_kept_dev, uint8_t* node_valid_dev, int32_t* counters_dev,
                        double* costs_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GTSFM_AMD_H */

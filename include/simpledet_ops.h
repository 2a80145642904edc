/*
 * simpledet_ops.h -- C ABI of libsimpledet_ops_hip.so: MI355X (gfx950) kernels for the
 * second-stage detection-ops hot path of tusen-ai/simpledet.
 *
 * This is the drop-in boundary.  The reference has no C ABI of its own: its operators are compiled
 * into libmxnet and reached by *operator name* (NNVM FCompute / legacy OperatorProperty), and its
 * only run-time extension hook is the Python mx.operator.CustomOp.  Each entry point below is what
 * a CustomOp (simpledet_amd/mxnet_plugin.py) or an FCompute<gpu> shim binds for one reference
 * operator; the comment above each names the reference interface it replaces (file:line relative to
 * the simpledet tree).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the name ends in _host
 *   - the caller owns every buffer (incl. workspaces: ask sd_*_workspace_bytes first); the library
 *     allocates nothing on the device and keeps no state between calls (the only process-wide
 *     state is the kernel-variant selection of sd_set_tuning, read lock-free at launch)
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on it; no entry
 *     point synchronises the device
 *   - all tensors are dense row-major ("C contiguous"), fp32 unless stated
 *   - `req` mirrors MXNet OpReqType: 0 = kNullOp, 1 = kWriteTo, 3 = kAddTo (kWriteInplace=2 is
 *     rejected exactly as the reference rejects it, roi_align_v2.cu:105-108)
 *   - return 0 on success, negative SD_ERR_* otherwise; sd_last_error() gives the message
 *     (thread local).  Nothing aborts or throws across this boundary.
 */
#ifndef SIMPLEDET_OPS_H_
#define SIMPLEDET_OPS_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_INVALID_ARG (-1)
#define SD_ERR_UNSUPPORTED (-2)
#define SD_ERR_HIP (-3)
#define SD_ERR_WORKSPACE (-4)

#define SD_REQ_NULL 0
#define SD_REQ_WRITE 1
#define SD_REQ_ADD 3

#define SD_MAX_FPN_LEVELS 8

const char* sd_last_error(void);
/* the kernels the calling thread's last fused-RoIAlign entry point launched, e.g.
 * "sd::roi_fwd_prep_kernel<7> + sd::roi_align_fwd_band<7,true,false> (tail tasks: 42 coordinate table + 90
 * backward plan)" (measurement tools label their numbers with the dispatch actually taken instead of
 * assuming one) */
const char* sd_last_dispatch(void);
/* ABI version of this header: bumped on any signature change AND on any change of a buffer layout
 * or size contract (a caller built against an older header must not pass it buffers of the old
 * size).  History: 1 round 1; 2 packed arg-max rows padded to whole dwords (7x7: 49 -> 52 bytes)
 * and 4-byte aligned; 3 sd_fpn_roi_align_workspace_bytes grew (the forward's band lists / tap
 * entries live in the workspace; with a smaller or NULL workspace the forward still runs, on the
 * slower tiled kernels); 4 sd_gemm_f32 computes products as three bf16 MFMA terms by default
 * (same signature, documented error model), sd_proposal_mask_target_ratio / sd_cast_* / *_f16 added;
 * 5 sd_gemm_f32_ws, the DCN products default to the scaled fp16 split (fp32-path accuracy), plain
 * sd_gemm_f32 to exact fp32; 8 sd_proposal and sd_proposal_v2 added (the existing entry points and
 * their workspace sizes are unchanged); 9 sd_hard_nms_batched and sd_bbox_post_processing added (nothing
 * existing changes); 10 sd_retina_anchor_target, sd_focal_loss_fwd / _bwd and sd_bbox_norm_bwd with their
 * workspace queries added (nothing existing changes); 11 sd_group_norm_fwd / _bwd and
 * sd_group_norm_workspace_bytes added (nothing existing changes); 12 sd_sigmoid_ce_fwd / _bwd and
 * sd_mask_loss_fwd / _bwd with their workspace queries added (nothing existing changes).  The
 * sd_quant_int8_* entry points were added at 12 as well: no existing signature, layout or size contract moved.
 * So were the sd_fcos_* entry points (FCOS targets and losses; sd_fcos_decode and sd_fcos_sigmoid, the test-time
 * decode): additions only.  So were sd_deform_psroi_pool_* and sd_fpn_deform_roi_pool_*, and
 * sd_msrcnn_mask_loss_* / sd_maskiou_loss_* (the Mask Scoring R-CNN training head), and sd_reppoints_decode (the
 * RepPoints test-time decode), and sd_crowdhuman_target / sd_emd_loss_* (the CrowdHuman double-prediction head),
 * and sd_scale_bias_act_* (the merged-BN affine and _contrib_BroadcastScale), and sd_rpn_loss_* / sd_rcnn_loss_*
 * (the Faster / Mask R-CNN loss heads), and sd_fpn_topdown_* (the FPN top-down pathway).
 * sd_abi_version() returns the library's value; compare with this macro. */
#define SD_ABI_VERSION 12
int sd_abi_version(void);
/* kernel-variant knobs for A/B measurements (bench.py, tests); every variant computes the same
 * result.  The knobs, their defaults and the ranges a read clamps to are the rows of ONE list, SD_KNOBS in
 * simpledet_amd/csrc/common.h; nothing else states a default.  A knob holds its default until sd_set_tuning
 * changes it (any integer is accepted), sd_get_tuning returns the value it holds, and sd_tuning_key(index) names
 * row `index` (NULL past the last row), so a caller can list the knobs and put back what it changed.  Unknown
 * keys are an error.  Knobs that disable parts of a kernel for profiling are rows only in the separate
 * -DSD_PROFILING build used by tools/, not in this library. */
int sd_set_tuning(const char* key, int value);
int sd_get_tuning(const char* key, int* value);
const char* sd_tuning_key(int index);

/* Block the calling host thread until `stream` has drained.  Only the MXNet CustomOp adapter
 * uses it (a CustomOp's outputs must be complete when forward()/backward() returns); the compute
 * entry points never synchronise. */
int sd_stream_synchronize(void* stream);

/* HBM streaming copy (measurement aid, no reference counterpart): dst[i] = src[i] with
 * width_bytes (4, 8 or 16) per lane.  bench.py uses it to report the achievable HBM rate next to
 * the 8 TB/s spec peak and to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE on a known byte count */
int sd_hbm_stream_copy(const void* src, void* dst, size_t bytes, int width_bytes, void* stream);

/* fp16 <-> fp32 streaming casts (X.to_fp32 / X.to_fp16 of the reference's fp16 graphs, where an op
 * boundary still needs them: the fp16 form of the RoIAlign backward).  n elements; dst of the
 * second honours req (write / add, the sum formed in fp32).  16-byte aligned buffers for the first. */
int sd_cast_f16_to_f32(const void* src, float* dst, size_t n, void* stream);
int sd_cast_f32_to_f16(const float* src, void* dst, size_t n, int req, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ROIAlign_v2  (mx.sym.contrib.ROIAlign_v2, registered as _contrib_ROIAlign_v2)
 *   replaces ROIAlignForward_v2<gpu>  operator_cxx/contrib/roi_align_v2-inl.h:157-195
 *            (kernel ROIAlignForwardKernel_v2::Map :61-153; shapes roi_align_v2.cc:187-208)
 *   data (B,C,H,W)  rois (B,R,4) [x1,y1,x2,y2] image coords, batch index = roi / R
 *   out, maxidx_x, maxidx_y (B,R,C,ph,pw)
 * ---------------------------------------------------------------------------------------------- */
int sd_roi_align_v2_fwd(const float* data, const float* rois, float* out, float* maxidx_x,
                        float* maxidx_y, int B, int C, int H, int W, int R, int pooled_h,
                        int pooled_w, float spatial_scale, void* stream);

/* The same with DEVICE scratch of sd_roi_align_v2_workspace_bytes(B, R) bytes: the forward then runs
 * on the band-resident kernel (feature planes streamed through LDS once, no per-RoI gathers; same
 * bits).  workspace may be NULL (= the call above, the tiled kernels). */
size_t sd_roi_align_v2_workspace_bytes(int B, int R);
int sd_roi_align_v2_fwd_ws(const float* data, const float* rois, float* out, float* maxidx_x,
                           float* maxidx_y, int B, int C, int H, int W, int R, int pooled_h,
                           int pooled_w, float spatial_scale, void* workspace, size_t workspace_bytes,
                           void* stream);

/*   replaces ROIAlignBackward_v2<gpu>  operator_cxx/contrib/roi_align_v2.cu:87-143
 *            (kernel ROIAlignBackwardKernelGPU_v2::Map :35-84; inputs per ROIAlignGrad_v2
 *            roi_align_v2-inl.h:206-218: [dY, rois, maxidx_x, maxidx_y] -> [dX, d_rois])
 *   d_data (B,C,H,W) honours req_data (write = zero first, add = accumulate);
 *   d_rois (B,R,4) is zero-filled when req_rois == write (may be NULL when req_rois == null). */
int sd_roi_align_v2_bwd(const float* out_grad, const float* rois, const float* maxidx_x,
                        const float* maxidx_y, float* d_data, float* d_rois, int req_data,
                        int req_rois, int B, int C, int H, int W, int R, int pooled_h, int pooled_w,
                        float spatial_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused FPN RoI feature extraction = FPNRoiAlign.get_roi_feature, models/FPN/builder.py:567-610:
 *   fpn_roi_assign (models/FPN/assign_layer_fpn.py:17-41) -> one ROIAlign_v2 per level on the
 *   zero-masked RoIs -> add_n.  One launch reads every level once and writes ONE output
 *   (the reference writes 4 x 3 full-size tensors and adds them).
 *   feats_host: host array of nlvl device pointers, level l is (B,C,Hs[l],Ws[l]), spatial_scale
 *   1/strides[l].  maxidx_x/y hold the argmax of each RoI's assigned level (-1 elsewhere).
 * ---------------------------------------------------------------------------------------------- */
int sd_fpn_roi_align_fwd(const float* const* feats_host, const int* Hs_host, const int* Ws_host,
                         const int* strides_host, int nlvl, const float* rois, float* out,
                         float* maxidx_x, float* maxidx_y, int B, int C, int R, int pooled_h,
                         int pooled_w, float roi_canonical_scale, float roi_canonical_level,
                         void* workspace, size_t workspace_bytes, void* stream);
/* DEVICE scratch for the forward: the band-resident kernel (the default: planes streamed through
 * LDS once, no per-RoI gathers) keeps its per-band item lists and per-RoI tap entries there; with
 * workspace == NULL (or too small) the forward runs on the tiled kernels instead -- same bits */
size_t sd_fpn_roi_align_workspace_bytes(int B, int R);
int sd_fpn_roi_align_bwd(const float* out_grad, const float* rois, const float* maxidx_x,
                         const float* maxidx_y, float* const* d_feats_host, const int* Hs_host,
                         const int* Ws_host, const int* strides_host, int nlvl, int req_data, int B,
                         int C, int R, int pooled_h, int pooled_w, float roi_canonical_scale,
                         float roi_canonical_level, void* stream);
/* The same fused op with the arg-max kept as ONE byte per output (row sample * 3 + column sample,
 * 255 = nothing pooled) plus a small per-RoI table (coords: B*R x 9*(pooled_h+pooled_w) 4-byte
 * words, 516 KB at the baseline; per RoI: 3*(ph+pw) fp32 sample coordinates, then 3*(ph+pw) pairs
 * {clamped neighbours lo | hi << 16, interpolation fraction} derived from them with the backward's
 * own expressions) instead of two fp32 planes: the arg-max is state between this op's own forward
 * and backward, not part of the reference's graph interface.  The backward looks the pair up, i.e.
 * uses exactly the values the float planes would have produced, without floor / clamp / divide
 * per gradient element.  Cuts the forward's writes from 3 to 1.25 planes and the backward's reads
 * likewise (7x7 and 14x14 pooling).  coords must be 8-byte aligned.
 * argmax layout: (B, R, C, sd_fpn_roi_align_argmax_stride(ph, pw)) bytes -- every (RoI, channel)
 * row of ph*pw codes is padded to whole 4-byte words (7x7: 52, 14x14: 196) so that the backward
 * fetches four codes with one aligned load; the padding bytes are never read as codes.  argmax
 * must be 4-byte aligned. */
int sd_fpn_roi_align_argmax_stride(int pooled_h, int pooled_w);
int sd_fpn_roi_align_fwd_packed(const float* const* feats_host, const int* Hs_host,
                                const int* Ws_host, const int* strides_host, int nlvl,
                                const float* rois, float* out, uint8_t* argmax, float* coords, int B,
                                int C, int R, int pooled_h, int pooled_w, float roi_canonical_scale,
                                float roi_canonical_level, void* workspace, size_t workspace_bytes,
                                void* stream);
/* fp16 I/O variant for fp16 graphs (the reference casts to fp32 around the op, models/FPN/builder.py:
 * 581-586, 607-608): feats are fp16 (B,C,H,W), out is fp16 (B,R,C,ph,pw); the arithmetic is the fp32
 * arithmetic of the op above (taps converted exactly, the maximum rounded to nearest even), i.e.
 * bit-equal to to_fp32 -> sd_fpn_roi_align_fwd_packed -> to_fp16 without the two cast passes and with
 * half the feature traffic.  argmax / coords / workspace as above; the workspace is REQUIRED (the fp16
 * path exists on the band-resident kernel only), feats must be 16-byte aligned. */
int sd_fpn_roi_align_fwd_packed_f16(const void* const* feats_host, const int* Hs_host,
                                    const int* Ws_host, const int* strides_host, int nlvl,
                                    const float* rois, void* out, uint8_t* argmax, float* coords, int B,
                                    int C, int R, int pooled_h, int pooled_w, float roi_canonical_scale,
                                    float roi_canonical_level, void* workspace, size_t workspace_bytes,
                                    void* stream);
int sd_fpn_roi_align_bwd_packed(const float* out_grad, const float* rois, const uint8_t* argmax,
                                const float* coords, float* const* d_feats_host, const int* Hs_host, const int* Ws_host,
                                const int* strides_host, int nlvl, int req_data, int B, int C, int R,
                                int pooled_h, int pooled_w, float roi_canonical_scale,
                                float roi_canonical_level, void* stream);
/* Numerics of the packed backward (and of the drop-in sd_roi_align_v2_bwd / sd_fpn_roi_align_bwd in
 * their default form).  Every tap value is computed in fp32 exactly as the reference does; the SUM a
 * pixel receives is accumulated in 32-bit fixed point whose unit is fixed per workgroup (one band of
 * one channel): 2^-30 .. 2^-29 of (max|dY| of the band) x (a bound on the weight one pixel can collect).  With
 * a workspace the bound is per PIXEL of the band (round 6: a 2-D difference array of the RoIs' footprints in the
 * list pre-pass, typically 20-100), without one it is summed over the band's RoIs (1,000-1,800 at the baseline).
 * The result is independent of the order of the adds (bit-reproducible; the reference's float atomics are not).
 *   Measured against the oracle (tests/test_fixed_point_precision.py, profiles/r06e_fixed_point_precision.json):
 * dY ~ N(0,1) at BASELINE's size: 1.1e-5 max abs error with the per-pixel bound (2.3e-5 with the summed bound,
 * 3.8e-6 for fp32 adds in hardware order; bar 1e-4).
 *   A fixed-point unit is ABSOLUTE for its band, so it is only used while the band's gradients span a range
 * it resolves (round 6): behind the scatter a workgroup compares the exponent of its largest |dY| plus the bits
 * of its weight bound with the MEAN exponent of its non-zero gradients (a quarter of them, sampled at fixed
 * positions; all-integer, so the verdict does not depend on any order) and keeps the integer sums only if
 *     E(max|dY|) + ceil(log2(weight bound)) <= mean E(dY) + 15,
 * i.e. the unit is below ~2^-13 of the gradients' geometric mean.  Near-Gaussian gradients pass with 4-9 bits to
 * spare (a loss scale cancels out); heavy-tailed ones -- dY = N(0,1) x lognormal(sigma = 3) x 128: until round 6
 * 39 % of the elements were off by more than 1e-4 relative, the median small element by 0.8 % -- make the
 * workgroup clear its band and sum it again with fp32 compare-and-swap adds, the reference's own arithmetic
 * (roi_align_v2.cu:67-83): then 9e-7 of the elements differ from the oracle by more than 1e-4 max(1, |want|), the
 * same as for the float adds alone (two float summation orders differ where a pixel's addends cancel), and
 * |err| <= 1e-4 max(median|dY|, sum of the pixel's |addends|) holds everywhere.  Non-finite dY (inf AND NaN:
 * the maximum is taken over bit patterns) and weight bounds above 2048 take the float adds as well.  Callers
 * that want fp32 adds in every workgroup select them with
 *     sd_set_tuning("roi_align_bwd_fx", 0)
 * (packed arg-max and float arg-max planes alike) at ~1.2-1.5 x the time; the sums then depend on the order
 * in which the hardware serves the adds, like the reference's.
 *   sd_roi_align_v2_bwd on a single map with C % 4 == 0 whose four planes fit 72 KB of LDS (the C4
 * family; square 7x7 / 14x14 pools) runs roi_align_bwd_flt4_kernel (four whole planes per workgroup), which sums
 * the same way, scaled by max|dY| of the workgroup x a per-pixel weight bound taken from
 * the RoIs' footprints (so `rois` must be the boxes the arg-max planes were produced with, as they are
 * in the operator): bit-reproducible, 4.9e-5 from the exact sums for dY ~ N(0,1) at the full C4 shape
 * (2,1024,50,84) x 512 RoIs; the same verdict, the same fall-backs and the same
 * sd_set_tuning("roi_align_bwd_fx", 0) as above.  sd_set_tuning("roi_align_bwd_flt4", 0) selects the banded
 * kernel there. */
/* The same with a device workspace of sd_fpn_roi_align_bwd_workspace_bytes(): the per-band RoI
 * lists are then built by one small pre-pass instead of by every channel's workgroup (same
 * results bit for bit).  workspace may be NULL (= the call above). */
size_t sd_fpn_roi_align_bwd_workspace_bytes(const int* Hs_host, const int* Ws_host, int nlvl, int B, int R);
int sd_fpn_roi_align_bwd_packed_ws(const float* out_grad, const float* rois, const uint8_t* argmax,
                                   const float* coords, float* const* d_feats_host, const int* Hs_host,
                                   const int* Ws_host, const int* strides_host, int nlvl, int req_data, int B,
                                   int C, int R, int pooled_h, int pooled_w, float roi_canonical_scale,
                                   float roi_canonical_level, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* fp16 gradient in, fp16 feature gradients out (the backward of sd_fpn_roi_align_fwd_packed_f16): the
 * sums are formed exactly as in the fp32 call -- fp32 tap values, fixed-point / fp32 accumulation --
 * only the two conversions of the graph's to_fp32 / to_fp16 casts (models/FPN/builder.py:581-586,
 * 607-608) happen inside the kernel: bit-equal to cast -> sd_fpn_roi_align_bwd_packed_ws -> cast with
 * req (write / add, the sum formed in fp32).  d_feats 8-byte aligned.  SD_ERR_UNSUPPORTED where the
 * default wide kernel does not apply (callers then use the casts). */
int sd_fpn_roi_align_bwd_packed_f16(const void* out_grad, const float* rois, const uint8_t* argmax,
                                    const float* coords, void* const* d_feats_host, const int* Hs_host,
                                    const int* Ws_host, const int* strides_host, int nlvl, int req_data,
                                    int B, int C, int R, int pooled_h, int pooled_w,
                                    float roi_canonical_scale, float roi_canonical_level, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* ONE rois-only pre-pass per training step.  Both pre-passes of the fused extractor -- the forward's
 * item lists / tap entries / coordinate table and the backward's band lists / tap tables -- are pure
 * functions of `rois` and the level geometry.  With a `plan` buffer of sd_fpn_roi_align_plan_bytes()
 * (16-byte aligned, op state between forward and backward like argmax / coords; ~9 MB at the
 * baseline) the forward builds both in its own two launches -- what its main kernel reads in the pre-pass
 * launch, the rest (coordinate table, the backward's tables) in the main kernel's tail; knob
 * roi_align_plan_tail = 0: all of it in the pre-pass launch -- and the backward launches its main
 * kernel only: 3 launches per step instead of 4.  Same bits as the _ws pair.  The plan is valid for the
 * shapes, rois and tuning knobs of the forward that filled it; where the band / tap-table form does
 * not apply (knob roi_align_bwd_lists != 1, a level that does not fit) both calls fall back to the
 * behaviour of the unplanned pair by the same deterministic decision.
 *   replaces the same reference code as sd_fpn_roi_align_fwd_packed / _bwd_packed
 *   (models/FPN/builder.py:567-610; roi_align_v2-inl.h:61-195, roi_align_v2.cu:35-143) */
size_t sd_fpn_roi_align_plan_bytes(const int* Hs_host, const int* Ws_host, int nlvl, int B, int R);
int sd_fpn_roi_align_fwd_packed_plan(const float* const* feats_host, const int* Hs_host, const int* Ws_host,
                                     const int* strides_host, int nlvl, const float* rois, float* out,
                                     uint8_t* argmax, float* coords, int B, int C, int R, int pooled_h,
                                     int pooled_w, float roi_canonical_scale, float roi_canonical_level,
                                     void* workspace, size_t workspace_bytes, void* plan, size_t plan_bytes,
                                     void* stream);
int sd_fpn_roi_align_bwd_packed_plan(const float* out_grad, const float* rois, const uint8_t* argmax,
                                     const float* coords, float* const* d_feats_host, const int* Hs_host,
                                     const int* Ws_host, const int* strides_host, int nlvl, int req_data,
                                     int B, int C, int R, int pooled_h, int pooled_w,
                                     float roi_canonical_scale, float roi_canonical_level, const void* plan,
                                     size_t plan_bytes, void* stream);
/* How the band forward staffs its virtual units with whole workgroups (knob roi_align_fwd_staff = 1): unit v has
 * n[v] channel reservations of t[v] cost units each; m_out[v] = workgroups that start on it, sum = nwg.  The smallest
 * T with sum_v ceil(n[v] / floor((T - setup) / t[v])) <= nwg gives m; workgroups left over go one at a time to the
 * unit that then finishes last (all of them at once when that unit already has a workgroup per reservation).
 * m_out is all zero where the rule does not apply (nvu > nwg, no work, products past 2^30): the kernel then keeps
 * the midpoint rule.  _ref runs on the host (host pointers), _dev runs the kernel's own form in one wave (device
 * pointers); both exist for the tests. */
int sd_band_staffing_ref(const int* n, const int* t, int nvu, int nwg, int setup, int* m_out);
int sd_band_staffing_dev(const int* n, const int* t, int nvu, int nwg, int setup, int* m_out, void* stream);
/* assign_layer_fpn CustomOp (models/FPN/assign_layer_fpn.py:10-73): rois (n_rois,4) ->
 * rois_per_level (nlvl, n_rois, 4) zero-masked, and optionally level (n_rois) int32 (-1 = none).
 * The rule is floor(level0 + log2(sqrt(area) / scale0 + 1e-6)) in float32.  A few arguments just under a power of
 * two make level0 + log2 an exact tie, so that the last bit of log2 picks the level (default pyramid: z = 2 - 3 ulp
 * and z = 0.5 - 1 / - 3 ulp).  There the spec is the correctly rounded log2f: the CPU oracle's (glibc) and the
 * fixture's (tests/golden/fpn_assign_thresholds.npz, the reference's Python class on numpy); the reference's own
 * CPU and CUDA log2 need not agree with each other at those arguments.  Strides are powers of two: with another
 * stride the reference feeds a non-integer k_min through 2 ** t and astype('uint8'); no config does, and nothing
 * here defines or tests it. */
int sd_fpn_roi_assign(const float* rois, int n_rois, const int* strides_host, int nlvl,
                      float roi_canonical_scale, float roi_canonical_level, float* rois_per_level,
                      int32_t* level, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ROIPooling_v1  (mx.sym.ROIPooling_v1)
 *   replaces ROIPoolForward (GPU)  operator_cxx/roi_pooling_v1.cu:48-113 / ROIPoolForward_v1 (CPU)
 *            roi_pooling_v1.cc:39-126, op wrapper roi_pooling_v1-inl.h:70-94
 *   data (B,C,H,W)  rois (K,5) [batch_index,x1,y1,x2,y2]  out, maxidx (K,C,ph,pw)
 *   maxidx holds the flat argmax h*W+w as a float, -1 for an empty bin.
 * ---------------------------------------------------------------------------------------------- */
int sd_roi_pool_v1_fwd(const float* data, const float* rois, float* out, float* maxidx, int B,
                       int C, int H, int W, int K, int pooled_h, int pooled_w, float spatial_scale,
                       void* stream);
/*   replaces ROIPoolBackward  roi_pooling_v1.cu:115-152, wrapper roi_pooling_v1-inl.h:96-133
 *   (d_data honours req_data: write = zero first, add = accumulate; d_rois zeroed on write) */
int sd_roi_pool_v1_bwd(const float* out_grad, const float* rois, const float* maxidx,
                       float* d_data, float* d_rois, int req_data, int req_rois, int B, int C,
                       int H, int W, int K, int pooled_h, int pooled_w, float spatial_scale,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_DeformablePSROIPooling  (mx.sym.contrib.DeformablePSROIPooling, upstream MXNet; the reference
 *   calls it from models/TSD/poolings.py:87-100, 151-164).  The arithmetic is restated in DESIGN.md 4.15.
 *   data (B,C,H,W), C == output_dim * group_size^2;  rois (K,5) [batch, x1, y1, x2, y2];
 *   trans (K, 2*num_classes, part, part), not read when no_trans (num_classes is then taken as 1);
 *   part_size 0 means pooled_size.  out, top_count (K, output_dim, pooled, pooled); top_count holds the
 *   number of samples each output kept (0: the output is 0) and is the backward's state.
 *   A batch index outside [0, B) pools nothing.  All arithmetic fp32.
 *   The tap table of a RoI and the backward's per-wave d_trans sums live in LDS.  ONE predicate,
 *   sd_deform_psroi_pool_supported(num_classes, pooled_size, sample_per_part) (1 / 0; num_classes = 1 when
 *   no_trans), names the sets all four entry points below take -- forward and backward alike; every other set
 *   is SD_ERR_UNSUPPORTED in each of them.  It holds when U = num_classes * pooled^2 and NT = U * sample_per_part^2
 *   satisfy NT <= 4096 and 4 * (3 NT + 8 U + 8) <= 65536 bytes (e.g. 7 x 7 x 16 with up to 5 classes, 14 x 14 x 16;
 *   not 32 x 32 x 4).  sd_set_tuning("deform_psroi_bwd_patch", 0) makes the backward add every tap to memory directly.
 * ---------------------------------------------------------------------------------------------- */
int sd_deform_psroi_pool_supported(int num_classes, int pooled_size, int sample_per_part);
int sd_deform_psroi_pool_fwd(const float* data, const float* rois, const float* trans, float* out,
                             float* top_count, int B, int C, int H, int W, int K, int num_classes,
                             float spatial_scale, int output_dim, int group_size, int pooled_size,
                             int part_size, int sample_per_part, float trans_std, int no_trans, void* stream);
/*   d_data (B,C,H,W) and d_trans (shape of trans) honour their req (write / add / null); d_rois (K,5) is
 *   zero-filled on write and untouched otherwise.  d_trans is bit-reproducible (fixed summation order);
 *   d_data is summed with global float atomics and depends on the order the hardware serves them in. */
int sd_deform_psroi_pool_bwd(const float* out_grad, const float* data, const float* rois, const float* trans,
                             const float* top_count, float* d_data, float* d_rois, float* d_trans, int req_data,
                             int req_rois, int req_trans, int B, int C, int H, int W, int K, int num_classes,
                             float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                             int sample_per_part, float trans_std, int no_trans, void* stream);
/* Fused TSD extractor = FPNRoIAlign_DeltaC / FPNRoIAlign_DeltaR.get_roi_feature, models/TSD/poolings.py:51-174:
 *   fpn_roi_assign_offset (:12-47) -> one DeformablePSROIPooling per level on the masked RoIs and offsets
 *   (group_size 1, output_dim == C, one class, part_size == pooled_size) -> add_n, as ONE launch.
 *   feats_host / Hs / Ws / strides as in sd_fpn_roi_align_fwd, nlvl <= 5;  rois (B,R,4);
 *   trans (B*R, 2, trans_part, trans_part), trans_part == pooled_size (DeltaC) or 1 (DeltaR: the
 *   reference tiles a (B*R,2) offset over the bins; here it is read with stride 0);
 *   out (B*R, C, pooled, pooled);  top_count (B*R, nlvl, pooled, pooled): the samples level l kept for a
 *   bin -- channel-independent, so stored once per (RoI, level, bin).
 *   A level a RoI is NOT assigned to pools the RoI (-1,-1,-1,-1) with zero offsets, as the reference's masks
 *   make it; where that keeps samples (levels with 1/stride < 0.1) they are pooled and summed like the
 *   reference does, and the backward returns their gradient to the same pixels.  d_trans receives the
 *   assigned level's terms only. */
int sd_fpn_deform_roi_pool_fwd(const float* const* feats_host, const int* Hs_host, const int* Ws_host,
                               const int* strides_host, int nlvl, const float* rois, const float* trans,
                               float* out, float* top_count, int B, int C, int R, int pooled_size,
                               int trans_part, int sample_per_part, float trans_std,
                               float roi_canonical_scale, float roi_canonical_level, void* stream);
int sd_fpn_deform_roi_pool_bwd(const float* out_grad, const float* const* feats_host,
                               float* const* d_feats_host, const int* Hs_host, const int* Ws_host,
                               const int* strides_host, int nlvl, const float* rois, const float* trans,
                               const float* top_count, float* d_trans, int req_data, int req_trans, int B,
                               int C, int R, int pooled_size, int trans_part, int sample_per_part,
                               float trans_std, float roi_canonical_scale, float roi_canonical_level,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_GenAnchor  (mx.sym.contrib.GenAnchor)
 *   replaces GenAnchorGPUOp::Forward  operator_cxx/contrib/generate_anchor.cu:97-153
 *            (base anchors generate_anchor-inl.h:140-181 in double on the host, grid kernel :61-81)
 *   out (H*W*A, 4) fp32, A = n_ratios*n_scales (ratio-major), row (h*W + w)*A + a.
 *   The same grid with H = W = max_side/stride is symbol/builder.py:904-938 add_anchor_to_arg.
 * ---------------------------------------------------------------------------------------------- */
int sd_gen_anchor(float* out, int H, int W, int feature_stride, const double* scales_host,
                  int n_scales, const double* ratios_host, int n_ratios, void* stream);
/* the same for every pyramid level in ONE launch (the reference runs one GenAnchor node per level,
 * models/FPN/builder.py; five 2.7 us kernels are launch bound): outs_host[l] = device buffer of
 * level l (Hs[l] * Ws[l] * A rows), same scales / ratios on every level, its own stride */
int sd_gen_anchor_levels(float* const* outs_host, const int* Hs_host, const int* Ws_host,
                         const int* strides_host, int nlvl, const double* scales_host, int n_scales,
                         const double* ratios_host, int n_ratios, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ProposalTarget  (mx.sym.ProposalTarget)
 *   replaces ProposalTargetOp::Forward  operator_cxx/proposal_target-inl.h:123-256 and SampleROI
 *            operator_cxx/proposal_target.cc:21-227 -- which copy to the host and run single
 *            threaded; here everything stays on the device.
 *   rois (B,N,4)  gt_boxes (B,M,5) [x1,y1,x2,y2,cls], cls == -1 padding
 *   roi_output (B,S,4)  label (B,S)  bbox_target, bbox_weight (B,S,4*num_classes)
 *   match_gt_iou (B,S)   (S = image_rois; all outputs are written, kWriteTo semantics)
 *   kept_index (B,S) int32, optional (may be NULL): index into the image's candidate list
 *   [rois with y2 > 0 in order, then the valid gt boxes] of every output row, -1 = unfilled.
 *   rng_state: DEVICE array of 33 int32 = glibc rand() TYPE_3 state (31-word ring, front index,
 *   rear index); advanced in place exactly as the reference advances libc's global state through
 *   std::random_shuffle.  Fill a host copy with sd_glibc_srand_host (seed 1 == never-seeded libc).
 *   workspace: DEVICE scratch of sd_proposal_target_workspace_bytes(B, N, M) bytes.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int num_classes, batch_images, image_rois;
  float fg_fraction, fg_thresh, bg_thresh_hi, bg_thresh_lo;
  int proposal_without_gt, class_agnostic;
  float bbox_mean[4], bbox_std[4], bbox_weight[4];
} sd_proposal_target_param;
#define SD_GLIBC_RAND_STATE_WORDS 33
int sd_glibc_srand_host(uint32_t seed, int32_t* state_host);
size_t sd_proposal_target_workspace_bytes(int B, int N, int M);
int sd_proposal_target(const float* rois, const float* gt_boxes, int N, int M,
                       const sd_proposal_target_param* param_host, int32_t* rng_state,
                       float* roi_output, float* label, float* bbox_target, float* bbox_weight,
                       float* match_gt_iou, int32_t* kept_index, void* workspace,
                       size_t workspace_bytes, void* stream);
/* ProposalTarget_v2 (mx.sym.ProposalTarget_v2, call site models/tridentnet/builder.py:281-299)
 *   replaces ProposalTargetOp_v2::Forward  operator_cxx/proposal_target_v2-inl.h:128-296 and
 *   proposal_target_v2::SampleROI  operator_cxx/proposal_target_v2.cc:21-177
 *   = ProposalTarget plus valid_ranges (B,2) DEVICE [min, max] object scale per image: with
 *   filter_scales a gt box is appended to the candidate rois only if min^2 <= w*h <= max^2; an
 *   image without candidates / without valid gt gets one all-zero roi / gt row.  image_rois = -1
 *   is rejected (the reference allocates (B,-1,.) tensors for it).  The `ohem` parameter of the
 *   reference is LOG(FATAL) "not implemented" there and has no counterpart here. */
/* ProposalMaskTarget (mx.sym.ProposalMaskTarget, call sites models/maskrcnn/builder.py:115,184,
 * models/tridentnet/builder.py:377,437)
 *   replaces ProposalMaskTargetOp::Forward  operator_cxx/proposal_mask_target-inl.h:141-330,
 *   SampleROIMask proposal_mask_target.cc:218-378 and convertPoly2Mask :148-216 (over rleFrPoly /
 *   rleDecode of the un-vendored COCO mask API)
 *   = the ProposalTarget_v2 sampling (valid_ranges may be NULL: num_args = 3) plus
 *   gt_polys (B,M,L) DEVICE, per gt box [category, n_seg, len_1..len_n, x,y,x,y,...] padded with -1
 *   mask_target (B, FG, mask_size, mask_size), FG = (int)(image_rois * fg_fraction): rows of the
 *   sampled foreground RoIs hold the 0/1 mask of their gt polygon in the RoI's frame, the rest -1.
 *   output_ratio = false; the _ratio entry below is output_ratio = true. */
int sd_proposal_mask_target(const float* rois, const float* gt_boxes, const float* gt_polys,
                            const float* valid_ranges, int filter_scales, int N, int M, int L,
                            int mask_size, const sd_proposal_target_param* param_host,
                            int32_t* rng_state, float* roi_output, float* label, float* bbox_target,
                            float* bbox_weight, float* match_gt_iou, float* mask_target,
                            int32_t* kept_index, void* workspace, size_t workspace_bytes,
                            void* stream);
/* ProposalMaskTarget with output_ratio = true (mask scoring R-CNN, models/msrcnn/builder.py:219-237)
 *   replaces convertPoly2MaskWithRatio  operator_cxx/proposal_mask_target.cc:20-152 (called :368-372)
 *   and the seventh output of ProposalMaskTargetOp  proposal_mask_target-inl.h:244,333-336,453-456
 *   mask_ratio (B, FG): for the sampled foreground rows, the pixels of the gt polygon inside the RoI
 *   (rasterised at image resolution, RoI corners truncated to int) over its pixels inside the
 *   bounding box of RoI and polygon, max(crop / (full + 1e-4), 1e-10); 0 for the other rows.  The
 *   mask itself is computed with the double coordinates of that function (:53-63) -- it can differ
 *   from output_ratio = false in a rounding case, as in the reference.
 *   max_raster_pixels bounds crop_h * crop_w and full_h * full_w (the image area suffices when RoIs
 *   and polygons lie inside the image); a row whose raster is larger gets NaN.
 *   workspace: sd_proposal_mask_target_ratio_workspace_bytes(B, N, M, image_rois, fg_fraction,
 *   max_raster_pixels) bytes (two bitmaps of max_raster_pixels bits per foreground row). */
size_t sd_proposal_mask_target_ratio_workspace_bytes(int B, int N, int M, int image_rois,
                                                     float fg_fraction, int max_raster_pixels);
int sd_proposal_mask_target_ratio(const float* rois, const float* gt_boxes, const float* gt_polys,
                                  const float* valid_ranges, int filter_scales, int N, int M, int L,
                                  int mask_size, const sd_proposal_target_param* param_host,
                                  int32_t* rng_state, float* roi_output, float* label,
                                  float* bbox_target, float* bbox_weight, float* match_gt_iou,
                                  float* mask_target, float* mask_ratio, int max_raster_pixels,
                                  int32_t* kept_index, void* workspace, size_t workspace_bytes,
                                  void* stream);
int sd_proposal_target_v2(const float* rois, const float* gt_boxes, const float* valid_ranges,
                          int filter_scales, int N, int M,
                          const sd_proposal_target_param* param_host, int32_t* rng_state,
                          float* roi_output, float* label, float* bbox_target, float* bbox_weight,
                          float* match_gt_iou, int32_t* kept_index, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_NMS  (mx.sym.contrib.NMS; the same kernel is embedded in Proposal_v3)
 *   replaces NMSGPUOp::Forward  operator_cxx/contrib/nms.cu:249-365 (nms_kernel :102-147, host
 *            scan _nms :149-202 with its D2H/H2D copies, PrepareOutput :207-233)
 *   dets (B,N,5) [x1,y1,x2,y2,score].  pre = pre_nms_top_n > 0 ? min(pre_nms_top_n, N) : N,
 *   post = min(post_nms_top_n, pre).  out (B,post,4), score (B,post): kept boxes in score order,
 *   zero padded.  keep_index (B,post) int32 optional: original row of every kept box, -1 pad.
 *   threshold_ge = 0: suppress IoU > threshold (nms.cu:140); 1: IoU >= threshold
 *   (proposal_v3.cu:319).  The sort is stable (ties keep the lower input row first).
 *   Sizes: pre <= 16384 (one LDS sort; the bit matrix is pre^2 / 8 bytes).  N itself is free
 *   (< 2^24): with more than 16384 unsorted rows the pre best are picked by a radix select and
 *   only they are sorted -- the rows nms.cu:311-313 keeps of its full sort (:303).
 *   workspace: DEVICE scratch of sd_nms_workspace_bytes(B, N, pre_nms_top_n) bytes.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_nms_workspace_bytes(int B, int N, int pre_nms_top_n);
int sd_nms(const float* dets, int B, int N, int pre_nms_top_n, int post_nms_top_n, float threshold,
           int threshold_ge, int already_sorted, float* out, float* score, int32_t* keep_index,
           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * soft_nms, batched  (operator_py/cython/cpu_nms.pyx:98-203 through operator_py/nms.py:5-16; the
 *   reference runs one Python-object loop per (image, class) in a process pool,
 *   detection_test.py:233-267)
 *   dets (P,Nmax,5): problem p uses rows [0, counts[p]).  method 0 hard, 1 linear, 2 gaussian.
 *   out_dets (P,Nmax,5) / out_inds (P,Nmax): the surviving boxes with their decayed scores and
 *   their input rows, in selection order; out_counts (P).  Rows past out_counts[p] are unspecified.
 * ---------------------------------------------------------------------------------------------- */
int sd_soft_nms_batched(const float* dets, const int32_t* counts, int P, int Nmax, float sigma,
                        float Nt, float threshold, int method, float* out_dets, int32_t* out_inds,
                        int32_t* out_counts, void* stream);
/* bbox_overlaps_cython  (operator_py/cython/bbox.pyx:31-72): overlaps (n,k) */
int sd_bbox_overlaps(const float* boxes, int n, const float* query_boxes, int k, float* overlaps,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * RPN anchor-target assignment -- SURVEY 8(f) rank 3.  The reference computes it on the host in its
 * data loader:
 *   replaces AnchorTarget2D.apply  core/detection_input.py:535-565 (anchors :373-437, label
 *            assignment :450-482, random subsampling :484-499, box encoding :501-510, valid-anchor
 *            gather / scatter :512-533) and PyramidAnchorTarget2D.apply  models/FPN/input.py:101-146,
 *            IoU operator_py/cython/bbox.pyx:31-72, encoding operator_py/bbox_transform.py:52-77
 *   im_info (B,3) DEVICE [h, w, scale]; gt_bbox (B,M,G) DEVICE, G = 4 or 5, rows with x1 == -1 padding
 *   mt_state: DEVICE int32[625] = numpy RandomState MT19937 key[624] + position, the generator
 *            np.random.choice draws from; advanced in place exactly as numpy advances it, images in
 *            order.  sd_mt19937_seed_host(seed, ...) fills the state np.random.seed(seed) produces.
 *   layout 0: cls_label (B,N), reg_target / reg_weight (B,N,4) in all-anchor order (level, y, x, a);
 *   layout 1: the loader's final arrays: cls_label (B, A * sumHW), reg_target / reg_weight
 *            (B, 4A, sumHW), levels concatenated along the last axis (one level: (4A, fh, fw)).
 *   An image with h >= w uses the (long, short) feature sizes, otherwise (short, long).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int nlvl;
  int stride[SD_MAX_FPN_LEVELS], short_side[SD_MAX_FPN_LEVELS], long_side[SD_MAX_FPN_LEVELS];
  int n_scales, n_aspects;
  double scales[16], aspects[16]; /* n_scales * n_aspects <= 16 */
  int allowed_border;
  float pos_thr, neg_thr, min_pos_thr;
  int image_anchor;
  double pos_fraction;
} sd_rpn_target_param;
#define SD_MT19937_STATE_WORDS 625
int sd_mt19937_seed_host(uint32_t seed, int32_t* state_host);
int sd_rpn_target_num_anchors(const sd_rpn_target_param* param_host);
size_t sd_rpn_target_workspace_bytes(const sd_rpn_target_param* param_host, int B, int M);
int sd_rpn_anchor_target(const float* im_info, const float* gt_bbox, int B, int M, int G,
                         const sd_rpn_target_param* param_host, int32_t* mt_state,
                         float* cls_label, float* reg_target, float* reg_weight, int layout,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DeformableConvolution v1  (mx.sym.contrib.DeformableConvolution; call site models/dcn/
 *   builder.py:14-17).  The arithmetic is upstream MXNet 1.6.0 (un-vendored third party,
 *   src/operator/contrib/nn/deformable_im2col.cuh + deformable_convolution-inl.h): each entry point
 *   replaces the function of the same name there.
 *   x (N,C,H,W)  offset (N, dgroup*2*kh*kw, Ho, Wo)  weight (F, C, kh, kw)  y (N,F,Ho,Wo)
 *   col (N, C*kh*kw, Ho*Wo), row (c*kh + i)*kw + j
 *   Ho = (H + 2*pad_h - (dil_h*(kh-1) + 1)) / stride_h + 1, Wo likewise; a dilated kernel extent larger than
 *   the padded input on either axis is SD_ERR_INVALID_ARG ("kernel size exceed input") at every stride.
 * ---------------------------------------------------------------------------------------------- */
int sd_deform_im2col(const float* x, const float* offset, float* col, int N, int C, int H, int W,
                     int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w, int dil_h,
                     int dil_w, int dgroup, void* stream);
/* data gradient: d_x (N,C,H,W) (+)= scatter of col (deformable_col2im) */
int sd_deform_col2im(const float* col, const float* offset, float* d_x, int req, int N, int C,
                     int H, int W, int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                     int dil_h, int dil_w, int dgroup, void* stream);
/* The same with a workspace of sd_deform_col2im_workspace_bytes(N, dgroup) bytes (ABI v7): the gradient planes
 * are summed in 32-bit fixed point with integer LDS adds (2.3x faster than the fp32 compare-and-swap adds of the
 * workspace-free call; bit-reproducible).  The unit is 2^-28 .. 2^-27 of (max|col| of a workgroup's own values
 * x the largest sum of bilinear weights one pixel of its (image, group) can collect); a workgroup whose values
 * are not finite, or whose max|col| x weight bound exceeds 8192 x its mean |col| (heavy-tailed gradients: the
 * unit would be too coarse for the typical element), sums with the float adds instead -- the reference's
 * arithmetic (upstream deformable_col2im: atomicAdd per corner).  This is the path the layer's backward takes. */
size_t sd_deform_col2im_workspace_bytes(int N, int dgroup);
int sd_deform_col2im_ws(const float* col, const float* offset, float* d_x, int req, int N, int C,
                        int H, int W, int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                        int dil_h, int dil_w, int dgroup, void* workspace, size_t workspace_bytes,
                        void* stream);
/* offset gradient: d_offset like offset (deformable_col2im_coord) */
int sd_deform_col2im_coord(const float* col, const float* x, const float* offset, float* d_offset,
                           int req, int N, int C, int H, int W, int kh, int kw, int pad_h,
                           int pad_w, int stride_h, int stride_w, int dil_h, int dil_w, int dgroup,
                           void* stream);
/* fp32-in / fp32-out matrix-core GEMM (row-major, batched): C[b] = op(A[b]) . op(B[b]); op(A) is
 * M x K.  accumulate: 0 store, 1 C += product, 2 atomic add (several batches into one C:
 * strideC = 0).  Replaces the linalg_gemm calls of deformable_convolution-inl.h (cuBLAS sgemm in
 * the reference).
 * Arithmetic (tuning key `deform_gemm_split`):
 *   2 (default)  scaled fp16 split: a pre-pass takes max|A| and max|B|, each operand is scaled by the
 *      power of two that brings its maximum into [2^13, 2^14) and split into two fp16 parts
 *      (hi = RNE(x s), lo = RNE(x s - hi): 22 mantissa bits), a product is a_hi*b_hi + a_hi*b_lo +
 *      a_lo*b_hi on v_mfma_f32_32x32x16_f16 (hi*hi exact in the fp32 accumulator), the result is scaled
 *      back exactly.  Error against fp64 = that of the fp32 MFMA path (measured 5e-7 x max|C| at K =
 *      2304; tests hold it to <= 2x the exact path's).  Elements below 2^-17 of their operand's maximum
 *      lose relative (not absolute) precision; non-finite inputs give NaN.  Needs the maxima, i.e. a
 *      workspace: sd_gemm_f32_ws and the sd_deform_conv_* entry points; plain sd_gemm_f32 runs the exact
 *      path (0) instead.
 *   1  bf16 split, no pre-pass: hi = RNE(x), lo = RNE(x - hi) in bf16, 16 mantissa bits: 4.5e-6 x
 *      max|C| (nine times the exact path's error); opt-in.
 *   0  v_mfma_f32_32x32x2_f32: exact fp32 products, 5e-7 x max|C|, ~2.5x slower.
 *   Split paths: when the last round of resident workgroups would be under half full its tiles are cut
 *   into k slices that add atomically (those tiles' last bits then depend on the order; key
 *   `deform_gemm_ksplit` = 0 turns that off). */
int sd_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, int lda, long strideA,
                const float* B, int ldb, long strideB, float* C, int ldc, long strideC, int batch,
                int accumulate, void* stream);
/* the same with a workspace of sd_gemm_f32_workspace_bytes() bytes for the operand maxima (two extra
 * small launches that read A and B once) */
size_t sd_gemm_f32_workspace_bytes(void);
int sd_gemm_f32_ws(int transA, int transB, int M, int N, int K, const float* A, int lda, long strideA,
                   const float* B, int ldb, long strideB, float* C, int ldc, long strideC, int batch,
                   int accumulate, void* workspace, size_t workspace_bytes, void* stream);
size_t sd_deform_conv_workspace_bytes(int N, int C, int H, int W, int kh, int kw, int pad,
                                      int stride, int dil);
/* forward WITHOUT the col matrix: deformable sampling fused into the GEMM's B-operand staging (every
 * sample taken once, all filters of a pixel tile in one workgroup).  3x3 kernels, C / dgroup % 16 == 0
 * and H*W % 4 == 0 (every DCN layer of the reference's configs); other shapes run the unfused forward
 * below through the same call (the workspace size says which: a few MB of pre-split weights against
 * the N*C*9*Ho*Wo*4-byte col matrix).  Same arithmetic as the unfused path (sampled values bit-equal to
 * sd_deform_im2col's, products by the scaled fp16 split), another summation order over k.
 *   replaces DeformableConvolutionOp::Forward (upstream MXNet 1.6 deformable_convolution-inl.h;
 *   call site models/dcn/builder.py:14-17) */
size_t sd_deform_conv_fwd_nocol_workspace_bytes(int N, int C, int H, int W, int F, int kh, int kw, int pad,
                                                int stride, int dil, int dgroup);
int sd_deform_conv_fwd_nocol(const float* x, const float* offset, const float* weight, float* y, int N,
                             int C, int H, int W, int F, int kh, int kw, int pad, int stride, int dil,
                             int dgroup, void* workspace, size_t workspace_bytes, void* stream);
/* forward = im2col + GEMM, num_group = 1, no bias (the reference's configuration) */
int sd_deform_conv_fwd(const float* x, const float* offset, const float* weight, float* y, int N,
                       int C, int H, int W, int F, int kh, int kw, int pad, int stride, int dil,
                       int dgroup, void* workspace, size_t workspace_bytes, void* stream);
/* backward: d_x, d_offset, d_weight with their own req (0 null / 1 write / 3 add) */
int sd_deform_conv_bwd(const float* out_grad, const float* x, const float* offset,
                       const float* weight, float* d_x, float* d_offset, float* d_weight,
                       int req_x, int req_offset, int req_weight, int N, int C, int H, int W,
                       int F, int kh, int kw, int pad, int stride, int dil, int dgroup,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same backward with the col matrix of the forward kept instead of recomputed: fwd_col =
 * sd_deform_conv_col_of_workspace(the workspace sd_deform_conv_fwd ran with, untouched since); the
 * backward needs a workspace of its own (dcol).  Same results as sd_deform_conv_bwd (im2col is
 * deterministic: the col matrix is the same bits); it trades N*C*kh*kw*Ho*Wo*4 bytes held per layer between the two
 * calls for the im2col pass (0.29 of 1.85 ms on the (16,256,50,84) layer). */
const float* sd_deform_conv_col_of_workspace(const void* fwd_workspace);
int sd_deform_conv_bwd_cached(const float* out_grad, const float* x, const float* offset,
                              const float* weight, const float* fwd_col, float* d_x,
                              float* d_offset, float* d_weight, int req_x, int req_offset,
                              int req_weight, int N, int C, int H, int W, int F, int kh, int kw,
                              int pad, int stride, int dil, int dgroup, void* workspace,
                              size_t workspace_bytes, void* stream);

/* The operator with ALL of DeformableConvolutionParam (upstream MXNet 1.6 deformable_convolution-inl.h:
 * kernel, stride, dilate, pad, num_filter, num_group, num_deformable_group, no_bias) -- the call sites
 * beside models/dcn/builder.py pass a bias (models/RepPoints/builder.py:215-245, no_bias=False) and
 * num_group / bias through (models/sepc/sepc_dconv.py:5-16; models/tridentnet/resnet_v1.py:85-90).
 *   weight (F, C / num_group, kh, kw): filter block g (F / num_group filters) sees input channels
 *   [g C / num_group, (g + 1) C / num_group) (the col rows of those channels), as the reference's loop
 *   over group_ does; bias (F) or NULL (= no_bias): y[n, f, :] += bias[f] after the products, as
 *   `out += broadcast<1>(bias)` does.  d_bias (F) (+)= sum over n, pixels of out_grad
 *   (`sumall_except_dim<1>`), its own req.
 * forward: keep_col = 0 -> the col-free fused kernel where the shape allows (num_group = 1, see
 *   sd_deform_conv_fwd_nocol; the bias is added in its epilogue), else im2col + one GEMM per group + a
 *   bias pass; keep_col = 1 -> always the latter, and the col matrix stays in the workspace for
 *   sd_deform_convolution_bwd(fwd_col = sd_deform_conv_col_of_workspace(workspace)).
 * backward: fwd_col NULL -> recomputed.  Workspace: sd_deform_conv_workspace_bytes. */
size_t sd_deform_convolution_fwd_workspace_bytes(int N, int C, int H, int W, int F, int kh, int kw, int pad,
                                                 int stride, int dil, int dgroup, int num_group, int keep_col);
int sd_deform_convolution_fwd(const float* x, const float* offset, const float* weight, const float* bias,
                              float* y, int N, int C, int H, int W, int F, int kh, int kw, int pad, int stride,
                              int dil, int dgroup, int num_group, int keep_col, void* workspace,
                              size_t workspace_bytes, void* stream);
int sd_deform_convolution_bwd(const float* out_grad, const float* x, const float* offset, const float* weight,
                              const float* fwd_col, float* d_x, float* d_offset, float* d_weight, float* d_bias,
                              int req_x, int req_offset, int req_weight, int req_bias, int N, int C, int H,
                              int W, int F, int kh, int kw, int pad, int stride, int dil, int dgroup,
                              int num_group, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_Proposal_v3  (mx.sym.contrib.Proposal_v3, models/FPN/builder.py:275-287) -- SURVEY 8(f)
 *   replaces ProposalGPUOp_v3::Forward  operator_cxx/contrib/proposal_v3.cu:428-638 (anchor grid
 *   :64-85, box decode :92-155, top-k by thrust sort, min-size filter :211-235, NMS with >= and its
 *   host scan :271-381, PrepareOutput :386-416; three D2H/H2D copies per image)
 *   cls_prob (B,2A,H,W) (foreground = second half)  bbox_pred (B,4A,H,W)  im_info (B,3) DEVICE
 *   out (B,post,4)  score (B,post): post = is_train ? min(post_nms_top_n, pre) : post_nms_top_n;
 *   padding past the kept boxes: zeros (test) or the kept boxes repeated cyclically (is_train).
 *   sd_proposal_v3_iou is the op with iou_loss = true: IoUPredKernel (proposal_v3.cu:163-205, the
 *   four deltas are added to the anchor's corners) in place of BBoxPredKernel; no reference config
 *   enables it.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_proposal_v3_workspace_bytes(int B, int A, int H, int W, int pre_nms_top_n);
int sd_proposal_v3(const float* cls_prob, const float* bbox_pred, const float* im_info, float* out,
                   float* score, int B, int A, int H, int W, int rpn_pre_nms_top_n,
                   int rpn_post_nms_top_n, float threshold, int rpn_min_size,
                   const float* scales_host, int n_scales, const float* ratios_host, int n_ratios,
                   int feature_stride, int is_train, void* workspace, size_t workspace_bytes,
                   void* stream);
int sd_proposal_v3_iou(const float* cls_prob, const float* bbox_pred, const float* im_info,
                       float* out, float* score, int B, int A, int H, int W, int rpn_pre_nms_top_n,
                       int rpn_post_nms_top_n, float threshold, int rpn_min_size,
                       const float* scales_host, int n_scales, const float* ratios_host,
                       int n_ratios, int feature_stride, int is_train, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_Proposal_v2  (mx.sym.contrib.Proposal_v2, models/tridentnet/builder.py:239-255) and
 * _contrib_Proposal     (mx.sym.contrib.Proposal, X.proposal of symbol/builder.py:241)
 *   replace ProposalGPUOp_v2::Forward  operator_cxx/contrib/proposal_v2.cu:413-620 and
 *   ProposalGPUOp::Forward proposal.cu:417-614 (im_info / valid_ranges D2H, per image a thrust
 *   stable sort of every anchor, the NMS mask D2H, a host scan and keep H2D).  The spec is the .cu:
 *   - decode BBoxPredKernel (:92-147): centre x1 + 0.5 (w - 1), corners centre -/+ 0.5 (pred_w - 1),
 *     dw / dh NOT clamped (exp may give inf; the clip to [0, im - 1] decides); or IoUPredKernel
 *     (:155-195) with iou_loss; anchors as proposal_v2-inl.h GenerateAnchors (floor(x + 0.5f), not
 *     the rintf of Proposal_v3)
 *   - score -1 for anchors at h >= (int)(im_h / stride) or w >= (int)(im_w / stride) (both
 *     variants).  An image taller / wider than H * stride (the reference aborts on CHECK_GE)
 *     marks no anchor.
 *   - FilterBoxKernel (:201-222) on ALL rows before the top-k: min_size = rpn_min_size * im_info[2];
 *     a side < min_size grows the box by min_size / 2 on each side and scores it -1; else, for v2
 *     with filter_scales, area < valid_ranges[i,0]^2 or > valid_ranges[i,1]^2 (fp32) scores it -1
 *   - top-`pre` of a stable descending sort over all rows (the -1 rows included), NMS with IoU > thr
 *     (strict, +1 areas); rows scored -1 are not excluded and can be emitted
 *   - out (B,post,4)  score (B,post): the kept boxes, then zeros (v2; v1 test) or the kept boxes
 *     repeated cyclically (v1 is_train).  Proposal in test mode keeps post as given
 *     (proposal.cu:453-455), so post > pre is well formed there and zero padded.
 *   cls_prob (B,2A,H,W) (foreground = second half)  bbox_pred (B,4A,H,W)  im_info (B,3)
 *   valid_ranges (B,2) DEVICE (read only with filter_scales; may be NULL otherwise).
 *   NaN rule: a NaN score is ordered by its bits (positive NaNs before +inf, negative after -inf);
 *   a NaN box coordinate is clipped to im - 1 (the reference's fminf); a NaN side or area fails no
 *   filter test; a NaN IoU suppresses nothing.
 *   SD_ERR_UNSUPPORTED: rpn_post_nms_top_n > min(pre, A*H*W) for v2, and for v1 with is_train (the
 *   reference shapes the output (B, post) but writes image i at stride min(post, pre): rows
 *   misplaced, the tail never written);
 *   pre > 16384 (the LDS sort capacity).  SD_ERR_INVALID_ARG: A*H*W >= 2^24.
 *   Backward (proposal_v2.cu:617-639) is all zeros and has no entry point.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_proposal_v2_workspace_bytes(int B, int A, int H, int W, int pre_nms_top_n);
int sd_proposal_v2(const float* cls_prob, const float* bbox_pred, const float* im_info,
                   const float* valid_ranges, float* out, float* score, int B, int A, int H, int W,
                   int rpn_pre_nms_top_n, int rpn_post_nms_top_n, float threshold,
                   int rpn_min_size, const float* scales_host, int n_scales,
                   const float* ratios_host, int n_ratios, int feature_stride, int filter_scales,
                   int iou_loss, void* workspace, size_t workspace_bytes, void* stream);
size_t sd_proposal_workspace_bytes(int B, int A, int H, int W, int pre_nms_top_n);
int sd_proposal(const float* cls_prob, const float* bbox_pred, const float* im_info, float* out,
                float* score, int B, int A, int H, int W, int rpn_pre_nms_top_n,
                int rpn_post_nms_top_n, float threshold, int rpn_min_size, const float* scales_host,
                int n_scales, const float* ratios_host, int n_ratios, int feature_stride,
                int is_train, int iou_loss, void* workspace, size_t workspace_bytes, void* stream);
/* get_top_proposal CustomOp (models/FPN/get_top_proposal.py:15-39): the top_n rows of bbox (B,N,4)
 * by score (B,N) descending (ties: lower row first), zero padded when N < top_n */
int sd_get_top_proposal(const float* bbox, const float* score, int B, int N, int top_n,
                        float* out_bbox, float* out_score, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_DecodeBBox  (mx.sym.contrib.DecodeBBox / X.decode_bbox, symbol/builder.py:384-392) and
 * the test-time per-class filter in front of soft-NMS -- SURVEY 8(f) rank 2
 *   replaces DecodeBBoxOp::Forward  operator_cxx/contrib/decodebbox.cc:147-215 (host round trip +
 *   BBoxTransformXYWH :34-80 / BBoxTransformXYXY :84-131)
 *   rois (B,R,4)  bbox_pred (B,R,4K)  im_info (B,3) DEVICE  out (B,R,4K), or (B,R,4) when
 *   class_agnostic (then the deltas of class 1 are used, decodebbox.cc:56)
 * ---------------------------------------------------------------------------------------------- */
int sd_decode_bbox(const float* rois, const float* bbox_pred, const float* im_info, float* out,
                   int B, int R, int K, const float* bbox_mean_host, const float* bbox_std_host,
                   int class_agnostic, int decode_xyxy, void* stream);
/* detection_test.py:233-247 (do_nms): for every (image, class) the rows with
 * cls_score > min_det_score as [x1,y1,x2,y2,score], row order kept -- written in the layout
 * sd_soft_nms_batched reads: dets (B*K, R, 5), counts (B*K).  bbox (B,R,4*bbox_classes),
 * bbox_classes = K (class specific boxes) or 1 (shared box). */
int sd_det_filter(const float* bbox, const float* cls_score, int B, int R, int K, int bbox_classes,
                  float min_det_score, float* dets, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * nms (numpy), batched  (operator_py/nms.py:41-75 through py_nms_wrapper :19-22 -- the default
 *   test-time NMS, detection_test.py:224-267, and the one BboxPostProcessing runs)
 *   dets (P,Nmax,5) [x1,y1,x2,y2,score]: problem p uses rows [0, counts[p]) (counts NULL: all Nmax)
 *   -- the layout sd_det_filter writes.  Every operation is a float32 operation, as numpy's:
 *   area = (x2-x1+1)*(y2-y1+1), w = max(0, xx2-xx1+1), ovr = w*h / (area_i + area_j - w*h); box j
 *   survives a kept box i iff ovr <= thresh (float32), so a NaN ovr suppresses.  NOT
 *   sd_soft_nms_batched(method 0), which adds 1 in double (cpu_nms.pyx) and selects by arg-max.
 *   Order: descending score; among EQUAL scores the LATER input row first (argsort(kind="stable")[::-1];
 *   the reference's own order of ties is numpy's unstable sort).  sd_nms keeps the LOWER row first.
 *   NaN scores come before every number (numpy sorts them last, the reversal first).
 *   out_dets (P,Nmax,5) / out_inds (P,Nmax): the kept rows (copies of the input's floats) and their
 *   input rows, in that order; out_counts (P).  Rows past out_counts[p] are unspecified (not written).
 *   SD_ERR_UNSUPPORTED: Nmax > 4096 (a problem is sorted and resolved in LDS).
 * ---------------------------------------------------------------------------------------------- */
int sd_hard_nms_batched(const float* dets, const int32_t* counts, int P, int Nmax, float thresh,
                        float* out_dets, int32_t* out_inds, int32_t* out_counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BboxPostProcessing CustomOp  (models/maskrcnn/bbox_post_processing.py:6-111, emitted by
 *   models/maskrcnn/builder.py:65-84 between DecodeBBox and the mask head's RoIAlign)
 *   replaces BboxPostProcessingOperator.forward :43-72 (asnumpy of both inputs, a Python loop over the
 *   classes around the numpy nms above, argsort, three copies back) and multiclass_nms :6-32
 *   cls_score (B,R,K), column 0 = background (dropped); bbox_xyxy (B,R,4*bbox_classes), bbox_classes
 *   = 1 (shared box) or K (class c's box in columns 4c..4c+3, background's unused).
 *   Per image and foreground class: the rows with score > min_det_score (NaN fails) in row order,
 *   hard NMS as sd_hard_nms_batched; classes stacked in class order; the max_det_per_image best by
 *   score, descending, among equal scores the LATER entry of the stacked list first.
 *   post_score (B,max_det,1) zero padded, post_bbox (B,max_det,4) zero padded, post_cls (B,max_det,1)
 *   = class id after dropping the background (0-based) as a float, padded with -1.  Every element of
 *   the three outputs is written by every call.  Backward is all zeros (:74-76) and has no entry point.
 *   Two launches on `stream` (per-class NMS, image top-k), no host synchronisation, capturable.
 *   The (B*K,R,5) tensor of sd_det_filter is never formed: the kept rows' keys go to the workspace
 *   (sd_bbox_post_processing_workspace_bytes, 8-byte aligned).
 *   SD_ERR_UNSUPPORTED: R > 4096, K > 256, max_det_per_image > 1024, bbox_classes not in {1, K}.
 *   B = 0, R = 0, K = 1 and "no row over the threshold" are valid and produce the padding.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_bbox_post_processing_workspace_bytes(int B, int R, int K, int bbox_classes, int max_det_per_image);
int sd_bbox_post_processing(const float* cls_score, const float* bbox_xyxy, int B, int R, int K,
                            int bbox_classes, float min_det_score, float nms_thr, int max_det_per_image,
                            float* post_score, float* post_bbox, float* post_cls, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_GenProposalRetina  (mx.sym.contrib.GenProposalRetina, models/retinanet/builder.py:358-389)
 *   replaces GenProposalRetinaGPUOp::Forward  operator_cxx/contrib/generate_proposal_retina.cu:301-468
 *   (im_info D2H, thrust::stable_sort of every (anchor, class, y, x) score per image); the spec is
 *   the .cu (grid :66-94, BBoxPredKernel :96-159, IoUPredKernel :161-209, FilterBoxKernel :211-233,
 *   PrepareOutput :275-297), not the stale generate_proposal_retina.cc.
 *   cls_prob (B,AK,H,W), channel c = anchor*K + class, K = AK / num_anchors; bbox_pred (B,4A,H,W);
 *   im_info (B,3) DEVICE; anchors (H*W*A,4), or (B,H*W*A,4) when batch_wise_anchor.
 *   out (B,rpn_pre_nms_top_n,4)  score (B,rpn_pre_nms_top_n,oc), oc = output_one_hot ? K+1 : 1:
 *   the first min(rpn_pre_nms_top_n, A*K*H*W) rows of the stable descending order of
 *   (filtered ? 0 : score), row i = (h*W + w)*AK + c; a filtered row (score <= thresh, box side <
 *   rpn_min_size*im_info[2], or a NaN score) is zeros; the score goes to column
 *   min(oc-1, class+1); every other element is zero.  Every element of out / score is written.
 *   mean_host / std_host: anchor_mean / anchor_std, 4 floats each (host).
 *   Limits: A*K*H*W <= 2^28 rows per image; min(rpn_pre_nms_top_n, rows) <= 16384.
 *   SD_ERR_UNSUPPORTED (the reference reads out of bounds): iou_loss with K > 1 (:161-209 indexes
 *   the deltas with a < A*K), batch_wise_anchor with B > 1 and K > 1 (anchor offset i*A*K*H*W*4,
 *   :383).  Backward (:471-493) is all zeros and has no entry point.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_gen_proposal_retina_workspace_bytes(int B, int AK, int H, int W);
int sd_gen_proposal_retina(const float* cls_prob, const float* bbox_pred, const float* im_info,
                           const float* anchors, float* out, float* score, int B, int AK, int H,
                           int W, int num_anchors, int rpn_pre_nms_top_n, int rpn_min_size,
                           float thresh, const float* mean_host, const float* std_host, int iou_loss,
                           int output_one_hot, int batch_wise_anchor, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RetinaNet anchor targets  (the loader's PyramidAnchorTarget2D of models/retinanet/input.py:33-199,
 *   over AnchorTarget2D core/detection_input.py:345-565; call site RetinaNetHead.get_loss
 *   models/retinanet/builder.py:239-339).  A different assignment from sd_rpn_anchor_target: labels
 *   are class-valued, nothing is subsampled (no generator state; image_anchor / pos_fraction of the
 *   parameter are ignored), every valid anchor gets a regression target, and there is a per-image
 *   foreground count.
 *   im_info (B,3) DEVICE; gt_bbox (B,M,5) DEVICE [x1,y1,x2,y2,class], rows with x1 == -1 padding.
 *   Labels (:42-66): -1; a valid anchor with max_overlap < neg_thr -> 0; every anchor i for which
 *   some gt j has overlap[i,j] == gt_max[j] and overlap[i,j] >= min_pos_thr -> gt[j,4], the LARGEST
 *   such j (numpy's fancy assignment keeps the last of np.where's row-major pairs; with
 *   min_pos_thr = 0 a gt that overlaps no valid anchor labels every zero-overlap anchor: the
 *   reference's own TODO, reproduced); max_overlap >= pos_thr -> gt[argmax,4], first maximum.
 *   reg_target (:69) is the nonlinear_transform encoding against the arg-max gt for EVERY valid
 *   anchor, reg_weight (:70) is 1 where label >= 1.  No valid gt: label 0 on valid anchors, targets
 *   and weights 0.  Anchors outside allowed_border: -1 / 0 / 0.
 *   fg_count (B) float = max(1, #(label > 0))  (:192).
 *   layout 0: cls_label (B,N), reg_target / reg_weight (B,N,4) in all-anchor order (level, y, x, a);
 *   layout 1: the loader's final arrays (:149-199): cls_label (B,N) = per level (A, fh, fw), levels
 *            concatenated; reg_target / reg_weight (B, 4A, sumHW), levels concatenated along the
 *            last axis -- the order get_loss's cls_logit_concat expects.
 *   Limits (those of sd_rpn_anchor_target): N < 2^28 anchors per image, A <= 16, nlvl <= 8,
 *   M <= 3276 (20 bytes of LDS per gt row).  reg_target / reg_weight 16-byte aligned.
 *   No host synchronisation; graph-capturable.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_retina_target_workspace_bytes(const sd_rpn_target_param* param_host, int B, int M);
int sd_retina_anchor_target(const float* im_info, const float* gt_bbox, int B, int M,
                            const sd_rpn_target_param* param_host, float* cls_label,
                            float* reg_target, float* reg_weight, float* fg_count, int layout,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_FocalLoss  (X.focal_loss; models/retinanet/builder.py:289-297, models/RepPoints/
 *   builder.py:404) and _contrib_BBoxNorm  (X.bbox_norm; builder.py:320-324), fp32.
 *   replaces FocalLossOp::Forward / Backward  operator_cxx/contrib/focal_loss-inl.h:90-231 (seven
 *   full-size temporaries out of a 1.5-1.8 GB workspace) and BBoxNormOp::Backward
 *   operator_cxx/contrib/bbox_norm-inl.h:99-129.
 *   sd_focal_loss_fwd: out = 1 / (1 + exp(-data)) over n elements (:113).
 *   sd_focal_loss_bwd: out / ograd / gdata (B,nbox,nclass), label (B,nbox).  Element rule (:186-230),
 *     p = out[b,n,c], eps = 1e-14f, every operation in fp32 in the reference's order:
 *       class c == int(label - 1)  [one_hot truncates toward zero; an index outside [0,nclass) and a
 *       NaN label select no class]:     alpha * (1-p)^gamma * (gamma * p * log(p + eps) + p - 1)
 *       elsewhere:                 -((1-alpha) * p^gamma * (gamma * (1-p) * log((1-p) + eps) - p))
 *       label == -1: the whole row is 0.
 *     Then * ograd when ograd_or_null is given (the op's out_grad=True), then
 *       normalization 2 (valid): (g * grad_scale) / (count + 1), count = #(label >= 1) over the whole
 *                                batch, reduced on the device as an integer; no max, as in :220-221
 *       normalization 1 (batch): g * (grad_scale / B)
 *       normalization 0 (null):  g * grad_scale.
 *     gamma == 2, 1, 0 multiply; any other gamma goes through powf.  gdata is written (kWriteTo);
 *     the label gradient (zeros in the reference) has no entry point.
 *   sd_bbox_norm_bwd: gout / gdata (B, n_per_image), label (B, n_label_per_image):
 *     gdata = gout / max(1, count + 1), the same count (bbox_norm-inl.h:116-126).  The forward is a copy.
 *   The count lives in the workspace (sd_focal_loss_workspace_bytes(), shared by both backwards) and
 *   the gradient kernels read it from device memory: no host synchronisation, graph-capturable.
 *   16-byte loads and stores when nclass % 4 == 0 (n for the other two) and every data pointer is
 *   16-byte aligned; a scalar path otherwise (4-byte alignment suffices).
 *   Limits: B * nbox * nclass <= 2^31 - 1 elements for the focal backward, B * n_label_per_image <= 2^31 - 1
 *   labels for sd_bbox_norm_bwd (the count is a 32-bit integer); SD_ERR_UNSUPPORTED beyond.  B = 0, nbox = 0 or
 *   nclass = 0 succeed without touching the device.
 * ---------------------------------------------------------------------------------------------- */
int sd_focal_loss_fwd(const float* data, float* out, long n, void* stream);
size_t sd_focal_loss_workspace_bytes(void);
int sd_focal_loss_bwd(const float* out, const float* label, const float* ograd_or_null, float* gdata,
                      int B, int nbox, int nclass, float alpha, float gamma, float grad_scale,
                      int normalization, void* workspace, size_t workspace_bytes, void* stream);
int sd_bbox_norm_bwd(const float* gout, const float* label, float* gdata, int B, long n_per_image,
                     long n_label_per_image, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_GroupNorm  (mx.sym.contrib.GroupNorm; config/scratch/mask_r50v1b_fpn_gn_scratch_2x.py,
 *   the five config/RepPoints and three config/efficientnet configs), fp32, NCHW.
 *   replaces GroupNormOp::Forward / Backward  operator_cxx/contrib/group_norm.cu:71-298 and the Moments /
 *   InvStd helpers of group_norm_helper.cu:36-63,258-268 (five launches; X read twice forward, dY and X three
 *   times backward).
 *   x / y / dy / dx (N,C,HxW) contiguous, gamma / beta / dgamma / dbeta (C), mu / rsig N*G floats, D = C / G.
 *   sd_group_norm_fwd, per group (n, g) over its D*HxW contiguous floats:
 *       mu = mean,  rsig = 1 / sqrt(var + eps) with the biased variance,
 *       y = gamma[c] * (x - mu) * rsig + beta[c]              (the reference's order, :87-89).
 *     The variance is taken ABOUT THE MEAN (two passes over resident data; Chan merging of per-chunk partials in
 *     double where a group is split over workgroups), not as the reference's fp32 E[x^2] - mu^2, which cancels
 *     when |mu| >> sigma and can go negative (NaN from rsqrtf): the one deliberate departure.
 *     mu and rsig receive N*G floats each; a larger buffer (the reference declares the outputs (N,C)) keeps its
 *     tail untouched.
 *   sd_group_norm_bwd, with the sums taken about mu (ds = sum gamma[c] * dy * (x - mu), db = sum gamma[c] * dy
 *     over the group, so the reference's (db * mu - ds) of :152 is -ds without its cancellation):
 *       dx = gamma[c] * dy * rsig + ((-ds) * (x - mu) * rsig^3 - db * rsig) * (1 / (D*HxW))      (:152-158)
 *       dgamma[c] = sum over n, hw of dy * (x - mu) * rsig,   dbeta[c] = sum over n, hw of dy    (:184-186)
 *     dx, dgamma and dbeta are written (kWriteTo).  dgamma and dbeta may be NULL together: they are skipped.
 *   Groups of up to 4096 (backward 2048) 16-byte items are held in registers: x (and dy) read once, y (dx)
 *   written once, one launch (+ one tiny launch for dgamma / dbeta).  Larger groups are split over workgroups:
 *   three launches, x (dy and x) read twice.  sd_last_dispatch() names the kernels taken.
 *   16-byte loads and stores when HxW % 4 == 0 and x, y (dy, x, dx) are 16-byte aligned; a scalar path otherwise
 *   (4-byte alignment suffices).  Every reduction has a fixed order and there are no floating-point atomics: two
 *   calls on the same inputs give equal bits.  The workspace (sd_group_norm_workspace_bytes, monotone in N and C,
 *   one size for both directions) needs no clearing; kernels only, no host synchronisation, graph-capturable.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: a null pointer, G <= 0, C % G != 0, a
 *   negative size, dgamma / dbeta not NULL together, a NULL or too small workspace; SD_ERR_UNSUPPORTED:
 *   N*C*HxW > 2^31 - 1 elements.  N = 0, C = 0 or HxW = 0 succeed without a launch (no pointer is looked at;
 *   sd_group_norm_workspace_bytes returns its minimum for them and for invalid sizes).
 * ---------------------------------------------------------------------------------------------- */
size_t sd_group_norm_workspace_bytes(int N, int C, long HxW, int G);
int sd_group_norm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mu, float* rsig,
                      int N, int C, long HxW, int G, float eps, void* workspace, size_t workspace_bytes,
                      void* stream);
int sd_group_norm_bwd(const float* dy, const float* x, const float* mu, const float* rsig, const float* gamma,
                      float* dx, float* dgamma, float* dbeta, int N, int C, long HxW, int G, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_SigmoidCrossEntropy  (mx.sym.contrib.SigmoidCrossEntropy; the mask loss of
 *   models/maskrcnn/builder.py:307-312 and models/msrcnn/builder.py:418-423) and the fused mask loss of
 *   MaskFasterRcnnHead.get_loss (models/maskrcnn/builder.py:278-313), fp32.
 *   replaces SigmoidCrossEntropyOp::Forward / Backward  operator_cxx/contrib/sigmoid_cross_entropy.cu:44-122,
 *   -inl.h:68-119 (the reference has no CPU implementation: sigmoid_cross_entropy.cc:40,50 are LOG(FATAL)) and,
 *   for the fused op, the split / stack / gather_nd / concat / reshape subgraph in front of it, whose backward
 *   zero-fills and scatters a (R, K, P) gradient.
 *   Element rule, x = logit, t = target; the reference's literals `-1.`, `1.` and `1. /` are doubles, so each
 *   expression is evaluated partly in double and rounded to float once:
 *       t == -1:  loss = 0, count = 0, gradient = +0.0.  The branch is on the target alone: the logit is not
 *                 looked at (NaN and inf included) and the element does not reach the row sum.
 *       else      loss = float((-1.0 * x) * double(t - [x >= 0]) + double(logf(1 + expf(x - 2 * x * [x >= 0]))))
 *                 g    = float(1.0 / (1.0 + double(expf(-x))) - double(t)),   count = 1
 *       per row:  loss_sum = sum loss,  count_sum = float(sum count) + 1e-5f,  out = loss_sum / count_sum,
 *                 d = (g / count_sum) * grad_scale                      (two float roundings, as the reference)
 *   Quirks kept: the operator's `normalization` parameter is parsed and never used (the division by the count
 *   always happens; there is no such argument here); `out` is NOT multiplied by grad_scale, only the gradient
 *   is; the backward recomputes count and count_sum itself.
 *   sd_sigmoid_ce_fwd: data / label / loss / count (n, k) rows, out / loss_sum / count_sum (n).  loss and count
 *     may be NULL: they are then not written (the full-size tensors the visible output does not need).
 *   sd_sigmoid_ce_bwd: d_data (n, k) is written (kWriteTo), count_sum (n) too; count (n, k) may be NULL.
 *   sd_mask_loss_fwd / _bwd: logits (R, K, P), cls (R) float -- the builder's mask_label --, target (R, P),
 *     out / count_sum one float each, d_logits (R, K, P).  Equivalent to gathering plane (int)cls[r] of every
 *     row, flattening to one row of R*P elements and applying the operator above with n = 1: out, count_sum and
 *     the selected planes' gradients are bit-equal to that (the same element and reduction code runs).
 *     The backward writes ALL of d_logits once, in one pass: +0.0 in the planes that are not selected, the
 *     gradient in the selected one (kWriteTo; there is no add mode).  A row whose cls is NaN, negative or >= K
 *     is fully ignored: its logits are not read, it is not counted, its gradient is zero (the reference's
 *     gather_nd has undefined behaviour there).
 *   Counts are integers reduced on the device and converted once (exact for any k; equal to the reference's
 *   float sum of ones for k <= 2^24).  Row sums have a fixed order and use no floating-point atomics: two
 *   calls give equal bits.  Partials live in the workspace (sd_*_workspace_bytes, monotone in their arguments)
 *   and need no clearing; kernels only, no memset node, no host synchronisation, graph-capturable.  One long
 *   row (n = 1, k ~ 2e5, the reference's call sites) is spread over k / 256 waves; short rows get a wave each.
 *   16-byte loads and stores when k % 4 == 0 (P % 4 == 0) and the pointers are 16-byte aligned -- in the fused
 *   backward the stores follow d_logits and the loads follow logits and target, separately; a scalar path
 *   otherwise (4-byte alignment suffices), with equal bits.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: a negative size, a null pointer (other
 *   than loss / count), a NULL or too small workspace (SD_ERR_WORKSPACE); SD_ERR_UNSUPPORTED: n*k (R*K*P)
 *   > 2^31 - 1 elements.  n = 0 or k = 0 (R, K or P = 0) succeed without a launch, the sizes still checked.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_sigmoid_ce_workspace_bytes(long n, long k);
int sd_sigmoid_ce_fwd(const float* data, const float* label, float* out, float* loss, float* loss_sum,
                      float* count, float* count_sum, long n, long k, void* workspace, size_t workspace_bytes,
                      void* stream);
int sd_sigmoid_ce_bwd(const float* data, const float* label, float* d_data, float* count, float* count_sum,
                      long n, long k, float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
size_t sd_mask_loss_workspace_bytes(int R, int K, long P);
int sd_mask_loss_fwd(const float* logits, const float* cls, const float* target, float* out, float* count_sum,
                     int R, int K, long P, void* workspace, size_t workspace_bytes, void* stream);
int sd_mask_loss_bwd(const float* logits, const float* cls, const float* target, float* d_logits, int R, int K,
                     long P, float grad_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The Mask Scoring R-CNN training head (models/msrcnn/builder.py), fp32: the mask loss of
 *   MaskFasterRcnnHead.get_loss (:383-424), which also returns the gathered sigmoid `mask_pred_prob`, and the
 *   MaskIoU loss of MaskIoUConvHead.get_loss (:143-168) with the Python CustomOp `maskiou_compute`
 *   (models/msrcnn/maskiou_compute.py:14-38: four asnumpy() copies, numpy, two copies back) inside it.
 *   R rows (RoIs), K classes, P = resolution^2 pixels; cls (R) float is the builder's mask_label (mask_inds).
 *   sd_msrcnn_mask_loss_fwd: logits (R, K, P), cls, target (R, P) -> out, count_sum (one float each), bit-equal to
 *     sd_mask_loss_fwd on the same inputs (the same unit and reduction code runs), and prob (R, P):
 *         prob[r, p] = 1.0f / (1.0f + expf(-logits[r, (int)cls[r], p]))       MXNet's Activation(sigmoid)
 *     for EVERY element of a row whose cls names a plane, those with target -1 included (the MaskIoU head reads
 *     them).  A row whose cls is NaN, negative or >= K is ignored as in sd_mask_loss_*: its logits are not
 *     read and its prob row is +0.0.  One pass over the selected planes, one launch, plus the fixed-order finish.
 *   sd_msrcnn_mask_loss_bwd: d_prob (R, P) may be NULL.  d_logits (R, K, P) is written once (kWriteTo): +0.0 in
 *     the planes that are not selected; in the selected plane
 *         g_ce + d_prob * (p * (1.0f - p)),   g_ce = sd_mask_loss_bwd's value (+0.0 where the target is -1),
 *     p recomputed by the forward's expression (equal bits to reading prob).  With d_prob == NULL all of d_logits
 *     is bit-equal to sd_mask_loss_bwd (the same kernel runs).  d_prob of ignored rows is not read.  16-byte loads
 *     (logits, target, d_prob) and 16-byte stores (d_logits) are decided separately; P % 4 != 0 or a pointer off
 *     its 16-byte boundary takes a scalar path with equal bits.
 *   sd_maskiou_loss_fwd: iou_pred (R, K), prob (R, P), target (R, P), ratio (R), cls (R) -> iou_target (R),
 *     weight (R), loss (1), weight_sum (1).  Per row, restating maskiou_compute.py:20-35 with numpy's types:
 *         pred = prob > 0.5f;  Ps = count(pred);  I = sum(target where pred);  T = sum(target)
 *         union = max(double(T) / double(ratio) + double(Ps) - double(I), 1.0)
 *         iou_target = float(double(max(I, 0)) / union);       weight = cls > 0 ? 1 : 0
 *     max is numpy.maximum (a NaN propagates); a zero ratio follows IEEE (a -inf union becomes 1, 0 / 0 a NaN).
 *     The contract is integer-valued targets (-1, 0, 1): any summation order gives the reference's bits; for other
 *     values I and T are fixed-order float sums.  Then p = iou_pred[r, (int)cls[r]] and
 *         S = sum_r ((iou_target - p)^2 * weight),  W = sum_r weight,  loss = 0.5f * S / max(W, 1),  weight_sum = W
 *     over the rows whose cls names a column; a row whose cls is NaN, negative or >= K reaches neither S nor W and
 *     its iou_pred is not read (iou_target and weight are still written for it).  Fixed-order sums, no float atomics.
 *   sd_maskiou_loss_bwd: d_iou_pred (R, K) written once: ((-(iou_target - p)) * weight) / max(W, 1) * grad_scale in
 *     column (int)cls[r], +0.0 everywhere else.  Nothing flows to prob, target or ratio (the reference BlockGrads
 *     the CustomOp's outputs).  It needs no workspace.
 *   All: kernels only, no memset node, no host synchronisation, graph-capturable; workspaces need no clearing and
 *   their sizes are monotone; repeated calls give equal bits; 4-byte alignment suffices.  Checked before anything
 *   touches the device -- SD_ERR_INVALID_ARG: a negative size, a null pointer (other than d_prob);
 *   SD_ERR_WORKSPACE: a NULL or too small workspace; SD_ERR_UNSUPPORTED: R*K*P (mask loss) or R*K, R*P (MaskIoU)
 *   > 2^31 - 1 elements.  A zero size succeeds without a launch, the sizes still checked.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_msrcnn_mask_loss_workspace_bytes(int R, int K, long P);
int sd_msrcnn_mask_loss_fwd(const float* logits, const float* cls, const float* target, float* out,
                            float* count_sum, float* prob, int R, int K, long P, void* workspace,
                            size_t workspace_bytes, void* stream);
int sd_msrcnn_mask_loss_bwd(const float* logits, const float* cls, const float* target, const float* d_prob,
                            float* d_logits, int R, int K, long P, float grad_scale, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t sd_maskiou_loss_workspace_bytes(int R, int K, long P);
int sd_maskiou_loss_fwd(const float* iou_pred, const float* prob, const float* target, const float* ratio,
                        const float* cls, float* iou_target, float* weight, float* loss, float* weight_sum, int R,
                        int K, long P, void* workspace, size_t workspace_bytes, void* stream);
int sd_maskiou_loss_bwd(const float* iou_pred, const float* cls, const float* iou_target, const float* weight,
                        const float* weight_sum, float* d_iou_pred, int R, int K, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The CrowdHuman double-prediction head's training side (models/crowdhuman), fp32.
 *
 * sd_crowdhuman_target: RoI sampling and box targets.  mode 0 replaces the Python CustomOp `bbox_target`
 *   (models/crowdhuman/bbox_target.py: _sample_proposal :12-81, _expand_bbox_targets :84-104, forward :121-178),
 *   mode 1 `doublebbox_target` (models/crowdhuman/bbox_sec_target.py: _sample_proposal :13-120,
 *   _expand_bbox_targets :123-143, forward :159-224); IoU operator_py/cython/bbox.pyx:31-72, encoding
 *   operator_py/detectron_bbox_utils.py:192-223.  Both copy to the host, sample with np.random.choice and copy back.
 *   proposal (B,P,4) DEVICE, rows with y2 == 0 padding; gt_bbox (B,M,5) DEVICE [x1,y1,x2,y2,class], class -1
 *   padding, class -2 "ignore".  With add_gt_to_proposal every non-padding gt box (the ignore rows included) joins
 *   the candidates behind the valid proposals, in order.
 *   mt_state: the DEVICE int32[625] of sd_rpn_anchor_target, advanced in place exactly as numpy advances it, images in
 *     order: per image one permutation(n) for the foreground list and one for the background list, each only when
 *     its list is not empty (n == 1 draws nothing; n >= 2 draws whatever the number of rows taken, also 0: checked by
 *     running numpy).  The first `size` entries of a permutation are the rows, foreground first, then background.
 *   Matching.  mode 0: the ignore rows are dropped, first maximum over the rest, the label is that gt's class value.
 *     mode 1: the ignore rows stay in place with class -1; for cid = 1 .. num_reg_class - 1 with at least one gt:
 *     first maximum, and the first maximum after the winner is set to -1 (a class with one gt: second IoU -1, second
 *     box = that gt); a class takes over where its maximum is strictly greater than the running one, which starts
 *     at 0 (IoU 0 leaves class 0, gt row 0, second IoU 0).
 *   Sampling.  fg quota = round-half-even(fg_fraction * image_rois); fg: max >= fg_thresh; bg: bg_thresh_lo <= max <
 *     bg_thresh_hi.  The thresholds compare as numpy 2 compares them: in float32 in mode 0 (a float32 array against a
 *     python float), in double in mode 1 (the running maxima are float64 arrays).
 *   Outputs, S = image_rois: sampled_proposal (B,S,4), bbox_cls (B,S) (background rows 0), bbox_target /
 *     bbox_target_weight (B,S,4*num_reg_class): columns 4c .. 4c+3 of class c > 0 (c = label > 0 when num_reg_class
 *     == 2) hold the float32 encoding against the matched gt / ones, everything else +0.0.  mode 1 also
 *     bbox_sec_cls (the assigned class, 0 where the second IoU < fg_thresh), bbox_sec_target / _weight against the
 *     second gt; in mode 0 the three pointers are not used and may be NULL.  count (B) int32: rows filled; rows >=
 *     count[b] are +0.0 in every output (-1: the generator stalled, see csrc/mt19937.h; all rows are zero).
 *     The dx / dy columns reproduce numpy bit for bit; dw / dh go through logf, numpy's float32 log is not correctly
 *     rounded either: they agree to the last bits, not bit for bit.
 *   Preconditions the reference enforces by raising, NOT emulated here: at least one non-padding gt per image (mode
 *     0: one non-ignore gt; without one every candidate gets IoU 0, label 0), classes < num_reg_class (a larger one
 *     never matches in mode 1 and writes no target columns in mode 0), and every image filling all image_rois rows
 *     (its np.array stacking fails otherwise; here count reports the short image).
 *   Limits: P + M <= 4096 rows per image, 1 <= M <= 1024, image_rois <= 1024, 2 <= num_reg_class <= 1024.
 *   Four kernels, no memset node, no host synchronisation, graph-capturable, integer arithmetic only between
 *   workgroups; the workspace needs no clearing.
 * sd_emd_loss_fwd / _bwd: DoublePredBboxHead.emd_loss (models/crowdhuman/builder.py:254-306) with the CustomOp
 *   `softmax_entropy` (softmax_entropy_op.py:8-31) inside it.  R rows, K classes, D = 4 * num_reg_class columns.
 *     ce(x, y) = -logf(softmax(x)[(int)y] + 1e-10f), 0 when y names no column;  sl1 = MXNet's smooth_l1 with
 *     sigma = smooth_l1_scalar (0.5 sigma^2 v^2 for |v| <= 1 / sigma^2, |v| - 0.5 / sigma^2 beyond)
 *     L1 = ce(x1, y1) + ce(x2, y2) + sum_d (w1 sl1(d1 - t1) + w2 sl1(d2 - t2))
 *     L2 = ce(x1, y2) + ce(x2, y1) + sum_d (w2 sl1(d1 - t2) + w1 sl1(d2 - t1))
 *     loss[0] = sum_r min(L1, L2) / R;  pairing[r] (optional, may be NULL) = 1 when L1 <= L2, else 2 (a tie goes to
 *     the first pairing, as mx.sym.minimum's backward sends it to the left operand).
 *   The backward writes all four gradients once, only the winning pairing contributing, scaled by grad_scale / R:
 *     (softmax(x) - onehot(y)) for the two logits, w * sl1'(d - t) for the two deltas, with the labels / targets /
 *     weights the winning pairing gave each head.  It recomputes the pairing with the forward's code (equal bits).
 *   One launch each; the forward's sum has a fixed order (no float atomics): repeated calls and graph replay give
 *   equal bits; 4-byte alignment suffices and changes nothing.  R * max(K, D) <= 2^31 - 1 (SD_ERR_UNSUPPORTED beyond);
 *   R == 0 succeeds without a launch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int num_reg_class;
  int add_gt_to_proposal;
  int image_rois;
  double fg_fraction, fg_thresh, bg_thresh_hi, bg_thresh_lo;
  double bbox_target_std[4];
} sd_crowdhuman_target_param;
size_t sd_crowdhuman_target_workspace_bytes(int B, int P, int M);
int sd_crowdhuman_target(const float* proposal, const float* gt_bbox, int B, int P, int M, int mode,
                         const sd_crowdhuman_target_param* param_host, int32_t* mt_state,
                         float* sampled_proposal, float* bbox_cls, float* bbox_target, float* bbox_target_weight,
                         float* bbox_sec_cls, float* bbox_sec_target, float* bbox_sec_target_weight, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream);
int sd_emd_loss_fwd(const float* cls_logit, const float* cls_sec_logit, const float* cls_label,
                    const float* cls_sec_label, const float* bbox_delta, const float* bbox_sec_delta,
                    const float* bbox_target, const float* bbox_sec_target, const float* bbox_weight,
                    const float* bbox_sec_weight, int R, int K, int D, float smooth_l1_scalar, float* loss,
                    int32_t* pairing, void* stream);
int sd_emd_loss_bwd(const float* cls_logit, const float* cls_sec_logit, const float* cls_label,
                    const float* cls_sec_label, const float* bbox_delta, const float* bbox_sec_delta,
                    const float* bbox_target, const float* bbox_sec_target, const float* bbox_weight,
                    const float* bbox_sec_weight, int R, int K, int D, float smooth_l1_scalar, float grad_scale,
                    float* d_cls_logit, float* d_cls_sec_logit, float* d_bbox_delta, float* d_bbox_sec_delta,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_Quantization_int8  (mx.sym.contrib.Quantization_int8; utils/graph_optimize.py:attach_quantize_node puts
 *   one in front of the data and the weight of every Convolution / FullyConnected / Deconvolution), fp32.
 *   replaces Quantization_int8Op::Forward / Backward  operator_cxx/contrib/quantization_int8-inl.h:113-294 in the
 *   "minmax" mode without per-channel weights.  The tensor is n flat floats.
 *   minmax: float[1], the operator's auxiliary state.  state: int32[2] = {countdown, init}, created as
 *   {delay_quant, 1}: the reference keeps both in the Operator object, here they live on the device.
 *   Forward, per call:
 *     is_train && countdown > 0:  out = data (a copy), countdown -= 1, nothing else changes.
 *     otherwise quantise.  When is_train && !fix_act_scale, with m = max |data|:
 *         weight:                   minmax = m
 *         activation, init != 0:    minmax = m if (double)minmax < 1e-6, else unchanged;  init = 0
 *         activation, init == 0:    minmax = fl(fl(d * minmax) + fl((1.0f - d) * m)),  d = (float)ema_decay
 *       then t = minmax, u = t / 127 (one IEEE divide) and out = roundf(c / u) * u with c = x for weights (the
 *       reference does not clip them) and c = x clipped to [-t, t] for activations; a NaN x passes through;
 *       roundf rounds halves away from zero; c / u is a correctly rounded divide, the product a second rounding.
 *       With is_train == 0 neither minmax nor state changes and the call quantises whatever countdown is.
 *       t == 0 gives NaN everywhere, as the reference's arithmetic does.  A NaN in data during a training
 *       reduction is outside the contract (the reference's min / max reduce is not defined for it either).
 *     A clearing kernel (only when the reduction spans several workgroups) and two kernels; the host reads nothing
 *     back, so the call captures into a graph and replays with the state evolving on the device.  max |data| is
 *     the unsigned maximum of the floats' bit patterns: it does not depend on any order.  Calls that need no
 *     reduction (eval, fix_act_scale, a delay step) do not read data in the first kernel.  out may equal data.
 *   Backward, one kernel: grad_clip == 0 ("ste", and every weight): dgrad = ograd; data and minmax may be NULL.
 *     grad_clip != 0 ("clip"): dgrad = (-t <= x && x <= t) ? ograd : +0.0, t read from minmax on the device; a
 *     NaN x gives 0.  req: SD_REQ_WRITE, SD_REQ_ADD (dgrad += ...) or SD_REQ_NULL (nothing is launched).
 *   sd_quant_int8_weights_fwd: the weight forward above for T <= 1024 tensors in the same two kernels.  The five
 *     tables are DEVICE arrays of T entries (data, out, minmax and state pointers, element counts); n_total is
 *     the sum of the counts (it sizes the grids; every access is bounded by the counts themselves).  Outputs,
 *     minmax and state are bit-equal to T single calls.  A tensor of 0 elements is skipped, like n == 0 below.
 *   Pointers need 4-byte alignment only; 16-byte stores start at the output's first 16-byte boundary, inputs on
 *   another phase are loaded by 4-byte accesses, with equal bits.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: a null pointer, a negative count,
 *   ema_decay outside [0, 1] (NaN included), an unknown req; SD_ERR_WORKSPACE: a NULL or too small workspace
 *   (sd_quant_int8*_workspace_bytes; its content needs no clearing); SD_ERR_UNSUPPORTED: T > 1024 or more than
 *   2^40 elements.  n == 0 (T == 0, n_total == 0) returns 0 without touching the device or the state.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_quant_int8_workspace_bytes(long n);
int sd_quant_int8_fwd(const float* data, float* out, float* minmax, int* state, long n, int is_weight,
                      int is_train, int fix_act_scale, double ema_decay, void* workspace, size_t workspace_bytes,
                      void* stream);
int sd_quant_int8_bwd(const float* ograd, const float* data, const float* minmax, float* dgrad, long n,
                      int grad_clip, int req, void* stream);
size_t sd_quant_int8_weights_workspace_bytes(int T, long n_total);
int sd_quant_int8_weights_fwd(const float* const* data_ptrs, float* const* out_ptrs, float* const* minmax_ptrs,
                              int* const* state_ptrs, const long* counts, int T, long n_total, int is_train,
                              int fix_act_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FCOS training head (config/fcos_r50v1_fpn_1x.py), fp32
 *   sd_fcos_target replaces make_fcos_gt with its two Python CustomOps make_fcos_gt_preparation and
 *     prepare_fcos_cls_gt (models/FCOS/input.py:14-263);
 *   sd_fcos_loss_fwd / _bwd replace make_sigmoid_focal_loss, make_binary_cross_entropy_loss (loss and `grad`
 *     symbols, with the pass-through CustomOps compute_focal_loss / compute_bce_loss) and IoULoss
 *     (models/FCOS/loss.py:86-196), and the per-level reshape + concat in front of them (builder.py:207-214).
 *   Location grid: level l has len(range(0, data_h, stride_l)) x len(range(0, data_w, stride_l)) locations at
 *     index * stride + stride / 2; HW is their sum over the L <= SD_MAX_FPN_LEVELS levels
 *     (sd_fcos_num_locations: hw_levels_host, L entries, may be NULL).  Image 0's im_info decides for the whole
 *     batch, on the device: ori_h < ori_w takes the row-major grid, otherwise the transposed one
 *     (loc_x_T / loc_y_T), and the padding mask loc_x < ori_w && loc_y < ori_h is image 0's as well.
 *   sd_fcos_target: gt_bbox (N, M, 5) [x1, y1, x2, y2, cls], im_info (N, 3) ->
 *       centerness (N, HW), offset (N, 4, HW), cls_id (N, HW) int32: -1 = ignored (padding), 0 = background,
 *       1..K = class; cls_dense_or_null (N, K*HW): the reference's one-hot with ignore_label rows;
 *       state int32[4]: [0] = #(cls_id >= 1) = the reference's sum(labels * mask), [1] = #(centerness !=
 *       ignore_label && centerness > 0), [2] = the BITS of the float sum(centerness * [offset_left !=
 *       ignore_offset && centerness > 0]) (reduced in a fixed order), [3] = 0.  The three are the normalisers of
 *       the losses: they depend on the targets alone.
 *     Per box, in the reference's float32 order: l, t, r, b; in-box = min >= 0; the stage test lower <= greatest
 *     offset < upper on the offsets AFTER the in-box masking; box_size = (l + r) * (t + b), 1e10 when unassigned;
 *     the first minimum wins (ties: the lowest box index; nothing assigned: box 0, whose offsets are then
 *     ignore_offset); centerness = sqrt(min * min / (max * max)) * [left != ignore_offset] with IEEE divide and
 *     sqrt -- a degenerate box gives 0/0 = NaN on its own line, as the reference does.  The stage bounds are two
 *     HOST tables of L floats, or both NULL for the reference's [-1e-5, 64, 128, 256, 512] /
 *     [64, 128, 256, 512, 1e5] (L <= 5).  ignore_offset and ignore_label must be negative (an in-box offset
 *     is >= 0 and a label is 0 or 1; the reference uses -1 for both).  M > 128 is served in chunks.
 *   sd_fcos_loss_fwd / _bwd: three HOST tables of L device pointers -- class logits (N, K, H_l, W_l), centerness
 *     logits (N, 1, H_l, W_l), offset predictions (N, 4, H_l, W_l) after the graph's exp -- and hw_host, L sizes
 *     H_l * W_l whose sum is the targets' HW; L = 1 is the concatenated form.  The tables are read during the
 *     call only (they travel as kernel arguments).  losses: float[3] = centerness, classification, offset, the
 *     order of FCOSFPNHead.get_loss.  The backward writes (kWriteTo) three gradients per level in the logits' own
 *     shapes; it takes no top gradient (the reference's CustomOps ignore it, MakeLoss has grad_scale = 1).
 *       focal:  p = 1 / (1 + exp(-x)), log(clip(p, 1e-5, 1)), -x * [x >= 0] - log(1 + exp(-|x|)), pow by gamma,
 *               norm = state[0] + 1; the gradient is the reference's explicit `grad` expression.  alpha and
 *               gamma are doubles: (1 - alpha) is formed in double and rounded once, as the Python float is.
 *       BCE:    mask = label != ignore_label && label > 0, both logs clipped at 1e-5, normaliser state[1] + 1e-30,
 *               gradient (p - label) * mask / normaliser.
 *       IoU:    predictions clipped to [0, 1e4], mask = target_left != ignore_offset && centerness > 0,
 *               -log((I + 1) / (U + 1)) * centerness, normaliser state[2] + 1e-30; the gradient is the true
 *               derivative with respect to the unclipped prediction, zero outside [0, 1e4]; at pred == target
 *               the min hands its gradient to the prediction.
 *     Ignored locations get +0.0 in all three gradients.  The one-hot labels are never formed.  The sums run
 *     over the concatenated index order whatever L is, in a fixed order without float atomics: L = 5 and L = 1,
 *     two calls, and a graph replay give equal bits.  The class gradient moves in 16-byte items from each
 *     gradient row's first 16-byte boundary, with a scalar path for the ragged ends and for logits on another
 *     phase: any 4-byte aligned pointers give the same bits.
 *   Kernels only (no memset node), no host synchronisation, graph-capturable.  Workspaces need no clearing.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: a negative dimension, a null pointer, a NaN
 *   parameter, a stride < 1, M == 0; SD_ERR_WORKSPACE: a NULL or too small workspace; SD_ERR_UNSUPPORTED: L > 8,
 *   N * max(K, 4) * HW or N * M * 5 > 2^31 - 1, N > 65535 (sd_fcos_target: one grid row per image).  N == 0, K == 0 (losses) or HW == 0 succeed without a launch.
 * ---------------------------------------------------------------------------------------------- */
int sd_fcos_num_locations(int data_h, int data_w, const int* strides_host, int L, long* hw_levels_host,
                          long* hw_total_host);
size_t sd_fcos_target_workspace_bytes(int N, long HW);
int sd_fcos_target(const float* gt_bbox, const float* im_info, float* centerness, float* offset, int* cls_id,
                   float* cls_dense_or_null, int* state, int N, int M, int K, int data_h, int data_w,
                   const int* strides_host, const float* lower_host_or_null, const float* upper_host_or_null, int L,
                   float ignore_offset, float ignore_label, void* workspace, size_t workspace_bytes, void* stream);
size_t sd_fcos_loss_workspace_bytes(int N, int K, long HW);
int sd_fcos_loss_fwd(const float* const* cls_ptrs_host, const float* const* ctr_ptrs_host,
                     const float* const* off_ptrs_host, const long* hw_host, int L, const float* centerness,
                     const float* offset, const int* cls_id, const int* state, float* losses, int N, int K,
                     double alpha, double gamma, float ignore_offset, float ignore_label, void* workspace,
                     size_t workspace_bytes, void* stream);
int sd_fcos_loss_bwd(const float* const* cls_ptrs_host, const float* const* ctr_ptrs_host,
                     const float* const* off_ptrs_host, float* const* dcls_ptrs_host, float* const* dctr_ptrs_host,
                     float* const* doff_ptrs_host, const long* hw_host, int L, const float* centerness,
                     const float* offset, const int* cls_id, const int* state, int N, int K, double alpha,
                     double gamma, float ignore_offset, float ignore_label, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FCOS test-time decode (config/fcos_r50v1_fpn_1x.py), fp32: FCOSFPNHead.get_all_proposal
 * (models/FCOS/builder.py:234-259) in ONE call -- the ten sigmoid nodes (input_logits = 1), the five Python
 * CustomOps get_proposal_single_stage (models/FCOS/utils.py:7-94), the concat and the Python CustomOp
 * get_batch_proposal (utils.py:99-149).  Additions only: the ABI version stays 12.
 *   Inputs: three HOST tables of L device pointers (the convention of sd_fcos_loss_fwd; read during the call
 *     only) -- cls (N, C, H_l, W_l), ctr (N, 1, H_l, W_l), off (N, 4, H_l, W_l) -- im_info (N, 3) [h, w, scale] ON
 *     THE DEVICE, three HOST tables of L ints (H_l, W_l, stride_l).  input_logits = 0: cls and ctr are
 *     probabilities (the CustomOps' own contract); 1: raw logits, 1.0f / (1.0f + expf(-x)) is applied first, the
 *     expression sd_fcos_sigmoid computes element-wise (equal bits).
 *   Outputs, R = L * top_n, every element written by every call: bbox (N, R, 4), score (N, R, 81), cls_id (N, R),
 *     and stage_out (N, R, 6) or NULL = the concat of the per-level rows [cls, fused, x1, y1, x2, y2] (builder.py:255).
 *   Per level and image (the reference is the spec, quirks included):
 *     cand = cls > thresh (float32; equality is no candidate), fused = cls * ctr (float32)       utils.py:17-19
 *     count(cand) >= top_n: the top_n best of ALL C*H*W fused scores, descending;                 utils.py:32-36
 *       flat idx = (c*H + y)*W + x, cls = c + 1 (integer arithmetic; the reference's float32 idx is exact up to
 *       2^24, beyond that SD_ERR_UNSUPPORTED)
 *     0 < count < top_n: the candidates in ascending flat index order; count == 0: nothing        utils.py:38-46
 *     cx = x*stride + stride/2, x1 = clip(cx - off[0], 0, img_w), y1 = clip(cy - off[1], 0, img_h),
 *       x2 = clip(cx + off[2], 0, img_w), y2 = clip(cy + off[3], 0, img_h)                          utils.py:49-55
 *     "remove small bboxes" works on the 6-column row: (cls >= x1) && (fused >= y1) turns the row into six -1
 *                                                                                                 utils.py:61-64
 *     rows past the selected ones are -1                                                          utils.py:22,66
 *   Per image: rows in descending order of fused; bbox = columns 2..5, cls_id = column 0, score zero except
 *     score[i, r, int(cls_r)] = sqrtf(clip(fused_r, 1e-20f, 1)) for EVERY row -- cls = -1 (padding, masked)
 *     indexes the LAST column, so column 80 of such rows holds sqrt(float32(1e-20)); column 0 is never written
 *     by a real row (utils.py:110-124).  81 is the reference's constant: C > 80 is SD_ERR_UNSUPPORTED.
 *   Ties (the project's choice; MXNet's order among equal keys is not documented): inside a level the lower flat
 *     index first, in the batch sort stable in concat order (the lower level first); -0.0 == +0.0.
 *   NaN (not part of the contract): a NaN cls is no candidate; NaN fused scores are ordered by their bits
 *     (positive NaN before +inf, negative NaN after -inf); NaN offsets give NaN coordinates and never mask a row.
 *   No host read of device data, no allocation, no float atomics, kernels only (the counters are cleared by a
 *   kernel of the call): equal bits between calls and under graph replay.  Loads are scalar: any 4-byte aligned
 *   tensor pointer works.  The workspace needs no clearing, must be 16-byte aligned and hold
 *   sd_fcos_decode_workspace_bytes(N, C, L, hw_host, top_n) bytes, hw_host = L sizes H_l * W_l.
 *   SD_ERR_INVALID_ARG: L outside 1..8, top_n < 1, C < 1, N < 0, a level size or stride < 1, a NaN threshold,
 *   input_logits outside {0, 1}, a null pointer, a misaligned workspace; SD_ERR_UNSUPPORTED: C > 80,
 *   C*H_l*W_l > 2^24, L*top_n > 16384, N > 65535; SD_ERR_WORKSPACE: a NULL or too small workspace.  N == 0
 *   succeeds without a launch (the query then returns 256, as it does for invalid dimensions).
 *   sd_fcos_sigmoid: p[i] = 1.0f / (1.0f + expf(-x[i])), n elements.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_fcos_decode_workspace_bytes(int N, int C, int L, const long* hw_host, int top_n);
int sd_fcos_decode(const float* const* cls_ptrs_host, const float* const* ctr_ptrs_host,
                   const float* const* off_ptrs_host, const float* im_info, const int* H_host, const int* W_host,
                   const int* stride_host, int L, int N, int C, int top_n, float pre_nms_thresh, int input_logits,
                   float* bbox, float* score, float* cls_id, float* stage_out, void* workspace,
                   size_t workspace_bytes, void* stream);
int sd_fcos_sigmoid(const float* x, float* p, long n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RepPoints training head (config/RepPoints/), fp32.  Additions only: the ABI version stays 12.
 *   sd_reppoints_target replaces _gen_points, _offset_to_boxes and both _point_target calls of
 *     RepPointsHead.get_loss (models/RepPoints/builder.py:328-388, models/RepPoints/point_ops.py:18-216);
 *   sd_reppoints_box_loss_fwd / _bwd replace _offset_to_pts, _points2bbox, the per-level concat, smooth_l1, the
 *     weight product, BBoxNorm and MakeLoss of both box branches (builder.py:415-481).
 *   Levels: three HOST tables of L ints (H_l, W_l, stride_l) and HOST tables of L device pointers to the point maps
 *     (N, 2 * num_points, H_l, W_l), channels (y0, x0, y1, x1, ...); the tables are read during the call only.
 *     P = sum H_l * W_l; point j = (level, h, w) in the reference's concat order, at (w * stride, h * stride);
 *     its level is floor(log2(stride)); lvl_min / lvl_max come from the strides passed.  An empty level is skipped.
 *   transform: 0 = minmax, 1 = partial_minmax (the first four points), 2 = moment (moment_transfer (2,) on the
 *     device: the half extents are std * exp(moment_transfer[0]) in x and std * exp(moment_transfer[1]) in y;
 *     may be NULL for 0 and 1).  Sums over the points of a set run sequentially in point order, the mean is the
 *     sum / num_points, the deviation sqrt(mean((v - mean)^2)).
 *   sd_reppoints_target: pts_init maps, gt_bbox (N, M, 5) [x1, y1, x2, y2, cls] ->
 *       label_init (N, P), gt_init (N, P, 4): the point assigner (point_ops.py:67-137).  A gt is valid if cls > 0;
 *         centre ((l + r) / 2, (t + b) / 2), w, h = max(r - l, 1e-6), max(b - t, 1e-6), level
 *         floor((log2(w / target_scale) + log2(h / target_scale)) / 2) clipped to the point levels; the distance of a
 *         point of that level is sqrt(dx * dx + dy * dy) of (point - centre) / (w, h); per valid gt the num_pos
 *         smallest distances survive (ties: the lower flat point index), per point the gt of least surviving
 *         distance wins (ties: the lower gt index): label = its cls, gt = its box; elsewhere label = -1, gt = 0.
 *       label_refine (N, P), gt_refine (N, P, 4): the IoU assigner (point_ops.py:140-175) on the init boxes
 *         centre + stride * _points2bbox(raw offsets) (in this order).  box_iou, corner format, no +1: extents
 *         clamped at 0, inter / (area_a + area_b - inter), 0 where the union is <= 0.  Per box the FIRST arg-max
 *         over the M rows (padding rows included) and the max; per gt the max over the P boxes of its image;
 *         assigned = -1; 0 where max < neg_iou_thr; 1 where some gt has iou == its column max and that column max >
 *         min_pos_iou; 1 where max >= pos_iou_thr; label = cls[argmax] where assigned > 0 else assigned,
 *         gt = box[argmax] where assigned > 0 else 0.
 *       state int32[4]: [0] = #(label_init >= 1), [1] = #(label_refine >= 1) over the batch, [2], [3] = the BITS
 *         of the floats [0] + 1 and [1] + 1, the BBoxNorm denominators (bbox_norm-inl.h:116-122).
 *     The weights are label > 0 and are not materialised.  Every output is bit-reproducible (integer atomics only).
 *   sd_reppoints_box_loss_fwd: per stage, points = pred * stride + centre after the (y, x) -> (x, y) flip, box =
 *     _points2bbox of those absolute points, loss = smooth_l1((box - gt) / (stride * scale), sigma 3) * [label > 0]
 *     -> loss_init, loss_refine (N, P, 4).
 *   sd_reppoints_box_loss_bwd: no top gradient; the head gradient is grad_scale / state denominator, taken back
 *     through the weight, smooth-L1, the normaliser and the transform (min / max: EVERY tied point takes the
 *     gradient; moment: the chain rule of the expressions as written, so a set of coincident points, std = 0,
 *     gives NaN) into HOST tables of gradient maps shaped like the inputs, req = 1 (write) or 3 (add), and into
 *     d_moment_transfer (2,) (same req; 0 for minmax / partial_minmax), summed over both stages from
 *     per-workgroup partials in a fixed order.
 *   Kernels only, no allocation, no host synchronisation, graph-capturable; workspaces need no clearing; any
 *   4-byte aligned tensor pointer works.  Checked before anything touches the device -- SD_ERR_INVALID_ARG: a
 *   negative dimension, a null pointer or table, a NaN or non-positive scale, a NaN threshold, a stride < 1, an
 *   unknown transform or req, partial_minmax with fewer than 4 points, M == 0; SD_ERR_UNSUPPORTED: L > 8,
 *   M > 128, num_pos outside 1..16, num_points not in {1, 9, 25}, N > 65535, N * 2 * num_points * P > 2^31 - 1, a
 *   coordinate beyond 2^24; SD_ERR_WORKSPACE: a NULL or too small workspace.  N == 0 or P == 0 succeed without a
 *   launch.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_reppoints_target_workspace_bytes(int N, int M, long P);
int sd_reppoints_target(const float* const* pts_init_ptrs_host, const int* H_host, const int* W_host,
                        const int* stride_host, int L, const float* gt_bbox, const float* moment_transfer_or_null,
                        float* label_init, float* gt_init, float* label_refine, float* gt_refine, int* state, int N,
                        int M, int num_points, int transform, float target_scale, int num_pos, float pos_iou_thr,
                        float neg_iou_thr, float min_pos_iou, void* workspace, size_t workspace_bytes, void* stream);
int sd_reppoints_box_loss_fwd(const float* const* pts_init_ptrs_host, const float* const* pts_refine_ptrs_host,
                              const int* H_host, const int* W_host, const int* stride_host, int L,
                              const float* moment_transfer_or_null, const float* label_init, const float* gt_init,
                              const float* label_refine, const float* gt_refine, float* loss_init,
                              float* loss_refine, int N, int num_points, int transform, float scale, void* stream);
size_t sd_reppoints_box_loss_workspace_bytes(int N, long P);
int sd_reppoints_box_loss_bwd(const float* const* pts_init_ptrs_host, const float* const* pts_refine_ptrs_host,
                              const int* H_host, const int* W_host, const int* stride_host, int L,
                              const float* moment_transfer_or_null, const float* label_init, const float* gt_init,
                              const float* label_refine, const float* gt_refine, const int* state,
                              float* const* d_init_ptrs_host, float* const* d_refine_ptrs_host,
                              float* d_moment_transfer, int N, int num_points, int transform, float scale,
                              float grad_scale_init, float grad_scale_refine, int req, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RepPoints test-time decode (config/RepPoints/), fp32: RepPointsHead.get_prediction
 * (models/RepPoints/builder.py:486-576) in ONE call -- per level the transposes, the sigmoid (input_logits = 1), the
 * max, the topk and the per-image take / scale / add / clip chains, then the padded column and the concat of the
 * levels.  Additions only: the ABI version stays 12.
 *   Inputs: two HOST tables of L device pointers (the convention of sd_fcos_decode; read during the call only) --
 *     cls (N, C, H_l, W_l) and pts_out_refine (N, 2 * num_points, H_l, W_l), channels (y0, x0, y1, x1, ...) --
 *     im_info (N, 3) [h, w, scale] and moment_transfer (2,) ON THE DEVICE (moment_transfer may be NULL unless
 *     transform = 2), four HOST tables of L ints: H_l, W_l, stride_l and k_l, the rows kept of the level; k_l <= 0
 *     keeps all H_l * W_l (MXNet's topk with k < 1).  The reference's rule k_l = pre_nms_top_n if stride <= 32 else
 *     -1 (builder.py:499-502) belongs to the caller.  input_logits = 0: cls holds probabilities; 1: raw logits,
 *     1.0f / (1.0f + expf(-x)) is applied to every element first, the expression sd_fcos_sigmoid computes (equal
 *     bits); the sigmoid is never taken of a maximum logit.
 *   Outputs, K_l = k_l > 0 ? k_l : H_l * W_l, R = sum K_l, every element written by every call:
 *     cls_score (N, R, C + 1) and bbox_xyxy (N, R, 4).
 *   Per level l and image i, p = y * W_l + x, s = stride_l (the reference is the spec):
 *     score[p, c] = cls[i, c, y, x] or its sigmoid; m[p] = max over c                          builder.py:518-519
 *     the K_l best m in descending order; rank r is output row (sum of K_l' over l' < l) + r: the levels are
 *       concatenated in the order given, there is NO batch sort                                builder.py:520,569-574
 *     cls_score[i, row, 0] = 0, cls_score[i, row, 1 + c] = score[p, c]                          builder.py:559-562
 *     box = _points2bbox(pts, transform, y_first=True) at p: 0 = minmax over all points, 1 = partial_minmax over
 *       the first four, 2 = moment: mean +- sqrt(mean((v - mean)^2)) * expf(moment_transfer[0 for x, 1 for y]),
 *       sums sequential in point order -- the expressions of the training head (sd_reppoints_*)  point_ops.py:219-274
 *     b = box * s + (x*s, y*s, x*s, y*s): a float32 product, then a float32 add                 builder.py:541
 *     bbox_xyxy = max(min(b, lim), 0), lim = im_info[i, 1] - 1 for x and im_info[i, 0] - 1 for y builder.py:545-548
 *   Ties (the project's choice; MXNet's order among equal keys is not documented): the lower p first;
 *     -0.0 == +0.0.  NaN (not part of the contract): a NaN maximum is ordered by its bits.
 *   No host read of device data, no allocation, no float atomics, no counter to clear, kernels only: equal bits between
 *   calls and under graph replay.  Loads are scalar: any 4-byte aligned tensor pointer works.  The workspace needs
 *   no clearing, must be 16-byte aligned and hold sd_reppoints_decode_workspace_bytes(N, C, L, hw_host, k_host)
 *   bytes, hw_host = L sizes H_l * W_l.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: L outside 1..8, C < 1, N < 0,
 *   num_points < 1, num_points < 4 with partial_minmax, a level size or stride < 1, k_l > H_l * W_l, transform
 *   outside 0..2, moment with a NULL moment_transfer, input_logits outside {0, 1}, a null pointer, a misaligned
 *   workspace; SD_ERR_UNSUPPORTED: K_l > 16384, H_l * W_l > 2^24, N > 65535, N * R * (C + 1) or N * C * H_l * W_l
 *   above 2^31 - 1; SD_ERR_WORKSPACE: a NULL or too small workspace.  N == 0 succeeds without a launch (the query
 *   then returns 256, as it does for invalid dimensions).
 * ---------------------------------------------------------------------------------------------- */
size_t sd_reppoints_decode_workspace_bytes(int N, int C, int L, const long* hw_host, const int* k_host);
int sd_reppoints_decode(const float* const* cls_ptrs_host, const float* const* pts_ptrs_host, const float* im_info,
                        const float* moment_transfer, const int* H_host, const int* W_host, const int* stride_host,
                        const int* k_host, int L, int N, int C, int num_points, int transform, int input_logits,
                        float* cls_score, float* bbox_xyxy, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_BroadcastScale and the merged-BN affine  (mx.sym.contrib.BroadcastScale; what
 *   utils/graph_optimize.py:merge_bn puts behind every Convolution of a fixbn backbone: BroadcastScale(gamma) ->
 *   broadcast_add(beta) [-> elemwise add of the shortcut] -> relu), fp32 and fp16, NCHW.  Additions only: the ABI
 *   version stays 12.
 *   replaces BroadcastScaleOp::Forward / Backward  operator_cxx/contrib/broadcast_scale-inl.h:57-103 and the
 *   upstream broadcast_add, elemwise add and relu nodes behind it (two to four launches each way, every one
 *   reading and writing the whole activation) by one launch each way.
 *   x / residual / y / dy / dx / dres (N,C,HxW) contiguous, gamma / beta / dbeta (C).
 *   sd_scale_bias_act_fwd, per element of plane (n, c), every step rounded on its own (no fused multiply-add):
 *       t = x * gamma[c];  u = t + beta[c] (beta NULL: u = t);  v = u + residual (residual NULL: v = u);
 *       y = act ? (v > 0 ? v : 0) : v            mshadow_op::relu: NaN and -0.0 give +0.0
 *     _contrib_BroadcastScale itself is beta = residual = NULL, act = 0.
 *   sd_scale_bias_act_bwd (y is read only under act, x never):
 *       g1 = act ? dy * (y > 0 ? 1 : 0) : dy     the product form: an infinite dy over a dead unit gives NaN
 *       dres = g1 (NULL: skipped);  dx = g1 * gamma[c];  dbeta[c] = sum over n, hw of g1 (NULL: skipped; float32)
 *     dx, dres and dbeta are written (kWriteTo).  There is no gradient for gamma: the reference's Backward writes
 *     none (:83-103).
 *   The *_f16 entry points take halves for every tensor but dbeta; each step above is the float operation on the
 *   half operands rounded once to half (round to nearest even) before the next step -- mshadow's half_t and numpy's
 *   float16 arithmetic -- and dbeta sums the half g1 values in float32.
 *   y may be x or residual; dx and dres may each be dy: an element depends on its own index only.
 *   Pointers need element alignment only.  16-byte stores from the first 16-byte boundary of y (dx), a capped grid
 *   of 2048 workgroups striding the rest; an input (or dres) on another phase is moved by element accesses; the
 *   bits do not depend on any pointer's phase.  dbeta is a two-stage sum in a fixed order through the workspace
 *   (sd_scale_bias_act_workspace_bytes, monotone in N and C, no clearing needed; only a call with dbeta != NULL
 *   looks at it): no floating-point atomics, two calls give equal bits.  sd_last_dispatch() names the kernels
 *   taken, the grid and the tile count.  Kernels only, no host synchronisation, graph-capturable.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: a negative size, act outside {0, 1}, a null
 *   x / gamma / y (dy / gamma / dx), y == NULL with act = 1 in the backward, a pointer off its element alignment;
 *   SD_ERR_WORKSPACE: dbeta != NULL with a NULL or too small workspace; SD_ERR_UNSUPPORTED: N*C*HxW > 2^31 - 1
 *   elements.  N = 0, C = 0 or HxW = 0 succeed without a launch (no pointer is looked at, nothing is written;
 *   sd_scale_bias_act_workspace_bytes returns its minimum for them and for invalid sizes).
 * ---------------------------------------------------------------------------------------------- */
size_t sd_scale_bias_act_workspace_bytes(int N, int C, long HxW);
int sd_scale_bias_act_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                          int N, int C, long HxW, int act, void* stream);
int sd_scale_bias_act_bwd(const float* dy, const float* y, const float* gamma, float* dx, float* dres, float* dbeta,
                          int N, int C, long HxW, int act, void* workspace, size_t workspace_bytes, void* stream);
int sd_scale_bias_act_fwd_f16(const void* x, const void* gamma, const void* beta, const void* residual, void* y,
                              int N, int C, long HxW, int act, void* stream);
int sd_scale_bias_act_bwd_f16(const void* dy, const void* y, const void* gamma, void* dx, void* dres, float* dbeta,
                              int N, int C, long HxW, int act, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * The Faster / Mask R-CNN loss heads (config/faster_r50v1_fpn_1x.py and its family), fp32: RpnHead.get_loss
 *   (symbol/builder.py:163-206), FPNRpnHead.get_loss (models/FPN/builder.py:156-237) and BboxHead.get_loss
 *   (symbol/builder.py:405-446) -- SoftmaxOutput, smooth_l1 behind MakeLoss, and the four numbers the AccWithIgnore
 *   and L1 metrics (core/detection_metric.py:40-66,134-156) compute.  Additions only: the ABI version stays 12.
 *   Upstream's SoftmaxOutput, smooth_l1 and MakeLoss are not vendored with the reference; DESIGN 4.23 is the
 *   specification and says what rests on memory of upstream.
 *   Softmax row: m = max x, e_c = expf(x_c - m), s = sum e_c, p_c = e_c / s (IEEE divide).
 *   Class gradient: (p_c - [c == (int)label]) * (cls_grad_scale / (float)max(1, state.valid)); a row whose
 *     (int)label equals ignore_label (RPN only) gets zeros; a label outside [0, C) hits no class.
 *   Box part: v = delta - target; reg_loss = weight * smooth_l1(v, sigma) (a product: weight 0 against a NaN delta
 *     gives NaN); d_delta = smooth_l1'(v) * (weight * reg_grad_scale).
 *   State block, int32[4] on the device, written by every forward: {valid, correct, fg, reg_sum (the bits of a
 *     float)} -- valid: labels != ignore (RPN), R (R-CNN); correct: valid rows whose first arg-max over p equals
 *     (int)label; fg: valid rows with (int)label != 0; reg_sum: the sum of reg_loss in a fixed order (per-workgroup
 *     partials in the workspace, then one workgroup), so two calls and a graph replay give equal bits.  The words
 *     of a half that is not computed are 0.
 *   sd_rpn_loss_fwd / _bwd: two HOST tables of L <= SD_MAX_FPN_LEVELS device pointers (the convention of
 *     sd_fcos_loss_fwd; read during the call only) -- cls_logit[l] (N, 2A, H_l, W_l), bbox_delta[l]
 *     (N, 4A, H_l, W_l) -- and hw_host, the L sizes H_l * W_l with sum HW; cls_label (N, A * HW), reg_target and
 *     reg_weight (N, 4A, HW): sd_rpn_anchor_target's layout 1.  The label of level l, anchor a, position p is at
 *     a * HW + off_l + p, its logits are channels a and A + a of the level.  prob (N, 2, A, HW) and reg_loss
 *     (N, 4A, HW) are in the reference's concat layout; either may be NULL (not stored).  A NULL cls table
 *     (delta table) leaves that half out altogether, its inputs are not looked at.  The forward is one launch and
 *     one finishing workgroup; the backward one launch that writes every level's gradients, a half whose gradient
 *     table is NULL left out.  L = 1 is the C4 head.
 *   sd_rcnn_loss_fwd / _bwd: cls_logit (R, K), cls_label (R,), bbox_delta / bbox_target / bbox_weight (R, D); a wave
 *     per row.  normalization = 'batch': the backward's normaliser is the state's valid = R.  NULL cls_logit
 *     (bbox_delta) in the forward, NULL d_cls_logit (d_bbox_delta) in the backward leave the half out.
 *   No memset, no host read, graph-capturable.  Pointers need element alignment only.
 *   SD_ERR_INVALID_ARG: L outside 1..8, A < 1, K < 1, a negative size, sigma <= 0, a fractional ignore_label, a
 *   null pointer of a computed half, neither half given; SD_ERR_UNSUPPORTED: K > 1024, more than 2^31 - 1
 *   elements; SD_ERR_WORKSPACE: a NULL or too small workspace (forward only).  An empty problem succeeds without
 *   a launch and writes nothing.
 * ---------------------------------------------------------------------------------------------- */
size_t sd_rpn_loss_workspace_bytes(int N, int A, long HW);
size_t sd_rcnn_loss_workspace_bytes(int R);
int sd_rpn_loss_fwd(const float* const* cls_ptrs_host, const float* const* delta_ptrs_host, const long* hw_host,
                    int L, const float* cls_label, const float* reg_target, const float* reg_weight, int N, int A,
                    float ignore_label, float sigma, float* prob, float* reg_loss, int32_t* state, void* workspace,
                    size_t workspace_bytes, void* stream);
int sd_rpn_loss_bwd(const float* const* cls_ptrs_host, const float* const* delta_ptrs_host, const long* hw_host,
                    int L, const float* cls_label, const float* reg_target, const float* reg_weight, int N, int A,
                    float ignore_label, float sigma, float cls_grad_scale, float reg_grad_scale,
                    const int32_t* state, float* const* dcls_ptrs_host, float* const* ddelta_ptrs_host,
                    void* stream);
int sd_rcnn_loss_fwd(const float* cls_logit, const float* cls_label, const float* bbox_delta,
                     const float* bbox_target, const float* bbox_weight, int R, int K, int D, float sigma,
                     float* prob, float* reg_loss, int32_t* state, void* workspace, size_t workspace_bytes,
                     void* stream);
int sd_rcnn_loss_bwd(const float* cls_logit, const float* cls_label, const float* bbox_delta,
                     const float* bbox_target, const float* bbox_weight, int R, int K, int D, float sigma,
                     float cls_grad_scale, float reg_grad_scale, const int32_t* state, float* d_cls_logit,
                     float* d_bbox_delta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * _contrib_SyncBatchNorm  (mx.sym.contrib.SyncBatchNorm; every normalizer_factory(type="syncbn") site), fp32 and
 *   fp16, NCHW.  Additions only: the ABI version stays 12.
 *   replaces SyncBatchNorm::Forward / Backward  operator_cxx/contrib/sync_batch_norm-inl.h:246-535 (three to
 *   five tensor passes, two device-to-host copies, a host barrier and a host-side add, two copies back, per layer
 *   and direction: :325-351, :464-494) by two entry points per direction with the exchange of a (2, C) float32
 *   block between them.  The exchange itself is the caller's (simpledet_amd/dist.py:all_gather_stats); with one
 *   rank there is none.
 *   x / y / dy / dx (N,C,HxW) contiguous (2-D data: HxW = 1); gamma / beta / mean / var / moving_* / dgamma / dbeta
 *   (C) float32.  n = N * HxW, the same on each of the W ranks (SharedND::MeanReady divides by ndev, :146-158).
 *   g = fix_gamma ? 1 : gamma[c].  Every float32 step is rounded on its own.
 *   Training forward:
 *     sd_sync_bn_stats      part (2,C): part[0,c] = the mean of the rank's n elements, part[1,c] = their biased
 *                           variance about that mean.  x is read once.
 *     sd_sync_bn_apply      parts (W,2,C) in rank order (W = 1: parts is part).  Per channel in double, ranks in
 *                           order: m = (sum_r mean_r) / W;  v = (sum_r (var_r + (mean_r - m)^2)) / W;
 *                           mean = (float)m, var = (float)v, both written (W = 1: the bits of part).  Then
 *                           inv = 1.0f / sqrtf(var + eps);  y = (g * (x - mean)) * inv + beta[c]        (:354-357)
 *   Inference forward, sd_sync_bn_infer_fwd (:359-363):
 *       a = g / sqrtf(moving_var + eps);  b = beta - (g * moving_mean) / sqrtf(moving_var + eps);  y = a * x + b
 *   Training backward:
 *     sd_sync_bn_bwd_stats  bpart (2,C): bpart[0,c] = sum dy, bpart[1,c] = sum dy * (x - mean)           (:476-477)
 *     sd_sync_bn_bwd_apply  bparts (W,2,C).  Per channel in double, ranks in order: SG = sum_r bpart_r[0],
 *                           SP = sum_r bpart_r[1];  sg = (float)(SG / (W * n)), sp = (float)(SP / (W * n));
 *                           inv = 1.0f / sqrtf(var + eps);  a = g * inv;  b = -(g * sp) * ((inv * inv) * inv);
 *                           c = -(g * sg) * inv;  dx = (dy * a + b * (x - mean)) + c
 *                           (:496-513 with its averaged sums and scale = 1 / n multiplied out).
 *                           dbeta[c] = bparts[rank][0][c];  dgamma[c] = fix_gamma ? 0 : bparts[rank][1][c] * inv
 *                           -- per rank, as the reference: the gradient all-reduce sums them.  NULL together: skipped.
 *                           moving_mean / moving_var (NULL together: skipped) are updated HERE, in the backward, with
 *                           the biased variance, as :471-472: moving = moving * momentum + stat * (1.0f - momentum).
 *   Departures from the reference: (1) the variance is taken about the mean (its fp32 E[x^2] - mean^2, :333-334 and
 *   :353, cancels when |mean| >> sigma); (2) y multiplies by inv where the reference divides per element; (3) dgamma
 *   is (sum dy * (x - mean)) * inv where the reference sums dy * (x - mean) / sqrt(var + eps) (:503); (4) gamma is
 *   never written (the reference's slope = 1.f under fix_gamma stores ones into the input, :320).  Not provided:
 *   kAddTo, the backward under use_global_stats, gradients arriving on mean / var.
 *   The *_f16 entry points take halves for x / y / dy / dx and compute in float32, rounding the result to half once:
 *   the bits of cast -> the fp32 entry point -> cast.
 *   Sums are defined on items of 8 (HxW % 8 == 0), 4 (HxW % 4 == 0) or 1 elements, whatever the element type and
 *   the pointers; 16-byte accesses where the data pointers are 16-byte aligned, element accesses otherwise
 *   (element alignment suffices; no bit depends on it).  A channel of more than 256 * 8 items (256 * 4 of 8) is
 *   split over workgroups and its partials are merged in double in a fixed order; sd_last_dispatch() says
 *   "(split)" then.  No floating-point atomics: two calls give equal bits.  The workspace
 *   (sd_sync_bn_workspace_bytes, one size for every entry point, monotone in N and C) needs no clearing.  Kernels
 *   only, no host read, graph-capturable; every grid depends on the shapes alone.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: a negative size, W < 1, rank outside
 *   0..W-1, dgamma / dbeta or moving_mean / moving_var given half, a null pointer, a pointer off its element
 *   alignment; SD_ERR_WORKSPACE: a NULL or too small workspace; SD_ERR_UNSUPPORTED: N*C*HxW > 2^31 - 1.  N = 0,
 *   C = 0 or HxW = 0 succeed without a launch (nothing is written; the query returns its minimum).
 * ---------------------------------------------------------------------------------------------- */
size_t sd_sync_bn_workspace_bytes(int N, int C, long HxW);
int sd_sync_bn_stats(const float* x, float* part, int N, int C, long HxW, void* workspace, size_t workspace_bytes,
                     void* stream);
int sd_sync_bn_apply(const float* x, const float* parts, int W, const float* gamma, const float* beta, float* y,
                     float* mean, float* var, int N, int C, long HxW, float eps, int fix_gamma, void* workspace,
                     size_t workspace_bytes, void* stream);
int sd_sync_bn_infer_fwd(const float* x, const float* gamma, const float* beta, const float* moving_mean,
                         const float* moving_var, float* y, int N, int C, long HxW, float eps, int fix_gamma,
                         void* stream);
int sd_sync_bn_bwd_stats(const float* dy, const float* x, const float* mean, float* bpart, int N, int C, long HxW,
                         void* workspace, size_t workspace_bytes, void* stream);
int sd_sync_bn_bwd_apply(const float* dy, const float* x, const float* mean, const float* var, const float* gamma,
                         const float* bparts, int W, int rank, float* dx, float* dgamma, float* dbeta,
                         float* moving_mean, float* moving_var, float momentum, int N, int C, long HxW, float eps,
                         int fix_gamma, void* workspace, size_t workspace_bytes, void* stream);
int sd_sync_bn_stats_f16(const void* x, float* part, int N, int C, long HxW, void* workspace,
                         size_t workspace_bytes, void* stream);
int sd_sync_bn_apply_f16(const void* x, const float* parts, int W, const float* gamma, const float* beta, void* y,
                         float* mean, float* var, int N, int C, long HxW, float eps, int fix_gamma, void* workspace,
                         size_t workspace_bytes, void* stream);
int sd_sync_bn_infer_fwd_f16(const void* x, const float* gamma, const float* beta, const float* moving_mean,
                             const float* moving_var, void* y, int N, int C, long HxW, float eps, int fix_gamma,
                             void* stream);
int sd_sync_bn_bwd_stats_f16(const void* dy, const void* x, const float* mean, float* bpart, int N, int C, long HxW,
                             void* workspace, size_t workspace_bytes, void* stream);
int sd_sync_bn_bwd_apply_f16(const void* dy, const void* x, const float* mean, const float* var, const float* gamma,
                             const float* bparts, int W, int rank, void* dx, float* dgamma, float* dbeta,
                             float* moving_mean, float* moving_var, float momentum, int N, int C, long HxW, float eps,
                             int fix_gamma, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The FPN top-down pathway  (UpSampling(scale=2, sample_type=nearest) -> slice_like(., lateral) -> add_n with two
 *   inputs: the merge every FPN-style neck of the reference builds per level, models/FPN/builder.py:444-524,
 *   models/retinanet/builder.py:498-543, models/FCOS/builder.py:338-386, ...), fp32 and fp16, NCHW.  Additions
 *   only: the ABI version stays 12.  The three operators are upstream MXNet's; their arithmetic is restated here.
 *   replaces three nodes forward and three backward per level, each reading and writing a whole tensor and keeping
 *   the up-sampled and the clipped intermediate alive for the backward, by one launch each way for the whole chain.
 *   Level 0 is the coarsest; 2 <= L <= 6.  hs / ws (host, L entries) are the levels' heights and widths; every
 *   tensor of level l is (N,C,hs[l],ws[l]) contiguous.  lateral / out / g / d_lateral are HOST tables of L - 1 device
 *   pointers, entry k for level k + 1.
 *   sd_fpn_topdown_fwd:  out_l[n,c,y,x] = p_{l-1}[n,c,y>>1,x>>1] + lateral_l[n,c,y,x],  p_0 = top, p_l = out_l
 *     -- the crop from the origin that slice_like makes; hs[l] <= 2 hs[l-1] and ws[l] <= 2 ws[l-1] are required, and
 *     the crop may take more than one row or column.
 *   sd_fpn_topdown_bwd (needs no forward tensor):  D_{L-1} = g_{L-1};  D_l = g_l + S_l (l = L-2 .. 1);  d_top = S_0;
 *     d_lateral_l = D_l.  S_l[i,j] starts at +0.0f and adds D_{l+1}[2i+a, 2j+b] in the order (a,b) = (0,0), (0,1),
 *     (1,0), (1,1), a position at or beyond hs[l+1], ws[l+1] left out (mshadow's pool<red::sum>, the backward of
 *     upstream's UpSampling, under the crop); an element whose whole window is cropped away is written as +0.0.
 *     g_l of an inner level may be NULL (that output had no other consumer: D_l = S_l, no add); g_{L-1} may not.
 *     Any d_lateral_l, or the table itself, may be NULL and is then not stored; d_lateral_{L-1} is a plain copy of
 *     g_{L-1} (a second launch), which only a caller that needs the buffer asks for.  Everything is written
 *     (kWriteTo).
 *   The *_f16 entry points take halves everywhere.  Forward: the float sum of the two halves rounded once to half,
 *   and the next level reads the rounded half.  Backward: the window sum and the add of g_l are fp32 with ONE
 *   rounding to half per stored element, and the next level reads the rounded half (cast -> fp32 level -> cast).
 *   So an L-level call equals L - 1 chained two-level calls bit for bit: forward in both dtypes, backward in fp32
 *   and, in fp16, wherever the inner g_l are NULL (a chain has to round S_l to half before an add outside it).
 *   A workgroup owns a plane and a tile of level 0 with every finer element that maps onto it; inner levels pass
 *   through LDS, so every tensor is read or written once.  Pointers need element alignment only: 16-byte stores
 *   from the first 16-byte boundary of each output run, 16 / 8-byte loads where an input's phase allows and
 *   element loads where not; no bit depends on any pointer's phase.  No workspace, no atomics, no host read,
 *   graph-capturable; two calls give equal bits.  sd_last_dispatch() names the kernel, the grid and the tiling.
 *   Checked before anything touches the device -- SD_ERR_INVALID_ARG: L outside 2..6, a negative N or C, a null
 *   hs / ws / top / table / required pointer, a dimension < 1, a level larger than twice the one before, a pointer
 *   off its element alignment, an output range that overlaps an input range; SD_ERR_UNSUPPORTED: more than
 *   2^31 - 1 elements in one tensor.  N = 0 or C = 0 succeed without a launch (no pointer but hs / ws is looked at).
 * ---------------------------------------------------------------------------------------------- */
int sd_fpn_topdown_fwd(const float* top, const float* const* lateral, float* const* out, int N, int C, const int* hs,
                       const int* ws, int L, void* stream);
int sd_fpn_topdown_bwd(const float* const* g, float* d_top, float* const* d_lateral, int N, int C, const int* hs,
                       const int* ws, int L, void* stream);
int sd_fpn_topdown_fwd_f16(const void* top, const void* const* lateral, void* const* out, int N, int C, const int* hs,
                           const int* ws, int L, void* stream);
int sd_fpn_topdown_bwd_f16(const void* const* g, void* d_top, void* const* d_lateral, int N, int C, const int* hs,
                           const int* ws, int L, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLEDET_OPS_H_ */

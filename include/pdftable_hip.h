/*
 * pdftable_hip.h -- C ABI of libpdftable_hip.so, the MI355X (gfx950) engine behind pdf_table's
 * four-stage page-vision path.
 *
 * The reference has NO FFI for this path: each stage is a Python ``BaseInferTask`` whose
 * ``_run_model`` calls ``self.infer(...)`` which dispatches to PyTorch-eager or onnxruntime
 * (reference: src/pdftable/model/ocr_pdf/base_infer_task.py:366-381).  The functions below are
 * what a ``predictor_type == "hip"`` branch of that ``infer()`` binds (INTEGRATION.md shows the
 * ctypes stub).  Conventions:
 *   - plain pointers and sizes only; no torch / numpy types cross this boundary;
 *   - every function returns an int status, 0 == PT_OK; pt_last_error() gives the message of the
 *     last failure on the calling thread;
 *   - pointers named d_* are DEVICE pointers on the engine's GPU, h_* are HOST pointers;
 *   - weights, activations and scratch are engine-owned; inputs and outputs are caller-owned;
 *   - one engine per GPU; calls on one engine must be issued by one host thread at a time (the
 *     reference is single-threaded, base_infer_task.py:311-315).  Every stage (layout + cls, det,
 *     rec, the tsr detector pt_tsr_forward* / pt_tsr_decode, the tsr processor pt_tsr_process) has
 *     its own activation arena and scratch inside the engine, so calls of DIFFERENT
 *     stages may be in flight on different streams at the same time (measured: +10 % pages/s with
 *     the recogniser on a second stream); two calls of the SAME stage -- and pt_cls_forward_lines
 *     with pt_rec_forward*, which share the crop buffers -- must be stream-ordered.  The line classifier
 *     pt_cls_forward_lines_direct owns its input buffer and activation arena: it may be in flight beside
 *     pt_rec_forward* and the layout net (pt_layout_forward*, the other pt_cls_forward*) on other streams;
 *     two calls of it must be stream-ordered.
 *     Distinct engines own all their state (weights,
 *     arena, scratch, the decode state between the steps of pt_tsr_forward_decode) and are
 *     independent, with ONE restriction per device: the bf16 recognition LSTM (pt_rec_forward*)
 *     is a cluster kernel whose workgroups must all be resident at once, so two such launches may
 *     not overlap in time on one GPU (two engines, streams or processes).  An overlap cannot hang:
 *     a workgroup gives up after a bounded wait, pt_engine_check() (or the next rec call on that
 *     engine) returns PT_ERR_HIP ("not co-resident") once and switches the engine to the streaming
 *     kernel; pt_engine_set_lstm_cluster(e, 0) selects it up front;
 *   - `stream` is a hipStream_t (0 = the null stream).  Calls are asynchronous on that stream
 *     unless stated otherwise.
 */
#ifndef PDFTABLE_HIP_H
#define PDFTABLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_INVALID 1   /* bad argument / shape */
#define PT_ERR_HIP 2       /* a HIP runtime call failed */
#define PT_ERR_STATE 3     /* e.g. weights for that model not loaded */
#define PT_ERR_FORMAT 4    /* malformed weight blob */

typedef struct pt_engine pt_engine;
typedef void* pt_stream; /* hipStream_t */

/* ---- lifetime (replaces DeployUtils.model_eval / prepare_onnx_model, utils/deploy_utils.py:227-280) ---- */
int pt_engine_create(int device_id, pt_engine** out);
void pt_engine_destroy(pt_engine* e);
const char* pt_last_error(void);
int pt_abi_version(void);
/* Failures the DEVICE detected in work already executed (today: the co-residency time-out of the recognition LSTM, see
 * above).  Call it after synchronising the stream whose results are about to be consumed; PT_OK if nothing was flagged.
 * No counterpart in the reference (a torch/onnxruntime call either returns or raises). */
int pt_engine_check(pt_engine* e);
/* on = 1 (default; PT_LSTM_CLUSTER=0 in the environment changes the default): the bf16 recognition LSTM runs as the
 * weight-stationary cluster kernel, whose workgroups must all be co-resident -- only safe when nothing else runs on the
 * GPU beside the recogniser.  on = 0: the streaming kernel (about twice the LSTM time, no co-residency requirement):
 * use it whenever pt_rec_forward* runs on a stream beside other work.  A failure pt_engine_check reports also
 * switches the engine to 0 and clears the flag, so the failed batch can simply be submitted again. */
int pt_engine_set_lstm_cluster(pt_engine* e, int on);
/* MtlTabNet (pt_tsr_mtl_structure), PT_PRECISION_BF16 only: on = 1 keeps a second copy of the source-attention keys / values of the
 * KV-cached structure loop as fp8 (e4m3, x 8) and streams THAT every step -- half the bytes of the loop's dominant HBM stream
 * (BASELINE.json configs[4] names fp8; this is where fp8 pays on this path).  A throughput option with recorded drift
 * (tests/test_gpu_mtl.py), off by default; ignored in PT_PRECISION_BF16X3.  Environment default: PT_MTL_KV_FP8. */
int pt_engine_set_mtl_kv_fp8(pt_engine* e, int on);
/* Lore detector (pt_tsr_forward*, pt_op_dcn), PT_PRECISION_BF16 only: on = 1 (dcn_mfma_kernel) or 2 (dcn_mfma2_kernel: full-line gathers, one workgroup
 * per CU; layers with 64 outputs, the others keep the VALU blend) runs the modulated deformable convolutions
 * (model/lore/dcnv2.py:71-86, DCNv2_latest/src/cuda/dcn_v2_im2col_cuda.cu:121-191) with the bilinear blend on the matrix pipe
 * (dcn_mfma_kernel: corner lines by LDS-DMA, blend = MFMA against block-diagonal bf16 weights); on = 0 (default) keeps the VALU blend
 * with fp32 weights (dcn_fused64_kernel).  Both are bf16-mode results: the sampled columns differ by the bf16 rounding of the four
 * bilinear x mask weights (<= 2^-9 of a column; tests/test_gpu_dcn_op.py holds both to the oracle).  Measured equal in speed
 * (profiles/r04/experiments.txt: both sit on the vector-memory path's gather rate), hence the exact weights by default.
 * Ignored in PT_PRECISION_BF16X3.  Environment default: PT_DCN_MFMA. */
int pt_engine_set_dcn_mfma(pt_engine* e, int on);

/* Arithmetic of the conv nets (DESIGN.md "numerics").  PT_PRECISION_BF16: bf16 activations/weights, fp32
 * accumulate -- the throughput mode BASELINE.json's configs name.  PT_PRECISION_BF16X3: every activation and
 * weight is a (hi, lo) bf16 pair and each product is three MFMA passes (hi*hi + lo*hi + hi*lo), fp32-class
 * accuracy (~1e-5 relative) at ~1/3 of the throughput: the mode that meets the reference-fp32 parity tolerance.
 * In BF16X3 mode every bf16 NHWC activation tensor of C channels crossing this ABI (pt_det_preprocess output,
 * pt_det_forward_net input, pt_op_* tensors with split=1) has 2C channels laid out [hi(C) | lo(C)].
 * PT_PRECISION_F16X2: the same (hi, lo) bf16 activation pairs -- same tensors across this ABI -- but the convolutions and GEMMs of
 * the DB / CRNN / Lore / PicoDet graphs multiply them with SINGLE fp16 weights in two fp16 MFMA passes (hi*w + lo*w; a bf16 value
 * converts to fp16 exactly): rounding the WEIGHTS to 11 bits moves the logits by ~1.5e-4 of their scale (tools/x2_emulation.py) --
 * inside the 1e-3 tolerance at 2/3 of BF16X3's matrix work; layers without the variant run as in BF16X3.
 * PT_PRECISION_F16 (ABI 14): single-pass IEEE half -- the reference's own GPU arithmetic (base_infer_task.py:56-57 precision="fp16",
 * utils/deploy_utils.py:227-240 model.half()): every 16-bit tensor crossing this ABI (activations, the weight tiles of the blob) holds fp16
 * bits instead of bf16 bits, products accumulate in fp32, stores round to nearest even and SATURATE at +-65504 (never Inf).  Same
 * kernels, bytes and MFMA rate as PT_PRECISION_BF16 with 11 significant bits instead of 8.  The weight blobs must have been packed for
 * it (weights.py fmt="f16"); a bf16 blob under this precision (or the reverse) is refused by every forward call.  The ONNX operator
 * entry points (pt_op_*) follow the engine's precision the same way. */
#define PT_PRECISION_BF16 0
#define PT_PRECISION_BF16X3 1
#define PT_PRECISION_F16X2 2
#define PT_PRECISION_F16 3
int pt_engine_set_precision(pt_engine* e, int precision);

/* Model kinds for pt_weights_load.  A blob is the "PTW1" container written by
 * pdf_table_amd/weights.py (BN-folded, bf16 KRSC-tiled conv weights, fp32 biases). It replaces
 * torch.load + load_state_dict of model/db_net/modeling_db_net.py:53-56 and
 * model/ocr_recognition/modeling_ocr_recognition.py:102-132. */
enum {
  PT_MODEL_DB_RESNET18 = 1, /* db_net/dbnet.py:715-728 */
  PT_MODEL_CRNN = 2,        /* crnn/modeling_crnn.py:36-113 */
  PT_MODEL_LORE_DLA34 = 3,  /* lore/lore_dla_34.py:137-206 (DLASeg on dla34 + DCN), modeling_lore.py:88-95 */
  PT_MODEL_LORE_PROCESSOR = 4, /* lore/lore_processor.py:399-514 (LoreProcessModel) */
  PT_MODEL_LORE_RESNET18 = 6, /* lore/lore_detector.py:155-389 (LoreDetectModel, the 'wireless' detector) */
  PT_MODEL_DB_NAS = 7,        /* db_net/dbnet.py:693-712 (DBNasModel: ProxylessNAS backbone + LightSegDetector) */
  PT_MODEL_PPLCNET = 8,       /* cls/cls_pp_lcnet.py:164-283 (PPLCNet classifier); kinds 8 .. 8 + PT_CLS_SLOTS - 1 = classifier slots */
  PT_MODEL_PICODET = 5,     /* picodet/lcnet.py:159-259 + csp_pan.py:233-347 + pico_head.py:966-1160 (assumed config) */
  PT_MODEL_CONVNEXT_VIT = 16, /* convnext_vit/modeling_convnext_vit.py:20-45 (ConvNextViT recogniser) */
  PT_MODEL_MTL_BACKBONE = 17, /* table/mtl_tabnet/table_resnet_extra.py:205-318 (TableResNetExtra, backbone of MtlTabNet) */
  PT_MODEL_MTL_DECODER = 18,  /* table/mtl_tabnet/master_decoder.py:194-531 (MtlTabNetDecoder: structure, box and cell-content decoders) */
  PT_MODEL_CENTERNET_DLA34 = 19, /* center_net/modeling_centernet.py:609-661 (DLASeg on dla34, no DCN: CenterNet table cells) */
  PT_MODEL_DOCX_DLA34 = 20,      /* docx_layout/model_dla.py:543-652 (DLASeg on dla34, eight heads: DocXLayout page layout) */
};
int pt_weights_load(pt_engine* e, int model_kind, const void* h_blob, size_t nbytes);
/* Same, but the blob already sits in device memory (e.g. after an RCCL broadcast from rank 0). */
int pt_weights_load_device(pt_engine* e, int model_kind, const void* d_blob, size_t nbytes, pt_stream stream);

/* ---- stage 1: layout detection (PicoDet) -------------------------------------------------------- */
#define PT_LAYOUT_LEVELS 4
#define PT_LAYOUT_HEAD_CS 40   /* fp32 values per anchor: ncls class logits, then 4 * (reg_max + 1) box logits, zero padded */
#define PT_LAYOUT_CAND_FLOATS 48 /* candidate record: int32 level, int32 anchor, 40 head values, zero padding */

/* Anchors of level l for an inp_h x inp_w input: strides 8, 16, 32 and the extra 5x5/s2 level (csp_pan.py:265-270). */
int pt_layout_plan(int inp_h, int inp_w, int32_t fm_h[PT_LAYOUT_LEVELS], int32_t fm_w[PT_LAYOUT_LEVELS]);

/* OCRPicodetPreProcessor.__call__ (picodet/processor_picodet.py:72-113): BGR flip, cv2.resize to inp_w x inp_h (8-bit
 * bilinear, aspect not kept), (x * 1/255 - mean) / std  ->  bf16 NHWC4 [n, inp_h, inp_w, 4] (8 in BF16X3 mode). */
int pt_layout_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n, int h, int w, int inp_h, int inp_w,
                         uint16_t* d_out_bf16, pt_stream stream);

/* Network only: LCNet -> CSP-PAN -> PicoHead.forward_eval(export_post_process=False) before the sigmoid.
 *   d_head[l] : float32 [n, fm_h[l] * fm_w[l], PT_LAYOUT_HEAD_CS] */
int pt_layout_forward_net(pt_engine* e, const uint16_t* d_input_bf16, int n, int inp_h, int inp_w, float* d_head0,
                          float* d_head1, float* d_head2, float* d_head3, pt_stream stream);

/* Anchors whose best class score exceeds thr_lo, with their raw head values -- everything
 * OCRPicodetPostProcessor.__call__ (processor_picodet.py:184-298) can keep when thr_lo <= its score_threshold.
 *   d_counts : int32 [n] candidates found (may exceed max_cands: only the first max_cands records are stored)
 *   d_cands  : float32 [n, max_cands, PT_LAYOUT_CAND_FLOATS] */
int pt_layout_candidates(pt_engine* e, const float* d_head0, const float* d_head1, const float* d_head2,
                         const float* d_head3, int n, int inp_h, int inp_w, int num_classes, float thr_lo, int max_cands,
                         int32_t* d_counts, float* d_cands, pt_stream stream);

/* pt_layout_preprocess + pt_layout_forward_net + pt_layout_candidates with engine-owned intermediates.
 * Replaces OcrLayoutTask._preprocess + _run_model (ocr_layout_task.py:70-123). */
int pt_layout_forward(pt_engine* e, const uint8_t* d_pages_rgb, int n, int h, int w, int inp_h, int inp_w, int num_classes,
                      float thr_lo, int max_cands, int32_t* d_counts, float* d_cands, pt_stream stream);

/* Host: greedy per-class hard NMS of OCRPicodetPostProcessor (processor_picodet.py:301-348) for one page.
 *   h_boxes    : float64 [n, 5] (x1, y1, x2, y2, score)
 *   h_order    : per group (class) the candidate indices in ascending score order (numpy argsort()[-200:]);
 *   h_group_off: int64 [n_groups + 1] offsets into h_order
 *   h_picked   : int64 [len(h_order)] picked indices per group, in pick order;  h_n_picked: int32 [n_groups] */
int pt_hard_nms(const double* h_boxes, const int64_t* h_order, const int64_t* h_group_off, int n_groups,
                double iou_threshold, int top_k, int64_t* h_picked, int32_t* h_n_picked);

/* ---- stage 2: DB text detection ------------------------------------------------------------- */

/* Pre-process flavours: how a page is resized before the net. */
#define PT_DET_PRE_DB_PP 0    /* max side <= 960, sides rounded to /32, ImageNet mean/std on BGR:
                                 db_pp/image_operators.py:269-316,78-102; processor_ocr_db_pp.py:124 */
#define PT_DET_PRE_DB_TORCH 1 /* short side 736, long side ceil to /32, (x - mean)/255 on BGR:
                                 db_net/processor_ocr_dbnet.py:50-102 */
#define PT_DET_PRE_NONE 2     /* no resize (h, w must be multiples of 32); db_pp normalisation */

/* Resized (network) size the reference's pre-processor gives an h x w page. Pure host arithmetic. */
int pt_det_plan(int h, int w, int pre_flavour, int* net_h, int* net_w);

/* Full detection forward for n pages of identical size.  The detector network is the one loaded LAST with
 * pt_weights_load: PT_MODEL_DB_RESNET18 (`DBModel`) or PT_MODEL_DB_NAS (`DBNasModel`), the two backbones
 * modeling_db_net.py:47-52 chooses between.
 *   d_pages_rgb : uint8 [n, h, w, 3] RGB (as np.array(PIL.Image) gives; the BGR flip is done inside)
 *   d_prob      : float32 [n, net_h, net_w]   sigmoid probability map   (may be NULL)
 *   d_bitmap    : uint32  [n, net_h, net_w/32] bit x%32 of word x/32 = (prob > thresh), optionally
 *                 2x2-dilated (DBPostProcess.__call__, db_pp/processor_ocr_db_pp.py:291-311) (may be NULL)
 * Replaces OcrDetectionTask._preprocess + _run_model (ocr_detection_task.py:77-124) and the
 * `pred > thresh` step of the post-processor. */
int pt_det_forward(pt_engine* e, const uint8_t* d_pages_rgb, int n, int h, int w, int pre_flavour,
                   float thresh, int use_dilation, float* d_prob, uint32_t* d_bitmap, pt_stream stream);

/* Network only: d_input is bf16 NHWC4 [n, net_h, net_w, 4] (4th channel zero), already normalised.
 * Used by parity tests to feed the net the exact tensor the oracle sees. d_logits (optional) gets the
 * pre-sigmoid fp32 map. */
int pt_det_forward_net(pt_engine* e, const uint16_t* d_input_bf16, int n, int net_h, int net_w,
                       float* d_prob, float* d_logits, pt_stream stream);

/* Pre-process only (tests / CPU-baseline inputs): writes bf16 NHWC4 [n, net_h, net_w, 4]. */
int pt_det_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n, int h, int w, int pre_flavour,
                      uint16_t* d_out_bf16, pt_stream stream);

/* prob -> bit-packed bitmap (see pt_det_forward). */
int pt_det_bitmap(pt_engine* e, const float* d_prob, int n, int net_h, int net_w, float thresh,
                  int use_dilation, uint32_t* d_bitmap, pt_stream stream);

/* box_score_fast (db_pp/processor_ocr_db_pp.py:253-268) for nb quads on the device.
 *   d_boxes : float32 [nb, 9] = (page index, x0,y0,x1,y1,x2,y2,x3,y3) in net-map pixels
 *   d_scores: float32 [nb] mean probability inside the quad (cv2.fillPoly mask semantics) */
int pt_det_box_scores(pt_engine* e, const float* d_prob, int n, int net_h, int net_w,
                      const float* d_boxes, int nb, float* d_scores, pt_stream stream);

/* Host side of DBPostProcess.boxes_from_bitmap (db_pp/processor_ocr_db_pp.py:174-251), split in the
 * two halves that sit either side of pt_det_box_scores.  Pure CPU (C++), no GPU needed.
 *
 * pt_db_candidates: contour tracing (cv2.findContours RETR_LIST / CHAIN_APPROX_SIMPLE), first
 *   max_candidates contours, min-area rectangle + get_mini_boxes ordering, drops sside < min_size.
 *   h_bitmap: uint32 [net_h, net_w/32] of ONE page. h_boxes: float32 [cap, 8]; returns count in *n_out. */
int pt_db_candidates(const uint32_t* h_bitmap, int net_h, int net_w, int max_candidates, float min_size,
                     float* h_boxes, float* h_sside, int cap, int* n_out);
/* pt_db_finalize: score gate, unclip (Clipper round-join offset by area*ratio/perimeter), second
 *   min-area rectangle, sside gate (min_size + 2), rescale to the source page, round, clip.
 *   Output h_out: int32 [cap, 8]; h_out_scores float32 [cap]. */
int pt_db_finalize(const float* h_boxes, const float* h_scores, int nb, float box_thresh, float unclip_ratio,
                   float min_size, int net_h, int net_w, int dest_h, int dest_w, int post_flavour, int32_t* h_out,
                   float* h_out_scores, int cap, int* n_out);
/* Batch forms of the two calls above: n pages in one call, walked by n_threads threads inside the library (0 = all
 * hardware threads).  h_bitmaps uint32 [n, net_h, net_w/32]; h_boxes float32 [n, cap, 8] (page i's candidates at
 * [i, 0 .. n_out[i])), h_sside float32 [n, cap] or NULL.  pt_db_finalize_batch: h_scores float32 [n, cap], nb int [n]
 * candidates per page; h_out int32 [n, cap, 8]; filter != 0 additionally applies PPOcrDetectionPostProcessor.
 * filter_tag_det_res (db_pp/processor_ocr_db_pp.py:344-386: clockwise order, clip to the page, drop boxes <= 3 px) and
 * writes the surviving boxes as float32 [n, cap, 8] to h_out_f32 (n_out then counts those). */
int pt_db_candidates_batch(const uint32_t* h_bitmaps, int n, int net_h, int net_w, int max_candidates, float min_size,
                           int n_threads, float* h_boxes, float* h_sside, int cap, int* n_out);
int pt_db_finalize_batch(const float* h_boxes, const float* h_scores, const int* nb, int n, int cap, float box_thresh,
                         float unclip_ratio, float min_size, int net_h, int net_w, int dest_h, int dest_w, int post_flavour,
                         int filter, int n_threads, int32_t* h_out, float* h_out_f32, float* h_out_scores, int* n_out);
#define PT_DET_POST_DB_PP 0    /* float32 box / W * dest, round, clip, astype(int16): processor_ocr_db_pp.py:211-217 */
#define PT_DET_POST_DB_TORCH 1 /* box.astype(int32) first, then the same in float64: ocr_detection_utils.py:198-206 */

/* ---- stage 3: text-line recognition (CRNN) -------------------------------------------------------- */
#define PT_REC_H 32     /* OCRRecognitionConfig.img_height                                        */
#define PT_REC_W 640    /* img_width for CRNN (configuration_ocr_document.py:47-48)                */
#define PT_REC_T 160    /* time steps = W / 4 (crnn/modeling_crnn.py: two 2x2 pools)               */
#define PT_REC_NCLS 7644 /* crnn/modeling_crnn.py:90                                               */

/* One text line to cut out of a page: the INVERSE perspective matrix (row-major 3x3, destination -> source, what
 * cv2.warpPerspective evaluates) of OcrCommonUtils.crop_image (utils/ocr/ocr_common_utils.py:214-266) and the
 * crop size int(img_width) x int(img_height) computed there. */
typedef struct pt_rec_line {
  double minv[9];
  int32_t page;
  int32_t crop_w;
  int32_t crop_h;
  int32_t reserved;
} pt_rec_line;

/* Recognise n_lines text lines cut from n_pages pages (uint8 [n_pages,h,w,3] RGB, on the GPU).
 *   d_lines   : device array of pt_rec_line;  h_crop_px: HOST array [n_lines] of crop_w*crop_h (sizes the crop
 *               scratch without a device round trip)
 *   d_ids     : int32 [n_lines, PT_REC_T] arg-max class per time step (0 = CTC blank); collapse on the host
 *   d_maxlogit: float [n_lines, PT_REC_T] the winning logit (may be NULL)
 * Replaces the per-line loop OcrSystemTask.text_recognition -> crop_image -> OcrRecognitionTask
 * (ocr_system_task.py:296-336, ocr_recognition_task.py:81-136) and the arg-max of OCRRecognition.postprocess. */
int pt_rec_forward(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int h, int w, const pt_rec_line* d_lines,
                   const int64_t* h_crop_px, int n_lines, int32_t* d_ids, float* d_maxlogit, pt_stream stream);
/* Same, for lines that are ALREADY cropped (what OcrRecognitionTask.__call__ receives, ocr_recognition_task.py:67-79):
 * d_crops_rgb is the concatenation of the n_lines uint8 [crop_h, crop_w, 3] images; only crop_w / crop_h of d_lines
 * are read.  Resize (OCRRecognitionPreprocessor.keepratio_resize) + CRNN + arg-max. */
int pt_rec_forward_crops(pt_engine* e, const uint8_t* d_crops_rgb, const pt_rec_line* d_lines, const int64_t* h_crop_px,
                         int n_lines, int32_t* d_ids, float* d_maxlogit, pt_stream stream);
/* Network only: d_gray bf16 [n, 32, 640] (BF16X3 mode: [n, 32, 640, 2] = hi, lo), values in [0, 1]. */
int pt_rec_forward_net(pt_engine* e, const uint16_t* d_gray, int n, int32_t* d_ids, float* d_maxlogit, pt_stream stream);
/* Crop + resize + gray only (tests): writes d_gray as above. */
int pt_rec_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int h, int w, const pt_rec_line* d_lines,
                      const int64_t* h_crop_px, int n_lines, uint16_t* d_gray, pt_stream stream);

/* ---- stage 3, ConvNextViT recogniser (OcrRecognitionTask(model="ConvNextViT"), BASELINE.json configs[4]) ---------
 * OCRRecognitionPreprocessor with do_chunking (model/ocr_recognition/processor_ocr_recognition.py:44-62,94-113): keep-ratio
 * resize to 32 x 804, three 300-px chunks at 252-px steps; ConvNextViT.forward (model/convnext_vit/modeling_convnext_vit.py:
 * 38-45, modeling_convnext.py:29-131, modeling_vit.py:31-143): every chunk through the ConvNext CNN and the 12-layer ViT, the
 * chunks' 75 tokens stitched to 201 per line, Linear(192 -> 7644); then the arg-max of OCRRecognitionPostProcessor (:147-150).
 *   d_ids / d_maxlogit: [n_lines, PT_CVIT_T] arg-max class (0 = CTC blank, vocabulary from class 2) and its logit.
 *   h_crop_wh (HOST int32 [n_lines][2] = crop_w, crop_h; may be NULL): with the crop sizes known on the host, the 300-px chunks
 *   that hold no text (text width after the resize <= 252 j for chunk j) are not computed line by line: every all-padding
 *   chunk yields the same 75 tokens, so ONE is computed per call and shared -- bit-identical results. */
#define PT_CVIT_W 804          /* OCRRecognitionConfig.img_width with do_chunking (configuration_ocr_recognition.py:47) */
#define PT_CVIT_CHUNK_W 300    /* processor_ocr_recognition.py:105-106 */
#define PT_CVIT_CHUNK_STEP 252 /* 300 - 48 */
#define PT_CVIT_T 201          /* modeling_vit.py:134 */
#define PT_CVIT_NCLS 7644      /* modeling_convnext_vit.py:33 */
/* lines cut from resident pages (as pt_rec_forward) */
int pt_rec_cvit_forward(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int h, int w, const pt_rec_line* d_lines,
                        const int64_t* h_crop_px, const int32_t* h_crop_wh, int n_lines, int32_t* d_ids, float* d_maxlogit,
                        pt_stream stream);
/* lines that are already cropped (as pt_rec_forward_crops) */
int pt_rec_cvit_forward_crops(pt_engine* e, const uint8_t* d_crops_rgb, const pt_rec_line* d_lines, const int64_t* h_crop_px,
                              const int32_t* h_crop_wh, int n_lines, int32_t* d_ids, float* d_maxlogit, pt_stream stream);
/* Network only.  d_gray fp32 in [0, 1]: layout 0 = chunks [3 n_lines, 32, 300] (the tensor the reference's model receives,
 * gray), layout 1 = lines [n_lines, 32, 804] (chunk j = columns [252 j, 252 j + 300)).  h_text_w (HOST int32 [n_lines], may be
 * NULL): columns >= h_text_w[i] of line i are zero padding (same chunk sharing as h_crop_wh above). */
int pt_rec_cvit_forward_net(pt_engine* e, const float* d_gray, int layout, int n_lines, const int32_t* h_text_w, int32_t* d_ids,
                            float* d_maxlogit, pt_stream stream);
/* Resize + gray only (tests): d_gray fp32 [n_lines, 32, 804]. */
int pt_rec_cvit_preprocess_crops(pt_engine* e, const uint8_t* d_crops_rgb, const pt_rec_line* d_lines, const int64_t* h_crop_px,
                                 int n_lines, float* d_gray, pt_stream stream);

/* PP-OCR recognition pre-processor -- PPOcrRecPreProcessor (model/ocr_rec_pp/processor_ocr_rec_pp.py:69-135,
 * resize_norm_img :43-67), the pre-processing of the recogniser the reference's system path selects
 * (fix_model_names, model/ocr_pdf/configuration_ocr_document.py:138-141).  The HOST orders the lines by aspect ratio and
 * groups them into mini-batches of rec_batch_num (np.argsort, as the reference; pdf_table_amd/rec_pp_stage.py); one item =
 * one line of that plan: which crop, the width it is resized to (height img_h = 48), the padded width img_w of its
 * mini-batch and where its [3, img_h, img_w] fp32 block starts in d_out (float offset; a mini-batch's items are
 * consecutive, which makes d_out the concatenation of the reference's [b, 3, 48, img_w] NCHW arrays).
 * Pixels: cv2.resize 8-bit INTER_LINEAR semantics, then (x / 255 - 0.5) / 0.5 in fp32, zeros right of resized_w. */
typedef struct pt_rec_pp_item {
  int32_t line;
  int32_t resized_w;
  int32_t img_w;
  int32_t reserved;
  int64_t out_off;
} pt_rec_pp_item;
/* lines cut from resident pages (crop_image on the device, as pt_rec_forward) */
int pt_rec_pp_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int h, int w, const pt_rec_line* d_lines,
                         const int64_t* h_crop_px, int n_lines, const pt_rec_pp_item* d_items, int n_items, int img_h,
                         int max_img_w, float* d_out, pt_stream stream);
/* lines that are already cropped (what OcrRecognitionTask.__call__ receives); d_crops_rgb / d_lines as pt_rec_forward_crops */
int pt_rec_pp_preprocess_crops(pt_engine* e, const uint8_t* d_crops_rgb, const pt_rec_line* d_lines, const int64_t* h_crop_px,
                               int n_lines, const pt_rec_pp_item* d_items, int n_items, int img_h, int max_img_w, float* d_out,
                               pt_stream stream);

/* ---- stage 4: table structure recognition (Lore) ------------------------------------------------- */
/* One table crop of a resident page and the INVERSE (destination -> crop) affine map of
 * TableLorePreProcessor.process (lore/processer_lore.py:66-90), i.e. cv::invertAffineTransform of
 * get_affine_transform(c, s, 0, [inp_w, inp_h]) (lineless_table_process.py:403-438), computed on the host in float64.
 * The crop is the integer box of crop_image_by_box (utils/ocr/ocr_common_utils.py:269-284). */
typedef struct pt_tsr_table {
  double minv[6];
  int32_t page, x0, y0, crop_w, crop_h, reserved;
} pt_tsr_table;

/* Warp + normalise n table crops into the detector's input (cv2.warpAffine INTER_LINEAR fixed-point semantics, zero
 * border, then ((x / 255) - mean) / std with Lore's constants).
 *   d_pages_rgb : uint8 [n_pages, ph, pw, 3];  d_tables : pt_tsr_table [n];  bgr != 0: feed channels reversed, as the
 *                 reference does for path / PIL inputs (processer_lore.py:48-64,152)
 *   d_out_bf16  : bf16 NHWC4 [n, inp_h, inp_w, 4] (8 channels = hi | lo in BF16X3 mode) */
int pt_tsr_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int ph, int pw, const pt_tsr_table* d_tables,
                      int n, int inp_h, int inp_w, int bgr, uint16_t* d_out_bf16, pt_stream stream);

/* Detector network only (LoreModel.forward's `self.detect_infer_model(pixel_values)`, lore/modeling_lore.py:147;
 * DLASeg.forward lore/lore_dla_34.py:184-196).
 *   d_input_bf16 : bf16 NHWC4 [n, H, W, 4] (4th channel zero; [hi rgb0 | lo rgb0] = 8 channels in BF16X3 mode),
 *                  already warped + normalised (TableLorePreProcessor.process, lore/processer_lore.py:66-109);
 *                  H, W multiples of 32
 *   outputs      : fp32 NHWC head maps at H/4 x W/4, channel strides PT_TSR_CS_*: hm [.,8] (2 valid: cell centres,
 *                  corners), st [.,8], wh [.,8], ax [.,256], cr [.,256], reg [.,8] (2 valid) -- the dict `z` of
 *                  DLASeg.forward, pre-sigmoid */
#define PT_TSR_CS_SMALL 8
#define PT_TSR_CS_FEAT 256
int pt_tsr_forward_net(pt_engine* e, const uint16_t* d_input_bf16, int n, int H, int W, float* d_hm, float* d_st,
                       float* d_wh, float* d_ax, float* d_cr, float* d_reg, pt_stream stream);

/* Same contract for the 'wireless' detector (LoreDetectModel.forward, lore/lore_detector.py:353-389; weights
 * PT_MODEL_LORE_RESNET18); H, W multiples of 64. */
int pt_tsr_forward_net_wireless(pt_engine* e, const uint16_t* d_input_bf16, int n, int H, int W, float* d_hm, float* d_st,
                                float* d_wh, float* d_ax, float* d_cr, float* d_reg, pt_stream stream);

/* Heat-map + corner-point decode (process_detect_output, lore/lineless_table_process.py:592-655: corner_decode :97-124,
 * ctdet_4ps_decode :127-267 incl. the wiz_rev vertex snapping :188-236, logi = ax + cr_feat :648) for n tables.
 *   head maps   : as written by pt_tsr_forward_net (fp32 NHWC at h x w)
 *   wiz_rev     : LoreConfig.wiz_rev (configuration_lore.py:79-92); vis_thresh: LoreConfig.vis_thresh
 *   d_counts    : int32 [n]            cells with final score >= vis_thresh (= rows of slct_logi_feat, :568-571)
 *   d_dets      : float32 [n, 3000, 9] x0,y0..x3,y3 in feature-map pixels + score, sorted like the reference's `dets`
 *   d_logi      : float32 [n, 3000, 256] logic features of the same rows
 * Only rows [0, number of peaks above vis_thresh) are written; rows past d_counts[i] are not part of the result. */
#define PT_TSR_MAX_CELLS 3000
int pt_tsr_decode(pt_engine* e, const float* d_hm, const float* d_st, const float* d_wh, const float* d_ax,
                  const float* d_cr, const float* d_reg, int n, int h, int w, int wiz_rev, float vis_thresh,
                  int32_t* d_counts, float* d_dets, float* d_logi, pt_stream stream);

/* pt_tsr_forward_net + pt_tsr_decode in one call for the DLA-34 detector (PT_MODEL_LORE_DLA34), same outputs as
 * pt_tsr_decode.  Of the six head maps the decode needs only `hm` everywhere: `reg` / `wh` / `st` are read at the kept
 * peaks (<= 3000 cells + 5000 corners per table, lineless_table_process.py:127-177), `ax` / `cr` at the final cells'
 * centres and corner pixels (:254-263, _get_4ps_feat :39-63).  Here those five heads run on 3x3-pixel patches around
 * exactly these positions instead of on the whole map; every value that is read is produced by the same kernels in the
 * same order as in the dense map (bit-identical to the two-call path when both use one conv kernel family). */
int pt_tsr_forward_decode(pt_engine* e, const uint16_t* d_input_bf16, int n, int in_h, int in_w, int wiz_rev,
                          float vis_thresh, int32_t* d_counts, float* d_dets, float* d_logi, pt_stream stream);

/* ---- letterbox rows of the DLA-34 detector's front segment ------------------------------------------------------------------------
 * A crop wider than high fills only the middle rows of the detector's input; the rest holds the warp's border value.  The front of the
 * net (base_layer, level0, level1, level2: everything up to the 64-channel map at H/4) has a static receptive field of
 * pt_tsr_band_radius() input rows, so its output farther than that from the content is what an all-padding table gives at the same
 * map position.  pt_tsr_plan_bands says, per table, which input rows the front segment has to see:
 *   full = 1          : all of them -- crop_h >= crop_w, a map with a rotation / shear term (minv[1], minv[3]: one that moves the warp's 10-bit
 *                       fixed-point coordinates somewhere on the map), or a window that would come
 *                       within 64 rows of the map's top or bottom (upper_left maps always do), where the convolutions' own zero padding counts
 *   [row0, row1)      : else, multiples of 64: every row whose bilinear footprint can touch the crop, +- 2, widened by twice the radius
 *   [keep0, keep1)    : the rows of the H/4 map taken from the band (content +- 2 +- radius; each at least the radius inside the band)
 *   stack, stack_row  : banded tables are stacked one under the other into tall one-image inputs of at most max_stack_rows rows
 *                       (<= 0 or more than 32768: 32768); the band starts at input row stack_row of stack `stack`
 * h_tables: host records.  *n_stacks and *row_fraction (rows planned / (n * inp_h)) may be null. */
typedef struct pt_tsr_band {
  int32_t full, row0, row1, keep0, keep1, stack, stack_row, reserved;
} pt_tsr_band;
int pt_tsr_band_radius(void);
int pt_tsr_plan_bands(const pt_tsr_table* h_tables, int n, int inp_h, int inp_w, int max_stack_rows, pt_tsr_band* h_out, int32_t* n_stacks,
                      double* row_fraction);

/* pt_tsr_preprocess + pt_tsr_forward_decode in one call with the tables known on the host as well (h_tables and d_tables hold the same n records):
 * the front segment of the detector runs on the planned row bands only, the rest of its level-2 map is filled from the cached map of an
 * all-padding table, and everything behind runs unchanged.  Same outputs, bit for bit, as the two calls.  The environment variable
 * PT_TSR_BAND_STACK_ROWS (read per call) lowers the stack cap. */
int pt_tsr_warp_forward_decode(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int ph, int pw, const pt_tsr_table* h_tables,
                               const pt_tsr_table* d_tables, int n, int inp_h, int inp_w, int bgr, int wiz_rev, float vis_thresh,
                               int32_t* d_counts, float* d_dets, float* d_logi, pt_stream stream);

/* Test hook: the detector's level-2 map (`layers[2]` of DLA.forward: [n, inp_h / 4, inp_w / 4, 64], (hi | lo) = 128 values per pixel in the pair
 * modes) of n table crops.  bands = 0: the warp and the front segment on whole maps; 1: on the planned row bands, planned with `margin` in place of
 * pt_tsr_band_radius() (< 0: the radius itself; below it the result is WRONG near the content's edge -- that is what the hook is for). */
int pt_op_tsr_level2(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int ph, int pw, const pt_tsr_table* h_tables,
                     const pt_tsr_table* d_tables, int n, int inp_h, int inp_w, int bgr, int bands, int margin, uint16_t* d_out,
                     pt_stream stream);

/* ---- CenterNet table cells (TableStructureRec = DLASeg('dla34', down_ratio 4, head_conv 256), center_net/modeling_table_structure.py:22-47;
 * weights PT_MODEL_CENTERNET_DLA34) ------------------------------------------------------------------------------------------- */
/* Detector network: d_input_bf16 as for pt_tsr_forward_net (pt_tsr_preprocess output; H, W multiples of 32).  Outputs: fp32 NHWC
 * head maps at H/4 x W/4, channel stride 8 each: hm (2 valid: cell centres, vertices; pre-sigmoid), v2c (8), c2v (8), reg (2 valid). */
int pt_centernet_forward_net(pt_engine* e, const uint16_t* d_input_bf16, int n, int H, int W, float* d_hm, float* d_v2c, float* d_c2v,
                             float* d_reg, pt_stream stream);

/* Decode (OCRTableCenterNetPostProcessor.__call__, center_net/processer_centernet.py:170-205) of n tables' head maps (h x w):
 * sigmoid, 3x3 peaks, top-1000 cell centres and top-4000 vertices, corners and vertex pointers mapped to crop pixels by
 * d_affine (device fp64 [n][6]: per table the inverse map get_affine_transform(c, s, 0, (w, h), inv=1)), group_bbox_by_gbox.
 *   d_counts : int32 [n]   cells with score >= 0.3 (at most 1000)
 *   d_cells  : float32 [n, 1000, 9]  rows [0, d_counts[i]): x0,y0..x3,y3 in crop pixels + score, in top-K order.  The reference's
 *              output filter (score > 0.3) and its reading-order sort are host work. */
#define PT_CENTERNET_MAX_CELLS 1000
int pt_centernet_decode(pt_engine* e, const float* d_hm, const float* d_v2c, const float* d_c2v, const float* d_reg, int n, int h, int w,
                        const double* d_affine, int32_t* d_counts, float* d_cells, pt_stream stream);

/* ---- DocXLayout page layout (DocXLayoutModel = DLASeg('dla34', down_ratio 4, head_conv 256) with eight heads, docx_layout/model_dla.py:543-652;
 * weights PT_MODEL_DOCX_DLA34).  Entry points added by name under the current ABI number: no existing signature changed. ------------------- */
/* pt_tsr_preprocess's warp (cv2.warpAffine INTER_LINEAR fixed-point arithmetic, zero border, pt_tsr_table records, bgr flag) with the normalisation
 * ((v / 255.) - mean[c]) / std[c] (fp64, rounded to fp32 once, as numpy evaluates it) for constants handed in: mean3 / std3 are HOST float32 [3] in
 * the order of the OUTPUT channels (after the bgr flip).  DocXLayout's are {0.40789655, 0.44719303, 0.47026116} / {0.2886383, 0.27408165,
 * 0.27809834} (docx_layout/image_processing_docxlayout.py:110-145).  A change of constants between calls rebuilds the engine's table behind a
 * device synchronisation. */
int pt_docx_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int ph, int pw, const pt_tsr_table* d_tables, int n, int inp_h,
                       int inp_w, int bgr, const float* mean3, const float* std3, uint16_t* d_out_bf16, pt_stream stream);

/* Detector network: d_input_bf16 as pt_docx_preprocess writes it (H, W multiples of 32).  Outputs: fp32 NHWC head maps at H/4 x W/4, pre-sigmoid;
 * d_hm has channel stride 16 (11 valid), every other head stride 8: cls (4 valid), ftype (3), hm_sub (2), reg (2), reg_sub (2), wh (8), wh_sub (8).
 * Activations live in the layout stage's arena, so a table-structure net of the same engine may be in flight on another stream. */
int pt_docx_forward_net(pt_engine* e, const uint16_t* d_input_bf16, int n, int H, int W, float* d_cls, float* d_ftype, float* d_hm, float* d_hm_sub,
                        float* d_reg, float* d_reg_sub, float* d_wh, float* d_wh_sub, pt_stream stream);

/* Device half of DocXLayoutImagePostProcessor.post_process_model + pnms (docx_layout/image_processing_docxlayout.py:265-308, processor_utils.py:22-158)
 * for n pages' head maps (h x w, layouts as pt_docx_forward_net writes them), one launch, no engine.  Per page two branches: 0 = main (d_hm: ncls_main
 * classes at channel stride 16, d_wh, d_reg, d_cls, d_ftype), 1 = sub (d_hm_sub: ncls_sub classes at stride 8, d_wh_sub, d_reg_sub).
 *   peaks    : fp32 sigmoid; a pixel of class c is a peak when its sigmoid equals the maximum of class c's sigmoids over its 3 x 3 window (outside
 *              the map does not count)
 *   list     : the first K peaks with sigmoid >= thr_lo over all classes of the branch, by (score descending, class * h * w + pixel ascending) --
 *              exactly that list whatever the number of peaks
 *   d_counts : int32 [n][2]      entries of each list (<= K)
 *   d_recs   : float32 [n][2][K][PT_DOCX_REC_FLOATS]  rows [0, count): x0, y0 .. x3, y3 in head-map pixels (xs = x + reg[0], ys = y + reg[1], corner i =
 *              (xs - wh[2i], ys - wh[2i + 1])), score, class (0-based in its branch), then for branch 0 the index of the first maximum of the 4 cls
 *              sigmoids and of the 3 ftype sigmoids at the pixel; branch 1 writes 0 in both (the reference copies branch 0's columns of the same
 *              rank there, and nothing reads them)
 *   d_inds   : int32 [n][2][K]   class * h * w + pixel of each row; may be null
 *   d_keep   : uint8 [n][2][K]   pnms: 1 when (double)score >= 0.3 and no other row of the list with (double)score >= 0.3 and a larger score has the
 *              row's centre strictly inside its quad (fp64, products and sums unfused); 0 otherwise
 * Rows at and behind `count` are not written.  PT_ERR_INVALID without a launch: K > PT_DOCX_MAX_K, a branch with more than 16 classes (or more than
 * its channel stride), a map above 512 x 512. */
#define PT_DOCX_REC_FLOATS 12
#define PT_DOCX_MAX_K 128
int pt_docx_decode(const float* d_hm, const float* d_wh, const float* d_reg, const float* d_cls, const float* d_ftype, const float* d_hm_sub,
                   const float* d_wh_sub, const float* d_reg_sub, int n, int h, int w, int ncls_main, int ncls_sub, int K, float thr_lo,
                   int32_t* d_counts, float* d_recs, int32_t* d_inds, uint8_t* d_keep, pt_stream stream);

/* Logical-location processor (LoreProcessModel.forward, lore/lore_processor.py:465-514, evaluation branch) for the
 * cells of n_tables tables at once.
 *   d_logi, d_dets : as written by pt_tsr_decode;  h_counts : HOST int32 [n_tables] = its d_counts copied back
 *   use_2dpe       : LoreConfig.wiz_2dpe -- add the x/y position embeddings of the (int-truncated, [0,255]-clamped)
 *                    quad coordinates 0,1,2,5 (:486-491; lineless_table_process.py:576-589)
 *   d_logic, d_stacked : float32 [n_tables, 3000, 4]: rows [0, h_counts[i]) = logic_axis / stacked_axis (post-ReLU,
 *                    not yet rounded: process_logic_output, lineless_table_process.py:658-663, is host work) */
int pt_tsr_process(pt_engine* e, const float* d_logi, const float* d_dets, const int32_t* h_counts, int n_tables,
                   int use_2dpe, float* d_logic, float* d_stacked, pt_stream stream);

/* ---- single operator (parity tests of the conv kernel variants) --------------------------------- */
/* NHWC bf16 convolution on the MFMA implicit-GEMM kernel. d_w_tiled is [N/64][Cin/32][ks*ks][64][32] bf16
 * (pdf_table_amd/weights.py:tile_conv_weight), d_bias fp32 [N]. ks in {1,3} (pad ks/2), stride in {1,2}.
 * rep > 1: every output pixel is replicated rep x rep (fused nn.Upsample(nearest)); shuffle_cout > 0:
 * N = 4*shuffle_cout and the output is the 2x up-sampled ConvTranspose2d(k=2,s=2) image;
 * res_mode 1: + d_res (same shape as the un-replicated output); 2: + nearest-x2-upsampled d_res. */
int pt_op_conv2d(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cin, const uint16_t* d_w_tiled,
                 const float* d_bias, int N, int ks, int stride, uint16_t* d_out, int out_cstride, int out_coff,
                 int rep, int shuffle_cout, const uint16_t* d_res, int res_mode, int relu, int split, int out_lo_off,
                 pt_stream stream);
/* split=1 (BF16X3): d_in/d_res/d_out carry (hi | lo) channel groups, d_w_tiled is [N/64][3*Cin/32][ks*ks][64][32]
 * (K chunks: w_hi for x_hi, w_hi for x_lo, w_lo for x_hi), out_lo_off = channel distance hi -> lo in d_out. */
/* 1x1 stride-1 bf16 convolution with the epilogues the network launchers use and pt_op_conv2d does not expose (parity tests of the 1x1
 * kernels): d_out bf16 [B,H,W,out_cstride] or, when d_out_f32 is set, fp32 [B,H,W,out_cstride] (d_out unused); n_valid > 0: only
 * channels [0, n_valid) are stored; d_res_f32: fp32 residual laid out like d_out_f32 (added before the activation); d_ylimit: device
 * int, output rows >= *d_ylimit are not computed (the row-limited launches of the Lore patch mosaics). */
int pt_op_conv1x1_ex(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cin, const uint16_t* d_w_tiled, const float* d_bias,
                     int N, uint16_t* d_out, float* d_out_f32, int out_cstride, int n_valid, const float* d_res_f32, int relu,
                     const int32_t* d_ylimit, pt_stream stream);

/* Fused modulated deformable 3x3 convolution (pad 1, stride 1, dilation 1, one deformable group) + bias (+ ReLU): the operator
 * DCN.forward (model/lore/dcnv2.py:71-86) hands to torchvision.ops.deform_conv2d, sampling rule of
 * model/lore/DCNv2_latest/src/cpu/dcn_v2_im2col_cpu.cpp:26-55,123-190 (bilinear, zero outside (-1,H)x(-1,W), per-corner bounds).
 *   d_in  bf16 NHWC [B,H,W,C] ([hi(C) | lo(C)] when split), C % 32 == 0
 *   d_om  fp32 [B*H*W][32]: channel 2k / 2k+1 = (dy, dx) of tap k, 18+k = mask LOGIT of tap k (the sigmoid is applied here), 27..31 unused
 *   d_w_tiled: the [N, 9*C, 1, 1] weight (K = tap * C + c) tiled like a 1x1 convolution (weights.py:tile_conv_weight, or
 *              tile_conv_weight_x3 when split), d_bias fp32 [N], N % 64 == 0
 *   d_out bf16 [B,H,W,N] ([hi | lo] when split).  Since ABI 12. */
int pt_op_dcn(pt_engine* e, const uint16_t* d_in, const float* d_om, int B, int H, int W, int C, const uint16_t* d_w_tiled,
              const float* d_bias, int N, uint16_t* d_out, int relu, int split, pt_stream stream);

/* IDAUp's up-sampler: depthwise ConvTranspose2d(C, C, 2f, stride f, padding f/2, groups = C) of d_in [B,h,w,C] (+ d_add [B,h*f,w*f,C], may be
 * NULL) -> d_out [B,h*f,w*f,C]; d_w fp32 [(2f)^2][C] (tap-major), f = 2 or 4, C % 8 == 0 ([hi | lo] maps when split).  Added under ABI 18 (no existing signature changed). */
int pt_op_dwconvt_up_add(pt_engine* e, const uint16_t* d_in, const float* d_w, const uint16_t* d_add, uint16_t* d_out, int B, int h, int w, int C,
                         int f, int split, pt_stream stream);
/* pt_op_dcn followed by pt_op_dwconvt_up_add(d_up_in, d_up_w, add = the convolution's output) in one launch, bit for bit: the up-sampler runs in
 * the convolution's epilogue and the un-summed output is never written.  d_up_in [B,up_h,up_w,N] with up_h * up_f == H and up_w * up_f == W,
 * d_up_w fp32 [(2 up_f)^2][N].  C == N == 64 (up_f 2 or 4) or 128 (up_f 2), split == 0, default kernel settings only (no PT_DCN_* variable, no
 * pt_engine_set_dcn_mfma): anything else is PT_ERR_INVALID.  Added under ABI 18. */
int pt_op_dcn_up_add(pt_engine* e, const uint16_t* d_in, const float* d_om, int B, int H, int W, int C, const uint16_t* d_w_tiled,
                     const float* d_bias, int N, uint16_t* d_out, int relu, int split, const uint16_t* d_up_in, int up_h, int up_w,
                     const float* d_up_w, int up_f, pt_stream stream);

/* Lore's heat-map head on a feature map d_in [B,H,W,64]: hm.0 (3x3 64 -> 256 + ReLU; d_w1_tiled [4][2][9][64][32], d_b1 fp32 [256]) and hm.2
 * (1x1 256 -> 2 padded to 64 GEMM columns; d_w2_tiled [1][8][1][64][32] with rows 2 .. 63 zero, d_b2 fp32 [64]).  Single-pass modes only.
 *   fused == 0: the two launches.  d_hid [B,H,W,256] receives the hidden map, d_logits fp32 [B,H,W,8] the 1x1 launch's eight stored channels.
 *   fused == 1: one launch, the hidden map stays on chip (d_hid unused).  d_logits (may be NULL) as above: channels 0, 1 sum the same 256 exact
 *               products in another fp32 order, channels 2 .. 7 are equal bits; d_sig (may be NULL) fp32 [B,H,W,2] = the sigmoid of the logits as the
 *               decode's peak test reads it.  PT_ERR_INVALID when the fused head is switched off (PT_LORE_HM_FUSE=0).
 *   d_sig_ref (may be NULL) fp32 [B,H,W,2]: the decode's own sigmoid launch run on d_logits afterwards.
 * Added under ABI 19 (no existing signature changed). */
int pt_op_lore_hm_head(pt_engine* e, const uint16_t* d_in, int B, int H, int W, const uint16_t* d_w1_tiled, const float* d_b1,
                       const uint16_t* d_w2_tiled, const float* d_b2, int fused, uint16_t* d_hid, float* d_logits, float* d_sig, float* d_sig_ref,
                       pt_stream stream);

/* Stem of the ResNet-18 backbone: 7x7 s2 p3 conv (BN folded) + ReLU on a bf16 NHWC4 image (dbnet.py:272-275).
 * d_w is bf16 [64][7][8][4] (K padded: tap s=7 and channel 3 are zero), d_bias fp32 [64]; out bf16 [B,H/2,W/2,64]. */
int pt_op_stem7x7(pt_engine* e, const uint16_t* d_in, int B, int H, int W, const uint16_t* d_w, const float* d_bias,
                  uint16_t* d_out, int split, pt_stream stream);
/* MaxPool2d(3, 2, 1) on bf16 NHWC (dbnet.py:276). */
int pt_op_maxpool3x3s2(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, uint16_t* d_out, int split,
                       pt_stream stream);
/* ConvTranspose2d(64 -> 1, k=2, s=2) + Sigmoid (dbnet.py:539): in bf16 [B,H,W,64], d_w bf16 [4][64] (quadrant
 * dy*2+dx major), d_bias fp32 [1]; d_prob / d_logits fp32 [B,2H,2W] (either may be NULL). */
int pt_op_db_head_final(pt_engine* e, const uint16_t* d_in, int B, int H, int W, const void* d_w, const float* d_bias,
                        float* d_prob, float* d_logits, int split, pt_stream stream);

/* ---- single operators of the generic ONNX layer-list executor (pdf_table_amd/onnx_exec.py) --------------------
 * Replaces: onnxruntime's execution of an arbitrary graph behind BaseInferTask.infer (model/ocr_pdf/base_infer_task.py:
 * 366-370, sessions built by utils/deploy_utils.py:243-280).  bf16 NHWC, C a multiple of 8; convolutions go to
 * pt_op_conv2d.  act: 0 none, 1 ReLU, 2 hardswish.
 * split (since ABI 12; every operator below except the pure data movers): 0 = plain bf16 tensors; 1 = the tolerance mode's (hi | lo) tensors --
 * a pixel / token row holds [hi(C) | lo(C)], value = hi + lo, arithmetic in fp32 on the sum, result split again (the convention of
 * PT_PRECISION_BF16X3).  pt_op_act / pt_op_mul then need C (channels of one half; n_elems counts VALUES, i.e. pixels x C); pt_op_copy_channels
 * and pt_op_upsample_nearest move halves like any channels (the caller addresses them through the channel stride / offset). */
/* depthwise k x k (k 3 or 5, pad k/2, stride 1 or 2) + bias + act; d_w_taps fp32 [k*k][C], d_bias fp32 [C] */
int pt_op_dwconv(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, const float* d_w_taps, const float* d_bias, int k,
                 int stride, int act, uint16_t* d_out, int split, pt_stream stream);
/* element-wise a + b over npix pixels of C channels */
int pt_op_add(pt_engine* e, const uint16_t* d_a, const uint16_t* d_b, uint16_t* d_out, long long npix, int C, int split, pt_stream stream);
/* MaxPool2d(3, 2, 1), or a non-overlapping k x k pool (stride k, no padding, H and W divisible by k) */
int pt_op_maxpool(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, int k, int stride, int pad, uint16_t* d_out,
                  int split, pt_stream stream);
/* AveragePool k x k, stride k, no padding (H and W divisible by k) */
int pt_op_avgpool(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, int k, uint16_t* d_out, int split, pt_stream stream);
/* GlobalAveragePool: [B, HW, C] -> bf16 [B, C] (B, HW > 0; C a multiple of 8, <= 2048); d_scratch: pt_op_chan_mean_scratch_floats(B, C) floats */
int pt_op_chan_mean(pt_engine* e, const uint16_t* d_in, int B, int HW, int C, float* d_scratch, uint16_t* d_mean, int split, pt_stream stream);
int pt_op_chan_mean_scratch_floats(int B, int C);
/* x [B, HW, C] * gate [B, C] (the Mul of a squeeze-and-excitation block) */
int pt_op_scale_channels(pt_engine* e, const uint16_t* d_in, const uint16_t* d_gate, int B, int HW, int C, uint16_t* d_out,
                         int split, pt_stream stream);
/* stand-alone activation over n_elems (multiple of 8) values; kind: 1 ReLU, 2 hardswish, 4 sigmoid,
 * 5 hardsigmoid = max(0, min(1, alpha x + beta)), 6 ReLU6, 7 GELU (erf form), 8 swish x * sigmoid(x) */
int pt_op_act(pt_engine* e, const uint16_t* d_in, long long n_elems, int kind, float alpha, float beta, uint16_t* d_out, int C, int split,
              pt_stream stream);
/* Data movement of the executor (ONNX Concat / Slice / Split over channels, nearest Resize): dst[pix][dst_coff + c] = src[pix][src_coff + c] for
 * c < n; nearest-neighbour up-sampling by an integer factor -> [B, H f, W f, C]; element-wise product of two equally shaped tensors */
int pt_op_copy_channels(pt_engine* e, const uint16_t* d_src, long long npix, int src_cstride, int src_coff, uint16_t* d_dst, int dst_cstride, int dst_coff,
                        int n, pt_stream stream);
int pt_op_upsample_nearest(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, int factor, uint16_t* d_out, pt_stream stream);
int pt_op_mul(pt_engine* e, const uint16_t* d_a, const uint16_t* d_b, uint16_t* d_out, long long n_elems, int C, int split, pt_stream stream);
/* nbytes from src to dst (16-byte aligned) by a kernel on `stream`; either side may be PINNED HOST memory (hipHostMalloc / torch pin_memory: mapped into
 * the device's address space).  For the few small transfers a host thread WAITS for while the compute stream holds a backlog: an asynchronous
 * hipMemcpy goes through a DMA engine's in-order queue and can sit there behind copies of other streams that wait for kernels still to run
 * (measured: 15-50 ms in a 7 MB copy); a kernel on a high-priority stream cannot.  Replaces nothing in the reference (torch's .cpu()). */
int pt_copy_bytes(pt_engine* e, const void* src, void* dst, long long nbytes, pt_stream stream);
/* Sequence operators (the attention / LayerNorm / soft-max blocks of SVTR-type recognisers such as PP-OCRv4 rec, the recogniser
 * fix_model_names() selects: model/ocr_pdf/configuration_ocr_document.py:138-141).  Token rows bf16 [rows, c_pad], the first c channels real.
 * pt_op_layernorm: LayerNormalization over the channels (biased variance, eps inside the root), padded channels written as zeros.
 * pt_op_softmax: Softmax over the channels -> fp32 [rows, c] (d_out_f32, network outputs) OR bf16 [rows, c_pad] (d_out_bf16); pass one.
 * pt_op_attention: multi-head self-attention of rows holding [q | k | v], channel = part * heads * d + head * d + j (the fused-qkv layout of
 * timm / PaddleOCR SVTR blocks): out[b, t, head * d + j] = softmax_k(scale q.k) v; T <= 1024, d <= 64. */
int pt_op_layernorm(pt_engine* e, const uint16_t* d_in, long long rows, int c_pad, int c, const float* d_gamma, const float* d_beta, float eps,
                    uint16_t* d_out, int split, pt_stream stream);
int pt_op_softmax(pt_engine* e, const uint16_t* d_in, long long rows, int c_pad, int c, float* d_out_f32, uint16_t* d_out_bf16, int split, pt_stream stream);
int pt_op_attention(pt_engine* e, const uint16_t* d_qkv, int B, int T, int heads, int d, int qkv_cstride, float scale, uint16_t* d_out, int out_cstride,
                    int split, pt_stream stream);

/* The ConvNextViT recogniser's kernels one at a time (csrc/cvit_model.hip; since ABI 19): the launches of pt_rec_cvit_forward_net on caller-owned
 * buffers, for op-level tests.  The engine handle and the stream only: no model is loaded.  No allocation, no host synchronisation.  16-bit tensors
 * are in the engine's storage format; split: (hi | lo) rows as everywhere (PT_PRECISION_BF16X3).
 * pt_op_cvit_mlp: d_x [rows, C] fp32 += W2 GELU(W1 xb + b1) + b2 in place (cvit_mlp_kernel).  d_xb 16-bit [rows, C]; d_w1 [4C, C]; d_w2p
 *   [4C / 32][C][32] (weights.py::pack_cvit_mlp); d_b1 fp32 [4C], d_b2 fp32 [C].  C is 96, 192 or 256, rows >= 1 (exactly `rows` rows are read and
 *   written, nothing is padded).  Single-pass modes only: the (hi | lo) modes run two GEMMs instead and get PT_ERR_INVALID here.
 * pt_op_cvit_attention: d_qkv [nchunks * 75, 576] = [q | k | v] of 3 heads x 64 (q already scaled) -> d_out [nchunks * 75, 192]; every chunk of 75
 *   tokens attends to itself only.  split: rows [hi 576 | lo 576] -> [hi 192 | lo 192].
 * pt_op_cvit_dwconv_ln: depthwise 7x7 (padding 3) + bias + LayerNorm(C, eps 1e-6) of d_x fp32 [B, H, W, C] -> 16-bit [B, H, W, C] ([hi C | lo C]
 *   when split).  d_w49 fp32 [49][C] (tap-major).  H is 1, 2, 4 or 8, C <= 512, W >= 1; the LayerNorm tile of (8 H C + 16 H) floats must fit 64 KB of LDS.
 * pt_op_cvit_ln: LayerNorm (d_g == d_beta == NULL: conversion only) of fp32 rows [.., C], C <= 512 -> 16-bit.  mode 0: row to row.  mode 1: rows
 *   (b, y, x) of [B, H, W] maps, H even, to row (b, y / 2, x) of 2C channels at channel offset (y & 1) C; `rows` = B H W.  mode 2: `rows` OUTPUT rows
 *   (line, pos) of 201-token lines gathered from 75-token chunks: pos < 69 token pos of chunk 0, pos < 132 token pos - 63 of chunk 1, else token
 *   pos - 126 of chunk 2; chunk j of a line is chunk d_cmap[3 line + j] of d_x (d_cmap NULL: 3 line + j).  H, W are read in mode 1 only. */
int pt_op_cvit_mlp(pt_engine* e, const uint16_t* d_xb, long long rows, int C, const uint16_t* d_w1, const float* d_b1, const uint16_t* d_w2p,
                   const float* d_b2, float* d_x, pt_stream stream);
int pt_op_cvit_attention(pt_engine* e, const uint16_t* d_qkv, int nchunks, uint16_t* d_out, int split, pt_stream stream);
int pt_op_cvit_dwconv_ln(pt_engine* e, const float* d_x, int B, int H, int W, int C, const float* d_w49, const float* d_bias, const float* d_g,
                         const float* d_beta, uint16_t* d_out, int split, pt_stream stream);
int pt_op_cvit_ln(pt_engine* e, const float* d_x, long long rows, int C, const float* d_g, const float* d_beta, float eps, uint16_t* d_out, int split,
                  int mode, int H, int W, const int32_t* d_cmap, pt_stream stream);

/* ONNX LSTM layer, the recurrence (csrc/lstm_op.hip; since ABI 17).  Hidden size H <= 128; Hp = H rounded up to 16.  The input projection is the
 * caller's: d_pregates [B T rows][pg_cstride] (row b T + t) = X W^T + Wb + Rb from pt_op_conv2d, channel d 4 Hp + gate Hp + unit with the gates in
 * ONNX order i, o, f, c and zeros in the padded units.  d_r_packed: the recurrent weights R [dirs, 4H, H] in MFMA operand order
 * (pdf_table_amd/weights.py::pack_lstm_r; pt_op_lstm_packed_elems(H, dirs, split) 16-bit values, 0 for an unsupported H).  Zero initial states.
 * dirs 1: one direction, walked t = T - 1 .. 0 when reverse; dirs 2: direction 0 forward, 1 reverse.  d_y [B T rows][y_cstride]: h_t at channel
 * d H + unit (the caller zeroes the padding channels once).  split (PT_PRECISION_BF16X3): pre-gates, R and h are (hi | lo) pairs, the lo half of a
 * row at cstride / 2.  c is kept in fp32 for the whole sequence, h is rounded to the storage format once per step.  One workgroup per direction and
 * 16 sequences, no cross-workgroup synchronisation; no allocation and no host synchronisation (capturable). */
int pt_op_lstm(pt_engine* e, const uint16_t* d_pregates, int pg_cstride, const uint16_t* d_r_packed, int T, int B, int H, int dirs, int reverse,
               uint16_t* d_y, int y_cstride, int split, pt_stream stream);
int pt_op_lstm_packed_elems(int H, int dirs, int split);

/* Per-axis strides, 1x3 / 3x1 kernels and rectangular pools (csrc/rect_ops.hip; since ABI 18): what a text-line recogniser's graph holds beyond the
 * square operators above -- PaddleOCR's recognisers shrink the image height and keep its width.  No allocation and no host synchronisation
 * (capturable).  Unsupported arguments return PT_ERR_INVALID with a message naming the values.
 * pt_op_conv2d_rect: dense convolution on the matrix pipe, kh, kw each 1 or 3 and sh, sw each 1 or 2, independently; padding k / 2 per axis, so
 * Ho = (H + 2 (kh / 2) - kh) / sh + 1 and likewise Wo.  Cin a multiple of 32, N of 64; d_w_tiled [N/64][Cin/32][kh kw][64][32]
 * (weights.tile_conv_weight; three K sections w_hi | w_hi | w_lo from tile_conv_weight_x3 when split), d_bias fp32 [N].  fp32 accumulate, bias,
 * act 0 none / 1 ReLU / 2 hardswish, one rounding on store into channels [out_coff, out_coff + N) of pixels out_cstride wide (the lo half
 * out_lo_off further when split; all three multiples of 4).  Only kept outputs are computed and only existing taps multiplied; padding reads as
 * zero and never reaches into the neighbouring image; H == 1 (token rows [B, 1, T, C]) is a first-class case.  No residual operand.  The first 3-tap
 * call on a device raises that kernel's LDS limit (a host-side setting): made inside a stream capture it returns PT_ERR_STATE, so call once before capturing. */
int pt_op_conv2d_rect(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cin, const uint16_t* d_w_tiled, const float* d_bias, int N, int kh,
                      int kw, int sh, int sw, uint16_t* d_out, int out_cstride, int out_coff, int act, int split, int out_lo_off, pt_stream stream);
/* depthwise k x k (k 3 or 5, pad k/2) with a stride per axis (sh, sw each 1 or 2) + bias + act; operands as pt_op_dwconv */
int pt_op_dwconv_rect(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, const float* d_w_taps, const float* d_bias, int k, int sh, int sw,
                      int act, uint16_t* d_out, int split, pt_stream stream);
/* kind 0 max, 1 average over kh x kw windows (1 <= kh, kw <= 4, kh kw >= 2), stride = window, no padding; Ho = H / kh, Wo = W / kw rounded down
 * (trailing rows / columns are dropped).  Max copies the winner's bits (compared on hi + lo when split, both halves copied); average sums in fp32,
 * multiplies by 1 / (kh kw) and rounds (splits again) once.  C a multiple of 8. */
int pt_op_pool_rect(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int C, int kind, int kh, int kw, uint16_t* d_out, int split,
                    pt_stream stream);

/* Dense convolutions with a kernel side of 5, 7 or 9 (csrc/large_conv.hip; added under ABI 19: one new entry point, no existing signature changed,
 * so the version stays): the LKPAN neck of the PP-OCRv4 server detector.  kh, kw each 1, 3, 5, 7 or 9, independently, at least one of them >= 5;
 * stride 1, no dilation, zero padding k / 2 per axis, so the output is [B, H, W, N].  Operands as pt_op_conv2d_rect: Cin a multiple of 32, N of 64;
 * d_w_tiled [N/64][Cin/32][kh kw][64][32] (weights.tile_conv_weight; the three K sections of tile_conv_weight_x3 when split), d_bias fp32 [N]; fp32
 * accumulate, bias, act 0 none / 1 ReLU / 2 hardswish, one rounding on store into channels [out_coff, out_coff + N) of pixels out_cstride wide (the
 * lo half out_lo_off further when split; all three multiples of 4).  Padding reads as zero and never reaches into the neighbouring image; maps
 * smaller than the kernel are a first-class case.  No residual operand.  No allocation and no host synchronisation (capturable), except that the
 * first call with a given kw on a device may raise that kernel's LDS limit (a host-side setting): made inside a stream capture it returns
 * PT_ERR_STATE, so call once before capturing. */
int pt_op_conv2d_large(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cin, const uint16_t* d_w_tiled, const float* d_bias, int N, int kh,
                       int kw, uint16_t* d_out, int out_cstride, int out_coff, int act, int split, int out_lo_off, pt_stream stream);

/* PP-OCRv4 mobile detector blocks (csrc/det_ops.hip; added under ABI 18: two new entry points, no existing signature changed, so the version stays).  No allocation and no host synchronisation (capturable).
 * pt_op_affine_act: y = s2[c] act(s1[c] x + b1[c]) + b2[c] over npix pixels of Cpad channels (a multiple of 8), 16-bit NHWC in the engine's storage
 * format; act 0 none / 1 ReLU / 2 hardswish; the four vectors are fp32 [Cpad]; channels C .. Cpad of the output are written as zeros whatever the
 * vectors hold there.  fp32 arithmetic, one rounding on store; split: (hi | lo) rows of 2 Cpad values, computed on hi + lo and split again.
 * PP-LCNetV3's LearnableAffineBlock (scale x + bias) where it cannot be folded into a convolution, with the activation in front of it.
 * pt_op_db_tail: the tail of a DB head in one launch -- ConvTranspose 2x2 / 2 (C -> C1) + ReLU, ConvTranspose 2x2 / 2 (C1 -> 1), Sigmoid:
 *   out[b, 4y + 2dy + ey, 4x + 2dx + ex] = sigmoid(b2 + sum_c1 W2[c1, 0, ey, ex] relu(b1[c1] + sum_c W1[c, c1, dy, dx] x[b, y, x, c]))
 * d_in 16-bit [B, H, W, Cpad] ([hi | lo] when split; channels C .. Cpad must hold zeros: the kernel reads C rounded up to 8, 16, 24, 32, 48 or 64 channels, i.e. up to 15 of them, against zero weights -- a NaN or Inf there would reach the result), d_w1 fp32 [C, C1, 2, 2],
 * d_b1 fp32 [C1], d_w2 fp32 [C1, 1, 2, 2], d_b2 fp32 [1] (BatchNorm already folded), 1 <= C, C1 <= 64; d_out fp32 [B, 4H, 4W], 16-byte aligned.
 * fp32 accumulation (fused multiply-adds); the C1-channel intermediate is never rounded to 16 bits.
 * Alignment: d_w2, d_out and the four vectors of pt_op_affine_act are read / written 16 bytes at a time and must be 16-byte aligned (as are all
 * 16-bit tensors of this ABI). */
int pt_op_affine_act(pt_engine* e, const uint16_t* d_in, long long npix, int Cpad, int C, const float* d_s1, const float* d_b1, const float* d_s2,
                     const float* d_b2, int act, uint16_t* d_out, int split, pt_stream stream);
int pt_op_db_tail(pt_engine* e, const uint16_t* d_in, int B, int H, int W, int Cpad, int C, int C1, const float* d_w1, const float* d_b1,
                  const float* d_w2, const float* d_b2, float* d_out, int split, pt_stream stream);

/* The tail of a CTC recognition head in one pass (csrc/ctc_ops.hip; added under ABI 19: one new entry point, no existing signature changed, so the
 * version stays).  Input as pt_op_softmax: token rows of 16-bit logits [rows, c_pad] in the engine's storage format, the first c channels real
 * ([hi(c_pad) | lo(c_pad)] when split, value = hi + lo in fp32).  Per row: d_ids[row] = the LOWEST index of the largest of the first c logits (numpy's
 * argmax), d_conf[row] = that class's soft-max probability 1 / sum_k exp(l_k - l_max) in fp32 -- what CTCLabelDecode reads out of the probabilities
 * (preds.argmax(axis=2), preds.max(axis=2)).  Every logit is read once; channels c .. c_pad - 1 are never read.  16-byte loads when c_pad is a
 * multiple of 8 and d_in is 16-byte aligned, 2-byte loads otherwise; any rows >= 1 and c >= 1.  No allocation, no host synchronisation (capturable). */
int pt_op_ctc_greedy(pt_engine* e, const uint16_t* d_in, long long rows, int c_pad, int c, int32_t* d_ids, float* d_conf, int split, pt_stream stream);

/* The tail of a PicoDet ONNX export in one launch (csrc/layout_ops.hip; added under ABI 19: one new entry point, no existing signature changed, so the
 * version stays).  Input: the 2 L output activations of the graph as the ONNX executor holds them, 1 <= levels <= 4: h_scores[l] token rows of 16-bit class
 * PROBABILITIES [B, h_anchors[l], c_pad_s] with the first ncls channels real, h_dists[l] box-distribution logits [B, h_anchors[l], c_pad_d] with the first
 * 32 channels real ([hi(c_pad) | lo(c_pad)] rows of twice that width when split, value = hi + lo as one fp32 add; float(hi) otherwise).  h_scores,
 * h_dists and h_anchors are HOST arrays of `levels` device pointers / anchor counts; they are read before the call returns.  Padding channels may hold
 * anything and are never loaded.  An anchor is a candidate when the fp32 maximum of its ncls values is > thr_lo (strict).  Output, as pt_layout_candidates:
 *   d_counts : int32 [B]       candidates of each page -- every one, also beyond max_cands (zeroed here on the stream: calls do not accumulate)
 *   d_cands  : float32 [B, max_cands, PT_LAYOUT_CAND_FLOATS]   the first max_cands arrivals of a page, in no defined order: (int32 level, int32 anchor,
 *              ncls class probabilities, 32 distribution logits, zeros up to 48); nothing is written outside a page's slab or past its stored records
 * ncls + 32 <= PT_LAYOUT_CAND_FLOATS - 2, i.e. ncls <= 14 (PT_ERR_INVALID otherwise, nothing is launched); B <= 65535.  The values are converted and
 * copied only: sigmoid, soft-max and box arithmetic stay with the caller.  One atomic per wave and page, records written 48 floats at a time by the wave;
 * one launch for all levels and pages, no allocation and no host synchronisation (capturable). */
int pt_op_pico_candidates(pt_engine* e, const uint16_t* const* h_scores, const uint16_t* const* h_dists, const int32_t* h_anchors, int levels, int B,
                          int c_pad_s, int c_pad_d, int ncls, float thr_lo, int max_cands, int32_t* d_counts, float* d_cands, int split,
                          pt_stream stream);

/* PaddleOCR's SLAHead, the table-structure head of SLANet, as one launch (csrc/sla_head.hip; added under ABI 19: three new entry points, no existing
 * signature changed, so the version stays).  The head is an ONNX Loop in the exported graph: an attention-GRU cell walked T times with the arg-max of
 * step t fed back as the one-hot input of step t + 1 (SLAHead.forward in eval mode + AttentionGRUCell).
 * d_fea: token rows 16-bit [B, N, c_pad] in the engine's storage format, the first C channels real ([hi(c_pad) | lo(c_pad)] when split); channels
 * C .. c_pad - 1 may hold anything.  State: h = 0 [H], previous id p = 0.  Once per table P = fea W_i2h^T [N, H] (no bias).  Per step t = 0 .. T - 1:
 *   q = W_h2h h + b_h2h;  e_n = w_score . tanh(P_n + q);  alpha = softmax_n(e);  ctx = sum_n alpha_n fea_n [C];  x = [ctx, onehot_V(p)]
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr);  z = sigmoid(W_iz x + b_iz + W_hz h + b_hz);  c = tanh(W_ic x + b_ic + r (W_hc h + b_hc))
 *   h <- (h - c) z + c   (the one-hot part of W_i* x is a column read of W_i*[:, C + p])
 *   s = W_s2 (W_s1 h + b_s1) + b_s2 [V];  d_probs[b, t] = softmax(s);  d_ids[b, t] = the LOWEST index of max(s);  p <- d_ids[b, t]
 *   d_loc[b, t] = sigmoid(W_l2 (W_l1 h + b_l1) + b_l2) [L]
 * h, the gate sums, both soft-maxes, c and P are fp32 for the whole walk; only the weights and d_fea are 16-bit.
 * eos_id >= 0: a table stops after the first step t > 0 whose id is eos_id; that row is written, the rows after it are written as zeros (d_ids too),
 * d_steps[b] = rows written.  eos_id < 0: every table walks all T steps (what the exported graph does).
 * d_force_ids ([B, T] or NULL): when given, p for step t + 1 is d_force_ids[b, t] (clamped into [0, V)) instead of the step's own arg-max; d_ids still
 * reports the arg-max.  For comparing a 16-bit walk step by step against a reference; products pass NULL.
 * d_w16 / d_f32: the images of pdf_table_amd/weights.py::pack_sla_head, n16 16-bit values (twice that when split: the hi image, then the lo image) and
 * n32 floats as pt_op_sla_packed_elems reports.  d_scratch: pt_op_sla_scratch_bytes(B, N, H) bytes, 16-byte aligned like every pointer here.
 * Outputs: d_probs fp32 [B, T, V], d_loc fp32 [B, T, L], d_ids int32 [B, T], d_steps int32 [B].
 * Built range: H a multiple of 32 up to 256, 1 <= C <= c_pad <= 128 (c_pad a multiple of 8), 1 <= V <= 64, L 4 or 8, 1 <= N <= 256, B >= 1, T >= 1;
 * anything else is PT_ERR_INVALID with a message.  One workgroup per table, no cross-workgroup synchronisation, the step loop bounded by T; one
 * launch, no allocation and no host synchronisation (capturable). */
int pt_op_sla_decode(pt_engine* e, const uint16_t* d_fea, int B, int N, int c_pad, int C, int H, int V, int L, int T, const uint16_t* d_w16,
                     const float* d_f32, void* d_scratch, long long scratch_bytes, int eos_id, const int32_t* d_force_ids, float* d_probs, float* d_loc,
                     int32_t* d_ids, int32_t* d_steps, int split, pt_stream stream);
int pt_op_sla_packed_elems(int H, int C, int V, int L, long long* n16, long long* n32);
int pt_op_sla_scratch_bytes(int B, int N, int H, long long* bytes);
/* SLANetPreprocessor for n table crops of resident pages (csrc/sla_head.hip; model/slanet/processor_slanet.py:32-53): the integer crop read as BGR,
 * ratio = size / max(h, w), cv2.resize (8-bit bilinear) to (int(w ratio), int(h ratio)), (v / 255 - mean) / std with DB's constants indexed in that BGR
 * order, zero padding to size x size at the top-left.  d_pages_rgb uint8 [n_pages, ph, pw, 3]; d_tables / h_tables: the same n pt_tsr_table records on
 * the device and on the host (page, x0, y0, crop_w, crop_h are read; the host copy is checked against the page, so no crop is read out of bounds);
 * d_out fp32 NHWC [n, size, size, 3], channels B, G, R.  No allocation, no host synchronisation (capturable). */
int pt_slanet_preprocess(pt_engine* e, const uint8_t* d_pages_rgb, int n_pages, int ph, int pw, const pt_tsr_table* d_tables, const pt_tsr_table* h_tables,
                         int n, int size, float* d_out, pt_stream stream);
/* Text lines -> cells of the tables a pt_op_sla_decode call walked (csrc/table_match.hip, compiled once, engine-free; added under ABI 19: one new entry
 * point, no existing signature changed, so the version stays): PP-Structure's TableMatch(filter_ocr_result=True).match_result on the device.
 * d_loc fp32 [B, T, L] (L = 4 or 8), d_ids int32 [B, T], d_steps int32 [B] (NULL: every table has T rows) as the head wrote them; d_cell_flags uint8 [V],
 * 1 at the cell tokens (TableLabelDecode.td_token).  Row t of table b is a CELL ROW when t < d_steps[b] and its id is flagged.  d_frames fp32 [B, 4] =
 * (w, h, x0, y0) per table: a cell coordinate is fl32(fl32(loc * w) + x0) at even positions, h and y0 at odd ones (the decode's scaling, then the shift
 * into page pixels); the cell box is the min / max over the row's points.  d_lines fp32 [M, 4] (min x, min y, max x, max y; 16-byte aligned), grouped by
 * table: table b owns lines d_offsets[b] .. d_offsets[b + 1] - 1 (int32 [B + 1], non-decreasing, from 0 to M; a line outside every range is not
 * written, and no index outside [0, M) is ever touched).  d_out int32 [M]: the step index t of the cell row with the smallest (1 - iou, distance, t) --
 * distance and iou in matcher.py's mixed float32 / float64 arithmetic, the line widened to double (see the kernel's header) -- or -1 when the line's
 * max(y1, y2) is strictly below the smallest cell y of its table, or the table has no cell row.  1 <= T <= 2048, 1 <= B <= 65535, M >= 0 (0: nothing
 * is launched).  One launch, no allocation, no host synchronisation (capturable). */
int pt_op_table_match(const float* d_loc, const int32_t* d_ids, const int32_t* d_steps, int B, int T, int L, const uint8_t* d_cell_flags, int V,
                      const float* d_frames, const float* d_lines, const int32_t* d_offsets, int M, int32_t* d_out, pt_stream stream);
/* Text lines -> cells of Lore tables (csrc/lore_match.hip, compiled once, engine-free; added under ABI 20: one new entry point, no existing signature
 * changed, so the version stays): OcrTableToHtmlTask's find_top1_mach_box over the outputs of pt_tsr_decode and pt_tsr_process while they are on the
 * device.  d_dets fp32 [B, PT_TSR_MAX_CELLS, 9] (the quads BEFORE the map back to source pixels), d_axes fp32 [B, PT_TSR_MAX_CELLS, 4] the final logical
 * axes [left, right, top, bottom], unrounded, d_counts int32 [B] (clamped to 0 .. PT_TSR_MAX_CELLS; rows at and beyond the count are never read).
 * d_affine fp64 [B, 6]: per table the inverse 2x3 map (t00 t01 t02 t10 t11 t12); d_offset fp64 [B, 2]: the crop's (x0, y0) on its page.  A vertex is
 * fl32((t00 px + t01 py) + t02) (y alike) plus the offset in double; the cell box is (bottom-left, top-right) = (vertex 3, vertex 1); an axis rounds up
 * where its fraction is > 0.5 (float32).  d_lines fp32 [M, 4] (min x, min y, max x, max y; 16-byte aligned) grouped by table, d_offsets int32 [B + 1] as
 * for pt_op_table_match (no index outside [0, M) is ever touched).  d_out int32 [M]: per line the ROW INDEX of its cell -- the first cell, in the
 * order sorted by (top, left, bottom, right, row), that contains the line grown by 2 pixels, else the first minimum of (1 - iou, corner distance), all
 * in double as table_text_match.find_top1_match computes them -- or -1 in a table whose clamped count is 0.  1 <= B <= 65535, M >= 0 (0: nothing is
 * launched).  One launch of one workgroup per table with 96,000 bytes of LDS: the first call on a device raises the kernel's LDS limit (a host-side
 * setting) and returns PT_ERR_STATE inside a stream capture, so call once before capturing.  No allocation, no host synchronisation. */
int pt_op_lore_match(const float* d_dets, const float* d_axes, const int32_t* d_counts, int B, const double* d_affine, const double* d_offset,
                     const float* d_lines, const int32_t* d_offsets, int M, int32_t* d_out, pt_stream stream);
/* PicoDet post-processing behind the candidate records (csrc/layout_decode.hip, compiled once, engine-free; added under ABI 20: one new entry point, no
 * existing signature changed, so the version stays): LayoutStage.decode_page on the device.  d_counts int32 [B] / d_cands fp32 [B, max_cands,
 * PT_LAYOUT_CAND_FLOATS] as pt_layout_candidates / pt_op_pico_candidates write them (records in no defined order; a count above max_cands reads max_cands
 * records; a record whose level is outside [0, levels) is dropped, its anchor is clamped to >= 0).  h_strides: `levels` ints on the HOST.  probs 0: the
 * class columns are logits (sigmoid here), 1: probabilities.  Per page: per-level top nms_top_k by the largest class score, per class the scores >
 * score_threshold (float32, strict; never a NaN), of those the candidate_size best, greedy hard NMS in float64 with pt_hard_nms's operation order (an entry
 * stays when iou <= nms_threshold), at most keep_top_k picks per class (<= 0: no limit), clip to the page, division by fl32(inp / org).  Equal scores are
 * ordered by (level, anchor) ascending -- the host's arg-sorts have no tie rule -- so the result does not depend on the records' order.
 * d_ndet int32 [B]: every detection of the page, also those beyond max_dets; d_dets fp64 [B, max_dets, 6] = (x0, y0, x1, y1, score, class), classes
 * ascending, within a class in pick order; rows at and beyond the page's count are left as they were.  1 <= ncls <= 14, 1 <= levels <= 4,
 * 1 <= candidate_size <= 256, 1 <= max_cands <= 4096 (what the kernel's LDS plan holds), 1 <= B <= 65535, nms_top_k >= 1, max_dets >= 1: anything else is
 * PT_ERR_INVALID with a message and nothing is launched.  One launch of one workgroup per page, no allocation, no host synchronisation (capturable). */
int pt_op_layout_decode(const int32_t* d_counts, const float* d_cands, int B, int max_cands, int ncls, int levels, const int32_t* h_strides, int inp_h,
                        int inp_w, int org_h, int org_w, int probs, float score_threshold, double nms_threshold, int nms_top_k, int candidate_size,
                        int keep_top_k, int max_dets, int32_t* d_ndet, double* d_dets, pt_stream stream);
/* DocXLayout's region list and reading order behind pt_docx_decode (csrc/docx_order.hip, compiled once, engine-free; added under ABI 21: one new entry
 * point, no existing signature changed, so the version stays): docx_page_result (pdf_table_amd/docxlayout_stage.py) on the device, step for step.
 * d_counts int32 [B][2], d_recs fp32 [B][2][K][PT_DOCX_REC_FLOATS], d_keep uint8 [B][2][K] as pt_docx_decode writes them (a count outside [0, K] is
 * clamped; use_nms 0: every row below the count is read, whatever its keep flag).  a00 .. a12: the float64 map from head-map to page pixels
 * (centernet_decode_affine), applied as (a x + b y) + c and stored as float32.  Rows of a class with float32 score > scores_thresh, one zero placeholder
 * per empty class, sub-branch classes shifted by n_main; above top_k rows the (rows - top_k)-th smallest score is the cut and ties at it stay;
 * vertices through rintf; every region (class < n_main) goes to the sub-field (class >= n_main) that covers most of it when that is more than a
 * tenth (float64 convex clipping in the host's operation order: the rate is the host's bit for bit), and fields, regions in a field and regions
 * outside all fields are put in order by CPython's list.sort for fewer than 64 elements, replayed on the bits of the comparator's `<`.
 *   d_nout int32 [B]          regions of the page (0 when flagged)
 *   d_flag int32 [B]          0: served.  1: the page needs the host route -- a list of 64 or more blocks in one of the sorts, scores_thresh <= 0, a vertex
 *                             that is not finite, or a comparison in which the host divides by zero
 *   d_rows fp32 [B][2 K][6]   (x0, y0, x2, y2 of the rounded vertices, the float32 score, the 0-based class) in reading order; rows at and behind
 *                             d_nout are not written
 * atan2 / sin / cos of a list's main angle are the device library's: exact for an axis-aligned list (angle 0), last-bit differences from the host's
 * libm otherwise.  PT_ERR_INVALID with a message and nothing launched: K > PT_DOCX_MAX_K, num_classes > 16, n_main >= num_classes, B < 1 (or any of them
 * below its lower bound, top_k < 1).  One launch of one workgroup per page, 32 KB of LDS at most, no allocation, no host synchronisation (capturable). */
int pt_op_docx_order(const int32_t* d_counts, const float* d_recs, const uint8_t* d_keep, int B, int K, double a00, double a01, double a02, double a10,
                     double a11, double a12, float scores_thresh, int top_k, int num_classes, int n_main, int use_nms, int32_t* d_nout, int32_t* d_flag,
                     float* d_rows, pt_stream stream);

/* DBPostProcess score_mode "slow" (db_pp/processor_ocr_db_pp.py:270-289, box_score_slow): the candidates with their traced contours, and the mean of the
 * probability map over each contour's own polygon (csrc/det_poly_score.hip, compiled once, engine-free; added under ABI 21: two new entry points, no
 * existing signature changed, so the version stays).
 * pt_db_contour_candidates_batch (HOST): pt_db_candidates_batch -- same tracer, same max_candidates cut before the min_size test, same order, h_boxes /
 *   h_sside / n_out bit for bit -- which also returns the contour of every kept candidate: the CHAIN_APPROX_SIMPLE vertices as the tracer emits them
 *   (hole contours included: RETR_LIST returns them and the reference scores them), int32 (x, y) in map pixels, flat in h_points [point_cap][2],
 *   page-major, in candidate order; h_offsets int32 [n * cap + 1]: candidate j (counted over all pages) owns points h_offsets[j] .. h_offsets[j + 1] - 1,
 *   sum(n_out) + 1 entries are written.  *n_points_needed: the points there are.  Where that is more than point_cap NO point is written, the rest of the
 *   output is complete and the call returns PT_OK: grow the buffer and call again.  Pages run on n_threads threads inside the library (0: all).
 * pt_op_det_poly_scores: d_prob fp32 [n, net_h, net_w]; d_points int32 [n_points][2]; d_offsets / h_offsets int32 [nb + 1]; d_pages / h_pages int32 [nb]:
 *   the page of each candidate.  The h_ arrays are the HOST copies of the d_ arrays: every limit is checked on them before anything is launched.
 *   Per candidate: the bounding rectangle of its points clipped to the map; the mask cv2.fillPoly(mask, [points - (xmin, ymin)], 1) -- the 8-connected
 *   Bresenham outline of every edge (left to right, exact halves toward the start) united with the scan-line interior for ymin <= y < ymax (edges in
 *   16.16 fixed point with a truncated slope, sorted crossings paired, spans [(xa + 0x8000) >> 16, (xb + 0x8000) >> 16]); points may lie outside the
 *   map.  d_scores fp32 [nb] = (float)(sum / count) of the map under the mask, added in double, or 0 when count == 0 (pt_det_box_scores's contract: a
 *   drop-in for pt_db_finalize_batch); d_sums fp64 [nb] / d_counts int32 [nb]: the sum and the pixel count themselves, either may be NULL.
 *   d_work: nb * PT_DET_POLY_WORK_BYTES bytes, 8-byte aligned (per-band partial results); work_bytes: its size.  A candidate's rows are split over up to
 *   PT_DET_POLY_BANDS workgroups and added in band order by a second kernel: two launches, no atomics on floating point, the same bits in every call.
 *   PT_ERR_INVALID with a message, nothing launched and nothing written: nb < 0, offsets that are not non-decreasing or leave [0, n_points], a page
 *   outside [0, n), net_w > PT_DET_POLY_MAX_W (the kernel keeps one int32 per pixel of a row and wave in 64 KiB of LDS), a work buffer too small.
 *   nb == 0 launches nothing.  No allocation, no host synchronisation (capturable). */
#define PT_DET_POLY_MAX_W 4096
#define PT_DET_POLY_BANDS 16
#define PT_DET_POLY_WORK_BYTES (PT_DET_POLY_BANDS * 12)
int pt_db_contour_candidates_batch(const uint32_t* h_bitmaps, int n, int net_h, int net_w, int max_candidates, float min_size, int n_threads,
                                   float* h_boxes, float* h_sside, int cap, int* n_out, int32_t* h_points, long long point_cap,
                                   int32_t* h_offsets, long long* n_points_needed);
int pt_op_det_poly_scores(const float* d_prob, int n, int net_h, int net_w, const int32_t* d_points, int n_points, const int32_t* d_offsets,
                          const int32_t* h_offsets, const int32_t* d_pages, const int32_t* h_pages, int nb, float* d_scores, double* d_sums,
                          int32_t* d_counts, void* d_work, long long work_bytes, pt_stream stream);

/* The TEDS table metric's two hot parts (csrc/teds.hip, compiled once, engine-free; added under ABI 21: new entry points, no existing signature
 * changed, so the version stays).  pdf_table_amd/table_metric.py packs these arrays and states the same arithmetic on the host.
 * pt_op_teds_cost: C = levenshtein(a, b) / max(len a, len b) in float64 (0 where both are empty) for every (row content, column content) of P table
 *   pairs.  d_tok int32 [n_tok]: token ids, compared as whole int32 values; d_coff / h_coff int32 [n_cont + 1]: content k owns tokens coff[k] ..
 *   coff[k + 1] - 1 (from 0, non-decreasing, at most 1024 tokens per content); d_pairs / h_pairs int64 [P, 5] = (first row content, row contents nr,
 *   first column content, column contents nc, offset of the pair's nr x nc row-major matrix in d_C, in elements); the two ranges may overlap, and a
 *   content against itself is 0 without a token read.  d_C fp64 [c_elems].  The h_ arrays are the HOST copies of the d_ arrays: every limit is checked
 *   on them, and anything outside (a content above 1024 tokens among them) is PT_ERR_INVALID with a message, nothing launched, nothing written.
 *   The quotient is one division of two exact integers.  0 <= P <= 65535.  One launch, no allocation, no host synchronisation (capturable).
 * pt_op_teds_dist: d_out fp64 [P] = the ordered tree edit distance (insert = delete = 1) of each pair, one workgroup per pair.  Trees are flattened in
 *   postorder.  d_node int32 [n_nodes, 4] = (tag id, colspan, rowspan, content id; spans -1 and content id -1 where the node carries none), 16-byte
 *   aligned; d_lml int32 [n_nodes]: the node's leftmost leaf, as an index inside its tree; d_kr int32 [n_kr]: per tree its keyroots, ordered by
 *   (height, size descending); d_grp int32 [n_grp]: per tree ngrp + 1 offsets into its keyroot list, one group per height that has a keyroot.
 *   d_pairs / h_pairs int64 [P, 16] = (n1, first node of tree 1, n2, first node of tree 2, first keyroot 1, keyroots 1, first group offset 1, groups
 *   1, the same four of tree 2, offset of the pair's cost matrix in d_C, its rows, its columns, offset of the pair's scratch in doubles).  Renaming
 *   node i into node j costs 1 where tag, colspan or rowspan differ, else C[content i, content j] where both carry a content, else 0.  1 <= n <=
 *   4096 per tree; a pair's scratch is pt_op_teds_scratch_bytes(n1, n2) bytes (two n1 x n2 fp64 planes), the pairs' regions ascending and disjoint.
 *   Checked on the host copies: anything outside (4097 nodes, a scratch too small) is PT_ERR_INVALID with a message, nothing launched.  The kernel
 *   clamps every index it reads from device memory all the same.  No atomics, no state shared between workgroups.  One launch, no allocation, no host
 *   synchronisation (capturable). */
int pt_op_teds_scratch_bytes(int n1, int n2, long long* bytes);
int pt_op_teds_cost(const int32_t* d_tok, long long n_tok, const int32_t* d_coff, const int32_t* h_coff, int n_cont, const int64_t* d_pairs,
                    const int64_t* h_pairs, int P, double* d_C, long long c_elems, pt_stream stream);
int pt_op_teds_dist(const int64_t* d_pairs, const int64_t* h_pairs, int P, const int32_t* d_node, const int32_t* d_lml, long long n_nodes,
                    const int32_t* d_kr, long long n_kr, const int32_t* d_grp, long long n_grp, const double* d_C, long long c_elems, double* d_scratch,
                    long long scratch_bytes, double* d_out, pt_stream stream);

/* The WTW cell metric's matching (csrc/cell_metric.hip, compiled once, engine-free; added under ABI 21: a new entry point, no existing signature
 * changed, so the version stays): TableEval.bubble_sort + PairTable.matching / eval_axis (utils/eval/eval_utils.py:23-113,
 * entity/table_entity.py:630-656) for P (prediction, truth) table pairs in one launch, one workgroup per pair.  pdf_table_amd/cell_metric.py packs
 * these arrays and states the same rule on the host.
 *   d_boxes fp64 [N, 4] = (x1, y1, x3, y3) of every cell of every table of the chunk (points 1 and 3 of the quad: the only ones compute_iou reads),
 *   16-byte aligned, finite; d_axes int32 [N, 4] = the cell's logical axes as the files list them, 16-byte aligned.
 *   d_pairs / h_pairs int64 [P, 4] = (first prediction cell, prediction cells, first truth cell, truth cells); the ranges may overlap.
 *   d_moff / h_moff int64 [P]: where the pair's matches start in d_match, ascending and disjoint (the prefix sum of the truth counts, or wider).
 *   d_match int32 [match_elems]: per truth cell, in the truth's input order, the input index (inside its table) of the FIRST prediction cell with
 *   iou >= iou_threshold, or -1 -- first in the order a stable sort of the predictions by (axis[2], axis[0], axis[3], axis[1]) leaves, never the best
 *   IoU; a prediction may serve several truth cells.  d_counts int32 [P, 2] = (matches, matches whose four axes equal the truth cell's).
 *   IoU in float64, the reference's operations in its order: 0 where max(x1) >= min(x3) or min(y3) <= max(y1), else Sx / ((S1 + S2) - Sx).
 * The h_ arrays are the HOST copies of the d_ arrays; every limit is checked on them: a count outside 0 .. PT_CELL_METRIC_MAX, a range outside
 * [0, N], matches outside d_match or a threshold that is not positive is PT_ERR_INVALID with a message, nothing launched, nothing written.  The kernel
 * clamps every index it reads from device memory all the same.  A pair with no truth cell writes its counts only; one with no prediction cell writes
 * -1.  P == 0 launches nothing.  0 <= P <= 65535.  No scratch, no atomics, no state shared between workgroups.  One launch, no allocation, no host
 * synchronisation (capturable). */
#define PT_CELL_METRIC_MAX 4096
int pt_op_cell_metric(const double* d_boxes, const int32_t* d_axes, long long N, const int64_t* d_pairs, const int64_t* h_pairs, int P,
                      const int64_t* d_moff, const int64_t* h_moff, double iou_threshold, int32_t* d_match, long long match_elems, int32_t* d_counts,
                      pt_stream stream);

/* ---- introspection used by bench.py (HIP-event timing of the dominant kernel) ------------------ */
/* ---- image classification (PP-LCNet) ------------------------------------------------------------
 * Replaces ClsImagePulcTask._preprocess/_run_model (ocr_pdf/cls_image_pulc_task.py:48-84): PPLCNetImageProcessor
 * (cls/image_processing_pplcnet.py:327-455: Pillow bilinear resize, * 1/255, ImageNet mean/std) and PPLCNet.forward
 * (cls/cls_pp_lcnet.py:262-283).  The soft-max / top-k of the post-processor (:155-192) stays on the host.
 * Up to PT_CLS_SLOTS classifiers are resident at once: load slot k with pt_weights_load(e, PT_MODEL_PPLCNET + k, ..).
 * `textline`: the task's stride_list is [2,[2,1],[2,1],[2,1],[2,1]] (textline_orientation, language_classification;
 * cls/configuration_cls_pulc.py:20-39). */
#define PT_CLS_SLOTS 4
#define PT_CLS_MAX_CLASSES 16
typedef struct pt_cls_image {
  int64_t offset; /* bytes from d_base to an RGB uint8 [h, w, 3] image */
  int32_t h, w;
} pt_cls_image;

/* d_images: DEVICE array of n descriptors; max_h / max_w: upper bounds of their sizes (host-known);
 * d_out_bf16: bf16 NHWC4 [n, out_h, out_w, 4] (8 channels [hi rgb0 | lo rgb0] in PT_PRECISION_BF16X3). */
int pt_cls_preprocess(pt_engine* e, const uint8_t* d_base, const pt_cls_image* d_images, int n, int max_h, int max_w,
                      int out_h, int out_w, uint16_t* d_out_bf16, pt_stream stream);
/* d_logits: float32 [n, PT_CLS_MAX_CLASSES], the first *n_classes columns valid (n_classes may be NULL). */
int pt_cls_forward_net(pt_engine* e, int slot, const uint16_t* d_input_bf16, int n, int in_h, int in_w, int textline,
                       float* d_logits, int* n_classes, pt_stream stream);
/* pre-process + network for n images. */
int pt_cls_forward(pt_engine* e, int slot, const uint8_t* d_base, const pt_cls_image* d_images, int n, int max_h, int max_w,
                   int out_h, int out_w, int textline, float* d_logits, int* n_classes, pt_stream stream);
/* Text lines cut from resident pages (the per-line loop of OcrSystemTask.text_line_orientation,
 * ocr_system_task.py:395-439: order_point -> crop_image -> classifier): d_lines / h_crop_px as for pt_rec_forward;
 * max_crop_h / max_crop_w: upper bounds of the lines' crop sizes. */
int pt_cls_forward_lines(pt_engine* e, int slot, const uint8_t* d_pages_rgb, int n_pages, int h, int w,
                         const pt_rec_line* d_lines, const int64_t* h_crop_px, int n_lines, int max_crop_h, int max_crop_w,
                         int out_h, int out_w, int textline, float* d_logits, int* n_classes, pt_stream stream);
/* The same logits as pt_cls_forward_lines (bit for bit), without h_crop_px and without the crop buffers it shares with
 * pt_rec_forward*: one kernel samples every crop pixel from the pages while it resizes and normalises, into the call's
 * own input buffer; the network runs in an activation arena of its own (see the concurrency rules at the top).
 * Micro-batched like pt_cls_forward_lines (PT_CLS_MICROBATCH lines per network call).  A line whose crop_w or crop_h
 * is <= 0 is read as a 1 x 1 crop sampled at its origin. */
int pt_cls_forward_lines_direct(pt_engine* e, int slot, const uint8_t* d_pages_rgb, int n_pages, int h, int w,
                                const pt_rec_line* d_lines, int n_lines, int max_crop_h, int max_crop_w, int out_h, int out_w,
                                int textline, float* d_logits, int* n_classes, pt_stream stream);

/* on = 1: every kernel launch of the forward calls is bracketed by hipEvents on `stream`; on = 2 + class: only the
 * launches of that kernel class (an event pair costs a few microseconds of idle GPU per launch, which adds up over the
 * ~1000 launches of a four-stage step); 0: off.  pt_profile_read returns accumulated milliseconds, launch count and
 * algorithmic FLOP per kernel class. */
#define PT_PROF_CONV3X3 0
#define PT_PROF_CONV1X1 1
#define PT_PROF_STEM 2
#define PT_PROF_OTHER 3
#define PT_PROF_NCLASS 4
int pt_profile_enable(pt_engine* e, int on);
int pt_profile_read(pt_engine* e, double* ms_per_class, long long* launches_per_class, double* flop_per_class);
/* Per-label readout of the launches recorded since the last read (pt_profile_enable(e, 1)): text lines
 * "label<TAB>launches<TAB>ms<TAB>algorithmic FLOP<TAB>algorithmic bytes<NL>" into buf (NUL-terminated; PT_ERR_INVALID if cap is too small).
 * Consumes the records like pt_profile_read.  bench.py's roofline.by_class is built from it.  Since ABI 12. */
int pt_profile_read_labels(pt_engine* e, char* buf, int cap);

/* ---- MtlTabNet (second half): backbone, then the decoders below -------------------------------
 * TableResNetExtra.forward (model/table/mtl_tabnet/table_resnet_extra.py:268-318) of the configuration in
 * mtl_tabnet_config.py:41-53: d_x bf16 [n, H, W, 32] NHWC (channels 0..2 = the normalised image, the rest zero; BF16X3:
 * [hi 32 | lo 32]), H and W multiples of 8 -> d_f3 fp32 [n, H/8, W/8, 512], the feature map the decoders read (feat[-1]). */
int pt_tsr_mtl_backbone_net(pt_engine* e, const uint16_t* d_x, int n, int H, int W, float* d_f3, pt_stream stream);

/* MtlTabNet test-time pre-processing (mtl_tabnet_config.py:136-160: TableResize(keep_ratio, long_size = 480) -> TablePad(480 x 480,
 * pad_val 0) -> ToTensorOCR -> NormalizeOCR(mean 0.5, std 0.5); model/table/lgpma/lgpma_preprocess.py:1067-1093, 1128-1152) of n
 * table crops given as rectangles of resident pages (pt_tsr_table.page / x0 / y0 / w / h; the affine fields are not read).  The
 * long side becomes `size`, the short side int(size / long * short) (cv2.resize INTER_LINEAR, 8-bit), the rest of the size x size
 * canvas is 0 BEFORE the normalisation, i.e. -1 after it.  d_out bf16 [n, size, size, 32] (BF16X3: [hi 32 | lo 32]), channels
 * 0..2 in the crop's own channel order (mean and std are the same for all three).  The resized size of crop i is what
 * pt_tsr_mtl_resized_size returns (host arithmetic in double, as the reference's Python floats). */
int pt_tsr_mtl_preprocess(pt_engine* e, const uint8_t* d_pages, int n_pages, int h, int w, const pt_tsr_table* d_tables, int n, int size,
                          uint16_t* d_out, pt_stream stream);
void pt_tsr_mtl_resized_size(int crop_w, int crop_h, int size, int32_t* out_w, int32_t* out_h);

/* The three decoders of MtlTabNet (master_decoder.py:354-517: greedy_forward / decode_test) for a batch of tables, KV-cached.
 * pt_weights_load(PT_MODEL_MTL_DECODER) first.  pt_tsr_mtl_decoder_config: the blob's 13 configuration integers (structure
 * classes, cell classes, <SOS>, <EOS>, <PAD>, max_seq_len, the same three ids and the limit of the cell alphabet, the two
 * structure ids that open a non-empty cell, padded d_ff).
 * pt_tsr_mtl_structure: d_f3 fp32 [n, hw, 512] = the backbone's last map (pt_tsr_mtl_backbone_net; NHWC = flattened row-major
 * like the reference's view + permute).  Every table is decoded as the reference decodes a batch of ONE: it stops at its own <EOS>
 * (or after max_seq_len + 1 positions).  d_tag_logits fp32 [n, max_seq_len + 1, classes] (raw cls_fc outputs), d_boxes fp32 [n,
 * max_seq_len + 1, 4] (sigmoid); h_lens[n] = positions written per table (the length of the reference's output), h_cell_counts[n] =
 * positions whose arg-max is '<td></td>' or '<td' (decode_test :389-392).  Synchronous: the call polls the sequences' end flags.
 * pt_tsr_mtl_cells: the cell-content decoder for those cells (ordered by table, then position; total = sum of h_cell_counts):
 * d_cell_ids int32 / d_cell_prob fp32 [total, max_seq_len_cell + 1] = arg-max and its soft-max probability per position,
 * d_cell_logits fp32 [total, max_seq_len_cell + 1, cell classes] or NULL; h_steps[n] = positions decoded per table (all cells of a
 * table share it: the loop ends when every cell emitted <EOS> in the same step, :451-453; 0 = no cells).
 * force_redecode = 1 runs the reference's own O(L^2) schedule (every step decodes the whole prefix again) instead of the cache:
 * the engine switches to it by itself when a <PAD> token is emitted (the reference's padding mask is not causal); tests use the
 * flag to show that both schedules agree.
 * TableMasterDecoder (master_decoder.py:532-645, model="TableMaster" of ocr_table_structure_task.py:71) is the same decoder without the
 * cell-content layer: a blob that says "0 cell classes" (pdf_table_amd/weights.py::pack_mtl_decoder on a state_dict without cell tensors).
 * pt_tsr_mtl_structure then reports zero cells for every table and pt_tsr_mtl_cells(total = 0) is a no-op.  Its greedy_forward (:599-608)
 * never stops at <EOS> (the output is the last of max_seq_len + 1 passes; the convertor cuts at <EOS>): the KV-cached loop's stop at
 * <EOS> is that output's prefix, and a table still running when a <PAD> appears runs on to the length limit as the reference's does. */
int pt_tsr_mtl_decoder_config(pt_engine* e, int32_t out13[13]);
int pt_tsr_mtl_structure(pt_engine* e, const float* d_f3, int n, int hw, float* d_tag_logits, float* d_boxes, int32_t* h_lens,
                         int32_t* h_cell_counts, int force_redecode, pt_stream stream);
int pt_tsr_mtl_cells(pt_engine* e, int total, int32_t* d_cell_ids, float* d_cell_prob, float* d_cell_logits, int32_t* h_steps,
                     int force_redecode, pt_stream stream);

/* The decoders' attention kernels one at a time (csrc/mtl_decoder.hip; since ABI 20): the launch functions of the decoding loops on caller-owned
 * buffers, for op-level tests.  The engine handle and the stream only: no model is loaded.  No allocation on the device, no host synchronisation.  16-bit
 * tensors are in the engine's storage format; split: rows [hi C | lo C] (PT_PRECISION_BF16X3).  d = 512 = 8 heads of 64; a key is stored already
 * divided by 8.  Arguments a kernel cannot take return PT_ERR_INVALID with a message naming the value, and nothing is launched.
 * pt_op_mtl_pick_split: how the loops cut hw keys into slices for `ntiles` query tiles: 1 <= *nsplit <= 16 slices of *keys_per_split keys (a multiple
 *   of 32), (*nsplit - 1) * *keys_per_split < hw <= *nsplit * *keys_per_split.  Host arithmetic.
 * pt_op_mtl_cross_attention: source attention.  kernel: PT_MTL_ATTN_STREAM (mtl_cross_decode_kernel, one query per tile), PT_MTL_ATTN_STREAM8 (the
 *   same over the e4m3 copy; single-pass modes only), PT_MTL_ATTN_MFMA (mtl_cross_attn_kernel, up to 32 queries per tile).  d_q / d_att: npos * Mp
 *   rows of 512 (row = position * Mp + sequence, sequences 0 .. M - 1 in use).  d_kv: 16-bit [n_tables * hw, 5120] = [k | v] of five layer slots, or
 *   its e4m3 copy (uint8, pt_op_mtl_kv_fp8) for STREAM8; the layer reads slot `slot`.  h_tiles: HOST int32 [ntiles, 4] = (table, first query row,
 *   queries, row stride), copied to d_tiles (device, 16 bytes per tile) on the stream; it must stay valid until that copy has run.  Every query row
 *   belongs to at most one tile.  The hw keys of a table are read in nsplit slices of keys_per_split (a multiple of 32; the slices must cover hw and
 *   the last one must hold a key).  nsplit == 1: normalised rows -> d_att, rows in no tile are not written.  nsplit > 1: per-slice (max, sum) ->
 *   d_mlpart fp32 [nsplit, npos * Mp, 8, 2] and accumulators -> d_opart fp32 [nsplit, npos * Mp, 512], then mtl_cross_combine_kernel merges them
 *   into EVERY row (position < npos, sequence < M) of d_att: the tiles must cover exactly those rows.  nb == 2 (stream kernels): a second layer in
 *   the same launches, reading slot + 1, its q / att rows row_bs elements behind the first layer's, its partials opart_bs / ml_bs floats behind.
 * pt_op_mtl_self_attention: self-attention of positions p0 .. p1 of M sequences over the cache d_cache [p1 + 1 positions][Mp][q 512 | k 512 | v 512]
 *   (split: [hi 1536 | lo 1536]); the query at position p reads keys 0 .. p, or -- where d_tok[p * Mp + sequence] == pad -- all p1 + 1 positions
 *   with equal weights (the reference's padding mask).  d_att [(p1 - p0 + 1) * Mp, 512], sequences >= M are not written.  nb == 2: a second layer
 *   cache_bs / att_bs elements behind.  p0 == p1: a KV-cached step; p0 == 0: the re-decode mode.
 * pt_op_mtl_kv_fp8: d_out[i] = e4m3(8 d_kv[i]) (saturating at +-448, round to nearest even), n_elems a multiple of 8. */
#define PT_MTL_ATTN_STREAM 0
#define PT_MTL_ATTN_STREAM8 1
#define PT_MTL_ATTN_MFMA 2
int pt_op_mtl_pick_split(int ntiles, int hw, int32_t* nsplit, int32_t* keys_per_split);
int pt_op_mtl_cross_attention(pt_engine* e, int kernel, const uint16_t* d_q, const void* d_kv, int n_tables, int hw, int slot, const int32_t* h_tiles,
                              int ntiles, int32_t* d_tiles, int keys_per_split, int nsplit, int npos, int M, int Mp, float* d_opart, float* d_mlpart,
                              uint16_t* d_att, int split, int nb, long long row_bs, long long opart_bs, long long ml_bs, pt_stream stream);
int pt_op_mtl_self_attention(pt_engine* e, const uint16_t* d_cache, const int32_t* d_tok, int pad, int p0, int p1, int Mp, int M, uint16_t* d_att, int split,
                             int nb, long long cache_bs, long long att_bs, pt_stream stream);
int pt_op_mtl_kv_fp8(pt_engine* e, const uint16_t* d_kv, long long n_elems, uint8_t* d_out, pt_stream stream);

/* The Lore processor's kernels one at a time (csrc/lore_processor.hip; since ABI 21): the launches of pt_tsr_process on caller-owned buffers, for
 * op-level tests.  The engine handle and the stream only: no model is loaded.  No allocation on the device, no host synchronisation.  16-bit tensors
 * are in the engine's storage format; split: rows [hi C | lo C] (PT_PRECISION_BF16X3).  h_counts: HOST int32 [n_tables], 0 <= count <=
 * PT_TSR_MAX_CELLS; N = their sum; token t of the batch is row r of table b in the order of the tables.  Npad: rows of the token matrices, a
 * multiple of 128, >= N.  N == 0 launches nothing.  Arguments a kernel cannot take return PT_ERR_INVALID, and nothing is launched.
 * pt_op_lore_tok_prepare: token t = d_logi[b][r][0:256] (fp32 [n_tables, PT_TSR_MAX_CELLS, 256]) + with use_pe the four position rows
 *   x_pe[p0] + y_pe[p1] + x_pe[p2] + y_pe[p5], p_i = clamp((int) d_dets[b][r][i], 0, 255) (d_dets fp32 [n_tables, PT_TSR_MAX_CELLS, 9], tables fp32
 *   [256, 256]) -> d_x0 [Npad, 256] and channels [256, 512) of d_cat [Npad, 512]; rows [N, Npad) are written as 0.  d_tok: device int32 [2 N], receives
 *   the (table, row) map of the tokens, which pt_op_lore_scatter4 reads.
 * pt_op_lore_norm: alpha (x - mean) / (std + 1e-6) + bias over the 256 channels of fp32 rows (unbiased std) -> 16-bit [rows, 256]; alpha == bias ==
 *   NULL: the conversion alone.
 * pt_op_lore_cvt_logic: fp32 [Npad, 8] (4 valid) -> 16-bit [Npad, 32], channels 4 .. 31 zero.
 * pt_op_lore_attention: d_qkv [Npad, 768] = [q | k | v] of 8 heads x 32 -> d_out [Npad, 256] = softmax(q k^T / sqrt(32)) v over the cells of the
 *   token's own table; rows [N, Npad) are neither read nor written.  d_tiles: device int32 [3 * sum ceil(count / 32)], receives the tile list.
 * pt_op_lore_scatter4: d_out[b][r][0:4] (fp32 [n_tables, PT_TSR_MAX_CELLS, 4]) = d_x[t][0:4] (fp32 [>= N, 8]) for the N tokens of d_tok. */
int pt_op_lore_tok_prepare(pt_engine* e, const float* d_logi, const float* d_dets, const int32_t* h_counts, int n_tables, int use_pe, const float* d_x_pe,
                           const float* d_y_pe, int Npad, int32_t* d_tok, uint16_t* d_x0, uint16_t* d_cat, int split, pt_stream stream);
int pt_op_lore_norm(pt_engine* e, const float* d_x, int rows, const float* d_alpha, const float* d_bias, uint16_t* d_out, int split, pt_stream stream);
int pt_op_lore_cvt_logic(pt_engine* e, const float* d_x, uint16_t* d_out, int Npad, int split, pt_stream stream);
int pt_op_lore_attention(pt_engine* e, const uint16_t* d_qkv, const int32_t* h_counts, int n_tables, int Npad, int32_t* d_tiles, uint16_t* d_out, int split,
                         pt_stream stream);
int pt_op_lore_scatter4(pt_engine* e, const float* d_x, const int32_t* d_tok, int N, float* d_out, pt_stream stream);


/* ---- image-page straightening before detection (OcrSystemTask.image_pre_process, ocr_system_task.py:441-491) ----------------
 * Engine-free: these read and write uint8 RGB pages [n, h, w, 3] only (csrc/page_pre.hip, compiled once).
 * pt_page_line_mask: the deskew's horizontal line mask of n same-shape pages in one launch -- 255 - gray (cv2's fixed-point
 *   BGR2GRAY on the reference's BGR = the same weights on R, G, B here), adaptiveThreshold(GAUSSIAN_C, BINARY, 15, -2), then erode
 *   and dilate with a (w / 40) x 1 rectangle.  d_bits uint64 [n, h, (w + 63) / 64]: bit b of word q = column 64 q + b (1 = line pixel),
 *   bits past the page end 0.  w >= 40 (cv2 rejects a zero-width element).
 * pt_page_line_angles (HOST): RETR_EXTERNAL contours of those masks; per page, get_line_angle of every contour wider than min_width
 *   (the reference's diff_angle, 400), in cv2's contour order: h_angles double [n, cap], h_counts int32 [n].  n_threads in 1 .. 16.
 * pt_page_warp_cubic: cv2.warpAffine(INTER_CUBIC, BORDER_REPLICATE) at the page's own size.  Output page j of d_out [m, h, w, 3] is page
 *   d_idx[j] of d_pages warped by d_minv[j] (double [m, 6]: the INVERSE map, as warpAffine computes it); an index outside 0 .. n - 1
 *   leaves output j unwritten.
 * pt_page_quarter_turn: cv2.rotate with cv2's codes; d_out [n, w, h, 3] for the 90-degree turns, [n, h, w, 3] for ROTATE_180.
 * pt_page_pre_tables: the host tables the kernels use (15 blur taps, sum 256; 1024 x 16 bicubic weights), for tests. */
#define PT_ROTATE_90_CLOCKWISE 0
#define PT_ROTATE_180 1
#define PT_ROTATE_90_COUNTERCLOCKWISE 2
int pt_page_line_mask(const uint8_t* d_pages, int n, int h, int w, uint64_t* d_bits, pt_stream stream);
int pt_page_line_angles(const uint64_t* h_bits, int n, int h, int w, int min_width, int n_threads, double* h_angles, int cap,
                        int32_t* h_counts);
int pt_page_warp_cubic(const uint8_t* d_pages, int n, int h, int w, const double* d_minv, const int32_t* d_idx, int m, uint8_t* d_out,
                       pt_stream stream);
int pt_page_quarter_turn(const uint8_t* d_pages, int n, int h, int w, int code, uint8_t* d_out, pt_stream stream);
int pt_page_pre_tables(int32_t* h_blur_taps, int16_t* h_cubic);

#ifdef __cplusplus
}
#endif
#endif /* PDFTABLE_HIP_H */

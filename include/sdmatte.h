/* sdmatte.h - C ABI of the MI355X-native SDMatte engine (libsdmatte_hip.so, gfx950 only).
 *
 * The reference (flybirdxx/ComfyUI-SDMatte) is pure Python and has no FFI; this header is the boundary a
 * maintainer binds with ctypes.  Each entry point names the reference interface it
 * replaces.  Plain pointers and sizes only - no torch types.  All functions return 0 on success or a
 * negative sdm_status; sdm_last_error() gives the message (the Python shim raises RuntimeError with it,
 * mirroring how exceptions propagate to ComfyUI in the reference).  Nothing here ever abort()s.
 *
 * Pointer kinds: every data pointer is either a HOST pointer or a DEVICE pointer of the engine's GPU,
 * selected by the `ptr_kind` argument (SDM_PTR_HOST / SDM_PTR_DEVICE).  Device pointers are what
 * `tensor.data_ptr()` returns for PyTorch-ROCm tensors at the node boundary.  Any other `ptr_kind` is SDM_ERR_INVALID: nothing is queued and no
 * output is written.
 */
#ifndef SDMATTE_H_
#define SDMATTE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdm_ctx sdm_ctx;

enum sdm_status {
  SDM_OK = 0,
  SDM_ERR_INVALID = -1,   /* bad argument / shape */
  SDM_ERR_HIP = -2,       /* HIP runtime error */
  SDM_ERR_STATE = -3,     /* weights not loaded / finalised */
  SDM_ERR_NOMEM = -4,
  SDM_ERR_NODEVICE = -5,  /* no gfx950 GPU visible: the product never falls back to the CPU */
  SDM_ERR_ARENA = -6      /* internal: the launch pass allocated activation memory differently from the pass that sized the arena (the result is
                             still correct: the diverging allocations were served outside the arena) */
};

enum sdm_ptr_kind { SDM_PTR_HOST = 0, SDM_PTR_DEVICE = 1 };
enum sdm_dtype { SDM_F32 = 0, SDM_F16 = 1, SDM_BF16 = 2 };

/* Architecture constants.  The reference reads them from stable-diffusion-2-1-base/{unet,vae}/config.json
 * (sdmatte_nodes.py:20-31, meta_arch.py:95-118) plus in-code defaults (meta_arch.py:107-112). */
typedef struct sdm_config {
  int32_t vae_channels[4];
  int32_t vae_layers_per_block;
  int32_t unet_channels[4];
  int32_t unet_heads[4];
  int32_t unet_layers_per_block;
  int32_t cross_attention_dim;
  int32_t unet_in_channels;
  int32_t unet_out_channels;
  int32_t bbox_embeddings_input_dim;
  int32_t groups;
  float vae_eps;
  float unet_res_eps;
  float unet_tf_gn_eps;
  float unet_ln_eps;
  float vae_scaling_factor;
  float attn_mask_value;
  int32_t stream_f32;      /* 1: residual stream tensors kept in fp32 (default), 0: fp16 */
  int32_t point_embeddings_input_dim;   /* 1680 (meta_arch.py:107-108); 0 = default */
  /* Arithmetic precision of the MFMA contractions, one bit per stage (enum sdm_precise_stage).  0 = fp16 operands everywhere
   * (fast: alpha within ~4e-3 of the fp32 reference path, the rounding floor of ANY fp16-operand evaluation).  A set bit evaluates
   * that stage with split operands (x = hi + lo with hi = fp16(x): 22 significant bits; hi.hi + lo.w + x.lo_w in fp32 accumulators)
   * and keeps every activation in fp32 between kernels: SDM_PRECISE_ALL reproduces the reference's fp32 CPU path to ~1.2e-4 (1e-3
   * is the parity bar, sdmatte_nodes.py:355-360) at roughly 2x the matrix-pipe time.  The residual terms (2^-11 of a product) run
   * on fp8 e4m3 operands in the wide 3x3 convs and the K >= 1024 GEMMs, on fp16 elsewhere; in the attention cores Q.K^T is split,
   * P.V is plain fp16. */
  int32_t precise_mask;
  int32_t reserved[5];
} sdm_config;

enum sdm_precise_stage {
  SDM_PRECISE_VAE_ENC = 1,        /* VAE encoder convs + quant_conv */
  SDM_PRECISE_VAE_DEC = 2,        /* post_quant_conv + VAE decoder convs */
  SDM_PRECISE_VAE_ATTN_LIN = 4,   /* q|k|v / to_out linears of the two VAE mid-block attentions */
  SDM_PRECISE_UNET_RES = 8,       /* U-Net conv_in/out, ResBlock convs, shortcuts, down/up-samplers */
  SDM_PRECISE_UNET_TF = 16,       /* U-Net transformer linears (proj_in/out, q|k|v, to_out, GEGLU, folded cross K|V) */
  SDM_PRECISE_UNET_ATTN = 32,     /* U-Net attention cores (QK^T, softmax, PV; head dim 64) */
  SDM_PRECISE_ALL = 63            /* (the single-head d=512 VAE attention core always runs on fp16 operands) */
};

/* Fill `cfg` with the SD-2.1-base / SDMatte constants and precise_mask = SDM_PRECISE_ALL (the precision that
 * meets the parity bar; set it to 0 for the fast fp16-operand graph). */
void sdm_default_config(sdm_config* cfg);

/* Create an engine on GPU `device_id`.  Replaces SDMatte.__init__ / init_submodule (meta_arch.py:31-124)
 * + `.to(device)` (sdmatte_nodes.py:323).  cfg == NULL selects sdm_default_config. */
int sdm_create(sdm_ctx** out, int device_id, const sdm_config* cfg);
void sdm_destroy(sdm_ctx* ctx);
const char* sdm_last_error(sdm_ctx* ctx);   /* ctx may be NULL: returns the last create() error */

/* Weight loading.  Replaces the safetensors read loop + load_state_dict(strict=False)
 * (sdmatte_nodes.py:300-321): call once per checkpoint tensor with its key (e.g.
 * "unet.down_blocks.0.resnets.0.conv1.weight"), dtype, shape and a HOST pointer (e.g. into the
 * safetensors mmap).  Unknown keys (text_encoder.*, point_embedding.*) are ignored and reported through
 * sdm_weight_stats; a shape mismatch is an error, as in torch.  Returns 1 if the key was consumed. */
int sdm_load_tensor(sdm_ctx* ctx, const char* name, int dtype, int ndim, const int64_t* shape, const void* host_ptr);
/* After the last tensor: folds constants and marks the engine ready.  n_missing = expected keys never
 * supplied (they stay zero-initialised; the reference would keep its random init). */
int sdm_finalize_weights(sdm_ctx* ctx);
int sdm_weight_stats(sdm_ctx* ctx, int64_t* n_loaded, int64_t* n_missing, int64_t* n_ignored);
/* Name of the i-th expected-but-missing key, or NULL. */
const char* sdm_missing_key(sdm_ctx* ctx, int64_t i);

/* Packed fp16 weight blob (for RCCL broadcast between ranks): size, and copy out/in to/from a
 * DEVICE buffer of that size.  Import marks every key as loaded; sdm_finalize_weights must follow. */
int64_t sdm_weight_blob_bytes(sdm_ctx* ctx);
int sdm_export_weight_blob(sdm_ctx* ctx, void* device_dst);
int sdm_import_weight_blob(sdm_ctx* ctx, const void* device_src);
/* Small host-side tensors needed for the time/bbox embedding constants (kept outside the blob). */
int64_t sdm_host_blob_bytes(sdm_ctx* ctx);
int sdm_export_host_blob(sdm_ctx* ctx, void* host_dst);
int sdm_import_host_blob(sdm_ctx* ctx, const void* host_src);

/* Model forward.  Replaces SDMatte.forward(data) (meta_arch.py:127-261):
 *   image  fp32 [B,3,S,S]  = data["image"]   (already resized + normalised to [-1,1])
 *   trimap fp32 [B,1,S,S]  = data["trimap"]  (in [-1,1])
 *   is_trans int32 [B]     = data["is_trans"];  coords fp32 [B,4] = data["trimap_coords"] (NULL -> [0,0,1,1])
 *   alpha  fp32 [B,1,S,S]  = return value in [0,1]
 * is_trans / coords are always HOST pointers (tiny).
 * Stream contract (all sdm_forward* / sdm_apply_matte): kernels run on a stream owned by the engine.  With SDM_PTR_DEVICE,
 * `stream` is the hipStream_t on which the caller produced the inputs and will consume the outputs - in PyTorch,
 * torch.cuda.current_stream().cuda_stream; NULL = the device's default stream.  The engine orders its work after everything
 * queued on that stream at call time (event wait, no host sync) and makes that stream wait for the outputs, so the call
 * behaves like any other kernel launch on `stream`.  With SDM_PTR_HOST the call copies in, runs, copies out and returns after
 * a host synchronisation; `stream` is ignored. */
int sdm_forward(sdm_ctx* ctx, const float* image_b3ss, const float* trimap_b1ss, int B, int S, const int32_t* is_trans,
                const float* coords_b4, float* alpha_b1ss, int ptr_kind, void* stream);

/* The other prompt types of the reference core (meta_arch.py:22-28,131-206): `aux` is data[aux_input]
 * ("trimap", "bbox_mask", "mask", "auto_mask" or "point_mask": [B,1,S,S] in [-1,1], encoded and used exactly like the trimap),
 * `cond` the matching coordinates: SDM_COND_BOX = data["*_coords"] [B,4] -> bbox_embedding (NULL -> [0,0,1,1], which is also
 * what use_coor_input=False feeds); SDM_COND_POINTS = data["point_coords"] [B,cond_dim] -> zero-padded to the first divisor of
 * point_embeddings_input_dim, sinusoid-embedded and sent through point_embedding (pass zeros for use_coor_input=False).
 * use_attention_mask = 0 runs the self-attention without the aux key mask (aux_input not in attn_mask_aux_input).
 * sdm_forward(...) == sdm_forward_ex(..., coords, 4, SDM_COND_BOX, 1, ...). */
enum sdm_cond_kind { SDM_COND_BOX = 0, SDM_COND_POINTS = 1 };
int sdm_forward_ex(sdm_ctx* ctx, const float* image_b3ss, const float* aux_b1ss, int B, int S, const int32_t* is_trans,
                   const float* cond, int cond_dim, int cond_kind, int use_attention_mask, float* alpha_b1ss, int ptr_kind, void* stream);

/* Rectangular inference (beyond the reference, whose attention-mask code asserts square latents,
 * replace.py:57-60): same as sdm_forward_ex with image [B,3,SH,SW], aux [B,1,SH,SW], alpha [B,1,SH,SW]; SH and SW multiples
 * of 64.  The level-k key bias keeps the reference's stride-2^k pick, bias_k[i,j] = bias_0[2^k i, 2^k j]. */
int sdm_forward_rect(sdm_ctx* ctx, const float* image_b3hw, const float* aux_b1hw, int B, int SH, int SW, const int32_t* is_trans,
                     const float* cond, int cond_dim, int cond_kind, int use_attention_mask, float* alpha_b1hw, int ptr_kind, void* stream);

/* Node-level call.  Replaces the device part of SDMatteApply.apply_matte (sdmatte_nodes.py:339-363):
 *   image fp32 [B,H,W,3] in [0,1], trimap fp32 [B,H,W] in [0,1]  ->  antialiased resize to SxS, normalise,
 *   forward, resize back to (H,W), clamp(0,1)  ->  alpha fp32 [B,H,W].
 * (alpha only; sdm_apply_matte_node below adds mask_refine and the output composition on the GPU.) */
int sdm_apply_matte(sdm_ctx* ctx, const float* image_bhwc, const float* trimap_bhw, int B, int H, int W, int S,
                    int is_transparent, float* alpha_bhw, int ptr_kind, void* stream);

/* The whole node in one call: sdm_apply_matte followed, at the original resolution and on the GPU, by
 * mask_refine (trimap_constraint; sdmatte_nodes.py:365-380) and the output composition (sdmatte_nodes.py:382-397):
 * output_mode 0 = alpha_only (matted = zeros [B,H,W,3]), 1 = matted_rgba ([B,H,W,4] = image | alpha), 2 = matted_rgb
 * ([B,H,W,3] = image gated by (trimap > 0.2) & (alpha > 0.1)).  Bit-identical to the reference's CPU tensor arithmetic. */
/* The trimap [B,trimap_h,trimap_w] is resized to SxS on its own, as in the reference (sdmatte_nodes.py:212-214,349): it only has to
 * match the image where the reference indexes the alpha with it, i.e. with mask_refine != 0 or output_mode 2 (SDM_ERR_INVALID otherwise).
 * trimap_constraint is a double: the thresholds are float32(c) and float32(1.0 - c) with 1.0 - c evaluated in double, as torch does
 * for the reference's Python-float comparisons. */
int sdm_apply_matte_node(sdm_ctx* ctx, const float* image_bhwc, const float* trimap_bhw, int B, int H, int W, int trimap_h, int trimap_w, int S,
                         int is_transparent, int output_mode, int mask_refine, double trimap_constraint, float* alpha_bhw, float* matted_bhwc,
                         int ptr_kind, void* stream);

/* Trimap from a mask, on the GPU (beyond the reference, whose README leaves "Create Trimap" to other nodes): mask fp32 [B,H,W] ->
 * trimap fp32 [B,H,W] with F = { p : mask[p] > threshold } (one fp32 compare, so NaN is background) and
 *   1.0 where p is in F and no pixel of the image outside F lies within Euclidean distance erode_px of p (dx^2 + dy^2 <= erode_px^2),
 *   0.0 where p is not in F and no pixel of F lies within distance dilate_px of p,
 *   0.5 elsewhere.
 * Pixels beyond the image border do not exist (neither foreground nor background): an object cut by the frame keeps its definite foreground up
 * to the edge.  Radii 0 give the binarised mask.  Integer arithmetic and compares only: the values are exactly 0.0 / 0.5 / 1.0.
 * Radii in 0 .. SDM_TRIMAP_MAX_RADIUS, any H, W >= 1 (SDM_ERR_INVALID otherwise).  Stream contract and pointer kinds as sdm_forward.  Needs no
 * weights: it works on a context that never loaded any.  Its scratch memory is part of the activation arena / I/O staging
 * (sdm_resident_bytes counts it, sdm_release_memory frees it). */
#define SDM_TRIMAP_MAX_RADIUS 255
int sdm_make_trimap(sdm_ctx* ctx, const float* mask_bhw, int B, int H, int W, float threshold, int erode_px, int dilate_px,
                    float* trimap_bhw, int ptr_kind, void* stream);
/* Mask clean-up on the GPU, in front of sdm_make_trimap (beyond the reference): masks from a segmenter carry stray islands, pin-holes and second
 * objects, and the trimap turns each of them into definite foreground or background.  mask fp32 [B,H,W] -> out fp32 [B,H,W].
 *   F        = { p : mask[p] > threshold } (one fp32 compare, so NaN is background).  Images of a batch are independent; rows do not wrap.
 *   stage A  label F with 8-connectivity; a component's area is its pixel count.  With keep_largest = 1 only the component of largest area survives
 *            (on a tie the one that contains the smallest pixel index y*W + x); a survivor must also have area >= min_area (0 and 1 remove nothing).
 *            The survivors form F1.
 *   stage B  label the complement of F1 with 4-connectivity.  A hole is a component without a pixel of the image border (row 0, row H-1, column 0,
 *            column W-1); holes with area <= max_hole_area join the foreground: F2.  max_hole_area = 0 fills nothing.
 *   The stages are sequential: holes are holes of the mask after island removal, so a removed island inside a hole enlarges that hole before its area
 *   is compared.
 *   out[p]   = mask[p] where the class of p did not change (1.0 / 0.0 everywhere when binarize != 0), 0.0 for a removed pixel, 1.0 for a filled one:
 *            out > threshold is exactly F2, and a soft mask stays soft where it was right.
 *   stats_b4 (may be NULL) int32 [B][SDM_CLEAN_STATS], of the same pointer kind as the planes: per image {components of F, components removed,
 *            holes filled, pixels whose class changed}.
 * threshold finite in [0, 1) (so that the written 0.0 and 1.0 lie on the right side of it), min_area and max_hole_area in 0 .. SDM_FG_MAX_PIXELS,
 * keep_largest and binarize 0 or 1, B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS (global pixel indices are the labels): SDM_ERR_INVALID
 * otherwise, and then nothing is queued or written.  Compares and counts only: GPU, emulator and sdmatte_nodes.clean_mask agree bit for bit.
 * Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the launches.  Needs no weights.  The number of kernel launches
 * depends only on which stages are on (stage A: min_area > 1 or keep_largest, 6 launches; stage B: max_hole_area > 0, 4 launches; stage A off: 1
 * threshold / copy launch, plus 3 for the component count when stats_b4 is given), never on B, H, W or the content (csrc/k_cclabel.h); no host
 * readback.  The three label planes (12 bytes per pixel) are part of the activation arena, host pointers go through the I/O staging
 * (sdm_resident_bytes counts both, sdm_release_memory frees them). */
#define SDM_CLEAN_STATS 4
int sdm_clean_mask(sdm_ctx* ctx, const float* mask_bhw, int B, int H, int W, float threshold, int min_area, int keep_largest, int max_hole_area,
                   int binarize, float* out_bhw, int32_t* stats_b4, int ptr_kind, void* stream);
/* sdm_apply_matte_node with the trimap made from `mask` [B,mask_h,mask_w] on the device, in the same call: bit-identical, in alpha,
 * matted and trimap, to sdm_make_trimap followed by sdm_apply_matte_node.  The size rule is that call's, with the mask in the trimap's place.
 * trimap_out (may be NULL) receives the trimap [B,mask_h,mask_w]. */
int sdm_apply_matte_mask(sdm_ctx* ctx, const float* image_bhwc, const float* mask_bhw, int B, int H, int W, int mask_h, int mask_w, int S,
                         int is_transparent, float threshold, int erode_px, int dilate_px, int output_mode, int mask_refine,
                         double trimap_constraint, float* alpha_bhw, float* matted_bhwc, float* trimap_out, int ptr_kind, void* stream);

/* The subject's box, on the GPU (beyond the reference, which shows the model the whole frame at `inference_size`: a subject that fills a quarter of a 4K
 * photo reaches the model at 256 pixels).  plane fp32 [B,H,W] -> roi_b4 int32 [B][4] = {y0, x0, h, w}, of the same pointer kind as the plane.
 *   U        = { p : plane[p] > roi_threshold } (one fp32 compare, so NaN is outside U); [ymin, ymax] x [xmin, xmax] is its bounding box, per image.
 *   margin   bh = ymax - ymin + 1, my = margin_px + (bh * margin_pct) / 100 (integer division); y0 = max(0, ymin - my), y1 = min(H, ymax + 1 + my),
 *            h = y1 - y0; x0 and w likewise from bw and W.
 *   square   (square != 0) L = max(h, w); per axis, shown for y: y0 = y0 - (L - h) / 2, then y0 = 0 if y0 < 0, then y0 = max(0, H - L) if y0 + L > H,
 *            and h = min(L, H): the shorter axis grows around its middle, is shifted back into the frame, and ends at the frame where that is shorter.
 *   An empty U gives the whole frame {0, 0, H, W}, square or not.
 * Integer arithmetic only: GPU, emulator and sdmatte_nodes.subject_roi agree exactly.  roi_threshold finite in [0, 1), margin_px in
 * 0 .. SDM_ROI_MAX_MARGIN_PX, margin_pct in 0 .. 100, square 0 or 1, B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS: SDM_ERR_INVALID
 * otherwise, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the launches.
 * Needs no weights.  Three kernel launches (initialise, reduce, finalise; csrc/k_roi.h), whatever B, H, W and the content: one read of the plane, no host
 * readback.  The raw extrema are part of the activation arena, host pointers go through the I/O staging (sdm_resident_bytes counts both,
 * sdm_release_memory frees them). */
#define SDM_ROI_MAX_MARGIN_PX 4096
int sdm_subject_roi(sdm_ctx* ctx, const float* plane_bhw, int B, int H, int W, float roi_threshold, int margin_px, int margin_pct, int square,
                    int32_t* roi_b4, int ptr_kind, void* stream);
/* sdm_apply_matte_node on the subject instead of the frame: the box of the trimap (sdm_subject_roi with the four box arguments) is resized to SxS in the
 * frame's place, and the model's alpha is resized back into the box; outside the box the alpha is 0.0, which is exact, not an approximation: every
 * pixel there has trimap <= roi_threshold.  mask_refine and the output composition then run over the whole frame as in sdm_apply_matte_node.
 * Bit-identical to: box on the host, sdm_apply_matte_node (alpha_only, no refine) on the cropped image and trimap, the alpha pasted into zeros,
 * and the node's tail on the frame.  The box never leaves the device: no host readback, a fixed number of launches, and the model's input is SxS
 * whatever the box is.  One box per image; the model still sees one image with global attention, and its box conditioning stays [0, 0, 1, 1].
 *   aux      [B,H,W], the image's size (there is no size of its own here): the trimap (aux_is_mask = 0), or a mask (aux_is_mask = 1) that becomes the
 *            trimap on the whole frame first, exactly as in sdm_apply_matte_mask (threshold, erode_px, dilate_px: read with aux_is_mask = 1 only).
 *   trimap_out (may be NULL) receives that trimap; passing it with aux_is_mask = 0 is SDM_ERR_INVALID.
 *   roi_out  (may be NULL) int32 [B][4] = {y0, x0, h, w}, of the same pointer kind as the other arguments.
 * An empty U makes the call equal to sdm_apply_matte_node / sdm_apply_matte_mask.  Argument limits as sdm_subject_roi and sdm_apply_matte_mask.  The
 * box and its scratch are part of the activation arena.  Six launches beyond the model's, each once per call: roi_init, roi_reduce, roi_finalize,
 * roi_prep_image, roi_prep_trimap, roi_paste in sdm_kernel_counts and the per-launch profile. */
int sdm_apply_matte_roi(sdm_ctx* ctx, const float* image_bhwc, const float* aux_bhw, int B, int H, int W, int S, int is_transparent, int aux_is_mask,
                        float threshold, int erode_px, int dilate_px, float roi_threshold, int margin_px, int margin_pct, int square,
                        int output_mode, int mask_refine, double trimap_constraint, float* alpha_bhw, float* matted_bhwc, float* trimap_out,
                        int32_t* roi_out, int ptr_kind, void* stream);

/* A box per subject, on the GPU (beyond the reference): two people at opposite ends of a group shot have a joint box that is nearly the frame, so
 * sdm_subject_roi gives each of them a fraction of `inference_size`.  plane fp32 [B,H,W] -> boxes_bk5 int32 [B][max_boxes][5] = {b, y0, x0, h, w} and
 * count_b (may be NULL) int32 [B], both of the same pointer kind as the plane.  Per image:
 *   U, components  U = { p : plane[p] > roi_threshold } (one fp32 compare, so NaN is outside U); its components are 8-connected, a component's area is
 *            its pixel count and its root its smallest pixel index y*W + x (stage A of sdm_clean_mask with roi_threshold as the threshold).
 *   rank     the candidates are the components with area >= min_area, ordered by area descending, then root ascending; the own components
 *            C_1 .. C_m are the first m = min(max_boxes - 1, number of candidates).
 *   box(X)   for a pixel set X: the rule of sdm_subject_roi (margin, clip, optional square) applied to X's extrema.
 *   containment  in rank order, C_i is kept unless its raw bounding box [ymin, ymax] x [xmin, xmax] lies inside box(C_j) of a kept C_j, j < i: a hand
 *            or a strand of hair that the mask separated from its owner gets no pass of its own.  The kept boxes, in rank order, are entries
 *            0 .. n_own-1.
 *   rest     R = the pixels of U in none of the kept boxes; if R is not empty, entry n_own is box(R): candidates beyond the own ones and components
 *            below min_area are never lost.
 *   An empty U gives one entry, the whole frame {b, 0, 0, H, W}.  count_b[b] is the number of entries, in 1 .. max_boxes; every further entry is void:
 *   {-1, 0, 0, 0, 0}.
 * Hence every pixel of U lies in at least one box, and with max_boxes = 1 the single entry is sdm_subject_roi's box for the same arguments.
 * Integer arithmetic only: GPU, emulator and sdmatte_nodes.subject_boxes agree exactly.  roi_threshold, margin_px, margin_pct, square, B, H, W as in
 * sdm_subject_roi, min_area in 0 .. SDM_FG_MAX_PIXELS, max_boxes in 1 .. SDM_BOXES_MAX: SDM_ERR_INVALID otherwise, and then nothing is queued or
 * written.  Stream contract and pointer kinds as sdm_subject_roi; sdm_last_forward_ms covers the launches.  Needs no weights.  8 + 2 (max_boxes - 1)
 * kernel launches (csrc/k_boxes.h: cc_tile, cc_seam, cc_flatten, boxes_init, boxes_rank x 2 per own slot, boxes_reduce, boxes_own, boxes_rest,
 * boxes_finalize), whatever B, H, W and the content; no host readback.  The three label planes (12 bytes per pixel) and the per-image state are part of
 * the activation arena, host pointers go through the I/O staging (sdm_resident_bytes counts both, sdm_release_memory frees them). */
#define SDM_BOXES_MAX 8
int sdm_subject_boxes(sdm_ctx* ctx, const float* plane_bhw, int B, int H, int W, float roi_threshold, int min_area, int max_boxes, int margin_px,
                      int margin_pct, int square, int32_t* boxes_bk5, int32_t* count_b, int ptr_kind, void* stream);
/* sdm_apply_matte_node over a list of boxes: the model runs with batch N, slot n on the box of entry n = {b, y0, x0, h, w} of boxes_n5 (int32 [N][5], of
 * the same pointer kind as the planes; N in 1 .. SDM_BOXES_MAX_TOTAL is known to the host, the list's content stays on the device), and the alphas go
 * back into the frames.  The trimap [B,H,W] has the image's size.
 *   sanitise an entry is valid iff 0 <= b < B, h >= 1, w >= 1, y0 >= 0, x0 >= 0, y0 + h <= H and x0 + w <= W (compared in 64 bits); every other entry is
 *            void, the void entries of sdm_subject_boxes among them.  The same rule for host and device pointers; a void entry is not an error, and no
 *            kernel of this call reads outside the planes whatever the list holds.
 *   prepare  slot n is fed the box of image b and of its trimap, resized to SxS as in sdm_apply_matte_roi.  A void slot is fed the whole frame of image 0
 *            and its result is discarded: it costs a model pass, so a caller who wants to avoid that compacts the list first.
 *   paste    alpha[b][p] = the maximum, over the valid entries of image b whose box contains p, of the clamped resize of that slot's alpha
 *            (sdm_apply_matte_roi's arithmetic); 0.0 if there is none.  A pixel in exactly one box gets that box's value unchanged; where boxes overlap,
 *            the maximum is the order-independent choice that never lets one box's edge cut into a neighbour.
 *   mask_refine and the output composition then run over the whole frame as in sdm_apply_matte_node.  The box conditioning stays [0, 0, 1, 1] and
 *   is_transparent is one flag.
 * "Outside every box = 0.0" is exact for a list from sdm_subject_boxes on the same trimap and threshold (every such pixel has trimap <= roi_threshold);
 * for a caller's own list it is the caller's statement.  With the list {b, roi[b]} of sdm_subject_roi the call is bit-identical to sdm_apply_matte_roi
 * (aux_is_mask = 0).  The model's kernels are chosen by launch size, so a slot's bits may depend on N.
 * N outside its range, a bad output_mode, S or plane size: SDM_ERR_INVALID, and then nothing is queued or written.  The arena is that of a
 * sdm_apply_matte_node call with batch N, plus the list.  Four launches beyond the model's, each once per call: boxes_sanitize, boxes_prep_image,
 * boxes_prep_trimap, boxes_paste in sdm_kernel_counts and the per-launch profile. */
#define SDM_BOXES_MAX_TOTAL 16
int sdm_apply_matte_boxes(sdm_ctx* ctx, const float* image_bhwc, const float* trimap_bhw, int B, int H, int W, int S, int is_transparent,
                          const int32_t* boxes_n5, int N, int output_mode, int mask_refine, double trimap_constraint, float* alpha_bhw,
                          float* matted_bhwc, int ptr_kind, void* stream);

/* Which tiles of a frame need the model, on the GPU (beyond the reference): a portrait that fills a 4K frame has the frame as its box, so the box calls
 * above still show the model its hair at a quarter of the resolution.  The frame is cut into overlapping tiles of `tile` pixels, and only the tiles that
 * hold a pixel of the trimap's unknown band are listed.  trimap fp32 [B,H,W] -> tiles_bk5 int32 [B][max_tiles][5] = {b, y0, x0, h, w} and count_b (may be
 * NULL) int32 [B], both of the same pointer kind as the plane.  Per image:
 *   band     pixel p is unknown iff band_lo < trimap[p] and trimap[p] < band_hi (two fp32 compares, so NaN is not in the band, nor is a value equal to
 *            either bound).  0.25 and 0.75 are the band of sdm_matte_metrics.
 *   grid     per axis of length L, with T = tile and O = overlap, in integers (64-bit products, truncating division): one tile of size L at 0 if L <= T;
 *            otherwise n = ceil((L - O) / (T - O)) tiles of size T at the origins o_i = (i * (L - T)) / (n - 1), i = 0 .. n-1.  The origins increase
 *            strictly, the first tile starts at 0 and the last ends at L, neighbours overlap by at least O, every pixel is covered - by at most three
 *            tiles per axis (three, not two: up to nine tiles meet in a pixel).  A grid tile is the product of a y-interval and an x-interval.
 *   active   a grid tile is active iff its rectangle holds at least one band pixel.  Hence every band pixel lies in every active tile that contains it,
 *            and in at least one.
 *   list     the active tiles in row-major grid order (iy, then ix) are entries 0, 1, ..; every further entry is void: {-1, 0, 0, 0, 0}.  count_b[b] is
 *            the number of active tiles, also when it exceeds max_tiles: then the first max_tiles are listed and the caller sees the overflow.  An image
 *            without a band pixel has count 0 and void entries only.
 * Integer and bitwise operations only: GPU, emulator and sdmatte_nodes.band_tiles agree exactly.  band_lo and band_hi finite with 0 <= band_lo < band_hi
 * <= 1, tile in 16 .. SDM_FG_MAX_SIDE, overlap in 0 .. tile / 2, max_tiles in 1 .. SDM_TILES_MAX, n_y * n_x <= SDM_TILES_MAX_GRID grid cells per image,
 * B, H, W as in sdm_subject_roi: SDM_ERR_INVALID otherwise, and then nothing is queued or written.  Stream contract and pointer kinds as
 * sdm_make_trimap; sdm_last_forward_ms covers the launches.  Needs no weights.  Three kernel launches (csrc/k_tiles.h: tiles_init, tiles_mark,
 * tiles_list), whatever B, H, W and the content: one read of the plane, no global atomic per pixel (at most SDM_TILES_MAX_GRID / 32 per block), no host
 * readback.  The flag words are part of the activation arena, host pointers go through the I/O staging (sdm_resident_bytes counts both,
 * sdm_release_memory frees them). */
#define SDM_TILES_MAX 16 /* = SDM_BOXES_MAX_TOTAL */
#define SDM_TILES_MAX_GRID 256
int sdm_band_tiles(sdm_ctx* ctx, const float* trimap_bhw, int B, int H, int W, float band_lo, float band_hi, int tile, int overlap, int max_tiles,
                   int32_t* tiles_bk5, int32_t* count_b, int ptr_kind, void* stream);
/* sdm_apply_matte_node over a list of tiles that cut through one subject: the model runs with batch N, slot n on the tile of entry n = {b, y0, x0, h, w}
 * of tiles_n5 (int32 [N][5], of the same pointer kind as the planes; N in 0 .. SDM_TILES_MAX is known to the host, the list's content stays on the
 * device), and the alphas are blended into the frames.  The trimap [B,H,W] has the image's size.
 *   sanitise, prepare  exactly as in sdm_apply_matte_boxes (the same kernels under the same names): an entry that does not lie inside the planes is void, a
 *            void entry is not an error and costs a model pass, and no kernel of this call reads outside the planes whatever the list holds.
 *   blend    each frame pixel is written once.  For image b and pixel p, over the valid entries i of image b whose rectangle contains p, in list order:
 *            a_i   = the clamped value of that slot at p as in sdm_apply_matte_roi: the plain copy when (h, w) == (S, S), else the resize from S x S;
 *            w_i   = wy * wx.  Per axis, a side of the tile that lies on the frame's border does not ramp; any other side ramps as
 *                    min(1, (d + 1) / (feather_px + 1)), d being the distance in pixels to that side's edge pixel (0 on it), a true fp32 division; the
 *                    axis weight is the minimum of its two sides (1 if both lie on the border).  feather_px = 0 gives weight 1 everywhere;
 *            Wsum  = the sum of the w_i in list order;
 *            out   = clamp(sum of (w_i / Wsum) * a_i in list order, 0, 1), true fp32 divisions.
 *            Hence a pixel inside exactly one tile gets that tile's value unchanged, bit for bit (w / w == 1), and with one tile equal to the frame the
 *            call is bit-identical to sdm_apply_matte_node.  The weights are normalised before the multiply, so that a constant slot value stays
 *            that constant.
 *   base     a pixel in no valid tile gets base_bhw[b][p] (NaN -> 0, then clamped to [0, 1]) if base_bhw (fp32 [B,H,W], may be NULL) is given, otherwise
 *            1.0 if trimap[p] > 0.5, else 0.0.  For a list from sdm_band_tiles on the same trimap every such pixel is definite, so this is exact; for
 *            a caller's own list it is the caller's statement.
 *   mask_refine and the output composition then run over the whole frame as in sdm_apply_matte_node.  The box conditioning stays [0, 0, 1, 1] and
 *   is_transparent is one flag.
 * N = 0 (tiles_n5 may be NULL then) runs no preparation and no model pass: the blend gives every pixel the base, and the tail follows.
 * N or feather_px (0 .. SDM_TILES_MAX_FEATHER) outside its range, a bad output_mode, S or plane size: SDM_ERR_INVALID, and then nothing is queued or
 * written.  The arena is that of sdm_apply_matte_boxes.  Four launches beyond the model's, each once per call: boxes_sanitize, boxes_prep_image,
 * boxes_prep_trimap, tiles_blend in sdm_kernel_counts and the per-launch profile (tiles_blend alone with N = 0). */
#define SDM_TILES_MAX_FEATHER 1024
int sdm_apply_matte_tiles(sdm_ctx* ctx, const float* image_bhwc, const float* trimap_bhw, int B, int H, int W, int S, int is_transparent,
                          const int32_t* tiles_n5, int N, int feather_px, const float* base_bhw, int output_mode, int mask_refine,
                          double trimap_constraint, float* alpha_bhw, float* matted_bhwc, int ptr_kind, void* stream);

/* Foreground / background colours from an image and its alpha, on the GPU (beyond the reference: its matted_rgba keeps the composite
 * a*F + (1-a)*B in every semi-transparent pixel, and with it a halo of the old background).  A multi-level estimator in the style of Germer et al.,
 * "Fast Multi-Level Foreground Estimation"; it uses the image and the alpha only.
 *   image fp32 [B,H,W,3] (values used as they are), alpha fp32 [B,H,W] (NaN -> 0, then clamped to [0,1])
 *   fg fp32 [B,H,W,fg_channels], fg_channels 3 or 4: with 4, channel 3 is the sanitised alpha (a straight-alpha RGBA cut-out)
 *   bg fp32 [B,H,W,3], may be NULL.  Colours are clamped to [0,1].
 * Levels (h,w) = (H,W), (ceil(h/2), ceil(w/2)), ... down to (1,1), processed from (1,1) upwards; a level with max(h,w) <= 32 runs n_small_iters
 * Jacobi steps, every other level n_big_iters.  Nearest resampling src = min(Ns-1, (i*Ns)/Nd): a level's image I and alpha a0 come from the
 * full-resolution inputs, F and B from the previous level (F = B = I at (1,1)).  Per pixel p, with neighbours q = left, right, up, down clamped
 * to the level: w_q = regularization + gradient_weight * |a0[p] - a0[q]|, s = sum w_q, a1 = 1 - a0, D = a0^2 + a1^2 + s, and per step and channel
 *   Fm = (sum w_q F[q]) / s, Bm = (sum w_q B[q]) / s, r = (I - a0 Fm - a1 Bm) / D, F' = clamp(Fm + a0 r, 0, 1), B' = clamp(Bm + a1 r, 0, 1).
 * Every step reads the previous step only, so an image's result does not depend on the batch it is in.  sdmatte_nodes.estimate_foreground is the
 * same function on CPU tensors (equal to fp32 rounding, not bit for bit).
 * regularization > 0, gradient_weight >= 0 (both finite), n_small_iters in 1 .. SDM_FG_MAX_SMALL_ITERS, n_big_iters in 1 .. SDM_FG_MAX_BIG_ITERS,
 * H and W in 1 .. SDM_FG_MAX_SIDE (the resampling products i*Ns are 32-bit) and B*H*W <= SDM_FG_MAX_PIXELS (pixel counts are 32-bit; byte offsets
 * are 64-bit): SDM_ERR_INVALID otherwise.  Stream contract and pointer kinds as sdm_make_trimap.  Needs no weights.  The level planes are part of
 * the activation arena, host pointers go through the I/O staging (sdm_resident_bytes counts both, sdm_release_memory frees them). */
#define SDM_FG_REGULARIZATION 1e-5f
#define SDM_FG_GRADIENT_WEIGHT 1.0f
#define SDM_FG_SMALL_ITERS 10
#define SDM_FG_BIG_ITERS 2
#define SDM_FG_MAX_SMALL_ITERS 64
#define SDM_FG_MAX_BIG_ITERS 4
#define SDM_FG_MAX_SIDE 32768
#define SDM_FG_MAX_PIXELS 268435456 /* 2^28 */
int sdm_estimate_foreground(sdm_ctx* ctx, const float* image_bhwc, const float* alpha_bhw, int B, int H, int W, float regularization,
                            float gradient_weight, int n_small_iters, int n_big_iters, float* fg_bhwc, int fg_channels, float* bg_bhwc,
                            int ptr_kind, void* stream);

/* Alpha refinement at the caller's resolution, on the GPU (beyond the reference, whose alpha is the model's alpha at `inference_size` brought back
 * with a bilinear resize: at 4K every edge is a ramp of several pixels).  The colour guided filter in its subsampled form (He, Sun, Tang, "Guided Image
 * Filtering"; He, Sun, "Fast Guided Filter"): fit alpha ~ a.I + b per window between the coarse alpha and the coarse image, apply the smoothed
 * coefficients to the full-resolution image.  Everything is fp32.
 *   image fp32 [B,H,W,3] (values used as they are), alpha fp32 [B,H,W] (p = alpha with NaN -> 0, then clamped to [0,1]), out fp32 [B,H,W] in [0,1]
 *   coarse    s = subsample, (h,w) = (ceil(H/s), ceil(W/s)); coarse pixel (i,j) of I' (3 channels) and p' is the mean over the existing pixels of block
 *             [i*s, min(H, i*s+s)) x [j*s, min(W, j*s+s)).  With s = 1 the coarse grid is the image.
 *   window    Win(i,j) = coarse pixels within Chebyshev distance `radius`, clipped to the grid; n = its pixel count; m(x) = (sum of x over Win) / n
 *   moments   mu = m(I'), mup = m(p'), c = m(I'*p') - mu*mup, Sigma = m(I' I'^T) - mu mu^T + eps*Id (symmetric: 6 distinct entries)
 *   solve     a = Sigma^-1 c by the closed-form adjugate of the symmetric 3x3, divided by the determinant; b = mup - a.mu
 *   smooth    abar = m(a), bbar = m(b)
 *   upsample  bilinear with half-pixel centres: u = clamp((y + 0.5)/s - 0.5, 0, h - 1), rows i0 = floor(u) and min(i0 + 1, h - 1) with weights
 *             1 - (u - i0) and u - i0, likewise in x (rows first, then columns)
 *   apply     out = clamp(abar^ . I + bbar^, 0, 1) at every full-resolution pixel
 * The window sums are direct sums in a fixed order and every division is a true fp32 division, so an image's result does not depend on the batch it is in.
 * The subsample is the point of the call: with s = 1 it is the classic filter on the already blurred alpha, which recovers almost nothing; with
 * s = ceil(max(H,W) / inference_size) the fit is made at the resolution the model saw.  sdmatte_nodes.guided_refine_alpha is the same function in torch
 * (equal to fp32 rounding, not bit for bit).
 * subsample in 1 .. SDM_GF_MAX_SUBSAMPLE, radius in 1 .. SDM_GF_MAX_RADIUS, eps finite in [1e-6, 1], H and W >= 1 and within SDM_FG_MAX_SIDE /
 * SDM_FG_MAX_PIXELS: SDM_ERR_INVALID otherwise.  Stream contract and pointer kinds as sdm_make_trimap.  Needs no weights.  Four kernel launches per call,
 * whatever B, H, W, subsample and radius (csrc/k_guided.h); with s > 1 exactly two of them touch full-resolution memory (16 bytes per pixel each).  The
 * three coarse planes are part of the activation arena, host pointers go through the I/O staging (sdm_resident_bytes counts both, sdm_release_memory
 * frees them). */
#define SDM_GF_RADIUS 2
#define SDM_GF_EPS 1e-4f
#define SDM_GF_MAX_SUBSAMPLE 16
#define SDM_GF_MAX_RADIUS 32
int sdm_refine_alpha_guided(sdm_ctx* ctx, const float* image_bhwc, const float* alpha_bhw, int B, int H, int W, int subsample, int radius, float eps,
                            float* out_bhw, int ptr_kind, void* stream);

/* The cut-out on a canvas, on the GPU (beyond the reference): the subject of a straight-alpha cut-out - found by its alpha - scaled to fill a share of a
 * canvas of a given size, centred or on a baseline, over transparency, a colour or an image, with an optional soft shadow.  Colours are resampled
 * premultiplied: resampling straight colours lets the invisible colour of alpha-0 pixels bleed into every soft edge.  Everything is fp32.
 *   fg fp32 [B,H,W,3] (values used as they are), alpha fp32 [B,H,W] (a = alpha with NaN -> 0, then clamped to [0,1]),
 *   out fp32 [B,canvas_h,canvas_w,out_channels], place_out (may be NULL) int32 [B][8], of the same pointer kind as the planes.
 *   box      {y0, x0, h, w} of sdm_subject_roi with the RAW alpha, roi_threshold, margin_px 0, margin_pct 0 and square 0 (one fp32 compare per pixel, so NaN is
 *            outside; an empty set gives the whole frame).
 *   fit      integers only, the products 64-bit, every division truncating: th = max(1, canvas_h*fill_pct/100), tw = max(1, canvas_w*fill_pct/100).
 *            If th*w <= tw*h: dh = th, dw = max(1, (w*th + h/2)/h); otherwise dw = tw, dh = max(1, (h*tw + w/2)/w).  dx0 = (canvas_w - dw)/2.  With
 *            mv = (canvas_h - th)/2: dy0 = mv for valign 0 (top), (canvas_h - dh)/2 for valign 1 (centre), canvas_h - mv - dh for valign 2 (bottom: the subject
 *            stands on the lower edge of the fill area).  The destination rectangle [dy0, dy0+dh) x [dx0, dx0+dw) lies inside the canvas.
 *            place_out[b] = {y0, x0, h, w, dy0, dx0, dh, dw}.  GPU, emulator and sdmatte_nodes.canvas_fit agree exactly.
 *   place    inside the destination rectangle the four planes (a*F.r, a*F.g, a*F.b, a) of the box are resampled from (h,w) to (dh,dw) with the antialiased
 *            bilinear filter of the node (torchvision Resize = interpolate(bilinear, align_corners=False, antialias=True); the plain copy when
 *            (dh,dw) == (h,w)).  Pixels outside the box do not exist: the result is that of crop, premultiply, resize.  Outside the rectangle the layer is 0.
 *            This is the premultiplied subject layer (P_s, A_s) on the canvas.
 *   shadow   skipped entirely when shadow_opacity == 0 (sigma and offsets are then not looked at).  r = ceil(3*shadow_sigma); w_i = exp(-i*i/(2*sigma*sigma))
 *            for i = -r .. r, divided by their sum: computed on the host in double from the fp32 sigma, rounded to fp32, at most
 *            2*SDM_CANVAS_MAX_SHADOW_RADIUS + 1 of them.  With A_s = 0 beyond the canvas,
 *              T(y,x) = sum over i = -r .. r (ascending) of w_i * A_s(y, x - shadow_dx + i)      (rows first; T of a row beyond the canvas is 0)
 *              S(y,x) = shadow_opacity * sum over j = -r .. r (ascending) of w_j * T(y - shadow_dy + j, x)
 *            i.e. S = shadow_opacity * (G * A_s)(y - shadow_dy, x - shadow_dx), the separable Gaussian with zero padding.  The colour is black.
 *   compose  "over" on premultiplied layers from bottom to top: the background (bg_mode 0: none; 1: the opaque colour bg_rgb3, 3 floats, ALWAYS a HOST
 *            pointer; 2: the opaque image bg_image [bg_batch,canvas_h,canvas_w,3] with bg_batch 1 or B, at canvas size), the shadow layer (0, S), the subject
 *            layer.  With C the background colour (0 without one) and S = 0 without a shadow: P = P_s + (1 - A_s) * ((1 - S) * C);
 *            A = 1 with a background, A_s + (1 - A_s) * S without one.
 *   out      out_channels 3: P (needs bg_mode 1 or 2).  out_channels 4: straight RGBA (P / A where A > 0, else 0; A).
 * Limits: B, H, W and roi_threshold as sdm_subject_roi; canvas sides in 1 .. SDM_FG_MAX_SIDE and B*canvas_h*canvas_w <= SDM_FG_MAX_PIXELS; fill_pct in 1 .. 100;
 * valign in 0 .. 2; bg_mode in 0 .. 2 (bg_rgb3 given with 1, bg_image given with 2), out_channels 4 with bg_mode 0; shadow_opacity finite in [0, 1];
 * shadow_sigma finite in (0, SDM_CANVAS_MAX_SHADOW_SIGMA] when the opacity is above 0; |shadow_dy| and |shadow_dx| at most SDM_CANVAS_MAX_SHADOW_OFFSET:
 * SDM_ERR_INVALID otherwise, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the
 * launches.  Needs no weights.  sdmatte_nodes.compose_canvas is the same function in torch (equal to fp32 rounding, not bit for bit).
 * The number of launches depends only on whether the shadow is on, never on B, the sizes or the content (csrc/k_canvas.h); no host readback.
 *   without a shadow 5: roi_init, roi_reduce, roi_finalize, canvas_fit, canvas_compose (the canvas is written once; no canvas-sized intermediate exists)
 *   with a shadow    7: roi_init, roi_reduce, roi_finalize, canvas_fit, canvas_place (the layer, 16 bytes per canvas pixel), canvas_blur_rows (T, 4 bytes per
 *                       canvas pixel), canvas_blur_compose (the column sums fused with the composition)
 * These are the names in sdm_kernel_counts and the per-launch profile.  The raw extrema, the box, the placements, the layer and T are part of the activation
 * arena, host pointers go through the I/O staging (sdm_resident_bytes counts both, sdm_release_memory frees them). */
#define SDM_CANVAS_MAX_SHADOW_SIGMA 32
#define SDM_CANVAS_MAX_SHADOW_RADIUS 96
#define SDM_CANVAS_MAX_SHADOW_OFFSET 4096
int sdm_compose_canvas(sdm_ctx* ctx, const float* fg_bhw3, const float* alpha_bhw, int B, int H, int W, float roi_threshold, int canvas_h, int canvas_w,
                       int fill_pct, int valign, int bg_mode, const float* bg_rgb3, const float* bg_image, int bg_batch, float shadow_opacity,
                       float shadow_sigma, int shadow_dy, int shadow_dx, float* out, int out_channels, int32_t* place_out, int ptr_kind, void* stream);

/* The exact Euclidean distance transform, on the GPU (beyond the reference): the primitive under "grow / shrink / feather a mask by any amount" and under
 * an outline around a cut-out; sdm_make_trimap's morphology is capped at SDM_TRIMAP_MAX_RADIUS and yields 0 / 0.5 / 1 only.
 * plane fp32 [B,H,W] -> field_bhw int32 [B,H,W], of the same pointer kind.
 *   F        = { p : plane[p] > threshold } (one fp32 compare, so NaN is outside F).  Images of a batch are independent; pixels beyond the border do not
 *            exist, as in sdm_make_trimap.
 *   d2(p)    the minimum of dy^2 + dx^2 over the pixels of the OTHER class (outside F for p in F, in F otherwise) of the same image; SDM_DF_NONE where
 *            that class is empty in the image.  No radius cap.
 *   field[p] = +d2(p) for p in F, -d2(p) otherwise.  Hence |field| >= 1 everywhere, and the largest real value, 2 * 32767^2, is below SDM_DF_NONE.
 * The trimap of sdm_make_trimap is 1.0 where field > erode_px^2, 0.0 where field < -dilate_px^2 and 0.5 elsewhere.
 * Integer arithmetic only: GPU, emulator and sdmatte_nodes.distance_field agree exactly.  threshold finite in [0, 1), B, H, W >= 1 within SDM_FG_MAX_SIDE /
 * SDM_FG_MAX_PIXELS: SDM_ERR_INVALID otherwise, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_subject_roi;
 * sdm_last_forward_ms covers the launches.  Needs no weights.  Four kernel launches (csrc/k_distance.h), whatever B, H, W and the content, no host
 * readback: df_bits (one class bit per pixel), df_carry (per column, the nearest row of either class above and below every 32-row tile), df_cols (the
 * column distances, 2 bytes per pixel), df_rows (per row the lower envelope of the columns' parabolas; writes the field).  These are the names in
 * sdm_kernel_counts and the per-launch profile.  The class words, the carries and the column distances are part of the activation arena, host
 * pointers go through the I/O staging (sdm_resident_bytes counts both, sdm_release_memory frees them). */
#define SDM_DF_NONE 2147483647
int sdm_distance_field(sdm_ctx* ctx, const float* plane_bhw, int B, int H, int W, float threshold, int32_t* field_bhw, int ptr_kind, void* stream);
/* Grow (offset_px > 0), shrink (< 0) and feather a mask by any amount: mask fp32 [B,H,W] -> out fp32 [B,H,W].  With the field of mask > threshold:
 *   sd(p)    = sqrt((float)|field[p]|) - 0.5, negated for the pixels of F: the signed distance to the silhouette, which runs half-way between the two
 *            classes.  Negative inside, positive outside, -0.5 to +0.5 across the silhouette.  sqrt is the correctly rounded fp32 square root.
 *   out[p]   = clamp((offset_px - sd(p)) / feather_px + 0.5, 0, 1), fp32 throughout, a true fp32 division.
 * Consequences, exact in fp32:
 *   offset_px = 0, feather_px = 1 returns the binarised mask (1.0 on F, 0.0 elsewhere);
 *   an integer offset_px = r >= 0 with feather_px = 1 gives out == 1.0 exactly on the dilation of F by the closed disk of radius r (d2 <= r^2),
 *   and out > 0 exactly where d2 < (r + 1)^2.
 * SDM_DF_MAX_OFFSET is what keeps the second one true: sqrtf(r^2 + 1) > r holds for r up to 2048 and fails at 4096.
 * An empty or a full F is not an error: |field| is SDM_DF_NONE and the formulas apply.  threshold, B, H, W as sdm_distance_field, offset_px finite
 * within +-SDM_DF_MAX_OFFSET, feather_px finite in [1, SDM_DF_MAX_FEATHER]: SDM_ERR_INVALID otherwise, and then nothing is queued or written.
 * sdmatte_nodes.offset_mask is the same function on CPU tensors.  Stream contract, pointer kinds, weights and memory as sdm_distance_field.  Four
 * launches: df_bits, df_carry, df_cols, df_offset (the row pass with the ramp applied in registers: the field is never stored). */
#define SDM_DF_MAX_OFFSET 1024
#define SDM_DF_MAX_FEATHER 1024
int sdm_offset_mask(sdm_ctx* ctx, const float* mask_bhw, int B, int H, int W, float threshold, float offset_px, float feather_px, float* out_bhw,
                    int ptr_kind, void* stream);
/* An outline (the "sticker" stroke) along the silhouette of a straight-alpha cut-out: fg fp32 [B,H,W,3], alpha fp32 [B,H,W] -> out_rgb [B,H,W,3],
 * out_alpha [B,H,W], straight again: what sdm_compose_canvas takes as foreground and alpha.
 *   a        the alpha with NaN -> 0, clamped to [0, 1].  The field is that of the RAW alpha > edge_threshold, sd as in sdm_offset_mask.
 *   band     [lo, hi] by position: 0 outside: lo = -inf, hi = width_px (the stroke is the dilated silhouette and lies UNDER the subject);
 *            1 centre: [-width_px / 2, width_px / 2]; 2 inside: [-width_px, 0] (both OVER the subject).
 *   coverage c = clamp((hi - sd) / softness_px + 0.5, 0, 1) * clamp((sd - lo) / softness_px + 0.5, 0, 1); the second factor is 1 for lo = -inf.
 *   layers   premultiplied: the stroke (c * opacity * rgb3, As = c * opacity) and the subject (a * F, a); "over" in the order of the position.
 *            out_alpha A = a + As * (1 - a) for position 0, As + a * (1 - As) otherwise.
 *   out_rgb  the straight colour P / A where A > 0, else 0, evaluated as F + (rgb3 - F) * (ws / A) with ws the stroke's share of A (As * (1 - a) for
 *            position 0, As otherwise): exactly F where the stroke adds nothing (opacity 0 returns the subject unchanged), and exactly rgb3 where
 *            a == 0 (the subject's colour means nothing there, whatever it holds).
 * rgb3 is 3 finite floats, ALWAYS a HOST pointer.  An empty or a full silhouette is not an error.  A stroke does not extend beyond the frame: place the
 * cut-out with sdm_compose_canvas first.  B, H, W as sdm_distance_field, edge_threshold finite in [0, 1), position in 0 .. 2, width_px finite in
 * (0, SDM_OUTLINE_MAX_WIDTH], softness_px finite in [1, SDM_DF_MAX_FEATHER], opacity finite in [0, 1]: SDM_ERR_INVALID otherwise, and then nothing is
 * queued or written.  sdmatte_nodes.outline_cutout is the same function in torch (equal to fp32 rounding).  Stream contract, pointer kinds, weights and
 * memory as sdm_distance_field.  Four launches: df_bits, df_carry, df_cols, df_outline (the row pass with the composition applied in registers). */
#define SDM_OUTLINE_MAX_WIDTH 1024
int sdm_outline(sdm_ctx* ctx, const float* fg_bhw3, const float* alpha_bhw, int B, int H, int W, float edge_threshold, int position, float width_px,
                float softness_px, const float* rgb3, float opacity, float* out_rgb_bhw3, float* out_alpha_bhw, int ptr_kind, void* stream);

/* Steady mattes for video, on the GPU (beyond the reference): a temporal filter of the alpha guided by the frames themselves, with no optical flow.  This is
 * the one call whose batch axis is TIME: image [B,H,W,3] is B consecutive frames.  A neighbouring frame contributes to a pixel only as far as the image
 * around that pixel did not change between the two frames: static regions are averaged over time (the frame-to-frame shimmer of per-frame matting goes),
 * and where something moved, or the shot changed, the weight is exactly zero and the frame keeps its own alpha.  Everything is fp32.
 *   image fp32 [B,H,W,3] (values used as they are), alpha fp32 [B,H,W] (a = alpha with NaN -> 0, then clamped to [0,1]), out fp32 [B,H,W] in [0,1]
 *   clips     L = clip_len, or B when clip_len == 0.  Frames [i*L, min(B, i*L + L)) form clip i; clips are independent; the last one may be shorter.
 *   distance  for frames t and s = t + k of the same clip, k != 0, |k| <= radius: e(q) = sum over the 3 channels of (I_s(q,c) - I_t(q,c))^2;
 *             D_k(p) = (sum of e over the pixels q within Chebyshev distance `patch` of p that exist in the frame) / (3*n), n the number of those pixels.
 *             Pixels beyond the border do not exist, as everywhere in this header.
 *   weight    u = 1 - D_k(p) / tau2 with tau2 = color_tolerance * color_tolerance (one fp32 product, a true fp32 division); u = u > 0 ? u : 0 (one compare,
 *             so a NaN distance gives weight 0); g = u*u; w_k = strength * (1 - |k| / (radius + 1)) * g
 *   filter    f = (a_t + sum_k w_k * a_s) / (1 + sum_k w_k) over the k whose frame lies in the clip (a true fp32 division; the denominator is at least 1)
 *   limit     out = clamp(a_t + clamp(f - a_t, -max_change, +max_change), 0, 1)
 * These hold bit for bit:
 *   out equals a when strength == 0, or max_change == 0, or B == 1, or clip_len == 1, or every D_k >= tau2 for the pixel;
 *   a zero weight is an exact no-op in both sums, so a sequence with a hard cut (every D >= tau2 across it) gives the bits of the two shots filtered on
 *   their own: a cut needs no flag;
 *   a call with clip_len = L gives the bits of one call per clip;
 *   a frame's neighbours contribute in a fixed order (k = -1 .. -radius, then +1 .. +radius): two calls, host and device pointers, aligned and unaligned
 *   pointers all give the same bits.
 * sdmatte_nodes.temporal_smooth_alpha is the same function in torch (equal to fp32 rounding, not bit for bit).
 * Limits: B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS; clip_len in 0 .. B; radius in 1 .. SDM_TS_MAX_RADIUS; patch in 0 .. SDM_TS_MAX_PATCH;
 * color_tolerance finite in [1/1024, 1]; strength finite in [0, 1]; max_change finite in [0, 1]: SDM_ERR_INVALID otherwise, with a message that names the
 * argument, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the launch.  Needs
 * no weights.  ONE kernel launch (csrc/k_temporal.h), `ts_smooth` in sdm_kernel_counts and the per-launch profile, whatever the arguments and the content;
 * every frame is read once per tile (about 20 bytes per pixel and frame), no host readback.  The call keeps nothing in the arena; host pointers go
 * through the I/O staging (sdm_resident_bytes counts it, sdm_release_memory frees it). */
#define SDM_TS_MAX_RADIUS 4
#define SDM_TS_MAX_PATCH 2
int sdm_smooth_alpha_temporal(sdm_ctx* ctx, const float* image_bhwc, const float* alpha_bhw, int B, int H, int W, int clip_len, int radius, int patch,
                              float color_tolerance, float strength, float max_change, float* out_bhw, int ptr_kind, void* stream);

/* The same filter along the motion (beyond the reference): sdm_smooth_alpha_temporal compares a pixel with the SAME pixel of the neighbouring frames, so
 * where the subject moves - its soft edge, its hair: the pixels that shimmer most - the weight is 0 and nothing is smoothed.  Here every pixel first looks
 * for the patch around it in the neighbouring frame, among the integer displacements within `search`, and is filtered with the alpha found there.  No
 * optical flow, no weights: a search with the patch distance of the call above.  Unchanged from that call: the batch axis is time; the sanitising (a), the
 * clips, tau2 = color_tolerance * color_tolerance, the filter and the limit; everything fp32, true fp32 divisions, no FMA contraction.  New, per target
 * frame t, neighbour s = t + k (same clip, 0 < |k| <= radius) and pixel p:
 *   candidates d = (dy, dx) with |dy|, |dx| <= search for which p + d lies in the frame
 *   distance   e_d(q) = sum over the 3 channels of (I_s(q + d, c) - I_t(q, c))^2;  D_d(p) = (sum of e_d(q) over the q within Chebyshev distance `patch` of p
 *              for which q and q + d both exist) / (3 * n_d), n_d the number of those q (n_d >= 1: q = p counts).  Pixels beyond the border do not exist.
 *   cost       C_d = D_d + pt * (float)(dy*dy + dx*dx), pt = motion_penalty * tau2 (one fp32 product)
 *   choice     a candidate is eligible iff C_d == C_d (not NaN); d* is the eligible candidate with the lexicographically smallest
 *              (C_d, dy*dy + dx*dx, dy, dx).  If none is eligible the pair contributes nothing.
 *   weight     u = 1 - D_d* / tau2 (the distance, not the cost); u = u > 0 ? u : 0; w_k = (strength * (1 - |k| / (radius + 1))) * (u*u); the sample is
 *              a_s(p + d*)
 *   filter     f = (a_t + sum_k w_k * a_s(p + d*_k)) / (1 + sum_k w_k), in the order k = -1 .. -radius, then +1 .. +radius; out as in the call above
 * The order in which the terms of a patch are summed is not part of the contract; the choice rule is.
 * search == 0 is accepted and IS sdm_smooth_alpha_temporal: the same launch (`ts_smooth`) and the same bits; motion_penalty is not looked at.
 * These hold bit for bit:
 *   out equals a when strength == 0, or max_change == 0, or B == 1, or clip_len == 1, or every D_d of every candidate is >= tau2;
 *   a clip with a hard cut gives the bits of its two shots, if every pixel of one shot differs by >= color_tolerance per channel from every pixel of the
 *   other (then every D_d across the cut is >= tau2, whatever the displacement);
 *   a call with clip_len = L gives the bits of one call per clip;
 *   two calls, host and device pointers, aligned and unaligned pointers all give the same bits.
 * sdmatte_nodes.temporal_smooth_alpha_motion is the same function in torch (equal to fp32 rounding wherever the choice is not a near-tie).
 * Limits: search in 0 .. SDM_TSM_MAX_SEARCH; motion_penalty finite in [0, 1]; every other limit is that of sdm_smooth_alpha_temporal: SDM_ERR_INVALID
 * otherwise, with a message that names the argument, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap;
 * sdm_last_forward_ms covers the launch.  Needs no weights.  For search >= 1 ONE kernel launch (csrc/k_motion.h), `tsm_smooth` in sdm_kernel_counts and
 * the per-launch profile, whatever the arguments and the content; no host readback.  The call keeps nothing in the arena; host pointers go through the
 * I/O staging. */
#define SDM_TSM_MAX_SEARCH 8
#define SDM_TSM_SEARCH 4
#define SDM_TSM_MOTION_PENALTY 0.02f
int sdm_smooth_alpha_motion(sdm_ctx* ctx, const float* image_bhwc, const float* alpha_bhw, int B, int H, int W, int clip_len, int radius, int patch,
                            int search, float color_tolerance, float motion_penalty, float strength, float max_change, float* out_bhw,
                            int ptr_kind, void* stream);

/* The subject over its own background, out of focus (beyond the reference): "portrait mode", background blur.  Blurring the photo and mixing it back by
 * alpha blurs the subject's colours into the background, where they show as a halo around the silhouette; here the blur is normalised and does not see
 * the subject, and its kernel is a disc, as a lens's is, with an optional boost of the highlights.  No weights.
 * image, fg, bg and out are fp32 [B,H,W,3], alpha is fp32 [B,H,W]; fg_bhwc and bg_bhwc may each be NULL; all of one pointer kind.  Colours are used as
 * they are.  They must be finite: a non-finite colour gives an unspecified value in every pixel whose disc contains it, never an out-of-bounds access.
 *   a      the alpha with NaN -> 0, then clamped to [0, 1]
 *   C, F   C = bg if given, else image; F = fg if given, else image.  (With the two planes of sdm_estimate_foreground the soft edge pixels are clean on
 *          both sides; without them the call still works.)
 *   weight Y(q) = (C.r + C.g + C.b) / 3;  w(q) = (1 - a(q)) * (1 + highlight_gain * max(0, Y(q) - highlight_threshold)).  With highlight_gain == 0 the
 *          second factor is exactly 1.
 *   disc   D(p) = the pixels q = p + (dy, dx) with dy*dy + dx*dx <= R*R that exist, R = radius_px: the closed disc, the membership rule of
 *          sdm_make_trimap.  Pixels beyond the border do not exist.  The half widths hw(dy) = the largest h with h*h <= R*R - dy*dy are computed in
 *          integers on the host.
 *   sums   S(p) = sum over q in D(p) of w(q) * C(q), per channel;  N(p) = sum over q in D(p) of w(q)
 *   blur   Bb(p) = (S(p) + e * C(p)) / (N(p) + e), e = SDM_DEFOCUS_FLOOR = 2^-10, a true fp32 division.  The floor removes the 0 / 0 deep inside a subject
 *          larger than the disc; it has no branch, so the function is continuous.  (N >= 0; an implementation may clamp a computed N at 0 so that a
 *          rounding error cannot take the denominator below e.)
 *   out    out(p) = a * F(p) + (1 - a) * Bb(p)
 * Everything is fp32, no FMA contraction.  The order in which the terms of a disc are summed is not part of the contract (the rule of
 * sdm_smooth_alpha_motion for its patch sums), but it depends on the pixel's position only, so these hold bit for bit:
 *   1. where a(p) == 1, out(p) == F(p);
 *   2. if w(q) * C_c(q) == 0 for every pixel q of an image and a channel c, then out_c == a * F_c in that image (no halo: every partial sum of whatever
 *      summation scheme is a sum of zeros.  This is a statement about the whole image, not about one disc);
 *   3. an image's result does not depend on the batch it is in; two calls, host and device pointers, and pointers 4 bytes off a 16-byte boundary all give
 *      the same bits.
 * sdmatte_nodes.defocus_background is the same function in torch (equal to fp32 rounding).
 * Limits: B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS; radius_px in 1 .. SDM_DEFOCUS_MAX_RADIUS; highlight_gain finite in [0, 64];
 * highlight_threshold finite in [0, 1]: SDM_ERR_INVALID otherwise, with a message that names the argument, and then nothing is queued or written.  Stream
 * contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the launches.  Needs no weights.  TWO kernel launches (csrc/k_defocus.h),
 * `dof_prefix` then `dof_gather` in sdm_kernel_counts and the per-launch profile, whatever the arguments, the sizes and the content; no host readback.
 * One plane of 16 bytes per pixel lives in the activation arena; host pointers go through the I/O staging. */
#define SDM_DEFOCUS_MAX_RADIUS 64
#define SDM_DEFOCUS_MAX_GAIN 64
#define SDM_DEFOCUS_FLOOR 0.0009765625f
#define SDM_DEFOCUS_RADIUS 16
#define SDM_DEFOCUS_HIGHLIGHT_GAIN 0.0f
#define SDM_DEFOCUS_HIGHLIGHT_THRESHOLD 0.8f
int sdm_defocus_background(sdm_ctx* ctx, const float* image_bhwc, const float* alpha_bhw, const float* fg_bhwc, const float* bg_bhwc, int B, int H, int W,
                           int radius_px, float highlight_gain, float highlight_threshold, float* out_bhwc, int ptr_kind, void* stream);

/* The photo without its subject (beyond the reference): the clean plate.  Every other call keeps the subject; this one gives back the background behind it,
 * for moving or rescaling the subject inside its own photo (sdm_compose_canvas over the plate), for a two-layer parallax split, as a background without a
 * subject-shaped hole for sdm_harmonize / sdm_defocus_background, or as the pre-fill in front of a generative inpainting model.  The hole is filled by
 * push-pull: weighted averages down a pyramid, then bilinear interpolation back up that keeps every pixel the pyramid knows.  Deterministic, no weights.
 * image, bg and out are fp32 [B,H,W,3]; alpha and hole are fp32 [B,H,W]; bg_bhwc and hole_bhw may each be NULL; all of one pointer kind.  Colours are
 * used as they are.  They must be finite: a non-finite colour gives unspecified values, never an out-of-bounds access.
 *   a       the alpha with NaN -> 0, then clamped to [0, 1].  With a hole plane, sanitised the same way, a = max(a, hole): a shadow, or a second object
 *           to take out.
 *   C       bg if given, else image (the image is then not read).  With the background plane of sdm_estimate_foreground the soft pixels carry clean
 *           colours.
 *   w_0     clamp(1 - a / alpha_cut, 0, 1), in fp32 with a true division: a == 0 gives exactly 1, a >= alpha_cut exactly 0.  alpha_cut is finite in
 *           [SDM_PLATE_MIN_CUT, 1] = [2^-10, 1]; the default SDM_PLATE_ALPHA_CUT = 1/16 suits a call WITHOUT bg: a soft pixel of the image is contaminated
 *           by the subject's colour, so only nearly pure background may count.  WITH bg the natural value is 1: w_0 = 1 - a.
 *   levels  (h_0, w_0) = (H, W), (h_{l+1}, w_{l+1}) = (ceil(h_l / 2), ceil(w_l / 2)), down to (1, 1).
 *   pull    pixel (i, j) of level l + 1 has the children (2 i + dy, 2 j + dx), dy, dx in {0, 1}, that exist at level l, taken in the order (0,0) (0,1)
 *           (1,0) (1,1) and summed as ((t0 + t1) + t2) + t3, missing children left out:  Sw = sum of w_l,  Sc = sum of w_l * C_l per channel;
 *           C_{l+1} = Sc / Sw if Sw > 0, else 0 (a true fp32 division);  w_{l+1} = min(1, Sw).
 *   push    F_top = C_top.  For pixel (y, x) of level l:  ny = y >> 1, fy = clamp(ny + (y odd ? 1 : -1), 0, h_{l+1} - 1), and nx, fx from x likewise;
 *           U = 0.75 * (0.75 * F[ny,nx] + 0.25 * F[ny,fx]) + 0.25 * (0.75 * F[fy,nx] + 0.25 * F[fy,fx])   (bilinear at half-pixel centres, integer addresses);
 *           F_l = w_l * C_l + (1 - w_l) * U;   out = F_0.
 * Everything is fp32, no FMA contraction, in the order written.  An image with no pixel of w_0 > 0 (all subject) gets an all-zero plate: there is no
 * colour to fill with.  These hold bit for bit:
 *   1. where w_0 == 1, out == C: background pixels are not touched, so there is no seam to hide;
 *   2. a channel of C that is 0 wherever w_0 > 0 is 0 in the whole plate: the subject's colour never enters;
 *   3. with an alpha of 0 and 1 only and C == 0.5 wherever a == 0, the plate is exactly 0.5 everywhere;
 *   4. an image's result does not depend on the batch it is in; two calls, host and device pointers, and pointers 4 bytes off a 16-byte boundary all give
 *      the same bits.
 * sdmatte_nodes.clean_plate is the same function in torch (equal to fp32 rounding).
 * Limits: B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS; alpha_cut as above: SDM_ERR_INVALID otherwise, with a message that names the argument,
 * and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the launches.  Needs no
 * weights.  Kernel launches (csrc/k_plate.h): with S = the number of levels l with max(h_l, w_l) > 32 (0 for a photo of at most 32 x 32, else
 * ceil(log2(max(H, W) / 32))), ceil(S / 3) of `plate_pull`, one of `plate_small`, then ceil(S / 3) of `plate_push` in sdm_kernel_counts and the per-launch
 * profile: 1 + 2 * ceil(S / 3) in all, a function of H and W only (7 at 2160 x 3840, where S = 7); no host readback, no atomics.  The pyramid (levels 1 .. S at
 * 16 bytes per pixel, about a third of 16 bytes per pixel of the photo) lives in the activation arena; host pointers go through the I/O staging. */
#define SDM_PLATE_ALPHA_CUT 0.0625f
#define SDM_PLATE_MIN_CUT 0.0009765625f
int sdm_fill_background(sdm_ctx* ctx, const float* image_bhwc, const float* alpha_bhw, const float* bg_bhwc, const float* hole_bhw, int B, int H, int W,
                        float alpha_cut, float* out_bhwc, int ptr_kind, void* stream);

/* The cut-out in its new scene (beyond the reference): colour match and light wrap.  A subject shot under one light and placed over a scene under another
 * looks pasted on with a plain "over": its colours do not match the scene's light, and its edge carries none of it.  This call moves the subject's colour
 * statistics towards the scene's, lets the scene's light spill over the subject's edge, and composes.  No weights.
 * fg is fp32 [B,H,W,3] straight colours (sdm_estimate_foreground), alpha is fp32 [B,H,W], bg_image is fp32 [bg_batch,H,W,3] with bg_batch 1 or B (the rule of
 * sdm_compose_canvas), out and fg_out are fp32 [B,H,W,3], map_out is fp32 [B,12]; fg_out and map_out may each be NULL; all of one pointer kind.  Colours
 * are used as they are.  They must be finite: a non-finite colour gives unspecified values, never an out-of-bounds access.
 *   a       the alpha with NaN -> 0, then clamped to [0, 1].  Bg = image b of bg_image, or image 0 when bg_batch == 1.
 *   o(c)    the opponent coordinates of a colour (r, g, b):  l = ((r + g) + b) / 3 (a true fp32 division), p = r - g, q = (r + g) / 2 - b
 *   moments per image.  Subject: Wf = sum of a;  mf_c = sum of a o_c(F) / Wf;  vf_c = sum of (a o_c(F)) o_c(F) / Wf - mf_c^2.  Scene, over all H W pixels
 *           of Bg with weight 1 (the scene's light is a property of the scene, its hidden part included): mb_c and vb_c, formed the same way.  The
 *           per-pixel terms are fp32; they are summed in fp32 over runs of at most SDM_HZ_RUN = 4096 consecutive pixels (row-major) of one image; the
 *           partials and everything after them are fp64.  The order of summation depends on H and W only, never on B or on the image's index.  A variance
 *           formed this way from rounded sums may come out a rounding error below 0 (a flat-coloured subject): vf_c and vb_c are clamped at 0.
 *   map     s_0 = luma_strength, s_1 = s_2 = chroma_strength;  rho_c = sqrt((vb_c + e) / (vf_c + e)), e = SDM_HZ_VAR_FLOOR = 2^-20, clamped to
 *           [1 / SDM_HZ_MAX_GAIN, SDM_HZ_MAX_GAIN];  g_c = 1 + contrast_strength s_c (rho_c - 1);  h_c = mf_c (1 - g_c) + s_c (mb_c - mf_c).  In RGB:
 *           M = I + sum over c of (g_c - 1) P_c,  t = sum over c of h_c k_c, with the projectors of the coordinates above,
 *             P_l = all 1/3;  P_p = [[1/2, -1/2, 0], [-1/2, 1/2, 0], [0, 0, 0]];  P_q = [[1/6, 1/6, -1/3], [1/6, 1/6, -1/3], [-1/3, -1/3, 2/3]];
 *             k_l = (1, 1, 1);  k_p = (1/2, -1/2, 0);  k_q = (1/3, 1/3, -2/3)
 *           (P_l + P_p + P_q = I, and g = 1 gives exactly I).  All fp64, rounded to fp32 at the end.  If Wf < SDM_HZ_MIN_WEIGHT = 1 (less than one pixel
 *           of subject) or luma_strength == chroma_strength == 0: M = I and t = 0.  map_out[b] = the nine entries of M row-major, then the three of t.
 *   match   F'_r = clamp(((t_r + M_r0 F.r) + M_r1 F.g) + M_r2 F.b, 0, 1), likewise g and b: fp32, in that order, no FMA contraction.
 *   wrap    skipped entirely when wrap_strength == 0 (wrap_sigma is then not looked at).  v = 1 - a;  X = (v Bg.r, v Bg.g, v Bg.b, v): the visible
 *           background only, premultiplied as in sdm_defocus_background.  r = ceil(3 wrap_sigma);  w_i = exp(-i^2 / (2 sigma^2)) for |i| <= r, normalised,
 *           computed in double and rounded to fp32 (the shadow of sdm_compose_canvas).  X and T are 0 beyond the frame.
 *             T(y, x) = sum over i = -r .. r (ascending) of w_i X(y, x + i);  (Wr, Wg, Wb, m)(y, x) = sum over j = -r .. r (ascending) of w_j T(y + j, x)
 *             F''_c = clamp(F'_c + wrap_strength (W_c - m F'_c), 0, 1).  Without the wrap F'' = F'.
 *   out     out = a F'' + (1 - a) Bg;  fg_out = F''.
 * These hold bit for bit:
 *   1. where a(p) == 0, out(p) == Bg(p);
 *   2. where a(p) == 1, out(p) == fg_out(p);
 *   3. with all five strengths 0 and F in [0, 1]: fg_out == F and out == a F + (1 - a) Bg (fp32, no contraction);
 *   4. if every existing pixel within Chebyshev distance r of p has a == 1, fg_out(p) equals the fg_out(p) of the same call with wrap_strength = 0 (every
 *      term of both passes is a zero);
 *   5. an image's result does not depend on the batch it is in; two calls, host and device pointers, and pointers 4 bytes off a 16-byte boundary all give
 *      the same bits;
 *   6. bg_batch = 1 gives the bits of the same background repeated B times.
 * sdmatte_nodes.harmonize_map and sdmatte_nodes.harmonize_cutout are the same function in torch (equal to fp32 rounding).
 * Limits: B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS; luma_strength, chroma_strength, contrast_strength and wrap_strength finite in [0, 1];
 * wrap_sigma finite in (0, SDM_HZ_MAX_WRAP_SIGMA] when wrap_strength > 0 (so r <= 48); bg_batch 1 or B: SDM_ERR_INVALID otherwise, with a message that
 * names the argument, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the
 * launches.  Needs no weights.  Kernel launches (csrc/k_harmonize.h), by these names in sdm_kernel_counts and the per-launch profile: `hz_stats` and
 * `hz_finalize` when luma_strength > 0 or chroma_strength > 0, `hz_rows` when wrap_strength > 0, `hz_compose` always - 4 with everything on, 3 without
 * the wrap, 2 without the match, 1 with neither; the count never depends on sizes or content; no host readback.  The partial sums (56 bytes per run), the
 * map and, with the wrap, one plane of 16 bytes per pixel live in the activation arena; host pointers go through the I/O staging. */
#define SDM_HZ_RUN 4096
#define SDM_HZ_VAR_FLOOR 9.5367431640625e-07
#define SDM_HZ_MAX_GAIN 4
#define SDM_HZ_MIN_WEIGHT 1.0
#define SDM_HZ_MAX_WRAP_SIGMA 16
#define SDM_HZ_LUMA_STRENGTH 0.6f
#define SDM_HZ_CHROMA_STRENGTH 0.8f
#define SDM_HZ_CONTRAST_STRENGTH 0.5f
#define SDM_HZ_WRAP_STRENGTH 0.5f
#define SDM_HZ_WRAP_SIGMA 6.0f
int sdm_harmonize(sdm_ctx* ctx, const float* fg_bhw3, const float* alpha_bhw, const float* bg_image, int bg_batch, int B, int H, int W,
                  float luma_strength, float chroma_strength, float contrast_strength, float wrap_strength, float wrap_sigma, float* out_bhw3,
                  float* fg_out_bhw3, float* map_out_b12, int ptr_kind, void* stream);

/* Green-screen shots (beyond the reference): the screen's colour, the colour-difference key, a trimap from the key, despill.  A subject in front of a green
 * or blue screen carries its own mask in its colours: a classical keyer is unreliable where the model is good (hair, blur, glass) and reliable where the
 * model needs help (which pixels are certainly screen, which certainly subject), so the keyer is the trimap source for such footage.  No weights.
 * All arithmetic is fp32 without FMA contraction, in the order written; a compare is one fp32 compare, so a NaN fails it.
 *
 * sdm_screen_colour: image is fp32 [B,H,W,3], screen_b3 is fp32 [B][3], info_b4 is int32 [B][4] or NULL; all of one pointer kind.
 *   eligible  for a pixel (r, g, b): s = (r + g) + b; mx the largest and mn the smallest of the three, formed by compares.  The pixel is eligible iff
 *             s >= SDM_KEY_MIN_SUM (0.15) and mx - mn >= SDM_KEY_MIN_SAT (0.25) * s and, for hint = 1 (green), g > r and g > b, for hint = 2 (blue),
 *             b > r and b > g; hint = 0 takes any saturated colour.
 *   bin       an eligible pixel falls into bin (iu, iv), iu = min(63, (int)((r / s) * 64)), iv = min(63, (int)((g / s) * 64)), of a 64 x 64 int32 histogram
 *             of chromaticity (normalising by s makes an unevenly lit screen one cluster).  Where the quotient times 64 is negative or a NaN (an image
 *             with negative or infinite colours) the index is 0: the cast would be undefined.
 *   slots     one histogram per image; with share = 1 one for the whole batch (a clip has one screen), and the slot's pixels are those of the images laid
 *             end to end as one image of B * H rows.
 *   mode      C(iu, iv) = the sum of the up to nine bins of the 3 x 3 neighbourhood inside the grid; the mode is the bin of the largest C, on a tie the
 *             smallest index iu * 64 + iv.
 *   colour    the mean of r, g, b over the slot's eligible pixels whose bin lies in the mode's 3 x 3 neighbourhood (the selected pixels): fp32 sums per
 *             run of SDM_KEY_RUN = 4096 consecutive pixels of the slot in a fixed tree (the summation contract of sdm_harmonize), an integer count;
 *             the runs are added in fp64 in ascending order, the division is fp64, rounded once to fp32.
 *   outputs   screen_b3[b] = the colour of image b's slot (with share = 1 every row is the same); info_b4[b] = {eligible pixels, selected pixels, iu, iv}
 *             of that slot.  A slot without an eligible pixel gives the colour (0, 0, 0) and {0, 0, -1, -1}.
 * Histogram, mode and info are integers: GPU, emulator and any other evaluation agree on them exactly.
 *
 * sdm_chroma_key: image is fp32 [B,H,W,3]; screen is fp32 [B][3] (screen_is_plane = 0) or [B][H][W][3] (screen_is_plane = 1: a colour per pixel, for
 * example the plate of sdm_fill_background), of the image's pointer kind; key_bhw and trimap_bhw are fp32 [B,H,W], despilled_bhwc is fp32 [B,H,W,3];
 * each output may be NULL, but not all three.  Per pixel, c the pixel and S its screen colour:
 *   k         the index of the largest component of S, the lowest on a tie; o1 < o2 the other two;  y(v) = (v[o1] > v[o2]) ? v[o1] : v[o2]
 *   m = c[k] - y(c);  mS = S[k] - y(S);  the pixel is VALID iff mS >= SDM_KEY_MIN_SEP (1/64) and m is finite.
 *   key       a valid pixel gets clamp01(q), t = clip_bg * mS, q = (t - m) / ((clip_bg - clip_fg) * mS), clamp01(q) = q > 0 ? (q < 1 ? q : 1) : 0; an
 *             invalid pixel gets 1.  (The colour-difference key: m / mS is 1 on the screen and 0 on anything whose k-th channel does not stand out.)
 *   class     F iff valid and m <= sure_fg * mS;  B iff valid, not F and m >= sure_bg * mS;  U otherwise.  Products, not quotients: the plane is exact.
 *   trimap    T0 = the trimap of sdm_make_trimap(key, 0.5, erode_px, dilate_px) as that call defines it, on this call's key.  The result is T0 where
 *             (T0 == 1 and the class is F) or (T0 == 0 and the class is B) or T0 == 0.5, and 0.5 elsewhere: the band follows the robust 0.5 contour of the
 *             key, a pixel counts as definite only where its own colour agrees, and a stray unsure pixel stays ONE unknown pixel (it does not grow).
 *   despilled the k-th channel becomes c[k] - despill * m where the pixel is valid and m > 0; everything else is a bit copy.
 * These hold bit for bit:
 *   1. despill = 0 copies the image;
 *   2. a valid pixel equal to its screen colour has key 0 and, with sure_fg < 1 and sure_bg <= 1, class B;
 *   3. a valid pixel with r = g = b has key 1 and, with sure_fg >= 0, class F;
 *   4. a plane that holds one colour per image gives the bits of the colour form;
 *   5. the trimap equals the formula above evaluated with sdm_make_trimap on the call's own key output;
 *   6. an image's results (sdm_screen_colour with share = 0, sdm_chroma_key) do not depend on the batch it is in; two calls, host and device pointers, and
 *      pointers 4 bytes off a 16-byte boundary all give the same bits;
 *   7. sdm_screen_colour with share = 1 equals the call on the images laid end to end as one image of B * H rows (rows do not interact in that call).
 * sdmatte_nodes.screen_colour and sdmatte_nodes.chroma_key are the same functions in torch (the integers and sdm_chroma_key bit for bit, the colour to fp32
 * rounding).
 * Limits: hint 0, 1 or 2; share 0 or 1; without share B <= SDM_KEY_MAX_SLOTS = 65536 (a histogram per image, indexed with ints); clip_fg finite in
 * [0, 1), clip_bg in (clip_fg, 1], sure_fg finite in [-1, 1], sure_bg in [sure_fg, 2], despill in [0, 1]; the radii in 0 .. SDM_TRIMAP_MAX_RADIUS (looked
 * at with or without trimap_bhw); B, H, W >= 1 within SDM_FG_MAX_SIDE / SDM_FG_MAX_PIXELS: SDM_ERR_INVALID otherwise, with a message that names the
 * argument, and then nothing is queued or written.  Stream contract and pointer kinds as sdm_make_trimap; sdm_last_forward_ms covers the launches.  Kernel
 * launches (csrc/k_key.h), by these names in sdm_kernel_counts and the per-launch profile: sdm_screen_colour makes 5 (`ck_clear`, `ck_hist`, `ck_mode`,
 * `ck_mean`, `ck_finalize`); sdm_chroma_key makes 1 (`ck_key`) without trimap_bhw and 4 with it (`ck_key`, `trimap_cols`, `trimap_rows`, `ck_veto`); the
 * counts depend on the arguments only; no host readback.  The histograms (16 KB per slot), the partials (16 bytes per run), the class bytes (1 per pixel),
 * the int16 plane of sdm_make_trimap and, when trimap_bhw is given without key_bhw, the key live in the activation arena; host pointers go through the
 * I/O staging. */
#define SDM_KEY_MIN_SUM 0.15f
#define SDM_KEY_MIN_SAT 0.25f
#define SDM_KEY_MIN_SEP 0.015625f
#define SDM_KEY_RUN 4096
#define SDM_KEY_MAX_SLOTS 65536
#define SDM_KEY_CLIP_FG 0.15f
#define SDM_KEY_CLIP_BG 0.85f
#define SDM_KEY_SURE_FG 0.05f
#define SDM_KEY_SURE_BG 0.95f
int sdm_screen_colour(sdm_ctx* ctx, const float* image_bhwc, int B, int H, int W, int hint, int share, float* screen_b3, int32_t* info_b4, int ptr_kind,
                      void* stream);
int sdm_chroma_key(sdm_ctx* ctx, const float* image_bhwc, const float* screen, int screen_is_plane, int B, int H, int W, float clip_fg, float clip_bg,
                   float sure_fg, float sure_bg, int erode_px, int dilate_px, float despill, float* key_bhw, float* trimap_bhw, float* despilled_bhwc,
                   int ptr_kind, void* stream);

/* Score a matte (beyond the reference): SAD, MSE, Grad and Conn, the four numbers of the matting literature (Rhemann et al., "A perceptually motivated
 * online benchmark for image matting"; the SDMatte paper reports them), over the unknown band of the trimap.  No weights.
 * pred and gt are fp32 [B,H,W]; trimap is fp32 [B,H,W] in [0, 1] or NULL; stats is fp64 [B][SDM_MM_STATS]; level is int32 [B,H,W] or NULL; all of one
 * pointer kind.
 *   p, g    pred and gt with NaN -> 0, then clamped to [0, 1] (the rule of sdm_estimate_foreground).
 *   R       { q : |trimap[q] - 0.5| < 0.25 }: one fp32 subtraction, fabsf and one compare, so a NaN lies outside.  With trimap == NULL R is the whole
 *           frame, bit for bit what a plane of 0.5 gives.
 *   terms   fp32, no FMA contraction: e = p - g;  SAD term |e|;  SSE term e e.
 *   Grad    the Gaussian-derivative form.  r = ceil(sigma sqrt(-2 ln(sqrt(2 pi) sigma 0.01))) (4 at sigma = 1.4, at most SDM_MM_MAX_GRAD_RADIUS);
 *           G_i = exp(-i^2 / (2 sigma^2)) / (sigma sqrt(2 pi)), D_i = -i G_i / sigma^2 for i = -r .. r, both divided by sqrt(sqrt(sum G^2 sum D^2)), so
 *           that the 2-D kernel G (x) D has unit L2 norm; computed in double from the fp32 sigma and rounded to fp32 (as the weights of
 *           sdm_compose_canvas and sdm_harmonize).  A pixel beyond the frame takes the value of the nearest pixel of the frame.  For a plane a:
 *             a_x(y, x) = sum over j of D_j (sum over i of G_i a(y + i, x + j)),  a_y(y, x) = sum over j of G_j (sum over i of D_i a(y + i, x + j)),
 *           the inner sums (over the rows, i) first, both sums ascending in their index, fp32, no FMA contraction;
 *           m(a) = sqrtf(a_x^2 + a_y^2);  Grad term (m(p) - m(g))^2.  The planes are NOT min-max normalised first, as the common Python port does: that
 *           step is the identity whenever a plane reaches 0 and 1, which a ground truth does.
 *   Conn    only when with_conn != 0 (step 0.1 and theta = SDM_MM_CONN_THETA of the common code).  t_k = (float)k / 10.0f for k = 0 .. 10, true fp32
 *           divisions (t_10 == 1.0f);  c = min(p, g);  S_k = { q : c[q] >= t_k } over the WHOLE FRAME, not over R;  Omega_k = the 4-connected component of
 *           S_k with the largest area, on a tie the one that contains the smallest pixel index, empty when S_k is.  L(q) = the largest k in 0 .. 10 with
 *           q in Omega_j for every 1 <= j <= k: a pixel is frozen at the first level it drops out of and stays frozen even if a later Omega contains it
 *           again (the Omega_k are not nested).  l = t_L;  phi(a) = 1 - d [d >= 0.15f] with d = a - l;  Conn term |phi(p) - phi(g)|.  level receives L:
 *           integers and compares only, so every implementation agrees exactly.  With with_conn == 0, level must be NULL and stats[4] is 0.
 *   stats[b]  0: n = |R|;  1: sum over R of |e|;  2: sum over R of e e;  3: sum over R of the Grad term;  4: sum over R of the Conn term;  5: max |e| over R
 *           (0 when R is empty);  6: sum of |e| over the frame;  7: sum of e e over the frame.  Raw sums: the literature's units (SAD / 1000, SSE / n,
 *           Grad / 1000, Conn / 1000) are made by the caller.
 *   sums    the fp32 terms are added in fp32 inside a unit - a tile of 64 columns x 32 rows for entries 1-3 and 5-7, a run of 4096 consecutive pixels
 *           (row-major) for entry 4 - in a fixed order (shuffle and LDS trees, no float atomics); the units of an image are added in fp64 in ascending
 *           order.  An image's eight numbers therefore do not depend on the batch it is in, on the pointer kind, or on the run.  n and the maximum are exact.
 * sdmatte_nodes.matte_metrics is the same function in torch (the level map exactly, the sums to the rounding of its dtype).
 * Limits: grad_sigma finite in [0.25, 4] (so r <= 9); with_conn 0 or 1; level NULL unless with_conn; B, H, W >= 1 within SDM_FG_MAX_SIDE /
 * SDM_FG_MAX_PIXELS (the ten levels are labelled one after the other, labels being global pixel indices, so B H W is also the labelled pixel count):
 * SDM_ERR_INVALID otherwise, also for an unknown ptr_kind, and then nothing is queued or written.  Stream contract, pointer kinds, staging and arena as
 * sdm_harmonize; sdm_last_forward_ms covers the launches.  Needs no weights.  No host readback.  Kernel launches (csrc/k_metrics.h, csrc/k_cclabel.h), by
 * these names in sdm_kernel_counts and the per-launch profile: `mm_pixel` and `mm_finalize` always; with Conn also, per level, `cc_tile`, `cc_seam`,
 * `cc_flatten`, `cc_select` x 2 and `mm_level` (60 in all), and `mm_conn` - 2 launches without Conn, 63 with it, whether or not level is given (mm_conn
 * writes it); the count never depends on B, H, W or the content.  With Conn five planes of 4 bytes per pixel live in the activation arena. */
#define SDM_MM_STATS 8
#define SDM_MM_GRAD_SIGMA 1.4f
#define SDM_MM_MAX_GRAD_RADIUS 9
#define SDM_MM_CONN_LEVELS 10
#define SDM_MM_CONN_THETA 0.15f
int sdm_matte_metrics(sdm_ctx* ctx, const float* pred_bhw, const float* gt_bhw, const float* trimap_bhw /* may be NULL */, int B, int H, int W,
                      float grad_sigma, int with_conn, double* stats_b8, int32_t* level_bhw /* may be NULL */, int ptr_kind, void* stream);

/* Memory the engine holds outside any framework allocator: packed weights + activation arena (sized by the largest batch /
 * resolution seen) + I/O staging.  sdm_release_memory frees everything but the weights (the next forward re-allocates). */
int64_t sdm_resident_bytes(sdm_ctx* ctx);
/* The weight part of it: the canonical blob (sdm_weight_blob_bytes) plus the kernel-specific layouts derived from it.
 * sdm_resident_bytes - sdm_weight_bytes = what sdm_release_memory gives back. */
int64_t sdm_weight_bytes(sdm_ctx* ctx);
int sdm_release_memory(sdm_ctx* ctx);

/* Kernel-selection options.  The library reads NO environment variable: every choice among its kernel variants has one default, and
 * this is the only way to change one (tests and the A/B tools under tools/ do; the ComfyUI node never does).  Process-wide; names and
 * meanings: sdm_option_name(i) / sdm_option_help(i) for i = 0 .. until NULL.  Options marked "read when a model is built" / "read at
 * sdm_create" must be set before that call.  Returns SDM_ERR_INVALID for an unknown name. */
int sdm_set_option(const char* name, int value);
int sdm_get_option(const char* name, int* value);
void sdm_reset_options(void);
const char* sdm_option_name(int i);
const char* sdm_option_help(int i);
/* Which kernel variants were launched since the last reset, as "name=count;..." (returns the full length; truncates to cap).  Lets a
 * test assert that the variant it means to check is the one that ran. */
int sdm_kernel_counts(char* buf, int cap);
void sdm_kernel_counts_reset(void);

/* Block until everything queued on the engine stream has finished. */
int sdm_synchronize(sdm_ctx* ctx);

/* Time (ms) spent by the GPU in the last sdm_forward/sdm_apply_matte (or sdm_make_trimap / sdm_clean_mask / sdm_subject_roi / sdm_estimate_foreground / sdm_refine_alpha_guided / sdm_compose_canvas / sdm_smooth_alpha_temporal / sdm_smooth_alpha_motion / sdm_defocus_background / sdm_fill_background / sdm_harmonize / sdm_matte_metrics: their launches), measured with HIP events on the
 * stream the kernels were launched on.  Valid after sdm_synchronize. */
float sdm_last_forward_ms(sdm_ctx* ctx);

/* Per-kernel-class event timing of the next forward (debug/bench): enable, run, then read back
 * `n` (name, ms, launches) triples.  Adds an event pair per launch - not for the timed bench loop. */
int sdm_profile_enable(sdm_ctx* ctx, int on);
int sdm_profile_count(sdm_ctx* ctx);
/* CSV (kernel,ms,gflop,mbytes,desc), one line per launch of the last profiled forward. */
const char* sdm_profile_dump(sdm_ctx* ctx);
int sdm_profile_get(sdm_ctx* ctx, int i, const char** name, float* ms, int64_t* launches, double* flops, double* bytes);

/* ---- single-operator entry points (parity tests call the same kernels the engine uses) --------------
 * All pointers are DEVICE pointers.  Activations are NHWC; fp16 unless the *_f32 flag says otherwise.
 * From here to the end of this header: test hooks and lab / bench helpers that no product path calls, implemented in csrc/sdm_hooks.h
 * (part of sdm_engine.cpp's translation unit); everything above is the product ABI, implemented in csrc/sdm_engine.cpp. */

/* conv3x3 (ntaps=9) or 1x1/linear (ntaps=1): y = conv(concat(in0,in1)) [*scale] [+bias] [+res] | GEGLU.
 * w: fp32 OIHW [O][I][kh][kw] or [O][I]; I = (C0+C1) real channels.  stride 1|2; pad_mode 0: symmetric pad 1,
 * 1: VAE asymmetric (0,1,0,1) (stride 2).  up=1 fuses a nearest x2 upsample.  tile_cfg = -1 picks
 * automatically, >= 0 forces one of the compiled tile configurations (see sdm_conv_num_cfgs). */
int sdm_op_conv(sdm_ctx* ctx, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up,
                int stride, int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32,
                const void* res, int res_f32, int geglu, float out_scale, int tile_cfg);
int sdm_conv_num_cfgs(int ntaps, int stride);
/* The same with (a) split != 0: split-fp16 operands (the precise mode's kernels; fp32 activations only) and (b) gn_gamma != NULL:
 * GroupNorm(gn_groups, eps)(+SiLU) of the input applied inside the conv's operand staging - the production path of every
 * ResnetBlock2D conv (3x3, stride 1; tile_cfg 0, 4 or 5). */
int sdm_op_conv_ex(sdm_ctx* ctx, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up,
                   int stride, int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32,
                   const void* res, int res_f32, int geglu, float out_scale, int tile_cfg, int split, const float* gn_gamma,
                   const float* gn_beta, float gn_eps, int gn_groups, int gn_silu);
/* Test hook: sdm_op_conv_ex that also hands back the partial {sum, sumsq} rows its epilogue writes for the NEXT GroupNorm - `stats`, [N][*srows][Cst][2] floats
 * with Cst = the stored channel count (O rounded up to 4), one row per (tile, wave row) of an image (split-K: per 64 rows; DESIGN.md 4, "partial rows"); channels
 * >= O of a row are unspecified; room for stats_cap rows per image, more is an error.  in_st0 / in_rows0 (+ in_st1 / in_rows1 for a concat input; NULL: none), with
 * gn_gamma: the fused GroupNorm takes its scale | shift table from these partial rows of the input through gn_partials_scale_shift_kernel, as the model does
 * (sdm_op_conv_ex computes the statistics with the stand-alone kernel).  Honours sdm_debug_set_input_cmask. */
int sdm_op_conv_stats(sdm_ctx* ctx, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int Hin, int Win, int up,
                      int stride, int pad_mode, int ntaps, const float* w, const float* bias, int O, void* out, int out_f32,
                      const void* res, int res_f32, int geglu, float out_scale, int tile_cfg, int split, const float* gn_gamma,
                      const float* gn_beta, float gn_eps, int gn_groups, int gn_silu, const float* in_st0, int in_rows0, const float* in_st1,
                      int in_rows1, float* stats, int stats_cap, int* srows);
/* Test hook: gn_partials_scale_shift_kernel alone.  st0 [N][rows0][C0][2] (+ st1 [N][rows1][C1][2]: second source of a channel concat, C1 = 0 for none) partial
 * rows of images of HW pixels -> scale [N][C0 + C1] = rstd * gamma, shift [N][C0 + C1] = beta - mean * rstd * gamma.  C0 % 8 == 0, (C0 + C1) % 8 == 0. */
int sdm_op_gn_partials(sdm_ctx* ctx, const float* st0, int rows0, const float* st1, int rows1, int C0, int C1, int N, int HW, int groups,
                       const float* gamma, const float* beta, float eps, float* scale, float* shift);
/* Test hook: the stand-alone GroupNorm statistics (gn_stats_kernel + gn_finalize_kernel) alone.  x0 [N][HW][C0] (+ x1 [N][HW][C1], C1 = 0 for none), fp32
 * (in_f32) or fp16 -> the same tables as sdm_op_gn_partials.  C0 % 8 == 0, (C0 + C1) % 8 == 0. */
int sdm_op_gn_tables(sdm_ctx* ctx, const void* x0, const void* x1, int C0, int C1, int in_f32, int N, int HW, int groups, const float* gamma,
                     const float* beta, float eps, float* scale, float* shift);
/* bench only (tools/gemm_p3_bench.py): ms per launch of the plane-fed GEMM on random operands; epi_flags = epilogue (0 fp32, 1 GEGLU, 2 q|k|v planes, 3 planes,
 * 4 fp32 + statistics) | 256 for an fp32 residual */
float sdm_bench_gemm_p3(sdm_ctx* ctx, long M, int K, int O, int epi_flags, int iters);
/* Plane-fed GEMM of the transformer blocks' Linear layers (k_gemm.h; reference call sites replace.py:232-362 -> diffusers BasicTransformerBlock) as a
 * stand-alone operator.  x: fp32 [N*H*W][K] on the device, K % 32 == 0; converted to the kernel's operand planes by the conversion kernel or, when
 * ln_gamma != NULL, by LayerNorm(eps) with plane output.  w: fp32 [O][K], packed exactly as a model layer.  mode 0: fp32 [rows][O] (+bias, +fp32 residual);
 * 1: GEGLU, O = 2 x outputs, result planes decoded to fp32 [rows][O/2]; 3: linear (+residual) to planes, decoded to fp32; 2: the raw q | k | v operand planes of
 * the attention cores (fp16 [rows][O], then the e5m2 pair plane of the same size; pair plane for channels < lo_cols only); 4: mode 0 + the per-(image, row
 * block, channel) {sum, sumsq} rows of the consumer's GroupNorm into `stats` ([N][*srows][O][2] floats; size it for 2 * ceil(H*W / 64) rows). */
int sdm_op_gemm_p3(sdm_ctx* ctx, const float* x, int N, int H, int W, int K, const float* w, const float* bias, int O, int mode, const float* res,
                   const float* ln_gamma, const float* ln_beta, float ln_eps, int lo_cols, void* out, float* stats, int* srows);
/* Test hook: Upsample2D (nearest x2 + 3x3 conv, split precision) on x fp32 NHWC [N][H][W][C] with the consumer's GroupNorm statistics, as the model's
 * up-sampling layers run it: out fp32 [N][2H][2W][O], stats [N][*srows][O][2] partial {sum, sumsq} rows (room for 8 * ceil((H + 2)(W + 2) / 64) + 4 * ceil(H / 2) * ceil(W / 4)
 * rows per image).  C % 32 == 0, O % 32 == 0.  Takes the phase path where the model would (option conv_up_phase: 1 by launch size, 2 always, 0 never: the 3x3 kernels). */
int sdm_op_conv_up_stats(sdm_ctx* ctx, const float* x, int N, int H, int W, int C, const float* w, const float* bias, int O, float* out, float* stats,
                         int* srows);
/* Test hooks for the exact algebraic folds done at load time (cross-attention K|V fold of aux_conv_in, logit scale in to_q,
 * time/opacity/bbox embedding constants in the conv1 bias tables): run one packed layer by name on an fp32 NHWC input
 * (DEVICE pointers; channel count = the layer's padded input channels), and read one folded bias row (HOST output). */
/* Test hook: class plane ([N][Hin][Win] bytes on the device; 0 = nothing known, 1..4 = region class) of the input of the NEXT sdm_op_conv_ex call.  The conv
 * then treats its input as the VAE encoder treats the trimap images ("constant tiles"): output tiles inside one region are filled, not multiplied. */
int sdm_debug_set_input_cmask(sdm_ctx* ctx, const unsigned char* mask);
int sdm_debug_run_layer(sdm_ctx* ctx, const char* layer_name, const float* x_nhwc, int N, int H, int W, float* out_nhwc, int Cout);
int sdm_debug_temb_row(sdm_ctx* ctx, int temb_index, int is_trans, const float* coords4, float* out_host, int cout);
/* Bench/ablation helper: ms per launch of one conv (random-ish data), HIP-event timed on the engine stream. */
/* (qt: 2 split-precision, 4 eight-wave blocks, 8 P.V on plain fp16, 16 the d = 64 ping-pong kernel, 32 without s_setprio, 64 the d = 512 kernel, 256 with 64: its
 * ping-pong form; ablate: the kernel's compile-time ABL mask) */
float sdm_bench_attn(sdm_ctx* ctx, int B, int heads, int Lq, int Lk, int qt, int ablate, int iters);
float sdm_bench_conv(sdm_ctx* ctx, int N, int H, int W, int Cin, int Cout, int ntaps, int stride, int in_f32, int tile_cfg, int ablate, int iters);
/* GroupNorm(groups)+optional SiLU over NHWC (concat of two sources) -> fp16 NHWC. */
int sdm_op_groupnorm(sdm_ctx* ctx, const void* in0, const void* in1, int C0, int C1, int in_f32, int N, int HW, int groups,
                     const float* gamma, const float* beta, float eps, int silu, void* out_f16);
/* LayerNorm over the last dim C of [rows, C] -> fp16. */
int sdm_op_layernorm(sdm_ctx* ctx, const void* x, int in_f32, long rows, int C, const float* gamma, const float* beta,
                     float eps, void* out_f16);
/* softmax(q k^T * scale + bias) v per (batch, head): q [B,Lq,heads*D], k,v [B,Lk,heads*D] fp16 with row
 * strides ldq/ldk/ldv, bias fp32 [B,Lk] or NULL (natural-log domain, as in the reference), out [B,Lq,heads*D].
 * D = 64 (any heads) or 512 (heads = 1).  With a bias (D = 64), 64-key tiles in which every key's bias lies more than
 * 2000*ln(2) below the image's largest bias are not loaded: their probabilities underflow to exactly 0 in fp32, as they do in
 * the reference's softmax (trimap keys carry (1-m)*-10000, replace.py:401-403).  The result is bit-identical to walking
 * every tile; the engine option attn_dense = 1 disables the skip. */
int sdm_op_attention(sdm_ctx* ctx, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* bias,
                     int B, int heads, int Lq, int Lk, int D, void* out, int ldo);
/* Test hook: sdm_op_attention without a bias and with an fp32 result (out_f32 != 0; head dim 512 only): the d = 512 core as the precise-mode VAE runs it. */
int sdm_op_attention_ex(sdm_ctx* ctx, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int B, int heads, int Lq, int Lk, int D, int out_f32,
                        void* out, int ldo);
/* Split-precision attention cores (head dim 64) as the default precision runs them: contiguous fp32 q [B,Lq,heads*64], k / v [B,Lk,heads*64]
 * are split into the operand planes the engine's GEMM epilogues produce (fp16 high parts + e5m2 residual pairs for Q.K^T, fp16 V), the
 * logit scale goes into Q; fp32 output [B,Lq,heads*64].  Test hook for the kernel the engine runs. */
int sdm_op_attention_split(sdm_ctx* ctx, const float* q, const float* k, const float* v, const float* bias, int B, int heads, int Lq, int Lk, float* out);
/* The same with the engine's other inputs and outputs.  tiles (needs bias; NULL: built from the bias as above): the active key tiles per image in the
 * engine's layout, int [B][ceil(Lk/64) + 1] on the device = count, then the ascending 64-key tile indices.  out_p3: 0 fp32 output as above; 1 the
 * kernels write the P3 operand planes of the GEMM that consumes the result (as the engine's transformer blocks run them; Lq % 32 == 0); 2 the fp32
 * result converted to P3 by to_p3_kernel (the reference of 1).  With out_p3 != 0 `out` receives the planes decoded to fp32 by from_p3_kernel and, if
 * planes != NULL, the raw planes (ceil(B*Lq/32)*32 * heads*64 * 3 bytes: fp16 hi plane, then the e5m2 xl plane). */
int sdm_op_attention_split_ex(sdm_ctx* ctx, const float* q, const float* k, const float* v, const float* bias, const int* tiles, int B, int heads, int Lq,
                              int Lk, int out_p3, float* out, void* planes);
/* Test hooks of the shared cross-attention operand.  sdm_op_cross_patch_planes: the key / value operand of every cross-attention of a forward
 * from the U-Net input tensor uin fp32 [B][H][W][16] (DEVICE; the trimap latent at channels 4..7) - k_hi [B][H*W][64] fp16 (the 3x3 patch matrix, 36 live columns),
 * k_pair the same number of bytes (its e5m2 pair plane), vt [B][64][rup(H*W, 64)] fp16 (k_hi transposed, zero filled).  sdm_op_attention_shared:
 * sdm_op_attention_split on ONE ks / vs fp32 [B,Lk,64] for every head (head stride 0, no transpose inside the operator); q_prescaled != 0: the logit scale
 * is in q already.  sdm_debug_cross_attention: the cross-attention of one transformer block of the loaded model ("unet.mid_block.attentions.0", ...) under the
 * current options, from the normalised hidden state x fp32 [B][H][W][C] and the U-Net input uin fp32 [B][h][w][16] to to_out(attention) (no residual). */
int sdm_op_cross_patch_planes(sdm_ctx* ctx, const float* uin, int B, int H, int W, void* k_hi, void* k_pair, void* vt);
/* ... ones_rows != 0: the operand as the engine builds it under the option cross_narrow - 1.0 in vt rows 59 and 63 for the key columns < H*W. */
int sdm_op_cross_patch_planes_ex(sdm_ctx* ctx, const float* uin, int B, int H, int W, void* k_hi, void* k_pair, void* vt, int ones_rows);
int sdm_op_attention_shared(sdm_ctx* ctx, const float* q, const float* ks, const float* vs, int B, int heads, int Lq, int Lk, int q_prescaled, float* out);
int sdm_debug_cross_attention(sdm_ctx* ctx, const char* block, const float* x, int B, int H, int W, const float* uin, int h, int w, float* out);
/* Test hook: the attention core of a cross-attention on the engine's own shared operand for any number of heads - q fp32 [B][Lq][heads*64] (pre-scaled, columns
 * 36..63 of every head zero) attends to the planes built from uin fp32 [B][h][w][16] under the current options (cross_narrow) -> fp32 [B][Lq][heads*64]. */
int sdm_op_cross_core(sdm_ctx* ctx, const float* q, const float* uin, int B, int heads, int Lq, int h, int w, float* out);
/* Test hook: the launch the attention operator would make for these shapes and flags under the current options, on a device of `cus` compute units:
 * the launch-counter name of the kernel (see sdm_kernel_counts) into kernel[cap] and the key split into *nsplit (1 = unsplit).  prec as in the engine:
 * 0 fp16 operands, 1 fp16 hi | lo planes, 2 fp16 + e5m2 pair planes (the default precision); has_bias / has_tiles: a key bias / a caller's tile list
 * comes with the call.  Touches neither a GPU nor an engine.  D = 64, or 512 with one head and prec 0. */
int sdm_debug_attn_plan(int B, int heads, int Lq, int Lk, int D, int prec, int out_f32, int has_bias, int has_tiles, int cus, char* kernel, int cap,
                        int* nsplit);
/* Antialiased bilinear resize of fp32 planes [P, Hin, Win] -> [P, Hout, Wout] (torchvision Resize). */
int sdm_op_resize_aa(sdm_ctx* ctx, const float* in, int P, int Hin, int Win, float* out, int Hout, int Wout);
/* Level-k additive key bias (natural-log domain) from the [-1,1] trimap plane [B,S,S] -> [B,(S/8>>k)^2]. */
int sdm_op_mask_bias(sdm_ctx* ctx, const float* trimap_plane, int B, int S, int level, float* bias_out);
/* Test hooks of the patch token order of the U-Net transformers (engine option attn_patch_tokens): inside a transformer of a level whose
 * latent H x W is whole 8x8 patches and at least 64 wide, token ((y>>3)*(W>>3) + (x>>3))*64 + (y&7)*8 + (x&7) is pixel (y, x) of its image.
 * sdm_debug_patch_token_map: the helper pair the kernels use, for one image (HOST arrays of H*W ints); returns 1 if H x W takes the order, 0 (identity maps) if not.
 * sdm_op_groupnorm_p3: the way in - GroupNorm of x fp32 [N][H][W][C] (DEVICE, C % 32 == 0) as the operand planes of proj_in (ceil(N*H*W/32)*32 * C * 3 bytes
 * each: fp16 hi plane, then the e5m2 xl plane), in row-major order into planes_rows and / or with row t of an image = token t into planes_tokens (either may be
 * NULL), both from one statistics pass.
 * sdm_op_gemm_p3_tokens: the way out - sdm_op_gemm_p3 mode 0 / 4 where the rows of x are tokens and out / res are pixel-order [N][H][W][O]; patch_tokens = 0:
 * the plain launch.  sdm_op_mask_bias_tokens: the key bias of a level as the U-Net passes it to its self-attentions (log2 domain, rectangles allowed), in patch
 * order where patch_tokens != 0 and the level takes it; returns the order written (1 / 0).  sdm_op_active_tiles: the engine's list of active 64-key tiles of a
 * bias [B][Lk] (DEVICE) -> int [B][ceil(Lk/64) + 1] (DEVICE): count, then the ascending tile indices. */
int sdm_debug_patch_token_map(int H, int W, int32_t* token_of_pixel, int32_t* pixel_of_token);
int sdm_op_groupnorm_p3(sdm_ctx* ctx, const float* x, int N, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, int silu,
                        void* planes_rows, void* planes_tokens);
int sdm_op_gemm_p3_tokens(sdm_ctx* ctx, const float* x, int N, int H, int W, int K, const float* w, const float* bias, int O, int mode, const float* res,
                          int patch_tokens, float* out, float* stats, int* srows);
int sdm_op_mask_bias_tokens(sdm_ctx* ctx, const float* trimap_plane, int B, int SH, int SW, int level, int patch_tokens, float* bias_out);
int sdm_op_active_tiles(sdm_ctx* ctx, const float* bias, int B, int Lk, int32_t* tiles);

#ifdef __cplusplus
}
#endif
#endif /* SDMATTE_H_ */

/*
 * vstab.h -- C ABI of libvstab_hip.so: FlowNetS-pyramid optical-flow inference and
 * bilinear flow warp for MI355X (gfx950), hand-written HIP kernels.
 *
 * The reference (posgraph/coupe.optical_flow_based_deep_video_stabilization) is pure
 * Python on TensorFlow 1.10 + TensorLayer and has no FFI of its own: its boundary for
 * this path is the pair of Python graph-builder calls
 *     flownetS_pyramid(feats, batch_size, is_train, reuse, scope)      model.py:786-893
 *     tf_warp(img, flow, H, W) / get_pixel_value(img, x, y)            main:70-130 / 44-68
 * ("main" = main_flownetS_pyramid_noprevloss_dataloader.py) plus the glue lines
 * main:497-498 and main:806 and the checkpoint restore main:520.  Each entry point below
 * cites the reference lines it replaces; INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all tensors fp32, NHWC, contiguous, DEVICE pointers unless a parameter says "host";
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream); no hidden host<->device copies, no allocation after vstab_load_weights;
 *   - the caller owns every I/O buffer and the workspace; the context owns only the
 *     packed weights (everything a forward writes -- activations, split-K slabs, the ticket
 *     words of the in-launch reductions -- lies in the caller's workspace);
 *   - every function returns 0 or a negative VSTAB_E_* code and never throws;
 *     vstab_last_error() gives the message for the last failure on that context
 *     (or the last context-less failure when ctx == NULL);
 *   - one context per device; forwards on one context may overlap in time (different
 *     streams, also issued from different host threads) when each uses its OWN workspace:
 *     a successful forward only reads the context (a failing one writes its message under a
 *     lock; with two threads failing at once vstab_last_error(ctx) is either message, and
 *     vstab_last_error(NULL) is always the calling thread's own).  Calls that write the
 *     context (vstab_load_weights, vstab_set_plan_batch, the DIAGNOSTIC section at the end
 *     of this header -- vstab_profile_enable(ctx, 1) makes every forward write its event
 *     and name slots) must not overlap with anything on that context;
 *   - product surface first; everything under "DIAGNOSTIC AND TEST SURFACE" at the end
 *     (plan flags, per-launch profilers, roctx ranges, self-tests, host-only views of the
 *     launch plan) exists for measurements and tests, is process- or context-global state,
 *     and is not part of the drop-in contract.
 */
#ifndef VSTAB_H
#define VSTAB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSTAB_OK          0
#define VSTAB_E_SHAPE    -1   /* bad dimensions / unsupported size                      */
#define VSTAB_E_ALIGN    -2   /* pointer not 16-byte aligned where required             */
#define VSTAB_E_HIP      -3   /* a HIP runtime call or kernel launch failed             */
#define VSTAB_E_NOMEM    -4   /* workspace too small / allocation failed                */
#define VSTAB_E_WEIGHTS  -5   /* missing or mis-shaped variable in vstab_load_weights   */
#define VSTAB_E_STATE    -6   /* call order (e.g. forward before load_weights)          */

#if defined(__GNUC__)
#define VSTAB_API __attribute__((visibility("default")))
#else
#define VSTAB_API
#endif

typedef struct vstab_ctx vstab_ctx;

/* One named variable of the checkpoint, in the reference's own layout:
 * conv W [kh][kw][Cin][Cout], deconv W [kh][kw][Cout][Cin], vectors [C].
 * `name` is the short variable name ("1/W_conv2d", "deconv5_bn/beta",
 * "upsample6_5/W_deconv2d", ... = the tensorlayer key without the
 * "main_net/flownetS/" prefix and ":0" suffix).  `data` is a HOST pointer. */
typedef struct vstab_tensor {
    const char  *name;
    const float *data;
    int32_t      ndim;
    int32_t      shape[4];
} vstab_tensor;

/* A tensor living in the forward workspace (for tests / debugging). */
typedef struct vstab_ws_entry {
    char    name[24];
    int64_t offset_bytes;
    int32_t n, h, w, c;      /* logical NHWC shape                           */
    int32_t c_stride;        /* floats between consecutive pixels (>= c)     */
} vstab_ws_entry;

/* ---- context ------------------------------------------------------------------- */
VSTAB_API int  vstab_create(vstab_ctx **out, int device);
VSTAB_API void vstab_destroy(vstab_ctx *ctx);
VSTAB_API const char *vstab_last_error(const vstab_ctx *ctx);
VSTAB_API const char *vstab_version(void);

/* Replaces tl.files.load_and_assign_npz_dict (main:520) + the variable creation inside
 * flownetS_pyramid: validates every variable of the graph, folds inference BatchNorm
 * (no gamma, eps 1e-5; model.py:809) into W and b, packs the weights into the MFMA
 * operand layout and uploads them.  Synchronous.  Input channels = shape[2] of
 * "1/W_conv2d" (27 in the reference). */
VSTAB_API int vstab_load_weights(vstab_ctx *ctx, const vstab_tensor *tensors, int count);

/* Bytes of workspace vstab_flownets_forward needs for this problem (0 on bad shape).  No
 * single tensor may reach 2 GiB (32-bit buffer offsets): larger batches are processed in
 * chunks of the largest batch that fits, and the workspace is sized for one chunk. */
VSTAB_API size_t vstab_workspace_bytes(int B, int H, int W, int Cin);

/* ---- pinned launch plans.  The forward takes a few per-layer decisions that change the ORDER of a sample's floating-point sums:
 * split-K factors, Winograd or direct form of the 3x3 stride-1 stages, weight-stream or tiled kernel for few-row layers.  By default
 * they are taken for the batch of each call, so the same sample can come out a few ulp different when it is batched differently (a
 * ragged last micro-batch of a sharded clip: main:553-558's samples are independent).  vstab_set_plan_batch(ctx, P)
 * pins them to what a batch of P samples gets: every call with B <= P then gives each sample bit-identical results, whatever B is
 * (B > P is VSTAB_E_SHAPE).  P = 0 (default) unpins.  The workspace of a pinned context is sized by vstab_workspace_bytes_ctx
 * (a workspace sized for P itself always suffices); vstab_workspace_bytes / vstab_workspace_layout describe the UNPINNED plan. */
VSTAB_API int vstab_set_plan_batch(vstab_ctx *ctx, int batch);
VSTAB_API size_t vstab_workspace_bytes_ctx(const vstab_ctx *ctx, int B, int H, int W, int Cin);

/* Names/offsets of the intermediate tensors inside the workspace.  Returns the number
 * of entries written (<= max_entries) or a negative error. */
VSTAB_API int vstab_workspace_layout(int B, int H, int W, int Cin, vstab_ws_entry *entries, int max_entries);
/* The same for the plan THIS context would run (its pinned batch and plan flags): the activation offsets depend on the shape alone,
 * the sizes of "splitk", "winograd_in", "winograd_out" (always the last three entries) on the plan. */
VSTAB_API int vstab_workspace_layout_ctx(const vstab_ctx *ctx, int B, int H, int W, int Cin, vstab_ws_entry *entries, int max_entries);

/* ---- the network: flownetS_pyramid(feats, batch_size, is_train=False) model.py:786-893
 * feats [B,H,W,Cin] -> predict_flow6..3 at the pyramid levels and predict_flow2
 * [B,H-2,W-2,2] (the 'flow' key is the same tensor).  The 384x512 literals of the
 * reference are generalised by SURVEY.md 8a-note-1.  `workspace` must be 256-byte
 * aligned and at least vstab_workspace_bytes() long. */
VSTAB_API int vstab_flownets_forward(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin,
                           float *pf6, float *pf5, float *pf4, float *pf3, float *pf2,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- glue: main:497-498 with the literals generalised (384 -> net_h, 512 -> net_w, 382 -> h = the flow's height).
 * out[B,oh,ow,2] = resize_images(flow*net_h/h, [oh,ow]), then x = x*ow/net_w, y = y*oh/net_h, every `*` and `/`
 * a separate fp32 operation in the reference's order ((a*b)/c) (legacy TF bilinear, align_corners=False; identity
 * resample when the size already matches). */
VSTAB_API int vstab_flow_resize_scale(const float *flow, int B, int h, int w, float *out, int oh, int ow,
                            int net_h, int net_w, void *stream);

/* ---- glue: main:806 / model.py:857 UpSampling2dLayer defaults.  Legacy TF bilinear
 * resize of an NHWC tensor. */
VSTAB_API int vstab_resize_bilinear(const float *x, int B, int h, int w, int C, float *out, int oh, int ow,
                          void *stream);

/* ---- main:806 without an intermediate copy: out [B,oh,ow,3] = tf.image.resize_images(x[..., c_off:c_off+3], [oh, ow]) for an
 * NHWC tensor x with Cs channels per pixel (the unstable frame is channels 24:27 of the 27-channel input stack).  Legacy
 * bilinear as vstab_resize_bilinear (bit-identical to it on a contiguous 3-channel copy).  out 16-byte aligned. */
VSTAB_API int vstab_resize_bilinear_slice3(const float *x, int B, int h, int w, int Cs, int c_off, float *out, int oh, int ow,
                                 void *stream);

/* ---- tf_warp(img, flow, H, W) main:70-130.  img [B,H,W,C], flow [B,H,W,2] (x, y),
 * out [B,H,W,C]; truncating corners, clipped indices, weights from the clipped corners. */
VSTAB_API int vstab_warp_flow(const float *img, const float *flow, float *out, int B, int H, int W, int C,
                    void *stream);

/* ---- main:497-514 as ONE launch (evaluate_originalSize builds them as one graph): outflow = the glue of
 * vstab_flow_resize_scale applied to flow [B,h,w,2], at [B,oh,ow,2]; warped = tf_warp(img [B,oh,ow,3], outflow).
 * `outflow` may be NULL when the caller does not need the output-resolution flow (it is then never written); when
 * given it is written once and not re-read.  Bit-identical to vstab_flow_resize_scale followed by vstab_warp_flow.
 * C must be 3; img/outflow/warped 16-byte aligned; B*oh*ow < 2^31. */
VSTAB_API int vstab_flow_glue_warp(const float *flow, int B, int h, int w, const float *img, float *outflow, float *warped,
                         int oh, int ow, int C, int net_h, int net_w, void *stream);

/* ---- evaluate_originalSize's graph (main:491-514) as ONE call: vstab_flownets_forward, then vstab_flow_glue_warp with the
 * constants of main:497-498 (net_h = H, net_w = W, the flow's height H-2) on a 3-channel frame [B,oh,ow,3].  Every
 * output buffer is the caller's (pre-allocated once, re-used every step): a step is one call and no allocation.  `outflow` may
 * be NULL.  Same results as the two calls. */
VSTAB_API int vstab_stabilise_originalsize(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, const float *frame,
                                           int oh, int ow, float *pf6, float *pf5, float *pf4, float *pf3, float *pf2,
                                           float *outflow, float *warped, void *workspace, size_t workspace_bytes, void *stream);

/* ---- get_pixel_value(img, x, y) main:44-68.  x, y int32 [B,H,W] -> out[b,h,w,:] =
 * img[b, y, x, :].  Indices are clamped into the image instead of faulting. */
VSTAB_API int vstab_get_pixel_value(const float *img, const int32_t *x, const int32_t *y, float *out, int B,
                          int H, int W, int C, int Hi, int Wi, void *stream);

/* ---- backward of tf_warp, get_pixel_value and the flow glue: what TensorFlow's autodiff yields for them.
 * vstab_warp_flow_backward: dout [B,H,W,C] is the gradient of vstab_warp_flow's output.  tf_warp's corner indices come from integer
 * casts and carry no gradient, so the flow enters through the four bilinear weights only:
 *   d_flow [B,H,W,2]: d_fx = sum_c dout_c [(y1f-y)(Ic-Ia) + (y-y0f)(Id-Ib)]_c, d_fy = sum_c dout_c [(x1f-x)(Ib-Ia) + (x-x0f)(Id-Ic)]_c
 *     with the CLIPPED corners (exactly 0 along an axis whose corners clip to one border pixel).  Plain stores, one thread per
 *     pixel: bit-reproducible.
 *   d_img [B,H,W,C]: the gather's adjoint with the forward's weights, added by fp32 atomics -- its last bits depend on the order
 *     in which the contributions arrive.  Zeroed first unless accumulate_img.
 * Either of d_img / d_flow may be NULL (that gradient's work is skipped; d_flow alone needs neither atomics nor the memset).  A NaN,
 * infinite or huge flow stays in bounds (its taps are border pixels), as in the forward.  flow / d_flow 8-byte aligned.
 * vstab_get_pixel_value_backward: dout[b,h,w,:] added to d_img[b, clip(y), clip(x), :] (the forward's clipping) by fp32 atomics;
 * d_img [B,Hi,Wi,C] zeroed first unless `accumulate`.
 * vstab_flow_resize_scale_backward: the adjoint of vstab_flow_resize_scale, d_flow [B,h,w,2] = gain_c * resize^T(dout [B,oh,ow,2])
 * with gain_x = (net_h/h)(ow/net_w), gain_y = (net_h/h)(oh/net_h).  A gather in a fixed order, no atomics: bit-reproducible.
 * VSTAB_E_STATE for a NULL buffer; VSTAB_E_SHAPE for a dimension < 1, H*W >= 2^31 (the glue: B > 65535 or h*w*2 >= 2^31) or
 * d_img and d_flow both NULL (as the other samplers' backwards answer it); VSTAB_E_ALIGN for a misaligned flow / d_flow. */
VSTAB_API int vstab_warp_flow_backward(const float *img, const float *flow, const float *dout, int B, int H, int W, int C,
                                       float *d_img, float *d_flow, int accumulate_img, void *stream);
VSTAB_API int vstab_get_pixel_value_backward(const float *dout, const int32_t *x, const int32_t *y, float *d_img, int B, int H, int W,
                                             int C, int Hi, int Wi, int accumulate, void *stream);
VSTAB_API int vstab_flow_resize_scale_backward(const float *dout, int B, int oh, int ow, float *d_flow, int h, int w, int net_h,
                                               int net_w, void *stream);

/* ---- secondary samplers named by north_star (never executed by the reference's live scripts) ---- */
/* AffineTransformer.transform / ProjectiveTransformer.transform / transformer()
 * (spatial_transformer.py:400-452, 539-608, 34-38): theta [B,6] or [B,8] (theta_dim = 6 | 8; the
 * projective 3x3 gets a trailing 1), sampling grid linspace(-1,1) of the OUTPUT size, bilinear_interp
 * sampler with a 1-pixel zero border.  img [B,H,W,C] -> out [B,oh,ow,C]. */
VSTAB_API int vstab_st_transform(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim,
                                 float *out, int oh, int ow, void *stream);
/* bilinear_interp(im, x, y, out_size) / _interpolate (spatial_transformer.py:902-964, 787-792): x, y flat
 * [B*oh*ow] normalised to [-1,1], out_size = (oh, ow) as the reference passes it; out [B*oh*ow, C]. */
VSTAB_API int vstab_st_bilinear_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                       int oh, int ow, float *out, void *stream);
/* _meshgrid(out_size) (spatial_transformer.py:755-779): out[3*oh*ow] = x_t row, y_t row, ones. */
VSTAB_API int vstab_st_meshgrid(float *out, int oh, int ow, void *stream);
/* ---- the rest of spatial_transformer.py's 2-D samplers (bicubic, symmetric-pad transformers, thin-plate spline).  Shapes as in
 * the entry points above; B <= 65535; VSTAB_E_SHAPE for anything outside the contract. */
#define VSTAB_INTERP_BILINEAR 0
#define VSTAB_INTERP_BICUBIC  1
#define VSTAB_SYM_AFFINE      0   /* AffineSymmetryTransformer      ST:454-517, theta [B,6] */
#define VSTAB_SYM_PROJECTIVE  1   /* ProjectiveSymmetryTransformer  ST:611-716, theta [B,8] */
#define VSTAB_SYM_SIMILARITY  2   /* SimilarityTransformer          ST:311-371, theta [B,4] */
#define VSTAB_TPS_GMAX       16   /* ElasticTransformer: at most 16 x 16 control points */
/* bicubic_interp(im, x, y, out_size) (ST:966-1072): x, y flat [B*oh*ow] clipped to [-1,1] (NaN -> -1), 4x4 taps with edges
 * replicated (no zero border), alpha = -0.75; out [B*oh*ow, C]. */
VSTAB_API int vstab_st_bicubic_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y, int oh, int ow,
                                      float *out, void *stream);
/* vstab_st_transform with a choice of sampler: VSTAB_INTERP_BILINEAR is vstab_st_transform itself (bit-equal),
 * VSTAB_INTERP_BICUBIC samples with bicubic_interp.  out [B,oh,ow,C]. */
VSTAB_API int vstab_st_transform_interp(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim, int interp,
                                        float *out, int oh, int ow, void *stream);
/* The symmetric-pad transformers' .transform: the image padded by 100 px per side in SYMMETRIC mode (H, W >= 100; never
 * materialised), sampled on the linspace grid of (oh+200) x (ow+200) points, then resize_image_with_crop_or_pad(out, ow, oh):
 * out [B,ow,oh,C] (height and width swapped, as the reference has them).  kind VSTAB_SYM_*. */
VSTAB_API int vstab_st_symmetry_transform(const float *img, int B, int H, int W, int C, const float *theta, int kind, int interp,
                                          float *out, int oh, int ow, void *stream);
/* Host only: ElasticTransformer's transpose(L_inv[:,3:]) for a g x g control grid (ST:187-225), inverted in double and rounded
 * to fp32: linv_t [g*g, g*g+3] (cap floats available).  2 <= g <= VSTAB_TPS_GMAX (g = 1 makes L singular). */
VSTAB_API int vstab_host_tps_linv(int g, float *linv_t, int cap);
/* ElasticTransformer.transform (ST:84-158): theta [B, 2*g*g] control-point offsets (x block then y block), linv_t (device) from
 * vstab_host_tps_linv; the thin-plate spline maps the linspace grid of (oh, ow) to source coordinates.  out [B,oh,ow,C]. */
VSTAB_API int vstab_st_elastic_transform(const float *img, int B, int H, int W, int C, const float *theta, int g, const float *linv_t,
                                         int interp, float *out, int oh, int ow, void *stream);
/* ---- backward of the BILINEAR sampler: vstab_st_transform (affine and projective) and vstab_st_bilinear_interp.  These two are the
 * differentiable samplers besides the thin-plate spline, the symmetric-pad transformers and the homography warps (further down);
 * the bicubic sampler's backward (vstab_st_bicubic_interp_backward and the _interp_backward entry points) follows these two.
 * What TensorFlow's autodiff gives for ST:902-964 / 438-452 / 578-608: floor and the casts have zero derivative, the clip passes the
 * gradient where -1 <= x <= W inclusive (0 outside and for NaN), taps on the zero border receive nothing; coordinates and taps are
 * the forward's fp32 values.  img, B, H, W, C, theta | x, y, oh, ow as in the forward (B <= 65535, B*H*W*C < 2^31);
 * dout [B,oh,ow,C] the gradient of the output.
 *   d_img   [B,H,W,C] (nullable): zero-filled on `stream` by the call itself when accumulate == 0, added into when accumulate == 1.
 *           Summed by float atomics: its last bits DEPEND ON ATOMIC ARRIVAL ORDER and may differ between two runs.
 *   d_theta [B,theta_dim] (nullable; the projective 3x3's constant ninth entry has no gradient): overwritten; the sum over pixels is
 *           taken in double in a fixed order -- two runs on the same inputs are bit-equal.  Needs
 *           vstab_st_transform_backward_workspace_bytes() of 8-byte aligned workspace (VSTAB_E_NOMEM when too small; not read when
 *           d_theta is NULL); the call makes no allocation.
 *   d_x, d_y [B*oh*ow] (each nullable): overwritten, reproducible.
 * A NULL output skips that gradient's work; all outputs NULL is VSTAB_E_SHAPE. */
VSTAB_API size_t vstab_st_transform_backward_workspace_bytes(int B, int H, int W, int C, int oh, int ow);
VSTAB_API int vstab_st_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim,
                                          const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                          void *workspace, size_t workspace_bytes, void *stream);
VSTAB_API int vstab_st_bilinear_interp_backward(const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                                const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_x,
                                                float *d_y, void *stream);
/* ---- backward of the BICUBIC sampler, and the backwards above and below with a choice of sampler.  What TensorFlow's autodiff gives
 * for bicubic_interp (ST:966-1072), out_c = sum_i sum_j wy_i wx_j I[ys_i, xs_j, c]: taps and weights are the forward's (every floor, clip
 * and edge decision is shared); floor and the casts have zero derivative, so the weights' derivatives w'_i = c_i1 + 2 c_i2 t + 3 c_i3 t^2
 * carry d x, d y; the clip to [-1,1] passes the gradient where -1 <= x <= 1 INCLUSIVE, 0 outside and for NaN (which the forward
 * reads as -1) -- the convention of the bilinear clip above.
 *   d_img   by float atomics like the bilinear one (last bits depend on arrival order): wy_i wx_j dout added to each of the 16 taps; at
 *           the image edge the replicate-clamp folds several taps onto one pixel and all of them add (there is no zero border).  The
 *           symmetric-pad kinds' taps are those of the padded extent mapped through the symmetric pad, as in the forward.
 *   d_theta, d_x, d_y  reproducible: d x, d y feed each source's existing chain, summed in double in a fixed order without atomics.
 * vstab_st_bicubic_interp_backward is vstab_st_bilinear_interp_backward for bicubic_interp.  The three _interp_backward entry points
 * take `interp` (VSTAB_INTERP_*; anything else is VSTAB_E_SHAPE) after theta_dim | kind | linv_t; with VSTAB_INTERP_BILINEAR each IS
 * the entry point without _interp (d_theta bit-equal).  Nullable outputs, accumulate, limits (B <= 65535, B*H*W*C < 2^31), error
 * codes and the order of the checks are those of the bilinear backwards, and the existing *_backward_workspace_bytes functions serve
 * both samplers: the partial-row workspace does not depend on the sampler. */
VSTAB_API int vstab_st_bicubic_interp_backward(const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                               const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_x, float *d_y,
                                               void *stream);
VSTAB_API int vstab_st_transform_interp_backward(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim, int interp,
                                                 const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                                 void *workspace, size_t workspace_bytes, void *stream);
VSTAB_API int vstab_st_symmetry_transform_interp_backward(const float *img, int B, int H, int W, int C, const float *theta, int kind,
                                                          int interp, const float *dout, int oh, int ow, float *d_img, int accumulate,
                                                          float *d_theta, void *workspace, size_t workspace_bytes, void *stream);
VSTAB_API int vstab_st_elastic_transform_interp_backward(const float *img, int B, int H, int W, int C, const float *theta, int g,
                                                         const float *linv_t, int interp, const float *dout, int oh, int ow, float *d_img,
                                                         int accumulate, float *d_theta, void *workspace, size_t workspace_bytes,
                                                         void *stream);
/* ---- ElasticTransformer (thin-plate spline): its source coordinates, and the backward of its BILINEAR sampler.  theta, g, linv_t,
 * oh, ow as in vstab_st_elastic_transform.
 * vstab_st_elastic_coords: x_out, y_out [B*oh*ow], the normalised source coordinates (x_s_flat, y_s_flat of ST:140-158) that
 * vstab_st_elastic_transform samples at, bit for bit: the same device code computes them.  Needs no image. */
VSTAB_API int vstab_st_elastic_coords(const float *theta, int B, int g, const float *linv_t, int oh, int ow, float *x_out, float *y_out,
                                      void *stream);
/* vstab_st_elastic_transform_backward: conventions, limits and error codes of vstab_st_transform_backward (d_img by float atomics, zero-
 * filled on `stream` when accumulate == 0; a NULL output skips that gradient's work, both NULL is VSTAB_E_SHAPE).
 *   d_theta [B, 2*g*g] (nullable): the gradient of the control-point offsets, x block then y block.  Nothing flows through
 *           U = r^2 ln r^2 (it depends on the grid alone); the 2 (g*g + 3) coefficient sums over the pixels and their product with
 *           linv_t are taken in double in a fixed order, without atomics -- two runs are bit-equal -- and rounded to fp32 once.
 *   workspace: vstab_st_elastic_transform_backward_workspace_bytes(), 8-byte aligned; VSTAB_E_NOMEM when too small, not read when
 *           d_theta is NULL.  Its size is B * wps * 2 (g*g + 3) * 8 bytes, wps = min(steps, max(16, 1024 / B)) workgroups walking
 *           each sample, steps = the sample's 16 x 32 output tiles (C == 3) or runs of 256 output pixels: bounded by
 *           max(1024, 16 B) rows whatever the frame size (about 4 MiB at g = 16 up to B = 64).  0 for a shape outside the contract. */
VSTAB_API size_t vstab_st_elastic_transform_backward_workspace_bytes(int B, int H, int W, int C, int g, int oh, int ow);
VSTAB_API int vstab_st_elastic_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int g,
                                                  const float *linv_t, const float *dout, int oh, int ow, float *d_img, int accumulate,
                                                  float *d_theta, void *workspace, size_t workspace_bytes, void *stream);
/* ---- the symmetric-pad transformers (SimilarityTransformer, AffineSymmetryTransformer, ProjectiveSymmetryTransformer): what the
 * forward computes on the way, and the backward of their BILINEAR sampler.  theta, kind, oh, ow as in vstab_st_symmetry_transform.
 * vstab_st_symmetry_matrix: out [B,9], the pre-mapped row-major 3x3 matrices (affine kinds: last row 0 0 1), SimilarityTransformer's
 *   interleave across samples included.  vstab_st_symmetry_coords: x_out, y_out [B*ow*oh], the normalised source coordinates of every
 *   FINAL pixel (layout of the output, [B,ow,oh]) on the (H+200) x (W+200) padded extent; 0 where the crop-or-pad pads.  Both come from
 *   the device code the forward calls, bit for bit, and need no image. */
VSTAB_API int vstab_st_symmetry_matrix(const float *theta, int B, int kind, float *out, void *stream);
VSTAB_API int vstab_st_symmetry_coords(const float *theta, int B, int kind, int oh, int ow, float *x_out, float *y_out, void *stream);
/* vstab_st_symmetry_transform_backward: conventions, limits and error codes of vstab_st_transform_backward (d_img by float atomics, zero-
 * filled on `stream` when accumulate == 0; a NULL output skips that gradient's work, both NULL is VSTAB_E_SHAPE; B*H*W*C < 2^31) and
 * the forward's H, W >= 100.  What TensorFlow's autodiff gives for ST:311-371, 454-517, 611-716 with the bilinear sampler.
 *   dout    [B,ow,oh,C], the gradient of the forward's output.  A pixel that the crop-or-pad pads contributes nothing: its dout is
 *           not read into any sum.
 *   d_img   [B,H,W,C] (nullable): the adjoint of gather . symmetric-pad -- a tap at padded index p adds into image pixel
 *           refl(p - 100), several padded taps may fold onto one pixel; nothing for a tap on the zero border outside the padded extent.
 *   d_theta [B,6|8|4] (nullable): overwritten; the gradient of the pre-mapped matrix is summed over the pixels in double in a fixed
 *           order and taken through the pre-map in double, rounded to fp32 once -- two runs are bit-equal.  VSTAB_SYM_AFFINE: the
 *           pre-map multiplies by 0, so d_theta is exactly zero for finite gradients (a non-finite one propagates).
 *           VSTAB_SYM_PROJECTIVE divides by z as is (no safe_z): z == 0 propagates by IEEE rules.  VSTAB_SYM_SIMILARITY: through
 *           cos / sin and the interleave, which couples the samples of a batch for B > 1.
 *   workspace: vstab_st_symmetry_transform_backward_workspace_bytes(), 8-byte aligned; VSTAB_E_NOMEM when too small, not read when
 *           d_theta is NULL.  0 for a shape outside the contract. */
VSTAB_API size_t vstab_st_symmetry_transform_backward_workspace_bytes(int B, int H, int W, int C, int oh, int ow);
VSTAB_API int vstab_st_symmetry_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int kind,
                                                   const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                                   void *workspace, size_t workspace_bytes, void *stream);
/* ---- the 3-D volume transformer (spatial_transformer.py:227-308, 725-753, 794-899), forward and backward.  vol [B,D,H,W,C];
 * out_size = (od, oh, ow) = (depth, height, width) as the reference passes it.  One thread per output voxel, any C; a workgroup
 * owns a VSTAB_ST3D_BRICK_Z x _Y x _X brick of one sample's output.  64-bit element offsets: the limits are B <= 65535, every
 * extent (plus 2 * edge_size) <= 2^24 (fp32 holds the indices exactly), at most 2^40 elements per tensor, and a launch grid of
 * B * bricks < 2^31; anything else is VSTAB_E_SHAPE, checked before the pointers are looked at. */
#ifndef VSTAB_ST3D_BRICK_Z            /* a measurement build may choose another brick */
#define VSTAB_ST3D_BRICK_Z 2
#define VSTAB_ST3D_BRICK_Y 8
#define VSTAB_ST3D_BRICK_X 16
#endif
/* _meshgrid3d(out_size) (ST:725-753): out[4*od*oh*ow] = x_t row, y_t row, z_t row, ones; x fastest, z slowest. */
VSTAB_API int vstab_st3d_meshgrid(float *out, int od, int oh, int ow, void *stream);
/* bilinear_interp3d(vol, x, y, z, out_size, edge_size) / _interpolate3d (ST:794-899): x, y, z flat [B*od*oh*ow] normalised to
 * [-1,1]; per axis v = (v+1)/2*(n-1) clipped to [-e, n-1+e] (NaN reads as -e) against a volume zero-padded by e = edge_size >= 0
 * voxels (never materialised); weights (wz*wy)*wx, the eight products summed in the order 000 ... 111 (x last).  out [B*od*oh*ow, C]. */
VSTAB_API int vstab_st3d_bilinear_interp(const float *vol, int B, int D, int H, int W, int C, const float *x, const float *y,
                                         const float *z, int od, int oh, int ow, int edge_size, float *out, void *stream);
/* AffineVolumeTransformer.transform (ST:252-308): theta [B,12] = row-major 3x4 acting on (x_t, y_t, z_t, 1) of the linspace(-1,1)
 * grid of the OUTPUT size, ((t0 x + t1 y) + t2 z) + t3 with every product and sum rounded to fp32; edge_size = 1.
 * out [B,od,oh,ow,C]. */
VSTAB_API int vstab_st3d_transform(const float *vol, int B, int D, int H, int W, int C, const float *theta, float *out, int od,
                                   int oh, int ow, void *stream);
/* Backward of the two, what TensorFlow's autodiff gives: floor and the casts have zero derivative, the clip passes the gradient where
 * -e <= v <= n-1+e inclusive (0 outside and for NaN), chain factor (n-1)/2 per axis, taps on the pad receive nothing; coordinates
 * and taps are the forward's fp32 values.  dout [B,od,oh,ow,C].
 *   d_vol   [B,D,H,W,C] (nullable): zero-filled on `stream` by the call when accumulate == 0, added into when accumulate == 1.
 *           Eight float atomics per voxel-channel: its last bits DEPEND ON ATOMIC ARRIVAL ORDER and may differ between two runs.
 *   d_theta [B,12] (nullable): overwritten; summed in double in a fixed order -- two runs are bit-equal.  Needs
 *           vstab_st3d_transform_backward_workspace_bytes() of 8-byte aligned workspace (VSTAB_E_NOMEM when too small; not read
 *           when d_theta is NULL); the call makes no allocation.
 *   dx, dy, dz [B*od*oh*ow] (each nullable): overwritten, reproducible.
 * A NULL output skips that gradient's work; all outputs NULL is VSTAB_E_SHAPE. */
VSTAB_API size_t vstab_st3d_transform_backward_workspace_bytes(int B, int D, int H, int W, int C, int od, int oh, int ow);
VSTAB_API int vstab_st3d_transform_backward(const float *vol, int B, int D, int H, int W, int C, const float *theta, const float *dout,
                                            int od, int oh, int ow, float *d_vol, int accumulate, float *d_theta, void *workspace,
                                            size_t workspace_bytes, void *stream);
VSTAB_API int vstab_st3d_bilinear_interp_backward(const float *vol, int B, int D, int H, int W, int C, const float *x, const float *y,
                                                  const float *z, int od, int oh, int ow, int edge_size, const float *dout,
                                                  float *d_vol, int accumulate, float *dx, float *dy, float *dz, void *stream);
/* warp.transformImage / transformCropImage (warp.py:46-86, 89-129): M [B,9] = refMtrx . pMtrx maps the canonical
 * linspace(-1,1) grid of the OUTPUT size to source pixel coordinates; floor/ceil taps, zero outside. */
VSTAB_API int vstab_homography_warp(const float *img, int B, int Hi, int Wi, int C, const float *M, float *out, int oh,
                                    int ow, void *stream);
/* The same with the composition warp.py:48-49 makes in front of it (tf.matmul(refMtrx, pMtrx)) done by the kernel: ref [9] (device,
 * one matrix for the batch), pM [B,9]; M = ref . pM with every product and sum rounded to fp32, (r0*p0 + r1*p1) + r2*p2. */
VSTAB_API int vstab_transform_image(const float *img, int B, int Hi, int Wi, int C, const float *ref, const float *pM, float *out,
                                    int oh, int ow, void *stream);
/* warp.vec2mtrx (warp.py:25-43): p [B,8] (homography, sl(3) generator) or [B,6] (affine) -> [B,9]
 * Taylor matrix exponential with `warp_approx` terms. */
VSTAB_API int vstab_vec2mtrx(const float *p, int B, int dim, int warp_approx, float *out, void *stream);
/* ---- backward of the three above: what TensorFlow's autodiff gives for warp.py:46-86 / 89-129 and :25-43.  Conventions, limits and
 * error codes of vstab_st_transform_backward (B <= 65535, B*Hi*Wi*C < 2^31; a NULL output skips that gradient's work, both NULL is
 * VSTAB_E_SHAPE).  floor, ceil and the int casts have zero derivative and there is no clip; coordinates and taps are the forward's fp32
 * values; a tap outside the image reads 0 and receives nothing.  Where a source coordinate is an exact integer floor == ceil, both
 * taps are the same pixel and that axis' slope is 0 (the reference's behaviour).  dout [B,oh,ow,C].
 *   d_img   [B,Hi,Wi,C] (nullable): zero-filled on `stream` when accumulate == 0, added into when accumulate == 1; float atomics, so its
 *           last bits DEPEND ON ATOMIC ARRIVAL ORDER.
 *   d_M     [B,9] (nullable): overwritten; d xh = gx / zs, d yh = gy / zs, d zh = -(gx xh + gy yh) / zs^2 with zs = zh + 1e-8f, times
 *           (X, Y, 1), products and sums in double in a fixed order (two runs are bit-equal), rounded to fp32 once.
 *   d_pM    [B,9] (nullable), vstab_transform_image_backward: M = ref . pM is composed as in the forward and d_pM = ref^T . d_M, in
 *           double, rounded once.  ref is configuration: it gets no gradient.
 *   workspace: vstab_homography_warp_backward_workspace_bytes() (both calls), 8-byte aligned; VSTAB_E_NOMEM when too small, not read
 *           when the matrix gradient is NULL.  0 for a shape outside the contract.
 * vstab_vec2mtrx_backward: d_out [B,9] the gradient of the matrix -> d_p [B,dim], the reverse of the Taylor recurrence
 * (d A = sum_i 1/i! sum_{j<i} (A^j)^T d_out (A^(i-1-j))^T mapped back through the generator layout), in double from the fp32 p,
 * rounded once; reproducible; needs no workspace. */
VSTAB_API size_t vstab_homography_warp_backward_workspace_bytes(int B, int Hi, int Wi, int C, int oh, int ow);
VSTAB_API int vstab_homography_warp_backward(const float *img, int B, int Hi, int Wi, int C, const float *M, const float *dout, int oh,
                                             int ow, float *d_img, int accumulate, float *d_M, void *workspace, size_t workspace_bytes,
                                             void *stream);
VSTAB_API int vstab_transform_image_backward(const float *img, int B, int Hi, int Wi, int C, const float *ref, const float *pM,
                                             const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_pM,
                                             void *workspace, size_t workspace_bytes, void *stream);
VSTAB_API int vstab_vec2mtrx_backward(const float *p, int B, int dim, int warp_approx, const float *d_out, float *d_p, void *stream);

/* ---- VGG16 convolutional trunk (vgg16.py:25-64; BASELINE config 5) ------------------------------
 * 13 x (conv 3x3 SAME + bias + ReLU) and 5 x (max pool 2x2 stride 2 SAME).  Weights in the layout of
 * vgg16.npy: for every layer L in conv1_1 .. conv5_3 a tensor "L/filter" [3][3][Cin][Cout] and
 * "L/biases" [Cout] (HOST pointers).  The input is whatever the caller feeds vgg.build -- NLDF.py:29
 * feeds x*255 - VGG_MEAN, see vstab_scale_shift. */
VSTAB_API int vstab_vgg16_load(vstab_ctx *ctx, const vstab_tensor *tensors, int count);
VSTAB_API size_t vstab_vgg16_workspace_bytes(int B, int H, int W);
/* Shapes of the 18 outputs in build() order (conv1_1, conv1_2, pool1, conv2_1, conv2_2, pool2, conv3_1,
 * conv3_2, conv3_3, pool3, conv4_1..3, pool4, conv5_1..3, pool5): hwc54[3*i..3*i+2] = (h, w, c). */
VSTAB_API int vstab_vgg16_shapes(int H, int W, int32_t *hwc54);
/* input [B,H,W,3] -> outputs[18] (device pointers, caller-allocated, NHWC, shapes as above).  Batches whose
 * conv1 activations would reach 2 GiB are processed in chunks. */
VSTAB_API int vstab_vgg16_forward(vstab_ctx *ctx, const float *input, int B, int H, int W, float *const *outputs18,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* out = x * scale - mean[c]  (NLDF.py:29: input_holder * 255. - vgg16.VGG_MEAN), x [npix, C], C <= 4, mean HOST. */
VSTAB_API int vstab_scale_shift(const float *x, long long npix, int C, float scale, const float *mean, float *out,
                                void *stream);
/* tf.nn.max_pool(ksize 2, strides 2, SAME) on NHWC, C % 4 == 0 (vgg16.py:51-53). */
VSTAB_API int vstab_maxpool2x2(const float *x, int B, int H, int W, int C, float *out, void *stream);

/* ---- VGG16 trunk, backward (Vgg16.backward / Vgg16.features) ----------------------------------------
 * The reverse walk over the 13 convolutions and 5 pools.  outputs18: the activations vstab_vgg16_forward wrote for `input`
 * (all 18 non-NULL).  douts18: the gradient at each output, NULL = none; the walk starts at the deepest non-NULL one and the
 * layers above it are not touched.  dinput [B,H,W,3] or NULL.  dparams26: {filter, biases} gradient per layer in the order of
 * vstab_vgg16_load's layers ([3][3][Cin][Cout], [Cout]), NULL (or NULL entries: that layer's are not computed) = none;
 * accumulate_params adds into them instead of writing them.  A max-pool window's gradient goes to its first maximum in the order
 * (0,0), (0,1), (1,0), (1,1) among the taps inside the image, and a gradient passes a ReLU only where its output is > 0.
 * Batches are processed in vstab_vgg16_forward's chunks; filter gradients accumulate across them.
 * VSTAB_E_STATE: no loaded weights, a NULL outputs18[i], no gradient at any output, neither dinput nor a parameter gradient;
 * VSTAB_E_ALIGN: a pointer not 16-byte (workspace: 256-byte) aligned; VSTAB_E_NOMEM: workspace below
 * vstab_vgg16_backward_workspace_bytes(); VSTAB_E_SHAPE: a size the forward refuses.  Nothing is launched before these checks. */
VSTAB_API size_t vstab_vgg16_backward_workspace_bytes(int B, int H, int W, int need_weights);
VSTAB_API int vstab_vgg16_backward(vstab_ctx *ctx, const float *input, int B, int H, int W, float *const *outputs18,
                                   const float *const *douts18, float *dinput, float *const *dparams26, int accumulate_params,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* Backward of vstab_maxpool2x2 fused with the ReLU gate of its input: y [B,H,W,C] (a ReLU's output), dpool
 * [B,ceil(H/2),ceil(W/2),C] -> dy [B,H,W,C], every element written.  accumulate: dy holds a gradient at y already and becomes
 * (dy + routed) where y > 0, 0 elsewhere.  C % 4 == 0. */
VSTAB_API int vstab_maxpool2x2_relu_backward(const float *y, int B, int H, int W, int C, const float *dpool, float *dy,
                                             int accumulate, void *stream);
/* dy[i] = y[i] > 0 ? dy[i] : 0 in place, n % 4 == 0. */
VSTAB_API int vstab_relu_backward(const float *y, float *dy, long long n, void *stream);
/* conv1_1 (3x3 SAME, 3 -> cout <= 64, cout % 4 == 0; W HWIO on the device): the input gradient dx [B,H,W,3] of gout
 * [B,H,W,cout], and the filter / bias gradient dW [3][3][3][cout], db [cout] (or NULL) from x [B,H,W,3] and gout. */
VSTAB_API int vstab_conv3x3_rgb_dgrad(const float *gout, int B, int H, int W, const float *Wf, int cout, float *dx, void *stream);
VSTAB_API size_t vstab_conv3x3_rgb_wgrad_workspace_bytes(int B, int H, int W);
VSTAB_API int vstab_conv3x3_rgb_wgrad(const float *x, const float *gout, int B, int H, int W, int cout, float *dW, float *db,
                                      int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* ---- NLDF saliency head (NLDF.py:24-101; tertiary, never instantiated by the reference) ----------
 * Weights: "<L>/W", "<L>/b" for L in Fea_Global_1, Fea_Global_2, Fea_Global, Fea_P1..Fea_P5, Local_Fea,
 * Local_Score, Global_Score (conv [k][k][Cin][Cout]) and Fea_P2_Deconv..Fea_P5_Deconv ([5][5][Cout][Cin]).
 * pools5 = device pointers to the VGG16 pool1..pool5 of a 352x352 input (176/88/44/22/11, NHWC).
 * prob [B,176,176,1] (required); score [B,176,176,2], local_fea [B,176,176,640], fea_global [B,1,1,128]
 * optional (NULL to skip). */
VSTAB_API int vstab_nldf_load(vstab_ctx *ctx, const vstab_tensor *tensors, int count);
VSTAB_API size_t vstab_nldf_workspace_bytes(int B);
/* Host-only: names, offsets and shapes of the head's tensors inside that workspace, from the plan vstab_nldf_forward runs (tests):
 * G1 [B,7,7,128], G2 [B,3,3,128], Fea_Global [B,1,1,128], cat1..cat5 = [Fea_Pk | Fea_Pk_LC | Fea_P(k+1)_Up] ([B,176,176,768],
 * [B,88,88,640], [B,44,44,512], [B,22,22,384], [B,11,11,256]), Local_Fea (unused when the caller passes local_fea), Local_Score
 * [B,176,176,2], Global_Score [B,1,1,2], splitk (h == 0: a flat run of c floats).  Returns the number of entries written
 * (<= max_entries) or a negative error. */
VSTAB_API int vstab_nldf_workspace_layout(int B, vstab_ws_entry *entries, int max_entries);
VSTAB_API int vstab_nldf_forward(vstab_ctx *ctx, const float *const *pools5, int B, float *prob, float *score,
                                 float *local_fea, float *fea_global, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* ---- NLDF saliency head, backward (NLDF.Model.backward / pools_grad) ------------
 * The reverse walk of vstab_nldf_forward at the same hard-wired geometry.  vstab_nldf_load keeps every variable as given on the
 * device; the launchers below it take raw weights.  pools5: as in the forward.  fwd_workspace: the forward's workspace of the same
 * batch as the forward left it (cat1..cat5, G1, G2, Fea_Global are read, nothing is written); local_fea: the tensor the forward
 * wrote.  dscore [B,176,176,2] is required; dprob [B,176,176,1] (with prob, the forward's), dlocal_fea [B,176,176,640] and dfea_global
 * [B,1,1,128] are the optional gradients at the forward's other outputs (NULL = none).  dpools5: five output pointers
 * [B,hw,hw,C_k] or NULL, each non-NULL one written in full.  dparams30: {W, b} gradient of the 15 layers in the order Fea_Global_1,
 * Fea_Global_2, Fea_Global, Fea_P1..Fea_P5, Fea_P5_Deconv..Fea_P2_Deconv, Local_Fea, Local_Score, Global_Score, in the variables' own
 * layouts; NULL, or NULL entries, are skipped (no filter-gradient launch is made for them, and an input gradient nothing asks for is not
 * launched either); accumulate_params adds into them instead of writing.  A gradient passes a ReLU only where its output is > 0.
 * No float atomics in the walk's own kernels and none in the launchers it composes: two calls give the same bits.
 * VSTAB_E_STATE: no loaded head, a required pointer NULL, dprob without prob, a bias gradient without its filter gradient, no
 * gradient asked for at all; VSTAB_E_ALIGN: a pointer not 16-byte (workspaces: 256-byte) aligned; VSTAB_E_NOMEM: a workspace below
 * vstab_nldf_workspace_bytes() / vstab_nldf_backward_workspace_bytes(); VSTAB_E_SHAPE: a batch the forward refuses.  Nothing is launched
 * before these checks. */
VSTAB_API size_t vstab_nldf_backward_workspace_bytes(int B, int need_weights);
VSTAB_API int vstab_nldf_backward(vstab_ctx *ctx, const float *const *pools5, int B, const void *fwd_workspace, size_t fwd_workspace_bytes,
                                  const float *local_fea, const float *prob, const float *dscore, const float *dprob, const float *dlocal_fea,
                                  const float *dfea_global, float *const *dpools5, float *const *dparams30, int accumulate_params,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* The walk's own kernels, one stage at a time (tests).
 * Score stage at the head's geometry (npix = 176*176, 640 features): dls [B,npix,2] = dscore + Prob's share (p0 (1 - p0) dprob on
 * channel 0, minus that on channel 1; written only when dprob != NULL, otherwise dscore itself is Local_Score's gradient and dls may
 * be NULL), dgs [B,2] = its sum over each sample's pixels (Global_Score's gradient), db2 [2] = sum_b dgs (either score bias),
 * dlf [B,npix,640] = dls[p,0] W[:,0] + dls[p,1] W[:,1] (+ dlocal_fea), dW [640,2] = sum_p local_fea[p,:]^T dls[p,:] (W, dW: Local_Score/W's
 * layout).  dlf, dW (with local_fea), db2 optional.  workspace: vstab_nldf_score_backward_workspace_bytes(B), 256-byte aligned. */
VSTAB_API size_t vstab_nldf_score_backward_workspace_bytes(int B);
VSTAB_API int vstab_nldf_score_backward(const float *dscore, const float *prob, const float *dprob, const float *local_fea, const float *dlocal_fea,
                                        const float *W, int B, float *dls, float *dgs, float *dlf, float *dW, float *db2, int accumulate,
                                        void *workspace, size_t workspace_bytes, void *stream);
/* Contrast_Layer's adjoint (the layer is self-adjoint) fused with Fea_Pk's ReLU gate, in place on a gradient buffer: act, dcat
 * [B,H,W,cs] with act[..., 0:C] = Fea_Pk, dcat = [dP | dLC | ...]; dcat[..., 0:C] becomes (Fea_Pk > 0) ? dP + dLC - avg3x3_sym(dLC) : 0.
 * C % 4 == 0, cs % 4 == 0, cs >= 2 C. */
VSTAB_API int vstab_nldf_contrast_gate_backward(const float *act, float *dcat, int B, int H, int W, int C, int cs, void *stream);
/* ReLU gate of a channel slice in place, d[row, c_off + c] = act[row, c_off + c] > 0 ? d : 0 for c < C, and (db != NULL) db [C] (+)= the
 * gated slice's column sums (a transposed convolution's bias gradient).  workspace: vstab_column_sum_scratch_bytes(rows, C). */
VSTAB_API int vstab_nldf_slice_gate_backward(const float *act, float *d, long long rows, int cs, int c_off, int C, float *db, int accumulate,
                                             void *workspace, size_t workspace_bytes, void *stream);

/* ---- NLDF's objective (NLDF.py:79-100, :136-171; csrc/nldf_loss_ops.hip states the formulas) -------------------------------
 * Shared refusals: VSTAB_E_STATE for a required pointer that is NULL, VSTAB_E_SHAPE unless every dimension is >= 1 and the tensor has
 * fewer than 2^31 elements, VSTAB_E_ALIGN / VSTAB_E_NOMEM for a workspace that is not 8-byte aligned / too short.  A refused call
 * launches nothing and writes nothing.  No float atomics: two calls give the same bits. */
/* im_gradient (NLDF.py:151-156) per channel of x [B,H,W,C], 1 <= C <= 4: sqrt(gx^2 + gy^2) of the two 3x3 Sobel correlations of the
 * one-pixel SYMMETRIC (= clamp-to-edge) pad.  out [B,H,W,C]. */
VSTAB_API int vstab_sobel_magnitude(const float *x, int B, int H, int W, int C, float *out, void *stream);
/* dx [B,H,W,C] = the adjoint of that map at x applied to dout [B,H,W,C].  A pixel whose magnitude is exactly 0 passes no gradient
 * (TensorFlow gives inf * 0 = NaN there). */
VSTAB_API int vstab_sobel_magnitude_backward(const float *x, const float *dout, int B, int H, int W, int C, float *dx, void *stream);
/* The fused loss on score, label [B,H,W,2] (8-byte aligned): Prob_Grad = tanh(sum_c im_gradient(softmax(score))_c), label_Grad =
 * (sum_c im_gradient(label)_c > contour_th), C_IoU_LOSS = 1 - 2 (sum pg lg + 1) / (sum pg^2 + sum lg^2 + 1) over the whole batch,
 * CE = mean over pixels of -sum_c label_c log_softmax(score)_c, accuracy = share of pixels whose argmax (ties to channel 0) agree.
 * scalars4 (device, required) = {Loss_Mean = C_IoU_LOSS + CE, C_IoU_LOSS, CE, accuracy}; prob_grad, label_grad [B,H,W,1] and dscore
 * [B,H,W,2] optional (NULL to skip); dscore = dscale * d Loss_Mean / d score (label_Grad carries no gradient; a channel whose Sobel
 * magnitude is exactly 0 passes none).  Two launches, three with dscore, whatever B, H and W.  workspace:
 * vstab_nldf_loss_workspace_bytes() bytes (0 for a refused shape), 8-byte aligned. */
VSTAB_API size_t vstab_nldf_loss_workspace_bytes(int B, int H, int W);
VSTAB_API int vstab_nldf_loss(const float *score, const float *label, int B, int H, int W, float contour_th, float *scalars4, float *prob_grad,
                              float *label_grad, float *dscore, float dscale, void *workspace, size_t workspace_bytes, void *stream);
/* The reductions behind Loss_IoU (mode 0: 1 - 2 (sum a b + 1) / (sum a^2 + sum b^2 + 1); NLDF.py:158-165, whose `inter == 0` branch is never
 * taken), Loss_Contour (mode 1: mean(-b log(a + 1e-5) - (1 - b) log(1 - a + 1e-5)); :167-168) and L2 (mode 2: wd sum a^2 / 2; :170-171, b not
 * read) over n elements: *value (device) and, when grad != NULL, grad [n] = d value / d a.  wd is read by mode 2 only.  Two launches, three
 * with grad.  VSTAB_E_SHAPE also for another mode. */
#define VSTAB_NLDF_REDUCE_IOU     0
#define VSTAB_NLDF_REDUCE_CONTOUR 1
#define VSTAB_NLDF_REDUCE_L2      2
VSTAB_API size_t vstab_nldf_reduce_workspace_bytes(long long n);
VSTAB_API int vstab_nldf_reduce(int mode, const float *a, const float *b, long long n, float wd, float *value, float *grad, void *workspace,
                                size_t workspace_bytes, void *stream);

/* ---- autoregressive clip driver pieces (per-frame loop of evaluate_originalSize, main:535-630) ----
 * All frames are uint8 [B,h,w,3] in cv2's BGR order, device memory. */
/* cv2.resize(src, (dw, dh)), INTER_LINEAR, 8-bit (main:550,556-558): restated fixed-point algorithm, see clip_ops.hip. */
VSTAB_API int vstab_resize_u8(const uint8_t *src, int B, int sh, int sw, uint8_t *dst, int dh, int dw, void *stream);
/* np.uint8(cv2.cvtColor(cv2.resize(img_f32, (dw, dh)) * 255, COLOR_RGB2BGR)) (main:861-863: the native evaluator's history frame):
 * float bilinear resize with cv2's half-pixel centres, * 255, channels 0 and 2 swapped, truncated to 8 bits.  src [B,sh,sw,3]. */
VSTAB_API int vstab_resize_f32_to_u8(const float *src, int B, int sh, int sw, uint8_t *dst, int dh, int dw, void *stream);
/* curinput (main:550-558): feats[B,h,w,27]; slot j < 8 = history frame of lag {31,23,15,7,4,3,2,1}[j], slot 8 = current
 * frame, each u8 [B,h,w,3] at network resolution; channels swapped (COLOR_RGB2BGR) and divided by 255.  feats 16-byte aligned. */
VSTAB_API int vstab_assemble_input(const uint8_t *const *slots9, int B, int h, int w, float *feats, void *stream);
/* The same with the current frame's cv2.resize inside (main:550 + 553-558 as one launch): frame u8 [B,sh,sw,3] at its own resolution;
 * slots8[j] == NULL reads the resized current frame (the first frame of a clip, main:548-549). */
VSTAB_API int vstab_assemble_input_resized(const uint8_t *const *slots8, const uint8_t *frame, int B, int h, int w, int sh, int sw,
                                           float *feats, void *stream);
/* The evaluator's frame path on 8-bit frames in ONE launch (main:568, 497-514, 625/630): out = uint8(swap(tf_warp(swap(frame)/255,
 * glue(flow)) * 255)); the fp32 frame and the fp32 warped frame never exist.  flow [B,h,w,2] (predict_flow2), frame / out u8
 * [B,oh,ow,3] BGR, outflow [B,oh,ow,2] or NULL.  Identical bytes to vstab_frame_to_float + vstab_flow_glue_warp + vstab_quantise_output. */
VSTAB_API int vstab_flow_glue_warp_u8(const float *flow, int B, int h, int w, const uint8_t *frame, float *outflow, uint8_t *out, int oh, int ow,
                                      int net_h, int net_w, void *stream);
/* One frame of the evaluator's loop as ONE call (main:550-558 input, 568-569 network, 497-514 + 625/630 the 8-bit glue + warp, 556 the
 * history frame): vstab_assemble_input_resized(slots8, frame) -> feats [n,net_h,net_w,27]; vstab_flownets_forward(feats) -> pf6..pf2;
 * vstab_flow_glue_warp_u8(pf2, frame) -> out u8 [n,oh,ow,3] (and outflow [n,oh,ow,2] unless NULL); vstab_resize_u8(out) -> ring_slot
 * u8 [n,net_h,net_w,3], the slot later frames read this one back from.  slots8: HOST array of 8 device pointers (lags 31,23,15,7,4,3,2,1;
 * NULL = the resized current frame).  Every buffer is the caller's, allocated once; identical bytes to the four calls.  The network
 * takes 27 input channels (8 history frames + the current one).  `out`, `ring_slot` and `frame` must not overlap (the warp gathers
 * frame pixels while `out` is being written): VSTAB_E_STATE otherwise. */
VSTAB_API int vstab_clip_step(vstab_ctx *ctx, const uint8_t *const *slots8, const uint8_t *frame, int n, int net_h, int net_w, int oh, int ow,
                              float *feats, float *pf6, float *pf5, float *pf4, float *pf3, float *pf2, float *outflow, uint8_t *out,
                              uint8_t *ring_slot, void *workspace, size_t workspace_bytes, void *stream);
/* ---- the training loader's batch (data_loader.py: _read_frame :203-206, read_dataset :132-169; main:179-184) ----
 * stab / unstab: one clip's two frame pools, uint8 [N,sh,sw,3] in RGB order (the loader's cvtColor(BGR2RGB) already applied), device
 * memory.  rows [n] and frame_idx [n][9] are HOST arrays: sample i fills output row rows[i] with
 *   feats[rows[i],:,:,3j+c] = resize(stab[frame_idx[i][j]] / 255.) for j < 8,
 *   feats[rows[i],:,:,24+c] = unstab_out[rows[i]] = resize(unstab[frame_idx[i][8]] / 255.),   gtstab[rows[i]] = resize(stab[frame_idx[i][8]] / 255.),
 * resize = cv2.resize(., (W, H)), INTER_LINEAR on the float64 image (restated, see train_batch_ops.hip), rounded to fp32 once.
 * feats [B,H,W,27] (16-byte aligned), gtstab / unstab_out [B,H,W,3]; rows not named are left untouched.  One call serves the samples of
 * one clip; a batch spanning clips is one call per clip.  The indices travel in the kernel arguments
 * (vstab_assemble_train_batch_launch_samples() samples per launch): no copy, no synchronisation, capturable.
 * VSTAB_E_SHAPE: a size < 1, frame_idx outside [0,N), rows outside [0,B) or not distinct, feats not 16-byte aligned. */
VSTAB_API int vstab_assemble_train_batch(const uint8_t *stab, const uint8_t *unstab, int N, int sh, int sw, const int *rows, const int *frame_idx,
                                         int n, float *feats, float *gtstab, float *unstab_out, int B, int H, int W, void *stream);
VSTAB_API int vstab_assemble_train_batch_launch_samples(void);
/* resizedInput (main:568): swap(frame)/255 -> float [npix,3]. */
VSTAB_API int vstab_frame_to_float(const uint8_t *frame, long long npix, float *out, void *stream);
/* np.uint8(swap(warped*255)) (main:625,630,556): float [npix,3] -> u8, truncating, saturating outside [0,255]. */
VSTAB_API int vstab_quantise_output(const float *warped, long long npix, uint8_t *out, void *stream);

/* ---- flow post-filters of the reference's other evaluators ---------------------
 * k x k box blur of a flow field with zero (SAME) padding, weights 1/(k*k), k odd
 * (main_flownetS_pyramid.py:634-641, k = 75).  tmp: scratch of the same size as flow. */
VSTAB_API int vstab_flow_box_blur(const float *flow, int B, int h, int w, int k, float *tmp, float *out, void *stream);
/* out = a*x + b*y elementwise (0.9*smooth + 0.1*prev, :643; prev = 0.9*prev + 0.1*cur, :695). */
VSTAB_API int vstab_axpby(const float *x, float a, const float *y, float b, float *out, long long n, void *stream);
/* ---- training objective, first slice of SURVEY.md 8f rank 4 -------------------------------------------
 * One pyramid level of the reference's loss (main:188-210, 269-273) and its gradient w.r.t. the flow:
 *   P = tf_warp(unstab, pf), M = tf_warp(ones, pf); masked_MSE = mean_b[ sum (P*M - gt*M)^2 / sum safe(M) ];
 *   TV = sum_b tf.image.total_variation(pf[b]).
 * gt / unstab: [B,h,w,3] already resized to the flow's size (vstab_resize_bilinear = tf.image.resize_images).
 * sums: device double[3*B], overwritten with {sum sq, sum safe(M), TV} per sample -- the level's loss is
 *   scale_mse * mean_b(sums[3b]/sums[3b+1]) + scale_tv * sum_b sums[3b+2]   (the caller adds the levels up).
 * grad_pf (may be NULL): [B,h,w,2] d(that loss)/d(pf), overwritten.
 * Limits: B <= 65535 and h * w * 3 < 2^31, VSTAB_E_SHAPE beyond them (nothing is launched).  This is vstab_loss_level_multi below
 * at Ct = 3, T = 1, c_off = {0}, weights = {1}, plus scale_mse. */
VSTAB_API int vstab_loss_level(const float *pf, const float *gt, const float *unstab, int B, int h, int w, double *sums,
                               float scale_mse, float scale_tv, float *grad_pf, void *stream);

/* loss_main (main:213-217, 269-275) over all pyramid levels in one call: per level the two tf.image.resize_images of the
 * full-size stable / unstable frames [B,H,W,3] to the flow's size (main:202-203), lossterm + the TV term, and (grad != NULL)
 * d loss_main / d flow written into channels 0..1 of the caller's [B,h,w,cs_grad] buffer.  pf: [B,h,w,cs_pf] pixels whose
 * channels 0..1 are the flow; channel strides even.  loss_out: one device double = sum over levels of
 * mean_b(masked_MSE) + tv_weight * TV.
 * Limits: 1..8 levels, B <= 65535 and h * w * 3 < 2^31 for every level: beyond them vstab_loss_main returns VSTAB_E_SHAPE before
 * anything is launched and vstab_loss_main_workspace_bytes returns 0.  This is vstab_loss_main_multi below at Ct = 3, T = 1,
 * c_off = {0}, weights = {1}, with one double of output. */
typedef struct vstab_loss_level_desc {
    const float *pf;
    float *grad;
    int h, w, cs_pf, cs_grad;
    float tv_weight;
} vstab_loss_level_desc;
VSTAB_API size_t vstab_loss_main_workspace_bytes(const vstab_loss_level_desc *levels, int n_levels, int B);
VSTAB_API int vstab_loss_main(const vstab_loss_level_desc *levels, int n_levels, const float *gtstab, const float *unstab, int B, int H,
                              int W, double *loss_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the full objective of main_flownetS_pyramid.py / main_flownetS_pyramid_highTV_noBBloss.py (:200-250) ----------------
 * One level against T weighted targets, 1 <= T <= 8: the warped unstable frame is compared with the ground-truth stable frame AND
 * with earlier stabilised frames, 3-channel slices c_off[t]..c_off[t]+2 of one tensor `targets` [B,h,w,Ct] (already resized, like
 * unstab [B,h,w,3]); c_off / weights are HOST arrays of T entries.  The warp, the mask, sum safe(M) and TV are shared:
 *   loss = sum_t weights[t] * mean_b(num_t / den) + scale_tv * sum_b TV
 * sums: device double[(T+2)*B], overwritten with {num_0 .. num_{T-1}, den, TV} per sample.  grad_pf (may be NULL): [B,h,w,2]
 * d loss / d pf, overwritten.  With T = 1, weights[0] = 1 both outputs are those of vstab_loss_level(scale_mse = 1) on that slice: the
 * same kernels.
 * VSTAB_E_STATE for a NULL buffer or array; VSTAB_E_SHAPE for T outside 1..8, c_off[t] < 0 or c_off[t] + 3 > Ct, bad sizes;
 * VSTAB_E_ALIGN when pf / grad_pf / sums are not 8-byte aligned. */
VSTAB_API int vstab_loss_level_multi(const float *pf, const float *targets, int Ct, int T, const int *c_off, const float *weights,
                                     const float *unstab, int B, int h, int w, double *sums, float scale_tv, float *grad_pf, void *stream);
/* All levels of that objective in one call, the levels described as for vstab_loss_main: per level ONE resize of the full-size
 * target tensor [B,H,W,Ct] (all Ct channels) and one of unstab [B,H,W,3], then the level above with its gradient written into
 * channels 0..1 of the level's grad buffer.  loss_out: device double[1 + T] = the objective (sum over levels of
 * sum_t weights[t] * mean_b(masked_MSE_t) + tv_weight * TV), then per target the unweighted sum over levels of mean_b(masked_MSE_t).
 * One target of weight 1 is vstab_loss_main on that slice (only the target's three channels are resized): value and gradients are
 * its bits.  The call allocates nothing; workspace as sized by vstab_loss_main_multi_workspace_bytes (0 for arguments the call would reject),
 * VSTAB_E_NOMEM when too small.  Errors as above; odd channel strides in a descriptor are VSTAB_E_SHAPE. */
VSTAB_API size_t vstab_loss_main_multi_workspace_bytes(const vstab_loss_level_desc *levels, int n_levels, int B, int Ct, int T);
VSTAB_API int vstab_loss_main_multi(const vstab_loss_level_desc *levels, int n_levels, const float *targets, int Ct, int T, const int *c_off,
                                    const float *weights, const float *unstab, int B, int H, int W, double *loss_out, void *workspace,
                                    size_t workspace_bytes, void *stream);
/* The loss report of the test pass (main:277-326, 346-372): vstab_loss_main_multi's value from the same sums, without the gradient
 * pass (levels[l].grad and cs_grad are ignored, nothing is written there), with the scalars the reference logs per level and, on
 * request, each level's warped frame.
 *   out: device double[1 + T + 2 * n_levels] = total (what vstab_loss_main[_multi] returns from the same sums: the same double
 *        arithmetic in the same order), the T unweighted per-target shares, then mse_l = sum_t weights[t] * mean_b(masked_MSE_t) of
 *        every level (loss6..loss2) and var_l = tv_weight_l * sum_b TV of every level (var6..var2).
 *   previews: NULL, or HOST array of n_levels device pointers, each NULL or [B,h,w,3] of that level's size: tf_warp(unstab resized,
 *        flow) -- lossterm's second return value `warpedimg`, before the mask -- as float32 (preview_dtype 0) or as uint8
 *        utils.fix_image_tf(warpedimg, 1) (preview_dtype 1): warpedimg * 255 saturated to 0..255, then truncated toward zero.  The
 *        preview is stored by the kernel that forms the sums: one flow read and one gather per pixel serve both.
 * Workspace, limits and errors as vstab_loss_main_multi, judged in its order; then VSTAB_E_SHAPE for preview_dtype outside {0, 1} and
 * VSTAB_E_ALIGN for a float32 preview that is not 4-byte aligned.  A refused call allocates and launches nothing. */
VSTAB_API size_t vstab_loss_report_workspace_bytes(const vstab_loss_level_desc *levels, int n_levels, int B, int Ct, int T);
VSTAB_API int vstab_loss_report(const vstab_loss_level_desc *levels, int n_levels, const float *targets, int Ct, int T, const int *c_off,
                                const float *weights, const float *unstab, int B, int H, int W, void *const *previews, int preview_dtype,
                                double *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- image similarity: tf_ssim / tf_ms_ssim of the reference's utils.py (:74-166) --------------------------------------------
 * img1, img2: [B,H,W] (one channel).  With the size x size window of _tf_fspecial_gauss(size, sigma) (:74-89; offsets
 * -size//2+1 .. size//2 with floor division, so an even size is not symmetric; applied in its separable form) and five VALID
 * correlations,
 *   mu1 = w*x, mu2 = w*y, s1 = w*x^2 - mu1^2, s2 = w*y^2 - mu2^2, s12 = w*xy - mu1 mu2,
 *   s = (s12^2 + C3) / (s1 s2 + C3),  C3 = 0.03^2 / 2        (:111; the factors l**0 and c**0 of :113 are the constant 1)
 * on oh x ow = (H-size+1) x (W-size+1) positions.  map (may be NULL): [B,oh,ow] receives s; means (may be NULL): [B] receives the
 * per-sample mean of s, summed without atomics in a fixed order (two calls give the same bits); at least one of the two.
 * workspace: vstab_ssim_forward_workspace_bytes() bytes, 4-byte aligned, needed only with means (VSTAB_E_NOMEM when too small).
 * VSTAB_E_STATE for a NULL image, both outputs NULL, or means without a workspace (checked first); VSTAB_E_SHAPE unless B >= 1
 * (<= 65535), 1 <= size <= 11, H, W >= size, sigma > 0 and B*H*W < 2^31; the workspace query returns 0 for such arguments. */
VSTAB_API size_t vstab_ssim_forward_workspace_bytes(int B, int H, int W, int size);
VSTAB_API int vstab_ssim_forward(const float *img1, const float *img2, int B, int H, int W, int size, float sigma, float *map, float *means,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* Gradient of the above with respect to both images for the upstream gradient dmap [B,oh,ow] of the map and / or dmeans [B] of the
 * per-sample means (either may be NULL, not both; both given add up): d_img1, d_img2 [B,H,W], overwritten; a NULL output skips
 * that image (both NULL is VSTAB_E_SHAPE).  l**0 and c**0 carry no gradient (TensorFlow's 0 * c^-1 is NaN on a flat window):
 *   ds/ds12 = 2 s12 / D, ds/ds1 = -N s2 / D^2, ds/ds2 = -N s1 / D^2 with N, D the numerator and denominator of s,
 * taken back through the adjoint of the VALID correlation (the flipped window) by gathering -- no atomics, bit-reproducible.
 * workspace: vstab_ssim_backward_workspace_bytes() bytes (five [B,oh,ow] planes), 4-byte aligned; other errors as the forward's. */
VSTAB_API size_t vstab_ssim_backward_workspace_bytes(int B, int H, int W, int size);
VSTAB_API int vstab_ssim_backward(const float *img1, const float *img2, int B, int H, int W, int size, float sigma, const float *dmap,
                                  const float *dmeans, float *d_img1, float *d_img2, void *workspace, size_t workspace_bytes, void *stream);
/* tf.nn.avg_pool(x, [1,2,2,1], [1,2,2,1], 'SAME') (utils.py:146-147): x [B,H,W,C] -> out [B,ceil(H/2),ceil(W/2),C]; a window that
 * hangs over the edge averages the pixels that exist.  The backward takes dout of the pooled size and writes dx [B,H,W,C] (H, W: the
 * INPUT size).  VSTAB_E_STATE for a NULL buffer; VSTAB_E_SHAPE for a dimension < 1 or B*H*W*C >= 2^31. */
VSTAB_API int vstab_avgpool2x2_same(const float *x, int B, int H, int W, int C, float *out, void *stream);
VSTAB_API int vstab_avgpool2x2_same_backward(const float *dout, int B, int H, int W, int C, float *dx, void *stream);

/* ---- flow visualisation: flow_to_image / compute_color / make_color_wheel of the reference's main scripts
 * (main_flownetS_pyramid.py:824-957), the Middlebury colour code ------------------------------------------------------------------
 * flow: [B,H,W,2] float32, dense, read only (the reference zeroes unknown pixels in the caller's array; this does not).
 * img: [B,H,W,3] uint8.  anglemap (may be NULL): [B,H,W,3] uint8, the angle as a gray value in all three channels.
 * maxrad_in: NULL, or [B] device floats, the radius each sample's flow is divided by (a video wants one value for all frames).
 * With NULL each sample's own largest radius is found first: a pixel with |u| > 1e7 or |v| > 1e7 is unknown and counts as (0,0), a
 * pixel with a NaN component is left out (in the reference it makes the maximum come out as -1, an accident of argument order),
 * and the radius is sqrt(max(u*u + v*v)) in float32.  maxrad_out (may be NULL): [B] receives the radii used, given or found.
 * Per pixel, with d = maxrad > 0 ? maxrad : 2^-52 and un = u / d, vn = v / d in float32 (the reference adds float64 eps to the
 * float32 maximum and divides a float32 array by the sum, which under the NumPy of its day is a float32 division by the maximum):
 *   rad = sqrtf(un*un + vn*vn);  a = atan2f(-vn, -un) / pi;  fk = (a + 1) / 2 * 54 + 1;  k0 = floor(fk), k1 = k0 + 1 (56 -> 1)
 *   col = (1 - f) wheel[k0-1]/255 + f wheel[k1-1]/255 with f = fk - k0, in float64 from here;
 *   col = rad <= 1 ? 1 - rad (1 - col) : 0.75 col;  img byte = floor(255 col);  anglemap byte = trunc(a * 127 + 128) in float32.
 * Unknown and NaN pixels are black in img and 1 (the angle of (+0,+0)) in anglemap.  Everything is stream-ordered, nothing
 * synchronises with the host, and no atomics are used: two calls give the same bytes.
 * workspace: vstab_flow_to_image_workspace_bytes() bytes, 4-byte aligned, needed only without maxrad_in.
 * VSTAB_E_STATE for a NULL flow or img, or a NULL workspace without maxrad_in (checked first); VSTAB_E_SHAPE unless
 * 1 <= B <= 65535, H, W >= 1 and B*H*W < 2^31 (the workspace query returns 0 for such arguments); VSTAB_E_ALIGN unless flow is
 * 8-byte and the radii are 4-byte aligned; VSTAB_E_NOMEM when the workspace is too small. */
VSTAB_API size_t vstab_flow_to_image_workspace_bytes(int B, int H, int W);
VSTAB_API int vstab_flow_to_image(const float *flow, int B, int H, int W, const float *maxrad_in, unsigned char *img, unsigned char *anglemap,
                                  float *maxrad_out, void *workspace, size_t workspace_bytes, void *stream);

/* The recurrent cells of cell.py (ConvLSTMCell :5-76, ConvGRUCell :78-136), forward (backward: next block): what follows each cell's SAME convolution
 * over concat([x, h]) -- that convolution is vstab_conv_forward on the caller's concat buffer.  y: the convolution's output
 * [B,H,W,ys] (ys >= the gate channels; rows may be padded); states [B,H,W,F] contiguous, or slices of a wider NHWC buffer given as
 * the address of the slice's first channel in pixel 0 plus the buffer's channel stride.  act: 0 tanh, 1 relu, 2 identity.
 * Layer norm = tf.contrib.layers.layer_norm's defaults: per sample, mean and biased variance over all H*W*F numbers of a gate,
 * (v - mean) * rsqrt(var + 1e-12) * gamma[ch] + beta[ch].  Statistics are per-workgroup moments about the workgroup's own mean,
 * combined in double in a fixed order: no atomics, two runs give the same bits.
 * VSTAB_E_STATE for a NULL buffer that the flags require; VSTAB_E_SHAPE for a dimension < 1, a stride below its channels, B > 65535,
 * act outside 0..2 or a tensor of 2^31 elements or more; with normalize: VSTAB_E_ALIGN unless the workspace is 16-byte aligned,
 * VSTAB_E_NOMEM when it is smaller than the *_workspace_bytes() value (0 without normalize: workspace may then be NULL).
 *
 * LSTM: j, i, f, o = y[..., 0:F], [F:2F], [2F:3F], [3F:4F];  peephole: i += w_ci c, f += w_cf c (w_*: [H,W,F]);  normalize: j, i, f =
 * LN;  c' = c sigmoid(f + forget_bias) + sigmoid(i) act(j);  peephole: o += w_co c';  normalize: o, c' = LN;  h' = sigmoid(o) act(c').
 * gamma, beta: [5][F] in the order j, i, f, o, c.  c_out (may be c), h_out: [B,H,W,F]; h_cat (may be NULL): h' also goes to this slice.
 * Launches: 5 with normalize (moments, statistics, gates + moments, statistics, output), 1 without. */
VSTAB_API size_t vstab_convlstm_gates_workspace_bytes(int B, int H, int W, int F, int normalize);
VSTAB_API int vstab_convlstm_gates(const float *y, int ys, const float *c, const float *w_ci, const float *w_cf, const float *w_co,
                                   const float *gamma, const float *beta, int B, int H, int W, int F, float forget_bias, int act, int normalize,
                                   int peephole, float *c_out, float *h_out, float *h_cat, int cs_cat, void *workspace, size_t workspace_bytes,
                                   void *stream);
/* GRU, first half: r, u = sigmoid(LN or identity of y[..., 0:F], [F:2F]) (without normalize the convolution has added gates/bias);
 * rh slice <- r * h, u [B,H,W,F] <- u.  h, hs: the old state as a slice; gamma, beta: [2][F] (r, u).
 * Second half: h' = u h + (1 - u) act(LN or identity of y2[..., 0:F]); h_out [B,H,W,F]; h_new (may be NULL, may be h): h' as a slice.
 * gamma, beta: [F].  One workspace of vstab_convgru_workspace_bytes() serves both calls. */
VSTAB_API size_t vstab_convgru_workspace_bytes(int B, int H, int W, int F, int normalize);
VSTAB_API int vstab_convgru_gates(const float *y, int ys, const float *h, int hs, const float *gamma, const float *beta, int B, int H, int W,
                                  int F, int normalize, float *rh, int rhs, float *u, void *workspace, size_t workspace_bytes, void *stream);
VSTAB_API int vstab_convgru_update(const float *y2, int ys, const float *h, int hs, const float *u, const float *gamma, const float *beta, int B,
                                   int H, int W, int F, int act, int normalize, float *h_out, float *h_new, int hns, void *workspace,
                                   size_t workspace_bytes, void *stream);
/* The backward of the three stages above: gradients with respect to the convolution output(s), the old state and the stage's own
 * parameters; the convolutions' own gradients are vstab_conv_wgrad / vstab_conv_dgrad on the caller's concat buffer.  Gate values are
 * recomputed from y, the old state and the forward's per-sample {mean, rstd} pairs, which the forward call left in ITS workspace at
 * *_stats_offset() bytes (0: bad shape): LSTM which = 0: [B][3] pairs of j, i, f, which = 1: [B][2] of o, c';  GRU: [B][2] (r, u) after
 * vstab_convgru_gates, [B][1] after vstab_convgru_update (the same place: copy the first before the second call).  NULL without
 * normalize.  Layer-norm adjoint, per sample over the N = H*W*F numbers of a gate, xhat = (v - mean) rstd, g = dout gamma[ch]:
 * dv = rstd (g - mean_N(g) - xhat mean_N(g xhat)), dgamma[ch] = sum_{b,pixel} dout xhat, dbeta[ch] = sum_{b,pixel} dout.
 * Same index space and guarantees as the forward: every reduction is combined in double in a fixed order, no atomics, two runs
 * give the same bits, and a sample's dy / state gradients depend on that sample only.  dy rows [B,H,W,dys] are written whole (pad
 * channels zero).  Parameter gradients may be NULL (not wanted; the three peephole gradients go together, as do dgamma and dbeta);
 * accumulate != 0 adds into them (BPTT: t = T-1 down to 0).  Errors as the forward's; a workspace of *_backward_workspace_bytes()
 * (which may be 0: then NULL is allowed) is needed whatever gradients are wanted.
 *
 * LSTM: dh (slice: pointer + stride dhs) and dc_new [B,H,W,F] are the gradients of the returned h' and c' (either may be NULL = zero).
 * do_n = dh act(c_n) sigmoid'(o_n), dc_n = dc_new + dh sigmoid(o_n) act'(c_n); through LN_3 / LN_4; dc_raw += w_co do_raw;
 * df = dc_raw c, di = dc_raw act(j), dj = dc_raw i act'(j), dc = dc_raw f; through the sigmoids and LN_0..2; dc += w_ci di + w_cf df.
 * dy = [dj, di, df, do]; dc [B,H,W,F]; dw_ci, dw_cf, dw_co [H,W,F] = sum_b of di c, df c, do c_raw; dgamma, dbeta [5][F].
 * Launches with normalize: pass, sums, pass, sums, pass (+ the parameter reductions); 1 without. */
VSTAB_API size_t vstab_convlstm_gates_stats_offset(int B, int H, int W, int F, int which);
VSTAB_API size_t vstab_convlstm_gates_backward_workspace_bytes(int B, int H, int W, int F, int normalize, int peephole);
VSTAB_API int vstab_convlstm_gates_backward(const float *y, int ys, const float *c, const float *w_ci, const float *w_cf, const float *w_co,
                                            const float *gamma, const float *beta, const float *stats_jif, const float *stats_oc,
                                            const float *dh, int dhs, const float *dc_new, int B, int H, int W, int F, float forget_bias, int act,
                                            int normalize, int peephole, float *dy, int dys, float *dc, float *dw_ci, float *dw_cf,
                                            float *dw_co, float *dgamma, float *dbeta, int accumulate, void *workspace, size_t workspace_bytes,
                                            void *stream);
/* GRU update: from dh_new (slice) du [B,H,W,F] = dh_new (h - act(y2_n)), dy2 = dh_new (1 - u) act'(y2_n) through the candidate's layer
 * norm, dh (slice, WRITTEN) = dh_new u; dgamma, dbeta [F].
 * GRU gates: from du and drh (slice: the r h part of the candidate convolution's input gradient) dr = drh h, dh (slice) += drh r,
 * through both sigmoids and layer norms to dy = [dr, du]; dgamma, dbeta [2][F].  One workspace serves both calls. */
VSTAB_API size_t vstab_convgru_stats_offset(int B, int H, int W, int F);
VSTAB_API size_t vstab_convgru_backward_workspace_bytes(int B, int H, int W, int F, int normalize);
VSTAB_API int vstab_convgru_update_backward(const float *y2, int ys, const float *h, int hs, const float *u, const float *gamma, const float *beta,
                                            const float *stats, const float *dh_new, int dhns, int B, int H, int W, int F, int act, int normalize,
                                            float *dy2, int dys, float *du, float *dh, int dhs, float *dgamma, float *dbeta, int accumulate,
                                            void *workspace, size_t workspace_bytes, void *stream);
VSTAB_API int vstab_convgru_gates_backward(const float *y, int ys, const float *h, int hs, const float *gamma, const float *beta, const float *stats,
                                           const float *du, const float *drh, int drhs, int B, int H, int W, int F, int normalize, float *dy, int dys,
                                           float *dh, int dhs, float *dgamma, float *dbeta, int accumulate, void *workspace,
                                           size_t workspace_bytes, void *stream);

/* Weight and bias gradient of PadLayer(pad) -> Conv2d(k, stride, VALID) (model.py:807-844; what tf.gradients yields for
 * the filter of tf.nn.conv2d): dW[ky,kx,ci,co] = sum_{n,oy,ox} x[n, s*oy+ky-pad, s*ox+kx-pad, ci] * gout[n,oy,ox,co] in the
 * reference's HWIO layout, db[co] = sum gout (db may be NULL).  x: [B,Hi,Wi,cs_x] using channels cx_off..cx_off+cin;
 * gout: [B,Ho,Wo,cs_g] using channels cg_off..cg_off+cout; all channel counts / strides / offsets multiples of 4.
 * accumulate != 0 adds to dW / db instead of overwriting.  With x = the output gradient and gout = the input of a
 * 4x4 stride-2 SAME transposed conv (k 4, stride 2, pad 1) the result is that layer's [4,4,cout,cin] filter gradient.
 * The first call for a geometry builds a 16 B-per-output-pixel table on the device (and synchronises the stream once); it is
 * kept for the life of the process. */
VSTAB_API size_t vstab_conv_wgrad_workspace_bytes(int B, int Ho, int Wo, int k, int cin, int cout);
VSTAB_API int vstab_conv_wgrad(const float *x, int B, int Hi, int Wi, int cs_x, int cx_off, int cin, const float *gout, int Ho,
                               int Wo, int cs_g, int cg_off, int cout, int k, int stride, int pad, float *dW, float *db,
                               int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* Input gradient of the same layer (tf.gradients w.r.t. the conv's input): dx = transposed conv of gout with
 * W [k,k,cin,cout] (DEVICE pointer, the reference's HWIO layout), stride 1 or 2.  Runs on the forward MFMA kernel:
 * stride 1 = conv over gout with the kernel flipped, stride 2 = four output-parity phases of ceil(k/2)^2 taps; the
 * packed operand is gathered on the device every call (index table cached per geometry).  accumulate != 0: dx += result.
 * With W = a 4x4 stride-2 transposed conv's [4,4,cout,cin] filter, gout = its input and (k,stride,pad) = (4,2,1) the
 * same call computes that layer's FORWARD output. */
VSTAB_API size_t vstab_conv_dgrad_workspace_bytes(int B, int Ho, int Wo, int cs_g, int cout, int k, int stride, int pad, int Hi, int Wi,
                                                  int cs_x, int cx_off, int cin, int accumulate);
VSTAB_API int vstab_conv_dgrad(const float *gout, int B, int Ho, int Wo, int cs_g, int cg_off, int cout, const float *W,
                               const float *bias /* device [cin] added to every output pixel, or NULL */, int k, int stride, int pad,
                               float *dx, int Hi, int Wi, int cs_x, int cx_off, int cin, int accumulate, void *workspace,
                               size_t workspace_bytes, void *stream);
/* PadLayer(pad) -> Conv2d(k, stride, VALID) + bias with DEVICE-resident raw weights W [k,k,cin,cout] (training: the weights
 * change every step, so the MFMA operand is gathered on the device from an index table cached per geometry).
 * act: 0 none, 1 leaky relu 0.1, 2 relu, 3 none and ADD to what is in y. */
/* Ho, Wo: the output size; 0, 0 = floor((Hi + 2 pad - k)/stride) + 1, or that + 1 (TF SAME on an odd size: the last window
 * sticks out of the image and reads zeros there). */
VSTAB_API size_t vstab_conv_forward_workspace_bytes(int B, int Hi, int Wi, int cs_x, int cin, int k, int stride, int pad, int cout, int cs_y,
                                                    int cy_off, int act, int Ho, int Wo);
VSTAB_API int vstab_conv_forward(const float *x, int B, int Hi, int Wi, int cs_x, int cx_off, int cin, const float *W, const float *bias,
                                 int k, int stride, int pad, float *y, int Ho, int Wo, int cs_y, int cy_off, int cout, int act,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* PadLayer(pad) -> Conv2d(k, stride, VALID) + bias for a FEW-channel input (the network's first layer, model.py:807-808: 27 -> 64, 7x7
 * stride 2) on the inference path's row-window kernel, with DEVICE-resident raw weights Wf [k,k,cs_w,cout] of which input channels
 * 0..Cin-1 are used (cs_w >= Cin: the training buffers pad 27 to 28).  x [B,H,W,Cin] contiguous; cout <= 64; act 0 none, 1 leaky relu,
 * 2 relu; VSTAB_E_SHAPE when the kernel does not take the geometry (the caller then uses vstab_conv_forward). */
VSTAB_API size_t vstab_conv_rowwin_forward_workspace_bytes(int B, int H, int W, int Cin, int cs_w, int cout, int k, int stride, int pad, int cs_y,
                                                           int cy_off, int act);
VSTAB_API int vstab_conv_rowwin_forward(const float *x, int B, int H, int W, int Cin, const float *Wf, int cs_w, int cout, const float *bias, int k,
                                        int stride, int pad, float *y, int cs_y, int cy_off, int act, void *workspace, size_t workspace_bytes,
                                        void *stream);
/* The same for a 3x3 stride-1 pad-1 layer in Winograd F(2x2,3x3) form (4/9 of the multiply-adds): transpose = 0 is the forward
 * convolution x [.., cin] -> y [.., cout]; transpose = 1 the input gradient (x = output gradient [.., cout] -> y = dx [.., cin], kernel
 * flipped, channel roles swapped).  W: DEVICE [3,3,cin,cout]; the Winograd-domain operand is rebuilt on the device every call.
 * bias [N] or NULL; act 0 none, 1 leaky relu, 3 ADD to what is in y.  Reduction channels % 32 == 0, output channels % 64 == 0. */
VSTAB_API size_t vstab_conv3x3_winograd_workspace_bytes(int B, int H, int W, int cin, int cout, int transpose);
VSTAB_API int vstab_conv3x3_winograd(const float *x, int B, int H, int W, int cs_x, int cx_off, const float *Wf, int cin, int cout, int transpose,
                                     const float *bias, float *y, int cs_y, int cy_off, int act, void *workspace, size_t workspace_bytes,
                                     void *stream);
/* Filter gradient of the same 3x3 stride-1 pad-1 layer in the Winograd domain: V = B^T d B of the input tiles, dM = A dY A^T of the
 * output-gradient tiles, the 16 position gradients dU_xi = V_xi^T dM_xi as ONE batched reduction on the weight-gradient MFMA
 * kernel (4/9 of the direct filter gradient's multiply-adds), dW = G^T dU G.  dW: HWIO [3][3][cin][cout], overwritten.
 * x: [B,H,W,cs_x] channels cx_off..+cin; gout: [B,H,W,cs_g] channels cg_off..+cout; channel counts multiples of 4. */
VSTAB_API size_t vstab_conv3x3_winograd_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout);
VSTAB_API int vstab_conv3x3_winograd_wgrad(const float *x, int B, int H, int W, int cs_x, int cx_off, int cin, const float *gout, int cs_g,
                                           int cg_off, int cout, float *dW, void *workspace, size_t workspace_bytes, void *stream);
/* din (+)= gain * (adjoint of tf.image.resize_images(., [oh,ow]))(dout): backward of the legacy bilinear resize. */
VSTAB_API int vstab_resize_bilinear_backward(const float *dout, int B, int oh, int ow, int C, float *din, int h, int w, float gain,
                                             int accumulate, void *stream);
/* PadLayer(1) -> nearest-neighbour resize (align_corners=True) to H x W (model.py:795-802, 882-884), and its adjoint. C % 4 == 0. */
VSTAB_API int vstab_pad_nearest_upsample(const float *src, int B, int h2, int w2, int C, float *out, int H, int W, void *stream);
VSTAB_API int vstab_pad_nearest_upsample_backward(const float *dout, int B, int H, int W, int C, float *dsrc, int h2, int w2, int accumulate,
                                                  void *stream);
/* The full-resolution head (model.py:882-887) through its tap table, as the inference path computes it: T [B,h2,w2,32] with
 * T[s][tap*2+o] = sum_c concat2[s][c] W[tap][c][o] (a 1x1 conv, vstab_conv_forward); pf2 [B,H-2,W-2,2] = bias + the nine
 * gathered taps + eight adds of the upsampled pf3 [B,h3,w3,2].  The backward of the gather: dT from the flow gradient
 * g [B,H-2,W-2,cs_g] (channels 0,1), columns 18..31 zeroed. */
VSTAB_API int vstab_pf2_from_taps(const float *T, int B, int h2, int w2, const float *bias2, const float *pf3, int h3, int w3, float *pf2,
                                  int H, int W, void *stream);
VSTAB_API int vstab_pf2_taps_backward(const float *g, int cs_g, int B, int H, int W, float *dT, int h2, int w2, void *stream);
/* The tap table itself as vstab_flownets_forward computes it (csrc/tap_panel.hip; model.py:882-885's 3x3 head applied per SOURCE pixel):
 * T [M,32] = concat2 [M,196] x table, M = B*h2*w2 pixel rows of 196 floats (194 channels + 2 of padding), table [200][32] on the device with
 * table[c][tap*2+o] = W[tap][c][o] for c < 194, zero elsewhere (rows 194..199 and columns 18..31).  concat2 and T 16-byte aligned,
 * M*784 < 2^31. */
VSTAB_API int vstab_predict2_tap_table(const float *concat2, long long M, const float *table, float *T, void *stream);
/* out[c] (+)= sum over the rows of g[row*cs + c_off + c] (bias gradients), deterministic two-stage reduction. */
VSTAB_API size_t vstab_column_sum_scratch_bytes(long long rows, int C);
VSTAB_API int vstab_column_sum(const float *g, long long rows, int cs, int c_off, int C, float *out, int accumulate, void *scratch,
                               size_t scratch_bytes, void *stream);
/* tf.train.AdamOptimizer update (main:333-335) on a flat tensor; lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) is the caller's. */
VSTAB_API int vstab_adam_step(float *w, const float *g, float *m, float *v, long long n, float lr_t, float beta1, float beta2, float eps,
                              void *stream);

/* BatchNormLayer(act=lrelu 0.1, is_train=True, gamma_init=None) (model.py:809...) IN PLACE on channels c_off..c_off+C of
 * an NHWC tensor viewed as [rows, cs]: batch mean / population variance (tf.nn.moments), y = lrelu((z-mean)*rsqrt(var+eps)
 * + beta), moving = moving*decay + batch*(1-decay) (moving_* may be NULL).  save_mean / save_rstd [C] feed the backward. */
VSTAB_API size_t vstab_bn_scratch_bytes(long long rows, int C);
VSTAB_API int vstab_bn_lrelu_train_forward(float *zy, long long rows, int cs, int c_off, int C, const float *beta, float *moving_mean,
                                           float *moving_var, float decay, float eps, float *save_mean, float *save_rstd, void *scratch,
                                           size_t scratch_bytes, void *stream);
/* The same layer with is_train=False (outputs_test, main:185), IN PLACE on the same slice: y = lrelu((z - moving_mean) * rstd + beta)
 * with rstd = (float)(1 / sqrt((double)moving_var + (double)eps)).  Writes nothing but the slice -- the moving statistics are only
 * read -- and needs no scratch.  As for the training entry: VSTAB_E_STATE for a NULL buffer; VSTAB_E_SHAPE for rows < 1, C < 1,
 * c_off < 0 or c_off + C > cs; VSTAB_E_ALIGN unless C, cs and c_off are multiples of 4 and zy, beta, moving_mean and moving_var are
 * 16-byte aligned. */
VSTAB_API int vstab_bn_lrelu_inference_forward(float *zy, long long rows, int cs, int c_off, int C, const float *beta,
                                               const float *moving_mean, const float *moving_var, float eps, void *stream);
/* The training-mode layer's backward: dy (gradient w.r.t. y, channels cg_off..+C of a [rows, cs_g] tensor) is overwritten by the gradient w.r.t.
 * the layer's input z; dbeta [C] = sum dy*lrelu'(y) (may be NULL).  y: the forward's output (xhat is recovered from it). */
VSTAB_API int vstab_bn_lrelu_train_backward(const float *y, int cs_y, int cy_off, float *dy, int cs_g, int cg_off, int C, long long rows,
                                            const float *beta, const float *save_rstd, float *dbeta, int accumulate, void *scratch,
                                            size_t scratch_bytes, void *stream);
/* dy *= (y > 0 ? 1 : 0.1): leaky-relu backward for layers without BatchNorm. */
VSTAB_API int vstab_lrelu_backward(const float *y, int cs_y, int cy_off, float *dy, int cs_g, int cg_off, int C, long long rows, void *stream);

/* scipy.signal.medfilt(np.squeeze(of), k) (evaluate_medianNma, main_flownetS_pyramid.py:809): order filter over a
 * kh x kw x kc window of each [h,w,2] field -- kc spans the channel axis; the reference's scalar 5 means 5x5x5 --
 * zero padded on all axes, output = element n/2 of the sorted window.  Odd sizes, kh,kw <= 31, kc <= 5; out != flow. */
VSTAB_API int vstab_flow_medfilt(const float *flow, int B, int h, int w, int kh, int kw, int kc, float *out, void *stream);
/* out[b,:,:,c] = mean over the image of flow[b,:,:,c] (main_flownetS_pyramid_highTV_noBBloss.py:629). */
VSTAB_API int vstab_flow_mean_fill(const float *flow, int B, int h, int w, float *out, void *stream);

/* Homography evaluator (main:728-743, main = main_flownetS_pyramid_noprevloss_dataloader.py): replaces
 *   h, mask = cv2.findHomography(gridmesh, gridmesh - flow, cv2.RANSAC)        (main:735)
 * on the dense [B,H,W,2] flow with a deterministic on-device RANSAC: K (<= 512) 4-point hypotheses per sample drawn
 * by a counter hash of `seed`, consensus = pixels (every `stride`-th) whose reprojection error is <= thresh (cv2's
 * default is 3.0), then `refine` (1..16) least-squares refits on the inlier set.  Hout[b][9] = row-major src->dst
 * matrix with h33 = 1 (float64, device), inliers[b] = size of the last consensus set (0: nothing fitted, Hout NaN).
 * cv2's own RNG cannot be reproduced, so the hypotheses differ from cv2's; the estimator is the same. */
VSTAB_API size_t vstab_homography_workspace_bytes(int B, int H, int W, int K);
VSTAB_API int vstab_homography_fit(const float *flow, int B, int H, int W, int K, unsigned seed, double thresh, int refine,
                                   int stride, double *Hout, int32_t *inliers, void *workspace, size_t workspace_bytes,
                                   void *stream);
/* cv2.warpPerspective(src, Hm[b], (ow, oh)) with default flags on uint8 [B,sh,sw,3] frames (main:736): INTER_LINEAR on
 * coordinates rounded to 1/32 px, 15-bit fixed-point blend, constant-0 border; Hm maps src -> dst (inverted inside). */
VSTAB_API int vstab_warp_perspective_u8(const uint8_t *src, int B, int sh, int sw, const double *Hm, uint8_t *dst, int oh, int ow,
                                        void *stream);

/* ==================================================================================================================
 * DIAGNOSTIC AND TEST SURFACE -- not part of the drop-in contract.  Nothing below is needed to run the path; these calls
 * exist for A/B measurements, profiles and tests, they hold context-global (plan flags, per-launch events) or PROCESS-global
 * (roctx ranges, the HBM-side profiler) state, and the plan flags change the ORDER of floating-point sums (results stay
 * within the parity tolerance but are not bit-identical across flag values).  A product caller leaves all of them alone.
 * ================================================================================================================== */

/* ---- plan flags (A/B measurements and the bit-equality tests; 3 = the round-3 schedule): VSTAB_PLAN_NO_SKINNY keeps few-row
 * layers on the tiled kernel with a split-K combine launch, VSTAB_PLAN_NO_DUAL launches a refinement level's flow head and
 * transposed convolution one after the other, VSTAB_PLAN_NO_TAIL keeps vstab_stabilise_originalsize's last two launches apart (it changes
 * no sum: A/B of the fused tail).  Context state; workspace sizes then come from vstab_workspace_bytes_ctx. */
#define VSTAB_PLAN_NO_SKINNY 1u
#define VSTAB_PLAN_NO_DUAL 2u      /* a refinement level as four launches (tap table, predict_up, transposed conv, combine) instead of two */
#define VSTAB_PLAN_NO_TAIL 4u      /* vstab_stabilise_originalsize: predict_flow2's gather and the glue + warp as two launches (bit-identical) */
#define VSTAB_PLAN_NO_WDEC 8u      /* transposed convolutions as four direct sub-pixel phases, never in Winograd F(2x2,2x2) form (round 6) */
#define VSTAB_PLAN_FORCE_WDEC 16u  /* deconv4 / deconv3 in Winograd F(2x2,2x2) form whatever their size (tests: small shapes) */
#define VSTAB_PLAN_CONV1_FP32 32u  /* conv1 on the fp32 MFMA (conv_rowwin.hip) instead of six bf16 piece-products per multiply on the bf16 MFMA
                                    * (conv1_bf16x3.hip: fp32 operands split into three bf16 pieces, fp32 accumulation); the A side of its A/B */
#define VSTAB_PLAN_NO_WINO_STREAM 64u  /* the 16 Winograd-domain GEMMs of every F(2x2,3x3) stage as one tiled launch, never as streams of positions
                                        * (wino_gemm_stream.hip); same sums in the same order (bit-identical), same workspace: the plan is unchanged */
VSTAB_API int vstab_set_plan_flags(vstab_ctx *ctx, unsigned flags);

/* The 16 Winograd-domain GEMMs of a 3x3 stride-1 stage by themselves, without the transforms around them: M[b][xi] = V[b][xi] . U[xi] for the
 * positions xi = 0..15 of the transformed 4x4 tile.  V [B][16][T][cin], U [16][cin][cout] plain row-major, M [B][16][T][cout], all in device
 * memory and 16-byte aligned; every tensor below 2 GiB; cin % 32 == 0, cout % 64 == 0.  U is packed on the device into the first
 * 16*cin*cout*4 bytes of the workspace (16 positions x [cin/32][cout][32], the layout vstab_load_weights gives a stage's operand) and both
 * forms read that operand: form 0 = the tiled launch (128x64 tiles, zero bias, no split-K), form 1 = streams of positions
 * (csrc/wino_gemm_stream.hip) with the number of positions per workgroup vstab_host_wino_stream_positions() gives -- VSTAB_E_SHAPE,
 * and no launch, when that is 0.  workspace: vstab_wino_domain_gemm_workspace_bytes() bytes, 256-byte aligned (VSTAB_E_NOMEM when smaller;
 * the query returns 0 for a shape the call refuses).  VSTAB_E_STATE for a NULL buffer, VSTAB_E_ALIGN for a misaligned one. */
VSTAB_API size_t vstab_wino_domain_gemm_workspace_bytes(int B, int T, int cin, int cout);
VSTAB_API int vstab_wino_domain_gemm(const float *V, const float *U, float *M, int B, int T, int cin, int cout, int form, void *workspace,
                                     size_t workspace_bytes, void *stream);
/* The stream launcher itself with a caller-chosen number of positions per workgroup (wpk: an operand packed as above): VSTAB_E_SHAPE, and
 * no launch, unless P is what vstab_host_wino_stream_positions() gives for the shape. */
VSTAB_API int vstab_wino_gemm_stream_launch(const float *V, const float *wpk, float *M, int B, int T, int cin, int cout, int P, void *stream);

/* conv1 alone, in the form this context's plan flags choose (six bf16 piece-products on the bf16 MFMA, or VSTAB_PLAN_CONV1_FP32's fp32 MFMA):
 * feats [B][H][W][Cin] -> channels c_off .. c_off + 64 of out [B][Ho][Wo][cs_out]; the other channels of a pixel are not touched.
 * VSTAB_E_SHAPE when the geometry is one the row-window kernels do not take (the forward then runs the generic kernel). */
VSTAB_API int vstab_conv1_forward(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *out, int cs_out, int c_off,
                                  void *stream);

/* ---- measurement support.  With profiling enabled every conv-like launch of
 * vstab_flownets_forward (15 per forward: encoder stages 1..6_1, deconv5..2, predict2 tap
 * table; the GEMM kernel itself, not the split-K combine that may follow it) is bracketed by
 * hipEvents recorded on the forward's stream.  vstab_profile_read must be called after that stream has been
 * synchronised: it returns, both summed over the forward passes recorded since the last
 * reset (a batch split into chunks records one pass per chunk; *n_forwards counts them), the
 * elapsed milliseconds per launch slot and the ALGORITHMIC flops per slot (2*MAC of the layer
 * as SURVEY.md 8d counts it; deconvs at 4 taps/output). */
VSTAB_API int vstab_profile_enable(vstab_ctx *ctx, int enable);
VSTAB_API int vstab_profile_reset(vstab_ctx *ctx);
VSTAB_API int vstab_profile_read(vstab_ctx *ctx, double *ms_sum15, double *flops15, int *n_forwards);
/* vstab_profile_read's flops are what the launches ISSUE: the 3x3 stride-1 encoder stages run in Winograd F(2x2,3x3) form and
 * issue 4/9 of the direct convolution's multiply-adds.  This returns the same slots counted as direct convolutions. */
VSTAB_API int vstab_profile_read_direct(vstab_ctx *ctx, double *flops15);
/* Name (as rocprofv3 prints it) of the kernel instantiation launch slot `slot` used in the last forward. */
VSTAB_API int vstab_profile_kernel_name(vstab_ctx *ctx, int slot, char *buf, int cap);

/* ---- device self-test of the glue's division by a launch constant (five fused operations on a host-side reciprocal instead
 * of a run-time IEEE division; quotients that do not come out normal -- signed zeros, denormals, infinities -- take the division
 * itself): compares it BIT FOR BIT with `x / d` for the `count` fp32 bit patterns x starting at `first_bits` (NaN numerators
 * skipped), and ADDS the number of mismatches to *bad_count_dev (device memory, 8-byte aligned).
 * VSTAB_E_SHAPE for a divisor the glue would divide plainly (outside [1, 2^24], or an all-ones significand). */
VSTAB_API int vstab_selftest_div_const(float d, unsigned first_bits, unsigned long long count, unsigned long long *bad_count_dev,
                                       void *stream);

/* ---- roctx ranges: with on = 1 every layer of vstab_flownets_forward (conv1 .. conv6_1, predict_flowN+upsample, deconvN,
 * predict_flow2) and the glue/warp launches run inside a named roctx range, so a `rocprofv3 --marker-trace --kernel-trace`
 * timeline reads as the network (model.py:807-887).  The roctx library is loaded with dlopen on first use; VSTAB_E_STATE if
 * none is installed.  Process-wide, off by default. */
VSTAB_API int vstab_trace_ranges(int on);

/* ---- instrumentation of the HBM-side kernels (tf_warp, the flow glue, the fused launch): with profiling on every such launch
 * is bracketed by dispatch-timestamp events on its own stream.  Process-wide; switching it on clears earlier records.
 * Slots: 0 = vstab_warp_flow, 1 = vstab_flow_resize_scale, 2 = vstab_flow_glue_warp, 3 = the predict_flow2 gather inside
 * vstab_flownets_forward / vstab_pf2_from_taps (128 B per tap-table row + 8 B per coarser-flow and output pixel).  Read after synchronising the stream(s):
 * summed kernel milliseconds, number of launches, summed ALGORITHMIC bytes (warp 32 B/px; glue 8 B per source +
 * 8 B per output pixel; fused 8 B per source pixel + 32 (flow written) or 24 B per output pixel). */
VSTAB_API int vstab_hbm_profile_enable(int mode);   /* 0 = off (records kept), 1 = clear + on, 2 = on again (records kept) */
VSTAB_API int vstab_hbm_profile_read(int slot, double *ms_sum, int *launches, double *alg_bytes_sum);

/* ---- host-only helpers (no GPU needed; used by the CPU tests) --------------------- */
/* Level sizes of the encoder for an HxW input: hw[2*i], hw[2*i+1] = (h, w) of stage i
 * (10 stages).  Returns 0 or VSTAB_E_SHAPE. */
/* host-only: the XCD-aware workgroup -> tile map the MFMA kernels apply (dispatch-order id `lin` of a gx x gy x gz grid ->
 * tile coordinates xyz[3]); exported so that its bijectivity and banding can be tested without a GPU. */
VSTAB_API int vstab_host_xcd_remap(int gx, int gy, int gz, int lin, int32_t *xyz);
VSTAB_API int vstab_level_sizes(int H, int W, int32_t *hw20);

/* Host-side view of one conv-like launch of the forward schedule (layer 0-9 = encoder
 * stages 1..6_1, 10-13 = deconv5..2, 14 = predict2 tap table, 15-18 = predict6..3 tap tables):
 * writes 26 + 7*nphase ints
 *   B Hi Wi Cs_in KH NSEG SEG SEGP SEG_STRIDE s_in s_out Ho Wo Cs_out c_off N Npad act
 *   nphase ksplit Mmax tile vec4 in_buf out_buf reserved, then per phase
 *   Hg Wg M off_y off_x o_y o_x
 * (buffers index vstab_workspace_layout entries, -1 = feats).  Returns ints written. */
VSTAB_API int vstab_host_layer_plan(int B, int H, int W, int Cin, int layer, int32_t *out, int cap);
/* the same under a pinned plan batch / plan flags (vstab_set_plan_batch, vstab_set_plan_flags); `reserved` = 1 when the stage runs in
 * Winograd form; tile 6 = the weight-stream kernel of few-row layers (conv_skinny.hip: 32- or 64-row x 32-column workgroups) */
VSTAB_API int vstab_host_layer_plan_pinned(int plan_batch, unsigned flags, int B, int H, int W, int Cin, int layer, int32_t *out, int cap);

/* Host-side weight packing exactly as vstab_load_weights does it for `layer` of a
 * Cin-channel network: W is the reference-layout tensor, scale (may be NULL = ones) the
 * folded BatchNorm scale per output channel.  Writes the packed floats ([phase][KT][Npad][32])
 * to `wpk` (capacity `cap` floats) and returns the number of floats, or a negative error. */
VSTAB_API long long vstab_host_pack_layer(int Cin, int layer, const float *W, const double *scale,
                                          float *wpk, long long cap);

/* The transposed convolution of refinement level l (0..3 = deconv5..deconv2) in Winograd F(2x2,2x2) form (csrc/winograd_ops.hip):
 * the 9-position GEMM's plan in vstab_host_layer_plan's format (26 ints + 7 per position; `reserved` = 1 when the default plan of this
 * problem chooses the form) followed by the tile geometry {NTy, NTx, nty[3], ntx[3]}; and its packed operands as vstab_load_weights
 * builds them (W = the reference-layout filter [4][4][Cout][Cin]; 9 positions x [KT][4 Cout][32]). */
VSTAB_API int vstab_host_wdec_plan(int B, int H, int W, int Cin, int l, int32_t *out, int cap);
VSTAB_API long long vstab_host_pack_wdec(int l, const float *W, const double *scale, float *wpk, long long cap);
/* The same operands for arbitrary channel counts: W [4][4][cout][cin], input pixels of cs_in >= cin floats (rows cin .. cs_in of every
 * position are zeros); 9 positions x [round_up(cs_in, 32) / 32][4 cout][32] floats.  vstab_host_pack_wdec(l, ...) is this call with level
 * l's channel counts. */
VSTAB_API long long vstab_host_pack_wdec_shape(const float *W, const double *scale, int cin, int cs_in, int cout, float *wpk, long long cap);

/* A refinement level's flow head by itself (csrc/flow_ops.hip: predict_flowN + upsample_flowN in one launch; the forward's launch_predict_up
 * without a combine or an inverse transform riding along).  taps: the tap table T [B][h][w][32] (T[.., 2 tap + o], tap = 3 dy + dx; columns
 * 18..31 are not read) or its `ks` split-K slabs `slab_stride` floats apart (even; at least one table when ks > 1), summed in slab order.
 * out [B][h][w][2] = bias2[o] + the in-image taps T[y+dy-1, x+dx-1, 2 tap + o] in (dy, dx) order, then, with prev [B][ph][pw][2] != NULL,
 * (.. + u) + u with u the legacy-bilinear sample of prev.  Then the 4x4 stride-2 SAME transposed convolution 2 -> 2 of `out` with the HOST
 * arrays up_w [4][4][co][ci] (64 floats) and up_b (2 floats), cropped to oh x ow (oh <= 2 h, ow <= 2 w), written as (u, v, 0, 0) into the four
 * floats at c_off of concat [B][oh][ow][Cs]; the other floats of a pixel are not touched.  bias2 is a device pointer.  VSTAB_E_SHAPE for
 * Cs % 4, c_off % 4, c_off + 4 > Cs, ks < 1, oh > 2 h, ow > 2 w or a tensor of 2 GiB; VSTAB_E_STATE for a NULL buffer (prev may be NULL);
 * VSTAB_E_ALIGN unless taps, prev and out are 8-byte and concat 16-byte aligned.  A refused call launches nothing. */
VSTAB_API int vstab_predict_up(const float *taps, int ks, long long slab_stride, int B, int h, int w, const float *bias2, const float *prev, int ph,
                               int pw, float *out, const float *up_w, const float *up_b, float *concat, int oh, int ow, int Cs, int c_off,
                               void *stream);
/* vstab_predict_up's arguments without the batch and the stream, for vstab_deconv4x4_winograd's `head` */
typedef struct vstab_predict_up_args {
    const float *taps; int ks; long long slab_stride; int h, w; const float *bias2; const float *prev; int ph, pw; float *out;
    const float *up_w; const float *up_b; float *concat; int oh, ow, Cs, c_off;
} vstab_predict_up_args;

/* A 4x4 stride-2 SAME transposed convolution in Winograd F(2x2,2x2) form by itself (csrc/winograd_ops.hip documents the algebra), through
 * the forward's launchers: the input transform, the 9-position GEMM on the 128x128 (tile = 0) or 64x128 (tile = 1) tile with a zero bias,
 * the inverse transform + bias + activation (act 0 = none, 1 = leaky relu 0.1).  x [B][Hi][Wi][cs_in]; wpk = a device copy of
 * vstab_host_pack_wdec_shape's operands; bias [cout]; the result goes to channels c_off .. c_off + cout of out [B][Ho][Wo][cs_out], the
 * other channels are not touched.  head == NULL: the inverse transform is a launch of its own; otherwise it rides in the flow head's launch
 * (the forward's wdec_output_predict_up_kernel) with *head's arguments and this call's B.  workspace:
 * vstab_deconv4x4_winograd_workspace_bytes() bytes, 256-byte aligned (the transformed tiles V [B][9][NTy][NTx][cs_in] at its start, the
 * GEMM's result M [B][9][NTy][NTx][4 cout] at the next multiple of 256 bytes, then the zero bias; NT = Ho / 4 + 1 per axis; tiles a
 * position does not need are left as they were; the query returns 0 for a shape the call refuses).  VSTAB_E_SHAPE for cs_in % 4, 4 cout not a multiple of 128 or above 2048, Ho not in {2 Hi - 1, 2 Hi} (Wo
 * likewise), cs_out % 4, c_off % 4, c_off + cout > cs_out, tile or act not 0 / 1, a tensor of 2 GiB, or a head vstab_predict_up refuses;
 * VSTAB_E_STATE for a NULL buffer; VSTAB_E_ALIGN unless every tensor is 16-byte aligned; VSTAB_E_NOMEM for a short workspace.  A refused
 * call launches nothing. */
VSTAB_API size_t vstab_deconv4x4_winograd_workspace_bytes(int B, int Hi, int Wi, int cs_in, int Ho, int Wo, int cout);
VSTAB_API int vstab_deconv4x4_winograd(const float *x, int B, int Hi, int Wi, int cs_in, const float *wpk, const float *bias, int act, float *out,
                                       int Ho, int Wo, int cs_out, int c_off, int cout, int tile, const vstab_predict_up_args *head,
                                       void *workspace, size_t workspace_bytes, void *stream);

/* Positions per workgroup of the stream form of a Winograd stage's 16 GEMMs (csrc/wino_gemm_stream.hip) for B samples of T tiles, cin -> cout
 * channels: 16, 8, 4 or 2, or 0 when the stage does not qualify (the forward then takes the tiled launch). */
VSTAB_API int vstab_host_wino_stream_positions(int B, int T, int cin, int cout);
/* How a filter gradient is launched (csrc/wgrad_mfma.hip), without a HIP call: out4 = {n_main, n_tail, ks_main, ks_tail} -- the columns and
 * the split-K count of the launches vstab_conv_wgrad makes for M = k*k*cin rows, cout columns and a reduction over K = B*Ho*Wo output pixels
 * (n_tail = ks_tail = 0: one launch).  nbatch = 0 or 1: that plain form; nbatch = 16: {cout, 0, ksplit, 0} of the 16-plane batched launch
 * vstab_conv3x3_winograd_wgrad makes for M = cin and K = B*ceil(H/2)*ceil(W/2) tiles.  VSTAB_E_SHAPE for anything else, or a shape the
 * batched form refuses. */
VSTAB_API int vstab_host_wgrad_split(int M, int cout, int K, int nbatch, int *out4);
/* The launches vstab_conv_forward (dgrad = 0) or vstab_conv_dgrad (dgrad = 1) makes for a geometry, without a HIP call.  x is the image
 * side (the forward's input, the input gradient's dx: Hi x Wi, cin of cs_x channels), y the output side (the forward's y, gout: Ho x Wo,
 * cout of cs_y channels; the forward takes Ho = Wo = 0 as the symmetric-pad size); c_off = channel offset of the tensor the launches
 * WRITE (the offset on the side they read only moves a pointer); act = the forward's epilogue / the input gradient's accumulate flag.
 * Writes 7 ints
 *   launches packed_floats part_floats blocked_K tbl_nfast workspace_bytes/256 table_entries
 * then per launch 8 ints
 *   nphase tile vec4 ksplit Mmax N Npad operand_offset(floats)
 * each followed by 12 per phase
 *   Hg Wg M off_y off_x o_y o_x KH NSEG SEG SEGP SEG_STRIDE
 * and, when `table` is not NULL, the gather table (table_entries ints: 0 = a zero, i > 0 = element i - 1 of the filter) that the
 * operand is packed through every call (none when blocked_K > 0).  Returns the ints written to `out`, or the entry point's own
 * refusal of the geometry (VSTAB_E_NOMEM: `cap` / `table_cap` too small) with both buffers untouched. */
VSTAB_API int vstab_host_train_conv_plan(int dgrad, int B, int Hi, int Wi, int cs_x, int cin, int k, int stride, int pad, int Ho, int Wo,
                                         int cs_y, int cout, int c_off, int act, int32_t *out, int cap, int32_t *table, long long table_cap);
/* The Winograd-domain operand of a 3x3 stride-1 stage as vstab_load_weights packs it: W [3][3][cin][cout], scale (may be NULL = ones) per
 * output channel; 16 positions x [cin/32][cout][32] floats to `wpk`.  Returns the number of floats, or a negative error. */
VSTAB_API long long vstab_host_pack_winograd(const float *W, const double *scale, int cin, int cout, float *wpk, long long cap);

/* ---- theta regressors (model.py:152-184 Localizer, :375-455 dense_homo, :897-1024 flownetS_prehomo / _variableWeight), inference ----
 * The blocks those graphs need beside vstab_conv_forward (csrc/theta_ops.hip).  Shared refusals, judged in this order and before any
 * launch: VSTAB_E_STATE for a NULL buffer, VSTAB_E_SHAPE for a size outside the contract, VSTAB_E_ALIGN for a misaligned buffer,
 * VSTAB_E_NOMEM for a short workspace. */

/* tf.pad(x, [[0,0],[p,p],[p,p],[0,0]], "SYMMETRIC") (PadLayer, model.py:907...): x [B,H,W,C] contiguous, any C >= 1 ->
 * y [B,H+2p,W+2p,cs_y] with y[i] = x[-i-1] before the edge and x[2H-1-i] after it (the edge sample repeated), channels C..cs_y-1
 * zeroed.  p = 0 is the channel-padding copy.  0 <= p <= min(H, W), cs_y >= C and cs_y % 4 == 0, B*(H+2p)*(W+2p)*cs_y < 2^31; y 16-byte
 * aligned (x: 4-byte; 16-byte accesses on x when C % 4 == 0 and x is 16-byte aligned). */
VSTAB_API int vstab_pad_symmetric(const float *x, int B, int H, int W, int C, int p, float *y, int cs_y, void *stream);

/* BatchNormLayer(act = lrelu(slope), is_train = False, gamma_init = None) IN PLACE on channels c_off..c_off+C of a [rows, cs] view:
 * y = act((z - moving_mean) * rstd + beta), act(u) = u >= 0 ? u : slope * u, rstd as in vstab_bn_lrelu_inference_forward.
 * twice != 0: the layer's input passes the activation first, y = act(bn(act(z))) -- DenseLayer(act = lrelu) -> BatchNormLayer(act = lrelu),
 * model.py:953-956, 409-412.  Refusals as vstab_bn_lrelu_inference_forward. */
VSTAB_API int vstab_bn_lrelu_slope_inference(float *zy, long long rows, int cs, int c_off, int C, const float *beta, const float *moving_mean,
                                             const float *moving_var, float eps, float slope, int twice, void *stream);
/* The same arithmetic fused with MaxPool2d((2,2),(2,2),'SAME'): z [B,H,W,C] contiguous -> out [B,ceil(H/2),ceil(W/2),C], the window clipped
 * at an odd edge as in vstab_maxpool2x2; z is read once and not written.  C % 4 == 0, B*H*W*C < 2^31, 16-byte aligned buffers. */
VSTAB_API int vstab_bn_lrelu_slope_pool_inference(const float *z, int B, int H, int W, int C, const float *beta, const float *moving_mean,
                                                  const float *moving_var, float eps, float slope, int twice, float *out, void *stream);

/* DenseLayer: y [B,N] = act(x [B,K] . W [K,N] + b [N]), W on the device in the reference's layout, read exactly once per call.
 * act: VSTAB_DENSE_IDENTITY, _LRELU (u >= 0 ? u : slope * u), _TANH, _TANH_AFFINE (tanh(u / 1000) * scale[n] + shift[n], dense_homo's tail,
 * model.py:381, 413-420; scale and shift are read by that act only).  1 <= B <= 32, K >= 4 and K % 4 == 0, N >= 1, K * N < 2^40.
 * K is cut into slabs that depend on K and N alone; each slab's partial sums go to the workspace and a second launch adds them in slab
 * order: no atomics, equal bits from call to call, and a row's bits do not depend on B.
 * workspace: vstab_dense_forward_workspace_bytes(B, K, N) bytes (0 for a shape the call refuses), 16-byte aligned; x and y 16-byte aligned. */
#define VSTAB_DENSE_IDENTITY    0
#define VSTAB_DENSE_LRELU       1
#define VSTAB_DENSE_TANH        2
#define VSTAB_DENSE_TANH_AFFINE 3
VSTAB_API size_t vstab_dense_forward_workspace_bytes(int B, int K, int N);
VSTAB_API int vstab_dense_forward(const float *x, int B, int K, int N, const float *W, const float *b, int act, float slope, const float *scale,
                                  const float *shift, float *y, void *workspace, size_t workspace_bytes, void *stream);
/* The slab plan of vstab_dense_forward for (K, N), without a HIP call: rows of W per slab and the number of slabs (0 when refused). */
VSTAB_API int vstab_host_dense_plan(int K, int N, int32_t *slab_rows, int32_t *slabs);

#ifdef __cplusplus
}
#endif
#endif /* VSTAB_H */

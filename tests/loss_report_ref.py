"""A numpy fp64 restatement of what the test pass of the reference's `train()` reads, written from the reference's text and sharing
no code with the package or `oracle/`: `lossterm` with its second return value `warpedimg` (main:200-210; "main" =
main_flownetS_pyramid_noprevloss_dataloader.py), `tf_warp` (main:70-130), `masked_MSE` (main:188-198), the total variation
(main:269-273), the per-level scalars loss6..loss2 / var6..var2 and their sum (main:275, 346-356), `fix_image_tf` (utils.py:434) and
BatchNormLayer(act=lrelu 0.1, is_train=False) (model.py:809).  tests/test_loss_report_ref_cpu.py holds it against the oracle.

Also the inputs of tests/test_gpu_loss_report.py (`gpu_case`), so that the CPU test can price that test's exclusion zone from the
oracle alone."""
import numpy as np

LEVELS = ("predict_flow6", "predict_flow5", "predict_flow4", "predict_flow3", "predict_flow2")


def resize_legacy(x, oh, ow):
    """tf.image.resize_images(x, [oh, ow]) of TF 1.x (bilinear, align_corners=False, no half-pixel centres): the source coordinate
    o * (in / out) and its fraction are fp32, as the op computes them; the blend is done here in x's type."""
    B, h, w, C = x.shape

    def axis(n_in, n_out):
        f = np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))
        lo = np.floor(f)
        t = (f - lo).astype(x.dtype)
        lo = lo.astype(np.int64)
        return lo, np.minimum(lo + 1, n_in - 1), t

    ylo, yhi, ty = axis(h, oh)
    xlo, xhi, tx = axis(w, ow)
    ty, tx = ty.reshape(1, oh, 1, 1), tx.reshape(1, 1, ow, 1)
    top = x[:, ylo][:, :, xlo] + (x[:, ylo][:, :, xhi] - x[:, ylo][:, :, xlo]) * tx
    bot = x[:, yhi][:, :, xlo] + (x[:, yhi][:, :, xhi] - x[:, yhi][:, :, xlo]) * tx
    return top + (bot - top) * ty


def tf_warp(img, flow):
    """main:70-130: sample point = pixel grid + flow in fp32 (the graph's tensors), corners by truncation, all four clipped, weights
    from the CLIPPED corners; the blend in img's type (fp64 here)."""
    B, H, W, _ = img.shape
    flow = np.asarray(flow, np.float32)
    x = np.arange(W, dtype=np.float32).reshape(1, 1, W) + flow[..., 0]
    y = np.arange(H, dtype=np.float32).reshape(1, H, 1) + flow[..., 1]
    x0, y0 = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)
    y0, y1 = np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
    b = np.arange(B).reshape(B, 1, 1)
    Ia, Ib, Ic, Id = img[b, y0, x0], img[b, y1, x0], img[b, y0, x1], img[b, y1, x1]
    xd, yd = x.astype(img.dtype), y.astype(img.dtype)
    wa = ((x1 - xd) * (y1 - yd))[..., None]
    wb = ((x1 - xd) * (yd - y0))[..., None]
    wc = ((xd - x0) * (y1 - yd))[..., None]
    wd = ((xd - x0) * (yd - y0))[..., None]
    return wa * Ia + wb * Ib + wc * Ic + wd * Id


def masked_mse(pred, gt, mask):
    """main:188-198"""
    mse = ((pred * mask - gt * mask) ** 2).sum(axis=(1, 2, 3))
    safe = np.where(mask == 0, mask + 1e-8, mask)
    return (mse / safe.sum(axis=(1, 2, 3))).mean()


def lossterm(flow, stab, unstab):
    """main:200-210 -> (masked_MSE, warpedimg)"""
    h, w = flow.shape[1], flow.shape[2]
    ds = resize_legacy(np.asarray(stab, np.float64), h, w)
    du = resize_legacy(np.asarray(unstab, np.float64), h, w)
    warped = tf_warp(du, flow)
    mask = tf_warp(np.ones_like(du), flow)
    return masked_mse(warped, ds, mask), warped


def total_variation(flow):
    """tf.image.total_variation summed over the batch (main:269)"""
    f = np.asarray(flow, np.float64)
    return np.abs(f[:, 1:] - f[:, :-1]).sum() + np.abs(f[:, :, 1:] - f[:, :, :-1]).sum()


def level_terms(flows, stab, unstab, target_channels, target_weights, tv_weights):
    """(mse [5], tv [5], total, per_target [T]): per level sum_t c_t * lossterm(flow, stab[..., off_t:off_t+3], unstab) and
    tv_weight * TV (the summary scalars of main:346-356), their sum over the levels (main:275), and every target's unweighted share."""
    mse, tv, per = [], [], np.zeros(len(target_channels))
    for name, tvw in zip(LEVELS, tv_weights):
        terms = [lossterm(flows[name], stab[..., o:o + 3], unstab)[0] for o in target_channels]
        per += np.asarray(terms)
        mse.append(sum(c * t for c, t in zip(target_weights, terms)))
        tv.append(tvw * total_variation(flows[name]))
    return np.asarray(mse), np.asarray(tv), float(np.sum(mse) + np.sum(tv)), per


def fix_image(image, norm_value):
    """utils.py:434 tf.cast(image / norm_value * 255., tf.uint8): truncation toward zero, saturated to 0..255 first (the cast is
    undefined outside)."""
    return np.trunc(np.clip(np.asarray(image) / norm_value * 255.0, 0.0, 255.0)).astype(np.uint8)


def bn_lrelu_inference(z, beta, moving_mean, moving_var, eps=1e-5):
    """BatchNormLayer(act=lrelu 0.1, is_train=False, gamma_init=None): tf.nn.batch_normalization on the moving statistics, no gamma"""
    z = np.asarray(z, np.float64)
    y = (z - moving_mean) * (1.0 / np.sqrt(np.asarray(moving_var, np.float64) + eps)) + beta
    return np.maximum(y, 0.1 * y)


# ----------------------------------------------------------------------------- the inputs of tests/test_gpu_loss_report.py
GPU_B, GPU_H, GPU_W = 2, 71, 97
GPU_SIZES = ((1, 1), (2, 3), (5, 7), (18, 25), (71, 97))     # the last: 6887 > 256 * 16 pixels, two workgroups per sample, ragged tail
GPU_SEED = 20


def gpu_case():
    """(flows {level: [B,h,w,2]}, stab [B,H,W,24], unstab [B,H,W,3]), float32 from one seeded generator.  Sample 0's flows are uniform
    in +-0.6 of the level's size, so a good share of its sample points leave the frame; every flow of sample 1 points more than
    twice the level's size outside (M == 0 everywhere: the safe_mask branch, an all-zero warped frame)."""
    rng = np.random.default_rng(GPU_SEED)
    stab = rng.random((GPU_B, GPU_H, GPU_W, 24), dtype=np.float32)
    unstab = rng.random((GPU_B, GPU_H, GPU_W, 3), dtype=np.float32)
    flows = {}
    for name, (h, w) in zip(LEVELS, GPU_SIZES):
        r = rng.random((GPU_B, h, w, 2), dtype=np.float32)
        size = np.asarray([w, h], np.float32)
        f = np.empty_like(r)
        f[0] = (r[0] - np.float32(0.5)) * np.float32(1.2) * size
        f[1] = r[1] + np.float32(2.0) * size + np.float32(3.0)
        flows[name] = f
    return flows, stab, unstab


def near_quantisation_step(v255, width=1e-3):
    """Where 255 * warpedimg lies within `width` of a step of saturate-then-truncate: the integers 1..255.  (At 0 the saturation
    leaves no step: everything in (-1, 1) maps to 0.)"""
    k = np.rint(v255)
    return (np.abs(v255 - k) <= width) & (k >= 1) & (k <= 255)

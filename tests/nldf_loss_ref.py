"""numpy restatement of NLDF's objective (NLDF.py:79-100: contour term, IoU loss, softmax cross-entropy, accuracy; :136-171:
sobel_filter, im_gradient, Loss_IoU, Loss_Contour, L2) and of its gradient with respect to Score, written from the semantics and not
from the kernels: an explicit one-pixel pad, tap-by-tap 3x3 correlations, and for the gradient the adjoint accumulated over the PADDED
image and then folded back onto the border pixels.  Every function takes the dtype it computes in (float32 or float64); float64 is the
yardstick of the GPU tests and float32's deviation from it their unit.

Tensors are NHWC.  The gradient takes the derivative of a Sobel magnitude that is exactly 0 as 0 (the library's documented departure
from TensorFlow, whose inf * 0 is NaN there)."""
import numpy as np

FX = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.float64)
FY = FX.T.copy()
CONTOUR_TH = 1.5


def sobel_filter():
    """The two [3,3,2,1] float32 depthwise filters of NLDF.py:136-149."""
    fx = np.stack((FX, FX), axis=2).reshape(3, 3, 2, 1).astype(np.float32)
    fy = np.stack((FY, FY), axis=2).reshape(3, 3, 2, 1).astype(np.float32)
    return fx, fy


def pad1(im):
    """tf.pad(im, [[0,0],[1,1],[1,1],[0,0]], 'SYMMETRIC'): for a pad of one, the edge pixel repeated."""
    return np.pad(im, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")


def _correlate(xp, f, H, W):
    acc = np.zeros((xp.shape[0], H, W, xp.shape[3]), dtype=xp.dtype)
    for a in range(3):
        for b in range(3):
            if f[a, b] != 0:
                acc += xp.dtype.type(f[a, b]) * xp[:, a:a + H, b:b + W, :]
    return acc


def sobel_gxy(im, dtype=np.float64):
    im = np.asarray(im, dtype=dtype)
    H, W = im.shape[1], im.shape[2]
    xp = pad1(im)
    return _correlate(xp, FX, H, W), _correlate(xp, FY, H, W)


def im_gradient(im, dtype=np.float64):
    """NLDF.py:151-156, [B,H,W,C] -> [B,H,W,C]."""
    gx, gy = sobel_gxy(im, dtype)
    return np.sqrt(gx * gx + gy * gy).astype(dtype)


def _fold(dxp):
    """adjoint of pad1: the pad's rows and columns are added onto the edge pixels they repeat."""
    d = dxp.copy()
    d[:, 1] += d[:, 0]
    d[:, -2] += d[:, -1]
    d = d[:, 1:-1]
    d[:, :, 1] += d[:, :, 0]
    d[:, :, -2] += d[:, :, -1]
    return d[:, :, 1:-1]


def _correlate_adjoint(a, f):
    B, H, W, C = a.shape
    dxp = np.zeros((B, H + 2, W + 2, C), dtype=a.dtype)
    for i in range(3):
        for j in range(3):
            if f[i, j] != 0:
                dxp[:, i:i + H, j:j + W, :] += a.dtype.type(f[i, j]) * a
    return dxp


def im_gradient_grad(im, dout, dtype=np.float64):
    """d sum(dout * im_gradient(im)) / d im; a pixel of magnitude 0 passes nothing."""
    gx, gy = sobel_gxy(im, dtype)
    mag = np.sqrt(gx * gx + gy * gy)
    dout = np.asarray(dout, dtype=dtype)
    safe = np.where(mag > 0, mag, dtype(1))
    ax = np.where(mag > 0, dout * gx / safe, dtype(0)).astype(dtype)
    ay = np.where(mag > 0, dout * gy / safe, dtype(0)).astype(dtype)
    return _fold(_correlate_adjoint(ax, FX) + _correlate_adjoint(ay, FY)).astype(dtype)


def softmax(score, dtype=np.float64):
    s = np.asarray(score, dtype=dtype)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(dtype)


def log_softmax(score, dtype=np.float64):
    s = np.asarray(score, dtype=dtype)
    m = s.max(axis=-1, keepdims=True)
    return (s - (m + np.log(np.exp(s - m).sum(axis=-1, keepdims=True)))).astype(dtype)


def label_grad_sum(label, dtype=np.float64):
    """sum_c im_gradient(label)_c, [B,H,W,1]: what is compared with contour_th."""
    return im_gradient(label, dtype).sum(axis=-1, keepdims=True, dtype=dtype)


def loss_iou(pred, gt, dtype=np.float64):
    """NLDF.py:158-165's else branch (`inter == 0` compares a tensor object with an int and is never true)."""
    pred, gt = np.asarray(pred, dtype=dtype), np.asarray(gt, dtype=dtype)
    inter = (pred * gt).sum(dtype=dtype)
    union = (pred * pred).sum(dtype=dtype) + (gt * gt).sum(dtype=dtype)
    return dtype(1) - dtype(2) * (inter + dtype(1)) / (union + dtype(1))


def loss_iou_grad(pred, gt, dtype=np.float64):
    pred, gt = np.asarray(pred, dtype=dtype), np.asarray(gt, dtype=dtype)
    inter = (pred * gt).sum(dtype=dtype)
    union = (pred * pred).sum(dtype=dtype) + (gt * gt).sum(dtype=dtype)
    u1 = union + dtype(1)
    return (dtype(-2) * gt / u1 + dtype(4) * (inter + dtype(1)) * pred / (u1 * u1)).astype(dtype)


def loss_contour(pred, gt, dtype=np.float64):
    """NLDF.py:167-168."""
    pred, gt = np.asarray(pred, dtype=dtype), np.asarray(gt, dtype=dtype)
    e = dtype(1e-5)
    return (-gt * np.log(pred + e) - (dtype(1) - gt) * np.log(dtype(1) - pred + e)).mean(dtype=dtype)


def loss_contour_grad(pred, gt, dtype=np.float64):
    pred, gt = np.asarray(pred, dtype=dtype), np.asarray(gt, dtype=dtype)
    e = dtype(1e-5)
    return ((-gt / (pred + e) + (dtype(1) - gt) / (dtype(1) - pred + e)) / dtype(pred.size)).astype(dtype)


def l2(t, wd, dtype=np.float64):
    """NLDF.py:170-171 / vgg16.py:99-100: wd * sum(t^2) / 2."""
    t = np.asarray(t, dtype=dtype)
    return dtype(wd) * (t * t).sum(dtype=dtype) / dtype(2)


def l2_grad(t, wd, dtype=np.float64):
    return (dtype(wd) * np.asarray(t, dtype=dtype)).astype(dtype)


def saliency_loss(score, label, contour_th=CONTOUR_TH, dtype=np.float64):
    """dict of Loss_Mean, C_IoU_LOSS, CE, accuracy, correct (the count behind accuracy), Prob_Grad, label_Grad [B,H,W,1] and
    label_sum (what the threshold is applied to)."""
    score, label = np.asarray(score, dtype=dtype), np.asarray(label, dtype=dtype)
    P = softmax(score, dtype)
    prob_grad = np.tanh(im_gradient(P, dtype).sum(axis=-1, keepdims=True, dtype=dtype)).astype(dtype)
    lsum = label_grad_sum(label, dtype)
    lab_grad = (lsum > dtype(contour_th)).astype(dtype)
    iou = loss_iou(prob_grad, lab_grad, dtype)
    ce = (-(label * log_softmax(score, dtype)).sum(axis=-1, dtype=dtype)).mean(dtype=dtype)
    correct = int((np.argmax(score, axis=-1) == np.argmax(label, axis=-1)).sum())          # np.argmax: the first of equal maxima
    npix = score.shape[0] * score.shape[1] * score.shape[2]
    return {"Loss_Mean": dtype(iou + ce), "C_IoU_LOSS": dtype(iou), "CE": dtype(ce), "accuracy": dtype(correct) / dtype(npix),
            "correct": correct, "Prob_Grad": prob_grad, "label_Grad": lab_grad, "label_sum": lsum}


def saliency_loss_grad(score, label, contour_th=CONTOUR_TH, dtype=np.float64):
    """d Loss_Mean / d score, [B,H,W,2]; label_Grad carries no gradient."""
    score, label = np.asarray(score, dtype=dtype), np.asarray(label, dtype=dtype)
    P = softmax(score, dtype)
    S = im_gradient(P, dtype).sum(axis=-1, keepdims=True, dtype=dtype)
    pred = np.tanh(S).astype(dtype)
    gt = (label_grad_sum(label, dtype) > dtype(contour_th)).astype(dtype)
    dS = (loss_iou_grad(pred, gt, dtype) * (dtype(1) - pred * pred)).astype(dtype)            # through tanh
    dP = im_gradient_grad(P, np.broadcast_to(dS, P.shape), dtype)                             # the channel sum broadcasts dS
    dscore = P * (dP - (P * dP).sum(axis=-1, keepdims=True, dtype=dtype))                     # softmax Jacobian
    npix = score.shape[0] * score.shape[1] * score.shape[2]
    dscore = dscore + (P * label.sum(axis=-1, keepdims=True, dtype=dtype) - label) / dtype(npix)
    return dscore.astype(dtype)

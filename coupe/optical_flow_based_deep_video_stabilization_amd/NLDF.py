"""Drop-in for the reference's `NLDF.py` (`Model.build_model`, NLDF.py:24-101): VGG16 trunk + the
non-local deep-feature saliency head at the reference's hard-wired 352x352 geometry.  The reference
never instantiates this model and the file only runs under Python 2 (`k_s / 2` as a pad width,
NLDF.py:132); it is provided because BASELINE.json's north_star names it.  Variable names follow the
TF scopes: `<layer>/W`, `<layer>/b` for Fea_Global_1, Fea_Global_2, Fea_Global, Fea_P1..5,
Fea_P2_Deconv..Fea_P5_Deconv, Local_Fea, Local_Score, Global_Score.

The objective the reference's build_model spells out (NLDF.py:79-100: contour term, IoU loss, softmax cross-entropy, accuracy) is
`Model.build_loss` and the module-level `saliency_loss`; `Model.sobel_filter`, `im_gradient`, `Loss_IoU`, `Loss_Contour` and `L2`
(:136-171) are its pieces, each differentiable through a HIP backward (nldf_loss.py).

The net is trainable end to end: `Model.backward` walks the head in reverse (vstab_nldf_backward) from the
gradient at Score to the five pools and the 30 head variables and hands the pool gradients to `Vgg16.backward`; `Model.pools_grad` is
the head walk alone; `Model.forward` is the autograd entry on top of both."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, nldf_loss, runtime, vgg16
from .nldf_loss import SaliencyLoss, saliency_loss  # noqa: F401  (the module-level entry of the fused loss)

img_size = 352
label_size = img_size // 2
FEA = 128

HEAD_SHAPES = {
    "Fea_Global_1/W": (5, 5, 512, FEA), "Fea_Global_2/W": (5, 5, FEA, FEA), "Fea_Global/W": (3, 3, FEA, FEA),
    "Fea_P1/W": (3, 3, 64, FEA), "Fea_P2/W": (3, 3, 128, FEA), "Fea_P3/W": (3, 3, 256, FEA),
    "Fea_P4/W": (3, 3, 512, FEA), "Fea_P5/W": (3, 3, 512, FEA),
    "Fea_P5_Deconv/W": (5, 5, FEA, 2 * FEA), "Fea_P4_Deconv/W": (5, 5, 2 * FEA, 3 * FEA),
    "Fea_P3_Deconv/W": (5, 5, 3 * FEA, 4 * FEA), "Fea_P2_Deconv/W": (5, 5, 4 * FEA, 5 * FEA),
    "Local_Fea/W": (1, 1, 6 * FEA, 5 * FEA), "Local_Score/W": (1, 1, 5 * FEA, 2), "Global_Score/W": (1, 1, FEA, 2),
}


# the 30 variables in the order of vstab_nldf_backward's dparams30: W then b of each layer of HEAD_SHAPES
PARAM_NAMES = tuple(n for w in HEAD_SHAPES for n in (w, w[:-1] + "b"))


def shape_of(name: str):
    """Shape of a head variable: HEAD_SHAPES for a filter; a bias has its layer's output channels (a transposed convolution's filter is
    [5,5,out,in])."""
    if name.endswith("/W"):
        return HEAD_SHAPES[name]
    shp = HEAD_SHAPES[name[:-1] + "W"]
    return (shp[2] if "Deconv" in name else shp[3],)


def synthetic_head_weights(seed: int = 11, gain: float = 1.0) -> Dict[str, np.ndarray]:
    """Variables of the head with the reference's initialisers scaled by `gain` (truncated normal
    stddev 0.01 for convs, NLDF.py:105-108; normal 0.01 for deconvs, :121-123; zero biases would make
    every bias path invisible to tests, so biases are small random numbers)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in HEAD_SHAPES.items():
        w = rng.standard_normal(shp)
        if "Deconv" not in name:
            w = np.clip(w, -2.0, 2.0)
        out[name] = (w * 0.01 * gain).astype(np.float32)
        cout = shp[2] if "Deconv" in name else shp[3]
        out[name[:-1] + "b"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
    return out


class _ForwardFn(torch.autograd.Function):
    """Model.forward: build_model forward, Model._backward backward.  `handle` is the model's one-element leaf that keeps a trainable
    net in the graph when the input itself needs no gradient; it never receives one."""

    @staticmethod
    def forward(ctx, model, x, handle):
        model.build_model(x, None)
        ctx.model, ctx.last = model, model._last
        ctx.set_materialize_grads(False)           # an output nothing uses brings None, not a tensor of zeros to walk through
        return model.Score.detach(), model.Prob.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, dscore, dprob):
        m, last = ctx.model, ctx.last
        need_input = ctx.needs_input_grad[1]
        if (dscore is None and dprob is None) or not (need_input or m.trainable or m.vgg.trainable):
            return None, None, None
        if dscore is None:
            dscore = torch.zeros_like(last["Score"])
        dev = last["x"].device
        head = m._grad_tensors(dev) if m.trainable else None
        trunk = m.vgg._grad_tensors(dev) if m.vgg.trainable else None
        dinput = m._backward(last, dscore, dprob, None, None, need_input, head, trunk, accumulate=True)
        return None, dinput, None


class Model:
    def __init__(self, vgg16_npy_path: Optional[str] = None, vgg_data_dict: Optional[dict] = None,
                 head_weights: Optional[Dict[str, np.ndarray]] = None, seed: Optional[int] = None, trainable: bool = False):
        """trainable=True: a backward through forward() accumulates the head variables' gradients into self.grads ({name: CUDA
        tensor}, names as in HEAD_SHAPES plus the '<layer>/b'; zero_grads() clears them, apply_grads(lr) takes an SGD step).  The trunk
        follows self.vgg.trainable."""
        self.trainable = trainable
        self.grads: Dict[str, torch.Tensor] = {}
        self._last = None                  # what the last build_model ran on
        self._params = None                # device-resident masters of the head variables, once apply_grads has stepped them
        self._handle = None
        if vgg_data_dict is None and vgg16_npy_path is None and seed is not None:
            self.vgg = vgg16.Vgg16(seed=seed)
        else:
            self.vgg = vgg16.Vgg16(vgg16_npy_path, data_dict=vgg_data_dict)
        if head_weights is None:
            if seed is None:
                raise ValueError("NLDF.Model needs head_weights (or seed= for synthetic ones): the reference "
                                 "creates them with tf.get_variable and restores a checkpoint that is not available")
            head_weights = synthetic_head_weights(seed)
        self.set_head_weights(head_weights)

    def set_head_weights(self, head_weights: Dict[str, np.ndarray]):
        """Replace the head's variables; the next build_model loads them into the trunk's context again."""
        hw = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in head_weights.items()}
        for k, shp in HEAD_SHAPES.items():
            if k not in hw or hw[k].shape != shp:
                raise ValueError(f"head weight {k}: expected shape {shp}")
        self.head_weights = hw
        self._loaded_on = None
        self._params = None

    def _load(self, ctx):
        if self._loaded_on is ctx:
            return
        w = self.head_weights
        arr = (_lib.VstabTensor * len(w))()
        keep = []
        for i, (name, a) in enumerate(w.items()):
            nb = name.encode()
            keep.append((nb, a))
            arr[i].name = nb
            arr[i].data = a.ctypes.data_as(_lib.c_float_p)
            arr[i].ndim = a.ndim
            for d in range(a.ndim):
                arr[i].shape[d] = a.shape[d]
        _lib.check(_lib.lib().vstab_nldf_load(ctx._h, arr, len(w)), ctx._h)
        self._loaded_on = ctx

    def build_model(self, input_holder, batch_size, reuse=False, scope='NLDF'):
        """input_holder [B,352,352,3] float32 CUDA in [0,1] -> Prob [B,176,176,1] (saliency probability).
        Also sets Fea_Global, Local_Fea, Local_Score+Global_Score = Score, Prob as attributes."""
        x = input_holder
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError("input_holder must be a float32 CUDA tensor [B,352,352,3]")
        if tuple(x.shape[1:]) != (img_size, img_size, 3):
            raise ValueError(f"NLDF is hard-wired to {img_size}x{img_size}x3 inputs (NLDF.py:58-64,74)")
        B = x.shape[0]
        if batch_size is not None and int(batch_size) != B:
            raise ValueError(f"batch_size={batch_size} but input has batch {B}")
        vgg = self.vgg
        vgg.build(vgg16.preprocess(x.contiguous()))                      # NLDF.py:29-31
        ctx = vgg._ctx
        self._load(ctx)
        L = _lib.lib()
        dev = x.device
        self.Prob = torch.empty((B, 176, 176, 1), dtype=torch.float32, device=dev)
        self.Score = torch.empty((B, 176, 176, 2), dtype=torch.float32, device=dev)
        self.Local_Fea = torch.empty((B, 176, 176, 5 * FEA), dtype=torch.float32, device=dev)
        self.Fea_Global = torch.empty((B, 1, 1, FEA), dtype=torch.float32, device=dev)
        nws = L.vstab_nldf_workspace_bytes(B)
        if nws == 0:
            raise ValueError(f"NLDF: unsupported batch {B}")
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        self._ws, self._ws_batch = ws, B                                  # kept for internals()
        pool_t = [vgg.pool1, vgg.pool2, vgg.pool3, vgg.pool4, vgg.pool5]
        pools = (C.c_void_p * 5)(*[t.data_ptr() for t in pool_t])
        with torch.cuda.device(dev):
            _lib.check(L.vstab_nldf_forward(ctx._h, pools, B, self.Prob.data_ptr(), self.Score.data_ptr(),
                                            self.Local_Fea.data_ptr(), self.Fea_Global.data_ptr(), ws.data_ptr(), nws,
                                            runtime.stream_ptr()), ctx._h)
        self._last = {"x": x, "B": B, "ctx": ctx, "ws": ws, "pools": pool_t, "vgg": vgg._last, "Score": self.Score, "Prob": self.Prob,
                      "Local_Fea": self.Local_Fea}
        return self.Prob

    # ---- backward
    def _head_backward(self, last, score_grad, prob_grad, local_fea_grad, fea_global_grad, need_pools, dparams, accumulate):
        """The C walk on the activations `last` recorded.  dparams: 30 tensors in PARAM_NAMES order or None.  Returns the five pool
        gradients, or None."""
        B, dev = last["B"], last["x"].device
        shapes = {"score_grad": (B, label_size, label_size, 2), "prob_grad": (B, label_size, label_size, 1),
                  "local_fea_grad": (B, label_size, label_size, 5 * FEA), "fea_global_grad": (B, 1, 1, FEA)}
        given = {"score_grad": score_grad, "prob_grad": prob_grad, "local_fea_grad": local_fea_grad, "fea_global_grad": fea_global_grad}
        held = {}
        for name, g in given.items():
            if g is None:
                if name == "score_grad":
                    raise ValueError("score_grad is missing: pass it or call build_loss() first")
                continue
            if not torch.is_tensor(g) or g.dtype != torch.float32 or g.device != dev or tuple(g.shape) != shapes[name]:
                raise ValueError(f"{name} must be a float32 tensor of shape {shapes[name]} on {dev}")
            held[name] = g.contiguous()
        if not need_pools and dparams is None:
            raise ValueError("neither the pool gradients nor the head variables' gradients are asked for")
        dpools = [torch.empty_like(p) for p in last["pools"]] if need_pools else None
        pptr = (C.c_void_p * 5)(*[p.data_ptr() for p in last["pools"]])
        dpptr = (C.c_void_p * 5)(*[p.data_ptr() for p in dpools]) if need_pools else None
        wptr = (C.c_void_p * 30)(*[p.data_ptr() for p in dparams]) if dparams is not None else None
        ctx = last["ctx"]
        if self._loaded_on is not ctx:
            raise RuntimeError("the head variables were replaced after the build_model this backward refers to")
        with torch.cuda.device(dev):
            ws = runtime.workspace(dev, "vstab_nldf_backward_workspace_bytes", B, 1 if dparams is not None else 0,
                                   refused=f"NLDF backward: unsupported batch {B}")
        runtime.call(dev, "vstab_nldf_backward", ctx._h, pptr, B, last["ws"].data_ptr(), last["ws"].numel(), last["Local_Fea"].data_ptr(),
                     last["Prob"].data_ptr(), held["score_grad"].data_ptr(), runtime.ptr(held.get("prob_grad")),
                     runtime.ptr(held.get("local_fea_grad")), runtime.ptr(held.get("fea_global_grad")), dpptr, wptr, 1 if accumulate else 0,
                     ws.data_ptr(), ws.numel(), ctx=ctx._h)
        return dpools

    def _backward(self, last, score_grad, prob_grad, local_fea_grad, fea_global_grad, need_input, head_dparams, trunk_dparams, accumulate):
        """Head walk, then the trunk's; returns dinput (with respect to input_holder: preprocess's factor 255 included) or None."""
        need_trunk = need_input or trunk_dparams is not None
        dpools = self._head_backward(last, score_grad, prob_grad, local_fea_grad, fea_global_grad, need_trunk, head_dparams, accumulate)
        if not need_trunk:
            return None
        dpre = self.vgg._backward(last["vgg"], {f"pool{k + 1}": g for k, g in enumerate(dpools)}, need_input, trunk_dparams, accumulate)
        if dpre is None:
            return None
        dinput = torch.empty_like(dpre)
        runtime.call(dpre.device, "vstab_axpby", dpre.data_ptr(), 255.0, dpre.data_ptr(), 0.0, dinput.data_ptr(), dpre.numel())
        return dinput

    def _need_last(self, who):
        if self._last is None:
            raise RuntimeError(f"{who}() needs a build_model() call first")
        return self._last

    def _default_score_grad(self, score_grad):
        if score_grad is None:
            score_grad = getattr(self, "Score_grad", None)
            if score_grad is None:
                raise ValueError("score_grad is None and build_loss() has not been called")
        return score_grad

    def _fresh_head_grads(self, dev):
        return [torch.zeros(shape_of(n), dtype=torch.float32, device=dev) for n in PARAM_NAMES]

    def pools_grad(self, score_grad=None, prob_grad=None, local_fea_grad=None, fea_global_grad=None, need_head_weights=False):
        """The head walk alone (a frozen trunk): ([d pool1 .. d pool5], {variable: gradient} or None) of the last build_model.
        score_grad=None takes self.Score_grad of build_loss; the other three are optional gradients at Prob, Local_Fea, Fea_Global."""
        last = self._need_last("pools_grad")
        dparams = self._fresh_head_grads(last["x"].device) if need_head_weights else None
        dpools = self._head_backward(last, self._default_score_grad(score_grad), prob_grad, local_fea_grad, fea_global_grad, True, dparams, False)
        return dpools, (dict(zip(PARAM_NAMES, dparams)) if need_head_weights else None)

    def backward(self, score_grad=None, prob_grad=None, local_fea_grad=None, fea_global_grad=None, need_input=False,
                 need_trunk_weights=False, need_head_weights=True):
        """Back-propagates through the last build_model: (dinput [B,352,352,3] with respect to input_holder or None, {head variable:
        gradient} or None, {trunk layer: (dW, db)} or None).  score_grad=None takes self.Score_grad of build_loss."""
        last = self._need_last("backward")
        dev = last["x"].device
        if not (need_input or need_trunk_weights or need_head_weights):
            raise ValueError("no gradient is asked for")
        head = self._fresh_head_grads(dev) if need_head_weights else None
        trunk = None
        if need_trunk_weights:
            trunk = [t for _, ci, co in vgg16.LAYERS for t in (torch.zeros((3, 3, ci, co), dtype=torch.float32, device=dev),
                                                              torch.zeros(co, dtype=torch.float32, device=dev))]
        dinput = self._backward(last, self._default_score_grad(score_grad), prob_grad, local_fea_grad, fea_global_grad, need_input, head, trunk,
                                accumulate=False)
        return (dinput, dict(zip(PARAM_NAMES, head)) if head is not None else None,
                {name: (trunk[2 * i], trunk[2 * i + 1]) for i, (name, _, _) in enumerate(vgg16.LAYERS)} if trunk is not None else None)

    def forward(self, input_holder):
        """build_model under torch.autograd: (Score, Prob) attached to the graph.  Their backward gives d/d input_holder when it
        requires grad, accumulates the head variables' gradients into self.grads for a trainable model and the trunk's into
        self.vgg.grads when self.vgg.trainable: saliency_loss(Score, label).backward() then trains the net."""
        x = runtime.f32_cuda(input_holder, "input_holder", rank=4, last=3, layout="[B,352,352,3]")
        if not torch.is_grad_enabled() or not (x.requires_grad or self.trainable or self.vgg.trainable):
            self.build_model(x, None)
            return self.Score, self.Prob
        if self._handle is None or self._handle.device != x.device:
            self._handle = torch.zeros(1, dtype=torch.float32, device=x.device, requires_grad=True)
        return _ForwardFn.apply(self, x, self._handle)

    def _grad_tensors(self, device):
        if not self.grads or next(iter(self.grads.values())).device != device:
            self.grads = {n: torch.zeros(shape_of(n), dtype=torch.float32, device=device) for n in PARAM_NAMES}
        return [self.grads[n] for n in PARAM_NAMES]

    def zero_grads(self):
        for g in self.grads.values():
            g.zero_()

    def export_head_weights(self) -> Dict[str, np.ndarray]:
        """The head variables as a numpy dict: the stepped ones once apply_grads has run."""
        if self._params is None:
            return {k: v.copy() for k, v in self.head_weights.items()}
        return {k: v.cpu().numpy() for k, v in self._params.items()}

    def apply_grads(self, lr: float):
        """One plain SGD step p -= lr * grad on device-resident masters of the head variables (vstab_axpby).  The packed operands
        the forward reads are built by the host packers of vstab_nldf_load, so the stepped variables then go through
        set_head_weights (one host round trip, as Vgg16.apply_grads)."""
        if not self.grads:
            raise RuntimeError("Model.apply_grads: no gradients (trainable=True and a backward through forward() fill them)")
        dev = next(iter(self.grads.values())).device
        if self._params is None or next(iter(self._params.values())).device != dev:
            self._params = {n: torch.from_numpy(self.head_weights[n]).to(dev) for n in PARAM_NAMES}
        for n in PARAM_NAMES:
            p, g = self._params[n], self.grads[n]
            runtime.call(dev, "vstab_axpby", p.data_ptr(), 1.0, g.data_ptr(), -float(lr), p.data_ptr(), p.numel())
        params = self._params
        self.set_head_weights(self.export_head_weights())
        self._params = params

    # ---- the objective (NLDF.py:79-100, :136-171): nldf_loss.py over csrc/nldf_loss_ops.hip
    def sobel_filter(self):
        """NLDF.py:136-149: the depthwise Sobel filters (fx, fy), each [3,3,2,1] float32 (host tensors; the kernels hold the taps)."""
        fx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float32)
        fy = fx.t().contiguous()
        return tuple(torch.stack((f, f), dim=2).reshape(3, 3, 2, 1) for f in (fx, fy))

    def im_gradient(self, im):
        """NLDF.py:151-156 on a float32 CUDA tensor [B,H,W,C], 1 <= C <= 4: per channel sqrt(gx^2 + gy^2) of the two 3x3 Sobel
        correlations of the one-pixel SYMMETRIC pad (clamp to edge).  Differentiable; a pixel whose magnitude is exactly 0 passes no
        gradient (TensorFlow: NaN)."""
        return nldf_loss.im_gradient(im)

    def Loss_IoU(self, pred, gt):
        """NLDF.py:158-165: 1 - 2 (sum pred gt + 1) / (sum pred^2 + sum gt^2 + 1) over every element, a 0-dim tensor.  The reference's
        `if inter == 0: return 0` compares a tensor object with an int, which is never true in TF 1.x: the else branch is the
        function.  Differentiable with respect to pred; a gt that requires grad raises."""
        return nldf_loss.loss_iou(pred, gt)

    def Loss_Contour(self, pred, gt):
        """NLDF.py:167-168: mean(-gt log(pred + 1e-5) - (1 - gt) log(1 - pred + 1e-5)).  Differentiable with respect to pred; a gt that
        requires grad raises."""
        return nldf_loss.loss_contour(pred, gt)

    def L2(self, tensor, wd=0.0005):
        """NLDF.py:170-171: wd * sum(tensor^2) / 2 (the product the reference's `tf.mul`, gone from TF 1.x, names).  Differentiable."""
        return nldf_loss.l2(tensor, wd)

    def build_loss(self, label_holder, contour_th=1.5):
        """The loss graph of NLDF.py:79-100 on the Score of the last build_model and label_holder [B,176,176,2] (per pixel a distribution
        over the two classes).  Sets label_holder, contour_th, Prob_Grad, label_Grad [B,176,176,1], C_IoU_LOSS, CE, Loss_Mean = C_IoU_LOSS +
        CE, accuracy (0-dim) and Score_grad = d Loss_Mean / d Score [B,176,176,2], all from one fused call.  Score has no autograd graph behind
        it here: Model.backward() takes Score_grad from this call through the head into the trunk and the variables (Model.forward() +
        saliency_loss() is the autograd form of the same).  Returns Loss_Mean."""
        if getattr(self, "Score", None) is None:
            raise RuntimeError("build_loss() needs a build_model() call first")
        if not torch.is_tensor(label_holder) or tuple(label_holder.shape) != tuple(self.Score.shape):
            raise ValueError(f"label_holder must be a float32 CUDA tensor {list(self.Score.shape)}")
        scalars, pg, lg, dscore = nldf_loss.saliency_loss_call(self.Score, label_holder, contour_th, True, True)
        self.label_holder, self.contour_th = label_holder, float(contour_th)
        self.Prob_Grad, self.label_Grad, self.Score_grad = pg, lg, dscore
        self.Loss_Mean, self.C_IoU_LOSS, self.CE, self.accuracy = scalars[0], scalars[1], scalars[2], scalars[3]
        return self.Loss_Mean

    def internals(self):
        """Views (no copy, no launch) of the head's intermediate tensors in the workspace of the last build_model (tests):
        G1 [B,7,7,128], G2 [B,3,3,128], cat1..cat5 = [Fea_Pk | Fea_Pk_LC | Fea_P(k+1)_Up] ([B,176,176,768] .. [B,11,11,256]),
        Local_Score [B,176,176,2], Global_Score [B,1,1,2]."""
        if getattr(self, "_ws", None) is None:
            raise RuntimeError("internals() needs a build_model() call first")
        views = workspace_views(self._ws, self._ws_batch)
        del views["Local_Fea"]                # build_model has it written to self.Local_Fea: the workspace's copy is never touched
        return views


def workspace_views(ws: torch.Tensor, B: int) -> Dict[str, torch.Tensor]:
    """Named views into a vstab_nldf_forward workspace `ws` (uint8) of batch B, by vstab_nldf_workspace_layout."""
    ent = (_lib.VstabWsEntry * 16)()
    n = _lib.lib().vstab_nldf_workspace_layout(B, ent, 16)
    if n < 0:
        _lib.check(n)
    out = {}
    for e in ent[:n]:
        name = e.name.decode()
        if e.h == 0:                          # the split-K partial sums
            continue
        nfl = e.n * e.h * e.w * e.c_stride
        flat = ws[e.offset_bytes:e.offset_bytes + 4 * nfl].view(torch.float32)
        out[name] = flat.view(e.n, e.h, e.w, e.c_stride)[..., :e.c]
    return out

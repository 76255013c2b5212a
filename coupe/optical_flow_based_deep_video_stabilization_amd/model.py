"""Drop-in for the reference's `model.flownetS_pyramid` (model.py:786-893).

Same name, argument order, NHWC shapes and returned dict keys; eager torch tensors on
the current HIP device instead of TF graph tensors.  All arithmetic runs in
libvstab_hip.so (hand-written HIP for gfx950); torch only owns the buffers.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import runtime, weights as _weights


def flownetS_pyramid(feats, batch_size, is_train=False, reuse=False, scope='flownetS'):
    """feats [B,H,W,C_in] float32 in [0,1] (channels 0-23 = 8 stabilised history frames,
    24-26 = current frame; main:550-558) -> dict with 'predict_flow6' ... 'predict_flow2'
    and 'flow' (= predict_flow2), model.py:893.

    `batch_size` only sized the deconv output_shapes in the reference (model.py:850);
    it must equal feats.shape[0].  `reuse` is accepted and ignored (no variable scopes
    here).  `is_train=False` is the inference path (BatchNorm on the moving statistics,
    folded into the conv weights); `is_train=True` (main:184) runs the training-mode forward
    of the scope's `train_step.Trainer` -- BatchNorm on batch statistics, moving averages
    updated -- whose `loss_and_backward` / `adam` / `step` continue from there."""
    if not torch.is_tensor(feats):
        raise TypeError("feats must be a torch tensor")
    if feats.dim() != 4:
        raise ValueError("feats must be [B,H,W,C]")
    if batch_size is not None and int(batch_size) != feats.shape[0]:
        raise ValueError(f"batch_size={batch_size} but feats has batch {feats.shape[0]}")
    if is_train:
        from . import train_step
        tr = train_step.get_trainer(scope, feats.shape[0], feats.shape[1], feats.shape[2])
        out = {k: v.contiguous() for k, v in tr.forward(feats).items()}
        out['flow'] = out['predict_flow2']
        return out
    ctx = runtime.get_context(scope, feats.device.index if feats.is_cuda else None)
    pf6, pf5, pf4, pf3, pf2 = ctx.forward(feats)
    return {'predict_flow6': pf6, 'predict_flow5': pf5, 'predict_flow4': pf4, 'predict_flow3': pf3,
            'predict_flow2': pf2, 'flow': pf2}


# ---- the theta regressors (reference model.py:152-184, 375-455, 897-1024): inference forward in theta_runtime.py
def _theta_forward(net, feats, is_train, scope, batch_size=None, last_act=None, out_param_dim=None):
    if not torch.is_tensor(feats):
        raise TypeError("feats must be a torch tensor")
    if feats.dim() != 4:
        raise ValueError("feats must be [B,H,W,C]")
    if batch_size is not None and int(batch_size) != feats.shape[0]:
        raise ValueError(f"batch_size={batch_size} but feats has batch {feats.shape[0]}")
    if is_train:
        raise NotImplementedError(f"{net}(is_train=True): only the inference graph (BatchNorm on the moving statistics) is built; the "
                                  f"training-mode forward and the backward of the theta regressors are a follow-up")
    from . import theta_runtime
    tn = theta_runtime.get_net(net, scope, feats.device.index if feats.is_cuda else None)
    if out_param_dim is not None and int(out_param_dim) != tn.units[-1]:
        raise ValueError(f"{net}: out_param_dim={out_param_dim}, but the assigned {tn.graph.dense[-1].name}/W has {tn.units[-1]} units")
    return tn.forward(feats, last_act)


def Localizer(feats, out_param_dim, is_train=False, reuse=False, is_tanh=False, scope='Localizer'):
    """model.py:152-184: feats [B,H,W,C] -> [B,out_param_dim], the theta of an AffineTransformer (6) or ProjectiveTransformer (8).
    Five VALID 3x3 convolutions (the first stride 2) need H, W >= 19.  `out_param_dim` must be the one the assigned `df/dense2`
    has; `is_tanh` puts tanh on that layer.  `reuse` is accepted and ignored."""
    return _theta_forward('Localizer', feats, is_train, scope, last_act='tanh' if is_tanh else 'identity', out_param_dim=out_param_dim)


def flownetS_prehomo(feats, batch_size, is_train=False, reuse=False, scope='dense_homo'):
    """model.py:897-959: feats [B,H,W,C] -> [B,8].  `batch_size` sized the reference's reshape and must equal feats.shape[0]."""
    return _theta_forward('flownetS_prehomo', feats, is_train, scope, batch_size)


def flownetS_variableWeight(feats, batch_size, is_train=False, reuse=False, scope='dense_homo'):
    """model.py:962-1024, the same graph and variables as `flownetS_prehomo`."""
    return _theta_forward('flownetS_variableWeight', feats, is_train, scope, batch_size)


def dense_homo(feats, is_train=False, reuse=False, scope='dense_homo'):
    """model.py:375-455: feats [B,H,W,C] -> [B,8], the theta `ProjectiveTransformer(out_size).transform(img, theta)` takes
    (flownet_trainer.py:422-426).  Only conv2_3 / bn2_3 / pool2 and the dense layers are computed: the reference's other
    convolutions read the input and feed nothing.  The batch is feats' (the reference reshapes to config.batch_size)."""
    return _theta_forward('dense_homo', feats, is_train, scope)


# ---- variable handling: stand-ins for tl.layers.initialize_global_variables (main:517)
# ---- and tl.files.load_and_assign_npz_dict (main:520)
def initialize_global_variables(seed: int = 1, cin: int = 27, random_bn: bool = False, flow_gain: float = 1.0,
                                scope: Optional[str] = None, net: Optional[str] = None, H: int = 384, W: int = 512,
                                out_param_dim: Optional[int] = None, dense_std: float = 0.1) -> Dict[str, np.ndarray]:
    """Seeded synthetic variables with the graph's initialisers (no checkpoint is
    available offline, README.md:24).  `net` names a theta regressor ('Localizer', 'flownetS_prehomo', 'flownetS_variableWeight',
    'dense_homo'; None = flownetS_pyramid): its first dense layer is sized for H x W inputs, `out_param_dim` is Localizer's, and
    `scope` defaults to the builder's own."""
    if net is not None:
        from . import theta_nets, theta_runtime
        w = theta_nets.synthetic_weights(net, seed, cin, H, W, out_param_dim, random_bn, dense_std)
        return theta_runtime.assign_weights(net, w, scope)
    w = _weights.synthetic_weights(seed, cin, random_bn, flow_gain)
    runtime.assign_weights(w, scope or 'flownetS')
    return w


def load_and_assign_npz_dict(name: str, sess=None, scope: Optional[str] = None, net: Optional[str] = None) -> Dict[str, np.ndarray]:
    """Load a tensorlayer `save_npz_dict` checkpoint (keys `main_net/<scope>/<var>:0`) for flownetS_pyramid, or for the theta
    regressor `net` (dense_homo's unused convolutions may be in the file or not)."""
    if net is not None:
        from . import theta_runtime
        with np.load(name, allow_pickle=False) as z:
            raw = {k: z[k] for k in z.files}
        return theta_runtime.assign_weights(net, raw, scope)
    w = _weights.load_npz_dict(name, scope or 'flownetS')
    runtime.assign_weights(w, scope or 'flownetS')
    return w


def assign_weights(weights: Dict[str, np.ndarray], scope: Optional[str] = None, net: Optional[str] = None) -> None:
    if net is not None:
        from . import theta_runtime
        theta_runtime.assign_weights(net, weights, scope)
        return
    runtime.assign_weights(weights, scope or 'flownetS')

"""fp64 reference of the objective with the previous-frame terms (main_flownetS_pyramid.py:200-250 and the highTV file): built from the
oracle's `lossterm` and `total_variation` and a `training.Objective`, differentiated by torch autograd.
tests/test_loss_prev_ref_cpu.py anchors it on the CPU, tests/test_gpu_loss_prev.py compares the kernels with it.

    loss_main = sum_levels [ sum_t w_t * lossterm(pf_l, stab[..., c_t:c_t+3], unstab) + tv_l * total_variation(pf_l) ]

The gradient bound of the GPU test is the project's bound for `loss_main` (test_gpu_training.py: 2e-5 of the largest reference
gradient of the level, + 1e-9) applied term by term: the kernel forms sum_t w_t * (P - g_t) in float32, so its rounding error scales
with the terms' sizes, not with the possibly cancelling sum.  `term_gradients` returns those per-term reference gradients, the TV part
counted once, in term 0."""
import torch

from oracle import vstab_oracle as vo


def case(B, H, W, sizes, seed, Ct=24, mag=1.5):
    """The inputs of test_gpu_training.py's `_case`, with a Ct-channel stable tensor."""
    g = torch.Generator().manual_seed(seed)
    stab, un = torch.rand(B, H, W, Ct, generator=g), torch.rand(B, H, W, 3, generator=g)
    flows = {n: torch.randn(B, h, w, 2, generator=g) * mag for n, (h, w) in zip(vo.LOSS_LEVELS, sizes)}
    return stab, un, flows


def terms(flows, stab, unstab, objective):
    """([T] per-target lossterms summed over the levels, unweighted; [levels] TV of each flow), fp64, differentiable."""
    per = [0.0] * len(objective.target_channels)
    tv = []
    for name in vo.LOSS_LEVELS:
        for t, c in enumerate(objective.target_channels):
            per[t] = per[t] + vo.lossterm(flows[name], stab[..., c:c + 3], unstab)[0]
        tv.append(vo.total_variation(flows[name]))
    return per, tv


def objective_loss(flows, stab, unstab, objective):
    """(loss_main of `objective`, the per-target lossterms), fp64, differentiable w.r.t. the flows."""
    per, tv = terms(flows, stab, unstab, objective)
    total = sum(w * p for w, p in zip(objective.target_weights, per)) + sum(w * v for w, v in zip(objective.tv_weights, tv))
    return total, per


def pieces(flows, stab, unstab, channels):
    """Everything an objective over these target channels is a linear combination of, computed once (fp64, autograd): per target the
    lossterms summed over the levels and their gradient w.r.t. every flow, per level the total variation and its gradient."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in flows.items()}
    leaves = [leaf[k] for k in vo.LOSS_LEVELS]
    per, per_grads = [], []
    for c in channels:
        f = sum(vo.lossterm(leaf[k], stab[..., c:c + 3], unstab)[0] for k in vo.LOSS_LEVELS)
        g = torch.autograd.grad(f, leaves)
        per.append(float(f.detach()))
        per_grads.append({k: gk.double() for k, gk in zip(vo.LOSS_LEVELS, g)})
    tv, tv_grads = [], {}
    for k in vo.LOSS_LEVELS:
        v = vo.total_variation(leaf[k])
        tv.append(float(v.detach()))
        tv_grads[k] = torch.autograd.grad(v, leaf[k])[0].double() if leaf[k].shape[1] * leaf[k].shape[2] > 1 else torch.zeros_like(leaf[k]).double()
    return {"channels": tuple(channels), "per": per, "per_grads": per_grads, "tv": tv, "tv_grads": tv_grads}


def term_gradients(p, objective):
    """{level: [T] gradients}: d (target t's lossterms [+ the weighted TV terms for t = 0]) / d flow, unweighted by w_t."""
    assert p["channels"] == tuple(objective.target_channels)
    out = {}
    for k, tvw in zip(vo.LOSS_LEVELS, objective.tv_weights):
        out[k] = [g[k] + (tvw * p["tv_grads"][k] if t == 0 else 0.0) for t, g in enumerate(p["per_grads"])]
    return out


def assemble(p, objective):
    """(loss, [T] per-target losses, {level: d loss / d flow}) of `objective` from `pieces`."""
    assert p["channels"] == tuple(objective.target_channels)
    loss = sum(w * v for w, v in zip(objective.target_weights, p["per"])) + sum(w * v for w, v in zip(objective.tv_weights, p["tv"]))
    grads = {}
    for k, tvw in zip(vo.LOSS_LEVELS, objective.tv_weights):
        grads[k] = sum(w * g[k] for w, g in zip(objective.target_weights, p["per_grads"])) + tvw * p["tv_grads"][k]
    return loss, list(p["per"]), grads


def loss_and_gradients(flows, stab, unstab, objective):
    """(loss, [T] per-target losses, {level: d loss / d flow}), fp64."""
    return assemble(pieces(flows, stab, unstab, objective.target_channels), objective)


def gradient_bound(term_grads, objective):
    """2e-5 * sum_t w_t * max|g_t_ref| + 1e-9 for one level's [T] term gradients."""
    return 2e-5 * sum(w * float(g.abs().max()) for w, g in zip(objective.target_weights, term_grads)) + 1e-9

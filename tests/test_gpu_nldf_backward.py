"""NLDF.Model.backward / pools_grad / forward / apply_grads and the C entries under them (vstab_nldf_backward and its stage kernels)
against tests/nldf_head_grad_ref.py (float64 numpy) applied to the activations read back from the device.

Tolerance (DESIGN.md section 21's rule; the same launchers do the work).  The error of a tensor is max|got - ref| / max|ref|.  The
yardstick is the same map in float32 on the CPU (ref.torch_walk on the same read-back activations); a GPU tensor must stay within
FACTOR = 4 x that, never asked to be closer than FLOOR = 2^-22.  DESIGN.md section 22 lists the measured errors.

The reference is computed once per sample (module fixture): the walk is linear in the gradient and a sample's pool gradients depend
on that sample only, so the B=2 reference is the two samples' side by side (pools) and summed (variables), and the B=1 problem is
sample 0 of the same forward, copied into a B=1 workspace: the B=1 and the B=2 call then see identical activations."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import NLDF, _lib, runtime, vgg16
from coupe.optical_flow_based_deep_video_stabilization_amd.nldf_loss import saliency_loss
from tests import nldf_head_grad_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 2.0 ** -22
FEA = 128
HW = (176, 88, 44, 22, 11)
GAIN = 1.2                                   # Score of order 1..10: the default 0.01 scale leaves every gradient near zero
NAMES = NLDF.PARAM_NAMES


def rel(got, want):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    return float(np.abs(got - np.asarray(want, np.float64)).max() / max(np.abs(want).max(), 1e-300))


def make_label(B):
    yy, xx = np.meshgrid(np.arange(176), np.arange(176), indexing="ij")
    lab = np.zeros((B, 176, 176, 2), np.float32)
    for b in range(B):
        fg = ((yy - 70 - 30 * b) ** 2 + (xx - 90 + 20 * b) ** 2) < (40 + 10 * b) ** 2
        lab[b, ..., 0] = fg
        lab[b, ..., 1] = ~fg
    return torch.from_numpy(lab).cuda()


def make_input(B):
    x = torch.rand(B, 352, 352, 3, generator=torch.Generator().manual_seed(1))
    if B > 1:
        x[1] *= torch.linspace(0.2, 1.0, 352)[None, :, None]
    return x.cuda()


def abi_backward(m, last, B, ws_fwd, pools, local_fea, prob, dscore, dprob=None, dlf=None, dfg=None, want_pools=True, want_params=True,
                 accumulate=0, dparams=None, ws=None, ws_bytes=None, ws_fwd_bytes=None):
    """vstab_nldf_backward through ctypes; returns (code, dpools, dparams)."""
    L = _lib.lib()
    dev = dscore.device
    dpools = [torch.full((B, h, h, c), float("nan"), device=dev) for h, c in zip(HW, (64, 128, 256, 512, 512))] if want_pools else None
    if dparams is None and want_params:
        dparams = [torch.full(NLDF.shape_of(n), float("nan"), device=dev) for n in NAMES]
    if ws is None:
        ws = torch.empty(L.vstab_nldf_backward_workspace_bytes(B, 1 if want_params else 0), dtype=torch.uint8, device=dev)
    pp = (C.c_void_p * 5)(*[p.data_ptr() for p in pools])
    dpp = (C.c_void_p * 5)(*[p.data_ptr() for p in dpools]) if want_pools else None
    wp = (C.c_void_p * 30)(*[p.data_ptr() for p in dparams]) if want_params else None
    code = L.vstab_nldf_backward(last["ctx"]._h, pp, B, ws_fwd.data_ptr(), ws_fwd.numel() if ws_fwd_bytes is None else ws_fwd_bytes,
                                 local_fea.data_ptr(), prob.data_ptr(), dscore.data_ptr(), runtime.ptr(dprob), runtime.ptr(dlf), runtime.ptr(dfg),
                                 dpp, wp, accumulate, ws.data_ptr() if torch.is_tensor(ws) else ws, ws.numel() if ws_bytes is None else ws_bytes,
                                 runtime.stream_ptr())
    return code, dpools, dparams


@pytest.fixture(scope="module")
def run():
    B = 2
    dd = vgg16.synthetic_data_dict(seed=5)
    hw = NLDF.synthetic_head_weights(seed=6, gain=GAIN)
    m = NLDF.Model(vgg_data_dict=dd, head_weights=hw)
    x, label = make_input(B), make_label(B)
    m.build_model(x, B)
    loss = m.build_loss(label)
    dscore = m.Score_grad
    last = m._last
    ws_before, lf_before = last["ws"].clone(), m.Local_Fea.clone()
    dpools, head = m.pools_grad(need_head_weights=True)
    torch.cuda.synchronize()
    print(f"Score range {float(m.Score.min()):.3f} .. {float(m.Score.max()):.3f}, Loss_Mean {float(loss):.4f}, max|dscore| {float(dscore.abs().max()):.3e}")
    views = m.internals()
    # the B=1 problem: sample 0 of the same forward in a B=1 workspace
    ws1 = torch.zeros(_lib.lib().vstab_nldf_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    v1 = NLDF.workspace_views(ws1, 1)
    for name, v in views.items():
        v1[name].copy_(v[0:1])
    one = SimpleNamespace(ws=ws1, pools=[p[0:1].contiguous() for p in last["pools"]], local_fea=m.Local_Fea[0:1].contiguous(),
                          prob=m.Prob[0:1].contiguous(), dscore=dscore[0:1].contiguous())
    # per-sample float64 reference and float32 CPU yardstick on the read-back activations
    per = []
    for s in range(B):
        acts = {k: v[s:s + 1].cpu().numpy() for k, v in views.items() if k.startswith("cat") or k in ("G1", "G2", "Fea_Global")}
        acts["pools"] = [p[s:s + 1].cpu().numpy() for p in last["pools"]]
        acts["Local_Fea"], acts["Prob"] = m.Local_Fea[s:s + 1].cpu().numpy(), m.Prob[s:s + 1].cpu().numpy()
        g = dscore[s:s + 1].cpu().numpy()
        per.append((ref.walk(acts, hw, g), ref.torch_walk(acts, hw, g, dtype=torch.float32)))
    (r0, y0), (r1, y1) = per
    ref2 = ([np.concatenate([a, b]) for a, b in zip(r0[0], r1[0])], {n: r0[1][n] + r1[1][n] for n in NAMES})
    yard2 = ([np.concatenate([a, b]) for a, b in zip(y0[0], y1[0])], {n: y0[1][n] + y1[1][n] for n in NAMES})
    return SimpleNamespace(m=m, hw=hw, x=x, label=label, last=last, dscore=dscore, dpools=dpools, head=head, ws_before=ws_before,
                           lf_before=lf_before, one=one, ref={2: ref2, 1: r0}, yard={2: yard2, 1: y0})


def check(tag, run, B, dpools, dparams):
    want, yard = run.ref[B], run.yard[B]
    rows = [(f"dpool{k + 1}", dpools[k], want[0][k], yard[0][k]) for k in range(5)]
    if dparams is not None:
        rows += [(n, dparams[n], want[1][n], yard[1][n]) for n in NAMES]
    bad = []
    for name, got, w, y in rows:
        e, b = rel(got, w), max(FACTOR * rel(y, w), FLOOR)
        print(f"{tag} B={B} {name}: gpu {e:.3e}  cpu-fp32 {rel(y, w):.3e}  bound {b:.3e}")
        if not e <= b:
            bad.append((name, e, b))
    assert not bad, bad


# --------------------------------------------------------------------------- the full walk
def test_full_walk_b2(run):
    assert set(run.head) == set(NAMES) and all(tuple(run.head[n].shape) == NLDF.shape_of(n) for n in NAMES)
    check("walk", run, 2, run.dpools, run.head)


def test_full_walk_b1_and_sample0_of_b2(run):
    o = run.one
    code, dpools, dparams = abi_backward(run.m, run.last, 1, o.ws, o.pools, o.local_fea, o.prob, o.dscore)
    assert code == 0
    check("walk", run, 1, dpools, dict(zip(NAMES, dparams)))
    # The plans differ between B=1 and B=2 (vstab_conv_dgrad's split-K factor follows the row count: Fea_P2's input gradient splits at
    # B=1 and not at B=2), so sample 0 of the B=2 call is held to the bound, not to bit-equality.
    check("sample0-of-B2", run, 1, [p[0:1] for p in run.dpools], None)


def test_extra_gradients_at_prob_local_fea_and_fea_global(run):
    """dprob, dlocal_fea and dfea_global enter the walk: against the reference on sample 0 (B=1 problem)."""
    o = run.one
    gen = torch.Generator().manual_seed(3)
    dprob = (torch.randn(1, 176, 176, 1, generator=gen) * 1e-4).cuda()
    dlf = (torch.randn(1, 176, 176, 640, generator=gen) * 1e-5).cuda()
    dfg = (torch.randn(1, 1, 1, FEA, generator=gen) * 1e-2).cuda()
    code, dpools, dparams = abi_backward(run.m, run.last, 1, o.ws, o.pools, o.local_fea, o.prob, o.dscore, dprob, dlf, dfg)
    assert code == 0
    views = NLDF.workspace_views(o.ws, 1)
    acts = {k: v.cpu().numpy() for k, v in views.items() if k.startswith("cat") or k in ("G1", "G2", "Fea_Global")}
    acts.update(pools=[p.cpu().numpy() for p in o.pools], Local_Fea=o.local_fea.cpu().numpy(), Prob=o.prob.cpu().numpy())
    g = [t.cpu().numpy() for t in (o.dscore, dprob, dlf, dfg)]
    want, yard = ref.walk(acts, run.hw, *g), ref.torch_walk(acts, run.hw, *g, dtype=torch.float32)
    run.ref["x"], run.yard["x"] = want, yard
    check("extras", run, "x", dpools, dict(zip(NAMES, dparams)))


# --------------------------------------------------------------------------- exact comparisons
def test_two_calls_are_bit_equal_and_nothing_else_is_written(run):
    dpools, head = run.m.pools_grad(need_head_weights=True)
    assert all(torch.equal(a, b) for a, b in zip(dpools, run.dpools))
    assert all(torch.equal(head[n], run.head[n]) for n in NAMES)
    assert torch.equal(run.last["ws"], run.ws_before) and torch.equal(run.m.Local_Fea, run.lf_before)
    only, none = run.m.pools_grad(need_head_weights=False)
    assert none is None and all(torch.equal(a, b) for a, b in zip(only, run.dpools))


def test_accumulate_params_twice_is_twice(run):
    o = run.one
    code, _, once = abi_backward(run.m, run.last, 1, o.ws, o.pools, o.local_fea, o.prob, o.dscore, want_pools=False)
    assert code == 0
    acc = [torch.zeros_like(t) for t in once]
    for _ in range(2):
        assert abi_backward(run.m, run.last, 1, o.ws, o.pools, o.local_fea, o.prob, o.dscore, want_pools=False, accumulate=1, dparams=acc)[0] == 0
    for n, a, b in zip(NAMES, acc, once):
        # 0 + g is exact; g + g' differs from 2 g by one rounding of the sum where a launcher adds its split-K parts to the old value
        assert rel(a, 2.0 * b.double().cpu().numpy()) <= 2.0 ** -23, n


# --------------------------------------------------------------------------- stage kernels alone
@pytest.mark.parametrize("extras", [False, True])
def test_score_stage(run, extras):
    B, L = 2, _lib.lib()
    gen = torch.Generator().manual_seed(7)
    dscore = torch.randn(B, 176, 176, 2, generator=gen).cuda()
    lf, W = run.m.Local_Fea, torch.from_numpy(run.hw["Local_Score/W"]).reshape(640, 2).cuda()
    prob = run.m.Prob
    dprob = torch.randn(B, 176, 176, 1, generator=gen).cuda() if extras else None
    dlfea = torch.randn(B, 176, 176, 640, generator=gen).cuda() if extras else None
    dls = torch.full((B, 176, 176, 2), float("nan"), device="cuda")
    dgs, dlf = torch.full((B, 2), float("nan"), device="cuda"), torch.full((B, 176, 176, 640), float("nan"), device="cuda")
    dW, db = torch.full((640, 2), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
    ws = runtime.workspace("cuda", "vstab_nldf_score_backward_workspace_bytes", B)
    runtime.call(dscore.device, "vstab_nldf_score_backward", dscore.data_ptr(), prob.data_ptr(), runtime.ptr(dprob), lf.data_ptr(), runtime.ptr(dlfea),
                 W.data_ptr(), B, dls.data_ptr() if extras else None, dgs.data_ptr(), dlf.data_ptr(), dW.data_ptr(), db.data_ptr(), 0, ws.data_ptr(),
                 ws.numel())
    n64 = lambda t: None if t is None else t.double().cpu().numpy()
    wl, wg = ref.score_backward(n64(dscore), n64(prob), n64(dprob))
    Wn, lfn = n64(W), n64(lf).reshape(-1, 640)
    want = {"dgs": wg, "db": wg.sum(0), "dlf": wl @ Wn.T + (n64(dlfea) if extras else 0.0), "dW": lfn.T @ wl.reshape(-1, 2)}
    if extras:
        want["dls"] = wl
    # the yardstick: the same sums in float32 on the CPU
    f32 = lambda a: torch.as_tensor(a).float()
    yl = f32(n64(dscore)).clone()
    if extras:
        t = prob.cpu()[..., 0] * (1 - prob.cpu()[..., 0]) * dprob.cpu()[..., 0]
        yl[..., 0] += t
        yl[..., 1] -= t
    yard = {"dls": yl, "dgs": yl.sum((1, 2)), "db": yl.sum((0, 1, 2)), "dlf": yl @ W.cpu().t() + (dlfea.cpu() if extras else 0.0),
            "dW": lf.cpu().reshape(-1, 640).t() @ yl.reshape(-1, 2)}
    got = {"dls": dls, "dgs": dgs, "db": db, "dlf": dlf, "dW": dW}
    bad = []
    for k, w in want.items():
        e, b = rel(got[k], w), max(FACTOR * rel(yard[k], w), FLOOR)
        print(f"score stage extras={extras} {k}: gpu {e:.3e} bound {b:.3e}")
        if not e <= b:
            bad.append((k, e, b))
    assert not bad, bad
    if not extras:
        assert torch.isnan(dls).all()                                      # without dprob, dscore itself is Local_Score's gradient


@pytest.mark.parametrize("hw,cs", [(11, 256), (22, 384)])
def test_contrast_gate_stage(hw, cs):
    B, Cn = 2, FEA
    gen = torch.Generator().manual_seed(hw)
    act = torch.randn(B, hw, hw, cs, generator=gen)
    act[..., 0] = -act[..., 0].abs() - 1.0                                  # nothing passes
    act[..., 1] = act[..., 1].abs() + 1.0                                   # everything passes
    d = torch.randn(B, hw, hw, cs, generator=gen)
    want = d.double().numpy().copy()
    want[..., :Cn] = ref.contrast_gate_backward(act[..., :Cn].double().numpy(), want[..., :Cn], want[..., Cn:2 * Cn])
    A, D = act.cuda(), d.cuda()
    runtime.call(A.device, "vstab_nldf_contrast_gate_backward", A.data_ptr(), D.data_ptr(), B, hw, hw, Cn, cs)
    got = D.cpu()
    assert torch.equal(got[..., Cn:], d[..., Cn:])                          # only the dP slice is written
    assert not got[..., 0].any() and got[..., 1].abs().min() > 0
    # 11 float32 operations on numbers of size <= 10 max|d| (the nine-term sum): 16 u x that covers them, u = 2^-24
    err = float(np.abs(got.double().numpy() - want).max())
    bound = 16 * 2.0 ** -24 * 10 * float(d.abs().max())
    print(f"contrast gate {hw}x{hw} cs {cs}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_up_slice_gate_and_bias_sum():
    B, hw, cs, c_off, Cn = 2, 22, 384, 256, 128
    gen = torch.Generator().manual_seed(22)
    act, d = torch.randn(B, hw, hw, cs, generator=gen), torch.randn(B, hw, hw, cs, generator=gen)
    act[..., c_off] = -1.0
    act[..., c_off + 1] = 1.0
    A, D = act.cuda(), d.cuda()
    db = torch.full((Cn,), float("nan"), device="cuda")
    rows = B * hw * hw
    ws = runtime.workspace("cuda", "vstab_column_sum_scratch_bytes", rows, Cn)
    runtime.call(A.device, "vstab_nldf_slice_gate_backward", A.data_ptr(), D.data_ptr(), rows, cs, c_off, Cn, db.data_ptr(), 0, ws.data_ptr(), ws.numel())
    want = d.clone()
    want[..., c_off:] = torch.where(act[..., c_off:] > 0, d[..., c_off:], torch.zeros(()))
    assert torch.equal(D.cpu(), want)
    wsum = want[..., c_off:].double().sum((0, 1, 2)).numpy()
    e, b = rel(db, wsum), max(FACTOR * rel(want[..., c_off:].sum((0, 1, 2)), wsum), FLOOR)
    print(f"up-slice bias sum: gpu {e:.3e} bound {b:.3e}")
    assert e <= b and float(db[0]) == 0.0
    first = db.clone()
    runtime.call(A.device, "vstab_nldf_slice_gate_backward", A.data_ptr(), D.data_ptr(), rows, cs, c_off, Cn, db.data_ptr(), 1, ws.data_ptr(), ws.numel())
    assert torch.equal(db, first + first)


# --------------------------------------------------------------------------- plumbing
def test_model_backward_is_pools_grad_then_the_trunk_times_255(run):
    m = run.m
    dinput, head, trunk = m.backward(need_input=True, need_trunk_weights=True)
    assert dinput.shape == run.x.shape and set(head) == set(NAMES) and set(trunk) == {n for n, _, _ in vgg16.LAYERS}
    dpre, tw = m.vgg.backward({f"pool{k + 1}": g for k, g in enumerate(run.dpools)}, need_input=True, need_weights=True)
    assert torch.equal(dinput, dpre * 255.0)
    assert all(torch.equal(head[n], run.head[n]) for n in NAMES)
    assert all(torch.equal(trunk[n][0], tw[n][0]) and torch.equal(trunk[n][1], tw[n][1]) for n in tw)
    assert float(dinput.abs().max()) > 0


def test_forward_under_autograd_fills_the_same_gradients(run):
    m = NLDF.Model(vgg_data_dict=vgg16.synthetic_data_dict(seed=5), head_weights=run.hw, trainable=True)
    m.vgg.trainable = True
    x = run.x.clone().requires_grad_(True)
    score, prob = m.forward(x)
    assert score.requires_grad and torch.equal(score.detach(), run.m.Score)
    saliency_loss(score, run.label).Loss_Mean.backward()
    dinput, head, trunk = run.m.backward(need_input=True, need_trunk_weights=True)
    # build_loss and saliency_loss are the same fused call: the same dscore bits, then the same walk
    assert torch.equal(x.grad, dinput)
    assert all(torch.equal(m.grads[n], head[n]) for n in NAMES)
    assert all(torch.equal(m.vgg.grads[n][0], trunk[n][0]) and torch.equal(m.vgg.grads[n][1], trunk[n][1]) for n in trunk)
    m.zero_grads()
    assert all(not g.any() for g in m.grads.values())
    # without anything that needs a gradient the graph is not recorded
    plain = NLDF.Model(vgg_data_dict=vgg16.synthetic_data_dict(seed=5), head_weights=run.hw)
    s2, _ = plain.forward(run.x)
    assert not s2.requires_grad and torch.equal(s2, run.m.Score)


def test_apply_grads_lowers_the_loss(run):
    m = NLDF.Model(vgg_data_dict=vgg16.synthetic_data_dict(seed=5), head_weights=run.hw, trainable=True)
    m.vgg.trainable = True
    score, _ = m.forward(run.x)
    loss0 = saliency_loss(score, run.label).Loss_Mean
    loss0.backward()
    g2 = sum(float((g.double() ** 2).sum()) for g in m.grads.values()) + sum(float((t.double() ** 2).sum()) for p in m.vgg.grads.values() for t in p)
    lr = 0.05 * float(loss0.detach()) / g2                   # to first order the step lowers the loss by lr |g|^2 = 5 % of it
    before = m.export_head_weights()["Local_Score/W"].copy()
    m.apply_grads(lr)
    m.vgg.apply_grads(lr)
    with torch.no_grad():
        score1, _ = m.forward(run.x)
        loss1 = saliency_loss(score1, run.label).Loss_Mean
    print(f"SGD step: lr {lr:.3e} |g|^2 {g2:.3e} Loss_Mean {float(loss0.detach()):.6f} -> {float(loss1):.6f}")
    assert float(loss1) < 0.99 * float(loss0.detach())
    after = m.export_head_weights()["Local_Score/W"]
    want = before.astype(np.float64) - lr * m.grads["Local_Score/W"].double().cpu().numpy()
    assert rel(after, want) <= 2.0 ** -22 and not np.array_equal(after, before)


# --------------------------------------------------------------------------- refusals
def test_refusals(run):
    m, o, L = run.m, run.one, _lib.lib()
    fresh = NLDF.Model(vgg_data_dict=vgg16.synthetic_data_dict(seed=5), head_weights=run.hw)
    for fn in (fresh.backward, fresh.pools_grad, lambda: fresh.backward(score_grad=run.dscore)):
        with pytest.raises(RuntimeError):
            fn()
    d = run.dscore
    for bad in (d[:1], d.double(), d.cpu(), d[..., :1]):
        with pytest.raises(ValueError):
            m.pools_grad(score_grad=bad)
    with pytest.raises(ValueError):
        m.pools_grad(prob_grad=d)
    with pytest.raises(ValueError):
        m.backward(local_fea_grad=d)
    with pytest.raises(ValueError):
        m.backward(need_input=False, need_trunk_weights=False, need_head_weights=False)
    # the raw ABI: nothing is launched by a refused call
    nws = L.vstab_nldf_backward_workspace_bytes(1, 1)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device="cuda")
    args = (m, run.last, 1, o.ws, o.pools, o.local_fea, o.prob, o.dscore)
    sentinel = [torch.full(NLDF.shape_of(n), 7.0, device="cuda") for n in NAMES]
    assert abi_backward(*args, dparams=sentinel, ws=ws, ws_bytes=nws - 1)[0] == -4               # short workspace: VSTAB_E_NOMEM
    assert abi_backward(*args, dparams=sentinel, ws=ws.data_ptr() + 16, ws_bytes=nws)[0] == -2   # misaligned: VSTAB_E_ALIGN
    assert abi_backward(*args, dparams=sentinel, ws=ws, ws_bytes=nws, ws_fwd_bytes=o.ws.numel() - 1)[0] == -4
    assert abi_backward(*args, want_pools=False, want_params=False, ws=ws, ws_bytes=nws)[0] == -6   # no gradient asked for: VSTAB_E_STATE
    assert abi_backward(m, run.last, 65, o.ws, o.pools, o.local_fea, o.prob, o.dscore, want_pools=False, dparams=sentinel, ws=ws, ws_bytes=nws)[0] == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in sentinel)
    assert L.vstab_nldf_backward_workspace_bytes(0, 0) == 0 and L.vstab_nldf_backward_workspace_bytes(65, 1) == 0

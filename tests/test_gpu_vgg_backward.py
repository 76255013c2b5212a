"""Vgg16.backward / features / apply_grads and the C entries under them against tests/vgg_grad_ref.py (float64 numpy).

Tolerance.  The error of a tensor is max|got - ref| / max|ref| against the float64 reference.  The yardstick is the same quantity
of the same network in float32 on the CPU (torch, direct convolution: vgg_grad_ref.torch_backward), computed here once per
problem; a GPU tensor must stay within FACTOR x that.  FACTOR = 4: the Winograd forms cost about two bits over direct fp32
(DESIGN.md section 8).  FLOOR = 2^-22: a float32 result is not asked to be closer to the float64 one than four units in the last
place of the tensor's largest element, however lucky the CPU's rounding was on a tensor of a few elements (a bias gradient summed
over two pixels is exact in float32).  DESIGN.md section 21 lists the measured errors per tensor.

Shapes: B=2 at 10x14 (pool levels 5x7, 3x4, 2x2, 1x1, 1x1: every pool has clipped windows), B=3 at 16x16 (even), and B=1 at
212x212, the smallest square at which an input gradient takes the transposed Winograd form (conv3_2 / conv3_3 at 53x53: 729
tiles; the break-even of the forward needs 715)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, vgg16
from tests import vgg_grad_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 2.0 ** -22
SEED = 5
NAMES = [n for n, _, _ in vgg16.LAYERS]


def rel(got, want):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def params():
    return vgg16.synthetic_data_dict(SEED)


@functools.lru_cache(maxsize=None)
def problem(B, H, W, names):
    """Input, gradients at `names`, the float64 reference and the float32 CPU yardstick of one problem."""
    rng = np.random.default_rng(B * 1000 + H)
    x = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    outs = ref.forward(x, params())
    grads = {n: rng.standard_normal(outs[ref.OUTPUTS.index(n)].shape).astype(np.float32) for n in names}
    dx, dparams = ref.backward(x, params(), grads, outs)
    cdx, cparams, _ = ref.torch_backward(x, params(), grads, torch.float32)
    bound = {"dinput": max(FACTOR * rel(cdx, dx), FLOOR)}
    for n in NAMES:
        for k, s in enumerate(("dW", "db")):
            if np.abs(dparams[n][k]).max() > 0:
                bound[f"{n}.{s}"] = max(FACTOR * rel(cparams[n][k], dparams[n][k]), FLOOR)
    return x, grads, outs, dx, dparams, bound


def run_gpu(B, H, W, names, **kw):
    x, grads, *_ = problem(B, H, W, names)
    net = vgg16.Vgg16(seed=SEED).build(torch.from_numpy(x).cuda())
    return net, net.backward({n: torch.from_numpy(g).cuda() for n, g in grads.items()}, **kw)


def check(tag, B, H, W, names, dinput, dW, layers=NAMES):
    _, _, _, dx, dparams, bound = problem(B, H, W, names)
    bad = []
    rows = []
    if dinput is not None:
        rows.append(("dinput", rel(dinput, dx), bound["dinput"]))
    if dW is not None:
        for n in layers:
            for k, s in enumerate(("dW", "db")):
                if f"{n}.{s}" in bound:
                    rows.append((f"{n}.{s}", rel(dW[n][k], dparams[n][k]), bound[f"{n}.{s}"]))
                else:
                    assert not dW[n][k].any(), f"{n}.{s} must be zero"
    for name, err, b in rows:
        print(f"{tag} {B}x{H}x{W} {name}: gpu {err:.3e}  cpu-fp32 {b / FACTOR:.3e}  bound {b:.3e}")
        if not err <= b:
            bad.append((name, err, b))
    assert not bad, bad


SHAPES = [(2, 10, 14), (3, 16, 16)]
ALL = ("pool1", "pool2", "conv3_2", "pool3", "pool4", "pool5")


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_case1_pool5_to_input_and_filters(B, H, W):
    _, (dinput, dW) = run_gpu(B, H, W, ("pool5",), need_weights=True)
    assert dinput.shape == (B, H, W, 3) and set(dW) == set(NAMES)
    check("case1", B, H, W, ("pool5",), dinput, dW)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_case2_gradients_at_every_pool_and_a_bare_conv(B, H, W):
    _, (dinput, dW) = run_gpu(B, H, W, ALL, need_weights=True)
    check("case2", B, H, W, ALL, dinput, dW)


def test_case2b_conv_output_that_feeds_a_pool_and_deepest_gradient_at_a_conv():
    """conv2_2 carries a gradient of its own besides pool2's (the pool kernel's accumulate path); conv4_2 is the deepest."""
    names = ("conv2_2", "pool2", "conv4_2")
    _, (dinput, dW) = run_gpu(2, 10, 14, names, need_weights=True)
    check("case2b", 2, 10, 14, names, dinput, dW)


def test_case3_and_4_input_only_and_filters_only_are_the_same_numbers():
    B, H, W = SHAPES[0]
    _, (dinput, dW) = run_gpu(B, H, W, ("pool5",), need_weights=True)
    _, (dinput3, none) = run_gpu(B, H, W, ("pool5",), need_weights=False)
    assert none is None and torch.equal(dinput3, dinput)
    _, (none, dW4) = run_gpu(B, H, W, ("pool5",), need_input=False, need_weights=True)
    assert none is None
    for n in NAMES:
        assert torch.equal(dW4[n][0], dW[n][0]) and torch.equal(dW4[n][1], dW[n][1]), n


def test_case5_gradient_at_pool2_leaves_the_layers_above_untouched():
    B, H, W = SHAPES[0]
    net, (dinput, dW) = run_gpu(B, H, W, ("pool2",), need_weights=True)
    for n in NAMES[4:]:
        assert not dW[n][0].any() and not dW[n][1].any(), n
    check("case5", B, H, W, ("pool2",), dinput, dW, layers=NAMES[:4])


def test_winograd_input_gradients_at_212():
    B, H, W = 1, 212, 212
    names = ("conv3_3", "pool3")
    _, (dinput, dW) = run_gpu(B, H, W, names, need_weights=True)
    check("wino", B, H, W, names, dinput, dW)


@pytest.mark.parametrize("Cn", [4, 12])
def test_case6_pool_kernel_on_the_tie_and_zero_plane(Cn):
    y, dpool, dy = ref.tie_plane()
    scale = np.arange(1, Cn + 1, dtype=np.float64)                       # every channel its own multiple of the gradient
    Y = torch.tensor(np.broadcast_to(y[None, :, :, None], (2, 3, 3, Cn)).copy(), dtype=torch.float32, device="cuda")
    G = torch.tensor(dpool[None, :, :, None] * scale * np.array([1.0, -1.0]).reshape(2, 1, 1, 1), dtype=torch.float32, device="cuda")
    want = torch.tensor(dy[None, :, :, None] * scale * np.array([1.0, -1.0]).reshape(2, 1, 1, 1), dtype=torch.float32, device="cuda")
    out = torch.full_like(Y, float("nan"))
    runtime.call(Y.device, "vstab_maxpool2x2_relu_backward", Y.data_ptr(), 2, 3, 3, Cn, G.data_ptr(), out.data_ptr(), 0)
    assert torch.equal(out, want)                                         # every element written: no NaN is left
    prior = torch.arange(Y.numel(), dtype=torch.float32, device="cuda").reshape(Y.shape) + 1.0
    out = prior.clone()
    runtime.call(Y.device, "vstab_maxpool2x2_relu_backward", Y.data_ptr(), 2, 3, 3, Cn, G.data_ptr(), out.data_ptr(), 1)
    assert torch.equal(out, (prior + want) * (Y > 0))
    # the bare gate
    d = prior.clone()
    runtime.call(Y.device, "vstab_relu_backward", Y.data_ptr(), d.data_ptr(), d.numel())
    assert torch.equal(d, prior * (Y > 0))


def test_case7_first_layer_gradients_alone():
    B, H, W = 2, 5, 7
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    g = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    Wf = params()["conv1_1"][0]
    dx, dW, db = ref.conv_backward(x.astype(np.float64), Wf.astype(np.float64), g.astype(np.float64))
    xt = torch.tensor(x).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.tensor(Wf).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    bt = torch.zeros(64, requires_grad=True)
    (torch.nn.functional.conv2d(xt, wt, bt, padding=1) * torch.tensor(g).permute(0, 3, 1, 2)).sum().backward()
    bound = {"dx": max(FACTOR * rel(xt.grad.permute(0, 2, 3, 1), dx), FLOOR), "dW": max(FACTOR * rel(wt.grad.permute(2, 3, 1, 0), dW), FLOOR),
             "db": max(FACTOR * rel(bt.grad, db), FLOOR)}
    X, G, WF = torch.tensor(x).cuda(), torch.tensor(g).cuda(), torch.tensor(Wf).cuda()
    gdx = torch.full_like(X, float("nan"))
    runtime.call(X.device, "vstab_conv3x3_rgb_dgrad", G.data_ptr(), B, H, W, WF.data_ptr(), 64, gdx.data_ptr())
    ws = runtime.workspace(X.device, "vstab_conv3x3_rgb_wgrad_workspace_bytes", B, H, W)
    gdW, gdb = torch.full((3, 3, 3, 64), float("nan"), device="cuda"), torch.full((64,), float("nan"), device="cuda")
    runtime.call(X.device, "vstab_conv3x3_rgb_wgrad", X.data_ptr(), G.data_ptr(), B, H, W, 64, gdW.data_ptr(), gdb.data_ptr(), 0, ws.data_ptr(), ws.numel())
    errs = {"dx": rel(gdx, dx), "dW": rel(gdW, dW), "db": rel(gdb, db)}
    print("case7", errs, bound)
    assert all(errs[k] <= bound[k] for k in errs), (errs, bound)
    first = gdW.clone()
    runtime.call(X.device, "vstab_conv3x3_rgb_wgrad", X.data_ptr(), G.data_ptr(), B, H, W, 64, gdW.data_ptr(), gdb.data_ptr(), 1, ws.data_ptr(), ws.numel())
    assert torch.equal(gdW, first + first)


def test_case8_features_under_autograd():
    B, H, W = SHAPES[0]
    names = ("pool2", "conv3_2")
    wk = (0.7, 1.3)
    x, *_ = problem(B, H, W, ("pool5",))
    raw = (torch.from_numpy(x).cuda() * 0.002 + 0.5).requires_grad_(True)          # an "image" in [0, 1]; preprocess scales it by 255
    net = vgg16.Vgg16(seed=SEED, trainable=True, reuse_outputs=True)
    f = net.features(vgg16.preprocess(raw), names)
    loss = sum(w * (t * t).mean() for w, t in zip(wk, f))
    loss.backward()
    # the reference: d loss / d f_k = 2 w_k f_k / numel, through the trunk, times 255
    pre = vgg16.preprocess(raw.detach())
    xin = pre.cpu().numpy()
    outs = ref.forward(xin, params())
    grads = {n: 2.0 * w * outs[ref.OUTPUTS.index(n)] / outs[ref.OUTPUTS.index(n)].size for n, w in zip(names, wk)}
    dx, dparams = ref.backward(xin, params(), grads, outs)
    cdx, cparams, _ = ref.torch_backward(xin, params(), {n: g.astype(np.float32) for n, g in grads.items()}, torch.float32)
    e, b = rel(raw.grad, 255.0 * dx), max(FACTOR * rel(255.0 * cdx, 255.0 * dx), FLOOR)
    print(f"case8 d raw: gpu {e:.3e} bound {b:.3e}")
    assert e <= b
    for n in NAMES[:6]:
        e, b = rel(net.grads[n][0], dparams[n][0]), max(FACTOR * rel(cparams[n][0], dparams[n][0]), FLOOR)
        print(f"case8 {n}.dW: gpu {e:.3e} bound {b:.3e}")
        assert e <= b, n
    assert not net.grads["conv5_3"][0].any()
    once = {n: net.grads[n][0].clone() for n in NAMES[:6]}
    # a second backward accumulates
    f = net.features(pre, names)                                                   # the input needs no gradient: the filters still get theirs
    sum(w * (t * t).mean() for w, t in zip(wk, f)).backward()
    for n in NAMES[:6]:
        assert rel(net.grads[n][0], 2.0 * once[n].double().cpu().numpy()) <= 1e-6, n
    net.zero_grads()
    assert all(not dW.any() and not db.any() for dW, db in net.grads.values())
    # reuse_outputs=True: a second build() overwrites the activations the first graph was recorded on
    f = net.features(pre, names)
    stale = sum((t * t).mean() for t in f)
    net.build(pre * 0.5)
    with pytest.raises(RuntimeError, match="stale"):
        stale.backward()


def test_case9_apply_grads_steps_the_filters_the_forward_reads():
    B, H, W = SHAPES[0]
    x, *_ = problem(B, H, W, ("pool5",))
    X = torch.from_numpy(x).cuda()
    net = vgg16.Vgg16(seed=SEED, trainable=True)
    (f,) = net.features(X, ("pool3",))
    (f * f).mean().backward()
    lr = 0.1 / max(float(net.grads[n][0].abs().max()) for n in NAMES)          # the largest filter element moves by 0.1
    stepped = {n: [(params()[n][0].astype(np.float64) - lr * net.grads[n][0].double().cpu().numpy()).astype(np.float32),
                   (params()[n][1].astype(np.float64) - lr * net.grads[n][1].double().cpu().numpy()).astype(np.float32)] for n in NAMES}
    before = {name: getattr(net, name).clone() for name in ("conv1_1", "pool3")}
    net.apply_grads(lr)
    net.build(X)
    want = ref.forward(x, stepped)
    zero = {"pool5": np.zeros(want[17].shape, np.float32)}
    _, _, cpu32 = ref.torch_backward(x, stepped, zero, torch.float32)           # the yardstick: the stepped forward in float32 on the CPU
    for name in ("conv1_1", "pool3", "pool5"):
        i = ref.OUTPUTS.index(name)
        e, b = rel(getattr(net, name), want[i]), max(FACTOR * rel(cpu32[i], want[i]), FLOOR)
        print(f"case9 {name}: gpu {e:.3e} bound {b:.3e}")
        assert e <= b, name
    for name, t in before.items():                                             # and the step was no rounding error
        assert rel(t, want[ref.OUTPUTS.index(name)]) > 1e-3, name
    exported = net.export()
    assert rel(exported["conv1_1"][0], stepped["conv1_1"][0]) <= 2.0 ** -22


def test_case10_refusals_return_their_codes():
    B, H, W = SHAPES[0]
    net = vgg16.Vgg16(seed=SEED).build(torch.zeros(B, H, W, 3, device="cuda"))
    last, ctx, L = net._last, net._ctx, _lib.lib()
    outs = last["outs"]
    g = torch.ones_like(outs[17])
    dinput = torch.empty_like(last["x"])
    nws = L.vstab_vgg16_backward_workspace_bytes(B, H, W, 0)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device="cuda")

    def call(h=ctx._h, optr=None, dptr=None, din=dinput.data_ptr(), dpar=None, wsp=None, wsn=nws):
        o = (C.c_void_p * 18)(*[t.data_ptr() for t in outs]) if optr is None else optr
        d = (C.c_void_p * 18)() if dptr is None else dptr
        if dptr is None:
            d[17] = g.data_ptr()
        return L.vstab_vgg16_backward(h, last["x"].data_ptr(), B, H, W, o, d, din, dpar, 0, ws.data_ptr() if wsp is None else wsp, wsn, None)

    assert call() == 0
    torch.cuda.synchronize()
    before = dinput.clone()
    o = (C.c_void_p * 18)(*[t.data_ptr() for t in outs]); o[3] = None
    assert call(optr=o) == -6                                             # a NULL outs[i]: VSTAB_E_STATE
    o = (C.c_void_p * 18)(*[t.data_ptr() for t in outs]); o[3] = outs[3].data_ptr() + 4
    assert call(optr=o) == -2                                             # misaligned: VSTAB_E_ALIGN
    assert call(wsp=ws.data_ptr() + 16) == -2
    assert call(wsn=nws - 1) == -4                                        # workspace too small: VSTAB_E_NOMEM
    assert call(dptr=(C.c_void_p * 18)()) == -6                           # no gradient at all
    assert call(din=None) == -6                                           # neither dinput nor dparams
    fresh = runtime.Context(0)
    assert call(h=fresh._h) == -6                                         # no loaded weights
    torch.cuda.synchronize()
    assert torch.equal(dinput, before)                                    # nothing was launched
    # the Python entry's own refusals
    with pytest.raises(RuntimeError):
        vgg16.Vgg16(seed=SEED).backward({"pool5": g})
    for bad in ({"pool6": g}, {"pool5": g[:1]}, {"pool5": g.double()}, {"pool5": g.cpu()}, {}):
        with pytest.raises(ValueError):
            net.backward(bad)
    with pytest.raises(ValueError):
        net.backward({"pool5": g}, need_input=False, need_weights=False)

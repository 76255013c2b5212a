"""Pins tests/cell_grad_ref.py (no GPU): in float64 against torch.autograd on an independently written torch composition of the cells
(NCHW, F.conv2d), every gradient within 1e-10 of its tensor's largest magnitude -- three orders above what float64 summation order
can cost at these sizes, far below any formula error; a central finite-difference spot check of the layer-norm adjoint alone; and the
conditioning that the GPU bounds of tests/test_gpu_cell_backward.py rely on, for every one of its cases: every normalised quantity
has a per-sample standard deviation >= 0.1 in float64, and in the relu cases every relu argument has a magnitude >= 1e-4 in float64
(so float32 and float64 take the same branch everywhere).  No seed had to be changed for that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cell_grad_ref as gref
from tests import cell_ref as ref

F64 = np.float64
REL = 1e-10
SMALL = {"f1": (1, 4, 5, 2, 1, 3), "odd": (2, 5, 6, 3, 3, 3)}          # B, H, W, Cx, F, k


# ---------------------------------------------------------------------------------------------------- the torch composition
def _t(a, grad=True):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _tln(v, gamma, beta):
    mean = v.mean(dim=(1, 2, 3), keepdim=True)
    var = ((v - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    return (v - mean) / torch.sqrt(var + 1e-12) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def _tact(v, activation):
    return {"tanh": torch.tanh, "relu": torch.relu, "identity": lambda t: t}[activation](v)


def _tconv(x, h, kernel, bias):
    """x, h NCHW; kernel HWIO"""
    return F.conv2d(torch.cat([x, h], 1), kernel.permute(3, 2, 0, 1), bias, padding=kernel.shape[0] // 2)


def torch_lstm(x, c, h, w, activation, normalize, peephole, forget_bias=1.0):
    """NHWC tensors in and out"""
    Fn = c.shape[3]
    y = _tconv(_nchw(x), _nchw(h), w["kernel"], None if normalize else w["bias"])
    j, i, f, o = torch.split(y, Fn, 1)
    cc = _nchw(c)
    if peephole:
        i = i + w["W_ci"].permute(2, 0, 1) * cc
        f = f + w["W_cf"].permute(2, 0, 1) * cc
    if normalize:
        j, i, f = (_tln(v, w[ref.LSTM_LN[n] + "/gamma"], w[ref.LSTM_LN[n] + "/beta"]) for n, v in enumerate((j, i, f)))
    cn = cc * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * _tact(j, activation)
    if peephole:
        o = o + w["W_co"].permute(2, 0, 1) * cn
    if normalize:
        o, cn = _tln(o, w["LayerNorm_3/gamma"], w["LayerNorm_3/beta"]), _tln(cn, w["LayerNorm_4/gamma"], w["LayerNorm_4/beta"])
    return _nhwc(cn), _nhwc(torch.sigmoid(o) * _tact(cn, activation))


def torch_gru(x, h, w, activation, normalize):
    Fn = h.shape[3]
    hh = _nchw(h)
    y = _tconv(_nchw(x), hh, w["gates/kernel"], None if normalize else w["gates/bias"])
    r, u = torch.split(y, Fn, 1)
    if normalize:
        r, u = (_tln(v, w[ref.GRU_LN[n] + "/gamma"], w[ref.GRU_LN[n] + "/beta"]) for n, v in enumerate((r, u)))
    r, u = torch.sigmoid(r), torch.sigmoid(u)
    y2 = _tconv(_nchw(x), r * hh, w["candidate/kernel"], None if normalize else w["candidate/bias"])
    if normalize:
        y2 = _tln(y2, w["candidate/LayerNorm/gamma"], w["candidate/LayerNorm/beta"])
    return _nhwc(u * hh + (1 - u) * _tact(y2, activation))


def _check(tag, got, want):
    want = want.detach().numpy() if torch.is_tensor(want) else want
    scale = max(float(np.abs(want).max()), 1e-300)
    err = ref.max_err(got, want)
    assert got.shape == want.shape and err <= REL * scale, (tag, err, scale)


def _rand(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape)


# ---------------------------------------------------------------------------------------------------- one step
LSTM_CASES = [("odd", n, p, "tanh") for n in (True, False) for p in (True, False)] + [("odd", True, True, "relu"), ("odd", False, True, "identity"),
                                                                                      ("f1", True, True, "tanh"), ("f1", False, False, "relu")]


@pytest.mark.parametrize("name,normalize,peephole,activation", LSTM_CASES)
def test_lstm_step_against_autograd(name, normalize, peephole, activation):
    shape = SMALL[name]
    B, H, W, _, Fn, _ = shape
    w = ref.make_weights("lstm", 11, shape, normalize, peephole)
    x, c, h = ref.make_inputs(12, shape)
    dh, dcn = _rand(13, B, H, W, Fn), _rand(14, B, H, W, Fn)
    kw = dict(activation=activation, normalize=normalize, peephole=peephole)
    dx, (dc, dh_old), grads = gref.lstm_call_backward(x, (c, h), w, F64, dh, dcn, **kw)
    tw = {n: _t(a) for n, a in w.items()}
    tx, tc, th = _t(x), _t(c), _t(h)
    cn, hn = torch_lstm(tx, tc, th, tw, **kw)
    ((cn * _t(dcn, False)).sum() + (hn * _t(dh, False)).sum()).backward()
    for tag, got, want in (("dx", dx, tx.grad), ("dc", dc, tc.grad), ("dh", dh_old, th.grad)):
        _check(tag, got, want)
    assert set(grads) == set(w)
    for n in w:
        _check(n, grads[n], tw[n].grad)


@pytest.mark.parametrize("name,normalize,activation", [("odd", True, "tanh"), ("odd", False, "tanh"), ("odd", True, "relu"), ("odd", False, "identity"),
                                                       ("f1", True, "tanh"), ("f1", False, "relu")])
def test_gru_step_against_autograd(name, normalize, activation):
    shape = SMALL[name]
    B, H, W, _, Fn, _ = shape
    w = ref.make_weights("gru", 21, shape, normalize)
    x, _, h = ref.make_inputs(22, shape)
    dhn = _rand(23, B, H, W, Fn)
    dx, dh_old, grads = gref.gru_call_backward(x, h, w, F64, dhn, activation=activation, normalize=normalize)
    tw = {n: _t(a) for n, a in w.items()}
    tx, th = _t(x), _t(h)
    (torch_gru(tx, th, tw, activation, normalize) * _t(dhn, False)).sum().backward()
    _check("dx", dx, tx.grad)
    _check("dh", dh_old, th.grad)
    assert set(grads) == set(w)
    for n in w:
        _check(n, grads[n], tw[n].grad)


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_sequence_against_autograd(kind):
    """T = 3 with a given non-zero initial state; the loss mixes every output and the final state"""
    shape = SMALL["odd"]
    B, H, W, _, Fn, _ = shape
    w = ref.make_weights(kind, 31, shape, True)
    xs, c, h = ref.make_inputs(32, shape, T=3)
    d_out, d_c, d_h = _rand(33, 3, B, H, W, Fn), _rand(34, B, H, W, Fn), _rand(35, B, H, W, Fn)
    state = (c, h) if kind == "lstm" else h
    d_in, d_state, grads = gref.run_sequence_backward(kind, xs, state, w, F64, d_out, (d_c, d_h) if kind == "lstm" else d_h)
    tw = {n: _t(a) for n, a in w.items()}
    txs, tc, th = _t(xs), _t(c), _t(h)
    cs, hs, loss = tc, th, 0.0
    for t in range(3):
        if kind == "lstm":
            cs, hs = torch_lstm(txs[t], cs, hs, tw, "tanh", True, True)
        else:
            hs = torch_gru(txs[t], hs, tw, "tanh", True)
        loss = loss + (hs * _t(d_out[t], False)).sum()
    loss = loss + (hs * _t(d_h, False)).sum() + ((cs * _t(d_c, False)).sum() if kind == "lstm" else 0.0)
    loss.backward()
    _check("d inputs", d_in, txs.grad)
    if kind == "lstm":
        _check("d c0", d_state[0], tc.grad)
        _check("d h0", d_state[1], th.grad)
    else:
        _check("d h0", d_state, th.grad)
    for n in w:
        _check(n, grads[n], tw[n].grad)


def test_layer_norm_adjoint_by_finite_differences():
    rng = np.random.RandomState(41)
    v, gamma, beta, dout = rng.standard_normal((2, 3, 4, 5)), rng.uniform(0.5, 1.5, 5), rng.uniform(-0.5, 0.5, 5), rng.standard_normal((2, 3, 4, 5))
    dv, dgamma, dbeta = gref.layer_norm_adjoint(v, gamma, dout)
    loss = lambda vv, gg, bb: float((ref.layer_norm(vv, gg, bb) * dout).sum())          # noqa: E731
    eps = 1e-6
    for idx in ((0, 0, 0, 0), (1, 2, 3, 4), (0, 1, 2, 3)):
        e = np.zeros_like(v)
        e[idx] = eps
        assert abs((loss(v + e, gamma, beta) - loss(v - e, gamma, beta)) / (2 * eps) - dv[idx]) <= 1e-7
    for ch in (0, 4):
        e = np.zeros(5)
        e[ch] = eps
        assert abs((loss(v, gamma + e, beta) - loss(v, gamma - e, beta)) / (2 * eps) - dgamma[ch]) <= 1e-7
        assert abs((loss(v, gamma, beta + e) - loss(v, gamma, beta - e)) / (2 * eps) - dbeta[ch]) <= 1e-7


# ---------------------------------------------------------------------------------------------------- conditioning of the GPU cases
def _assert_std(trace, tag):
    for n, v in enumerate(trace):
        std = v.std(axis=(1, 2, 3))
        assert std.min() >= 0.1, (tag, n, float(std.min()))


def test_gpu_cases_are_well_conditioned():
    for name, shape in ref.SHAPES.items():
        for normalize in (True, False):
            for peephole in (True, False):
                w, x, c, h, _, _ = gref.lstm_case(shape, normalize, peephole)
                w64 = ref.cast(w, F64)
                if normalize:
                    trace = []
                    ref.lstm_gates(gref.stage_y(shape, 4).astype(F64), c.astype(F64), w64, normalize=True, peephole=peephole, trace=trace)
                    _assert_std(trace, ("lstm stage", name, peephole))
                    trace = []
                    ref.lstm_call(x, (c, h), w, F64, normalize=True, peephole=peephole, trace=trace)
                    _assert_std(trace, ("lstm cell", name, peephole))
            w, x, h = gref.gru_case(shape, normalize)[:3]
            if normalize:
                trace = []
                w64 = ref.cast(w, F64)
                ref.gru_gates(gref.stage_y(shape, 2).astype(F64), h.astype(F64), w64, True, trace)
                ref.gru_update(gref.stage_y(shape, 1).astype(F64), h.astype(F64), gref.stage_u(shape).astype(F64), w64, normalize=True, trace=trace)
                ref.gru_call(x, h, w, F64, normalize=True, trace=trace)
                _assert_std(trace, ("gru", name))
    for kind in ("lstm", "gru"):
        w, xs, c, h = gref.sequence_case(kind)[:4]
        for state in (None, (c, h) if kind == "lstm" else h):
            trace = []
            ref.run_sequence(kind, xs, state, w, F64, trace=trace)
            _assert_std(trace, (kind, "sequence"))
    # the relu cases (the raw stages on `odd`, normalize and peephole on): every relu argument away from zero
    shape = ref.SHAPES["odd"]
    w, _, c, _, _, _ = gref.lstm_case(shape, True, True)
    y = gref.stage_y(shape, 4).astype(F64)
    w64 = ref.cast(w, F64)
    for activation in ("identity", "relu"):                   # (the activation changes what LN_3 / LN_4 see: o + W_co c' and c')
        trace = []
        cn, _ = ref.lstm_gates(y, c.astype(F64), w64, activation=activation, trace=trace)
        _assert_std(trace, ("lstm stage", activation))
    j = ref.layer_norm(trace[0], w64["LayerNorm/gamma"], w64["LayerNorm/beta"])
    assert np.abs(j).min() >= 1e-4 and np.abs(cn).min() >= 1e-4, (float(np.abs(j).min()), float(np.abs(cn).min()))
    wg, _, hg = gref.gru_case(shape, True)[:3]
    wg64 = ref.cast(wg, F64)
    y2n = ref.layer_norm(gref.stage_y(shape, 1).astype(F64), wg64["candidate/LayerNorm/gamma"], wg64["candidate/LayerNorm/beta"])
    assert np.abs(y2n).min() >= 1e-4, float(np.abs(y2n).min())

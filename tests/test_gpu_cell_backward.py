"""The backward of ConvLSTMCell / ConvGRUCell (differentiable=True; csrc/cell_ops.hip's backward half, cell.py's autograd Functions)
against tests/cell_grad_ref.py.

Bound of every comparison: a tensor may deviate from the float64 restatement by 4 x the float32 restatement's own deviation from float64 on
the same case (computed here, on the CPU), floor 8 float32 epsilons of that tensor's largest reference magnitude (the `unit`); all elements are
compared.  Each comparison prints `deviation / unit / bound` (pytest -s).  Inputs as tests/test_gpu_cell.py makes them with seeds of their own,
upstream gradients N(0,1) (cell_grad_ref.lstm_case ...); the conditioning the bounds rely on is asserted in tests/test_cell_grad_ref_cpu.py.

Measured on an MI355X, the largest deviation of each family in units (8 eps of the tensor's largest magnitude) and as a fraction of its
bound:  raw LSTM stage 0.28 / 0.28 (100 comparisons);  raw GRU stages 0.24 / 0.24 (74);  LSTM cell 0.93 / 0.93 (176; the F = 1 layer-norm
gains, one number each, are the tight ones);  GRU cell 0.55 / 0.51 (64);  LSTM sequence 0.55 / 0.44 (60);  GRU sequence 0.66 / 0.40 (35).
With the gamma / beta column sums taken in float32 instead of double the F = 1 cell missed: dLayerNorm_2/gamma 1.08 units."""
import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, cell, runtime, training
from tests import cell_grad_ref as gref
from tests import cell_ref as ref

pytestmark = pytest.mark.gpu
_up4 = cell._up4

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(np.float32).eps)
E_SHAPE, E_ALIGN, E_NOMEM, E_STATE = -1, -2, -4, -6
SHAPE_IDS = list(ref.SHAPES)
ACTS = {"tanh": 0, "relu": 1, "identity": 2}


def _close(tag, got, want64, got32):
    got = got.detach().cpu().numpy()
    unit = 8.0 * EPS * float(np.abs(want64).max())
    dev, bound = ref.max_err(got, want64), max(4.0 * ref.max_err(got32, want64), unit)
    print(f"[cell grad {tag}] deviation {dev:.3e} unit {unit:.3e} bound {bound:.3e}")
    assert got.shape == want64.shape and dev <= bound, (tag, dev, unit, bound)          # (a NaN fails too)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ws(n):
    return torch.full((max(int(n), 256),), 0xFF, dtype=torch.uint8, device="cuda")           # (stale: bytes of a NaN)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _p(t):
    return t.data_ptr() if t is not None else None


def _both(fn):
    """fn(dtype) -> the float64 and the float32 restatement"""
    return fn(F64), fn(F32)


# ---------------------------------------------------------------------------------------------------- raw entry points
def _lstm_dev(w, normalize, peephole):
    pe = [_cuda(w[n]) if peephole else None for n in ("W_ci", "W_cf", "W_co")]
    gamma = _cuda(np.stack([w[n + "/gamma"] for n in ref.LSTM_LN])) if normalize else None
    beta = _cuda(np.stack([w[n + "/beta"] for n in ref.LSTM_LN])) if normalize else None
    return pe, gamma, beta


def raw_lstm_backward(y, c, w, dh, dcn, normalize, peephole, act=0, want=True, accumulate=False, into=None, ws_bytes=None, dys=None):
    """the forward (for its statistics), then the backward on a stale workspace and NaN-filled outputs.
    Returns (code, dy [B,H,W,dys], dc, {W_ci, W_cf, W_co, gamma, beta})"""
    B, H, W, F = c.shape
    L, st = _lib.lib(), runtime.stream_ptr()
    yd, cd = _cuda(y), _cuda(c)
    pe, gamma, beta = _lstm_dev(w, normalize, peephole)
    fws = _ws(L.vstab_convlstm_gates_workspace_bytes(B, H, W, F, int(normalize)))
    tmp = _nan(2, B, H, W, F)
    _lib.check(L.vstab_convlstm_gates(yd.data_ptr(), y.shape[3], cd.data_ptr(), _p(pe[0]), _p(pe[1]), _p(pe[2]), _p(gamma), _p(beta), B, H, W, F, 1.0,
                                      act, int(normalize), int(peephole), tmp[0].data_ptr(), tmp[1].data_ptr(), None, 0, fws.data_ptr(), fws.numel(), st))
    stats = [None, None]
    if normalize:
        for q, n in ((0, 3), (1, 2)):
            off = int(L.vstab_convlstm_gates_stats_offset(B, H, W, F, q))
            assert off > 0
            stats[q] = fws[off:off + B * n * 8].clone()
    dys = _up4(4 * F) if dys is None else dys
    dy, dc = _nan(B, H, W, dys), _nan(B, H, W, F)
    g = into if into is not None else {n: (_nan(H, W, F) if want and peephole else None) for n in ("W_ci", "W_cf", "W_co")}
    if into is None:
        g.update({n: (_nan(5, F) if want and normalize else None) for n in ("gamma", "beta")})
    need = int(L.vstab_convlstm_gates_backward_workspace_bytes(B, H, W, F, int(normalize), int(peephole)))
    ws = _ws(need if ws_bytes is None else ws_bytes)
    dhd, dcnd = (_cuda(dh) if dh is not None else None), (_cuda(dcn) if dcn is not None else None)
    code = L.vstab_convlstm_gates_backward(yd.data_ptr(), y.shape[3], cd.data_ptr(), _p(pe[0]), _p(pe[1]), _p(pe[2]), _p(gamma), _p(beta), _p(stats[0]),
                                           _p(stats[1]), _p(dhd), F, _p(dcnd), B, H, W, F, 1.0, act, int(normalize), int(peephole), dy.data_ptr(), dys,
                                           dc.data_ptr(), _p(g["W_ci"]), _p(g["W_cf"]), _p(g["W_co"]), _p(g["gamma"]), _p(g["beta"]), int(accumulate),
                                           ws.data_ptr(), need if ws_bytes is None else ws_bytes, st)
    torch.cuda.synchronize()
    return code, dy, dc, g


def _lstm_stage_ref(shape, normalize, peephole, activation="tanh", dh_none=False, dc_none=False):
    w, _, c, _, dh, dcn = gref.lstm_case(shape, normalize, peephole)
    y = gref.stage_y(shape, 4)
    dh, dcn = (None if dh_none else dh), (None if dc_none else dcn)
    cast = lambda a, dt: None if a is None else a.astype(dt)          # noqa: E731
    r64, r32 = _both(lambda dt: gref.lstm_gates_backward(y.astype(dt), c.astype(dt), ref.cast(w, dt), cast(dh, dt), cast(dcn, dt),
                                                         activation=activation, normalize=normalize, peephole=peephole))
    return (w, y, c, dh, dcn), r64, r32


def _check_lstm_stage(tag, F, out, r64, r32, normalize, peephole):
    _, dy, dc, g = out
    _close(f"{tag} dy", dy[..., :4 * F], r64[0], r32[0])
    _close(f"{tag} dc", dc, r64[1], r32[1])
    if peephole:
        for n in ("W_ci", "W_cf", "W_co"):
            _close(f"{tag} d{n}", g[n], r64[2][n], r32[2][n])
    if normalize:
        for leaf in ("gamma", "beta"):
            _close(f"{tag} d{leaf}", g[leaf], *(np.stack([r[2][f"{ln}/{leaf}"] for ln in ref.LSTM_LN]) for r in (r64, r32)))


@pytest.mark.parametrize("peephole", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_lstm_gates_backward_alone(name, normalize, peephole):
    shape = ref.SHAPES[name]
    (w, y, c, dh, dcn), r64, r32 = _lstm_stage_ref(shape, normalize, peephole)
    out = raw_lstm_backward(y, c, w, dh, dcn, normalize, peephole)
    _lib.check(out[0])
    _check_lstm_stage(f"lstm stage {name}", shape[4], out, r64, r32, normalize, peephole)


def _gru_dev(w, normalize):
    g = lambda names, leaf: _cuda(np.stack([w[n + leaf] for n in names])) if normalize else None          # noqa: E731
    return g(ref.GRU_LN[:2], "/gamma"), g(ref.GRU_LN[:2], "/beta"), g(ref.GRU_LN[2:], "/gamma"), g(ref.GRU_LN[2:], "/beta")


def raw_gru_backward(y, y2, h, u, w, dhn, du, drh, normalize, act=0, accumulate=False, into=None):
    """both stages, each on its own inputs.  Returns ((du, dy2, dh, {gamma, beta}), (dy, dh_added_to_zero, {gamma, beta}))"""
    B, H, W, F = h.shape
    L, st = _lib.lib(), runtime.stream_ptr()
    yd, y2d, hd, ud = _cuda(y), _cuda(y2), _cuda(h), _cuda(u)
    dhnd, dud, drhd = _cuda(dhn), _cuda(du), _cuda(drh)
    gg, gb, cg, cb = _gru_dev(w, normalize)
    fws = _ws(L.vstab_convgru_workspace_bytes(B, H, W, F, int(normalize)))
    tmp = _nan(3, B, H, W, F)
    off = int(L.vstab_convgru_stats_offset(B, H, W, F))
    _lib.check(L.vstab_convgru_gates(yd.data_ptr(), y.shape[3], hd.data_ptr(), F, _p(gg), _p(gb), B, H, W, F, int(normalize), tmp[0].data_ptr(), F,
                                     tmp[1].data_ptr(), fws.data_ptr(), fws.numel(), st))
    stats_g = fws[off:off + B * 16].clone() if normalize else None
    _lib.check(L.vstab_convgru_update(y2d.data_ptr(), y2.shape[3], hd.data_ptr(), F, ud.data_ptr(), _p(cg), _p(cb), B, H, W, F, act, int(normalize),
                                      tmp[2].data_ptr(), None, 0, fws.data_ptr(), fws.numel(), st))
    stats_c = fws[off:off + B * 8].clone() if normalize else None
    need = int(L.vstab_convgru_backward_workspace_bytes(B, H, W, F, int(normalize)))
    ws = _ws(need)
    new = lambda *s: _nan(*s) if normalize else None          # noqa: E731
    gu = into[0] if into is not None else {"gamma": new(F), "beta": new(F)}
    gg_ = into[1] if into is not None else {"gamma": new(2, F), "beta": new(2, F)}
    du_out, dy2, dh1 = _nan(B, H, W, F), _nan(B, H, W, _up4(F)), _nan(B, H, W, F)
    _lib.check(L.vstab_convgru_update_backward(y2d.data_ptr(), y2.shape[3], hd.data_ptr(), F, ud.data_ptr(), _p(cg), _p(cb), _p(stats_c), dhnd.data_ptr(),
                                               F, B, H, W, F, act, int(normalize), dy2.data_ptr(), dy2.shape[3], du_out.data_ptr(), dh1.data_ptr(), F,
                                               _p(gu["gamma"]), _p(gu["beta"]), int(accumulate), ws.data_ptr(), need, st))
    ws.fill_(0xFF)
    dy, dh2 = _nan(B, H, W, _up4(2 * F)), torch.zeros(B, H, W, F, device="cuda")
    _lib.check(L.vstab_convgru_gates_backward(yd.data_ptr(), y.shape[3], hd.data_ptr(), F, _p(gg), _p(gb), _p(stats_g), dud.data_ptr(),
                                              drhd.data_ptr(), F, B, H, W, F, int(normalize), dy.data_ptr(), dy.shape[3], dh2.data_ptr(), F,
                                              _p(gg_["gamma"]), _p(gg_["beta"]), int(accumulate), ws.data_ptr(), need, st))
    torch.cuda.synchronize()
    return (du_out, dy2, dh1, gu), (dy, dh2, gg_)


def _gru_stage_ref(shape, normalize, activation="tanh"):
    w, _, h, dhn, du, drh = gref.gru_case(shape, normalize)
    y, y2, u = gref.stage_y(shape, 2), gref.stage_y(shape, 1), gref.stage_u(shape)
    upd = _both(lambda dt: gref.gru_update_backward(y2.astype(dt), h.astype(dt), u.astype(dt), ref.cast(w, dt), dhn.astype(dt), activation, normalize))
    gat = _both(lambda dt: gref.gru_gates_backward(y.astype(dt), h.astype(dt), ref.cast(w, dt), du.astype(dt), drh.astype(dt), normalize))
    return (w, y, y2, h, u, dhn, du, drh), upd, gat


def _check_gru_stage(tag, F, out, upd, gat, normalize):
    (du_out, dy2, dh1, gu), (dy, dh2, gg) = out
    for n, (name, got) in enumerate((("du", du_out), ("dy2", dy2[..., :F]), ("dh", dh1))):
        _close(f"{tag} update {name}", got, upd[0][n], upd[1][n])
    _close(f"{tag} gates dy", dy[..., :2 * F], gat[0][0], gat[1][0])
    _close(f"{tag} gates dh", dh2, gat[0][1], gat[1][1])
    if normalize:
        for leaf in ("gamma", "beta"):
            _close(f"{tag} update d{leaf}", gu[leaf], upd[0][3][f"{ref.GRU_LN[2]}/{leaf}"], upd[1][3][f"{ref.GRU_LN[2]}/{leaf}"])
            _close(f"{tag} gates d{leaf}", gg[leaf], *(np.stack([r[2][f"{ln}/{leaf}"] for ln in ref.GRU_LN[:2]]) for r in gat))


@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_gru_stages_backward_alone(name, normalize):
    shape = ref.SHAPES[name]
    (w, y, y2, h, u, dhn, du, drh), upd, gat = _gru_stage_ref(shape, normalize)
    out = raw_gru_backward(y, y2, h, u, w, dhn, du, drh, normalize)
    _check_gru_stage(f"gru stage {name}", shape[4], out, upd, gat, normalize)


@pytest.mark.parametrize("act", ["relu", "identity"])
def test_other_activations_backward(act):
    shape = ref.SHAPES["odd"]
    (w, y, c, dh, dcn), r64, r32 = _lstm_stage_ref(shape, True, True, act)
    out = raw_lstm_backward(y, c, w, dh, dcn, True, True, act=ACTS[act])
    _lib.check(out[0])
    _check_lstm_stage(f"lstm stage {act}", shape[4], out, r64, r32, True, True)
    (w, y, y2, h, u, dhn, du, drh), upd, gat = _gru_stage_ref(shape, True, act)
    _check_gru_stage(f"gru stage {act}", shape[4], raw_gru_backward(y, y2, h, u, w, dhn, du, drh, True, act=ACTS[act]), upd, gat, True)


def test_absent_upstream_gradients_are_zero():
    shape = ref.SHAPES["odd"]
    for kw in (dict(dh_none=True), dict(dc_none=True)):
        (w, y, c, dh, dcn), r64, r32 = _lstm_stage_ref(shape, True, True, **kw)
        out = raw_lstm_backward(y, c, w, dh, dcn, True, True)
        _lib.check(out[0])
        _check_lstm_stage(f"lstm stage {sorted(kw)[0]}", shape[4], out, r64, r32, True, True)


@pytest.mark.parametrize("name", ["odd", "f1"])
def test_pad_channels_of_dy_are_zero(name):
    """F = 6 -> 24 gate channels in rows of 28 (and of 24 + the default's none: dys = 24 is covered by the stage tests); F = 1 -> 4 of 8"""
    shape = ref.SHAPES[name]
    F = shape[4]
    w, _, c, _, dh, dcn = gref.lstm_case(shape, True, True)
    code, dy, _, _ = raw_lstm_backward(gref.stage_y(shape, 4), c, w, dh, dcn, True, True, dys=4 * F + 4)
    _lib.check(code)
    assert dy.shape[3] == 4 * F + 4 and torch.equal(dy[..., 4 * F:], torch.zeros_like(dy[..., 4 * F:])) and not torch.isnan(dy).any()
    (w, y, y2, h, u, dhn, du, drh), _, _ = _gru_stage_ref(shape, True)
    (_, dy2, _, _), (dyg, _, _) = raw_gru_backward(y, y2, h, u, w, dhn, du, drh, True)
    for t, used in ((dy2, F), (dyg, 2 * F)):
        assert t.shape[3] == _up4(used) and not torch.isnan(t).any() and torch.equal(t[..., used:], torch.zeros_like(t[..., used:]))


# ---------------------------------------------------------------------------------------------------- whole cell
def _make(kind, shape, w, **kw):
    _, H, W, _, F, k = shape
    c = (cell.ConvLSTMCell if kind == "lstm" else cell.ConvGRUCell)([H, W], F, [k, k], **kw)
    c.assign_weights(w)
    return c


def _leaf(a):
    return _cuda(a).requires_grad_()


def _check_params(tag, params, r64, r32):
    assert set(params) == set(r64)
    for n, p in params.items():
        _close(f"{tag} d{n}", p.grad, r64[n], r32[n])


@pytest.mark.parametrize("peephole", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_lstm_cell_backward(name, normalize, peephole):
    shape = ref.SHAPES[name]
    w, x, c, h, dh, dcn = gref.lstm_case(shape, normalize, peephole)
    kw = dict(normalize=normalize, peephole=peephole)
    lc = _make("lstm", shape, w, differentiable=True, **kw)
    xd, cd, hd = _leaf(x), _leaf(c), _leaf(h)
    out, state = lc.call(xd, (cd, hd))
    assert out.grad_fn is not None and state.h is out
    ((out * _cuda(dh)).sum() + (state.c * _cuda(dcn)).sum()).backward()
    r64, r32 = _both(lambda dt: gref.lstm_call_backward(x, (c, h), w, dt, dh, dcn, **kw))
    tag = f"lstm cell {name}"
    _close(f"{tag} dx", xd.grad, r64[0], r32[0])
    _close(f"{tag} dc", cd.grad, r64[1][0], r32[1][0])
    _close(f"{tag} dh", hd.grad, r64[1][1], r32[1][1])
    _check_params(tag, lc.parameters(), r64[2], r32[2])


@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_gru_cell_backward(name, normalize):
    shape = ref.SHAPES[name]
    w, x, h, dhn = gref.gru_case(shape, normalize)[:4]
    gc = _make("gru", shape, w, differentiable=True, normalize=normalize)
    xd, hd = _leaf(x), _leaf(h)
    out, state = gc.call(xd, hd)
    assert state is out and out.grad_fn is not None
    (out * _cuda(dhn)).sum().backward()
    r64, r32 = _both(lambda dt: gref.gru_call_backward(x, h, w, dt, dhn, normalize=normalize))
    tag = f"gru cell {name}"
    _close(f"{tag} dx", xd.grad, r64[0], r32[0])
    _close(f"{tag} dh", hd.grad, r64[1], r32[1])
    _check_params(tag, gc.parameters(), r64[2], r32[2])


@pytest.mark.parametrize("with_state", [True, False], ids=["state", "zero"])
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_sequence_backward(kind, with_state):
    """T = 3 on `odd`; the loss mixes every output and the final state.  The forward, d inputs and d state equal T chained calls' to the
    bit; the chained calls' parameter gradients (autograd's own sums over the steps) stay within the same bounds"""
    shape = ref.SHAPES["odd"]
    w, xs, c, h, d_out, d_c, d_h = gref.sequence_case(kind)
    sc = _make(kind, shape, w, differentiable=True)
    xd, cd, hd = _leaf(xs), _leaf(c), _leaf(h)
    state = None if not with_state else ((cd, hd) if kind == "lstm" else hd)
    d_final = (d_c, d_h) if kind == "lstm" else d_h

    def loss_of(outs, final):
        loss = (outs * _cuda(d_out)).sum()
        return loss + ((final.c * _cuda(d_c)).sum() + (final.h * _cuda(d_h)).sum() if kind == "lstm" else (final * _cuda(d_h)).sum())

    outs, final = cell.run_sequence(sc, xd, state)
    loss_of(outs, final).backward()
    np_state = None if not with_state else ((c, h) if kind == "lstm" else h)
    r64, r32 = _both(lambda dt: gref.run_sequence_backward(kind, xs, np_state, w, dt, d_out, d_final))
    tag = f"{kind} sequence {'state' if with_state else 'zero'}"
    _close(f"{tag} d inputs", xd.grad, r64[0], r32[0])
    if with_state and kind == "lstm":
        _close(f"{tag} d c0", cd.grad, r64[1][0], r32[1][0])
        _close(f"{tag} d h0", hd.grad, r64[1][1], r32[1][1])
    elif with_state:
        _close(f"{tag} d h0", hd.grad, r64[1], r32[1])
    else:
        assert cd.grad is None and hd.grad is None
    _check_params(tag, sc.parameters(), r64[2], r32[2])
    # T chained calls
    seq_grads = {n: p.grad.clone() for n, p in sc.parameters().items()}
    for p in sc.parameters().values():
        p.grad = None
    x2, c2, h2 = _leaf(xs), _leaf(c), _leaf(h)
    zero = torch.zeros_like(outs[0])
    st = ((c2, h2) if kind == "lstm" else h2) if with_state else ((zero, zero) if kind == "lstm" else zero)
    chained = []
    for t in range(3):
        o, st = sc.call(x2[t], st)
        chained.append(o)
    assert torch.equal(torch.stack(chained), outs)
    assert (torch.equal(st.c, final.c) and torch.equal(st.h, final.h)) if kind == "lstm" else torch.equal(st, final)
    loss_of(torch.stack(chained), st).backward()
    # d inputs and d state to the bit: every sum on their way (upstream + carried dh) has two operands.  The parameter gradients are
    # summed over the steps by autograd here (rounded float32 step totals) and on the device there: within the bounds, not to the bit
    assert torch.equal(x2.grad, xd.grad)
    if with_state:
        assert torch.equal(h2.grad, hd.grad) and (kind != "lstm" or torch.equal(c2.grad, cd.grad))
    _check_params(f"{tag} chained", sc.parameters(), r64[2], r32[2])
    assert set(seq_grads) == set(w)


# ---------------------------------------------------------------------------------------------------- properties
def _grads_of(kind, shape, x, c, h, dh, dcn, w, detach_x=False):
    """(dx, dc, dh, parameter gradients) of one differentiable step on device tensors"""
    sc = _make(kind, shape, w, differentiable=True)
    xd, cd, hd = (x.clone().requires_grad_(not detach_x), c.clone().requires_grad_(), h.clone().requires_grad_())
    if kind == "lstm":
        out, state = sc.call(xd, (cd, hd))
        ((out * dh).sum() + (state.c * dcn).sum()).backward()
    else:
        (sc.call(xd, hd)[0] * dh).sum().backward()
    return xd.grad, cd.grad, hd.grad, {n: p.grad for n, p in sc.parameters().items()}


def _cases(shape):
    w, x, c, h, dh, dcn = gref.lstm_case(shape, True, True)
    wg, xg, hg, dhg = gref.gru_case(shape, True)[:4]
    return (("lstm", w) + tuple(_cuda(a) for a in (x, c, h, dh, dcn)), ("gru", wg) + tuple(_cuda(a) for a in (xg, hg, hg, dhg, dhg)))


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


def test_two_runs_give_the_same_bits():
    shape = ref.SHAPES["big"]
    for kind, w, x, c, h, dh, dcn in _cases(shape):
        a, b = _grads_of(kind, shape, x, c, h, dh, dcn, w), _grads_of(kind, shape, x, c, h, dh, dcn, w)
        assert all(_same(s, t) for s, t in zip(a[:3], b[:3])) and all(torch.equal(a[3][n], b[3][n]) for n in a[3])


def test_samples_are_independent():
    shape = ref.SHAPES["k5"]
    perm = torch.tensor([2, 0, 1], device="cuda")
    for kind, w, x, c, h, dh, dcn in _cases(shape):
        base = _grads_of(kind, shape, x, c, h, dh, dcn, w)
        moved = _grads_of(kind, shape, *(t[perm].contiguous() for t in (x, c, h, dh, dcn)), w)
        one = _grads_of(kind, shape, *(t[1:2].contiguous() for t in (x, c, h, dh, dcn)), w)
        for n in range(3):
            if base[n] is not None:
                assert torch.equal(moved[n], base[n][perm]) and torch.equal(one[n][0], base[n][1])


def test_needs_input_grad_is_honoured():
    shape = ref.SHAPES["odd"]
    for kind, w, x, c, h, dh, dcn in _cases(shape):
        full, nox = _grads_of(kind, shape, x, c, h, dh, dcn, w), _grads_of(kind, shape, x, c, h, dh, dcn, w, detach_x=True)
        assert nox[0] is None and _same(full[1], nox[1]) and torch.equal(full[2], nox[2])
        assert all(torch.equal(full[3][n], nox[3][n]) for n in full[3])
    # only one parameter asks: the others get none, and its gradient is the same
    w = gref.lstm_case(shape, True, True)[0]
    sc = _make("lstm", shape, w, differentiable=True)
    for n, p in sc.parameters().items():
        p.requires_grad_(n == "LayerNorm_2/gamma")
    _, _, x, c, h, dh, dcn = _cases(shape)[0]
    out, state = sc.call(x, (c, h))
    ((out * dh).sum() + (state.c * dcn).sum()).backward()
    want = _grads_of("lstm", shape, x, c, h, dh, dcn, w)[3]
    assert all((p.grad is None) != (n == "LayerNorm_2/gamma") for n, p in sc.parameters().items())
    assert torch.equal(sc.parameters()["LayerNorm_2/gamma"].grad, want["LayerNorm_2/gamma"])


def test_stale_workspaces_and_wrappers_agree():
    """the raw helpers run on 0xFF workspaces and NaN outputs; training's wrappers on fresh allocations: the same bits"""
    shape = ref.SHAPES["odd"]
    (w, y, c, dh, dcn), _, _ = _lstm_stage_ref(shape, True, True)
    _, dy, dc, g = raw_lstm_backward(y, c, w, dh, dcn, True, True)
    # the wrapper needs the forward's statistics: take them as raw_lstm_backward does
    B, H, W, F = c.shape
    L = _lib.lib()
    pe, gamma, beta = _lstm_dev(w, True, True)
    fws = torch.zeros(int(L.vstab_convlstm_gates_workspace_bytes(B, H, W, F, 1)), dtype=torch.uint8, device="cuda")
    tmp = _nan(2, B, H, W, F)
    yd, cd = _cuda(y), _cuda(c)
    _lib.check(L.vstab_convlstm_gates(yd.data_ptr(), y.shape[3], cd.data_ptr(), _p(pe[0]), _p(pe[1]), _p(pe[2]), _p(gamma), _p(beta), B, H, W, F, 1.0, 0, 1, 1,
                                      tmp[0].data_ptr(), tmp[1].data_ptr(), None, 0, fws.data_ptr(), fws.numel(), runtime.stream_ptr()))
    offs = [int(L.vstab_convlstm_gates_stats_offset(B, H, W, F, q)) for q in (0, 1)]
    stats = (fws[offs[0]:offs[0] + B * 24].clone(), fws[offs[1]:offs[1] + B * 16].clone())
    dy2, dc2, g2 = training.convlstm_gates_backward(yd, cd, _cuda(dh), _cuda(dcn), pe, gamma, beta, stats)
    assert torch.equal(dy2, dy) and torch.equal(dc2, dc) and all(torch.equal(g2[n], g[n]) for n in g)


def test_accumulate_adds():
    shape = ref.SHAPES["odd"]
    B, H, W, _, F, _ = shape
    (w, y, c, dh, dcn), _, _ = _lstm_stage_ref(shape, True, True)
    base = raw_lstm_backward(y, c, w, dh, dcn, True, True)[3]
    init = {n: torch.full_like(t, 0.5) for n, t in base.items()}
    got = raw_lstm_backward(y, c, w, dh, dcn, True, True, accumulate=True, into={n: t.clone() for n, t in init.items()})[3]
    for n in base:
        # (the sums are taken in double and rounded once: base rounds the sum, got the sum + 0.5 -- one rounding of each apart)
        assert torch.all((got[n] - (base[n] + init[n])).abs() <= EPS * (base[n].abs() + 0.5)), n
    (w, y, y2, h, u, dhn, du, drh), _, _ = _gru_stage_ref(shape, True)
    (_, _, _, gu), (_, _, gg) = raw_gru_backward(y, y2, h, u, w, dhn, du, drh, True)
    into = ({n: torch.full_like(t, 0.5) for n, t in gu.items()}, {n: torch.full_like(t, 0.5) for n, t in gg.items()})
    (_, _, _, gu2), (_, _, gg2) = raw_gru_backward(y, y2, h, u, w, dhn, du, drh, True, accumulate=True, into=into)
    for a, b in ((gu, gu2), (gg, gg2)):
        for n in a:
            assert torch.all((b[n] - (a[n] + 0.5)).abs() <= EPS * (a[n].abs() + 0.5)), n


def test_differentiable_forward_has_the_default_bits_and_reads_current_parameters():
    shape = ref.SHAPES["odd"]
    for kind, w, x, c, h, _, _ in _cases(shape):
        plain, diff = _make(kind, shape, w), _make(kind, shape, w, differentiable=True)
        state = (c, h) if kind == "lstm" else h
        want = plain.call(x, state)[0]
        assert torch.equal(diff.call(x, state)[0], want)                          # with a graph
        with torch.no_grad():
            assert torch.equal(diff.call(x, state)[0], want)                      # without
        xs = torch.stack([x, x.flip(0)])
        assert torch.equal(cell.run_sequence(diff, xs)[0], cell.run_sequence(plain, xs)[0])
        params = diff.parameters()
        name = "kernel" if kind == "lstm" else "candidate/kernel"
        assert all(p.is_leaf and p.requires_grad and p.is_cuda and tuple(p.shape) == tuple(w[n].shape) for n, p in params.items())
        with torch.no_grad():
            params[name].add_(0.25)               # (not a scaling: a layer norm would undo that to the bit)
        plain.assign_weights(dict(w, **{name: w[name] + np.float32(0.25)}))
        assert torch.equal(diff.call(x, state)[0], plain.call(x, state)[0]) and not torch.equal(plain.call(x, state)[0], want)
    with pytest.raises(ValueError):
        _make("lstm", shape, gref.lstm_case(shape, True, True)[0]).parameters()


def test_default_cells_still_carry_no_graph():
    shape = ref.SHAPES["odd"]
    w, x, c, h, _, _ = gref.lstm_case(shape, True, True)
    out, state = _make("lstm", shape, w).call(_leaf(x), (_leaf(c), _leaf(h)))
    assert out.grad_fn is None and state.c.grad_fn is None
    with torch.no_grad():
        out, _ = _make("lstm", shape, w, differentiable=True).call(_leaf(x), (_leaf(c), _leaf(h)))
    assert out.grad_fn is None


# ---------------------------------------------------------------------------------------------------- errors
def test_abi_errors():
    shape = ref.SHAPES["odd"]
    B, H, W, _, F, _ = shape
    (w, y, c, dh, dcn), _, _ = _lstm_stage_ref(shape, True, True)
    L = _lib.lib()
    need = int(L.vstab_convlstm_gates_backward_workspace_bytes(B, H, W, F, 1, 1))
    assert need > 0 and L.vstab_convlstm_gates_backward_workspace_bytes(B, H, W, F, 0, 0) == 0
    assert L.vstab_convlstm_gates_backward_workspace_bytes(B, H, W, 0, 1, 1) == 0 and L.vstab_convgru_backward_workspace_bytes(B, H, W, 0, 1) == 0
    assert L.vstab_convgru_backward_workspace_bytes(B, H, W, F, 0) == 0 and L.vstab_convgru_backward_workspace_bytes(B, H, W, F, 1) > 0
    assert L.vstab_convlstm_gates_stats_offset(B, H, W, F, 2) == 0 and L.vstab_convgru_stats_offset(B, 0, W, F) == 0
    assert raw_lstm_backward(y, c, w, dh, dcn, True, True, ws_bytes=need - 256)[0] == E_NOMEM
    yd, cd, dhd = _cuda(y), _cuda(c), _cuda(dh)
    dy, out = _nan(B, H, W, 4 * F), _nan(B, H, W, F)
    st = runtime.stream_ptr()

    def lstm(yp=yd.data_ptr(), Fv=F, act=0, normalize=0, dw=None, ws=None, ws_bytes=0, dys=4 * F):
        return L.vstab_convlstm_gates_backward(yp, 4 * F, cd.data_ptr(), None, None, None, None, None, None, None, dhd.data_ptr(), F, None, B, H, W, Fv, 1.0,
                                               act, normalize, 0, dy.data_ptr(), dys, out.data_ptr(), dw, None, None, None, None, 0, ws, ws_bytes, st)
    assert lstm(yp=None) == E_STATE
    assert lstm(normalize=1) == E_STATE                              # normalize without gamma / statistics
    assert lstm(dw=out.data_ptr()) == E_STATE                        # a peephole gradient without peepholes (and alone)
    assert lstm(Fv=0) == E_SHAPE and lstm(act=3) == E_SHAPE and lstm(dys=4 * F - 1) == E_SHAPE
    ws = _ws(need)
    pe, gamma, beta = _lstm_dev(w, True, True)
    full = lambda wp, nb: L.vstab_convlstm_gates_backward(yd.data_ptr(), 4 * F, cd.data_ptr(), _p(pe[0]), _p(pe[1]), _p(pe[2]), _p(gamma), _p(beta),  # noqa: E731
                                                          ws.data_ptr(), ws.data_ptr(), dhd.data_ptr(), F, None, B, H, W, F, 1.0, 0, 1, 1, dy.data_ptr(), 4 * F,
                                                          out.data_ptr(), None, None, None, None, None, 0, wp, nb, st)
    assert full(None, need) == E_STATE and full(ws.data_ptr() + 4, need) == E_ALIGN and full(ws.data_ptr(), need - 1) == E_NOMEM
    gru_u = lambda hp, Fv, act: L.vstab_convgru_update_backward(yd.data_ptr(), 4 * F, hp, F, cd.data_ptr(), None, None, None, dhd.data_ptr(), F, B, H, W, Fv,  # noqa: E731
                                                                act, 0, dy.data_ptr(), 4 * F, out.data_ptr(), out.data_ptr(), F, None, None, 0, None, 0, st)
    assert gru_u(None, F, 0) == E_STATE and gru_u(cd.data_ptr(), 0, 0) == E_SHAPE and gru_u(cd.data_ptr(), F, -1) == E_SHAPE
    gru_g = lambda drh, dys: L.vstab_convgru_gates_backward(yd.data_ptr(), 4 * F, cd.data_ptr(), F, None, None, None, cd.data_ptr(), drh, F, B, H, W, F, 0,  # noqa: E731
                                                            dy.data_ptr(), dys, out.data_ptr(), F, None, None, 0, None, 0, st)
    assert gru_g(None, 4 * F) == E_STATE and gru_g(dhd.data_ptr(), 2 * F - 1) == E_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dy).all()


def test_python_errors():
    shape = ref.SHAPES["odd"]
    B, H, W, _, F, _ = shape
    (w, y, c, dh, dcn), _, _ = _lstm_stage_ref(shape, False, False)
    yd, cd, dhd = _cuda(y), _cuda(c), _cuda(dh)
    for bad in (dict(y=yd[..., :-1].contiguous()), dict(dh=dhd[:, :-1]), dict(dh=dhd.double()), dict(dc_new=dhd.cpu()), dict(c=cd.half()),
                dict(gamma=torch.ones(5, F, device="cuda")), dict(dh=dhd.permute(0, 2, 1, 3))):
        args = dict(y=yd, c=cd, dh=dhd)
        args.update(bad)
        with pytest.raises(ValueError):
            training.convlstm_gates_backward(**args)
    with pytest.raises(ValueError):
        training.convgru_update_backward(yd, cd, cd, dhd[..., :-1])
    with pytest.raises(ValueError):
        training.convgru_gates_backward(yd, cd, cd, dhd, dhd.cpu())
    with pytest.raises(TypeError):
        cell.ConvLSTMCell([H, W], F, [3, 3], differentiabel=True)
    fresh = cell.ConvGRUCell([H, W], F, [3, 3], differentiable=True)
    with pytest.raises(ValueError):
        fresh.parameters()                                          # no weights yet

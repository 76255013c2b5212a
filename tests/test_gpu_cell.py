"""ConvLSTMCell / ConvGRUCell (coupe...cell, csrc/cell_ops.hip) against tests/cell_ref.py.

Bound of every comparison: 4 x the largest error of the float32 restatement against the float64 one on the same case (computed here, on
the CPU), floor 4 eps_fp32; the factor 4 is the SSIM tests' margin for another summation order.  Each comparison prints its measured
error and bound (pytest -s).  Inputs U(-1,1), fixed seeds, weights scaled for O(1) pre-activations (cell_ref.make_weights); that every
normalised quantity has a per-sample standard deviation >= 0.1 is checked in tests/test_cell_ref_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, cell, runtime
from tests import cell_ref as ref

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(np.float32).eps)
E_SHAPE, E_NOMEM, E_STATE = -1, -4, -6
SHAPE_IDS = list(ref.SHAPES)


# ---------------------------------------------------------------------------------------------------- cases (also read by the CPU tests)
def _seed(shape, *flags):
    return 1000 + 37 * shape[1] + 11 * shape[4] + sum(1 << n for n, f in enumerate(flags) if f)


@functools.lru_cache(maxsize=None)
def lstm_case(shape, normalize, peephole):
    s = _seed(shape, normalize, peephole)
    return (ref.make_weights("lstm", s, shape, normalize, peephole),) + ref.make_inputs(s + 1, shape)


@functools.lru_cache(maxsize=None)
def gru_case(shape, normalize):
    s = _seed(shape, normalize) + 500
    x, _, h = ref.make_inputs(s + 1, shape)
    return ref.make_weights("gru", s, shape, normalize), x, h


@functools.lru_cache(maxsize=None)
def stage_y(shape, gates):
    return ref.make_y(2000 + shape[1] + gates, shape, gates)


@functools.lru_cache(maxsize=None)
def sequence_case(kind):
    shape = ref.SHAPES["odd"]
    return ref.make_weights(kind, 3000, shape, True), ref.make_inputs(3001, shape, T=3)[0]


def _close(tag, got, want64, got32):
    got = got.detach().cpu().numpy()
    err, bound = ref.max_err(got, want64), max(4.0 * ref.max_err(got32, want64), 4.0 * EPS)
    print(f"[cell {tag}] err {err:.3e} bound {bound:.3e}")
    assert got.shape == want64.shape and err <= bound, (tag, err, bound)          # (a NaN fails too)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lstm(shape, normalize, peephole, **kw):
    _, H, W, _, F, k = shape
    c = cell.ConvLSTMCell([H, W], F, [k, k], normalize=normalize, peephole=peephole, **kw)
    c.assign_weights(lstm_case(shape, normalize, peephole)[0])
    return c


def _gru(shape, normalize, **kw):
    _, H, W, _, F, k = shape
    c = cell.ConvGRUCell([H, W], F, [k, k], normalize=normalize, **kw)
    c.assign_weights(gru_case(shape, normalize)[0])
    return c


# ---------------------------------------------------------------------------------------------------- raw entry points
def _ws(n):
    return torch.full((max(int(n), 256),), 0xFF, dtype=torch.uint8, device="cuda")           # (bytes of a NaN)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def raw_lstm(y, c, w, normalize, peephole, forget_bias=1.0, act=0, ws_bytes=None):
    B, H, W, F = c.shape
    L = _lib.lib()
    yd, cd = _cuda(y), _cuda(c)
    pe = [_cuda(w[n]) if peephole else None for n in ("W_ci", "W_cf", "W_co")]
    gamma = _cuda(np.stack([w[n + "/gamma"] for n in ref.LSTM_LN])) if normalize else None
    beta = _cuda(np.stack([w[n + "/beta"] for n in ref.LSTM_LN])) if normalize else None
    ws = _ws(L.vstab_convlstm_gates_workspace_bytes(B, H, W, F, int(normalize)) if ws_bytes is None else ws_bytes)
    c_out, h_out = _nan(B, H, W, F), _nan(B, H, W, F)
    p = lambda t: t.data_ptr() if t is not None else None            # noqa: E731
    code = L.vstab_convlstm_gates(yd.data_ptr(), y.shape[3], cd.data_ptr(), p(pe[0]), p(pe[1]), p(pe[2]), p(gamma), p(beta), B, H, W, F,
                                  forget_bias, act, int(normalize), int(peephole), c_out.data_ptr(), h_out.data_ptr(), None, 0, ws.data_ptr(),
                                  ws.numel() if ws_bytes is None else ws_bytes, runtime.stream_ptr())
    torch.cuda.synchronize()
    return code, c_out, h_out


def raw_gru(y, y2, h, w, normalize, act=0):
    """gates on y, then update on y2 with the gates' u: returns (r h, u, h')"""
    B, H, W, F = h.shape
    L = _lib.lib()
    yd, y2d, hd = _cuda(y), _cuda(y2), _cuda(h)
    g = lambda names, leaf: _cuda(np.stack([w[n + leaf] for n in names])) if normalize else None          # noqa: E731
    gg, gb, cg, cb = g(ref.GRU_LN[:2], "/gamma"), g(ref.GRU_LN[:2], "/beta"), g(ref.GRU_LN[2:], "/gamma"), g(ref.GRU_LN[2:], "/beta")
    ws = _ws(L.vstab_convgru_workspace_bytes(B, H, W, F, int(normalize)))
    rh, u, h_out = _nan(B, H, W, F), _nan(B, H, W, F), _nan(B, H, W, F)
    p = lambda t: t.data_ptr() if t is not None else None            # noqa: E731
    _lib.check(L.vstab_convgru_gates(yd.data_ptr(), y.shape[3], hd.data_ptr(), F, p(gg), p(gb), B, H, W, F, int(normalize), rh.data_ptr(), F,
                                     u.data_ptr(), ws.data_ptr(), ws.numel(), runtime.stream_ptr()))
    _lib.check(L.vstab_convgru_update(y2d.data_ptr(), y2.shape[3], hd.data_ptr(), F, u.data_ptr(), p(cg), p(cb), B, H, W, F, act, int(normalize),
                                      h_out.data_ptr(), None, 0, ws.data_ptr(), ws.numel(), runtime.stream_ptr()))
    torch.cuda.synchronize()
    return rh, u, h_out


@pytest.mark.parametrize("peephole", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_lstm_gates_alone(name, normalize, peephole):
    shape = ref.SHAPES[name]
    w, _, c, _ = lstm_case(shape, normalize, peephole)
    y = stage_y(shape, 4)
    code, c_out, h_out = raw_lstm(y, c, w, normalize, peephole)
    _lib.check(code)
    kw = dict(normalize=normalize, peephole=peephole)
    c64, h64 = ref.lstm_gates(y.astype(F64), c.astype(F64), ref.cast(w, F64), **kw)
    c32, h32 = ref.lstm_gates(y, c, ref.cast(w, F32), **kw)
    _close(f"lstm gates {name} c'", c_out, c64, c32)
    _close(f"lstm gates {name} h'", h_out, h64, h32)


@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_gru_gates_and_update_alone(name, normalize):
    shape = ref.SHAPES[name]
    w, _, h = gru_case(shape, normalize)
    y, y2 = stage_y(shape, 2), stage_y(shape, 1)
    rh, u, h_out = raw_gru(y, y2, h, w, normalize)
    out = {}
    for dt in (F64, F32):
        wd = ref.cast(w, dt)
        rh_r, u_r = ref.gru_gates(y.astype(dt), h.astype(dt), wd, normalize)
        out[dt] = (rh_r, u_r, ref.gru_update(y2.astype(dt), h.astype(dt), u_r, wd, normalize=normalize))
    for n, got in enumerate((rh, u, h_out)):
        _close(f"gru stage {name} {('r h', 'u', 'h_new')[n]}", got, out[F64][n], out[F32][n])


@pytest.mark.parametrize("act", ["relu", "identity"])
def test_other_activations(act):
    shape = ref.SHAPES["odd"]
    w, _, c, h = lstm_case(shape, True, True)
    y = stage_y(shape, 4)
    code, c_out, h_out = raw_lstm(y, c, w, True, True, act={"relu": 1, "identity": 2}[act])
    _lib.check(code)
    c64, h64 = ref.lstm_gates(y.astype(F64), c.astype(F64), ref.cast(w, F64), activation=act)
    c32, h32 = ref.lstm_gates(y, c, ref.cast(w, F32), activation=act)
    _close(f"lstm gates {act} c'", c_out, c64, c32)
    _close(f"lstm gates {act} h'", h_out, h64, h32)
    wg, _, hg = gru_case(shape, True)
    y2 = stage_y(shape, 1)
    _, u, h_out = raw_gru(stage_y(shape, 2), y2, hg, wg, True, act={"relu": 1, "identity": 2}[act])
    un = u.cpu().numpy()
    _close(f"gru update {act}", h_out, ref.gru_update(y2.astype(F64), hg.astype(F64), un.astype(F64), ref.cast(wg, F64), activation=act),
           ref.gru_update(y2, hg, un, ref.cast(wg, F32), activation=act))


def test_layer_norm_known_answer_on_the_device():
    """y constant per gate, no peephole, c constant, identity activation, beta of j / i / f constant (0.25 / 40 / 40): j = 0.25 and
    i = f = sigmoid(40) = 1 exactly, c' = 0.5 + 0.25 before its layer norm -- constants of a few bits, which float32 sums exactly, so
    the restatement's float32 form is exact as well.  Then LN(c') is beta_c to the bit and h' = sigmoid(beta_o) beta_c to 2 ulp (the
    device's exp against numpy's)."""
    shape = ref.SHAPES["big"]
    B, H, W, _, F, _ = shape
    w = dict(lstm_case(shape, True, False)[0])
    for ln, v in (("LayerNorm", 0.25), ("LayerNorm_1", 40.0), ("LayerNorm_2", 40.0)):
        w[ln + "/beta"] = np.full(F, v, F32)
    y = np.repeat(np.array([0.25, -1.25, 0.75, 2.0], F32), F)[None, None, None, :] * np.ones((B, H, W, 1), F32)
    c = np.full((B, H, W, F), 0.5, F32)
    code, c_out, h_out = raw_lstm(y, c, w, True, False, act=2)
    _lib.check(code)
    c32, h32 = ref.lstm_gates(y, c, ref.cast(w, F32), activation="identity", peephole=False)
    assert np.array_equal(c32, np.broadcast_to(w["LayerNorm_4/beta"], c32.shape))
    assert np.array_equal(c_out.cpu().numpy(), c32)
    ulps = np.abs(h_out.cpu().numpy().astype(F64) - h32) / np.spacing(np.abs(h32))
    print(f"[cell ln known answer] h' max {ulps.max():.2f} ulp")
    assert ulps.max() <= 2.0


# ---------------------------------------------------------------------------------------------------- whole cell
@pytest.mark.parametrize("peephole", [True, False], ids=["peep", "nopeep"])
@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_lstm_cell(name, normalize, peephole):
    shape = ref.SHAPES[name]
    w, x, c, h = lstm_case(shape, normalize, peephole)
    out, state = _lstm(shape, normalize, peephole).call(_cuda(x), (_cuda(c), _cuda(h)))
    assert isinstance(state, cell.LSTMStateTuple) and state.h is out
    kw = dict(normalize=normalize, peephole=peephole)
    h64, (c64, _) = ref.lstm_call(x, (c, h), w, F64, **kw)
    h32, (c32, _) = ref.lstm_call(x, (c, h), w, F32, **kw)
    _close(f"lstm cell {name} c'", state.c, c64, c32)
    _close(f"lstm cell {name} h'", out, h64, h32)


@pytest.mark.parametrize("normalize", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_gru_cell(name, normalize):
    shape = ref.SHAPES[name]
    w, x, h = gru_case(shape, normalize)
    out, state = _gru(shape, normalize).call(_cuda(x), _cuda(h))
    assert state is out
    _close(f"gru cell {name} h'", out, ref.gru_call(x, h, w, F64, normalize=normalize)[0], ref.gru_call(x, h, w, F32, normalize=normalize)[0])


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_sequence(kind):
    shape = ref.SHAPES["odd"]
    _, H, W, _, F, k = shape
    w, xs = sequence_case(kind)
    c = (cell.ConvLSTMCell if kind == "lstm" else cell.ConvGRUCell)([H, W], F, [k, k])
    c.assign_weights(w)
    xd = _cuda(xs)
    outs, final = cell.run_sequence(c, xd)
    o64, f64 = ref.run_sequence(kind, xs, None, w, F64)
    o32, f32 = ref.run_sequence(kind, xs, None, w, F32)
    _close(f"{kind} sequence outputs", outs, o64, o32)
    if kind == "lstm":
        _close("lstm sequence final c", final.c, f64[0], f32[0])
        _close("lstm sequence final h", final.h, f64[1], f32[1])
    else:
        _close("gru sequence final h", final, f64, f32)
    zero = torch.zeros_like(outs[0])
    state = cell.LSTMStateTuple(zero, zero) if kind == "lstm" else zero
    for t in range(3):
        o, state = c.call(xd[t], state)
        assert torch.equal(o, outs[t])
    assert (torch.equal(state.c, final.c) and torch.equal(state.h, final.h)) if kind == "lstm" else torch.equal(state, final)
    # a given state continues the sequence
    o2, _ = cell.run_sequence(c, xd[2:], state=(cell.run_sequence(c, xd[:2])[1]))
    assert torch.equal(o2[0], outs[2])


# ---------------------------------------------------------------------------------------------------- properties
def _both(shape):
    w, x, c, h = lstm_case(shape, True, True)
    wg, xg, hg = gru_case(shape, True)
    lc, gc = _lstm(shape, True, True), _gru(shape, True)
    return ((lambda xs, cs, hs: torch.stack(list(lc.call(xs, (cs, hs))[1])), _cuda(x), _cuda(c), _cuda(h)),
            (lambda xs, cs, hs: gc.call(xs, hs)[0], _cuda(xg), _cuda(hg), _cuda(hg)))


def test_two_runs_give_the_same_bits():
    for fn, x, c, h in _both(ref.SHAPES["big"]):
        assert torch.equal(fn(x, c, h), fn(x, c, h))


def test_samples_are_independent():
    for fn, x, c, h in _both(ref.SHAPES["k5"]):
        base = fn(x, c, h)
        perm = torch.tensor([2, 0, 1], device="cuda")
        assert torch.equal(fn(x[perm].contiguous(), c[perm].contiguous(), h[perm].contiguous()), base.index_select(base.dim() - 4, perm))
    for fn, x, c, h in _both(ref.SHAPES["big"]):
        assert torch.equal(fn(x[:1].contiguous(), c[:1].contiguous(), h[:1].contiguous()).select(-4, 0), fn(x, c, h).select(-4, 0))


def test_stale_buffers_change_nothing():
    shape = ref.SHAPES["odd"]
    w, x, c, h = lstm_case(shape, True, True)
    lc = _lstm(shape, True, True)
    args = (_cuda(x), (_cuda(c), _cuda(h)))
    base = lc.call(*args)[1]
    b = lc.buffers(shape[0], args[0].device)
    for t in (b.y, b.conv_ws, b.gate_ws):
        t.view(torch.uint8).fill_(0xFF)
    again = lc.call(*args)[1]
    assert torch.equal(again.c, base.c) and torch.equal(again.h, base.h)
    wg, xg, hg = gru_case(shape, True)
    gc = _gru(shape, True)
    base = gc.call(_cuda(xg), _cuda(hg))[0]
    b = gc.buffers(shape[0], _cuda(xg).device)
    for t in (b.y, b.y2, b.u, b.conv_ws, b.gate_ws):
        t.view(torch.uint8).fill_(0xFF)
    assert torch.equal(gc.call(_cuda(xg), _cuda(hg))[0], base)


def test_results_carry_no_graph():
    shape = ref.SHAPES["odd"]
    w, x, c, h = lstm_case(shape, True, True)
    t = [_cuda(a).requires_grad_() for a in (x, c, h)]
    out, state = _lstm(shape, True, True).call(t[0], (t[1], t[2]))
    assert out.grad_fn is None and state.c.grad_fn is None and not out.requires_grad
    wg, xg, hg = gru_case(shape, True)
    out, _ = _gru(shape, True).call(_cuda(xg).requires_grad_(), _cuda(hg).requires_grad_())
    assert out.grad_fn is None and not out.requires_grad
    outs, _ = cell.run_sequence(_gru(shape, True), _cuda(xg)[None].requires_grad_())
    assert outs.grad_fn is None


# ---------------------------------------------------------------------------------------------------- errors
def test_python_errors():
    shape = ref.SHAPES["odd"]
    B, H, W, Cx, F, k = shape
    w, x, c, h = lstm_case(shape, True, True)
    lc = _lstm(shape, True, True)
    xd, cd, hd = _cuda(x), _cuda(c), _cuda(h)
    for bad in ((xd, (cd[:, :-1], hd)), (xd, (cd, hd[..., :-1])), (xd.cpu(), (cd, hd)), (xd, (cd.cpu(), hd)), (xd.double(), (cd, hd)),
                (xd, (cd, hd.half())), (xd[..., :-1], (cd, hd)), (xd, (cd[:1], hd[:1]))):
        with pytest.raises(ValueError):
            lc.call(*bad)
    gc = _gru(shape, True)
    for bad in ((xd, hd[:, :-1]), (xd.cpu(), hd), (xd, hd.double())):
        with pytest.raises(ValueError):
            gc.call(*bad)
    for kw in (dict(data_format="channels_first"), dict(kernel=[2, 2]), dict(kernel=[3, 5]), dict(kernel=[9, 9]), dict(activation="gelu"),
               dict(activation=torch.sigmoid)):
        args = dict(shape=[H, W], filters=F, kernel=[k, k])
        args.update(kw)
        for cls in (cell.ConvLSTMCell, cell.ConvGRUCell):
            with pytest.raises(NotImplementedError):
                cls(**args)
    assert cell.ConvGRUCell([H, W], F, [k, k], activation=torch.relu)._act == 1 and cell.ConvLSTMCell([H, W], F, [k, k], activation=None)._act == 2
    fresh = cell.ConvLSTMCell([H, W], F, [k, k])
    for drop in ("kernel", "W_co", "LayerNorm_4/beta"):
        with pytest.raises(ValueError):
            fresh.assign_weights({n: a for n, a in w.items() if n != drop})
    with pytest.raises(ValueError):
        fresh.assign_weights(dict(w, W_ci=w["W_ci"][:-1]))
    with pytest.raises(ValueError):
        fresh.call(xd, (cd, hd))                                    # no weights yet
    wg = gru_case(shape, True)[0]
    with pytest.raises(ValueError):
        cell.ConvGRUCell([H, W], F, [k, k]).assign_weights({n: a for n, a in wg.items() if n != "candidate/LayerNorm/gamma"})


def test_abi_errors():
    shape = ref.SHAPES["odd"]
    B, H, W, _, F, _ = shape
    w, _, c, _ = lstm_case(shape, True, True)
    y = stage_y(shape, 4)
    L = _lib.lib()
    need = int(L.vstab_convlstm_gates_workspace_bytes(B, H, W, F, 1))
    assert need > 0 and L.vstab_convlstm_gates_workspace_bytes(B, H, W, F, 0) == 0 and L.vstab_convgru_workspace_bytes(B, H, W, 0, 1) == 0
    assert raw_lstm(y, c, w, True, True, ws_bytes=need - 256)[0] == E_NOMEM
    yd, cd, out = _cuda(y), _cuda(c), _nan(B, H, W, F)
    st = runtime.stream_ptr()
    args = lambda yp, Fv: (yp, 4 * F, cd.data_ptr(), None, None, None, None, None, B, H, W, Fv, 1.0, 0, 0, 0, out.data_ptr(), out.data_ptr(),  # noqa: E731
                           None, 0, None, 0, st)
    assert L.vstab_convlstm_gates(*args(None, F)) == E_STATE
    assert L.vstab_convlstm_gates(*args(yd.data_ptr(), 0)) == E_SHAPE
    assert L.vstab_convlstm_gates(yd.data_ptr(), 4 * F, cd.data_ptr(), None, None, None, None, None, B, H, W, F, 1.0, 0, 1, 0, out.data_ptr(),
                                  out.data_ptr(), None, 0, None, 0, st) == E_STATE               # normalize without gamma / workspace
    assert L.vstab_convgru_gates(yd.data_ptr(), 4 * F, None, F, None, None, B, H, W, F, 0, out.data_ptr(), F, out.data_ptr(), None, 0, st) == E_STATE
    assert L.vstab_convgru_update(yd.data_ptr(), 4 * F, cd.data_ptr(), F, cd.data_ptr(), None, None, B, H, W, 0, 0, 0, out.data_ptr(), None, 0,
                                  None, 0, st) == E_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(out).all()

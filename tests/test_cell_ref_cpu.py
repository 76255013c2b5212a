"""Pins tests/cell_ref.py (the numpy restatement of ConvLSTMCell / ConvGRUCell that the GPU tests compare against) without a GPU:
known answers of the layer norm, the order of the gate blocks, the cells' limit cases, which c each peephole sees, the SAME
convolution against torch, the sequence helper, and the conditioning of the GPU tests' inputs."""
import numpy as np
import pytest
import torch

from tests import cell_ref as ref

F64 = np.float64
SHAPE = (2, 6, 10, 5, 6, 3)         # B, H, W, Cx, F, k


def _rel(a, b):
    return ref.max_err(a, b) / max(float(np.max(np.abs(b))), 1e-300)


# ---------------------------------------------------------------------------------------------------- layer norm
def test_layer_norm_of_a_constant_is_beta():
    rng = np.random.RandomState(0)
    gamma, beta = rng.uniform(0.5, 1.5, 4), rng.uniform(-1, 1, 4)
    for dt in (np.float64, np.float32):
        v = np.full((2, 3, 5, 4), 0.75, dt)         # (a few bits: its sums are exact in float32 too)
        out = ref.layer_norm(v, gamma.astype(dt), beta.astype(dt))
        assert np.array_equal(out, np.broadcast_to(beta.astype(dt), v.shape))


def test_layer_norm_of_two_values():
    rng = np.random.RandomState(1)
    gamma, beta = rng.uniform(0.5, 1.5, 4), rng.uniform(-1, 1, 4)
    v = np.empty((2, 4, 6, 4), F64)
    v[:, ::2], v[:, 1::2] = 3.0, 1.0                # half the numbers of a sample each: mean 2, variance 1
    out = ref.layer_norm(v, gamma, beta)
    want = np.where(v > 2.0, gamma + beta, -gamma + beta)
    assert _rel(out, want) <= 1e-12


def test_layer_norm_output_moments():
    rng = np.random.RandomState(2)
    v = rng.standard_normal((3, 5, 7, 4)) * np.array([0.3, 1.0, 4.0]).reshape(3, 1, 1, 1) + 2.0
    out = ref.layer_norm(v, np.ones(4), np.zeros(4))
    var = v.var(axis=(1, 2, 3))
    assert np.max(np.abs(out.mean(axis=(1, 2, 3)))) <= 1e-12
    assert _rel(out.var(axis=(1, 2, 3)), var / (var + 1e-12)) <= 1e-12
    # per sample: scaling one sample leaves the others alone
    v2 = v.copy()
    v2[1] *= 10.0
    out2 = ref.layer_norm(v2, np.ones(4), np.zeros(4))
    assert np.array_equal(out2[0], out[0]) and np.array_equal(out2[2], out[2])


# ---------------------------------------------------------------------------------------------------- gate order
def _lstm_plain(seed=3):
    w = ref.make_weights("lstm", seed, SHAPE, normalize=False, peephole=False)
    x, c, h = ref.make_inputs(seed + 1, SHAPE)
    return w, x, c, h


@pytest.mark.parametrize("block", [0, 1, 2, 3], ids=["j", "i", "f", "o"])
def test_lstm_gate_order(block):
    """a kernel that is zero except for one output block, zero bias, forget_bias 0: the other gates see 0, so sigmoid = 1/2, act(j) = 0"""
    w, x, c, h = _lstm_plain()
    F = SHAPE[4]
    k = np.zeros_like(w["kernel"])
    k[..., block * F:(block + 1) * F] = w["kernel"][..., block * F:(block + 1) * F]
    w = {"kernel": k, "bias": np.zeros_like(w["bias"])}
    hn, (cn, _) = ref.lstm_call(x, (c, h), w, F64, forget_bias=0.0, normalize=False, peephole=False)
    g = ref.conv_same(np.concatenate([x, h], 3).astype(F64), k.astype(F64))[..., block * F:(block + 1) * F]
    assert float(np.abs(g).mean()) > 0.2
    c = c.astype(F64)
    want_c = {0: 0.5 * c + 0.5 * np.tanh(g), 1: 0.5 * c, 2: c * ref.sigmoid(g), 3: 0.5 * c}[block]
    want_h = (ref.sigmoid(g) if block == 3 else 0.5) * np.tanh(want_c)
    assert _rel(cn, want_c) <= 1e-12 and _rel(hn, want_h) <= 1e-12


# ---------------------------------------------------------------------------------------------------- limit cases
def test_lstm_zero_weights_and_a_large_forget_bias_keep_c():
    w, x, c, h = _lstm_plain()
    w = {n: np.zeros_like(a) for n, a in w.items()}
    _, (cn, _) = ref.lstm_call(x, (c, h), w, F64, forget_bias=30.0, normalize=False, peephole=False)
    assert ref.max_err(cn, c) <= 1e-12              # f = sigmoid(30) = 1 - 9e-14, i act(j) = 0.5 tanh(0) = 0


def test_lstm_a_large_negative_i_freezes_the_input():
    w, x, c, h = _lstm_plain()
    F = SHAPE[4]
    w["bias"] = w["bias"].copy()
    w["bias"][F:2 * F] = -40.0
    _, (cn, _) = ref.lstm_call(x, (c, h), w, F64, normalize=False, peephole=False)
    y = ref.conv_same(np.concatenate([x, h], 3).astype(F64), w["kernel"].astype(F64)) + w["bias"]
    assert ref.max_err(cn, c * ref.sigmoid(y[..., 2 * F:3 * F] + 1.0)) <= 1e-12


def _gru_plain(seed=5):
    w = ref.make_weights("gru", seed, SHAPE, normalize=False)
    x, _, h = ref.make_inputs(seed + 1, SHAPE)
    return w, x, h


def test_gru_u_to_one_keeps_h():
    w, x, h = _gru_plain()
    F = SHAPE[4]
    w["gates/bias"] = np.concatenate([w["gates/bias"][:F], np.full(F, 40.0, np.float32)])
    hn, _ = ref.gru_call(x, h, w, F64, normalize=False)
    assert ref.max_err(hn, h) <= 1e-12


def test_gru_u_to_zero_gives_the_candidate_and_r_to_zero_forgets_h():
    w, x, h = _gru_plain()
    F = SHAPE[4]
    w["gates/bias"] = np.full(2 * F, -40.0, np.float32)                 # r -> 0 and u -> 0
    hn, _ = ref.gru_call(x, h, w, F64, normalize=False)
    y2 = ref.conv_same(np.concatenate([x, np.zeros_like(h)], 3).astype(F64), w["candidate/kernel"].astype(F64)) + w["candidate/bias"]
    assert ref.max_err(hn, np.tanh(y2)) <= 1e-12
    # r -> 0 alone (u from an x-only gate kernel): another h moves h' only through u h, not through the candidate
    w["gates/bias"] = np.concatenate([np.full(F, -40.0, np.float32), np.zeros(F, np.float32)])
    w["gates/kernel"] = w["gates/kernel"].copy()
    w["gates/kernel"][:, :, SHAPE[3]:] = 0.0
    h2 = -h[:, ::-1].copy()
    a, _ = ref.gru_call(x, h, w, F64, normalize=False)
    b, _ = ref.gru_call(x, h2, w, F64, normalize=False)
    y = ref.conv_same(np.concatenate([x, h], 3).astype(F64), w["gates/kernel"].astype(F64)) + w["gates/bias"]
    u = ref.sigmoid(y[..., F:])
    assert ref.max_err(a - u * h, b - u * h2) <= 1e-12
    assert ref.max_err(a, b) > 1e-2


# ---------------------------------------------------------------------------------------------------- peephole
@pytest.mark.parametrize("normalize", [True, False])
def test_peephole_sees_old_c_for_i_f_and_new_c_for_o(normalize):
    w = ref.cast(ref.make_weights("lstm", 7, SHAPE, normalize, peephole=True), F64)
    _, c, _ = ref.make_inputs(8, SHAPE)
    c = c.astype(F64)
    y = ref.make_y(9, SHAPE, 4).astype(F64)
    F = SHAPE[4]
    cn, hn = ref.lstm_gates(y, c, w, normalize=normalize)
    # by hand, without the layer norm: i, f from the OLD c; o from the NEW, un-normalised c'
    if not normalize:
        i = ref.sigmoid(y[..., F:2 * F] + w["W_ci"] * c)
        f = ref.sigmoid(y[..., 2 * F:3 * F] + w["W_cf"] * c + 1.0)
        c1 = c * f + i * np.tanh(y[..., :F])
        assert ref.max_err(cn, c1) <= 1e-12
        assert ref.max_err(hn, ref.sigmoid(y[..., 3 * F:] + w["W_co"] * c1) * np.tanh(c1)) <= 1e-12
    for wrong in ("new_for_if", "old_for_o"):
        _, hw = ref.lstm_gates(y, c, w, normalize=normalize, peephole_wrong=wrong)
        assert ref.max_err(hw, hn) > 1e-3, wrong


# ---------------------------------------------------------------------------------------------------- convolution, sequence
@pytest.mark.parametrize("k", [1, 3, 5])
def test_conv_same_matches_torch(k):
    rng = np.random.RandomState(10 + k)
    x, w = rng.standard_normal((2, 6, 9, 5)), rng.standard_normal((k, k, 5, 7))
    want = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(3, 2, 0, 1), padding=(k - 1) // 2)
    assert _rel(ref.conv_same(x, w), want.permute(0, 2, 3, 1).numpy()) <= 1e-12


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_run_sequence_is_stepping_by_hand(kind):
    w = ref.make_weights(kind, 20, SHAPE, True)
    x, c, h = ref.make_inputs(21, SHAPE, T=3)
    state = (c, h) if kind == "lstm" else h
    outs, final = ref.run_sequence(kind, x, state, w, F64)
    call = ref.lstm_call if kind == "lstm" else ref.gru_call
    s = state
    for t in range(3):
        o, s = call(x[t], s, w, F64)
        assert np.array_equal(o, outs[t])
    assert all(np.array_equal(a, b) for a, b in zip(final, s)) if kind == "lstm" else np.array_equal(final, s)
    z, _ = ref.run_sequence(kind, x, None, w, F64)
    zero = np.zeros_like(c)
    o0, _ = call(x[0], (zero, zero) if kind == "lstm" else zero, w, F64)
    assert np.array_equal(z[0], o0)


# ---------------------------------------------------------------------------------------------------- conditioning of the GPU tests' inputs
def _min_std(trace):
    return min(float(v.std(axis=(1, 2, 3)).min()) for v in trace)


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_gpu_test_inputs_are_well_conditioned(name):
    """every quantity a layer norm is applied to in a GPU test case has per-sample standard deviation >= 0.1 in float64, so
    rsqrt(var + 1e-12) is well conditioned and the error bounds of tests/test_gpu_cell.py mean something"""
    import tests.test_gpu_cell as g
    shape = ref.SHAPES[name]
    for peephole in (True, False):
        tr = []
        w, x, c, h = g.lstm_case(shape, True, peephole)
        ref.lstm_call(x, (c, h), w, F64, peephole=peephole, trace=tr)
        ref.lstm_gates(g.stage_y(shape, 4).astype(F64), c.astype(F64), ref.cast(w, F64), peephole=peephole, trace=tr)
        assert len(tr) == 10 and _min_std(tr) >= 0.1
    tr = []
    w, x, h = g.gru_case(shape, True)
    ref.gru_call(x, h, w, F64, trace=tr)
    ref.gru_gates(g.stage_y(shape, 2).astype(F64), h.astype(F64), ref.cast(w, F64), trace=tr)
    ref.gru_update(g.stage_y(shape, 1).astype(F64), h.astype(F64), h.astype(F64), ref.cast(w, F64), trace=tr)
    assert len(tr) == 6 and _min_std(tr) >= 0.1
    if name == "odd":
        for kind in ("lstm", "gru"):
            tr = []
            w, xs = g.sequence_case(kind)
            ref.run_sequence(kind, xs, None, w, F64, trace=tr)
            assert _min_std(tr) >= 0.1


def test_synthetic_weights_follow_the_reference_initialisers():
    from coupe.optical_flow_based_deep_video_stabilization_amd import cell
    w = cell.ConvLSTMCell([6, 10], 6, [3, 3], normalize=False).synthetic_weights(1, 5)
    assert set(w) == set(ref.weight_shapes("lstm", 6, 10, 5, 6, 3, False)) and not w["bias"].any()
    w = cell.ConvGRUCell([6, 10], 6, [3, 3], normalize=False).synthetic_weights(1, 5)
    assert np.all(w["gates/bias"] == 1) and not w["candidate/bias"].any()
    w = cell.ConvGRUCell([6, 10], 6, [3, 3]).synthetic_weights(1, 5)
    assert {n: a.shape for n, a in w.items()} == ref.weight_shapes("gru", 6, 10, 5, 6, 3, True)
    assert all(np.all(a == 1) for n, a in w.items() if n.endswith("gamma")) and not any(a.any() for n, a in w.items() if n.endswith("beta"))
    assert w["gates/LayerNorm/gamma"].dtype == np.float32

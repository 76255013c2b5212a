"""GPU parity of the NLDF drop-in against the oracle at its only geometry (352x352): end to end, and stage
by stage with teacher forcing -- every stage's fp64 reference is computed on the CPU from the tensor the kernel itself read (the
trunk's pools, or the workspace views of `Model.internals()`), so a stage's bound holds that stage's rounding alone, and every
sample of the batch is compared.  No reference is sub-sampled: the largest one (Fea_P2_Deconv, 127 GFLOP per sample in fp64) is
evaluated on all rows, columns, channels and samples."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import NLDF as vnldf, vgg16 as vvgg, _lib, runtime
from oracle import vstab_oracle as vo

pytestmark = pytest.mark.gpu

F64 = torch.float64
B = 2
EPS32 = 2.0 ** -23
LAYER_TOL = 2e-4                       # one fp32 MFMA layer against fp64, relative to max(1, max|ref|): the bound of test_gpu_vgg.py
HW = (176, 88, 44, 22, 11)             # pool1..pool5 of a 352x352 input
CAT_C = (768, 640, 512, 384, 256)      # cat_k = [Fea_Pk | Fea_Pk_LC | Fea_P(k+1)_Up]
FEA = 128


def _readback(m):
    t = {name: v.cpu() for name, v in m.internals().items()}
    t["Fea_Global_ws"] = t.pop("Fea_Global")
    for name in ("Fea_Global", "Local_Fea", "Score", "Prob"):
        t[name] = getattr(m, name).cpu()
    return t


@pytest.fixture(scope="module")
def run():
    """One trunk pass and one head pass with the weights every stage test refers to -- AFTER a pass with other head weights on the
    same context, so that all of them also check that a second vstab_nldf_load takes effect (test_reload_takes_effect)."""
    dd = vvgg.synthetic_data_dict(seed=5)
    hw = vnldf.synthetic_head_weights(seed=6, gain=1.5)           # scores of order 10: probabilities not saturated
    x = torch.rand(B, 352, 352, 3, generator=torch.Generator().manual_seed(1))
    x[1] *= torch.linspace(0.2, 1.0, 352)[None, :, None]          # two different images, also in their global statistics
    m = vnldf.Model(vgg_data_dict=dd, head_weights=vnldf.synthetic_head_weights(seed=16, gain=1.5))
    m.build_model(x.cuda(), B)
    first = {name: getattr(m, name).cpu() for name in ("Fea_Global", "Score", "Prob")}
    ctx_first = m.vgg._ctx
    m.set_head_weights(hw)
    prob = m.build_model(x.cuda(), B, reuse=False, scope="NLDF")
    assert m.vgg._ctx is ctx_first                                 # the same context: the second load replaced the first
    torch.cuda.synchronize()
    pools = [getattr(m.vgg, f"pool{k}").cpu() for k in range(1, 6)]
    return SimpleNamespace(m=m, dd=dd, hw=hw, x=x, first=first, prob=prob.cpu(), pools=pools, t=_readback(m))


def _var(hw, name):
    return torch.from_numpy(hw[name + "/W"]).double(), torch.from_numpy(hw[name + "/b"]).double()


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _conv_ref(hw, name, x_nhwc, pad, relu):
    r = vo.nldf_conv(_nchw(x_nhwc), *_var(hw, name), pad)
    return _nhwc(torch.relu(r) if relu else r), _nhwc(r)


def _compare(failures, name, got, ref, bound):
    """Largest error of every sample against `bound`; prints each figure and notes the ones that miss."""
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    assert not torch.isnan(got).any(), name
    for n in range(got.shape[0]):
        err = float((got[n].double() - ref[n]).abs().max())
        print(f"NLDF stage {name} sample {n}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            failures.append((name, n, err, bound))


def _layer_bound(ref):
    return LAYER_TOL * max(1.0, float(ref.abs().max()))


# --------------------------------------------------------------------------- Model.internals()
def test_internals_are_views_of_the_workspace(run):
    m = run.m
    views = m.internals()
    want = {"G1": (B, 7, 7, FEA), "G2": (B, 3, 3, FEA), "Local_Score": (B, 176, 176, 2), "Global_Score": (B, 1, 1, 2)}
    want.update({f"cat{k + 1}": (B, HW[k], HW[k], CAT_C[k]) for k in range(5)})
    lo, hi = m._ws.data_ptr(), m._ws.data_ptr() + m._ws.numel()
    assert hi - lo == _lib.lib().vstab_nldf_workspace_bytes(B)
    spans = []
    for name, shape in want.items():
        v = views[name]
        assert tuple(v.shape) == shape and v.dtype == torch.float32 and v.is_contiguous(), name
        assert v.untyped_storage().data_ptr() == m._ws.untyped_storage().data_ptr(), name          # no copy
        assert lo <= v.data_ptr() and v.data_ptr() + 4 * v.numel() <= hi and v.data_ptr() % 256 == 0, name
        spans.append((v.data_ptr(), v.data_ptr() + 4 * v.numel()))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))      # the buffers do not overlap
    assert torch.equal(views["cat5"].cpu(), m.internals()["cat5"].cpu())


# --------------------------------------------------------------------------- stage by stage, teacher-forced
def test_global_branch_stages(run):
    """Fea_Global_1 (5x5 VALID + ReLU) from pool5, Fea_Global_2 (5x5 VALID + ReLU) from G1, Fea_Global (3x3 VALID, linear) from G2."""
    t, bad = run.t, []
    for name, src, out, relu in (("Fea_Global_1", run.pools[4], t["G1"], True), ("Fea_Global_2", t["G1"], t["G2"], True),
                                 ("Fea_Global", t["G2"], t["Fea_Global"], False)):
        ref, pre = _conv_ref(run.hw, name, src, 0, relu)
        _compare(bad, name, out, ref, _layer_bound(ref))
        assert float(pre.min()) < -10 * _layer_bound(ref), name            # the ReLU, or its absence, is visible in this case
        assert (float(out.min()) >= 0) == relu, name
    assert torch.equal(t["Fea_Global"], t["Fea_Global_ws"])                 # the B * FEA copy out of the workspace, every sample
    assert not bad, bad


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_local_feature_stage(run, k):
    """Fea_Pk (3x3 SAME + ReLU) = channels [0, 128) of cat_k, from pool_k."""
    bad = []
    ref, pre = _conv_ref(run.hw, f"Fea_P{k}", run.pools[k - 1], 1, True)
    assert float(pre.min()) < 0
    _compare(bad, f"Fea_P{k}", run.t[f"cat{k}"][..., :FEA], ref, _layer_bound(ref))
    assert not bad, bad


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_contrast_stage(run, k):
    """Fea_Pk_LC = channels [128, 256) of cat_k, from channels [0, 128) of the same buffer.  Bound 8 EPS32 max|input|: nine additions
    cost at most 8u sum|x| <= 72 u M, 9 u M after the division by 9, the subtraction adds 2 u M: 11 u M < 16 u M, u = 2^-24."""
    bad = []
    src = run.t[f"cat{k}"][..., :FEA]
    ref = _nhwc(vo.nldf_contrast(_nchw(src)))
    _compare(bad, f"Fea_P{k}_LC", run.t[f"cat{k}"][..., FEA:2 * FEA], ref, 8 * EPS32 * float(src.abs().max()))
    assert not bad, bad


@pytest.mark.parametrize("k", [5, 4, 3, 2])
def test_transposed_convolution_stage(run, k):
    """Fea_Pk_Deconv (5x5 stride 2 SAME + ReLU): cat_(k-1)[..., 256:] from all of cat_k -- in full, and separately on the first and
    last two output rows and columns, so that a failure names the edge."""
    bad = []
    src, out = run.t[f"cat{k}"], run.t[f"cat{k - 1}"][..., 2 * FEA:]
    n_out = HW[k - 2]
    pre = vo.nldf_deconv(_nchw(src), *_var(run.hw, f"Fea_P{k}_Deconv"), n_out)
    ref = _nhwc(torch.relu(pre))
    assert float(pre.min()) < 0 and out.shape[3] == CAT_C[k - 2] - 2 * FEA
    bound = _layer_bound(ref)
    name = f"Fea_P{k}_Deconv"
    _compare(bad, name + " top 2 rows", out[:, :2], ref[:, :2], bound)
    _compare(bad, name + " bottom 2 rows", out[:, -2:], ref[:, -2:], bound)
    _compare(bad, name + " left 2 columns", out[:, :, :2], ref[:, :, :2], bound)
    _compare(bad, name + " right 2 columns", out[:, :, -2:], ref[:, :, -2:], bound)
    _compare(bad, name, out, ref, bound)
    assert not bad, bad


def test_local_fea_and_score_stages(run):
    """Local_Fea (1x1, 768 -> 640) from cat1, Local_Score (1x1, 640 -> 2) from Local_Fea, Global_Score (1x1, 128 -> 2) from
    Fea_Global; all linear.  The two 2-column outputs run the unsplit (ksplit = 1) launch that only this head reaches."""
    t, bad = run.t, []
    for name, src, out in (("Local_Fea", t["cat1"], t["Local_Fea"]), ("Local_Score", t["Local_Fea"], t["Local_Score"]),
                           ("Global_Score", t["Fea_Global"], t["Global_Score"])):
        ref, _ = _conv_ref(run.hw, name, src, 0, False)
        _compare(bad, name, out, ref, _layer_bound(ref))
    assert not bad, bad


def test_score_and_prob(run):
    t = run.t
    # Score = Local_Score + the sample's Global_Score: one rounded fp32 addition, so bit for bit
    assert torch.equal(t["Score"], t["Local_Score"] + t["Global_Score"])
    # Prob against the fp64 two-way softmax of that Score: a quotient of values <= 1 from two expf, one addition, one division
    ref = torch.softmax(t["Score"].double(), dim=3)[..., 0:1]
    bad = []
    _compare(bad, "Prob", t["Prob"], ref, 8 * EPS32)
    assert not bad, bad
    assert 0.02 < float(ref.std())                                # the case is not degenerate
    assert float(t["Prob"].min()) >= 0 and float(t["Prob"].max()) <= 1


def test_samples_differ(run):
    """Without this a swapped or repeated sample index could hide: the two samples' tensors differ by far more than the bounds."""
    t = run.t
    for name, a in (("Fea_Global", t["Fea_Global"]), ("Global_Score", t["Global_Score"]), ("cat5", t["cat5"]),
                    ("Fea_P5_Up", t["cat4"][..., 2 * FEA:]), ("Local_Score", t["Local_Score"])):
        diff = float((a[0] - a[1]).abs().max())
        print(f"NLDF samples differ: {name} {diff:.3e} (scale {float(a.abs().max()):.3e})")
        assert diff > 100 * LAYER_TOL * max(1.0, float(a.abs().max())), (name, diff)


def test_reload_takes_effect(run):
    """The fixture ran the head with other weights first, then loaded run.hw on the same context and ran again: every stage test of
    this file compares that second run with the reference for run.hw.  Here: the first run really was a different network."""
    for name in ("Fea_Global", "Score", "Prob"):
        a, b = run.first[name], run.t[name]
        diff = float((a - b).abs().max())
        assert diff > (0.1 if name == "Prob" else 100 * LAYER_TOL * max(1.0, float(b.abs().max()))), (name, diff)
    ref, _ = _conv_ref(run.hw, "Global_Score", run.t["Fea_Global"], 0, False)
    assert float((run.t["Global_Score"].double() - ref).abs().max()) <= _layer_bound(ref)


def test_nldf_vs_oracle(run):
    """End to end against the oracle's own trunk and head, both samples."""
    m = run.m
    ref = vo.nldf_build_model(run.x, run.dd, run.hw, torch.float64)
    assert run.prob.shape == (B, 176, 176, 1)
    for n in range(B):
        for name, tol in (("Fea_Global", 1e-3), ("Local_Fea", 1e-3), ("Score", 1e-3), ("Prob", 2e-3)):
            got, r = run.t[name][n:n + 1].double(), ref[name][n:n + 1]
            scale = max(1.0, float(r.abs().max()))
            assert float((got - r).abs().max()) <= tol * scale, (name, n, float((got - r).abs().max()), scale)
    assert 0.02 < float(ref["Prob"].std())                       # the case is not degenerate
    assert float(run.prob.min()) >= 0 and float(run.prob.max()) <= 1
    assert torch.equal(run.prob, run.t["Prob"]) and m.Prob.shape == (B, 176, 176, 1)


# --------------------------------------------------------------------------- saturated scores
@pytest.mark.parametrize("sign", [1, -1])
def test_saturated_probabilities_are_exact(run, sign):
    """Global_Score bias (+200, -200): Score[..., 0] - Score[..., 1] is about 400, exp(-400) underflows to 0 in fp32 and Prob is
    exactly 1 (0 in the reverse case).  Without the subtraction of the maximum exp(200) would overflow and Prob would be NaN."""
    hw = dict(run.hw)
    hw["Global_Score/b"] = np.array([200.0 * sign, -200.0 * sign], dtype=np.float32)
    m = run.m
    try:
        m.set_head_weights(hw)
        prob = m.build_model(run.x.cuda(), B).cpu()
        score = m.Score.cpu()
    finally:
        m.set_head_weights(run.hw)
    assert float(((score[..., 0] - score[..., 1]) * sign).min()) > 300
    assert torch.isfinite(prob).all()
    assert torch.equal(prob, torch.full_like(prob, 1.0 if sign > 0 else 0.0))


# --------------------------------------------------------------------------- the C ABI itself
def _abi_forward(ctx_h, pools, batch, prob, score, local_fea, fea_global, ws_ptr, ws_bytes):
    arr = (C.c_void_p * 5)(*pools)
    return _lib.lib().vstab_nldf_forward(ctx_h, arr, batch, prob, score, local_fea, fea_global, ws_ptr, ws_bytes, runtime.stream_ptr())


def _loaded_context(run):
    m = run.m
    m.set_head_weights(run.hw)
    m._load(m.vgg._ctx)
    return m.vgg._ctx, [getattr(m.vgg, f"pool{k}").data_ptr() for k in range(1, 6)]


def test_unwritten_workspace_is_never_read(run):
    """The workspace and the output start as NaN (all-ones bytes), and the optional outputs are NULL so that Local_Fea lands in the
    workspace too: no stage output may hold a NaN afterwards, and Prob equals the Model's (the head has no atomics: same bits)."""
    ctx, pools = _loaded_context(run)
    nws = _lib.lib().vstab_nldf_workspace_bytes(B)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    prob = torch.full((B, 176, 176, 1), float("nan"), device="cuda")
    assert torch.isnan(ws[:64].view(torch.float32)).all()
    with torch.cuda.device(ws.device):
        assert _abi_forward(ctx._h, pools, B, prob.data_ptr(), None, None, None, ws.data_ptr(), nws) == 0
    torch.cuda.synchronize()
    views = vnldf.workspace_views(ws, B)
    assert set(views) == {"G1", "G2", "Fea_Global", "cat1", "cat2", "cat3", "cat4", "cat5", "Local_Fea", "Local_Score", "Global_Score"}
    for name, v in views.items():
        assert not torch.isnan(v).any(), name
    assert not torch.isnan(prob).any()
    assert torch.equal(views["Local_Fea"].cpu(), run.t["Local_Fea"]) and torch.equal(prob.cpu(), run.t["Prob"])


def test_abi_error_codes(run):
    E_SHAPE, E_ALIGN, E_NOMEM, E_STATE = -1, -2, -4, -6             # include/vstab.h
    ctx, pools = _loaded_context(run)
    L = _lib.lib()
    nws = L.vstab_nldf_workspace_bytes(B)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device="cuda")
    prob = torch.full((B, 176, 176, 1), 7.0, device="cuda")
    assert ws.data_ptr() % 256 == 0
    fresh = runtime.Context(ctx.device)
    try:
        assert _abi_forward(fresh._h, pools, B, prob.data_ptr(), None, None, None, ws.data_ptr(), nws) == E_STATE      # forward before load
        assert b"vstab_nldf_load" in L.vstab_last_error(fresh._h)
    finally:
        fresh.close()
    assert _abi_forward(ctx._h, pools, B, prob.data_ptr(), None, None, None, ws.data_ptr(), nws - 1) == E_NOMEM        # one byte short
    assert _abi_forward(ctx._h, pools, B, prob.data_ptr(), None, None, None, ws.data_ptr() + 16, nws) == E_ALIGN       # workspace + 16 bytes
    for k in range(5):
        off = list(pools)
        off[k] += 4
        assert _abi_forward(ctx._h, off, B, prob.data_ptr(), None, None, None, ws.data_ptr(), nws) == E_ALIGN, k       # pool + 4 bytes
    for batch in (0, 65):
        assert _abi_forward(ctx._h, pools, batch, prob.data_ptr(), None, None, None, ws.data_ptr(), nws) == E_SHAPE, batch
        assert L.vstab_nldf_workspace_bytes(batch) == 0
        assert L.vstab_nldf_workspace_layout(batch, (_lib.VstabWsEntry * 16)(), 16) == E_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(prob.cpu(), torch.full((B, 176, 176, 1), 7.0))        # a refused call writes nothing


def test_nldf_errors():
    with pytest.raises(ValueError):
        vnldf.Model(vgg_data_dict=vvgg.synthetic_data_dict(1))            # no head weights, no seed
    m = vnldf.Model(seed=3)
    with pytest.raises(ValueError):
        m.build_model(torch.zeros(1, 256, 256, 3, device="cuda"), 1)
    with pytest.raises(ValueError):
        m.build_model(torch.zeros(2, 352, 352, 3, device="cuda"), 1)
    with pytest.raises(RuntimeError):
        m.internals()                                                     # nothing has run yet

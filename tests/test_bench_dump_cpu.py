"""bench.py --dump-outputs without a GPU: what dump_outputs writes for a step's outputs, whole or as a fixed sample."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("vstab_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _step_outputs(B=2, H=40, W=56):
    g = torch.Generator().manual_seed(3)
    flows = {f"predict_flow{k}": torch.randn(B, H >> (k - 1), W >> (k - 1), 2, generator=g) for k in (6, 5, 4, 3)}
    flows["predict_flow2"] = torch.randn(B, H - 2, W - 2, 2, generator=g)
    flows["flow"] = flows["predict_flow2"]                 # the library's alias of predict_flow2
    return flows, torch.randn(B, H, W, 2, generator=g), torch.rand(B, H, W, 3, generator=g)


def test_dump_writes_every_output_whole_within_the_budget(tmp_path):
    bench = _bench()
    flows, outflow, warped = _step_outputs()
    bench.dump_outputs((flows, outflow, warped), str(tmp_path))
    want = {k: v for k, v in flows.items() if k != "flow"}
    want.update(outflow=outflow, warped=warped)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        a = np.load(os.path.join(tmp_path, k + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy()), k


def test_dump_samples_a_larger_output_the_same_way_every_time(tmp_path):
    bench = _bench()
    out = _step_outputs(B=4, H=96, W=128)
    total = sum(v.numel() * 4 for k, v in out[0].items() if k != "flow") + (out[1].numel() + out[2].numel()) * 4
    budget = total // 5
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d), budget=budget)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 7
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert sum(a.nbytes for a in got.values()) <= budget
    for n, a in got.items():
        assert a.dtype == np.float32 and a.ndim == 1 and a.size > 0
        assert np.array_equal(a, np.load(tmp_path / "b" / n)), n           # a fixed sample: the same elements on every run
    # the sample is a strided subset of the flattened array
    full = out[2].numpy().reshape(-1)
    w = got["warped.npy"]
    off = int(np.flatnonzero(full == w[0])[0])
    stride = int(np.flatnonzero(full == w[1])[0]) - off
    assert np.array_equal(w, full[off::stride])

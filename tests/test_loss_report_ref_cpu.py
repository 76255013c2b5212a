"""tests/loss_report_ref.py -- the numpy restatement the GPU tests of the loss report lean on -- against the oracle, the quantisation
rule of the uint8 previews at hand-made values, and the share of pixels tests/test_gpu_loss_report.py may leave out of its exact
comparison, computed for that test's own inputs from the oracle alone."""
import numpy as np
import torch

from oracle import vstab_oracle as vo
from tests import loss_report_ref as ref


def _case(seed=3, B=2, H=23, W=31, sizes=((1, 1), (2, 3), (4, 5), (9, 12), (23, 31))):
    rng = np.random.default_rng(seed)
    stab = rng.random((B, H, W, 6), dtype=np.float32)
    unstab = rng.random((B, H, W, 3), dtype=np.float32)
    flows = {k: ((rng.random((B, h, w, 2), dtype=np.float32) - np.float32(0.5)) * np.float32(1.4) * np.asarray([w, h], np.float32))
             for k, (h, w) in zip(ref.LEVELS, sizes)}
    return flows, stab, unstab


def test_lossterm_and_warped_frame_match_the_oracle():
    flows, stab, unstab = _case()
    for k in ref.LEVELS:
        loss, warped = ref.lossterm(flows[k], stab[..., :3], unstab)
        oloss, owarped = vo.lossterm(torch.from_numpy(flows[k]), stab[..., :3], unstab)
        assert abs(loss - float(oloss)) <= 1e-12 * max(1.0, abs(float(oloss))), k
        assert np.abs(warped - owarped.numpy()).max() <= 1e-12, k
        tv = ref.total_variation(flows[k])
        assert abs(tv - float(vo.total_variation(torch.from_numpy(flows[k])))) <= 1e-12 * tv, k


def test_level_terms_add_up_to_the_oracles_loss_main():
    flows, stab, unstab = _case()
    mse, tv, total, per = ref.level_terms(flows, stab, unstab, (0,), (1.0,), vo.TV_WEIGHTS)
    want = float(vo.loss_main({k: torch.from_numpy(v) for k, v in flows.items()}, stab[..., :3], unstab))
    assert abs(total - want) <= 1e-12 * max(1.0, abs(want))
    assert abs(mse.sum() + tv.sum() - total) <= 1e-15 * max(1.0, abs(total))
    assert abs(per[0] - mse.sum()) <= 1e-15
    # two weighted targets: each target's terms are the one-target terms on its slice
    mse2, tv2, total2, per2 = ref.level_terms(flows, stab, unstab, (0, 3), (1.0, 0.25), vo.TV_WEIGHTS)
    other = ref.level_terms(flows, stab[..., 3:], unstab, (0,), (1.0,), vo.TV_WEIGHTS)
    assert np.abs(mse2 - (mse + 0.25 * other[0])).max() <= 1e-15
    assert np.abs(tv2 - tv).max() == 0.0 and abs(per2[1] - other[3][0]) <= 1e-15


def test_inference_batchnorm_matches_the_oracle():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((2, 3, 4, 8))
    beta, mean = rng.standard_normal(8), rng.standard_normal(8)
    var = rng.random(8)
    var[2] = 0.0
    got = ref.bn_lrelu_inference(z, beta, mean, var)
    want = vo.bn_lrelu(torch.from_numpy(z), torch.from_numpy(beta), torch.from_numpy(mean), torch.from_numpy(var)).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_quantisation_rule_at_hand_made_values():
    """fix_image_tf(., 1): x 255, saturated, truncated toward zero"""
    v = np.asarray([0.0, 1.0, 254.999 / 255.0, -1e-9, 1.5, 0.5, 1.0 / 255.0, 0.999 / 255.0])
    assert ref.fix_image(v, 1).tolist() == [0, 255, 254, 0, 255, 127, 1, 0]
    assert ref.fix_image(np.float32(2.0) * v.astype(np.float32), 2.0).tolist() == ref.fix_image(v.astype(np.float32), 1).tolist()
    from coupe.optical_flow_based_deep_video_stabilization_amd import utils
    t = torch.from_numpy(v.astype(np.float32))
    assert utils.fix_image_tf(t, 1).tolist() == ref.fix_image(v.astype(np.float32), 1).tolist()
    assert utils.fix_image_tf(t, 1).dtype == torch.uint8


def test_share_of_pixels_near_a_quantisation_step_in_the_gpu_tests_inputs():
    """tests/test_gpu_loss_report.py compares uint8 previews exactly except within 1e-3 of a step of the quantiser, and caps that
    share at 1 %.  For its inputs the oracle alone puts the share here (a uniform value spends 2e-3 of its range there; samples that
    leave the frame warp to ~0, where the saturating quantiser has no step)."""
    flows, stab, unstab = ref.gpu_case()
    near = total = 0
    for k in ref.LEVELS:
        _, warped = vo.lossterm(torch.from_numpy(flows[k]), stab[..., :3], unstab)
        v = 255.0 * warped.numpy()
        near += int(ref.near_quantisation_step(v).sum())
        total += v.size
        assert np.abs(v[1]).max() == 0.0, k                          # the far-outside sample: M == 0, an all-zero frame
        inside = np.abs(v[0]) > 1e-6
        assert 0.2 <= inside.mean() <= 0.9 or v[0].size < 100, (k, inside.mean())      # a good share leaves the frame, a good share stays
    print(f"near a quantisation step: {near} of {total} = {near / total:.3%}")
    assert near / total <= 0.01

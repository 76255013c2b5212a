"""The loader's host side without a GPU: `plan_epoch` against the step-by-step restatement of the reference's index bookkeeping
(tests/data_loader_ref.py: RefPlan, which shares no code with it), the data-parallel slicing, the constructors' validation and the
path constructor's directory walk."""
from collections import Counter

import numpy as np
import pytest

from coupe.optical_flow_based_deep_video_stabilization_amd import data_loader as dl
from tests.data_loader_ref import RefPlan

SKIP = [1, 9, 17, 25, 28, 29, 30, 31, 32]
COUNTS = [33, 40, 35]
TOTAL = (1 + 8) + (8 + 8) + (3 + 8)          # candidate offsets N - 32, plus the eight zeros, per clip


@pytest.mark.parametrize("is_train", [True, False])
@pytest.mark.parametrize("batch_size", [1, 3, 4, 5])               # 36 entries: 5 leaves a short last batch
@pytest.mark.parametrize("seed", range(5))
def test_plan_epoch_equals_the_restated_plan(seed, batch_size, is_train):
    ref = RefPlan(COUNTS, SKIP, batch_size, is_train, np.random.RandomState(seed))
    want = ref.epoch()
    got = dl.plan_epoch(COUNTS, SKIP, batch_size, is_train, np.random.RandomState(seed))
    assert got == want
    assert len(got) == ref.num_itr == -(-TOTAL // batch_size)
    # the last batch is short exactly when the total is not a multiple of the batch size
    assert all(len(b) == batch_size for b in got[:-1])
    assert len(got[-1]) == (TOTAL % batch_size or batch_size)
    # every (clip, offset) entry exactly once per epoch, offset 0 nine times
    drawn = Counter(s for b in got for s in b)
    for clip, n in enumerate(COUNTS):
        assert drawn[(clip, 0)] == 9
        assert all(drawn[(clip, o)] == 1 for o in range(1, n - 32))
    assert sum(drawn.values()) == TOTAL and set(c for c, _ in drawn) == {0, 1, 2}
    if not is_train:                                                   # evaluation: clip by clip, the entries in list order
        flat = [s for b in got for s in b]
        assert flat == [(c, o) for c, n in enumerate(COUNTS) for o in list(range(n - 32)) + [0] * 8]


def test_numpy_global_state_gives_the_same_picks():
    """the reference draws from np.random: a RandomState in the global one's state makes the same picks"""
    np.random.seed(11)
    state = np.random.get_state()
    rs = np.random.RandomState()
    rs.set_state(state)
    got = dl.plan_epoch(COUNTS, SKIP, 4, True, rs)
    want = RefPlan(COUNTS, SKIP, 4, True, np.random).epoch()
    assert got == want


def test_length_33_has_one_candidate_offset_plus_eight_zeros():
    assert dl.candidate_offsets(33, SKIP) == [0] * 9
    assert dl.candidate_offsets(35, SKIP) == [0, 1, 2] + [0] * 8
    plan = dl.plan_epoch([33], SKIP, 4, True, np.random.RandomState(0))
    assert [len(b) for b in plan] == [4, 4, 1] and all(s == (0, 0) for b in plan for s in b)


def test_a_second_epoch_rebuilds_the_plan():
    rng, ref = np.random.RandomState(3), RefPlan(COUNTS, SKIP, 4, True, np.random.RandomState(3))
    first, second = dl.plan_epoch(COUNTS, SKIP, 4, True, rng), dl.plan_epoch(COUNTS, SKIP, 4, True, rng)
    assert first == ref.epoch() and second == ref.epoch()
    assert first != second and Counter(s for b in first for s in b) == Counter(s for b in second for s in b)


class _HostLoader(dl.Data_Loader):
    """the loader's planning and slicing with the device side cut off: what is under test here is host arithmetic"""

    def __init__(self, batch_size, is_train, rng, rank, world_size):
        self.frame_counts, self._skip_i32 = COUNTS, np.asarray(SKIP, np.int32)
        self.batch_size, self.is_train, self.rng, self.rank, self.world_size = batch_size, is_train, rng, rank, world_size
        self._plan = None

    def _assemble(self, samples):
        return (np.asarray(samples, np.int64).reshape(len(samples), 2),) * 3

    def epoch(self):
        out = []
        while True:
            feed, is_end, short = self.feed_the_network()
            if is_end:
                return out
            out.append((list(self.last_samples), short))


@pytest.mark.parametrize("world_size", [2, 4])
@pytest.mark.parametrize("batch_size", [1, 3, 5])                  # 5: the last global batch is short
def test_ranks_partition_the_global_batches(world_size, batch_size):
    whole = dl.plan_epoch(COUNTS, SKIP, batch_size * world_size, True, np.random.RandomState(5))
    ranks = [_HostLoader(batch_size, True, np.random.RandomState(5), r, world_size) for r in range(world_size)]
    epochs = [ld.epoch() for ld in ranks]
    assert all(ld.num_itr == len(whole) == -(-TOTAL // (batch_size * world_size)) for ld in ranks)
    assert all(len(e) == len(whole) for e in epochs)                               # the same step count on every rank
    for step, batch in enumerate(whole):
        assert sum((e[step][0] for e in epochs), []) == batch                      # contiguous slices, in rank order, nothing lost
        short = len(batch) != batch_size * world_size
        assert all(e[step][1] == short for e in epochs)                            # a short global batch is short on every rank
    assert [short for _, short in epochs[0]][:-1] == [False] * (len(whole) - 1)
    # the second epoch is planned again, from the same stream on every rank
    again = [ld.epoch() for ld in ranks]
    assert all(len(e) == len(whole) for e in again) and again[0] != epochs[0]
    assert Counter(s for e in again for b, _ in e for s in b) == Counter(s for b in whole for s in b)


def test_iter_skips_short_batches():
    ld = _HostLoader(5, True, np.random.RandomState(1), 0, 1)
    plan = [dl.plan_epoch(COUNTS, SKIP, 5, True, rng) for rng in [np.random.RandomState(1)] for _ in range(2)]
    assert TOTAL % 5 != 0
    for epoch in plan:                                                     # iterating again runs the next epoch
        seen = [[tuple(s) for s in f.tolist()] for f, _, _ in ld]
        assert seen == epoch[:-1]


def _clips(n=(33, 40), hw=((5, 6), (4, 7)), dtype=np.uint8):
    return [np.zeros((k,) + s + (3,), dtype) for k, s in zip(n, hw)]


def test_validation_errors():
    mk = lambda s, u, skip=SKIP: dl.Data_Loader.from_clips(skip, s, u, 6, 10, 2, True)      # noqa: E731
    with pytest.raises(ValueError, match="stab clips"):
        mk(_clips(), _clips()[:1])
    with pytest.raises(ValueError, match="stab frames"):
        mk(_clips(), _clips(n=(33, 41)))
    with pytest.raises(ValueError, match="no candidate offset"):
        mk(_clips(n=(33, 32)), _clips(n=(33, 32)))
    with pytest.raises(ValueError, match="uint8"):
        mk(_clips(dtype=np.float32), _clips(dtype=np.float32))
    with pytest.raises(ValueError, match="uint8"):
        mk(_clips(), [c.astype(np.int16) for c in _clips()])
    with pytest.raises(ValueError, match=r"\[N,h,w,3\]"):
        mk([np.zeros((33, 5, 6, 4), np.uint8)], [np.zeros((33, 5, 6, 4), np.uint8)])
    with pytest.raises(ValueError, match=r"\[N,h,w,3\]"):
        mk([np.zeros((33, 5, 6), np.uint8)], [np.zeros((33, 5, 6), np.uint8)])
    with pytest.raises(ValueError, match="skip_length"):
        mk(_clips(), _clips(), SKIP[:8])
    with pytest.raises(ValueError, match="rank"):
        dl.Data_Loader.from_clips(SKIP, _clips(), _clips(), 6, 10, 2, True, rank=2, world_size=2)


def test_path_constructor_walk_and_decode(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    frames = {}
    # written in an order that is neither the folders' nor the files' sorted order
    for clip in ("b/inner", "a", "c"):
        (tmp_path / clip).mkdir(parents=True)
        for name in ("10.png", "2.png", "1.png"):
            f = rng.integers(0, 256, (3, 4, 3), dtype=np.uint8)
            Image.fromarray(f, "RGB").save(str(tmp_path / clip / name))
            frames[(clip, name)] = f
    folders, files = dl.list_clips(str(tmp_path))
    # leaf directories only ("b" itself is no clip), sorted by path; names sorted as STRINGS within a clip ("1" < "10" < "2")
    assert [f[len(str(tmp_path)) + 1:] for f in folders] == ["a", "b/inner", "c"]
    assert [[p.rsplit("/", 1)[1] for p in clip] for clip in files] == [["1.png", "10.png", "2.png"]] * 3
    for folder, clip in zip(("a", "b/inner", "c"), files):
        got = dl.decode_clip(clip)
        assert got.dtype == np.uint8 and got.shape == (3, 3, 4, 3)
        assert np.array_equal(got, np.stack([frames[(folder, n)] for n in ("1.png", "10.png", "2.png")]))      # PNG decodes exactly, RGB order
    # the constructor pairs the two trees clip by clip and refuses what does not pair
    with pytest.raises(ValueError, match="stab clips"):
        dl.Data_Loader(SKIP, str(tmp_path), str(tmp_path / "a"), 6, 10, 2, True)
    (tmp_path / "c" / "3.png").write_bytes((tmp_path / "c" / "1.png").read_bytes())
    with pytest.raises(ValueError, match="stab frames"):
        dl.Data_Loader(SKIP, str(tmp_path / "a"), str(tmp_path / "c"), 6, 10, 2, True)

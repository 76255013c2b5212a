"""Drop-in for the reference's `data_loader.Data_Loader` (the feeder of train(), main:170-171, 385, 405-407; "main" =
main_flownetS_pyramid_noprevloss_dataloader.py) with the clips resident in HBM as uint8 frames.

The reference builds every batch on the host: per sample nine frames of the stable clip and one of the unstable clip, each
`cv2.resize(cv2.cvtColor(cv2.imread(path), BGR2RGB) / 255., (w, h))` on a float64 image (`_read_frame`, :203-206), concatenated and
fed as 30 fp32 planes per pixel.  Here the frames are decoded once, uploaded once as uint8 and stay on the device; a batch is one
launch per clip present in it (`vstab_assemble_train_batch`, csrc/train_batch_ops.hip) that resizes and lays out the three tensors
`Trainer.step` takes.  train() uses no augmentation (utils.random_crop / random_flip / add_gaussian_noise are never called by it),
so the sampling plan and the read-and-resize are the whole loader.

What is pinned: the kernel equals tests/data_loader_ref.py -- a NumPy float64 restatement of `_read_frame` + `read_dataset` -- bit
for bit, and `plan_epoch` equals a line-for-line restatement of `init_idx` / `get_batch` / `_update_idx` draw for draw.  What is not:
cv2's own 64-bit resize (cv2 is not installed; the restatement follows OpenCV's published generic path, like `resize_u8`) and JPEG
decoding (see `Data_Loader.__init__`)."""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, runtime

SAMPLE_NUM = 9                                   # init_data_loader :28


def candidate_offsets(total_frames: int, skip_length) -> List[int]:
    """A clip's entries of one epoch (`init_idx`, :52-58): every offset whose nine frames fit, then sample_num - 1 = 8 extra zeros --
    offset 0 is drawn up to nine times per epoch.  The reference's quirk, kept."""
    skip = [int(s) for s in skip_length]
    return list(range(0, int(total_frames) - (skip[-1] - skip[0] + 1))) + [0] * (SAMPLE_NUM - 1)


def plan_epoch(frame_counts: Sequence[int], skip_length, batch_size: int, is_train: bool,
               rng: Optional[np.random.RandomState] = None) -> List[List[Tuple[int, int]]]:
    """One epoch of `get_batch` (:64-108) as a pure host function: the list of batches, each a list of (clip, offset).

    Training draws `rng.randint(clips left)` then `rng.randint(entries left in that clip)` per sample, in the reference's order, so a
    `RandomState` in the state of NumPy's global one gives the reference's picks; evaluation always takes the first entry of the first
    clip left.  A drawn entry is deleted, a clip leaves when its list is empty, a batch ends early when no clip is left (the last batch
    may be short; train() skips it, main:407)."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    if rng is None:
        rng = np.random.RandomState()
    entries = [candidate_offsets(n, skip_length) for n in frame_counts]
    clips = list(range(len(entries)))
    batches = []
    while clips:
        batch = []
        while clips and len(batch) < batch_size:
            x = int(rng.randint(len(clips))) if is_train else 0
            clip = clips[x]
            y = int(rng.randint(len(entries[clip]))) if is_train else 0
            batch.append((clip, entries[clip].pop(y)))
            if not entries[clip]:
                clips.pop(x)
        batches.append(batch)
    return batches


def list_clips(root_path: str) -> Tuple[List[str], List[List[str]]]:
    """`_load_file_list` (:182-201): every leaf directory under `root_path` is a clip; file names sorted within a clip, clips sorted by
    folder path.  Returns (folder paths, per-clip file paths)."""
    found = []
    for root, dirnames, filenames in os.walk(root_path):
        if len(dirnames) == 0:
            found.append((root, sorted(os.path.join(root, f) for f in filenames)))
    found.sort(key=lambda e: e[0])
    return [e[0] for e in found], [e[1] for e in found]


def decode_clip(paths: Sequence[str]) -> np.ndarray:
    """The frames of one clip as uint8 [N,h,w,3] RGB (`cvtColor(imread(path, IMREAD_COLOR), BGR2RGB)`), decoded with Pillow."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("Data_Loader(stab_path, unstab_path) decodes image files with Pillow, which cannot be imported; install it, or "
                          "decode the frames yourself and use Data_Loader.from_clips(...)") from e
    frames = []
    for p in paths:
        with Image.open(p) as im:
            frames.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
    if any(f.shape != frames[0].shape for f in frames):
        raise ValueError(f"the frames of clip {os.path.dirname(paths[0])} differ in size")
    return np.stack(frames)


def _check_clips(stab_clips, unstab_clips, skip):
    """The ValueErrors of the constructors; returns the frame counts."""
    if len(skip) != SAMPLE_NUM:
        raise ValueError(f"skip_length must have {SAMPLE_NUM} entries (eight history frames and the target), got {len(skip)}")
    if min(skip) < 0 or skip[0] > 1:
        raise ValueError("skip_length must be non-negative and start at 0 or 1: the last candidate offset reads frame N + skip_length[0] - 2")
    if len(stab_clips) != len(unstab_clips):
        raise ValueError(f"{len(stab_clips)} stab clips but {len(unstab_clips)} unstab clips")
    if len(stab_clips) == 0:
        raise ValueError("no clips")
    counts = []
    for i, (s, u) in enumerate(zip(stab_clips, unstab_clips)):
        for name, c in (("stab", s), ("unstab", u)):
            if c.dtype != (torch.uint8 if torch.is_tensor(c) else np.uint8):
                raise ValueError(f"{name} clip {i}: dtype {c.dtype}, expected uint8")
            if len(c.shape) != 4 or c.shape[3] != 3:
                raise ValueError(f"{name} clip {i}: shape {tuple(c.shape)}, expected [N,h,w,3]")
        if s.shape[0] != u.shape[0]:
            raise ValueError(f"clip {i}: {s.shape[0]} stab frames but {u.shape[0]} unstab frames")
        if tuple(s.shape[1:]) != tuple(u.shape[1:]):
            raise ValueError(f"clip {i}: stab frames are {tuple(s.shape[1:3])} but unstab frames {tuple(u.shape[1:3])}; one launch reads both pools "
                             "at one source size")
        n = int(s.shape[0])
        if n - (skip[-1] - skip[0] + 1) <= 0:
            raise ValueError(f"clip {i}: {n} frames leave no candidate offset for skip_length {skip} (needs more than {skip[-1] - skip[0] + 1})")
        counts.append(n)
    return counts


class Data_Loader:
    def __init__(self, skip_length, stab_path, unstab_path, height, width, batch_size, is_train, thread_num=3, *, device=None, rng=None,
                 rank=0, world_size=1):
        """The reference's constructor (main:170-171): walks `stab_path` and `unstab_path` as `_load_file_list` does (clip i of one pairs
        with clip i of the other, frame by frame), decodes every frame once with Pillow and keeps the clips on the device as uint8.

        PNG (and any lossless format) decodes exactly, so the frames are the bytes `cv2.imread` yields.  JPEG bytes depend on the decoder
        (IDCT and chroma upsampling differ between libjpeg builds, and between Pillow's and OpenCV's): they are NOT claimed equal to
        `cv2.imread`'s.  Raises ImportError if Pillow cannot be imported.

        `thread_num` is accepted and unused: nothing is read or resized on the host after construction.  `rng`: the
        `np.random.RandomState` the epoch plans draw from (default: a fresh one).  `rank` / `world_size`: data parallelism, see
        `init_data_loader`."""
        _, stab_files = list_clips(stab_path)
        _, unstab_files = list_clips(unstab_path)
        if len(stab_files) != len(unstab_files):
            raise ValueError(f"{len(stab_files)} stab clips under {stab_path} but {len(unstab_files)} unstab clips under {unstab_path}")
        for i, (s, u) in enumerate(zip(stab_files, unstab_files)):
            if len(s) != len(u):
                raise ValueError(f"clip {i}: {len(s)} stab frames but {len(u)} unstab frames")
        self._setup(skip_length, [decode_clip(f) for f in stab_files], [decode_clip(f) for f in unstab_files], height, width, batch_size, is_train,
                    thread_num, device, rng, rank, world_size)

    @classmethod
    def from_clips(cls, skip_length, stab_clips, unstab_clips, height, width, batch_size, is_train, thread_num=3, *, device=None, rng=None,
                   rank=0, world_size=1):
        """The same loader over frames already decoded: lists of uint8 [N_i, h_i, w_i, 3] RGB tensors or arrays (clips may differ in
        size), uploaded once."""
        self = cls.__new__(cls)
        self._setup(skip_length, list(stab_clips), list(unstab_clips), height, width, batch_size, is_train, thread_num, device, rng, rank, world_size)
        return self

    def _setup(self, skip_length, stab_clips, unstab_clips, height, width, batch_size, is_train, thread_num, device, rng, rank, world_size):
        self.skip_length = np.array(skip_length)
        skip = [int(s) for s in self.skip_length.reshape(-1)]
        self.h, self.w, self.batch_size = int(height), int(width), int(batch_size)
        self.is_train, self.thread_num, self.num_partition = is_train, thread_num, 1
        self.rank, self.world_size = int(rank), int(world_size)
        if self.h < 1 or self.w < 1 or self.batch_size < 1:
            raise ValueError("height, width and batch_size must be >= 1")
        if self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError(f"rank {rank} is outside [0, world_size = {world_size})")
        stab_clips, unstab_clips = ([c if torch.is_tensor(c) else np.asarray(c) for c in cl] for cl in (stab_clips, unstab_clips))
        self.frame_counts = _check_clips(stab_clips, unstab_clips, skip)
        self.num_files = int(sum(self.frame_counts))
        self.rng = rng if rng is not None else np.random.RandomState()
        runtime._require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        up = lambda c: torch.as_tensor(c).to(self.device).contiguous()        # noqa: E731
        self.stab_clips, self.unstab_clips = [up(c) for c in stab_clips], [up(c) for c in unstab_clips]
        # two sets of outputs, allocated once: the batch handed out stays valid while the next one is assembled
        B = self.batch_size
        self._buffers = [tuple(torch.empty((B, self.h, self.w, c), dtype=torch.float32, device=self.device) for c in (27, 3, 3)) for _ in range(2)]
        self._turn = 0
        self._skip_i32 = np.asarray(skip, dtype=np.int32)
        self._plan = None
        self.is_end = False
        self.last_samples: List[Tuple[int, int]] = []

    def init_data_loader(self, inputs=None):
        """Draws the epoch's plan (`init_idx` + the draws of `get_batch`).  `inputs` (the reference's dict of placeholders) is accepted
        and unused: the feed's names are fixed.

        Data parallelism: every rank plans the SAME epoch from an `rng` in the same state, with batch_size * world_size draws per step,
        and takes the contiguous slice [rank * batch_size, (rank + 1) * batch_size) of each global batch -- the epoch stays without
        replacement across ranks and every rank sees the same number of steps (Trainer.step's all-reduce needs that).  A global batch
        that is not full is reported short on every rank."""
        self.sample_num = SAMPLE_NUM
        self._plan = plan_epoch(self.frame_counts, self._skip_i32, self.batch_size * self.world_size, self.is_train, self.rng)
        self._pos = 0
        self.num_itr = len(self._plan)           # == ceil(entries / (batch_size * world_size)), :34
        self.is_end = False

    def _assemble(self, samples):
        """The samples [(clip, offset)] into rows 0.. of the next buffer set: one launch sequence per clip present."""
        feats, gtstab, unstab = self._buffers[self._turn]
        self._turn ^= 1
        by_clip = collections.OrderedDict()
        for row, (clip, _) in enumerate(samples):
            by_clip.setdefault(clip, []).append(row)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for clip, rows in by_clip.items():
                s, u = self.stab_clips[clip], self.unstab_clips[clip]
                r = np.asarray(rows, dtype=np.int32)
                fi = np.ascontiguousarray(np.asarray([samples[k][1] for k in rows], dtype=np.int32)[:, None] + self._skip_i32[None, :])
                _lib.check(L.vstab_assemble_train_batch(s.data_ptr(), u.data_ptr(), s.shape[0], s.shape[1], s.shape[2],
                                                        r.ctypes.data_as(_lib.c_int32_p), fi.ctypes.data_as(_lib.c_int32_p), len(rows),
                                                        feats.data_ptr(), gtstab.data_ptr(), unstab.data_ptr(), self.batch_size, self.h, self.w,
                                                        runtime.stream_ptr()))
        n = len(samples)
        return feats[:n], gtstab[:n], unstab[:n]

    def feed_the_network(self):
        """(feed, is_end, is_not_batchsize) as the reference's (:240-255).  `feed` is an ordered dict of CUDA tensors under the
        reference's placeholder names -- 'unstab_image' [n,h,w,3], 'gtstab_image' [n,h,w,3], 'stab_image' [n,h,w,24] -- plus 'feats'
        [n,h,w,27] = concat([stab_image, unstab_image], 3) (main:184), of which 'stab_image' is the [..., :24] view.  The first request
        after the last batch returns (None, True, False) and draws the next epoch's plan."""
        if self._plan is None:
            self.init_data_loader()
        if self._pos == len(self._plan):
            self.init_data_loader()
            return None, True, False
        whole = self._plan[self._pos]
        self._pos += 1
        self.last_samples = whole[self.rank * self.batch_size:(self.rank + 1) * self.batch_size]
        is_not_batchsize = len(whole) != self.batch_size * self.world_size
        feats, gtstab, unstab = self._assemble(self.last_samples)
        feed = collections.OrderedDict()
        feed['unstab_image'] = unstab
        feed['gtstab_image'] = gtstab
        feed['stab_image'] = feats[..., :24]
        feed['feats'] = feats
        return feed, False, is_not_batchsize

    def __iter__(self):
        """One epoch of main:405-407 as (feats, gtstab, unstab) batches, short batches skipped: `trainer.train_epoch(loader, epoch)`."""
        while True:
            feed, is_end, is_not_batchsize = self.feed_the_network()
            if is_end:
                return
            if is_not_batchsize:
                continue
            yield feed['feats'], feed['gtstab_image'], feed['unstab_image']

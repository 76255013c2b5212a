"""Restatements the data loader is held to (not a test module).

1. `read_frame` / `read_dataset`: the reference's `_read_frame` (data_loader.py:203-206) and `read_dataset` (:132-169) in NumPy
   float64.  cv2 is not installed, so `cv2.resize` on the float64 image is restated from OpenCV's published generic linear path
   (imgproc/resize.cpp), as oracle.vstab_oracle.cv_resize_u8 / cv_resize_f32 are: UNPINNED against cv2 itself, pinned by
   tests/test_data_loader_ref_cpu.py.
2. `RefPlan`: the reference's epoch plan (`init_idx` :49-62, `get_batch` :64-108, `_update_idx` :173-178) line for line on Python
   lists.  It shares no code with data_loader.plan_epoch."""
import numpy as np


def _taps(dn, sn):
    """Taps and FLOAT32 coefficients of one axis (the ones cv_resize_f32's taps() computes)."""
    scale = np.float64(1.0) / (np.float64(dn) / np.float64(sn))
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)      # fx = (float)((dx+0.5)*scale - 0.5)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    f[lo] = 0; s[lo] = 0
    hi = s >= sn - 1
    f[hi] = 0; s[hi] = sn - 1
    return s, np.minimum(s + 1, sn - 1), (np.float32(1) - f).astype(np.float32), f


def resize_f64(img, dh, dw):
    """cv2.resize(img, (dw, dh)), INTER_LINEAR, on a float64 HxWxC image: float32 coefficients widened to double, both passes in double,
    every operation one IEEE multiply or add (NumPy never fuses them); dsize == ssize copies."""
    img = np.asarray(img, dtype=np.float64)
    sh, sw = img.shape[:2]
    if (dh, dw) == (sh, sw):
        return img.copy()
    x0, x1, ax0, ax1 = _taps(dw, sw)
    y0, y1, ay0, ay1 = _taps(dh, sh)
    ax0, ax1, ay0, ay1 = (a.astype(np.float64) for a in (ax0, ax1, ay0, ay1))
    R = img[:, x0] * ax0[None, :, None] + img[:, x1] * ax1[None, :, None]
    return ay0[:, None, None] * R[y0] + ay1[:, None, None] * R[y1]


def read_frame(rgb_u8, h, w):
    """_read_frame on a decoded RGB frame: `/ 255.` (float64), cv2.resize to (w, h)."""
    return resize_f64(np.asarray(rgb_u8, dtype=np.uint8) / 255., h, w)


def read_dataset(stab_clip, unstab_clip, offset, skip_length, h, w):
    """One sample as the float32 placeholders receive it (main:179-184): (feats [h,w,27], gtstab [h,w,3], unstab [h,w,3])."""
    idx = offset + np.asarray(skip_length)
    stab_image = np.concatenate([read_frame(stab_clip[i], h, w) for i in idx[:-1]], axis=2)
    gtstab = read_frame(stab_clip[idx[-1]], h, w)
    unstab = read_frame(unstab_clip[idx[-1]], h, w)
    return (np.concatenate([stab_image, unstab], axis=2).astype(np.float32), gtstab.astype(np.float32), unstab.astype(np.float32))


def read_batch(stab_clips, unstab_clips, samples, skip_length, h, w):
    """The samples [(clip, offset)] stacked: (feats [n,h,w,27], gtstab, unstab [n,h,w,3])."""
    parts = [read_dataset(stab_clips[c], unstab_clips[c], o, skip_length, h, w) for c, o in samples]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


class RefPlan:
    """The reference's bookkeeping restated step by step on Python lists: `left[v]` is clip v's list of offsets not drawn yet,
    `alive` the clips whose list is not empty.  Each step below names the statement of data_loader.py it restates."""

    def __init__(self, frame_counts, skip_length, batch_size, is_train, rng):
        self.counts, self.skip = [int(n) for n in frame_counts], [int(s) for s in skip_length]
        self.batch_size, self.is_train, self.rng = int(batch_size), bool(is_train), rng
        self.rebuild()
        self.num_itr = int(np.ceil(sum(len(l) for l in self.left) / self.batch_size))           # :34

    def rebuild(self):
        span = self.skip[-1] - self.skip[0] + 1
        self.left, self.alive = [], []
        for v, total in enumerate(self.counts):                                                  # :52
            offsets = [o for o in range(total - span)]                                           # :56 (num_partition = 1)
            offsets += [0 for _ in range(9 - 1)]                                                 # :57-58, sample_num = 9
            self.left.append(offsets)
            self.alive.append(v)                                                                 # :60
        self.ended = False                                                                       # :62

    def next_batch(self):
        """One batch as [(clip, offset)], or None: the request that finds nothing left ends the epoch (:82-86)."""
        if self.ended:                                                                           # :72
            return None
        picked = []
        for k in range(self.batch_size):                                                         # :81
            if not self.alive:
                if k == 0:                                                                       # :82-86
                    self.ended = True
                    return None
                break                                                                            # :87-88: a short batch
            if self.is_train:
                x = self.rng.randint(len(self.alive))                                            # :92
                y = self.rng.randint(len(self.left[self.alive[x]]))                              # :94
            else:
                x, y = 0, 0                                                                      # :96-97
            v = self.alive[x]
            picked.append((int(v), int(self.left[v][y])))                                        # :100-102
            del self.left[v][y]                                                                  # :175
            if len(self.left[v]) == 0:                                                           # :177-178
                del self.alive[x]
        return picked

    def epoch(self):
        """Every batch up to the end of the epoch; the lists are rebuilt afterwards (`_init_data_thread`, :231, 272-274)."""
        out = []
        while True:
            b = self.next_batch()
            if b is None:
                self.rebuild()
                return out
            out.append(b)

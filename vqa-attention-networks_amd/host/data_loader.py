"""Device-side half of the reference's input pipeline.

`VqaDataset.__getitem__` (data_loader.py:27-33) loads one `[2048, 14, 14]` .npy per image and
transposes it to `(196, 2048)` on the CPU; `DataLoader` collates a batch and `solver.py:77,84`
sends it with a blocking `.to(device)`.  At batch 512 that is 822 MB per step.

`FeatureStager` replaces the transpose + copy:

* the loader writes each image's array *as stored* (channels outermost) into a pinned host slot
  (`host_slot()` hands out the numpy view, so `np.load`-ed data is copied once);
* `commit()` issues the host-to-device copy on a dedicated copy stream and the layout change
  (`vqf_feat_transpose`, optionally narrowing to bf16) right behind it on the same stream;
* `next()` makes the compute stream wait for that slot's event and returns the `(N, 196, 2048)`
  tensor the modules consume.  With `depth` >= 2 slots the copy of batch k+1 overlaps the
  training step of batch k (822 MB over PCIe Gen5 is ~15 ms, a third of an fp32 step).

Dataset indexing, question/answer encoding and GloVe lookup stay with the reference's loader; this
class only owns the image-feature path, which is the part that touches the GPU.
"""
import collections

import numpy as np
import torch

from . import ops
from .lib import VqfError
from .grouping import PackedRegions


class FeatureStager:
    def __init__(self, batch_size, channels=2048, regions=196, device=None, bf16=False, depth=2):
        if not torch.cuda.is_available():
            raise VqfError("FeatureStager needs a GPU (no CPU fallback)")
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.N, self.D, self.L = int(batch_size), int(channels), int(regions)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.bf16 = bool(bf16)
        self.copy_stream = torch.cuda.Stream(self.device)
        self._slots = []
        for _ in range(depth):
            self._slots.append(dict(
                host=torch.empty((self.N, self.D, self.L), dtype=torch.float32).pin_memory(),
                raw=torch.empty((self.N, self.D, self.L), dtype=torch.float32, device=self.device),
                ready=torch.cuda.Event(), used=False))
        self._free = collections.deque(range(depth))
        self._inflight = collections.deque()
        self._filling = None

    # -- producer side --------------------------------------------------------
    def host_slot(self):
        """numpy view (N, D, L) of the next free pinned slot; fill rows [0, n) then commit(n)."""
        if self._filling is None:
            if not self._free:
                raise VqfError("FeatureStager: all %d slots are in flight; call next() first" % len(self._slots))
            self._filling = self._free.popleft()
            sl = self._slots[self._filling]
            if sl["used"]:                 # the previous H2D copy out of this pinned buffer must have finished
                sl["ready"].synchronize()
        return self._slots[self._filling]["host"].numpy()

    def commit(self, rows=None):
        """Queue H2D copy + transpose of the slot handed out by host_slot()."""
        if self._filling is None:
            raise VqfError("FeatureStager.commit() without host_slot()")
        i, self._filling = self._filling, None
        sl = self._slots[i]
        n = self.N if rows is None else int(rows)
        if not 0 < n <= self.N:
            raise ValueError("rows must be in 1..%d" % self.N)
        sl["used"] = True
        with torch.cuda.stream(self.copy_stream):   # stream order protects `raw` (copy k+1 follows transpose k)
            sl["raw"][:n].copy_(sl["host"][:n], non_blocking=True)
            sl["out"] = ops.feat_transpose(sl["raw"][:n], bf16=self.bf16)
            sl["ready"].record(self.copy_stream)
        self._inflight.append(i)

    def submit(self, batch):
        """Convenience: batch = array-like (n, D, L) or (n, D, 14, 14), or a list of per-image arrays."""
        host = self.host_slot()
        if isinstance(batch, (list, tuple)):
            n = len(batch)
            for k, a in enumerate(batch):
                host[k] = np.asarray(a, dtype=np.float32).reshape(self.D, self.L)
        else:
            b = np.asarray(batch, dtype=np.float32)
            n = b.shape[0]
            host[:n] = b.reshape(n, self.D, self.L)
        self.commit(n)

    # -- consumer side --------------------------------------------------------
    def next(self):
        """-> (n, L, D) device tensor of the oldest committed batch; the current stream is made to
        wait for its copy + transpose.  The tensor is a fresh allocation owned by the caller; the
        slot's pinned / raw buffers go back to the free list."""
        if not self._inflight:
            raise VqfError("FeatureStager.next(): nothing committed")
        i = self._inflight.popleft()
        sl = self._slots[i]
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(sl["ready"])
        out = sl.pop("out")
        out.record_stream(cur)           # allocated on the copy stream, consumed on this one
        self._free.append(i)
        return out


def stage_features(batch, bf16=False, device=None):
    """One-shot form: (n, D, L) / (n, D, 14, 14) host array -> (n, L, D) device tensor."""
    b = np.asarray(batch, dtype=np.float32)
    n, D = b.shape[0], b.shape[1]
    st = FeatureStager(n, channels=D, regions=int(np.prod(b.shape[2:])), device=device, bf16=bf16, depth=1)
    st.submit(b)
    return st.next()


def group_batch(image_ids):
    """The host half of a shared-image batch (forward(..., img_index)): image_ids = the batch's image ids as the loader has
    them, one per question (any hashable) -> (rows (U,), img_index (N,)), both int64 CPU tensors.  rows[u] is the position in
    the batch of the FIRST question about the u-th distinct image, in order of appearance; question n looks at image
    img_index[n] of [features[r] for r in rows] -- the only features the loader then has to stage (FeatureStager.submit)."""
    ids = list(image_ids)
    if not ids:
        raise ValueError("group_batch: an empty batch")
    seen, rows, index = {}, [], []
    for n, key in enumerate(ids):
        u = seen.get(key)
        if u is None:
            u = seen[key] = len(rows)
            rows.append(n)
        index.append(u)
    return torch.tensor(rows, dtype=torch.int64), torch.tensor(index, dtype=torch.int64)


def _region_arrays(name, features, multiple):
    """The input checks pad_region_features and pack_region_features share -> (float32 (K_i, D) arrays, D, Lmax)."""
    arrs = [np.asarray(a, dtype=np.float32) for a in features]
    if not arrs:
        raise ValueError(name + ": an empty list")
    if int(multiple) < 1:
        raise ValueError(name + ": multiple must be >= 1")
    if any(a.ndim != 2 or a.shape[0] < 1 for a in arrs):
        raise ValueError(name + ": every entry must be a (K_i, D) array with K_i >= 1")
    D = arrs[0].shape[1]
    if any(a.shape[1] != D for a in arrs):
        raise ValueError(name + ": mixed channel counts %s" % sorted({a.shape[1] for a in arrs}))
    m = int(multiple)
    return arrs, D, (max(a.shape[0] for a in arrs) + m - 1) // m * m


def pad_region_features(features, multiple=1):
    """The host half of a region-count batch (forward((img, img_length), ...)): features = one (K_i, D) array per image (detector
    boxes, K_i >= 1, the same D) -> (img (N, Lmax, D) float32, zero-padded on the right, img_length (N,) int64), both CPU
    tensors.  Lmax is the largest K_i rounded up to a multiple of `multiple`."""
    arrs, D, Lmax = _region_arrays("pad_region_features", features, multiple)
    img = torch.zeros((len(arrs), Lmax, D), dtype=torch.float32)
    for n, a in enumerate(arrs):
        img[n, :a.shape[0]] = torch.from_numpy(np.ascontiguousarray(a))
    return img, torch.tensor([a.shape[0] for a in arrs], dtype=torch.int64)


def pack_region_features(features, multiple=1):
    """The host half of a packed batch (forward(PackedRegions, ...)): the same input and the same checks as pad_region_features
    -> a CPU PackedRegions whose rows (sum K_i, D) float32 are the images' regions one after the other, never padded, with
    offsets (N + 1,) int64 and max_regions = the largest K_i rounded up to a multiple of `multiple`.  Its .unpack() equals
    pad_region_features(features, multiple); .to(device) moves it."""
    arrs, D, Lmax = _region_arrays("pack_region_features", features, multiple)
    offsets = torch.zeros(len(arrs) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor([a.shape[0] for a in arrs], dtype=torch.int64), 0)
    rows = torch.from_numpy(np.ascontiguousarray(np.concatenate(arrs, 0)))
    return PackedRegions(rows, offsets, Lmax)

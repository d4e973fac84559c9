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

`RegionStager` is the same pipeline for detector-box features that are never padded (the packed call
forms of MFB, MHBCoAtt and HieCoAttenLadder): the pinned slot holds the real rows of every image one
after the other, as fp32 or fp16, exactly `sum K_i` rows cross PCIe, and `vqf_region_rows_stage`
widens them (or places them into the zero-padded pair) on the copy stream.

Dataset indexing, question/answer encoding and GloVe lookup stay with the reference's loader; these
classes only own the image-feature path, which is the part that touches the GPU.
"""
import collections

import numpy as np
import torch

from . import ops
from .lib import VqfError
from .grouping import PackedRegions, SoftAnswers, SOFT_MAX_SLOTS


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


def soft_answers(answer_dicts, slots=10):
    """The host half of a soft-answer batch (BCEWithLogitsLoss(logits, SoftAnswers)): answer_dicts = one {answer_id: score} dict
    per question, the `answers` entry the reference's loader reads (data_loader.py:40-42; keys str or int, as there) -> a CPU
    SoftAnswers with ids (N, slots) int64 and scores (N, slots) float32, each dict's entries in its own order, unused slots
    id -1 / score 0.  An empty list, a dict with more than `slots` entries or slots outside 1..16: ValueError."""
    if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= SOFT_MAX_SLOTS:
        raise ValueError("soft_answers: slots must be an int in [1, %d], got %r" % (SOFT_MAX_SLOTS, slots))
    dicts = list(answer_dicts)
    if not dicts:
        raise ValueError("soft_answers: an empty list")
    ids = np.full((len(dicts), slots), -1, dtype=np.int64)
    scores = np.zeros((len(dicts), slots), dtype=np.float32)
    for n, d in enumerate(dicts):
        if len(d) > slots:
            raise ValueError("soft_answers: question %d has %d answers, more than the %d slots" % (n, len(d), slots))
        for k, (a, v) in enumerate(d.items()):
            ids[n, k] = int(a)
            scores[n, k] = v
    return SoftAnswers(torch.from_numpy(ids), torch.from_numpy(scores))


def _region_shapes(name, features):
    """The checks of _region_arrays without its fp32 copies -> (arrays as given, D, largest K_i, sum K_i)."""
    arrs = [np.asarray(a) for a in features]
    if not arrs:
        raise ValueError(name + ": an empty list")
    if any(a.ndim != 2 or a.shape[0] < 1 for a in arrs):
        raise ValueError(name + ": every entry must be a (K_i, D) array with K_i >= 1")
    D = arrs[0].shape[1]
    if any(a.shape[1] != D for a in arrs):
        raise ValueError(name + ": mixed channel counts %s" % sorted({a.shape[1] for a in arrs}))
    return arrs, D, max(a.shape[0] for a in arrs), sum(a.shape[0] for a in arrs)


def pack_into(rows, counts, features, max_regions=None):
    """The host-side filling of a RegionStager slot, on plain numpy buffers (no GPU): features = one (K_i, D) array per image ->
    rows[:sum K_i] holds image u's regions behind those of image u - 1, cast to rows' dtype (float32 or float16, round to nearest
    even), counts[u] = K_u; returns the number of images.  The input checks are pack_region_features' (an empty list, K_i = 0, mixed
    D), plus what the buffers hold: D == rows.shape[1], K_i <= max_regions when given, sum K_i <= rows.shape[0], images <=
    counts.shape[0].  Nothing is written when a check refuses."""
    arrs, D, kmax, total = _region_shapes("pack_into", features)
    if rows.ndim != 2 or D != rows.shape[1]:
        raise ValueError("pack_into: the features have %d channels, the row buffer %s" % (D, rows.shape[1:]))
    if max_regions is not None and kmax > int(max_regions):
        raise ValueError("pack_into: an image with %d regions, max_regions is %d" % (kmax, int(max_regions)))
    if total > rows.shape[0]:
        raise ValueError("pack_into: %d rows in all, the row buffer holds %d" % (total, rows.shape[0]))
    if len(arrs) > counts.shape[0]:
        raise ValueError("pack_into: %d images, the counts buffer holds %d" % (len(arrs), counts.shape[0]))
    r = 0
    for u, a in enumerate(arrs):
        k = a.shape[0]
        rows[r:r + k] = a
        counts[u] = k
        r += k
    return len(arrs)


class RegionStager:
    """Pinned, double-buffered staging of packed region features.  Producer: host_slot() -> (rows, counts) numpy views of a free
    pinned slot, fill them (pack_into), commit(images, img_index=None); or submit(features, image_ids=None).  Consumer: next() ->
    (features, img_index) of the oldest committed batch, features a PackedRegions (form "packed") or the pair (img, img_length)
    (form "padded"), both fp32 with int32 offsets / counts, whatever `storage` (the dtype that crosses PCIe) is."""

    def __init__(self, max_images, channels=2048, max_regions=100, max_rows=None, max_questions=None, device=None,
                 storage="fp32", form="packed", depth=2):
        if storage not in ("fp32", "fp16"):
            raise ValueError("storage must be 'fp32' or 'fp16', got %r" % (storage,))
        if form not in ("packed", "padded"):
            raise ValueError("form must be 'packed' or 'padded', got %r" % (form,))
        if depth < 1:
            raise ValueError("depth must be >= 1")
        if not 1 <= int(max_regions) <= 1024:
            raise ValueError("max_regions must be in 1..1024")
        if int(max_images) < 1 or int(channels) < 1:
            raise ValueError("max_images and channels must be >= 1")
        self.U, self.D, self.L = int(max_images), int(channels), int(max_regions)
        self.R = self.U * self.L if max_rows is None else int(max_rows)
        self.Q = self.U if max_questions is None else int(max_questions)
        if self.R < 1 or self.Q < 1:
            raise ValueError("max_rows and max_questions must be >= 1")
        if not torch.cuda.is_available():
            raise VqfError("RegionStager needs a GPU (no CPU fallback)")
        self.storage, self.form = storage, form
        self._kernel = form == "padded" or storage == "fp16"
        if self._kernel and not ops.region_rows_stage_supported(self.U if form == "padded" else 1, self.R, self.L, self.D):
            raise VqfError("RegionStager: vqf_region_rows_stage takes up to 65535 images, fewer than 2^29 rows and channels %% 4 == 0, "
                           "4 <= channels <= 65536 (got max_images=%d, max_rows=%d, channels=%d)" % (self.U, self.R, self.D))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dt = torch.float16 if storage == "fp16" else torch.float32
        self.copy_stream = torch.cuda.Stream(self.device)
        self._slots = []
        for _ in range(depth):
            self._slots.append(dict(
                host=torch.empty((self.R, self.D), dtype=dt).pin_memory(),
                counts=torch.zeros(self.U, dtype=torch.int32),
                offsets=torch.zeros(self.U + 1, dtype=torch.int32).pin_memory(),
                index=torch.zeros(self.Q, dtype=torch.int64).pin_memory(),
                raw=torch.empty((self.R, self.D), dtype=dt, device=self.device) if self._kernel else None,
                ready=torch.cuda.Event(), used=False))
        self._free = collections.deque(range(depth))
        self._inflight = collections.deque()
        self._filling = None

    # -- producer side --------------------------------------------------------
    def host_slot(self):
        """(rows (max_rows, D) in the storage dtype, counts (max_images,) int32): numpy views of the next free slot.  Write image
        u's K_u regions behind those of image u - 1, set counts[u] = K_u, then commit(images)."""
        if self._filling is None:
            if not self._free:
                raise VqfError("RegionStager: all %d slots are in flight; call next() first" % len(self._slots))
            self._filling = self._free.popleft()
            sl = self._slots[self._filling]
            if sl["used"]:                 # the previous H2D copies out of this slot's pinned buffers must have finished
                sl["ready"].synchronize()
        sl = self._slots[self._filling]
        return sl["host"].numpy(), sl["counts"].numpy()

    def _release(self):
        """A refused commit / submit: the slot goes back to the FRONT of the free list, nothing was queued."""
        self._free.appendleft(self._filling)
        self._filling = None

    def commit(self, images, img_index=None):
        """Queue the H2D copies of the slot handed out by host_slot() -- exactly sum(counts[:images]) rows, images + 1 offsets and
        the (N,) img_index when given -- and the kernel the form needs behind them.  Everything is checked on the host first; a
        refusal (ValueError) frees the slot."""
        if self._filling is None:
            raise VqfError("RegionStager.commit() without host_slot()")
        sl = self._slots[self._filling]
        try:
            n = int(images)
            if not 1 <= n <= self.U:
                raise ValueError("images must be in 1..%d" % self.U)
            counts = sl["counts"].numpy()[:n]
            if counts.min() < 1 or counts.max() > self.L:
                raise ValueError("every region count must be in 1..%d (got %d..%d)" % (self.L, counts.min(), counts.max()))
            R = int(counts.sum(dtype=np.int64))
            if R > self.R:
                raise ValueError("%d rows in all, max_rows is %d" % (R, self.R))
            nq = 0
            if img_index is not None:
                idx = np.asarray(img_index.numpy() if torch.is_tensor(img_index) else img_index)
                if idx.ndim != 1 or not 1 <= idx.shape[0] <= self.Q or idx.dtype.kind not in "iu":
                    raise ValueError("img_index must be (N,) integers with 1 <= N <= max_questions = %d" % self.Q)
                if idx.min() < 0 or idx.max() >= n:
                    raise ValueError("img_index must lie in 0..%d" % (n - 1))
                nq = idx.shape[0]
        except ValueError:
            self._release()
            raise
        i, self._filling = self._filling, None
        off = sl["offsets"].numpy()
        off[0] = 0
        np.cumsum(counts, out=off[1:n + 1])
        if nq:
            sl["index"].numpy()[:nq] = idx
        sl["used"] = True
        with torch.cuda.stream(self.copy_stream):   # stream order protects `raw` (copy k+1 follows the kernel of k)
            doff = torch.empty(n + 1, dtype=torch.int32, device=self.device)
            doff.copy_(sl["offsets"][:n + 1], non_blocking=True)
            didx = None
            if nq:
                didx = torch.empty(nq, dtype=torch.int64, device=self.device)
                didx.copy_(sl["index"][:nq], non_blocking=True)
            if self._kernel:
                src = sl["raw"][:R]
                src.copy_(sl["host"][:R], non_blocking=True)
                if self.form == "padded":
                    out = (ops.region_rows_stage(src, doff, self.L), doff[1:] - doff[:-1])
                else:
                    out = (ops.region_rows_stage(src), doff)
            else:                                   # packed fp32: the copy lands in the result
                rows = torch.empty((R, self.D), dtype=torch.float32, device=self.device)
                rows.copy_(sl["host"][:R], non_blocking=True)
                out = (rows, doff)
            sl["out"] = out + (didx,)
            sl["ready"].record(self.copy_stream)
        self._inflight.append(i)

    def submit(self, features, image_ids=None):
        """Convenience: features = a list of (K_i, D) arrays, one per image; with image_ids (one hashable per entry) one per
        QUESTION: group_batch picks the first occurrence of each distinct image, only those are staged, and its img_index travels
        with the batch."""
        feats, index = list(features), None
        if image_ids is not None:
            ids = list(image_ids)
            if len(ids) != len(feats):
                raise ValueError("submit: %d features for %d image_ids" % (len(feats), len(ids)))
            first, index = group_batch(ids)
            feats = [feats[r] for r in first.tolist()]
        rows, counts = self.host_slot()
        try:
            n = pack_into(rows, counts, feats, self.L)
        except ValueError:
            self._release()
            raise
        self.commit(n, index)

    # -- consumer side --------------------------------------------------------
    def next(self):
        """-> (features, img_index) of the oldest committed batch: PackedRegions(rows (R, D) fp32, offsets (images + 1,) int32,
        max_regions = the stager's) or (img (images, max_regions, D) fp32, img_length (images,) int32); img_index (N,) int64 on
        the device or None.  The current stream is made to wait for the slot's copies and kernel; the tensors are fresh allocations
        owned by the caller, the slot's buffers go back to the free list.  No host synchronisation, no device tensor read."""
        if not self._inflight:
            raise VqfError("RegionStager.next(): nothing committed")
        i = self._inflight.popleft()
        sl = self._slots[i]
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(sl["ready"])
        a, b, didx = sl.pop("out")
        for t in (a, b, didx):
            if t is not None:
                t.record_stream(cur)     # allocated on the copy stream, consumed on this one
        self._free.append(i)
        return (PackedRegions(a, b, self.L) if self.form == "packed" else (a, b)), didx


def stage_regions(features, image_ids=None, storage="fp32", form="packed", device=None):
    """One-shot form, the packed counterpart of stage_features: a list of (K_i, D) host arrays (one per image, or one per question
    with image_ids) -> RegionStager.next()'s (features, img_index), max_regions = the largest K_i."""
    feats, ids = list(features), None if image_ids is None else list(image_ids)
    if ids is not None and len(ids) != len(feats):
        raise ValueError("stage_regions: %d features for %d image_ids" % (len(feats), len(ids)))
    shown = feats if ids is None else [feats[r] for r in group_batch(ids)[0].tolist()]
    _, D, kmax, total = _region_shapes("stage_regions", shown)
    st = RegionStager(len(shown), channels=D, max_regions=kmax, max_rows=total, max_questions=len(feats), device=device,
                      storage=storage, form=form, depth=1)
    st.submit(feats, ids)
    return st.next()

"""Batches whose questions share images: the index machinery of forward(..., img_index) (HieCoAttenLadder, MFB, MHBCoAtt),
the region counts of forward((img, img_length), ...) (MFB, MHBCoAtt, HieCoAttenLadder) and the packed region features of
forward(PackedRegions(rows, offsets, max_regions), ...) (MFB, MHBCoAtt, HieCoAttenLadder).

img_index (N,) says which of the U images of the batch question n looks at.  It is never read on the host: _group_index clamps
it and derives, on the device, what the grouped kernels of include/vqa_fusion.h take (idx / order / grp_off), and every kernel
clamps what it reads from those arrays again.
"""
import collections

import torch

from .lib import VqfError


def _group_index(img_index, U):
    """img_index (N,) int64 / int32 on any device, U images -> (idx32 (N,), order (N,), grp_off (U + 1,)), int32 on that device:
    idx32 = the index clamped to [0, U - 1]; order = the questions sorted by image (stable: ascending n inside an image);
    image u's questions are order[grp_off[u]:grp_off[u + 1]].  O(N) torch ops, nothing read back to the host (the counts are
    a scatter_add_: torch.bincount would read the maximum back)."""
    idx = img_index.to(torch.int64).clamp(0, U - 1)
    order = torch.sort(idx, stable=True).indices
    counts = torch.zeros(U, dtype=torch.int64, device=idx.device).scatter_add_(0, idx, torch.ones_like(idx))
    grp_off = torch.zeros(U + 1, dtype=torch.int64, device=idx.device)
    grp_off[1:] = torch.cumsum(counts, 0)
    return idx.to(torch.int32).contiguous(), order.to(torch.int32).contiguous(), grp_off.to(torch.int32).contiguous()


def check_img_index(who, img_index, N, U, device):
    """The refusals every forward(..., img_index) shares: type, integer dtype, shape (N,), the questions' device, and the
    16-bit extents of the grouped kernels' grids.  Raises VqfError naming what was passed."""
    if not torch.is_tensor(img_index) or img_index.dtype not in (torch.int64, torch.int32):
        raise VqfError("%s: img_index must be an int64 or int32 tensor, got %s"
                       % (who, img_index.dtype if torch.is_tensor(img_index) else type(img_index).__name__))
    if tuple(img_index.shape) != (N,):
        raise VqfError("%s: img_index must have shape (N,) = (%d,), got %s" % (who, N, tuple(img_index.shape)))
    if img_index.device != device:
        raise VqfError("%s: img_index must be on the questions' device (%s), got %s" % (who, device, img_index.device))
    if not (1 <= U <= 65535 and 1 <= N <= 65535):
        raise VqfError("%s: img_index takes 1 <= U <= 65535 images and 1 <= N <= 65535 questions (got U=%d, N=%d)" % (who, U, N))


def check_img_length(who, img_length, count, device):
    """The refusals of forward((img, img_length), ...): type, integer dtype, shape (count,) -- one count per image: N, or U with
    img_index -- and the questions' device.  Raises VqfError naming what was passed."""
    if not torch.is_tensor(img_length) or img_length.dtype not in (torch.int64, torch.int32):
        raise VqfError("%s: img_length must be an int64 or int32 tensor, got %s"
                       % (who, img_length.dtype if torch.is_tensor(img_length) else type(img_length).__name__))
    if tuple(img_length.shape) != (count,):
        raise VqfError("%s: img_length must have shape (%d,) (one region count per image), got %s"
                       % (who, count, tuple(img_length.shape)))
    if img_length.device != device:
        raise VqfError("%s: img_length must be on the questions' device (%s), got %s" % (who, device, img_length.device))


def _region_lens(img_length, L, idx=None):
    """img_length (count,) int64 / int32 -> what the region-count kernels take, int32 on that device, clamped to [1, L] there and
    never read on the host: lens (N,) without img_index; with it (idx = _group_index's idx32) the pair (lens_q (N,) =
    lens_u[idx], lens_u (U,)) -- one O(N) gather."""
    lens = img_length.clamp(1, L).to(torch.int32).contiguous()
    if idx is None:
        return lens
    return lens[idx.to(torch.int64)].contiguous(), lens


class RegionLayout(collections.namedtuple("_RegionLayout", "N U L R idx order grp_off lens_u lens_q roff offsets grouped counted packed plain grp rows")):
    """Where the image rows of a batch are: what forward(..., img_index), forward((img, img_length), ...) and
    forward(PackedRegions, ...) hand to the nodes, in one immutable object.  N questions, U images (U = N without img_index), L the
    padded width, R the rows of the image tensor (U * L unless packed).  idx / order / grp_off: _group_index's output, or None
    without img_index.  lens_u (U,) / lens_q (N,) = lens_u[idx]: _region_lens' counts per image and per question (the same tensor
    without img_index), or None without img_length.  roff (U + 1,) int32: the row offsets of the packed form (which carries its
    counts there: no lens), or None; offsets: the tensor roff was converted from, kept for padded().
    Views, so that no node tests two fields to find its form: grouped (questions share images), counted (region counts beside a
    padded tensor), packed (the image tensor holds the real rows only), plain (none of the three), grp = (idx, order, grp_off) or
    None.  rows (packed only; see packed_rows()): what the fusion hands on -- its output, the co-attention head's hidden layers and
    logits, and their gradients -- holds the R real rows as well.  Every tensor is made on the device; nothing here reads a tensor's
    values on the host."""
    __slots__ = ()

    def __new__(cls, N, U, L, img_index=None, img_length=None, offsets=None, R=None):
        idx, order, grp_off = (None, None, None) if img_index is None else _group_index(img_index, U)
        lens_q = lens_u = None
        if img_length is not None:
            lens = _region_lens(img_length, L, idx)
            lens_q, lens_u = (lens, lens) if idx is None else lens
        roff = None if offsets is None else offsets.to(torch.int32).contiguous()
        return cls._of(N, U, L, U * L if R is None else R, idx, order, grp_off, lens_u, lens_q, roff, offsets)

    @classmethod
    def _of(cls, N, U, L, R, idx, order, grp_off, lens_u, lens_q, roff, offsets, rows=False):
        grouped, counted, packed = idx is not None, lens_u is not None, roff is not None
        return tuple.__new__(cls, (N, U, L, R, idx, order, grp_off, lens_u, lens_q, roff, offsets, grouped, counted, packed,
                                   not (grouped or counted or packed), (idx, order, grp_off) if grouped else None,
                                   bool(rows) and packed and not grouped))

    def packed_rows(self):
        """The same packed batch with the rows BEHIND the fusion packed too (MFB / MHBCoAtt packed_coatt): the fusion's output, the
        co-attention head's tensors and their gradients are (R, .); the attention weights stay (N, G, L).  Only a packed layout
        without shared images has that form; any other is returned as it is."""
        if not self.packed or self.grouped or self.rows:
            return self
        return self._of(self.N, self.U, self.L, self.R, None, None, None, None, None, self.roff, self.offsets, True)

    def padded(self):
        """The same batch after its packed rows were laid out padded, (U*L, .): roff is dropped and the counts are those of the
        offsets, through img_length's clamp.  Any other layout is returned as it is."""
        if not self.packed:
            return self
        lens = _region_lens(self.offsets[1:] - self.offsets[:-1], self.L, self.idx)
        lens_q, lens_u = lens if self.grouped else (lens, lens)
        return self._of(self.N, self.U, self.L, self.U * self.L, self.idx, self.order, self.grp_off, lens_u, lens_q, None, None)

    def per_question(self):
        """The layout behind a row-block gather of the padded rows (hie_ladder.RowBlockGatherFn): one image per question."""
        return self._of(self.N, self.N, self.L, self.N * self.L, None, None, None, self.lens_q, self.lens_q, None, None)


class PackedRegions:
    """Region features that were never padded (forward(PackedRegions(rows, offsets, max_regions), ...); MFB, MHBCoAtt,
    HieCoAttenLadder, fp32):
    rows (R, D) holds every image's real regions, one image after the other; image i owns rows offsets[i] .. offsets[i + 1] - 1
    (offsets (N + 1,) int64 / int32 -- (U + 1,) with img_index --, offsets[0] = 0, non-decreasing, offsets[-1] = R, every count
    in [1, max_regions]); max_regions is a Python int L in [1, 1024], the padded width of what stays per (image, region) slot.
    The model's result is, by definition, its result on (unpack(), ...): the region-count call.  data_loader.pack_region_features
    builds one on the CPU; .to(device) moves both tensors.  The models never read offsets on the host."""
    __slots__ = ("rows", "offsets", "max_regions")

    def __init__(self, rows, offsets, max_regions):
        self.rows, self.offsets, self.max_regions = rows, offsets, max_regions

    def to(self, device, non_blocking=False):
        return PackedRegions(self.rows.to(device, non_blocking=non_blocking), self.offsets.to(device, non_blocking=non_blocking),
                             self.max_regions)

    def unpack(self):
        """-> (img (N, L, D) zero-padded on the right, img_length (N,) int64) on the tensors' devices: what
        data_loader.pad_region_features returns for the same features."""
        off = self.offsets.to(torch.int64)
        R, D = self.rows.shape
        N, L = off.numel() - 1, int(self.max_regions)
        counts = off[1:] - off[:-1]
        dev = self.rows.device
        owner = torch.repeat_interleave(torch.arange(N, device=off.device), counts, output_size=R).to(dev)
        pos = torch.arange(R, device=dev) - off.to(dev)[owner]
        img = torch.zeros((N, L, D), dtype=self.rows.dtype, device=dev)
        img[owner, pos] = self.rows
        return img, counts


def check_packed_regions(who, packed, owners, device):
    """The refusals of forward(PackedRegions, ...) that concern the object itself: rows 2-D fp32, offsets an int64 / int32 tensor of
    shape (owners + 1,) on the questions' device (owners = N, or U with img_index), max_regions an int in [1, 1024].  Raises VqfError
    naming what was passed."""
    rows, off, L = packed.rows, packed.offsets, packed.max_regions
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.dtype != torch.float32 or rows.shape[0] < 1:
        raise VqfError("%s: PackedRegions.rows must be a 2-D fp32 tensor (R, D) with R >= 1, got %s"
                       % (who, "%s %s" % (rows.dtype, tuple(rows.shape)) if torch.is_tensor(rows) else type(rows).__name__))
    if not torch.is_tensor(off) or off.dtype not in (torch.int64, torch.int32):
        raise VqfError("%s: PackedRegions.offsets must be an int64 or int32 tensor, got %s"
                       % (who, off.dtype if torch.is_tensor(off) else type(off).__name__))
    if tuple(off.shape) != (owners + 1,):
        raise VqfError("%s: PackedRegions.offsets must have shape (%d,) (one more than the images), got %s"
                       % (who, owners + 1, tuple(off.shape)))
    if off.device != device:
        raise VqfError("%s: PackedRegions.offsets must be on the questions' device (%s), got %s" % (who, device, off.device))
    if isinstance(L, bool) or not isinstance(L, int) or not 1 <= L <= 1024:
        raise VqfError("%s: PackedRegions.max_regions must be a Python int in [1, 1024], got %r" % (who, L))


SOFT_MAX_SLOTS = 16      # VQF_SOFT_MAX_SLOTS of include/vqa_fusion.h


class SoftAnswers:
    """Sparse soft targets of BCEWithLogitsLoss / ops.bce_logits_loss: ids (N, K) int64 / int32, scores (N, K) fp32, 1 <= K <= 16.
    Row n holds K (answer id, soft score) slots; a slot whose id is negative or >= A (the logits' width) is empty and its score is
    ignored; a repeated id adds its scores.  Every call with a SoftAnswers is, by definition, the call with .dense(A).
    data_loader.soft_answers builds one on the CPU; .to(device) moves both tensors.  The ids are never read on the host."""
    __slots__ = ("ids", "scores")

    def __init__(self, ids, scores):
        self.ids, self.scores = ids, scores

    def to(self, device, non_blocking=False):
        return SoftAnswers(self.ids.to(device, non_blocking=non_blocking), self.scores.to(device, non_blocking=non_blocking))

    def dense(self, A):
        """-> the (N, A) fp32 tensor the slots stand for, on the tensors' device: zeros, then the live slots added."""
        check_soft_answers("SoftAnswers.dense", self)
        A = int(A)
        ids = self.ids.to(torch.int64)
        N, K = ids.shape
        live = (ids >= 0) & (ids < A)
        rows = torch.arange(N, device=ids.device).unsqueeze(1).expand(N, K)
        t = torch.zeros((N, A), dtype=torch.float32, device=ids.device)
        t.index_put_((rows[live], ids[live]), self.scores[live], accumulate=True)
        return t


def check_soft_answers(who, soft, N=None, device=None):
    """The refusals that concern the SoftAnswers itself: ids an int64 / int32 (N, K) tensor, scores an fp32 tensor of the same
    shape on the same device, 1 <= K <= 16; with N / device given, that many rows on that device.  Raises VqfError."""
    ids, sc = soft.ids, soft.scores
    if not torch.is_tensor(ids) or ids.dtype not in (torch.int64, torch.int32) or ids.dim() != 2:
        raise VqfError("%s: SoftAnswers.ids must be a 2-D int64 or int32 tensor (N, K), got %s"
                       % (who, "%s %s" % (ids.dtype, tuple(ids.shape)) if torch.is_tensor(ids) else type(ids).__name__))
    if not torch.is_tensor(sc) or sc.dtype != torch.float32:
        raise VqfError("%s: SoftAnswers.scores must be an fp32 tensor, got %s"
                       % (who, sc.dtype if torch.is_tensor(sc) else type(sc).__name__))
    if sc.shape != ids.shape:
        raise VqfError("%s: SoftAnswers.ids and .scores must have the same shape, got %s and %s"
                       % (who, tuple(ids.shape), tuple(sc.shape)))
    if not 1 <= ids.shape[1] <= SOFT_MAX_SLOTS:
        raise VqfError("%s: SoftAnswers holds 1 to %d slots per row, got K = %d" % (who, SOFT_MAX_SLOTS, ids.shape[1]))
    if sc.device != ids.device:
        raise VqfError("%s: SoftAnswers.ids and .scores must be on one device, got %s and %s" % (who, ids.device, sc.device))
    if N is not None and ids.shape[0] != N:
        raise VqfError("%s: SoftAnswers must have one row per logits row (%d), got %d" % (who, N, ids.shape[0]))
    if device is not None and ids.device != device:
        raise VqfError("%s: SoftAnswers must be on the logits' device (%s), got %s" % (who, device, ids.device))

"""Batches whose questions share images: the index machinery of forward(..., img_index) (HieCoAttenLadder, MFB, MHBCoAtt),
and the region counts of forward((img, img_length), ...) (MFB, MHBCoAtt).

img_index (N,) says which of the U images of the batch question n looks at.  It is never read on the host: _group_index clamps
it and derives, on the device, what the grouped kernels of include/vqa_fusion.h take (idx / order / grp_off), and every kernel
clamps what it reads from those arrays again.
"""
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

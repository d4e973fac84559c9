"""fp64 specification of HieCoAttenLadder.forward(img (U, L, D), ids (N, T), q_length, img_index (N,)): U images shared by N
questions.  It is the existing restatements (tests/hie_ladder_ref.py, hie_ladder_len_ref.py, hie_ladder_alt_ref.py) run on the
EXPANDED batch img[idx], with the per-image 'img' keep-mask (U*L, E) expanded the same way; idx is the index clamped to
[0, U - 1].  index_select's autograd backward is the sum over each image's questions, so gradients need no further statement.
Nothing of the kernels is restated here."""
import torch

import hie_ladder_ref as R
import hie_ladder_len_ref as RL
import hie_ladder_alt_ref as RA


def clamp_index(img_index, U):
    return img_index.to(torch.int64).clamp(0, U - 1)


def expand_masks(masks, idx, U):
    """the 'img' keep-mask (U*L, E) -> (N*L, E): question n gets the mask of its image; the other masks are per question"""
    if not masks or masks.get("img") is None:
        return masks
    m = dict(masks)
    k = m["img"]
    E = k.shape[-1]
    m["img"] = k.reshape(U, -1, E).index_select(0, idx.to(k.device)).reshape(-1, E)
    return m


def forward(sd, img, ids, img_index, lengths=None, masks=None, p=0.5, dtype=torch.float64, coatt="parallel"):
    """sd, ids, lengths, masks, p, dtype as in the underlying references; img (U, L, D); img_index (N,) integers; masks['img'] is
    (U*L, E).  -> (logits (N, out), av (N, 3, L), aq (N, 3, T))"""
    U = img.shape[0]
    idx = clamp_index(img_index, U).to(img.device)
    big = img.index_select(0, idx)
    m = expand_masks(masks, idx, U)
    if coatt == "alternating":
        return RA.forward(sd, big, ids, lengths, masks=m, p=p, dtype=dtype)
    if lengths is not None:
        return RL.forward(sd, big, ids, lengths, masks=m, p=p, dtype=dtype)
    return R.forward(sd, big, ids, masks=m, p=p, dtype=dtype)

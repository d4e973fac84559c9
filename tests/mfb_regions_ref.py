"""TEST INFRASTRUCTURE ONLY: MFB / MHBCoAtt with per-image region counts (forward((img, img_length), ...)), restated in torch.

img (N, L, D) is right-padded and sample n has lens[n] real regions; with valid[n, l] = l < lens[n] the result is the model on
the first lens[n] regions of each sample: the fusion's signed square roots are zero on padding (so the per-sample L2 norm runs
over the real rows), the co-attention softmax runs over the real regions (under the reference's singleton-axis softmax the
weights are 1 there) and its weights are zero on padding.  Everything that does not touch the region axis is the oracle's own
code (oracle.ref_torch), so the restatement differs from it on the image side only.  Runs in the dtype of `sd` / `img`
(fp32 or fp64); explicit keep masks as in the oracle.  tests/test_mfb_regions_cpu.py pins it against the oracle.
"""
import torch
import torch.nn.functional as F

from oracle import ref_torch as O


def valid_mask(lens, L):
    """(N, L) bool: l < clamp(lens[n], 1, L)"""
    return torch.arange(L)[None, :] < lens.to(torch.int64).clamp(1, L)[:, None]


def _trunk(sd, cfg, img, q, lens, glove, drop, mhb, live_softmax):
    drop = drop or {}
    unit = (not mhb) and not live_softmax
    multilayer = (not mhb) and getattr(cfg, "model_name", "") == "mfb-multilayer"
    N, L, D = img.shape
    valid = valid_mask(lens, L)                                           # (N, L)
    vf = valid.to(img.dtype)

    # question side: the oracle's lines, unchanged (oracle.ref_torch._coatt_trunk a2-a4)
    e = torch.tanh(F.embedding(q, sd["word_embedding.weight"]))
    if mhb and getattr(cfg, "glove", False):
        e = torch.cat((e, glove), dim=2)
    lw = [sd["lstm.weight_ih_l0"], sd["lstm.weight_hh_l0"], sd["lstm.bias_ih_l0"], sd["lstm.bias_hh_l0"]]
    if mhb:
        h = O._apply_keep(O.lstm_layer(e.permute(1, 0, 2), *lw), drop.get("l"), 0.3).permute(1, 0, 2)
    else:
        h = O._apply_keep(O.lstm_layer(e, *lw), drop.get("l"), 0.3)
    a = F.relu(h @ sd["ques_att_conv1.weight"].flatten(1).t() + sd["ques_att_conv1.bias"])
    if multilayer:
        a = F.relu(a @ sd["ques_att_multiconv.weight"].flatten(1).t() + sd["ques_att_multiconv.bias"])
    qlog = a @ sd["ques_att_conv2.weight"].flatten(1).t() + sd["ques_att_conv2.bias"]
    qa, _ = O.glimpse_attention(h, qlog, compat_unit_softmax=unit)
    qp = qa @ sd["ques_proj1.weight"].t() + sd["ques_proj1.bias"]

    # image side with valid[n, l]
    P = img @ sd["img_conv1d.weight"].flatten(1).t() + sd["img_conv1d.bias"]              # every row, padded ones included
    Z = O._apply_keep(P * qp[:, None, :], drop.get("m1"), 0.1)
    S = Z.reshape(N, L, O.O_POOL, O.K_POOL).sum(3)
    # (a padded row never reaches the square root: neither its value nor its derivative at 0)
    R = O.signed_sqrt(torch.where(valid[:, :, None], S, torch.ones_like(S))) * vf[:, :, None]
    Y = F.normalize(R.reshape(N, -1)).reshape(N, L, O.O_POOL)                              # norm over the real rows
    c = F.relu(Y @ sd["co_att_conv1.weight"].flatten(1).t() + sd["co_att_conv1.bias"])
    if multilayer:
        c = F.relu(c @ sd["co_att_multiconv.weight"].flatten(1).t() + sd["co_att_multiconv.bias"])
    clog = c @ sd["co_att_conv2.weight"].flatten(1).t() + sd["co_att_conv2.bias"]         # (N, L, 2)
    if unit:
        # mfb.py:118: softmax over a singleton axis == 1 on every real region; padding has no weight
        w = torch.softmax(clog.permute(0, 2, 1).unsqueeze(-1), dim=3).squeeze(-1) * vf[:, None, :]
    else:
        w = torch.softmax(clog.permute(0, 2, 1).masked_fill(~valid[:, None, :], float("-inf")), dim=2)
    va = torch.einsum("ngs,nsc->ngc", w, img * vf[:, :, None]).reshape(N, -1)
    return dict(qa=qa, qp=qp, P=P, S=S, R=R, Y=Y, clog=clog, vw=w, va=va, valid=valid)


def mfb_forward(sd, cfg, img, q, lens, drop=None, live_softmax=False, return_all=False):
    """MFB on the first lens[n] regions of each sample -> logits (N, A)"""
    drop = drop or {}
    t = _trunk(sd, cfg, img, q, lens, None, drop, False, live_softmax)
    y = O._final_block(sd, t["qa"], t["va"], "ques_proj2", "img_proj2", drop.get("m2"))
    logits = y @ sd["linear_pred.weight"].t() + sd["linear_pred.bias"]
    if return_all:
        t.update(y=y, logits=logits)
        return t
    return logits


def mhbcoatt_forward(sd, cfg, img, q, lens, glove=None, drop=None, return_all=False):
    """MHBCoAtt on the first lens[n] regions of each sample -> log-probs (N, A)"""
    drop = drop or {}
    t = _trunk(sd, cfg, img, q, lens, glove, drop, True, False)
    y2 = O._final_block(sd, t["qa"], t["va"], "ques_proj2", "img_proj2", drop.get("m2"))
    y3 = O._final_block(sd, t["qa"], t["va"], "ques_proj3", "img_proj3", drop.get("m3"))
    logits = torch.cat([y2, y3], 1) @ sd["linear_pred.weight"].t() + sd["linear_pred.bias"]
    out = F.log_softmax(logits, dim=1)
    if return_all:
        t.update(logits=logits, out=out)
        return t
    return out


def fuse_ref(P, pb, q, lens, N, L, O_, keep=None, p=0.1, idx=None, U=None):
    """The fusion stage alone in the dtype of P (fp64 in the kernel tests): P (rows, 5 O_) leaf, pb (5 O_), q (N, 5 O_);
    idx (N) gathers the rows of shared images (P is (U*L, 5 O_), lens per question).  -> (R (N*L, O_) with zero padded rows,
    Y = R / ||R_n||, norm (N), valid (N, L))."""
    W5 = 5 * O_
    Pg = (P + pb).view(-1, L, W5)
    if idx is not None:
        Pg = Pg[idx]
    z = Pg * q[:, None, :]
    if keep is not None:
        z = z * (keep.to(z.dtype).view(N, L, W5) / (1.0 - p))
    valid = valid_mask(lens, L)
    S = z.reshape(N, L, O_, 5).sum(3)
    R = O.signed_sqrt(torch.where(valid[:, :, None], S, torch.ones_like(S))) * valid[:, :, None].to(S.dtype)
    norm = R.reshape(N, -1).norm(dim=1)
    Y = F.normalize(R.reshape(N, -1)).reshape(N * L, O_)
    return R.reshape(N * L, O_), Y, norm, valid

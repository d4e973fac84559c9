"""fp64 references of the packed forms of HieCoAttenLadder's alternating image side (include/vqa_fusion.h
vqf_guided_logits_fwd_packed / _bwd_packed, vqf_glimpse_pool_bwd_packed_dfeat): Xh / dXh (R, G E) and feat / dfeat (R, C) hold the
real rows of every owner, one owner after the other; logits / dlogits (N, L, G), gp / dgp (N, G E), dw (G, E) and wts (N, G, L)
stay in padded coordinates.  Every function takes ANY offsets through mfb_packed_ref.clamped_spans -- owner u has
start = clamp(off[u], 0, R - 1) and cnt = clamp(off[u+1] - off[u], 1, min(L, R - start)) -- which is the kernels' rule; idx (N,)
or None: question n reads owner idx[n] (clamped to [0, U - 1]), None: owner n.

tests/test_hie_ladder_alt_packed_cpu.py pins them to hie_ladder_regions_ref.coattention_alt on the unpacked copy (values and,
through autograd, every gradient of the image step)."""
import torch

import mfb_packed_ref as PR


def _owners(idx, N, U):
    return list(range(N)) if idx is None else [min(max(int(i), 0), U - 1) for i in torch.as_tensor(idx).tolist()]


def _hidden(xh, gp, n, start, cnt, G, E):
    """H (cnt, G, E) of question n over its owner's rows"""
    pre = xh[start:start + cnt].double().view(cnt, G, E)
    if gp is not None:
        pre = pre + gp[n].double().view(1, G, E)
    return torch.tanh(pre)


def guided_logits_fwd(xh, gp, w, offsets, N, L, idx=None):
    """xh (R, G E), gp (N, G E) or None, w (G, E) -> logits (N, L, G) fp64, exact zeros behind each count"""
    G, E = w.shape
    R = xh.shape[0]
    spans = PR.clamped_spans(offsets, R, L)
    out = torch.zeros(N, L, G, dtype=torch.float64)
    for n, u in enumerate(_owners(idx, N, len(spans))):
        start, cnt = spans[u]
        out[n, :cnt] = (_hidden(xh, gp, n, start, cnt, G, E) * w.double().view(1, G, E)).sum(2)
    return out


def guided_logits_bwd(dl, xh, gp, w, offsets, N, L, idx=None):
    """dl (N, L, G) (rows behind a count are not read) -> (dxh (R, G E): the sum over the questions of each owner, zero rows for an
    owner without one and for rows no span covers; dgp (N, G E); dw (G, E)), fp64"""
    G, E = w.shape
    R = xh.shape[0]
    spans = PR.clamped_spans(offsets, R, L)
    dxh = torch.zeros(R, G * E, dtype=torch.float64)
    dgp = torch.zeros(N, G * E, dtype=torch.float64)
    dw = torch.zeros(G, E, dtype=torch.float64)
    for n, u in enumerate(_owners(idx, N, len(spans))):
        start, cnt = spans[u]
        H = _hidden(xh, gp, n, start, cnt, G, E)
        d = dl[n, :cnt].double().view(cnt, G, 1)
        t = d * w.double().view(1, G, E) * (1 - H * H)
        dxh[start:start + cnt] += t.view(cnt, G * E)
        dgp[n] = t.sum(0).view(G * E)
        dw += (d * H).sum(0)
    return dxh, dgp, dw


def pool_fwd(feat, logits, offsets, N, L, idx=None):
    """feat (R, C), logits (N, L, G) -> (wts (N, G, L): the softmax over each owner's cnt rows, zeros behind; pooled (N, G C))"""
    R, C = feat.shape
    G = logits.shape[2]
    spans = PR.clamped_spans(offsets, R, L)
    wts = torch.zeros(N, G, L, dtype=torch.float64)
    pooled = torch.zeros(N, G * C, dtype=torch.float64)
    for n, u in enumerate(_owners(idx, N, len(spans))):
        start, cnt = spans[u]
        a = torch.softmax(logits[n, :cnt].double(), 0)                       # (cnt, G)
        wts[n, :, :cnt] = a.t()
        pooled[n] = (a.t() @ feat[start:start + cnt].double()).reshape(G * C)
    return wts, pooled


def pool_bwd(dpooled, dwts, feat, wts, offsets, N, L, idx=None):
    """dpooled (N, G C), dwts (N, G, L) or None, wts (N, G, L) -> (dlogits (N, L, G), zeros behind each count; dfeat (R, C): the sum
    over the questions of each owner, zero rows for an owner without one), fp64"""
    R, C = feat.shape
    G = wts.shape[1]
    spans = PR.clamped_spans(offsets, R, L)
    dl = torch.zeros(N, L, G, dtype=torch.float64)
    dfeat = torch.zeros(R, C, dtype=torch.float64)
    for n, u in enumerate(_owners(idx, N, len(spans))):
        start, cnt = spans[u]
        a = wts[n, :, :cnt].double()                                          # (G, cnt)
        dp = dpooled[n].double().view(G, C)
        da = dp @ feat[start:start + cnt].double().t()                        # (G, cnt)
        if dwts is not None:
            da = da + dwts[n, :, :cnt].double()
        dl[n, :cnt] = (a * (da - (a * da).sum(1, keepdim=True))).t()
        dfeat[start:start + cnt] += a.t() @ dp
    return dl, dfeat

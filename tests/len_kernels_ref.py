"""fp64 reference of the twelve length-masked entry points (include/vqa_fusion.h *_len: embed_tanh, phrase_ngram, dropout_bt,
glimpse_pool and its grouped form, hie_affinity / _levels, tanh_bwd_rows), in plain torch.

ONE definition for all of them: the masked operation on sample n is the UNMASKED operation applied to that sample cut to its first
lens[n] rows (lens clamped to [1, T]); the result is put back into the padded shape with zero rows behind it (3 for the phrase
winners).  No masked arithmetic is written here -- the truncation is the mask -- so nothing below can agree with a kernel by
sharing its row test, and what the padded rows of an input hold cannot reach a result.  The unmasked operations are the fp64
formulas the tests of the unmasked kernels use (tests/test_gpu_hie_ladder.py: the phrase windows and gather, the affinity's bmm
and epilogues, the softmax pool and its backward; torch.tanh(W[ids]); x keep / (1 - fp32(p)); dy (1 - y^2)).
tests/test_len_kernels_ref_cpu.py pins this file to the masked model restatement tests/hie_ladder_len_ref.py.

Tensors carry the sample axis first and the padded axis second: (N, T, ...).  Operands are fp64 holding fp32 values."""
import numpy as np
import torch

# (N, T, E, lens) of the phrase kernels' GPU cases (tests/test_gpu_len_kernels.py); the CPU test checks the winners' tie cap on them
PHRASE_CASES = [(6, 7, 8, [1, 2, 3, 6, 7, 4]), (3, 32, 64, [32, 31, 17]), (2, 1, 64, [1, 1])]
IDX_GAP = 1e-5          # the winner is compared where the fp64 top two differ by more than this ...
IDX_CAP = 1e-3          # ... which may exclude at most this share of the real elements


def rnd(shape, seed, scale=1.0):
    """seeded uniform values in [-scale, scale], fp32-representable, as fp64"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().double()


def clamp_lens(lens, T):
    return [min(max(int(l), 1), T) for l in lens]


def fill_padding(x, lens, fill, seed=0):
    """copy of x (N, T, ...) with the rows t >= lens[n] replaced: fill = a number (nan included), "rand": seeded values in [-4, 4],
    or None: x as it is"""
    if fill is None:
        return x
    junk = rnd(x.shape, seed, 4.0).to(x.dtype) if isinstance(fill, str) else torch.full_like(x, fill)
    x = x.clone()
    for n, l in enumerate(clamp_lens(lens, x.shape[1])):
        x[n, l:] = junk[n, l:]
    return x


def padded(rows, T, fill=0.0):
    """per-sample results [(len_n, ...)] -> (N, T, ...), `fill` behind each sample's rows"""
    out = torch.full((len(rows), T) + tuple(rows[0].shape[1:]), fill, dtype=rows[0].dtype)
    for n, r in enumerate(rows):
        out[n, :r.shape[0]] = r
    return out


def truncated(fn, lens, T, *xs, fill=0.0):
    """the definition: fn over each sample cut to its length.  xs: (N, T, ...) tensors or None; fn(n, *cut) -> a tuple of
    (len_n, ...) tensors -> the tuple of padded (N, T, ...) tensors"""
    res = [fn(n, *[None if x is None else x[n, :l] for x in xs]) for n, l in enumerate(clamp_lens(lens, T))]
    fills = fill if isinstance(fill, (tuple, list)) else (fill,) * len(res[0])
    return tuple(padded([r[i] for r in res], T, fills[i]) for i in range(len(res[0])))


# ---- phrase level -------------------------------------------------------------------------------------------------------------------
def phrase_inputs(N, T, E):
    """Z (N, T, 6E), bias (3E), dQp (N, T, E) of one GPU case (scales of test_phrase_ngram_kernels)"""
    return rnd((N, T, 6 * E), 1 + T, 1.5), rnd((3 * E,), 2 + T, 0.5), rnd((N, T, E), 3 + T)


def phrase_u(Z, bias):
    """one unpadded sample: Z (T, 6E), bias (3E) -> u (3, T, E), u_k[t] = b_k + sum_{j<k, t+j<T} Z[t + j, tap(k, j)]"""
    T, E = Z.shape[0], Z.shape[1] // 6
    u = []
    for k in (1, 2, 3):
        acc = bias[(k - 1) * E:k * E].expand(T, E).clone()
        for j in range(min(k, T)):
            c0 = (k * (k - 1) // 2 + j) * E
            acc[:T - j] += Z[j:, c0:c0 + E]
        u.append(acc)
    return torch.stack(u, 0)


def phrase_fwd(Z, bias, lens):
    """-> Qp (N, T, E) = tanh(max_k u_k) (0 on padding), idx (N, T, E) int64 = the winning k - 1 (3 on padding), clear (N, T, E)
    bool: the fp64 top two differ by more than IDX_GAP (padding: True, its 3 is exact)"""
    def one(n, z):
        u = phrase_u(z, bias)
        top2 = u.sort(0, descending=True).values
        return torch.tanh(top2[0]), u.argmax(0), top2[0] - top2[1] > IDX_GAP
    return truncated(one, lens, Z.shape[1], Z, fill=(0.0, 3, True))


def phrase_bwd(dQp, Qp, idx, lens):
    """-> dZ (N, T, 6E): du = dQp (1 - Qp^2) gathered at the winning taps (Qp, idx: the forward's)"""
    def one(n, dq, qp, win):
        T, E = dq.shape
        du = dq * (1 - qp ** 2)
        ref = torch.zeros(T, 6 * E, dtype=torch.float64)
        for k in (1, 2, 3):
            for j in range(min(k, T)):
                c0 = (k * (k - 1) // 2 + j) * E
                ref[j:, c0:c0 + E] = torch.where(win[:T - j] == k - 1, du[:T - j], torch.zeros(()).double())
        return (ref,)
    return truncated(one, lens, dQp.shape[1], dQp, Qp, idx)[0]


# ---- embedding ----------------------------------------------------------------------------------------------------------------------
def embed_fwd(W, ids, lens):
    """-> (N, Tq, E) = tanh(W[ids]) on the real tokens (whose ids are inside [0, V))"""
    return truncated(lambda n, i: (torch.tanh(W[i]),), lens, ids.shape[1], ids)[0]


def embed_bwd(dout, out, ids, lens, V):
    """-> dW (V, E): the real tokens' dout (1 - out^2) summed per id"""
    dW = torch.zeros(V, dout.shape[2], dtype=torch.float64)

    def one(n, d, o, i):
        dW.index_add_(0, i, d * (1 - o ** 2))
        return (d,)
    truncated(one, lens, ids.shape[1], dout, out, ids)
    return dW


# ---- element-wise -------------------------------------------------------------------------------------------------------------------
def dropout_bt(x, keep, p, lens):
    """x, keep (B, T, H) -> x keep / (1 - fp32(p))"""
    inv = 1.0 / (1.0 - float(np.float32(p)))
    return truncated(lambda n, a, k: (a * k.double() * inv,), lens, x.shape[1], x, keep)[0]


def tanh_bwd_rows(dy, y, lens):
    return truncated(lambda n, d, v: (d * (1 - v ** 2),), lens, dy.shape[1], dy, y)[0]


# ---- softmax pool -------------------------------------------------------------------------------------------------------------------
def pool_fwd(feat, logits, lens, unit=False, idx=None):
    """feat (N, S, C) (idx: (U, S, C), question n pools feat[idx[n]]), logits (N, S, G) -> wts (N, G, S), pooled (N, G C)"""
    if idx is not None:
        feat = feat[idx]

    def one(n, f, lg):
        sm = torch.ones_like(lg.t()) if unit else torch.softmax(lg.t(), 1)          # (G, len)
        return sm.t(), (sm @ f).reshape(1, -1).expand(f.shape[0], -1)
    wts, pooled = truncated(one, lens, feat.shape[1], feat, logits)
    return wts.transpose(1, 2).contiguous(), pooled[:, 0].contiguous()


def pool_bwd(dpooled, dwts_extra, feat, wts, lens, unit=False, idx=None, U=None):
    """dpooled (N, G C), dwts_extra (N, G, S) or None, wts (N, G, S) (the forward's) -> dlogits (N, S, G), dfeat (N, S, C) (idx:
    (U, S, C), summed per image)"""
    N, G, S = wts.shape
    if idx is not None:
        feat = feat[idx]
    C = feat.shape[2]

    def one(n, f, w, dx):
        sm, dp = w.t(), dpooled[n].view(G, C)                                        # (G, len), (G, C)
        dwt = dp @ f.t() + (0.0 if dx is None else dx.t())
        dl = torch.zeros_like(sm) if unit else sm * (dwt - (sm * dwt).sum(1, keepdim=True))
        return dl.t(), sm.t() @ dp
    dl, df = truncated(one, lens, S, feat, wts.transpose(1, 2), None if dwts_extra is None else dwts_extra.transpose(1, 2))
    if idx is not None:
        df = torch.zeros(U, S, C, dtype=torch.float64).index_add_(0, idx, df)
    return dl, df


# ---- affinity -----------------------------------------------------------------------------------------------------------------------
def affinity(x1, y1, lens, x2=None, y2=None, epi=0, yprev=None, keep=None, p=0.0):
    """x* (N, T, E), y* (N, L, E), yprev / keep (N, T, L) -> (N, T, L): epi(x1 y1^T [+ x2 y2^T]); epi 1: tanh(.) keep / (1 - p),
    epi 2: its backward given its output yprev (without keep: tanh and (1 - yprev^2))"""
    inv = 1.0 / (1.0 - float(np.float32(p))) if keep is not None else 1.0

    def one(n, a1, a2, yp, k):
        s = a1 @ y1[n].t()
        if a2 is not None:
            s = s + a2 @ y2[n].t()
        sc = 1.0 if k is None else k.double() * inv
        if epi == 1:
            s = torch.tanh(s) * sc
        elif epi == 2:
            s = s * sc * (1 - (yp / inv) ** 2)
        return (s,)
    return truncated(one, lens, x1.shape[1], x1, x2, yprev, keep)[0]

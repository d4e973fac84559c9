"""tests/len_kernels_ref.py (the truncation reference of the *_len kernels) against what the project already trusts, on the CPU:
the masked model restatement tests/hie_ladder_len_ref.py (itself pinned sample by sample on hie_ladder_ref by
tests/test_hie_ladder_lengths_cpu.py) for the phrase level, the affinity and the question-side softmax pool; for every input
family, that the reference does not depend on what the padded rows hold; and the cap on the phrase winners that
tests/test_gpu_len_kernels.py leaves uncompared."""
import pytest
import torch

import hie_ladder_len_ref as MR
import len_kernels_ref as LR

NAN = float("nan")
LENS = [1, 7, 3, 6, 2]


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol


@pytest.mark.parametrize("N,T,E,lens", LR.PHRASE_CASES)
def test_phrase_reference_matches_the_masked_phrase_level(N, T, E, lens):
    valid = MR.valid_mask(torch.tensor(lens), T)
    qw = LR.rnd((N, T, E), 11) * valid.unsqueeze(2)
    sd = {}
    for k, name in ((1, "phrase_uni"), (2, "phrase_bi"), (3, "phrase_tri")):
        sd[name + ".weight"], sd[name + ".bias"] = LR.rnd((E, E, k), 20 + k, 0.4), LR.rnd((E,), 30 + k, 0.5)
    want = MR.phrase_level(qw, valid, sd, torch.float64)
    # Z = Qw Wcat^T, tap (k, j) at column block k (k - 1) / 2 + j; its padded rows are zero in the model -- here they hold + 50
    taps = [sd[name + ".weight"][:, :, j] for k, name in ((1, "phrase_uni"), (2, "phrase_bi"), (3, "phrase_tri")) for j in range(k)]
    Z = torch.cat([qw @ w.t() for w in taps], 2)
    bias = torch.cat([sd[n + ".bias"] for n in ("phrase_uni", "phrase_bi", "phrase_tri")])
    qp, idx, clear = LR.phrase_fwd(LR.fill_padding(Z, lens, 50.0), bias, lens)
    assert _close(qp, want)
    assert bool((idx[~valid] == 3).all()) and bool((qp[~valid] == 0).all()) and bool((idx[valid] < 3).all())


def test_pool_and_affinity_reference_match_the_masked_coattention():
    N, T, L, E = 5, 7, 6, 8
    valid = MR.valid_mask(torch.tensor(LENS), T)
    V, Q = LR.rnd((N, L, E), 41), LR.rnd((N, T, E), 42) * valid.unsqueeze(2)
    sd = {"coatt.0.%s.weight" % n: LR.rnd(s, 50 + i, 0.6) for i, (n, s) in enumerate(
        (("Wb", (E, E)), ("Wv", (E, E)), ("Wq", (E, E)), ("whv", (1, E)), ("whq", (1, E))))}
    v, q, av, aq = MR.coattention(V, Q, valid, sd, 0)
    # the operands of the kernels, with values in the padded rows that would win: C = tanh(Cq V^T), then the logits of Hq
    Cq = LR.fill_padding(Q @ sd["coatt.0.Wb.weight"].t(), LENS, "rand", 1)
    C = LR.affinity(Cq, V, LENS, epi=1)
    want_C = torch.tanh(torch.matmul(Q @ sd["coatt.0.Wb.weight"].t(), V.transpose(1, 2))) * valid.unsqueeze(2)
    assert _close(C, want_C) and bool((C[~valid] == 0).all())
    Hq = torch.tanh(Q @ sd["coatt.0.Wq.weight"].t() + torch.matmul(C, V @ sd["coatt.0.Wv.weight"].t()))
    lq = Hq @ sd["coatt.0.whq.weight"].t()                                            # (N, T, 1)
    wts, pooled = LR.pool_fwd(LR.fill_padding(Q, LENS, "rand", 2), LR.fill_padding(lq, LENS, 30.0), LENS)
    assert _close(wts[:, 0], aq) and _close(pooled, q)
    assert bool((wts[:, 0][~valid] == 0).all()) and bool((aq[~valid] == 0).all())
    assert _close(wts.sum(2), torch.ones(N, 1))


def test_reference_does_not_depend_on_the_padded_rows():
    """every input family, two fillings of the padded rows (values that would win / NaN): equal bits"""
    N, T, E, L, G, C, V = 5, 7, 8, 6, 2, 4, 12
    ids = torch.randint(0, V, (N, T), generator=torch.Generator().manual_seed(3))
    keep = (torch.rand((N, T, L), generator=torch.Generator().manual_seed(4)) >= 0.3).to(torch.uint8)
    img = torch.tensor([2, 0, 0, 2, 1])
    got = []
    for hot, other, seed in ((50.0, "rand", 5), (NAN, NAN, 6)):
        f = lambda x, v=other, s=0: LR.fill_padding(x, LENS, v, seed + s)
        Z, bias, dQp = LR.phrase_inputs(N, T, E)
        qp, idx, _ = LR.phrase_fwd(f(Z, hot), bias, LENS)
        wts, pooled = LR.pool_fwd(f(LR.rnd((N, T, C), 7)), f(LR.rnd((N, T, G), 8), 30.0 if hot == 50.0 else NAN), LENS)
        res = [qp, idx.double(), LR.phrase_bwd(f(dQp), qp, idx, LENS),
               LR.embed_fwd(LR.rnd((V, E), 9), torch.where(MR.valid_mask(torch.tensor(LENS), T), ids, ids * 0 + (seed % V)), LENS),
               LR.embed_bwd(f(LR.rnd((N, T, E), 10), "rand"), f(LR.rnd((N, T, E), 11, 0.9), "rand", 1), ids, LENS, V),
               LR.dropout_bt(f(LR.rnd((N, T, L), 12)), keep, 0.3, LENS), LR.tanh_bwd_rows(f(LR.rnd((N, T, L), 13)), f(LR.rnd((N, T, L), 14)), LENS),
               wts, pooled,
               *LR.pool_bwd(LR.rnd((N, G * C), 15), f(LR.rnd((N, T, G), 16)).transpose(1, 2), f(LR.rnd((N, T, C), 7)), wts, LENS),
               LR.affinity(f(LR.rnd((N, T, E), 17)), LR.rnd((N, L, E), 18), LENS, x2=f(LR.rnd((N, T, E), 19)), y2=LR.rnd((N, L, E), 20),
                           epi=2, yprev=f(LR.rnd((N, T, L), 21, 0.9)), keep=keep, p=0.3)]
        # grouped: the padded rows of an image are those beyond its count, lens per question = counts[img]
        counts = [3, 7, 1]
        lq = [counts[u] for u in img.tolist()]
        fu = LR.fill_padding(LR.rnd((3, T, C), 22), counts, other, seed)
        gw, gp = LR.pool_fwd(fu, LR.fill_padding(LR.rnd((N, T, G), 23), lq, other, seed), lq, idx=img)
        res += [gw, gp, *LR.pool_bwd(LR.rnd((N, G * C), 24), None, fu, gw, lq, idx=img, U=3)]
        got.append(res)
    for a, b in zip(*got):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b)
    dfeat_u = got[0][-1]
    assert bool((dfeat_u[0, 3:] == 0).all()) and bool((dfeat_u[2, 1:] == 0).all()) and float(dfeat_u[1].abs().max()) > 0


@pytest.mark.parametrize("N,T,E,lens", LR.PHRASE_CASES)
def test_phrase_winner_exclusion_cap(N, T, E, lens):
    """the GPU test compares idx where the fp64 top two differ by more than IDX_GAP: with the seeds of phrase_inputs that leaves
    out at most IDX_CAP of the real elements (none at these sizes), by the reference alone"""
    Z, bias, _ = LR.phrase_inputs(N, T, E)
    valid = MR.valid_mask(torch.tensor(lens), T)
    clear = LR.phrase_fwd(LR.fill_padding(Z, lens, 50.0), bias, lens)[2]
    real = int(valid.sum()) * E
    excluded = int((~clear[valid]).sum())
    assert excluded <= LR.IDX_CAP * real, (excluded, real)
    assert bool(clear[~valid].all())

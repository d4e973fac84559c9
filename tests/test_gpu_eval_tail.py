"""The evaluation tail on the MI355X: vqf_ce_loss_pred (loss + prediction + hit count in the loss kernel's row pass),
vqf_answer_match_rows (the soft-target models), vqf_topk_rows, and the host layer over them (loss_and_accuracy, Evaluator,
predict).  References are plain torch on the CPU, in integers or fp64.

Shapes (N, A): fewer columns than the 256 threads of a row's workgroup, exactly one stride, one past it, an odd width whose
rows are not 16-byte aligned, and the real answer count.  The top-k list adds W = 16384: the only width whose LDS request
(the row plus the reduction words) exceeds the 64 KB default.

Tolerances.  Predictions, counts and copied values are exact.  loss / dlogits are compared BIT for bit (int32 views, so that a
NaN loss compares too).  Top-k probabilities: 1e-4 relative to an fp64 softmax, the project's forward tolerance.  Double sums of
fp32 row values against the same rows in another order: 1e-6 relative.  loss sums against an fp64 cross entropy: 5e-6 relative --
an fp32 row loss lse - x[t] at |x| <= 4, A <= 5000 carries the rounding of lse (|lse| < 16: half an ulp = 4.8e-7), of the
subtraction (the same) and of expf / logf / the fp32 sum of exponentials (< 1e-6 on se, so < 1e-6 absolute on its log): under
3e-6 absolute on row losses that average above 2, and the rows' errors do not all point one way."""
import ctypes

import pytest
import torch

from cases import MFB_CASES
from golden_util import mfb_inputs
import recipe

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (3, 7), (5, 256), (4, 257), (6, 1003), (2, 5000)]


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _perm_rows(N, A, seed, lo=-4.0, hi=4.0):
    """(N, A) fp32 on the CPU, every row a random permutation of A distinct values in [lo, hi)"""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randperm(A, generator=g).double() / A * (hi - lo) + lo for _ in range(N)]
    x = torch.stack(rows).float()
    assert all(len(set(r.tolist())) == A for r in x)
    return x


def _targets(N, A, seed):
    return torch.randint(0, A, (N,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def _ce64(x, t):
    """per-row fp64 cross entropy of the rows with 0 <= t < A (others: NaN)"""
    x = x.double()
    ok = (t >= 0) & (t < x.shape[1])
    lse = torch.logsumexp(x, dim=1)
    out = torch.full((x.shape[0],), float("nan"), dtype=torch.float64)
    out[ok] = lse[ok] - x[ok].gather(1, t[ok].unsqueeze(1)).squeeze(1)
    return out


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,A", SHAPES)
@pytest.mark.parametrize("ignore", [False, True])
def test_loss_and_gradient_bits_are_vqf_ce_loss(vqa, N, A, ignore):
    ops = vqa.ops
    x = _perm_rows(N, A, 10 + A).to(DEV)
    t = _targets(N, A, 20 + A)
    if ignore:
        t[::3] = -100            # (1, 1): the only row is ignored, the loss is 0 / 0
    t = t.to(DEV)
    loss0, d0 = ops.ce_loss(x, t, want_grad=True)
    loss1, d1, pred = ops.ce_loss_pred(x, t, want_grad=True)
    assert _same_bits(loss0, loss1) and _same_bits(d0, d1)
    assert torch.equal(pred.cpu(), torch.argmax(x.cpu(), dim=1))
    loss2, d2, _ = ops.ce_loss_pred(x, t, want_grad=False)            # dlogits NULL
    assert d2 is None and _same_bits(loss0, loss2)
    loss3, _ = ops.ce_loss(x, t, want_grad=False)
    assert _same_bits(loss3, loss2)


# ---- 2. prediction, tie-free --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,A", SHAPES)
def test_prediction_is_argmax(vqa, N, A):
    x = _perm_rows(N, A, 30 + A)
    _, _, pred = vqa.ops.ce_loss_pred(x.to(DEV), _targets(N, A, 1).to(DEV), want_grad=False)
    assert pred.dtype == torch.int64 and torch.equal(pred.cpu(), torch.argmax(x, dim=1))
    # the maximum planted at the ends of the row, around the first stride boundary and at both ends of the last partial stride
    last_stride = ((A - 1) // 256) * 256
    spots = sorted({p for p in (0, A - 1, 255, 256, last_stride) if 0 <= p < A})
    y = _perm_rows(len(spots), A, 40 + A)
    for r, p in enumerate(spots):
        y[r, p] = 10.0
    _, _, pred = vqa.ops.ce_loss_pred(y.to(DEV), _targets(len(spots), A, 2).to(DEV), want_grad=False)
    assert pred.tolist() == spots


# ---- 3. ties, NaN, -inf -------------------------------------------------------------------------------------------------------
def test_ties_nan_and_infinities(vqa):
    A = 1003
    inf, nan = float("inf"), float("nan")
    rows, want = [], []

    def add(row, w):
        rows.append(row)
        want.append(w)

    r = _perm_rows(1, A, 50)[0]; r[5] = r[300] = 9.0; add(r, 5)                  # different waves and strides
    r = _perm_rows(1, A, 51)[0]; r[64] = r[65] = 9.0; add(r, 64)                 # adjacent waves
    r = _perm_rows(1, A, 52)[0]; r[63] = r[64] = 9.0; add(r, 63)
    add(torch.full((A,), 1.25), 0)                                               # all equal
    add(torch.zeros(A), 0)
    r = torch.zeros(A); r[0] = -0.0; r[1] = 0.0; add(r, 0)                       # -0 == +0
    r = _perm_rows(1, A, 53)[0]; r[7] = r[900] = nan; add(r, 7)                  # NaN: the lowest index holding one
    r = _perm_rows(1, A, 54)[0]; r[3] = inf; r[900] = nan; add(r, 900)           # NaN above +inf
    r = _perm_rows(1, A, 55)[0]; r[3] = r[700] = inf; add(r, 3)
    r = torch.full((A,), -inf); r[400] = -2.0; r[401] = -1.0; r[999] = -1.0; add(r, 401)      # finite values plus -inf
    add(torch.full((A,), -inf), 0)                                               # -inf is an ordinary value
    r = _perm_rows(1, A, 56)[0]; r[10] = -inf; add(r, int(torch.argmax(r)))
    x = torch.stack(rows)
    _, _, pred = vqa.ops.ce_loss_pred(x.to(DEV), _targets(len(rows), A, 3).to(DEV), want_grad=False)
    assert pred.tolist() == want
    # the soft-target kernel applies the same order to both of its rows
    p2, t2, _ = vqa.ops.answer_match_rows(x.to(DEV), x.flip(0).contiguous().to(DEV))
    assert p2.tolist() == want and t2.tolist() == want[::-1]


# ---- 4. counts and sums -------------------------------------------------------------------------------------------------------
def _count_case(N, A, seed, out_of_range):
    x = _perm_rows(N, A, seed)
    am = torch.argmax(x, dim=1)
    t = _targets(N, A, seed + 1)
    t[1::2] = am[1::2]                      # every other row is a hit
    t[2] = -100
    t[5] = -100                             # an ignored row that would have been a hit
    if out_of_range:
        t[4] = A + 3
        t[7] = -5
    return x, t, am


@pytest.mark.parametrize("A", [7, 257, 1003])
def test_counts_and_loss_sum(vqa, A):
    ops, N = vqa.ops, 11
    for oor in (False, True):
        x, t, am = _count_case(N, A, 60 + A, oor)
        live = t != -100
        hits = int(((am == t) & live).sum())
        rows = int(live.sum())
        counts = torch.full((2,), 77, dtype=torch.int64, device=DEV)          # accumulate = 0 overwrites
        lsum = torch.full((1,), 77.0, dtype=torch.float64, device=DEV)
        acc = torch.full((1,), 77.0, dtype=torch.float32, device=DEV)
        loss, _, pred = ops.ce_loss_pred(x.to(DEV), t.to(DEV), want_grad=False, counts=counts, loss_sum=lsum, acc=acc)
        assert torch.equal(pred.cpu(), am)
        assert counts.tolist() == [hits, rows]
        assert acc.item() == (torch.tensor(float(hits)) / torch.tensor(float(rows))).item()
        ref = _ce64(x, t)[live]
        if oor:                                                               # loss NaN, never a hit
            assert torch.isnan(loss).all() and torch.isnan(lsum).all() and torch.isnan(ref).any()
        else:
            rel = abs(lsum.item() - ref.sum().item()) / ref.sum().item()
            print("A=%d loss_sum %.9f fp64 %.9f rel %.2e" % (A, lsum.item(), ref.sum().item(), rel))
            assert rel <= 5e-6
            assert abs(loss.item() - ref.mean().item()) <= 5e-6 * ref.mean().item()
    # no counted row: the accuracy of nothing is NaN
    t0 = torch.full((3,), -100, dtype=torch.int64, device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    acc = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.ce_loss_pred(_perm_rows(3, A, 1).to(DEV), t0, want_grad=False, counts=counts, acc=acc)
    assert counts.tolist() == [0, 0] and torch.isnan(acc).all()


def test_accumulated_split_batch_equals_the_whole(vqa):
    ops, N, A = vqa.ops, 11, 257
    x, t, _ = _count_case(N, A, 70, False)
    xg, tg = x.to(DEV), t.to(DEV)
    whole_c = torch.zeros(2, dtype=torch.int64, device=DEV)
    whole_s = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.ce_loss_pred(xg, tg, want_grad=False, counts=whole_c, loss_sum=whole_s)
    c = torch.zeros(2, dtype=torch.int64, device=DEV)
    s = torch.zeros(1, dtype=torch.float64, device=DEV)
    for lo, hi in ((0, 4), (4, 8), (8, 11)):
        ops.ce_loss_pred(xg[lo:hi], tg[lo:hi], want_grad=False, counts=c, loss_sum=s, accumulate=True)
    assert c.tolist() == whole_c.tolist()
    rel = abs(s.item() - whole_s.item()) / abs(whole_s.item())
    print("split %.12f whole %.12f rel %.2e" % (s.item(), whole_s.item(), rel))
    assert rel <= 1e-6


# ---- 5. soft targets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,A", SHAPES)
def test_answer_match_rows(vqa, N, A):
    ops = vqa.ops
    logp = torch.log_softmax(_perm_rows(N, A, 80 + A), dim=1)
    tgt = _perm_rows(N, A, 90 + A, 0.0, 1.0)
    if N > 1:
        tgt[1] = 0.0
        tgt[1, int(torch.argmax(logp[1]))] = 1.0               # a certain hit
    if A > 250 and N > 2:
        tgt[2, 3] = tgt[2, 200] = 2.0                           # two equal largest entries: the lower index
    counts = torch.full((2,), 77, dtype=torch.int64, device=DEV)
    ssum = torch.full((1,), 77.0, dtype=torch.float64, device=DEV)
    lsum = torch.full((1,), 77.0, dtype=torch.float64, device=DEV)
    acc = torch.full((1,), 77.0, dtype=torch.float32, device=DEV)
    loss, _ = ops.kldiv_loss(logp.to(DEV), tgt.to(DEV), want_grad=False)
    pred, tpred, score = ops.answer_match_rows(logp.to(DEV), tgt.to(DEV), counts=counts, score_sum=ssum, loss=loss,
                                               loss_sum=lsum, acc=acc)
    rp, rt = torch.argmax(logp, dim=1), torch.argmax(tgt, dim=1)
    if A > 250 and N > 2:
        assert rt[2] == 3
    assert torch.equal(pred.cpu(), rp) and torch.equal(tpred.cpu(), rt)
    assert torch.equal(score.cpu(), tgt.gather(1, rp.unsqueeze(1)).squeeze(1))
    hits = int((rp == rt).sum())
    assert counts.tolist() == [hits, N] and (N == 1 or hits >= 1)
    assert acc.item() == (torch.tensor(float(hits)) / torch.tensor(float(N))).item()
    want_s = score.cpu().double().sum().item()
    assert abs(ssum.item() - want_s) <= 1e-12 * max(abs(want_s), 1.0)
    want_l = N * float(loss.item())
    assert abs(lsum.item() - want_l) <= 1e-12 * max(abs(want_l), 1.0)
    # accumulate adds; score may be left out
    p2, t2, s2 = ops.answer_match_rows(logp.to(DEV), tgt.to(DEV), want_score=False, counts=counts, score_sum=ssum,
                                       accumulate=True)
    assert s2 is None and torch.equal(p2, pred) and torch.equal(t2, tpred)
    assert counts.tolist() == [2 * hits, 2 * N] and abs(ssum.item() - 2 * want_s) <= 1e-12 * max(abs(want_s), 1.0)


# ---- 6. top-k -----------------------------------------------------------------------------------------------------------------
TOPK = [(3, 7, 1), (3, 7, 5), (3, 7, 7), (5, 256, 1), (5, 256, 16), (4, 257, 5), (6, 1003, 5), (6, 1003, 16), (2, 5000, 1),
        (2, 5000, 5), (2, 5000, 16), (2, 16384, 16), (1, 1, 1)]


@pytest.mark.parametrize("R,W,k", TOPK)
def test_topk_rows_tie_free(vqa, R, W, k):
    x = _perm_rows(R, W, 100 + W)
    want = torch.topk(x, k, dim=1)
    idx0, val0 = vqa.ops.topk_rows(x.to(DEV), k, mode=0)
    assert idx0.dtype == torch.int64 and idx0.shape == (R, k)
    assert torch.equal(idx0.cpu(), want.indices) and torch.equal(val0.cpu(), want.values)
    idx1, val1 = vqa.ops.topk_rows(x.to(DEV), k, mode=1)
    assert torch.equal(idx1.cpu(), want.indices)
    ref = torch.softmax(x.double(), dim=1).gather(1, want.indices)
    ratio = ((val1.cpu().double() - ref).abs() / ref).max().item()
    print("topk R=%d W=%d k=%d: worst relative error of the probabilities %.2e" % (R, W, k, ratio))
    assert ratio <= 1e-4


def test_topk_ties_nan_inf_and_strided_rows(vqa):
    ops = vqa.ops
    inf, nan = float("inf"), float("nan")
    W = 1003
    x = _perm_rows(4, W, 110)
    x[0, 700] = x[0, 9] = x[0, 300] = 9.0                       # three equal largest: ascending indices
    x[1, 2] = inf; x[1, 5] = nan; x[1, 1] = nan                  # NaN above +inf, the lower NaN first
    x[2] = 0.5                                                   # all equal: 0, 1, 2, ...
    x[3] = -inf; x[3, 600] = 1.0; x[3, 20] = -inf                # -inf entries rank like any value, in index order
    idx, val = ops.topk_rows(x.to(DEV), 4, mode=0)
    assert idx[0, :3].tolist() == [9, 300, 700] and idx[0, 3].item() == int(torch.topk(x[0], 4).indices[3])
    assert idx[1, :3].tolist() == [1, 5, 2] and torch.isnan(val[1, :2]).all() and val[1, 2].item() == inf
    assert idx[2].tolist() == [0, 1, 2, 3] and val[2].tolist() == [0.5] * 4
    assert idx[3].tolist() == [600, 0, 1, 2] and val[3].tolist() == [1.0, -inf, -inf, -inf]
    # a small row with k == W: a full descending sort, equal values in index order
    s = torch.tensor([[1.0, -inf, 3.0, 1.0, -inf, 2.0, 3.0]])
    idx, val = ops.topk_rows(s.to(DEV), 7, mode=0)
    assert idx[0].tolist() == [2, 6, 5, 0, 3, 1, 4] and val[0].tolist() == [3.0, 3.0, 2.0, 1.0, 1.0, -inf, -inf]
    # strided rows (ldx > W): a column slice whose rows start on and off 16-byte boundaries
    big = _perm_rows(4, 301, 111).to(DEV)                        # an odd row pitch: the rows' alignment alternates
    for c0, c1 in ((10, 267), (8, 265), (0, 256)):
        view = big[:, c0:c1]
        assert not view.is_contiguous()
        idx, val = ops.topk_rows(view, 5, mode=0)
        want = torch.topk(view.cpu(), 5, dim=1)
        assert torch.equal(idx.cpu(), want.indices) and torch.equal(val.cpu(), want.values)
        idx1, val1 = ops.topk_rows(view, 5, mode=1)
        ref = torch.softmax(view.cpu().double(), dim=1).gather(1, want.indices)
        assert torch.equal(idx1.cpu(), want.indices) and ((val1.cpu().double() - ref).abs() / ref).max().item() <= 1e-4


def test_topk_unsupported_width_launches_nothing(vqa):
    lib = vqa.lib.load()
    W = 16385
    assert lib.vqf_topk_rows_supported(W, 1) == 0 and lib.vqf_topk_rows_supported(W - 1, 1) == 1      # VQF_TOPK_MAX_W
    x = torch.zeros(2, W, device=DEV)
    idx = torch.full((2, 1), -7, dtype=torch.int64, device=DEV)
    val = torch.full((2, 1), -7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.vqf_topk_rows(p(x), 2, W, W, 1, 0, p(idx), p(val), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -3 and (idx == -7).all() and (val == -7.0).all()
    with pytest.raises(vqa.VqfError):
        vqa.ops.topk_rows(x, 1)
    with pytest.raises(vqa.VqfError):
        vqa.topk_answers(torch.zeros(2, 100, device=DEV), 17)


# ---- 7. host ------------------------------------------------------------------------------------------------------------------
def _host_case(soft):
    N, A = 11, 257
    x = _perm_rows(N, A, 120)
    if soft:
        a = torch.softmax(_perm_rows(N, A, 121), dim=1)
        a[1::2] = 0.0
        a[1::2].scatter_(1, torch.argmax(x[1::2], dim=1, keepdim=True), 1.0)
        hard = torch.argmax(a, dim=1)
    else:
        a = _targets(N, A, 122)
        a[1::2] = torch.argmax(x[1::2], dim=1)
        hard = a
    return x, a, hard


@pytest.mark.parametrize("soft", [False, True])
def test_loss_and_accuracy(vqa, soft):
    x, a, hard = _host_case(soft)
    crit = vqa.KLDivLoss() if soft else vqa.CrossEntropyLoss()
    head = (lambda z: torch.log_softmax(z, dim=1)) if soft else (lambda z: z)
    x1 = x.to(DEV).requires_grad_(True)
    l1 = crit(head(x1), a.to(DEV))
    (l1 * 1.5).backward()
    x2 = x.to(DEV).requires_grad_(True)
    l2, pred, acc = vqa.loss_and_accuracy(crit, head(x2), a.to(DEV))
    assert l2.shape == () and l2.requires_grad and not pred.requires_grad and not acc.requires_grad
    (l2 * 1.5).backward()
    assert _same_bits(l1.detach(), l2.detach()) and _same_bits(x1.grad, x2.grad)
    assert pred.dtype == torch.int64 and torch.equal(pred.cpu(), torch.argmax(x, dim=1))
    want = (pred == hard.to(DEV)).float().mean()
    assert acc.shape == () and acc.dtype == torch.float32 and acc.is_cuda and acc.item() == want.item()
    assert 0.4 < acc.item() < 1.0
    # without a graph (validation): same values
    with torch.no_grad():
        l3, p3, a3 = vqa.loss_and_accuracy(crit, head(x.to(DEV)), a.to(DEV))
    assert _same_bits(l3, l2.detach()) and torch.equal(p3, pred) and a3.item() == acc.item()


@pytest.mark.parametrize("soft", [False, True])
def test_evaluator_over_three_batches(vqa, soft):
    x, a, hard = _host_case(soft)
    crit = vqa.KLDivLoss() if soft else vqa.CrossEntropyLoss()
    out = torch.log_softmax(x, dim=1) if soft else x
    pred = torch.argmax(out, dim=1)
    N = x.shape[0]
    correct = int((pred == hard).sum())
    if soft:
        t64 = a.double()
        elem = torch.where(t64 > 0, t64 * (t64.clamp_min(1e-300).log() - out.double()), torch.zeros_like(t64))
        loss_mean = elem.mean().item()                         # every batch has the same A: the row-weighted mean of batch means
        score = a.gather(1, pred.unsqueeze(1)).double().mean().item()
    else:
        loss_mean = _ce64(x, a).mean().item()
    ev = vqa.Evaluator(crit)
    assert ev.result()["rows"] == 0
    og, ag = out.to(DEV), a.to(DEV)
    runs = []
    for _ in range(2):
        for lo, hi in ((0, 4), (4, 8), (8, 11)):
            assert ev.update(og[lo:hi], ag[lo:hi]) is None
        runs.append(ev.result())
        ev.reset()
    r = runs[0]
    print(r)
    assert runs[1] == r                                        # after reset(): the same totals again
    assert r["correct"] == correct and r["rows"] == N and r["accuracy"] == correct / N
    # (KL: fp32 elements t * (log t - logp) with |log| < 16, i.e. under 1e-6 * t absolute each, summed over rows whose t sum to 1,
    #  against per-row divergences of several nats: the bound of the cross-entropy sums covers it)
    assert abs(r["loss_mean"] - loss_mean) <= 5e-6 * abs(loss_mean)
    with torch.no_grad():
        last = crit(og[8:11], ag[8:11]).item()
    assert r["loss_last"] == last
    if soft:
        assert abs(r["vqa_score"] - score) <= 1e-12 * max(score, 1.0)
    else:
        assert "vqa_score" not in r
    assert ev.result()["rows"] == 0 and ev.result()["correct"] == 0


# ---- 8. predict ---------------------------------------------------------------------------------------------------------------
def _check_predict(vqa, model, args, kwargs, k=5):
    model.train()
    ids, probs = vqa.predict(model, *args, k=k, **kwargs)
    assert model.training                                       # the flag is restored
    ids2, probs2 = vqa.predict(model, *args, k=k, **kwargs)
    assert torch.equal(ids, ids2) and _same_bits(probs, probs2)   # dropout is off inside predict
    model.eval()
    with torch.no_grad():
        out = model(*args, **kwargs)
    out = out[0] if isinstance(out, (tuple, list)) else out
    N = out.shape[0]
    assert ids.shape == (N, k) and ids.dtype == torch.int64 and probs.shape == (N, k) and probs.dtype == torch.float32
    assert torch.equal(ids[:, 0], torch.argmax(out, dim=1))
    ref = torch.softmax(out.double().cpu(), dim=1).gather(1, ids.cpu())
    assert ((probs.cpu().double() - ref).abs() / ref).max().item() <= 1e-4
    assert (probs.sum(dim=1) <= 1 + 1e-4).all() and (probs[:, :-1] >= probs[:, 1:]).all() and (probs > 0).all()
    ids3, _ = vqa.predict(model, *args, k=k, **kwargs)
    assert not model.training and torch.equal(ids3, ids)
    # callers that already hold logits
    ids4, probs4 = vqa.topk_answers(out, k)
    assert torch.equal(ids4, ids) and _same_bits(probs4, probs)


def test_predict_mfb(vqa):
    case = MFB_CASES[2]                                         # small_n3
    cfg, img, q, _, _, _ = mfb_inputs(case, DEV)
    model = vqa.MFB(cfg)
    model.load_state_dict({k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"]))
                           for k, v in model.state_dict().items()})
    _check_predict(vqa, model.to(DEV), (img, q), {})


def test_predict_hie_ladder_with_lengths(vqa):
    N, T, L, E, D = 3, 5, 50, 64, 96                            # the smallest configuration of tests/test_gpu_hie_ladder_lengths.py
    torch.manual_seed(0)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=40, embed_size=E, hidden_size=48, output_size=30, drop_p=0.5)
    g = torch.Generator().manual_seed(100)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    g = torch.Generator().manual_seed(0)
    img = torch.rand(N, L, D, generator=g)
    ids = torch.randint(1, 40, (N, T), generator=g)
    lens = torch.tensor([2, 1, T], dtype=torch.int64)
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens.unsqueeze(1), ids, torch.zeros_like(ids))
    _check_predict(vqa, m.to(DEV), (img.to(DEV), ids.to(DEV)), {"q_length": lens.to(DEV)})

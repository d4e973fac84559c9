"""BCE-with-logits on soft answers, on the MI355X (vqf_bce_loss, vqf_bce_loss_sparse, ops.bce_logits_loss, BCEWithLogitsLoss,
loss_and_accuracy, Evaluator): loss and gradient against the fp64 reference of soft_loss_ref.py within the bounds derived there
(roundings counted from the kernel's code, not measured), prediction and score exactly; a SoftAnswers is the call on its
.dense(A) -- with distinct ids the dense call's gradient bits --; empty slots touch nothing; ties, NaN rows and +-1e4 logits;
device totals with `accumulate`; the autograd route gives the bits of a backward seeded with the kernel's gradient.

_compare prints the measured error / bound ratio of every case (pytest -s): profiles/soft_loss_parity.txt keeps them."""
import ctypes

import pytest
import torch

import recipe
import soft_loss_ref as R
from cases import MFB_CASES
from golden_util import mfb_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (1, 3, 11)
WIDTHS = (1, 3, 255, 257, 1003, 3000)      # one element, below the 256 threads, one short of / one past them, odd, the ladder's default
SLOTS = (1, 10, 16)
REDUCTIONS = ("mean", "batchmean")


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


def _dense_target(N, A, seed):
    """soft scores in [0, 1], most of them 0, like the annotators' (N, A) target"""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(N, A, generator=g)
    return torch.where(torch.rand(N, A, generator=g) < 0.2, t, torch.zeros_like(t)).contiguous()


def _with_hits(ids, x):
    """distinct ids in, distinct ids out: every even row gets its arg-max answer into a slot and (where A > K) every odd row
    loses it, so that some predictions score and some do not"""
    ids = ids.clone()
    K, A = ids.shape[1], x.shape[1]
    for n in range(ids.shape[0]):
        p = int(torch.argmax(x[n]))
        at = (ids[n] == p).nonzero()
        if n % 2 == 0 and at.numel() == 0:
            ids[n, K // 2] = p
        elif n % 2 == 1 and at.numel() and A > K:
            ids[n, int(at[0])] = next(a for a in range(A) if a != p and a not in ids[n].tolist())
    return ids


def _call(vqa, x, target, c, **kw):
    """ops.bce_logits_loss on the GPU -> (loss, dlogits, pred, score) as CPU tensors"""
    tgt = target.to(DEV)
    out = vqa.ops.bce_logits_loss(x.to(DEV), tgt, c, **kw)
    return [o.cpu() if o is not None else None for o in out]


def _compare(tag, out, ref, target, N, A, c, K=0, repeats=1):
    """the four outputs against the fp64 reference; prints and returns the worst error / bound ratios (loss, gradient).
    K: the slots per row of a sparse target (0: dense); repeats: the most slots of a row that may share an id"""
    loss, d, pred, score = out
    lr = abs(float(loss.double()) - float(ref["loss"])) / R.loss_bound(ref, N, A, c, K)
    gr = float(((d.double() - ref["grad"]).abs() / R.grad_bound(ref, target, c, repeats)).max())
    print("soft_loss_parity %-34s N=%-2d A=%-4d loss err/bound %.3f  grad err/bound %.3f" % (tag, N, A, lr, gr))
    assert lr <= 1.0 and gr <= 1.0, (tag, N, A, lr, gr)
    assert torch.equal(pred, ref["pred"]), (tag, N, A)
    serr = (score.double() - ref["score"].double()).abs()             # exact unless an id repeats (bound 0 then)
    assert bool((serr <= R.score_bound(ref, repeats)).all()), (tag, N, A, float(serr.max()))
    return lr, gr


@pytest.mark.parametrize("A", WIDTHS)
def test_dense_and_sparse_against_fp64(vqa, A):
    for N in NS:
        x = R.perm_rows(N, A, 8.0, seed=N * 7 + A)
        t = _dense_target(N, A, seed=N + A)
        for red in REDUCTIONS:
            c = R.scale_of(red, N, A)
            ref = R.reference(x, t, c)
            out = _call(vqa, x, t, c)
            _compare("dense %s" % red, out, ref, t, N, A, c)
            assert _same_bits(out[3], ref["score"])                       # score = target[n, pred[n]], a copy
        for K in SLOTS:
            distinct = K <= A
            ids, sc = R.soft_slots(N, A, K, seed=K + N + A, distinct=distinct)
            if distinct:
                ids = _with_hits(ids, x)
            soft = vqa.SoftAnswers(ids if K != 10 else ids.to(torch.int32), sc)
            td = soft.dense(A)
            for red in REDUCTIONS:
                c = R.scale_of(red, N, A)
                ref = R.reference(x, td, c)
                out = _call(vqa, x, soft, c)
                _compare("sparse K=%d%s %s" % (K, "" if distinct else " repeats", red), out, ref, td, N, A, c, K,
                         repeats=1 if distinct else K)
                if distinct:
                    dense = _call(vqa, x, td, c)
                    assert _same_bits(out[1], dense[1]), ("gradient bits", N, A, K)
                    hit = ids == ref["pred"].unsqueeze(1)
                    want = torch.where(hit, sc, torch.zeros_like(sc)).sum(1)      # one slot at most: that slot's score, or exactly 0
                    assert _same_bits(out[3], want) and _same_bits(out[3], dense[3])
                    if N >= 3 and A > K:
                        assert float(want[0]) > 0 and float(want[1]) == 0


def _raw_sparse(vqa, x, ids, sc, c, guard=64):
    """vqf_bce_loss_sparse straight through the C ABI with guard values around dlogits and pred"""
    lib = vqa.lib.load()
    N, A = x.shape
    xg, ig, sg = x.to(DEV), ids.to(DEV).contiguous(), sc.to(DEV).contiguous()
    dbuf = torch.full((N * A + 2 * guard,), 777.0, dtype=torch.float32, device=DEV)
    pbuf = torch.full((N + 2 * guard,), -555, dtype=torch.int64, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    score = torch.empty(N, dtype=torch.float32, device=DEV)
    nb = int(lib.vqf_bce_loss_ws_bytes(N))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = lib.vqf_bce_loss_sparse(p(xg), p(ig), 1 if ig.dtype == torch.int64 else 0, p(sg), ids.shape[1], N, A, c, p(loss),
                                 p(dbuf, 4 * guard), p(pbuf, 8 * guard), p(score), None, None, None, None, 0, p(ws), nb,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    d, pr = dbuf.cpu(), pbuf.cpu()
    assert bool((d[:guard] == 777.0).all()) and bool((d[guard + N * A:] == 777.0).all()), "guard around dlogits"
    assert bool((pr[:guard] == -555).all()) and bool((pr[guard + N:] == -555).all()), "guard around pred"
    return loss.cpu(), d[guard:guard + N * A].view(N, A), pr[guard:guard + N], score.cpu()


@pytest.mark.parametrize("A", [3, 257, 1003])
def test_slot_semantics(vqa, A):
    N, K = 3, 10
    x = R.perm_rows(N, A, 8.0, seed=A)
    c = R.scale_of("mean", N, A)
    zero = torch.zeros(N, A)
    ref0 = R.reference(x, zero, c)
    base = _call(vqa, x, zero, c)
    nan = float("nan")
    # empty slots only: ids of -1 mixed with ids >= A (far past the row and the tensor), NaN scores in them
    ids = torch.tensor([-1, A, -7, A + 1, -(2 ** 31), 2 ** 31 - 1, N * A, N * A + 5, -2, A + 100]).repeat(N, 1)
    sc = torch.full((N, K), nan)
    for dt in (torch.int64, torch.int32):
        out = _raw_sparse(vqa, x, ids.to(dt), sc, c)
        assert _same_bits(out[1], base[1]) and _same_bits(out[0], base[0]), "the all-zero target's bits"
        assert torch.equal(out[2], ref0["pred"]) and bool((out[3] == 0).all()) and not bool(torch.isnan(out[1]).any())
    big = torch.tensor([2 ** 40 + 1, -(2 ** 40), 2 ** 32, 2 ** 32 + 2] + [-1] * (K - 4)).repeat(N, 1)      # int64 ids whose low word is a valid column
    out = _raw_sparse(vqa, x, big, sc, c)
    assert _same_bits(out[1], base[1]) and _same_bits(out[0], base[0])
    # live slots between empty ones, one id repeated three times: within the bounds of the fp64 reference on .dense(A)
    ids2, sc2 = R.soft_slots(N, A, K, seed=A + 1, distinct=False)
    ids2[:, 1], ids2[:, 4], ids2[:, 7] = -1, A, ids2[:, 0]
    ids2[:, 9] = ids2[:, 0]
    sc2[:, 1], sc2[:, 4] = nan, nan
    soft = vqa.SoftAnswers(ids2, sc2)
    td = soft.dense(A)
    assert not bool(torch.isnan(td).any())
    out = _raw_sparse(vqa, x, ids2, sc2, c)
    _compare("slots: empty + repeated id", out, R.reference(x, td, c), td, N, A, c, K, repeats=K)


def test_ties_nan_and_large_magnitudes(vqa):
    N, A = 3, 1003
    x = R.perm_rows(N, A, 8.0, seed=1)
    x[0, 700], x[0, 41], x[0, 999] = 9.0, 9.0, 9.0                   # equal maxima: the lowest index
    x[1, 600], x[1, 12] = float("nan"), float("nan")                  # a NaN row: its first NaN, and a NaN loss
    x[1, 3] = float("inf")
    t = _dense_target(N, A, seed=2)
    ids, sc = R.soft_slots(N, A, 10, seed=3)
    for target in (t, vqa.SoftAnswers(ids, sc)):
        loss, d, pred, score = _call(vqa, x, target, R.scale_of("batchmean", N, A))
        assert pred.tolist()[:2] == [41, 12] and int(pred[2]) == int(torch.argmax(x[2]))
        assert bool(torch.isnan(loss).all())
        assert not bool(torch.isnan(d[0]).any()) and not bool(torch.isnan(d[2]).any())
    # +-1e4: exp(-|x|) underflows; everything stays finite and within the bounds
    for A2 in (257, 3000):
        xl = R.perm_rows(N, A2, 1e4, seed=A2)
        t2 = _dense_target(N, A2, seed=4)
        ids, sc = R.soft_slots(N, A2, 10, seed=5)
        soft = vqa.SoftAnswers(_with_hits(ids, xl), sc)
        for red in REDUCTIONS:
            c = R.scale_of(red, N, A2)
            for tag, target, td in (("dense", t2, t2), ("sparse K=10", soft, soft.dense(A2))):
                out = _call(vqa, xl, target, c)
                assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
                _compare("%s %s at +-1e4" % (tag, red), out, R.reference(xl, td, c), td, N, A2, c, 10 if target is soft else 0)


@pytest.mark.parametrize("sparse", [False, True])
def test_totals_and_accumulation(vqa, sparse):
    N, A = 11, 1003
    x = R.perm_rows(N, A, 8.0, seed=21)
    ids, sc = R.soft_slots(N, A, 10, seed=22)
    ids = _with_hits(ids, x)
    t = _dense_target(N, A, seed=23)
    part = (lambda a, b: vqa.SoftAnswers(ids[a:b], sc[a:b]).to(DEV)) if sparse else (lambda a, b: t[a:b].contiguous().to(DEV))
    td = vqa.SoftAnswers(ids, sc).dense(A) if sparse else t
    ref = R.reference(x, td, 1.0 / (N * A))
    xg = x.to(DEV)
    mk = lambda: (torch.full((1,), -9, dtype=torch.int64, device=DEV), torch.full((1,), -9.0, dtype=torch.float64, device=DEV),
                  torch.full((1,), -9.0, dtype=torch.float64, device=DEV), torch.full((1,), -9.0, device=DEV))

    def run(spans, bufs):
        outs = []
        for i, (a, b) in enumerate(spans):
            outs.append(vqa.ops.bce_logits_loss(xg[a:b].contiguous(), part(a, b), 1.0 / ((b - a) * A), rows=bufs[0],
                                                score_sum=bufs[1], loss_sum=bufs[2], acc=bufs[3], accumulate=i > 0))
        return outs

    one, split = mk(), mk()
    o1 = run([(0, N)], one)
    o3 = run([(0, 4), (4, 8), (8, 11)], split)
    assert int(one[0]) == N and int(split[0]) == N                   # accumulate = False overwrote the -9
    for a, b in ((one[1], split[1]), (one[2], split[2])):
        assert abs(float(a) - float(b)) <= 1e-12 * abs(float(a))
    assert abs(float(one[1]) - float(ref["score"].double().sum())) <= 1e-12 * float(one[1]) and float(one[1]) > 0
    assert abs(float(one[2]) - N * float(ref["loss"])) <= R.loss_bound(ref, N, A, 1.0 / (N * A), 10 if sparse else 0) * N
    assert float(one[3]) == float(torch.tensor(float(ref["score"].double().mean())).float())            # this call's mean score
    assert float(split[3]) == float(torch.tensor(float(ref["score"][8:].double().mean())).float())      # the LAST call's, not the total
    assert torch.equal(torch.cat([o[2] for o in o3]).cpu(), ref["pred"]) and torch.equal(o1[0][2].cpu(), ref["pred"])
    # a second identical call: the same bits everywhere
    again = mk()
    o2 = run([(0, N)], again)
    (l1, d1, p1, s1), (l2, d2, p2, s2) = o1[0], o2[0]
    assert _same_bits(l1, l2) and _same_bits(d1, d2) and torch.equal(p1, p2) and _same_bits(s1, s2)
    assert int(again[0]) == int(one[0]) and torch.equal(_bits(again[3]), _bits(one[3]))
    assert torch.equal(again[1].view(torch.int64), one[1].view(torch.int64))
    assert torch.equal(again[2].view(torch.int64), one[2].view(torch.int64))


def _old_criteria_results(vqa, seed=31):
    """one Evaluator run of each existing criterion -> their result dicts (compared before / after the new one is used)"""
    N, A = 5, 257
    x = R.perm_rows(N, A, 4.0, seed=seed).to(DEV)
    hard = torch.randint(0, A, (N,), generator=torch.Generator().manual_seed(seed)).to(DEV)
    softt = torch.softmax(R.perm_rows(N, A, 2.0, seed=seed + 1), 1).to(DEV)
    logp = torch.log_softmax(x, 1)
    res = []
    for crit, inp, tgt in ((vqa.CrossEntropyLoss(), x, hard), (vqa.KLDivLoss(), logp, softt)):
        ev = vqa.Evaluator(crit)
        ev.update(inp, tgt)
        ev.update(inp[:3].contiguous(), tgt[:3].contiguous())
        loss, pred, acc = vqa.loss_and_accuracy(crit, inp, tgt)
        res.append((ev.result(), float(loss), pred.tolist(), float(acc)))
    return res


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_loss_and_accuracy_and_evaluator(vqa, reduction):
    before = _old_criteria_results(vqa)
    assert set(before[0][0]) == {"correct", "rows", "accuracy", "loss_mean", "loss_last"}
    assert set(before[1][0]) == {"correct", "rows", "accuracy", "loss_mean", "loss_last", "vqa_score"}
    A = 1003
    crit = vqa.BCEWithLogitsLoss(reduction)
    for sparse in (False, True):
        ev = vqa.Evaluator(crit)
        score_sum, loss_sum, bound_sum, rows, last = 0.0, 0.0, 0.0, 0, None
        for b, N in enumerate((11, 3, 4)):
            x = R.perm_rows(N, A, 8.0, seed=40 + b)
            ids, sc = R.soft_slots(N, A, 10, seed=50 + b)
            soft = vqa.SoftAnswers(_with_hits(ids, x), sc)
            td = soft.dense(A) if sparse else _dense_target(N, A, seed=60 + b)
            target = soft.to(DEV) if sparse else td.to(DEV)
            c = R.scale_of(reduction, N, A)
            ref = R.reference(x, td, c)
            xg = x.to(DEV).requires_grad_(True)
            loss, pred, acc = vqa.loss_and_accuracy(crit, xg, target)
            loss.backward()
            x2 = x.to(DEV).requires_grad_(True)
            plain = crit(x2, target)
            plain.backward()
            assert _same_bits(loss.detach().view(1), plain.detach().view(1)) and _same_bits(xg.grad, x2.grad)
            assert not pred.requires_grad and not acc.requires_grad and torch.equal(pred.cpu(), ref["pred"])
            assert float(acc) == float(torch.tensor(float(ref["score"].double().mean())).float())
            assert abs(float(loss.detach()) - float(ref["loss"])) <= R.loss_bound(ref, N, A, c, 10 if sparse else 0)
            ev.update(xg.detach(), target)
            score_sum += float(ref["score"].double().sum())
            loss_sum += N * float(ref["loss"])
            bound_sum += N * R.loss_bound(ref, N, A, c, 10 if sparse else 0)
            rows += N
            last = float(loss.detach())
        r = ev.result()
        assert set(r) == {"rows", "vqa_score", "accuracy", "loss_mean", "loss_last"}
        assert r["rows"] == rows and r["accuracy"] == r["vqa_score"] and r["loss_last"] == last
        assert abs(r["vqa_score"] - score_sum / rows) <= 1e-12 * (score_sum / rows) and r["vqa_score"] > 0
        assert abs(r["loss_mean"] - loss_sum / rows) <= bound_sum / rows
        ev.reset()
        assert ev.result()["rows"] == 0
    after = _old_criteria_results(vqa)
    assert repr(before) == repr(after)


@pytest.mark.parametrize("view", ["slice", "transpose"])
def test_non_contiguous_logits_that_need_a_gradient(vqa, view):
    """a sliced or transposed logits view: the loss and the gradient bits of the call on a contiguous copy, through the
    criterion and through loss_and_accuracy, for a dense and a sparse target"""
    N, A = 3, 257
    x = R.perm_rows(N, A, 8.0, seed=71)
    ids, sc = R.soft_slots(N, A, 10, seed=72)
    soft = vqa.SoftAnswers(ids, sc).to(DEV)
    dense = _dense_target(N, A, seed=73).to(DEV)
    for red in REDUCTIONS:
        crit = vqa.BCEWithLogitsLoss(red)
        for target in (dense, soft):
            for route in (lambda z: crit(z, target), lambda z: vqa.loss_and_accuracy(crit, z, target)[0]):
                plain = x.to(DEV).requires_grad_(True)
                want = route(plain)
                want.backward()
                if view == "slice":
                    base = torch.cat([x, torch.full((N, 5), 50.0)], 1).to(DEV).requires_grad_(True)
                    z, pick = base[:, :A], (lambda g: g[:, :A])
                else:
                    base = x.t().contiguous().to(DEV).requires_grad_(True)
                    z, pick = base.t(), (lambda g: g.t())
                assert not z.is_contiguous() and z.requires_grad
                got = route(z)
                assert got.requires_grad and _same_bits(got.detach().view(1), want.detach().view(1))
                got.backward()
                assert _same_bits(pick(base.grad).contiguous(), plain.grad)
                if view == "slice":
                    assert bool((base.grad[:, A:] == 0).all())


def _grads(model):
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _two_routes(vqa, model, forward, soft, reduction):
    """criterion(logits, soft).backward() against an identical forward + logits.backward(d), d from ops.bce_logits_loss"""
    crit = vqa.BCEWithLogitsLoss(reduction)
    model.zero_grad()
    logits = forward()
    loss = crit(logits, soft)
    loss.backward()
    g1 = _grads(model)
    model.zero_grad()
    logits2 = forward()
    assert _same_bits(logits2.detach(), logits.detach())
    N, A = logits2.shape
    l2, d, _, _ = vqa.ops.bce_logits_loss(logits2.detach().contiguous(), soft, R.scale_of(reduction, N, A))
    logits2.backward(d)
    g2 = _grads(model)
    assert _same_bits(l2, loss.detach().view(1))
    assert len(g1) > 0 and set(g1) == set(g2) and all(_same_bits(g1[k], g2[k]) for k in g1), \
        [k for k in g1 if not _same_bits(g1[k], g2[k])]
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    opt = vqa.Adam(model.parameters(), lr=1e-3)
    opt.step()
    with torch.no_grad():
        after = crit(forward(), soft)
    assert bool(torch.isfinite(after)) and bool(torch.isfinite(loss.detach()))


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_autograd_plumbing_hie_ladder(vqa, reduction):
    N, T, L, E, D, O = 3, 5, 50, 64, 96, 30          # the smallest configuration of test_gpu_eval_tail.py's ladder case
    torch.manual_seed(0)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=40, embed_size=E, hidden_size=48, output_size=O, drop_p=0.5)
    g = torch.Generator().manual_seed(100)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    g = torch.Generator().manual_seed(0)
    img = torch.rand(N, L, D, generator=g)
    ids = torch.randint(1, 40, (N, T), generator=g)
    lens = torch.tensor([2, 1, T], dtype=torch.int64)
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens.unsqueeze(1), ids, torch.zeros_like(ids))
    counts = (L - 1, 1, L)
    packed = vqa.pack_region_features([img[n, :k].numpy() for n, k in enumerate(counts)]).to(DEV)
    assert packed.max_regions == L
    m = m.to(DEV).eval()
    idsg, lensg = ids.to(DEV), lens.to(DEV)
    aid, asc = R.soft_slots(N, O, 10, seed=7)
    soft = vqa.SoftAnswers(aid, asc).to(DEV)
    _two_routes(vqa, m, lambda: m(packed, idsg, lensg)[0], soft, reduction)


def test_autograd_plumbing_mfb(vqa):
    case = MFB_CASES[2]                                         # small_n3
    cfg, img, q, _, _, _ = mfb_inputs(case, DEV)
    model = vqa.MFB(cfg)
    model.load_state_dict({k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"]))
                           for k, v in model.state_dict().items()})
    model = model.to(DEV).eval()
    N, A = case["N"], cfg.a_vocab_size
    aid, asc = R.soft_slots(N, A, 10, seed=8)
    soft = vqa.SoftAnswers(aid, asc).to(DEV)
    _two_routes(vqa, model, lambda: model(img, q), soft, "mean")

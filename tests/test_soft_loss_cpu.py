"""CPU-side checks of BCE-with-logits on soft answers (vqf_bce_loss, vqf_bce_loss_sparse, SoftAnswers, soft_answers,
BCEWithLogitsLoss): the symbols are declared and bound, bad arguments are refused before any GPU call (NULL or dummy device
pointers: nothing can have been launched), the workspace query answers without a device, the host objects build and refuse
what they should, CPU tensors and torch criteria are refused, and the fp64 reference of soft_loss_ref.py is torch's criterion."""
import os
import re
import sys

import pytest
import torch

import soft_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, WORKSPACE = -1, -4
NEW = ("vqf_bce_loss_ws_bytes", "vqf_bce_loss", "vqf_bce_loss_sparse")


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def test_symbols_are_declared_and_bound(vqa):
    hdr = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    assert re.search(r"#define\s+VQF_SOFT_MAX_SLOTS\s+16\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = vqa.lib.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in vqa.lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.vqf_abi_version() == 7 and vqa.lib.ABI_VERSION == 7


def test_profiler_names_the_new_kernels(vqa):
    lib = vqa.lib.load()
    names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
    assert {"bce_loss", "bce_loss_sparse"} <= set(names) and len(set(names)) == len(names)


def test_workspace_query_needs_no_gpu(vqa):
    lib = vqa.lib.load()
    assert lib.vqf_bce_loss_ws_bytes(1) == 8 and lib.vqf_bce_loss_ws_bytes(512) == 8 * 512
    assert lib.vqf_bce_loss_ws_bytes(0) == 0 and lib.vqf_bce_loss_ws_bytes(-3) == 0


def _dense(lib, logits=1, target=1, N=4, A=7, loss=1, ws=1, ws_bytes=64):
    # non-NULL "pointers" are the address 16: never dereferenced when the call is refused
    p = lambda f: 16 if f else None
    return lib.vqf_bce_loss(p(logits), p(target), N, A, 0.25, p(loss), None, None, None, None, None, None, None, 0, p(ws),
                            ws_bytes, None)


def _sparse(lib, logits=1, ids=1, scores=1, K=10, N=4, A=7, loss=1, ws=1, ws_bytes=64, ids64=1):
    p = lambda f: 16 if f else None
    return lib.vqf_bce_loss_sparse(p(logits), p(ids), ids64, p(scores), K, N, A, 0.25, p(loss), None, None, None, None, None,
                                   None, None, 0, p(ws), ws_bytes, None)


def test_bad_arguments_are_refused_before_any_gpu_call(vqa):
    lib = vqa.lib.load()
    for kw in (dict(N=0), dict(N=-3), dict(A=0), dict(A=-1), dict(logits=0), dict(target=0), dict(loss=0), dict(ws=0)):
        assert _dense(lib, **kw) == BADARG, kw
    assert _dense(lib, ws_bytes=8 * 4 - 1) == WORKSPACE          # 8 bytes per row, the status of the other loss entry points
    for kw in (dict(N=0), dict(N=-3), dict(A=0), dict(K=0), dict(K=-1), dict(K=17), dict(logits=0), dict(ids=0), dict(scores=0),
               dict(loss=0), dict(ws=0), dict(K=17, ids64=0)):
        assert _sparse(lib, **kw) == BADARG, kw
    assert _sparse(lib, ws_bytes=8 * 4 - 1) == WORKSPACE


def test_soft_answers_builder(vqa):
    a = vqa.soft_answers([{"7": 1.0, "2": 0.3}, {}, {"11": 0.6}], slots=3)
    b = vqa.soft_answers([{7: 1.0, 2: 0.3}, {}, {11: 0.6}], slots=3)
    assert isinstance(a, vqa.SoftAnswers) and vqa.data_loader.soft_answers is vqa.soft_answers
    assert a.ids.dtype == torch.int64 and a.scores.dtype == torch.float32
    assert torch.equal(a.ids, b.ids) and torch.equal(a.scores, b.scores)
    assert a.ids.tolist() == [[7, 2, -1], [-1, -1, -1], [11, -1, -1]]
    assert torch.equal(a.scores, torch.tensor([[1.0, 0.3, 0.0], [0.0, 0.0, 0.0], [0.6, 0.0, 0.0]]))
    assert vqa.soft_answers([{1: 0.9}]).ids.shape == (1, 10)                 # the ten annotators' slots by default
    with pytest.raises(ValueError):
        vqa.soft_answers([])
    with pytest.raises(ValueError):
        vqa.soft_answers([{1: 0.3, 2: 0.3, 3: 0.3}], slots=2)
    for slots in (0, 17, -1):
        with pytest.raises(ValueError):
            vqa.soft_answers([{1: 0.3}], slots=slots)
    assert vqa.soft_answers([{k: 0.3 for k in range(16)}], slots=16).ids.shape == (1, 16)


def test_dense_of_soft_answers(vqa):
    S = vqa.SoftAnswers
    ids = torch.tensor([[4, 0, 2], [1, 1, 3], [-1, 2, -7], [5, 9, 1]])
    sc = torch.tensor([[0.3, 1.0, 0.6], [0.3, 0.6, 0.9], [float("nan"), 0.9, 0.3], [0.6, float("nan"), 1.0]])
    want = torch.zeros(4, 5)
    want[0, 4], want[0, 0], want[0, 2] = 0.3, 1.0, 0.6                       # distinct ids
    want[1, 1], want[1, 3] = torch.tensor(0.3) + torch.tensor(0.6), 0.9      # a repeated id: the scores add
    want[2, 2] = 0.9                                                         # negative ids: empty, their scores ignored
    want[3, 1] = 1.0                                                         # ids >= A: dropped
    for dt in (torch.int64, torch.int32):
        d = S(ids.to(dt), sc).dense(5)
        assert d.dtype == torch.float32 and d.shape == (4, 5) and torch.equal(d, want)
    moved = S(ids, sc).to("cpu")
    assert isinstance(moved, S) and torch.equal(moved.ids, ids)


def test_soft_answers_refusals(vqa):
    S, x = vqa.SoftAnswers, torch.zeros(2, 5)
    check = sys.modules[S.__module__].check_soft_answers
    bad = (S(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4)),                      # shapes differ
           S(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 0)),                      # K = 0
           S(torch.zeros(2, 17, dtype=torch.int64), torch.zeros(2, 17)),                    # K = 17
           S(torch.zeros(2, 3), torch.zeros(2, 3)),                                         # float ids
           S(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.float64)),  # scores not fp32
           S(torch.zeros(6, dtype=torch.int64), torch.zeros(6)))                            # not (N, K)
    for s in bad:
        with pytest.raises(vqa.VqfError):
            s.dense(5)
        with pytest.raises(vqa.VqfError):
            check("test", s, 2, x.device)
    ok = S(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3))
    check("test", ok, 2, x.device)
    with pytest.raises(vqa.VqfError):
        check("test", ok, 3, x.device)                  # rows != the logits' rows
    with pytest.raises(vqa.VqfError):
        check("test", ok, 2, torch.device("meta"))      # another device than the logits'


def test_criterion_reductions_and_cpu_refusals(vqa):
    assert vqa.BCEWithLogitsLoss().reduction == "mean" and vqa.BCEWithLogitsLoss("batchmean").reduction == "batchmean"
    for red in ("sum", "none", None):
        with pytest.raises(ValueError):
            vqa.BCEWithLogitsLoss(reduction=red)
    x, t = torch.zeros(2, 5), torch.zeros(2, 5)
    soft = vqa.SoftAnswers(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3))
    for crit in (vqa.BCEWithLogitsLoss(), vqa.BCEWithLogitsLoss("batchmean")):
        for tgt in (t, soft):
            with pytest.raises(vqa.VqfError):
                crit(x, tgt)
            with pytest.raises(vqa.VqfError):
                vqa.loss_and_accuracy(crit, x, tgt)
            ev = vqa.Evaluator(crit)
            with pytest.raises(vqa.VqfError):
                ev.update(x, tgt)
            r = ev.result()
            assert r["rows"] == 0 and "correct" not in r
            assert all(r[k] != r[k] for k in ("vqa_score", "accuracy", "loss_mean", "loss_last"))      # NaN: no row seen
    with pytest.raises(vqa.VqfError):
        vqa.ops.bce_logits_loss(x, t, 0.1)


def test_torch_criteria_are_still_refused(vqa):
    x, t = torch.zeros(2, 5), torch.zeros(2, 5)
    with pytest.raises(vqa.VqfError):
        vqa.loss_and_accuracy(torch.nn.BCEWithLogitsLoss(), x, t)
    with pytest.raises(vqa.VqfError):
        vqa.Evaluator(torch.nn.BCEWithLogitsLoss())
    assert type(vqa.train_step.criterion_for("mfb")).__name__ == "CrossEntropyLoss"     # solver.py:25-28, unchanged
    assert type(vqa.train_step.criterion_for("mhb")).__name__ == "KLDivLoss"


@pytest.mark.parametrize("reduction", ["mean", "batchmean"])
def test_reference_is_torchs_criterion(reduction):
    """soft_loss_ref.reference against torch.nn.functional.binary_cross_entropy_with_logits, fp64 on the CPU, 1e-12 relative:
    the loss, and the gradient through autograd; for a dense target and for the .dense(A) of a sparse one."""
    import vqa_amd
    N, A = 5, 257
    x = R.perm_rows(N, A, 8.0, seed=3)
    ids, sc = R.soft_slots(N, A, 10, seed=4)
    ids[1, 3] = ids[1, 0]                      # a repeated id
    ids[2, 5] = -1
    ids[3, 1] = A + 2
    g = torch.Generator().manual_seed(5)
    for t in (torch.rand(N, A, generator=g), vqa_amd.SoftAnswers(ids, sc).dense(A)):
        c = R.scale_of(reduction, N, A)
        ref = R.reference(x, t, c)
        xd = x.double().requires_grad_(True)
        want = R.torch_bce(xd, t, reduction)
        want.backward()
        want = want.detach()
        assert abs(float(ref["loss"]) - float(want)) <= 1e-12 * abs(float(want))
        assert float((ref["grad"] - xd.grad).abs().max()) <= 1e-12 * float(xd.grad.abs().max())
        assert abs(float(ref["row_loss"].sum() * c) - float(want)) <= 1e-12 * abs(float(want))
        assert torch.equal(ref["pred"], torch.argmax(x, 1)) and torch.equal(ref["score"], t[torch.arange(N), ref["pred"]])
        assert float(ref["abs_terms"]) >= float(ref["row_loss"].sum()) > 0
        assert R.loss_bound(ref, N, A, c) > 0 and bool((R.grad_bound(ref, t, c) > 0).all())

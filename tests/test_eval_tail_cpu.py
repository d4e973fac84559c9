"""CPU-side checks of the evaluation tail (vqf_ce_loss_pred, vqf_answer_match_rows, vqf_topk_rows): the symbols are declared
and bound, bad arguments are refused before any GPU call (NULL device pointers: nothing can have been launched), the top-k
support query answers without a device, and the host layer exports its four names and refuses a foreign criterion."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -3
NEW = ("vqf_ce_loss_pred", "vqf_answer_match_rows", "vqf_topk_rows")


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def test_symbols_are_declared_and_bound(vqa):
    hdr = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = vqa.lib.load()
    for s in NEW + ("vqf_topk_rows_supported",):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in vqa.lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.vqf_abi_version() == 7


def _ce(lib, logits=1, target=1, N=4, A=7, loss=1, ws=1, ws_bytes=64):
    # non-NULL "pointers" are the address 16: never dereferenced when the call is refused
    p = lambda f: 16 if f else None
    return lib.vqf_ce_loss_pred(p(logits), p(target), N, A, p(loss), None, None, None, None, None, 0, p(ws), ws_bytes, None)


def _match(lib, logp=1, target=1, N=4, A=7, ws=1, ws_bytes=64):
    p = lambda f: 16 if f else None
    return lib.vqf_answer_match_rows(p(logp), p(target), N, A, None, None, None, None, None, None, None, None, 0, p(ws),
                                     ws_bytes, None)


def _topk(lib, x=1, R=2, W=7, ldx=7, k=3, mode=0, idx=1, val=1):
    p = lambda f: 16 if f else None
    return lib.vqf_topk_rows(p(x), R, W, ldx, k, mode, p(idx), p(val), None)


def test_bad_arguments_are_refused_before_any_gpu_call(vqa):
    lib = vqa.lib.load()
    for kw in (dict(N=0), dict(N=-3), dict(A=0), dict(logits=0), dict(target=0), dict(loss=0), dict(ws=0)):
        assert _ce(lib, **kw) == BADARG, kw
    assert _ce(lib, ws_bytes=8 * 4 - 1) == -4          # VQF_E_WORKSPACE: 8 bytes per row
    for kw in (dict(N=0), dict(A=0), dict(logp=0), dict(target=0), dict(ws=0)):
        assert _match(lib, **kw) == BADARG, kw
    assert _match(lib, ws_bytes=8 * 4 - 1) == -4
    for kw in (dict(R=0), dict(W=0), dict(k=0), dict(k=-1), dict(k=8), dict(ldx=6), dict(x=0), dict(idx=0), dict(val=0),
               dict(mode=2)):
        assert _topk(lib, **kw) == BADARG, kw
    # well-formed but outside the kernel's range: refused as unsupported, still nothing launched
    assert _topk(lib, W=16385, ldx=16385, k=1) == UNSUPPORTED
    assert _topk(lib, W=100, ldx=100, k=17) == UNSUPPORTED


def test_topk_support_query(vqa):
    lib = vqa.lib.load()
    for W, k in ((5000, 5), (16384, 16), (1, 1)):
        assert lib.vqf_topk_rows_supported(W, k) == 1, (W, k)
        assert vqa.ops.topk_rows_supported(W, k) is True
    for W, k in ((5000, 0), (5000, -1), (4, 5), (1, 2), (0, 0)):
        assert lib.vqf_topk_rows_supported(W, k) == 0, (W, k)


def test_profiler_names_the_new_kernels(vqa):
    lib = vqa.lib.load()
    names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
    assert {"ce_loss_pred", "answer_match_rows", "topk_rows"} <= set(names) and len(set(names)) == len(names)


def test_package_exports_and_no_torch_route(vqa):
    for name in ("loss_and_accuracy", "Evaluator", "predict", "topk_answers"):
        assert callable(getattr(vqa, name)), name
    assert vqa.evaluate.predict is vqa.predict
    with pytest.raises(vqa.VqfError):
        vqa.loss_and_accuracy(torch.nn.MSELoss(), torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(vqa.VqfError):
        vqa.loss_and_accuracy(torch.nn.CrossEntropyLoss(), torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(vqa.VqfError):
        vqa.Evaluator(torch.nn.KLDivLoss())
    # the product path refuses CPU tensors here too
    with pytest.raises(vqa.VqfError):
        vqa.loss_and_accuracy(vqa.CrossEntropyLoss(), torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))
    with pytest.raises(vqa.VqfError):
        vqa.topk_answers(torch.zeros(2, 3), 2)
    assert vqa.Evaluator(vqa.CrossEntropyLoss()).result()["rows"] == 0

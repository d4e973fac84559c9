"""CPU-side checks of the optimizer tail (vqf_grad_norm_clip, vqf_grad_scale, vqf_adam_step_scaled, vqf_adamax_step,
clip_grad_norm_, Adam(max_grad_norm=...), Adamax): the restatements of optim_tail_ref.py are torch's clip_grad_norm_, Adam and
Adamax in fp64; what needs no device is refused without one; header, binding table and library agree."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_tail_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, ALIGN, WORKSPACE = -1, -2, -4
NEW = ("vqf_grad_norm_ws_bytes", "vqf_grad_norm_clip", "vqf_grad_scale", "vqf_adam_step_scaled", "vqf_adamax_step")


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def test_symbols_are_declared_bound_and_named(vqa):
    hdr = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = vqa.lib.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in vqa.lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.vqf_abi_version() == 7 and vqa.lib.ABI_VERSION == 7
    names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
    assert names[-4:] == ["grad_sumsq", "grad_scale", "adam_step_scaled", "adamax_step"]      # appended after the existing ids
    assert names.index("adam_step") == 29 and len(set(names)) == len(names)
    for name in ("Adam", "Adamax", "clip_grad_norm_"):
        assert getattr(vqa, name) is getattr(vqa.train_step, name)


def _table(vqa, sizes, grad=16):
    tab = (vqa.lib.AdamTensor * max(len(sizes), 1))()
    for i, n in enumerate(sizes):
        tab[i].param = tab[i].exp_avg = tab[i].exp_avg_sq = 16       # never dereferenced: every call below is refused
        tab[i].grad, tab[i].n = grad, n
    return ctypes.cast(tab, ctypes.c_void_p), tab


def test_workspace_query_needs_no_gpu(vqa):
    lib = vqa.lib.load()
    t, keep = _table(vqa, [1, 4096, 4097, 0, 3 * 5000])
    assert lib.vqf_grad_norm_ws_bytes(t, 5) == 4 * (1 + 1 + 2 + 0 + 4)      # one fp32 partial per 4096 elements of a tensor
    assert lib.vqf_grad_norm_ws_bytes(t, 0) == 0 and lib.vqf_grad_norm_ws_bytes(None, 3) == 0


def test_bad_arguments_are_refused_before_any_gpu_call(vqa):
    lib = vqa.lib.load()
    t, keep = _table(vqa, [5, 4097])
    ok = dict(t=t, count=2, max_norm=0.25, norm=16, coef=20, ws=32, ws_bytes=12)

    def clip(**kw):
        a = dict(ok, **kw)
        return lib.vqf_grad_norm_clip(a["t"], a["count"], a["max_norm"], a["norm"], a["coef"], a["ws"], a["ws_bytes"], None)

    for kw in (dict(count=-1), dict(t=None), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")),
               dict(norm=None), dict(coef=None), dict(ws=None), dict(t=_table(vqa, [5, -1])[0]),
               dict(t=_table(vqa, [5, 7], grad=None)[0])):
        assert clip(**kw) == BADARG, kw
    assert clip(ws_bytes=11) == WORKSPACE
    for kw in (dict(norm=18), dict(coef=21), dict(ws=33)):
        assert clip(**kw) == ALIGN, kw
    assert lib.vqf_grad_scale(t, 2, None, None) == BADARG and lib.vqf_grad_scale(t, -1, 16, None) == BADARG
    assert lib.vqf_grad_scale(None, 2, 16, None) == BADARG and lib.vqf_grad_scale(t, 2, 18, None) == ALIGN
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.vqf_adam_step_scaled(t, 2, *hyper, 1, None, None) == BADARG          # the scale is not optional here
    assert lib.vqf_adam_step_scaled(t, 2, *hyper, 0, 16, None) == BADARG            # steps count from 1
    assert lib.vqf_adam_step_scaled(t, 2, *hyper, 1, 18, None) == ALIGN
    assert lib.vqf_adam_step_scaled(None, 2, *hyper, 1, 16, None) == BADARG
    assert lib.vqf_adamax_step(t, 2, *hyper, 0, None, None) == BADARG and lib.vqf_adamax_step(t, -1, *hyper, 1, None, None) == BADARG
    assert lib.vqf_adamax_step(None, 2, *hyper, 1, None, None) == BADARG and lib.vqf_adamax_step(t, 2, *hyper, 1, 18, None) == ALIGN
    nop, keep2 = _table(vqa, [5, 7], grad=None)
    assert lib.vqf_adamax_step(nop, 2, *hyper, 1, None, None) == BADARG             # a non-empty tensor without a gradient
    assert lib.vqf_adam_step(t, 2, *hyper, 0, None) == BADARG                       # the existing entry point, as it was


def test_host_refusals_need_no_gpu(vqa):
    p = torch.nn.Parameter(torch.ones(8))
    p.grad = torch.ones(8)
    with pytest.raises(ValueError):
        vqa.clip_grad_norm_([p], 0.25, norm_type=1)
    with pytest.raises(ValueError):
        vqa.clip_grad_norm_([p], 0.25, norm_type=float("inf"))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            vqa.clip_grad_norm_([p], bad)
        for cls in (vqa.Adam, vqa.Adamax):
            with pytest.raises(ValueError):
                cls([p], max_grad_norm=bad)
    with pytest.raises(vqa.VqfError):
        vqa.clip_grad_norm_([p], 0.25)                          # a CPU gradient
    with pytest.raises(vqa.VqfError):
        vqa.clip_grad_norm_(p, 0.25)                            # a single tensor, as torch takes it
    assert torch.equal(p.grad, torch.ones(8))
    q = torch.nn.Parameter(torch.ones(8))
    assert float(vqa.clip_grad_norm_([q], 0.25)) == 0.0         # nothing has a gradient: torch's answer
    for cls in (vqa.Adam, vqa.Adamax):
        for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(betas=(0.9, 1.0)),
                   dict(weight_decay=-0.1)):
            with pytest.raises(ValueError):
                cls([p], **kw)
            with pytest.raises(ValueError):       # the same argument checks as torch
                (torch.optim.Adam if cls is vqa.Adam else torch.optim.Adamax)([p], **kw)
        with pytest.raises(vqa.VqfError):
            cls([p]).step()
        with pytest.raises(vqa.VqfError):
            cls([p], max_grad_norm=0.25).step()
    assert vqa.Adamax([p]).defaults == dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    # without the keyword the groups are torch's, key for key; with it the value is a group default
    assert "max_grad_norm" not in vqa.Adam([p]).param_groups[0]
    opt = vqa.Adam([p], max_grad_norm=0.25)
    assert opt.param_groups[0]["max_grad_norm"] == 0.25 and opt.grad_norm is None and opt.clip_coef is None
    two = vqa.Adam([{"params": [p]}, {"params": [q], "max_grad_norm": 1.0}], max_grad_norm=0.25)
    with pytest.raises(ValueError):
        two.step()                                              # one global norm: one limit


def test_state_dict_keys_interchange_with_torch_on_the_cpu(vqa):
    """load_state_dict moves no data through the library: the group keys survive both directions without a device"""
    p = torch.nn.Parameter(torch.ones(8))
    for ours, theirs in ((vqa.Adam, torch.optim.Adam), (vqa.Adamax, torch.optim.Adamax)):
        a, b = ours([p], lr=3e-3, max_grad_norm=0.25), theirs([p], lr=5e-3)
        a.load_state_dict(b.state_dict())
        assert a.param_groups[0]["lr"] == 5e-3 and a.param_groups[0]["max_grad_norm"] == 0.25
        b.load_state_dict(ours([p], lr=7e-3, max_grad_norm=0.25).state_dict())
        assert b.param_groups[0]["lr"] == 7e-3


@pytest.mark.parametrize("max_norm", [0.25, 5.0, 100.0, float("inf")])
def test_norm_and_coefficient_are_torchs(max_norm):
    gs = R.case_grads(R.SHAPES, 0)
    ps = [torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float64)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.double()
    want = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    norm = R.total_norm(gs)
    assert abs(norm - float(want)) <= 1e-13 * norm and 5.0 < norm < 100.0        # 0.25 and 5.0 clip, 100.0 does not
    # the fp32 formation, on the fp32 norm: bit for bit what torch's expression gives
    n32 = torch.tensor(norm, dtype=torch.float32)
    formed = torch.clamp(max_norm / (n32 + 1e-6), max=1.0)
    assert formed.dtype == torch.float32
    assert R.clip_coef(n32.numpy(), max_norm).tobytes() == formed.numpy().tobytes()
    _, coef, clipped = R.clip_scale(gs, max_norm)
    for p, c in zip(ps, clipped):
        assert float((p.grad - c).abs().max()) <= 2e-7 * float(c.abs().max())         # an fp32 coefficient against an fp64 one
    assert (float(coef) == 1.0) == (max_norm > norm)


def test_coefficient_edge_cases_are_torchs():
    for norm in (0.0, 1e-7, 0.2499999, 0.25, 0.2500001, 3.0, 8.8, 1e30, float("inf"), float("nan")):
        for max_norm in (0.25, 5.0, 0.3, 1e-3, 100.0, float("inf")):
            n32 = torch.tensor(norm, dtype=torch.float32)
            want = torch.clamp(max_norm / (n32 + 1e-6), max=1.0).numpy()
            assert R.clip_coef(n32.numpy(), max_norm).tobytes() == want.tobytes(), (norm, max_norm)
    assert float(R.clip_coef(0.0, 0.25)) == 1.0 and float(R.clip_coef(np.inf, 0.25)) == 0.0 and np.isnan(R.clip_coef(np.nan, 0.25))


@pytest.mark.parametrize("rule", ["adam", "adamax"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", [0.25, 100.0])
def test_clip_then_step_is_torchs(rule, wd, max_norm):
    steps = 6
    ps = [torch.nn.Parameter(p.double()) for p in R.case_params(R.SHAPES)]
    opt = (torch.optim.Adam if rule == "adam" else torch.optim.Adamax)(ps, lr=R.LR0, weight_decay=wd, foreach=False)
    for step in range(steps):
        for grp in opt.param_groups:
            grp["lr"] = R.case_lr(step)
        for p, g in zip(ps, R.case_grads(R.SHAPES, step)):
            p.grad = g.double()
        torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
    got, norms = R.run(rule, R.SHAPES, steps, wd, max_norm)
    assert len(norms) == steps and all(5.0 < n < 100.0 for n in norms)
    for p, g in zip(ps, got):
        # the restatement's coefficient is formed in fp32 (that is what is restated), torch's here in fp64: 2^-24 on each gradient
        assert float((p.detach() - g).abs().max()) <= 2e-7 * float(g.abs().max())
    plain, _ = R.run(rule, R.SHAPES, steps, wd, None)
    if max_norm == 100.0:         # a coefficient of exactly 1: the unclipped run, bit for bit
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
    else:
        assert any(not torch.equal(a, b) for a, b in zip(got, plain))


def test_error_bound_is_a_few_roundings():
    assert 14 * R.U32 <= R.norm_bound_rel(7) <= 14.1 * R.U32
    assert R.norm_bound_rel(1 << 19) <= 14.1 * R.U32

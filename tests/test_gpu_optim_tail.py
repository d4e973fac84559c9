"""The optimizer tail on the GPU (csrc/train.hip): the multi-tensor gradient norm with its clip coefficient, clip_grad_norm_,
Adam / Adamax reading the coefficient in their one launch -- against fp64 (optim_tail_ref.py), against torch on the CPU, and
bit for bit against clip_grad_norm_ followed by the plain step.

Norm: within optim_tail_ref.norm_bound_rel (14 x 2^-24, counted from the kernel).  Measured on the MI355X: at most 0.033 of the
bound on the four gradient sets below (the figures are printed by the test and kept in profiles/optim_tail_parity.txt).
Parameters after six steps: 2e-6 (golden_util.rel_err), the figure tests/test_gpu_train_step.py holds Adam to."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import optim_tail_ref as R
from golden_util import rel_err

pytestmark = pytest.mark.gpu

SENT = -777.0          # no partial sum, norm or coefficient is negative
MAX_NORMS = (0.25, 5.0, 100.0)


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    return vqa_amd


def _views(tensors, offset=3):
    """the tensors as views at odd offsets of one flat GPU buffer: what the all-reducer hands over (no view is 16-byte aligned
    unless its offset happens to be a multiple of four elements)"""
    flat = torch.zeros(sum(t.numel() for t in tensors) + offset, device="cuda")
    out, off = [], offset
    for t in tensors:
        v = flat[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        out.append(v)
        off += t.numel()
    return out


LARGE = (1900 * 4096 + 17,)      # 1901 of the 1902 partials: some threads of the finish take its eight-loads-at-a-time loop, the others do not


def _grad_set(name):
    if name == "shapes":
        return [g.cuda() for g in R.case_grads(R.SHAPES, 0)]
    if name == "many_views":
        return _views(R.case_grads(R.MANY_SHAPES, 0))
    if name == "large":
        return [g.cuda() for g in R.case_grads([LARGE, (5,)], 0)]
    c = [g.cuda() for g in R.case_grads(R.SHAPES, 1)]
    c.insert(3, torch.empty(0, device="cuda"))
    return c


def _raw_clip(vqa, grads, max_norm):
    """vqf_grad_norm_clip on buffers with sentinels on both sides of norm, coef and the workspace's used range
    -> (out (5,): [s, norm, s, coef, s], ws, number of partials)"""
    lib = vqa.lib.load()
    tab = (vqa.lib.AdamTensor * len(grads))()
    for i, g in enumerate(grads):
        tab[i].grad, tab[i].n = g.data_ptr(), g.numel()
    t = ctypes.cast(tab, ctypes.c_void_p)
    nb = int(lib.vqf_grad_norm_ws_bytes(t, len(grads)))
    assert nb == 4 * sum((g.numel() + 4095) // 4096 for g in grads)
    out = torch.full((5,), SENT, device="cuda")
    ws = torch.full((nb // 4 + 8,), SENT, device="cuda")
    rc = lib.vqf_grad_norm_clip(t, len(grads), float(max_norm), out.data_ptr() + 4, out.data_ptr() + 12, ws.data_ptr() + 16, nb,
                                vqa.ops._stream())
    assert rc == 0
    return out.cpu(), ws.cpu(), nb // 4


def _torch_coef(norm, max_norm):
    """torch's expression in fp32 on the kernel's own norm (a 0-d CPU tensor)"""
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def _same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("name", ["shapes", "many_views", "with_empty", "large"])
def test_norm_against_fp64_bits_repeat_sentinels_intact(vqa, name):
    grads = _grad_set(name)
    if name == "many_views":
        assert len(grads) == 70 and sum(g.data_ptr() % 16 != 0 for g in grads) > 32
    out, ws, parts = _raw_clip(vqa, grads, 0.25)
    out2, ws2, _ = _raw_clip(vqa, grads, 0.25)
    assert out.numpy().tobytes() == out2.numpy().tobytes() and ws.numpy().tobytes() == ws2.numpy().tobytes()
    assert out[0] == SENT and out[2] == SENT and out[4] == SENT
    assert bool((ws[:4] == SENT).all()) and bool((ws[4 + parts:] == SENT).all())
    assert bool((ws[4:4 + parts] >= 0).all())                              # every partial of the used range was written
    want = R.total_norm(grads)
    err, bound = abs(float(out[1]) - want), R.norm_bound_rel(parts) * want
    print("optim_tail norm %-11s tensors %2d partials %2d norm %.9g fp64 %.17g err %.3e bound %.3e err/bound %.3f"
          % (name, len(grads), parts, float(out[1]), want, err, bound, err / bound))
    assert err <= bound
    assert _same_bits(out[3], _torch_coef(out[1], 0.25)) and float(out[3]) < 1.0
    # the wrapper is the same call
    norm, coef = vqa.ops.grad_norm_clip(grads, 0.25)
    assert norm.shape == () and coef.shape == () and norm.is_cuda and coef.is_cuda
    assert _same_bits(norm, out[1]) and _same_bits(coef, out[3])


def test_norm_is_exact_on_small_integers(vqa):
    g = torch.Generator().manual_seed(11)
    ints = [torch.randint(-2, 3, s, generator=g).float() for s in R.SHAPES]
    for grads in ([t.cuda() for t in ints], _views(ints)):
        out, ws, parts = _raw_clip(vqa, grads, 1.0)
        exact = sum(int((t.long() ** 2).sum()) for t in ints)
        assert exact < 2 ** 24 and float(ws[4:4 + parts].double().sum()) == float(exact)      # the fp32 sums are exact
        want = np.float32(np.sqrt(np.float64(exact)))
        assert abs(float(out[1]) - float(want)) <= R.ulp32(want)


@pytest.mark.parametrize("kind", ["case", "zero", "nan", "inf"])
@pytest.mark.parametrize("max_norm", [0.25, 100.0, float("inf")])
def test_coefficient_is_torchs_expression_on_the_kernels_norm(vqa, kind, max_norm):
    grads = [g.cuda() for g in R.case_grads(R.SHAPES, 0)]
    if kind == "zero":
        grads = [torch.zeros_like(g) for g in grads]
    elif kind != "case":
        grads[6].view(-1)[4096] = float(kind)               # one element, in the scalar tail of a tensor's last block
    out, _, _ = _raw_clip(vqa, grads, max_norm)
    norm, coef, want = out[1], out[3], _torch_coef(out[1], max_norm)
    if kind == "nan":
        assert torch.isnan(norm) and torch.isnan(coef) and torch.isnan(want)
        return
    if kind == "inf" and max_norm == float("inf"):
        assert float(norm) == float("inf") and torch.isnan(coef) and torch.isnan(want)      # 0 * inf, as torch
        return
    assert _same_bits(coef, want)
    if kind == "inf":
        assert float(norm) == float("inf") and float(coef) == 0.0
    elif kind == "zero":
        assert float(norm) == 0.0 and float(coef) == 1.0
    else:
        assert 5.0 < float(norm) < 100.0 and (float(coef) == 1.0) == (max_norm > 5.0)


@pytest.mark.parametrize("max_norm", [0.25, 100.0])
@pytest.mark.parametrize("views", [False, True])
def test_clip_grad_norm_scales_in_place(vqa, max_norm, views):
    shapes = R.MANY_SHAPES if views else R.SHAPES
    gs = R.case_grads(shapes, 2)
    ps = [torch.nn.Parameter(p.cuda()) for p in R.case_params(shapes)]
    for p, g in zip(ps, _views(gs) if views else [g.cuda() for g in gs]):
        p.grad = g
    ps[1].grad = None
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    data = [p.detach().clone() for p in ps]
    want_norm, want_coef = vqa.ops.grad_norm_clip([p.grad for p in ps if p.grad is not None], max_norm)   # (scales nothing)
    norm = vqa.clip_grad_norm_(ps, max_norm)
    assert norm.shape == () and norm.is_cuda and _same_bits(norm, want_norm)
    assert abs(float(norm) - R.total_norm([g for g in before if g is not None])) <= R.norm_bound_rel(100) * float(norm)
    assert ps[1].grad is None
    for p, g0, d in zip(ps, before, data):
        assert _same_bits(p.detach(), d)                                    # parameters are not touched
        if g0 is not None:
            assert _same_bits(p.grad, g0 * want_coef)                       # one fp32 multiply, formed by torch
    assert (float(want_coef) == 1.0) == (max_norm == 100.0)
    want_one = vqa.ops.grad_norm_clip([ps[0].grad], max_norm)[0]
    assert _same_bits(vqa.clip_grad_norm_(ps[0], max_norm), want_one)      # a single tensor, as torch takes it


def _classes(vqa, rule):
    return (vqa.Adam, torch.optim.Adam) if rule == "adam" else (vqa.Adamax, torch.optim.Adamax)


def _state(opt, ps):
    second = "exp_avg_sq" if "exp_avg_sq" in opt.state[ps[0]] else "exp_inf"
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p][second].cpu()) for p in ps]


@functools.lru_cache(maxsize=None)
def _runs(rule, wd, max_norm, many=False, steps=6):
    """The case driven four ways -> dict: 'fused' cls(max_grad_norm), 'two' clip_grad_norm_ + the plain step, 'plain' no clipping
    (each a list of (param, exp_avg, second state) on the CPU), 'torch' torch's clip_grad_norm_ + optimizer on the CPU,
    'fp64' the restatement; 'grad_kept': p.grad after every fused step had the bits of before; 'coefs' of the fused steps."""
    import vqa_amd
    ours, theirs = _classes(vqa_amd, rule)
    shapes = R.MANY_SHAPES if many else R.SHAPES
    mk = lambda: [torch.nn.Parameter(p.cuda()) for p in R.case_params(shapes)]
    pf, pt, pp = mk(), mk(), mk()
    pr = [torch.nn.Parameter(p.clone()) for p in R.case_params(shapes)]
    fused = ours(pf, lr=R.LR0, weight_decay=wd, max_grad_norm=max_norm)
    two = ours(pt, lr=R.LR0, weight_decay=wd)
    plain = ours(pp, lr=R.LR0, weight_decay=wd)
    ref = theirs(pr, lr=R.LR0, weight_decay=wd)
    kept, coefs, norms = True, [], []
    for step in range(steps):
        gs = R.case_grads(shapes, step)
        for o in (fused, two, plain, ref):
            for grp in o.param_groups:
                grp["lr"] = R.case_lr(step)
        for group in (pf, pt, pp):
            for p, g in zip(group, _views(gs) if many else [g.cuda() for g in gs]):
                p.grad = g
        for p, g in zip(pr, gs):
            p.grad = g.clone()
        before = [p.grad.clone() for p in pf]
        fused.step()
        kept = kept and all(_same_bits(p.grad, g) for p, g in zip(pf, before))
        coefs.append(float(fused.clip_coef))
        norms.append(float(fused.grad_norm))
        assert fused.grad_norm.shape == () and fused.grad_norm.is_cuda and fused.clip_coef.is_cuda
        vqa_amd.clip_grad_norm_(pt, max_norm)
        two.step()
        plain.step()
        torch.nn.utils.clip_grad_norm_(pr, max_norm)
        ref.step()
    fp64, ref_norms = R.run(rule, shapes, steps, wd, max_norm)
    return dict(fused=_state(fused, pf), two=_state(two, pt), plain=_state(plain, pp), torch=[p.detach() for p in pr], fp64=fp64,
                grad_kept=kept, coefs=coefs, norms=norms, ref_norms=ref_norms)


@pytest.mark.parametrize("rule", ["adam", "adamax"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", MAX_NORMS)
def test_fused_step_has_the_bits_of_clip_then_step(rule, wd, max_norm):
    r = _runs(rule, wd, max_norm)
    for a, b in zip(r["fused"], r["two"]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))              # the parameter and both state tensors
    assert r["grad_kept"]
    clips = max_norm < 100.0
    assert all((c < 1.0) == clips for c in r["coefs"])
    same_as_plain = all(_same_bits(x, y) for a, b in zip(r["fused"], r["plain"]) for x, y in zip(a, b))
    assert same_as_plain == (not clips)        # a coefficient of exactly 1: every bit of the optimizer built without the keyword


@pytest.mark.parametrize("rule", ["adam", "adamax"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", MAX_NORMS)
def test_fused_step_tracks_torch_and_fp64(rule, wd, max_norm):
    r = _runs(rule, wd, max_norm)
    for n, m in zip(r["norms"], r["ref_norms"]):
        assert abs(n - m) <= R.norm_bound_rel(8) * m + R.ulp32(m)       # (ref_norms: the fp64 norm rounded to fp32)
    for (p, _, _), pt, p64 in zip(r["fused"], r["torch"], r["fp64"]):
        assert rel_err(p, pt) < 2e-6
        assert rel_err(p, p64) < 2e-6


@pytest.mark.parametrize("rule", ["adam", "adamax"])
def test_many_tensors_as_unaligned_views(rule):
    r = _runs(rule, 0.0, 0.25, many=True, steps=3)
    assert len(r["fused"]) == 70 and r["grad_kept"] and all(c < 1.0 for c in r["coefs"])
    for a, b in zip(r["fused"], r["two"]):
        assert all(_same_bits(x, y) for x, y in zip(a, b))
    for (p, _, _), pt, p64 in zip(r["fused"], r["torch"], r["fp64"]):
        assert rel_err(p, pt) < 2e-6 and rel_err(p, p64) < 2e-6


def test_adamax_state_dict_interchanges_with_torch(vqa):
    shapes = [(10, 3), (5,)]

    def drive(opt, ps, steps, first=0):
        for step in range(first, first + steps):
            for p, g in zip(ps, R.case_grads(shapes, step)):
                p.grad = g.to(p.device)
            opt.step()

    ps_gpu = [torch.nn.Parameter(p.cuda()) for p in R.case_params(shapes)]
    ps_ref = [torch.nn.Parameter(p.clone()) for p in R.case_params(shapes)]
    opt, ref = vqa.Adamax(ps_gpu, lr=R.LR0), torch.optim.Adamax(ps_ref, lr=R.LR0)
    drive(opt, ps_gpu, 2)
    drive(ref, ps_ref, 2)
    sd = opt.state_dict()
    assert sorted(sd["state"][0].keys()) == ["exp_avg", "exp_inf", "step"]
    assert sorted(sd["param_groups"][0].keys()) == ["betas", "eps", "lr", "params", "weight_decay"]
    t_ps = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps_gpu]
    t_from_ours = torch.optim.Adamax(t_ps, lr=1e-3)
    t_from_ours.load_state_dict(sd)
    o_ps = [torch.nn.Parameter(p.detach().clone().cuda()) for p in ps_ref]
    ours_from_t = vqa.Adamax(o_ps, lr=1e-3, max_grad_norm=100.0)
    ours_from_t.load_state_dict(ref.state_dict())
    assert ours_from_t.param_groups[0]["lr"] == R.LR0 and ours_from_t.param_groups[0]["max_grad_norm"] == 100.0
    drive(t_from_ours, t_ps, 1, first=2)
    drive(ours_from_t, o_ps, 1, first=2)
    for a, b in zip(t_ps, o_ps):
        assert rel_err(a.detach(), b.detach().cpu()) < 2e-6
    assert float(ours_from_t.state[o_ps[0]]["step"]) == 3.0 and float(ours_from_t.clip_coef) == 1.0


def test_adamax_skips_params_without_grad_and_rejects_cpu(vqa):
    a = torch.nn.Parameter(torch.ones(8, device="cuda"))
    b = torch.nn.Parameter(torch.ones(8, device="cuda"))
    for kw in ({}, {"max_grad_norm": 0.25}):
        opt = vqa.Adamax([a, b], lr=0.1, **kw)
        a.grad = torch.ones(8, device="cuda")
        before = float(a.detach()[0])
        opt.step()
        assert float(b.detach().sum()) == 8.0 and float(a.detach()[0]) < before
        assert len(opt.state[b]) == 0 and sorted(opt.state[a].keys()) == ["exp_avg", "exp_inf", "step"]
    c = torch.nn.Parameter(torch.ones(8))
    c.grad = torch.ones(8)
    with pytest.raises(vqa.VqfError):
        vqa.Adamax([c]).step()
    with pytest.raises(vqa.VqfError):
        vqa.Adamax([c], max_grad_norm=0.25).step()
    d = torch.nn.Parameter(torch.ones(8, device="cuda", dtype=torch.float64))
    d.grad = torch.ones_like(d)                                 # a non-fp32 gradient
    with pytest.raises(vqa.VqfError):
        vqa.clip_grad_norm_([d], 0.25)


def test_full_train_steps_with_clipping_track_torch(vqa):
    """Three solver iterations on the small MFB of test_full_train_steps_track_torch_solver_tail, dropout off: the package
    criterion + Adam(max_grad_norm=0.25) against torch's CrossEntropyLoss + clip_grad_norm_(0.25) + Adam."""
    from cases import MFB_CASES
    from golden_util import recipe_sd, mfb_inputs
    from oracle import ref_torch as O
    case = MFB_CASES[1]
    cfg, img, q, _, hard, _ = mfb_inputs(case)
    sd = recipe_sd(O.mfb_shapes(cfg), case["salt"])
    outs, coefs = [], []
    for mine in (True, False):
        m = vqa.MFB(cfg).cuda()
        m.load_state_dict(sd)
        m.train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        crit = vqa.CrossEntropyLoss() if mine else torch.nn.CrossEntropyLoss()
        opt = vqa.Adam(m.parameters(), lr=1e-4, max_grad_norm=0.25) if mine else torch.optim.Adam(m.parameters(), lr=1e-4)
        for _ in range(3):
            loss = crit(m.forward(img.cuda(), q.cuda()), hard.cuda())
            opt.zero_grad()
            loss.backward()
            if mine:
                opt.step()
                coefs.append(float(opt.clip_coef))
            else:
                coefs.append(float(torch.clamp(0.25 / (torch.nn.utils.clip_grad_norm_(m.parameters(), 0.25) + 1e-6), max=1.0)))
                opt.step()
        with torch.no_grad():
            outs.append(m.forward(img.cuda(), q.cuda()).cpu())
    print("optim_tail train-level clip coefficients ours %s torch %s" % (coefs[:3], coefs[3:]))
    assert rel_err(outs[0], outs[1]) < 1e-4

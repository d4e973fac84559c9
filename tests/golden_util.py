"""Helpers shared by the oracle/golden tests and the GPU parity tests."""
import os
import numpy as np
import torch

import recipe
from cases import make_cfg, sample_indices

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def recipe_sd(shapes, salt, device="cpu", requires_grad=False):
    sd = {}
    for k, shp in shapes.items():
        t = torch.from_numpy(recipe.weight_for(k, shp, salt)).to(device)
        if requires_grad:
            t.requires_grad_(True)
        sd[k] = t
    return sd


def mfb_inputs(case, device="cpu"):
    cfg = make_cfg(case)
    N, T = case["N"], case["T"]
    img = torch.from_numpy(recipe.img_features(N, cfg.img_feature_dim, cfg.img_feature_channel, case["salt"])).to(device)
    q = torch.from_numpy(recipe.question_tokens(N, T, cfg.q_vocab_size, case["salt"])).to(device)
    glove = None
    if case["glove"]:
        glove = torch.from_numpy(recipe.sym_tensor((N, T, cfg.emb_dim), 0.5, recipe.name_seed("glove", case["salt"]))).to(device)
    hard = torch.from_numpy(recipe.hard_answers(N, cfg.a_vocab_size, case["salt"])).to(device)
    soft = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, case["salt"])).to(device)
    return cfg, img, q, glove, hard, soft


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def check_tensor_digest(prefix, t, gold, tol):
    a = t.detach().cpu().reshape(-1).double().numpy()
    s, ab = float(gold[prefix + "/sum"]), float(gold[prefix + "/abs"])
    assert abs(np.abs(a).sum() - ab) <= tol * max(ab, 1e-30) + 1e-12, (prefix, "abs", np.abs(a).sum(), ab)
    assert abs(a.sum() - s) <= tol * max(ab, 1e-30) + 1e-12, (prefix, "sum", a.sum(), s)
    if prefix + "/full" in gold:
        assert rel_err(t.detach().cpu().numpy().reshape(-1), gold[prefix + "/full"].reshape(-1)) <= tol, prefix
    else:
        idx = sample_indices(prefix, a.size, 64)
        assert rel_err(a[idx], gold[prefix + "/samp"]) <= tol, prefix


FP32_SPREAD = 2.0    # check_grads: two fp32 runs differ by up to ~2x what one of them is from the fp64 value


def check_grads(named_grads, gold, tol, zero_ok_abs=1e-9):
    """named_grads: {name: tensor or None}.  Compares norms + sampled entries.

    Sampled entries are compared relative to the gradient's RMS magnitude
    (norm / sqrt(numel)) so that near-zero samples do not dominate.

    Where the golden also holds the reference's fp64 norm (g64norm/), a tensor whose recorded fp32 norm is itself
    further than tol / FP32_SPREAD from it is compared at FP32_SPREAD x that recorded distance instead of tol: the fp32
    rounding behind the signed square root depends on the host's BLAS code path (AVX-512, AVX2, SSE), and two fp32 runs
    can differ by the sum of their distances to the fp64 value.  The fp64 digests pin such tensors exactly (check_grads64).
    """
    gmax = max([float(v) for kk, v in gold.items() if kk.startswith("gnorm/")] + [0.0])
    zero_ok_abs = max(zero_ok_abs, 1e-6 * gmax)
    for k, g in named_grads.items():
        if ("gnone/" + k) in gold:
            assert g is None or float(g.abs().max()) == 0.0, (k, "reference grad is None")
            continue
        assert g is not None, (k, "missing gradient")
        a = g.detach().cpu().reshape(-1).double().numpy()
        gn = float(gold["gnorm/" + k])
        n = float(np.sqrt((a * a).sum()))
        if gn <= zero_ok_abs:
            # exactly-zero (dead) or pure rounding-noise gradients (e.g. the bias in
            # front of a shift-invariant softmax): only require "still negligible"
            assert n <= 10 * zero_ok_abs, (k, "reference gradient is (numerically) zero", n)
            continue
        tol_k = tol
        g64n = float(gold.get("g64norm/" + k, 0.0))
        if g64n > zero_ok_abs:
            tol_k = max(tol, FP32_SPREAD * abs(gn - g64n) / g64n)
        assert abs(n - gn) <= tol_k * gn, (k, "norm", n, gn, tol_k)
        idx = sample_indices(k, a.size, 16)
        rms = gn / np.sqrt(a.size)
        d = np.abs(a[idx] - gold["gsamp/" + k].astype(np.float64)).max()
        scale = max(np.abs(gold["gsamp/" + k]).max(), rms)
        assert d <= tol_k * scale * 4, (k, "samples", d, scale)


def check_grads64(named_grads, gold, tol=1e-8):
    """fp64 oracle gradients vs the reference run in fp64 (g64norm/g64samp digests)."""
    gmax = max([float(v) for kk, v in gold.items() if kk.startswith("g64norm/")] + [0.0])
    for k, g in named_grads.items():
        if ("gnone/" + k) in gold:
            assert g is None or float(g.abs().max()) == 0.0, (k, "reference grad is None")
            continue
        a = g.detach().cpu().reshape(-1).double().numpy()
        gn = float(gold["g64norm/" + k])
        n = float(np.sqrt((a * a).sum()))
        floor = 1e-12 * gmax          # mathematically-zero gradients (bias before a softmax)
        assert abs(n - gn) <= max(tol * gn, floor), (k, "norm64", n, gn)
        idx = sample_indices(k, a.size, 16)
        d = np.abs(a[idx] - gold["g64samp/" + k]).max()
        assert d <= max(tol * max(np.abs(gold["g64samp/" + k]).max(), gn / np.sqrt(a.size)), floor), (k, d)


def _report_parity(label, worst, worst_name, detail=""):
    """Drift visibility: the worst err/bound of every grad_parity call is printed and, on
    the GPU box, appended to gpurun_out/grad_parity.log (copied to profiles/ per round) -- with the ABSOLUTE relative
    errors behind it: err/|g64| and the fp32 noise term noise/|g64| of that tensor, and the largest of each over all
    tensors of the call, so that a drift of the noise term itself (a looser bound, not a better kernel) shows."""
    import inspect
    if not label:
        for fr in inspect.stack()[2:8]:
            if fr.function.startswith("test_"):
                label = fr.function
                break
    line = "grad_parity %-70s worst err/bound %.3f  (%s)%s" % (label or "?", worst, worst_name, detail)
    print(line)
    root = os.environ.get("GRAFT_REPO_ROOT")
    if root and os.path.isdir(os.path.join(root, "gpurun_out")):
        with open(os.path.join(root, "gpurun_out", "grad_parity.log"), "a") as f:
            f.write(line + "\n")


ILL_CONDITIONED = 0.05      # noise/|g64| above which grad_parity's bound (8x the noise) is too loose to pin a tensor on its own


def grad_parity(gpu_grads, g32, g64, k=8.0, floor=5e-4, label="", node_checked=None, noise32=None):
    """Conditioning-aware gradient criterion.

    g64 = oracle gradients in float64 (pinned to the reference's fp64 run at 1e-8),
    g32 = oracle gradients in float32 (the reference CPU path's arithmetic).
    The HIP path must be as close to the exact gradient as the CPU fp32 path is:
        |g_gpu - g64| <= max(k * |g32 - g64|, floor * |g64|, 1e-6 * max_k |g64_k|)      (k = 8, floor = 5e-4)
    (l2 norms per parameter tensor).  The signed square root's derivative
    0.5*|s|^-1/2 makes fp32 gradients differ by up to ~1e-2 between ANY two
    summation orders, which is why a fixed relative tolerance against the
    reference's own fp32 gradients is not meaningful.

    node_checked (names of the parameters whose gradient was produced by a node that tests/node_harness.check_every_node
    compared with an fp64 evaluation of THAT node in the same step): at the BASELINE batches the CPU fp32 path itself is
    5-300 % from the fp64 gradient for the tensors behind the signed square root, so this criterion alone would accept an
    all-zero gradient there.  Every tensor with noise/|g64| > ILL_CONDITIONED must be in node_checked (asserted, and listed
    in the report line); callers at the full batch sizes pass it.

    noise32 ({name: |g32 - g64|}, recorded under tests/golden/ by make_golden.py): the fp32 noise term of a recorded oracle run
    in place of the one computed on this host.  The CPU fp32 path's summation order depends on the host's BLAS code path (the noise of
    one tensor differs by up to ~5x between hosts), so a recorded yardstick keeps the bound the same on every machine.
    """
    gmax = max(float(g.norm()) for g in g64.values() if g is not None)
    worst, worst_name, worst_rel = 0.0, "-", (0.0, 0.0)
    max_err_rel, max_noise_rel = (0.0, "-"), (0.0, "-")
    ill = []
    for name, gg in gpu_grads.items():
        r64 = g64[name]
        if r64 is None:
            assert gg is None or float(gg.abs().max()) == 0.0, (name, "oracle grad is None")
            continue
        assert gg is not None, (name, "missing gradient")
        r64 = r64.double()
        noise = float(noise32[name]) if noise32 is not None else float((g32[name].double() - r64).norm())
        err = float((gg.detach().cpu().double() - r64).norm())
        bound = max(k * noise, floor * float(r64.norm()), 1e-6 * gmax)
        assert err <= bound, (name, "err %.3e bound %.3e noise32 %.3e norm %.3e" % (err, bound, noise, float(r64.norm())))
        n64 = float(r64.norm())
        if n64 > 1e-6 * gmax:                      # relative errors of numerically-zero gradients say nothing
            if err / n64 > max_err_rel[0]:
                max_err_rel = (err / n64, name)
            if noise / n64 > max_noise_rel[0]:
                max_noise_rel = (noise / n64, name)
            if noise / n64 > ILL_CONDITIONED:
                ill.append((name, noise / n64))
        if err / bound > worst:
            tiny = n64 <= 1e-6 * gmax              # a numerically-zero gradient: its relative errors say nothing
            worst, worst_name = err / bound, name
            worst_rel = (float("nan"), float("nan")) if tiny else (err / n64, noise / n64)
    cover = ""
    if node_checked is not None:
        missing = [n for n, _ in ill if n not in node_checked]
        assert not missing, ("tensors whose fp32 noise exceeds %.0f %% of the gradient and that no node check covers" % (100 * ILL_CONDITIONED),
                             missing)
        cover = "; %d tensor(s) with noise/|g64| > %.2f, ALL covered by this step's fp64 node checks: %s" % (
            len(ill), ILL_CONDITIONED, ", ".join("%s %.2f" % (n, r) for n, r in sorted(ill, key=lambda t: -t[1])[:6]) or "-")
    elif ill:
        cover = "; %d tensor(s) with noise/|g64| > %.2f (no node checks in this test)" % (len(ill), ILL_CONDITIONED)
    _report_parity(label, worst, worst_name,
                   "  err/|g64| %.2e noise/|g64| %.2e there; max over tensors: err/|g64| %.2e (%s), noise/|g64| %.2e (%s)%s"
                   % (worst_rel[0], worst_rel[1], max_err_rel[0], max_err_rel[1], max_noise_rel[0], max_noise_rel[1], cover))
    return worst

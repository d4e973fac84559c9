"""LSTM sequence kernels (MHBCoAtt's batch-axis recursion) vs torch.nn.LSTM in fp64."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("S,B,I,H", [(40, 14, 300, 256), (7, 22, 48, 512), (3, 32, 16, 256), (5, 1, 8, 256),
                                     (1, 14, 300, 1024), (64, 14, 600, 1024), (9, 16, 32, 768), (33, 3, 20, 512)])
def test_lstm_seq_matches_torch_lstm(S, B, I, H):
    import vqa_amd
    vqa_amd.lib.load()
    fn = vqa_amd.functions.LstmSeqFn
    torch.manual_seed(S * 1000 + B)
    ref = torch.nn.LSTM(I, H, 1).double()
    x = (torch.rand(S, B, I, dtype=torch.float64) * 2 - 1).float().double().requires_grad_()
    for p in ref.parameters():
        p.data = p.data.float().double()
    out_ref, _ = ref(x)
    w = torch.linspace(-1, 1, out_ref.numel(), dtype=torch.float64).view_as(out_ref)
    (out_ref * w).sum().backward()
    xs = x.detach().float().cuda().requires_grad_()
    ps = [p.detach().float().cuda().requires_grad_() for p in
          (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)]
    hs = fn.apply(xs, *ps)
    assert _rel(hs, out_ref) <= 2e-5
    (hs * w.float().cuda()).sum().backward()
    assert _rel(xs.grad, x.grad) <= 1e-4
    for p, r in zip(ps, (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)):
        assert _rel(p.grad, r.grad) <= 1e-4


def test_unsupported_shapes_are_reported():
    import vqa_amd
    ops = vqa_amd.ops
    assert ops.lstm_seq_supported(14, 1024) and ops.lstm_seq_supported(32, 256)
    assert not ops.lstm_seq_supported(33, 1024) and not ops.lstm_seq_supported(14, 64)
    with pytest.raises(vqa_amd.VqfError):
        ops.lstm_seq_fwd(torch.zeros(2, 40, 4 * 256, device="cuda"), torch.zeros(4 * 256, 256, device="cuda"))


def test_mhbcoatt_hip_lstm_equals_miopen_lstm():
    """MHBCoAtt with the HIP sequence kernel vs the same module on nn.LSTM (full dims, N=6)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import vqa_amd, recipe
    from cases import MHBCOATT_CASES
    from golden_util import mfb_inputs
    case = dict(MHBCOATT_CASES[-1], N=6, salt=91)
    cfg, img, q, glove, hard, soft = mfb_inputs(case, "cuda")
    model = vqa_amd.MHBCoAtt(cfg)
    model.load_state_dict({k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"]))
                           for k, v in model.state_dict().items()})
    model = model.cuda().train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    res = {}
    for hip in (True, False):
        model.use_hip_lstm = hip
        model.zero_grad(set_to_none=True)
        out = model.forward(img, q)
        torch.nn.KLDivLoss()(out, soft).backward()
        res[hip] = (out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
    assert _rel(res[True][0], res[False][0]) <= 1e-5
    for k in res[True][1]:
        a, b = res[True][1][k], res[False][1][k]
        assert float((a - b).norm()) <= 2e-3 * float(b.norm()) + 1e-9, k


def _seq_inputs(S, B, H, seed):
    g = torch.Generator().manual_seed(seed)
    xw = ((torch.rand((S, B, 4 * H), generator=g) * 2 - 1) * 1.5).cuda()
    w_hh = ((torch.rand((4 * H, H), generator=g) * 2 - 1) * 0.04).cuda()
    dhs = ((torch.rand((S, B, H), generator=g) * 2 - 1)).cuda()
    return xw, w_hh, dhs


@pytest.mark.parametrize("S,B,H", [(64, 14, 1024), (40, 22, 256), (9, 16, 768), (33, 3, 512)])
def test_bf16_operand_recursion_tracks_fp32(S, B, H):
    """bf16 mode (config 3): W_hh and h / dG enter the MFMA as bf16, everything else fp32.  Against the fp32
    kernels on the same inputs: h within 2e-2 of max|h| (8 mantissa bits, K = H products per gate, recurrent),
    dgates within 5 % in norm (sanity; bf16 gradients are not a parity target).
    The sharp check of both modes is per step and per element: tests/test_gpu_lstm_seq_kernels.py."""
    import vqa_amd
    ops = vqa_amd.ops
    xw, w_hh, dhs = _seq_inputs(S, B, H, 3 * S + B)
    hs0, cs0, g0 = ops.lstm_seq_fwd(xw, w_hh)
    hs1, cs1, g1 = ops.lstm_seq_fwd(xw, w_hh, bf16=True)
    assert not torch.equal(hs0, hs1)                               # the bf16 kernels really ran
    assert _rel(hs1, hs0) <= 2e-2 and _rel(cs1, cs0) <= 2e-2
    d0 = ops.lstm_seq_bwd(dhs, g0, cs0, w_hh)
    d1 = ops.lstm_seq_bwd(dhs, g0, cs0, w_hh, bf16=True)
    assert float((d1 - d0).norm()) <= 5e-2 * float(d0.norm())
    # exactness of the formulation: with bf16-representable W_hh and a single step the rounding of h is the only
    # difference, and step 0 (no recurrent term) must be bit-identical
    assert torch.equal(hs1[0], hs0[0]) and torch.equal(d1[-1], d0[-1])


@pytest.mark.parametrize("T,B,I,H", [(14, 512, 300, 1024), (7, 33, 24, 64), (1, 5, 8, 16), (22, 3, 600, 1024)])
def test_lstm_batch_matches_torch_lstm(T, B, I, H):
    """Large-batch form (MFB's orientation: T steps of an N-row batch): GEMMs + point-wise cell kernels vs
    torch.nn.LSTM in fp64: 2e-5 forward, 1e-4 gradients."""
    import vqa_amd
    vqa_amd.lib.load()
    fn = vqa_amd.functions.LstmBatchFn
    torch.manual_seed(T * 100 + B)
    ref = torch.nn.LSTM(I, H, 1).double()
    x = (torch.rand(T, B, I, dtype=torch.float64) * 2 - 1).float().double().requires_grad_()
    for p in ref.parameters():
        p.data = p.data.float().double()
    out_ref, _ = ref(x)
    w = torch.linspace(-1, 1, out_ref.numel(), dtype=torch.float64).view_as(out_ref)
    (out_ref * w).sum().backward()
    xs = x.detach().float().cuda().requires_grad_()
    ps = [p.detach().float().cuda().requires_grad_() for p in
          (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)]
    hs = fn.apply(xs, *ps)
    assert _rel(hs, out_ref) <= 2e-5
    (hs * w.float().cuda()).sum().backward()
    assert _rel(xs.grad, x.grad) <= 1e-4
    for p, r in zip(ps, (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)):
        assert _rel(p.grad, r.grad) <= 1e-4


def test_mfb_hip_lstm_equals_miopen_lstm():
    """MFB with the HIP question-encoder recursion vs the same module on nn.LSTM (full dims, N = 6)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import vqa_amd, recipe
    from cases import MFB_CASES
    from golden_util import mfb_inputs
    case = dict(MFB_CASES[-2], N=6, salt=92)
    cfg, img, q, glove, hard, soft = mfb_inputs(case, "cuda")
    model = vqa_amd.MFB(cfg)
    model.load_state_dict({k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"]))
                           for k, v in model.state_dict().items()})
    model = model.cuda().train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.unit_softmax = False                  # live attention: the encoder's gradients reach every tensor
    res = {}
    for hip in (True, False):
        model.use_hip_lstm = hip
        model.zero_grad(set_to_none=True)
        out = model.forward(img, q)
        torch.nn.CrossEntropyLoss()(out, hard).backward()
        res[hip] = (out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
    assert _rel(res[True][0], res[False][0]) <= 1e-5
    # the encoder-side tensors sit behind the signed square root's 0.5 |s|^-1/2: two fp32
    # summation orders of the same LSTM move them by a few 1e-3 in norm; everything else agrees to 5e-3
    # (ques_proj2.weight measured 2.3e-3); LstmBatchFn itself is checked against fp64 to 1e-4 above
    loose = ("word_embedding", "lstm", "ques_att", "ques_proj1", "img_conv1d", "co_att")
    gmax = max(float(g.norm()) for g in res[False][1].values())
    for k, g in res[False][1].items():
        if float(g.norm()) > 1e-6 * gmax:            # skip the mathematically-zero ones (biases in front of a softmax)
            tol = 2e-2 if k.startswith(loose) else 5e-3
            assert float((res[True][1][k] - g).norm()) <= tol * float(g.norm()) + 1e-9, k


@pytest.mark.parametrize("B,H", [(512, 1024), (128, 256), (256, 768)])
def test_fused_lstm_step_vs_fp64_and_bitwise_where_the_k_order_is_shared(B, H):
    """vqf_lstm_step_fwd (recurrent product with the cell in its epilogue, gate-interleaved W_hh rows) and the two-launch form
    vqf_gemm_f32(VQF_GEMM_ACCUM) + vqf_lstm_cell_fwd on the same operands.  Neither is the other's reference: EACH is bounded
    against an fp64 product + cell (activated gates, c, h; max-abs relative to the largest entry): 2e-6 * max(1, sqrt(H) / 8) for
    the fp32 accumulation over K = H + 5e-7 for the fast tanh / sigmoid (1e-7 absolute each).  Where both products run on the
    per-wave kernel they add k in the same order and must agree BIT for bit (the headline shape does); where the two-launch
    form is a split-K product the sums are re-associated and only the fp64 bounds apply (round 4 compared the two forms with
    each other and widened that tolerance after a red run: 2.2e-6 measured at K = 768, each side ~1e-6 from fp64).
    Then the module-level sequence (LstmBatchFn, T = 5) both ways incl. gradients, the same way."""
    import vqa_amd
    from node_harness import ref_lstm_seq, gemm_tol, LSTM_BATCH_TOL_F32
    ops = vqa_amd.ops
    assert ops.lstm_step_supported(B, H) and not ops.lstm_step_supported(B + 32, H) and not ops.lstm_step_supported(B, 64)
    g = torch.Generator().manual_seed(B + H)
    r = lambda *s: ((torch.rand(s, generator=g) * 2 - 1)).cuda()
    h_prev, w_hh, pre, c_prev = r(B, H), r(4 * H, H) * 0.05, r(B, 4 * H) * 1.5, r(B, H)
    step_tol = gemm_tol(H) + 5e-7
    same_order = True
    worst = 0.0
    on16 = False
    for cp in (c_prev, None):
        g1, c1, h1 = pre.clone(), torch.empty(B, H, device="cuda"), torch.empty(B, H, device="cuda")
        n16 = ops.stat("gemm_f32_n80")
        ops.lstm_step_fwd(h_prev, w_hh, g1, cp, c1, h1)
        on16 = ops.stat("gemm_f32_n80") == n16 + 1            # round 5: one round of 16x16x4 gate tiles (csrc/gemm_f32_n80.hip) took the step
        g3, c3, h3 = pre.clone(), torch.empty(B, H, device="cuda"), torch.empty(B, H, device="cuda")
        with ops.options(gemm_f32_n80=0):                     # the per-wave form of the fused step (rounds 3-4), always available
            ops.lstm_step_fwd(h_prev, w_hh, g3, cp, c3, h3)
        assert ops.stat("gemm_f32_n80") == n16 + (1 if on16 else 0)
        g2, c2, h2 = pre.clone(), torch.empty(B, H, device="cuda"), torch.empty(B, H, device="cuda")
        n0 = ops.stat("gemm_f32_wave")
        ops.gemm(h_prev, w_hh, out=g2, accumulate=True)
        same_order = ops.stat("gemm_f32_wave") == n0 + 1      # the two-launch product ran on the per-wave kernel: one k-ordered chain
        ops.lstm_cell_fwd(g2, cp, c2, h2)
        # fp64 product + cell (gate order i, f, g, o: torch.nn.LSTM's)
        p64 = pre.double() + h_prev.double() @ w_hh.double().t()
        i64, f64, gg64, o64 = p64.chunk(4, dim=1)
        act64 = torch.cat((torch.sigmoid(i64), torch.sigmoid(f64), torch.tanh(gg64), torch.sigmoid(o64)), 1)
        c64 = torch.sigmoid(i64) * torch.tanh(gg64) + (torch.sigmoid(f64) * cp.double() if cp is not None else 0.0)
        h64 = torch.sigmoid(o64) * torch.tanh(c64)
        for form, (ga, ca, ha) in (("fused step", (g1, c1, h1)), ("fused step, per-wave form", (g3, c3, h3)), ("product + cell", (g2, c2, h2))):
            for what, got, ref in (("gates", ga, act64), ("c", ca, c64), ("h", ha, h64)):
                e = _rel(got, ref)
                assert e <= step_tol, (form, what, e, step_tol)
                worst = max(worst, e)
        if same_order:
            assert torch.equal(g3, g2) and torch.equal(c3, c2) and torch.equal(h3, h2)
            if not on16:
                assert torch.equal(g1, g3) and torch.equal(c1, c3) and torch.equal(h1, h3)
    print("lstm step B=%d H=%d: all forms vs fp64 worst %.2e (bound %.2e); same k order: %s; gate-tile kernel: %s"
          % (B, H, worst, step_tol, same_order, on16))
    if B == 512 and H == 1024:
        assert same_order, "the headline shape's two-launch form is the per-wave kernel"
        assert on16, "the headline shape's fused step is one round of gate tiles"
    fn = vqa_amd.functions.LstmBatchFn
    x = r(5, B, 40)
    ps = [r(4 * H, 40) * 0.1, w_hh, r(4 * H) * 0.1, r(4 * H) * 0.1]
    wgt = torch.linspace(-1, 1, 5 * B * H, device="cuda").view(5, B, H)
    l64 = [t.double().requires_grad_() for t in ps]
    hs64 = ref_lstm_seq(x.double(), *l64, False)
    (hs64 * wgt.double()).sum().backward()
    res = []
    for fused in (True, False):
        fn.FUSED_STEP = fused
        try:
            leaves = [p.clone().requires_grad_() for p in ps]
            hs = fn.apply(x, *leaves)
            (hs * wgt).sum().backward()
            res.append((hs.detach(), [p.grad for p in leaves]))
        finally:
            fn.FUSED_STEP = True
        nrel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        assert nrel(hs.detach(), hs64.detach()) <= LSTM_BATCH_TOL_F32, ("fused" if fused else "two-launch", "hs")
        for a, b in zip(res[-1][1], l64):
            assert nrel(a, b.grad) <= LSTM_BATCH_TOL_F32, ("fused" if fused else "two-launch", "gradient", nrel(a, b.grad))
    if same_order and not on16:
        assert torch.equal(res[0][0], res[1][0])
        for a, b in zip(res[0][1], res[1][1]):
            assert torch.equal(a, b)
    elif same_order:
        # the gate-tile kernel adds k in its own order: the per-wave form of the fused step is the one that shares the two-launch
        # form's bits
        with ops.options(gemm_f32_n80=0):
            leaves = [p.clone().requires_grad_() for p in ps]
            hs = fn.apply(x, *leaves)
            (hs * wgt).sum().backward()
        assert torch.equal(hs.detach(), res[1][0])
        for a, b in zip([p.grad for p in leaves], res[1][1]):
            assert torch.equal(a, b)

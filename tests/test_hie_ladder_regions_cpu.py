"""Region counts of HieCoAttenLadder (forward((img, img_length), ...)), the part that needs no GPU: the masked restatement
tests/hie_ladder_regions_ref.py against the existing references -- the yardsticks -- run sample by sample on the image cut to its
count, the kernel references against the masked formulas on the padded shapes, and the call form's refusals."""
import inspect

import pytest
import torch

import hie_ladder_ref as R
import hie_ladder_len_ref as RL
import hie_ladder_alt_ref as RA
import hie_ladder_shared_ref as RS
import hie_ladder_regions_ref as RR
import hie_stream_ref as SR
import len_kernels_ref as LK

L, D, E, H, O, V, T = 7, 12, 16, 10, 6, 23, 6


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _sd(vqa, coatt, seed=0):
    m = vqa.HieCoAttenLadder(block_num=L, word_num=T, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, coatt=coatt)
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * 0.6 for k, v in m.state_dict().items()}


def _case(U, N, seed=1):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(U, L, D, generator=g, dtype=torch.float64)
    ids = torch.randint(1, V, (N, T), generator=g)
    lens = torch.randint(1, T + 1, (N,), generator=g)
    ids = torch.where(RL.valid_mask(lens, T), ids, torch.zeros_like(ids))
    masks = {"img": (torch.rand(U * L, E, generator=g) >= 0.5).to(torch.uint8),
             "word": (torch.rand(N * T, E, generator=g) >= 0.5).to(torch.uint8),
             "ans_w": (torch.rand(N, E, generator=g) >= 0.5).to(torch.uint8)}
    return img, ids, lens, masks


def _under(coatt, sd, img, ids, lens, masks):
    if coatt == "alternating":
        return RA.forward(sd, img, ids, lens, masks=masks)
    return R.forward(sd, img, ids, masks=masks) if lens is None else RL.forward(sd, img, ids, lens, masks=masks)


def _sample(coatt, sd, img, ids, lens, masks, counts, idx, n):
    """the existing reference on question n alone, its image cut to its count -> (logits (O), av (3, count), aq (3, T))"""
    u = n if idx is None else int(idx[n])
    c = int(counts[u])
    m = {"img": masks["img"].view(-1, L, E)[u, :c].reshape(c, E), "word": masks["word"].view(-1, T, E)[n].reshape(T, E),
         "ans_w": masks["ans_w"][n:n + 1]}
    out = _under(coatt, sd, img[u:u + 1, :c], ids[n:n + 1], None if lens is None else lens[n:n + 1], m)
    return out[0][0], out[1][0], out[2][0], c


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("with_lens", [False, True], ids=["no_q_length", "q_length"])
@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_each_sample_is_the_reference_on_its_cut_image(vqa, coatt, with_lens, shared):
    U, N = (3, 7) if shared else (5, 5)
    sd = _sd(vqa, coatt)
    img, ids, lens, masks = _case(U, N)
    lens = lens if with_lens else None
    idx = torch.tensor([2, 0, 0, 2, 0, 2, 0]) if shared else None              # image 1 without a question
    counts = torch.tensor([1, L, L - 1] if shared else [1, L, L - 1, 3, 4])
    junk = torch.where(RR.region_mask(counts, L).unsqueeze(2), img, torch.full_like(img, 1e3))      # the padding holds anything
    for im in (img, junk):
        logits, av, aq = RR.forward(sd, im, ids, counts, lens, idx, masks=masks, coatt=coatt)
        assert logits.shape == (N, O) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
        for n in range(N):
            rl, rav, raq, c = _sample(coatt, sd, img, ids, lens, masks, counts, idx, n)
            assert torch.equal(av[n, :, c:], torch.zeros(3, L - c, dtype=torch.float64))
            for got, ref in ((logits[n], rl), (av[n, :, :c], rav), (aq[n], raq)):
                assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), (n, c)


@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_full_counts_and_clamping(vqa, coatt):
    """counts all L: the bits of the references without counts; 0 and L + 5 act as 1 and L; int32 counts are int64 counts"""
    N = 4
    sd = _sd(vqa, coatt)
    img, ids, lens, masks = _case(N, N)
    full = torch.full((N,), L)
    a = RR.forward(sd, img, ids, full, lens, masks=masks, coatt=coatt)
    assert all(torch.equal(x, y) for x, y in zip(a, _under(coatt, sd, img, ids, lens, masks)))
    idx = torch.tensor([3, 0, 3, 1])
    b = RR.forward(sd, img, ids, full, lens, idx, masks=masks, coatt=coatt)
    assert all(torch.equal(x, y) for x, y in zip(b, RS.forward(sd, img, ids, idx, lens, masks=masks, coatt=coatt)))
    c = RR.forward(sd, img, ids, torch.tensor([1, L, 3, L]), lens, masks=masks, coatt=coatt)
    d = RR.forward(sd, img, ids, torch.tensor([0, L + 5, 3, L], dtype=torch.int32), lens, masks=masks, coatt=coatt)
    assert all(torch.equal(x, y) for x, y in zip(c, d)) and not torch.equal(a[0], c[0])


@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_img_emb_learns_nothing_from_padding(vqa, coatt):
    """the gradients are those of the samples on their cut images, summed: the padded rows of img reach no gradient"""
    N = 4
    img, ids, lens, masks = _case(N, N, seed=4)
    counts = torch.tensor([1, L, L - 1, 3])
    w = [torch.randn(s, generator=torch.Generator().manual_seed(11), dtype=torch.float64) for s in ((N, O), (N, 3, L), (N, 3, T))]
    grads = []
    for cut in (False, True):
        sd = {k: v.clone().requires_grad_(True) for k, v in _sd(vqa, coatt).items()}
        if not cut:
            junk = torch.where(RR.region_mask(counts, L).unsqueeze(2), img, torch.full_like(img, -7e2))
            out = RR.forward(sd, junk, ids, counts, lens, masks=masks, coatt=coatt)
            sum((o * x).sum() for o, x in zip(out, w)).backward()
        else:
            for n in range(N):
                rl, rav, raq, c = _sample(coatt, sd, img, ids, lens, masks, counts, None, n)
                ((rl * w[0][n]).sum() + (rav * w[1][n][:, :c]).sum() + (raq * w[2][n]).sum()).backward()
        grads.append({k: v.grad for k, v in sd.items()})
    assert float(grads[0]["img_emb.weight"].abs().max()) > 0
    for k in grads[0]:
        assert float((grads[0][k] - grads[1][k]).abs().max()) <= 1e-12 * max(1.0, float(grads[1][k].abs().max())), k


# ---- the kernel references --------------------------------------------------------------------------------------------------------
KN, KL, KE, KT, KLC = 5, 11, 8, 3, 4
COUNTS = [1, 4, 5, 10, 11]                      # a count on a chunk edge (4), one past it (5), a full sample, chunks left empty


def _cols(rlens, Lx):
    return (torch.arange(Lx).unsqueeze(0) < torch.tensor(RR.clamp_counts(rlens, Lx)).unsqueeze(1)).double()     # (N, L)


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("with_lens", [False, True])
def test_affinity_reference_is_the_masked_formula(epi, with_lens):
    """the truncated affinity == len_kernels_ref.affinity on the padded operands with the padded y rows zeroed, times the column
    mask (zero y rows give zero sums, tanh(0) = 0; epilogue 2 multiplies the zero sum)"""
    x1, y1 = LK.rnd((KN, KT, KE), 1, 0.5), LK.rnd((KN, KL, KE), 2, 0.5)
    x2, y2 = LK.rnd((KN, KT, KE), 3, 0.5), LK.rnd((KN, KL, KE), 4, 0.5)
    yprev = LK.rnd((KN, KT, KL), 5, 0.9)
    keep = (torch.rand((KN, KT, KL), generator=torch.Generator().manual_seed(6)) >= 0.3).to(torch.uint8)
    lens = [3, 1, 2, 3, 2] if with_lens else None
    cm = _cols(COUNTS, KL)
    for pairs in (1, 2):
        for k in ((None,) if epi == 0 else (None, keep)):
            kw = dict(x2=x2 if pairs == 2 else None, epi=epi, yprev=yprev if epi == 2 else None, keep=k, p=0.3 if k is not None else 0.0)
            got = RR.affinity(x1, RR.fill_rows(y1, COUNTS, float("nan")), COUNTS, lens,
                              y2=RR.fill_rows(y2, COUNTS, float("nan")) if pairs == 2 else None, **kw)
            ref = LK.affinity(x1, y1 * cm.unsqueeze(2), lens if with_lens else [KT] * KN,
                              y2=y2 * cm.unsqueeze(2) if pairs == 2 else None, **kw) * cm.unsqueeze(1)
            assert float((got - ref).abs().max()) <= 1e-12
            assert torch.equal(got * (1 - cm.unsqueeze(1)), torch.zeros_like(got))
    full = RR.affinity(x1, y1, [KL] * KN, lens, epi=epi, yprev=yprev if epi == 2 else None)
    assert torch.equal(full, LK.affinity(x1, y1, lens if with_lens else [KT] * KN, epi=epi, yprev=yprev if epi == 2 else None))


@pytest.mark.parametrize("Lc", [None, KLC])
def test_streaming_references_are_the_masked_formulas(Lc):
    """values: hie_stream_ref on the padded shapes with the padded rows of a / z and the padded columns of C / U zeroed (out times
    the row mask); bounds: never wider than those; counts = L: hie_stream_ref itself, value and bound"""
    a, z = LK.rnd((KN, KL, KE), 11, 1.5), LK.rnd((KN, KL, KE), 12)
    C, Vq = torch.tanh(LK.rnd((KN, KT, KL), 13, 3.0)), LK.rnd((KN, KT, KE), 14)
    keep = (torch.rand((KN, KL, KE), generator=torch.Generator().manual_seed(15)) >= 0.5).to(torch.uint8)
    rm = _cols(COUNTS, KL)
    am, zm, Cm = a * rm.unsqueeze(2), z * rm.unsqueeze(2), C * rm.unsqueeze(1)
    nan = float("nan")
    an, zn, Cn = RR.fill_rows(a, COUNTS, nan), RR.fill_rows(z, COUNTS, nan), RR.fill_rows(C, COUNTS, nan, dim=2)
    pairs = [(RR.hv_fwd(an, Cn, Vq, COUNTS, keep, 0.5, Lc=Lc), SR.hv_fwd(am, Cm, Vq, keep, 0.5, Lc=Lc)),
             (RR.rank_add(an, Cn, Vq, COUNTS, Lc=Lc), SR.rank_add(am, Cm, Vq, Lc=Lc)),
             (RR.rank_left(Cn, Vq, zn, COUNTS, Lc=Lc), SR.rank_left(Cm, Vq, zm, Lc=Lc))]
    for got, ref in pairs:
        assert set(got) == set(ref) - ({"slabs"} if Lc is None else set())
        for name in got:
            (gv, gb), (rv, rb) = got[name], ref[name]
            if name == "out":
                rv, rb = rv * rm.unsqueeze(2), rb * rm.unsqueeze(2)
                assert torch.equal(gv * (1 - rm.unsqueeze(2)), torch.zeros_like(gv)) and torch.equal(gb * (1 - rm.unsqueeze(2)), torch.zeros_like(gb))
            assert gv.shape == rv.shape and float((gv - rv).abs().max()) <= 1e-12, name
            assert bool((gb <= rb * (1 + 1e-12) + 1e-300).all()), name
    if Lc is not None:                                   # chunks beyond a count: zero slabs, zero column partials
        slabs = pairs[0][0]["slabs"][0]
        assert torch.equal(slabs[1:, 0], torch.zeros_like(slabs[1:, 0])) and float(slabs[0, 0].abs().max()) > 0
        assert torch.equal(pairs[1][0]["colpart"][0][2:, 2], torch.zeros(1, KE, dtype=torch.float64))
    fullc = [KL] * KN
    for got, ref in ((RR.hv_fwd(a, C, Vq, fullc, keep, 0.5, Lc=Lc), SR.hv_fwd(a, C, Vq, keep, 0.5, Lc=Lc)),
                     (RR.rank_add(a, C, Vq, fullc, Lc=Lc), SR.rank_add(a, C, Vq, Lc=Lc)),
                     (RR.rank_left(C, Vq, z, fullc, Lc=Lc), SR.rank_left(C, Vq, z, Lc=Lc))):
        for name in got:
            for k in range(2):
                assert float((got[name][k] - ref[name][k]).abs().max()) <= 1e-15 * max(1.0, float(ref[name][k].abs().max())), name
    # on top of padd (one chunk per sample): the plain sums plus padd, a bound one term wider
    if Lc is None:
        padd = LK.rnd((KN, KT, KE), 16)
        p0, p1 = RR.hv_fwd(a, C, Vq, COUNTS)["part"], RR.hv_fwd(a, C, Vq, COUNTS, padd=padd)["part"]
        assert float((p1[0] - p0[0] - padd).abs().max()) <= 1e-12 and bool((p1[1] >= p0[1]).all())


def test_zero_cols_reference():
    x = LK.rnd((2, KN, KT, KL), 21)
    got = RR.zero_cols(x, COUNTS, KN, KT)
    assert torch.equal(got, x * _cols(COUNTS, KL).view(1, KN, 1, KL))


# ---- the call form ----------------------------------------------------------------------------------------------------------------
def test_forward_takes_the_pair_and_refuses_what_mfb_refuses(vqa):
    m = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=32, hidden_size=10, output_size=6)
    assert list(inspect.signature(m.forward).parameters) == ["img_features", "que_features", "q_length", "img_index"]
    img, ids = torch.randn(2, 9, 12), torch.randint(0, 20, (2, 5))
    for bad in ((img,), (img, torch.ones(2), 3), [img, torch.ones(2), torch.ones(2)], (None, torch.ones(2))):
        with pytest.raises(vqa.VqfError, match="pair"):
            m(bad, ids)
    with pytest.raises(vqa.VqfError, match="GPU"):         # taken apart, then the usual refusal of CPU tensors: no CPU fallback
        m((img, torch.tensor([3, 9])), ids)
    assert "img_length" in vqa.HieCoAttenLadder.__doc__ and "Region counts" in inspect.getmodule(vqa.HieCoAttenLadder).__doc__
    assert "HieCoAttenLadder about right-padded" in vqa.predict.__doc__


def test_new_entry_points_refuse_null_counts_without_a_gpu(vqa):
    """NULL or misaligned rlens: VQF_E_BADARG before anything else is looked at (no launch, so no GPU is needed)"""
    lib = vqa.lib.load()
    Ex, N_, L_, T_ = 32, 2, 3, 3
    for rl in (None, 6):
        assert lib.vqf_hie_affinity_regions(None, Ex, None, Ex, None, 0, None, 0, 0, None, None, 0, 0.0, None, rl, N_, L_, Ex, T_, None,
                                            None) == -1
        assert lib.vqf_hie_affinity_levels_regions(None, Ex, 0, None, Ex, 0, None, 0, 0, None, 0, 0, 1, 0, None, None, rl, N_, L_, Ex, T_,
                                                   None, None) == -1
        assert lib.vqf_hie_hv_fwd_regions(None, Ex, None, None, Ex, None, 0, 0.0, rl, N_, L_, Ex, T_, None, Ex, None, Ex, None, 0, None) == -1
        assert lib.vqf_hie_rank_add_regions(None, Ex, None, None, Ex, rl, N_, L_, Ex, T_, None, Ex, None, 0, None) == -1
        assert lib.vqf_hie_rank_left_regions(None, None, Ex, None, Ex, rl, N_, L_, Ex, T_, None, Ex, None, Ex, None, 0, None, 0, None) == -1
        assert lib.vqf_zero_cols_len(None, rl, 6, T_, N_, L_, None) == -1

"""HieCoAtten's streaming passes (csrc/hie.hip: vqf_hie_hv_fwd, vqf_hie_head_bwd, vqf_hie_rank_add, vqf_hie_rank_left,
vqf_hie_slab_sum) called on their own and compared ELEMENT by element with the fp64 references of tests/hie_stream_ref.py:
|got - ref| <= bound at every element of out, the T-row sums, wpart and colpart -- not a norm over a weight gradient, which
dilutes exactly what these kernels can get wrong (one row per chunk or trip, a partial row in the wrong slot, a dropout draw
indexed by the strided position).  Operands are column blocks of wider buffers (and once contiguous), every destination lies in
a sentinel-filled buffer with guard rows and columns that must come back untouched.  The shapes are chosen per regime of the
launch logic (chunks per sample, threads per workgroup, row slots, the TMAX instantiation) and each test asserts its regime."""
import math
import pytest
import torch

import hie_stream_ref as R
from hie_stream_util import Report, _r, _views, _only, _vqa, SENT

pytestmark = pytest.mark.gpu
P = 0.5
SEED = 1234

# (N, L, E, T): (one chunk per sample?, threads per workgroup, row slots RS, what the shape is there for)
# The table and _threads_for restate the launch rule of csrc/hie.hip (chunks_for on 256 CUs, threads_for) so that every shape can
# ASSERT the regime it is there for.  A deliberate retune of that rule fails these asserts without any result being wrong: then
# regenerate the table (and pick shapes that reach every regime of the new rule); do not remove the asserts.
CASES = {
    (3, 196, 512, 14): (False, 512, 4, "S > 1, ragged last chunk, the model's shape"),
    (300, 196, 512, 14): (True, 1024, 8, "S == 1, 1024 threads, ragged last trip"),
    (4, 196, 512, 16): (False, 512, 4, "TMAX = 16, chunked"),
    (300, 50, 256, 15): (True, 1024, 16, "TMAX = 16, one workgroup per sample"),
    (5, 37, 64, 8): (False, 256, 16, "T = 8: last of TMAX = 8"),
    (5, 37, 64, 9): (False, 256, 16, "T = 9: first of TMAX = 14"),
    (2, 20, 64, 1): (False, 256, 16, "T = 1"),
    (2, 40, 1024, 6): (False, 1024, 4, "RS = 4: the fold's row slot takes one t per round"),
    (2, 3, 1024, 6): (True, 256, 1, "RS = 1: one row slot folds all four t of a round"),
    (3, 24, 4, 5): (False, 256, 256, "one column group, 256 row slots on 8-row chunks, wpart pitch 8"),
    (3, 24, 8, 16): (False, 256, 128, "two column groups, 128 row slots, TMAX = 16"),
    (300, 1, 64, 7): (True, 256, 16, "L = 1"),
    (2, 7, 128, 14): (True, 256, 8, "L < 8, RS > rows"),
    (300, 9, 32, 3): (True, 256, 32, "256-thread workgroups, RS > rows, S == 1"),
    (2, 1000, 256, 14): (False, 256, 4, "long L: 125 chunks"),
    (7, 197, 512, 14): (False, 512, 4, "odd L"),
}
BOTH_LAYOUTS = {(3, 196, 512, 14), (300, 9, 32, 3), (3, 24, 4, 5), (2, 7, 128, 14)}      # also run with contiguous operands


def _threads_for(E, Lc):
    """the launch rule of csrc/hie.hip: 1024 threads, halved down to 256 while a row slot would not get two rows per trip"""
    nt = 1024
    while nt > 256 and (nt // (E // 4)) * 2 > Lc:
        nt >>= 1
    return nt


def _inputs(N, L, E, T):
    """fp32 operands: tanh arguments spanning about [-3, 3]; C = a tanh; some logit-gradient rows exactly zero; some Hv entries
    saturated (|tanh| = 1 - eps, times 1 / (1 - p) under dropout)"""
    M, MT = N * L, N * T
    x = dict(a=_r((M, E), 1, 1.5), C=torch.tanh(_r((N, T, L), 2, 3.0)), V=_r((MT, E), 3, 3.0 / math.sqrt(T)), z=_r((M, E), 4),
             dl=_r((M,), 5), w=_r((E,), 6), padd=_r((MT, E), 7), dti=_r((MT, E), 8))
    x["dl"][[0, M // 2, M - 1]] = 0.0
    x["keep"] = (torch.rand((M, E), generator=torch.Generator().manual_seed(9)) >= P).to(torch.uint8)
    hv0 = torch.tanh(_r((M, E), 10, 3.0))
    sat = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    flat = hv0.view(-1)
    for j, i in enumerate(sorted({0, 1, (M * E) // 3, M * E - 2, M * E - 1})):
        flat[i] = sat if j % 2 == 0 else -sat
    x["hv0"] = hv0
    x["hv"] = hv0 * x["keep"].float() * (1.0 / (1.0 - P))       # (exact: a power of two)
    return x


def _run_shape(N, L, E, T, wide):
    vqa = _vqa()
    ops, VqfError = vqa.ops, vqa.lib.VqfError
    one, nt, RS, _ = CASES[(N, L, E, T)]
    # ---- the regime this shape is there for
    assert ops.hie_stream_supported(N, L, E, T)
    S = ops.hie_chunks(N, L)
    Lc = (L + S - 1) // S
    assert (S == 1) == one and (L + Lc - 1) // Lc == S, (S, Lc)
    assert _threads_for(E, Lc) == nt and nt // (E // 4) == RS, (_threads_for(E, Lc), Lc)
    if (N, L, E, T) in ((3, 196, 512, 14), (7, 197, 512, 14), (5, 37, 64, 8)):
        assert L % Lc != 0                                     # ragged last chunk
    if (N, L, E, T) == (300, 196, 512, 14):
        assert L % (2 * RS) not in (0,) and (L % (2 * RS)) <= RS      # last trip: the second row of a slot is missing
    M, MT = N * L, N * T
    rep = Report((N, L, E, T), wide)
    x = _inputs(N, L, E, T)
    d3 = lambda t, rows: t.double().view(N, rows, -1)
    C = x["C"].cuda()
    Cd, Vd, ad, zd = x["C"].double(), d3(x["V"], T), d3(x["a"], L), d3(x["z"], L)
    keepd = d3(x["keep"], L)
    keep = x["keep"].cuda()
    LcR = None if S == 1 else Lc
    _, (a, hv) = _views(M, E, wide)                            # [a | hv] like [Cv | img_]
    a.copy_(x["a"].cuda())
    _, (V, dti) = _views(MT, E, wide)                          # [que_ | dti]
    V.copy_(x["V"].cuda())
    dti.copy_(x["dti"].cuda())
    padd = x["padd"].cuda()

    def new_part():
        """(buffers, part for the launch, the (MT, E) strided destination of the final sums)"""
        fin_f, (_, fin) = _views(MT, E, True)
        if S == 1:
            return fin_f, fin, fin
        pf = torch.full((S * MT + 2, E), SENT, device="cuda")
        return [pf] + fin_f, pf[1:-1].view(S, MT, E), fin

    def sums(name, part, fin, res):
        """the T-row sums: S == 1 final in place; else the slabs, then vqf_hie_slab_sum of them (its own reference: the slabs as given)"""
        if S == 1:
            rep.check(name + ".part", fin, res["part"])
            return
        rep.check(name + ".slabs", part.view(S, N, T, E), res["slabs"])
        ops.hie_slab_sum(part, fin)
        rep.check("slab_sum.out", fin, R.slab_sum(part.cpu().double()))
        rep.check(name + ".part", fin, res["part"])

    # ---- hv_fwd: no dropout, explicit keep, Philox
    of, (_, out) = _views(M, E, wide)
    for tag, drop, again, kd in (("nodrop", (None, 0, 0.0), (None, SEED, 0.0), None), ("keep", (keep, 0, P), (keep, 0, P), keepd)):
        res = R.hv_fwd(ad, Cd, Vd, kd, P if kd is not None else 0.0, Lc=LcR)
        out.fill_(SENT)
        pf, part, fin = new_part()
        ops.hie_hv_fwd(a, C, V, drop, N, L, T, out, part)
        assert _only(of, out) and _only(pf, part if S > 1 else fin), "hv_fwd wrote outside its destination"
        rep.check("hv_fwd.out_" + tag, out, res["out"])
        if kd is not None:
            assert not bool(((out != 0) & (keep == 0)).any())
        saved, psaved = out.clone(), part.clone()
        sums("hv_fwd", part, fin, res)
        del res
        _, part2, _ = new_part()
        ops.hie_hv_fwd(a, C, V, again, N, L, T, out, part2)    # a second launch; for the plain pass with a seed and p = 0
        assert torch.equal(out, saved) and torch.equal(part2, psaved), "hv_fwd: a second launch / p = 0 differs (%s)" % tag
        del saved, psaved, part2, pf, part, fin
    _, part2, _ = new_part()
    ops.hie_hv_fwd(a, C, V, (None, SEED, P), N, L, T, out, part2)
    ones = torch.ones((M, E), device="cuda")
    ops.dropout(ones, seed=SEED, p_drop=P, out=ones)           # the flat kernel's mask over the LOGICAL (M, E) tensor
    pattern = (ones != 0).to(torch.uint8)
    del ones, part2
    assert torch.equal(out == 0, pattern == 0), "hv_fwd: Philox mask differs from ops.dropout's on the flat tensor"
    rep.check("hv_fwd.out_philox", out, R.hv_fwd(ad, Cd, Vd, d3(pattern.cpu(), L), P)["out"])

    # ---- head_bwd
    dl, w = x["dl"].cuda(), x["w"].cuda()
    dld, wd = x["dl"].double().view(N, L), x["w"].double()
    paddd = x["padd"].double().view(N, T, E)
    zero_rows = (dl == 0).nonzero().flatten()

    def new_head():
        """fresh sentinel destinations: (buffers of part, part, final sums, buffers of wpart, wpart)"""
        pf, part, fin = new_part()
        if wide:                                               # [colsum dCv | colsum dimg_ | dl^T Hv | sum dl | 0 0 0] as functions.py
            cp = torch.full((S * N + 2, 3 * E + 4), SENT, device="cuda")
            return pf, part, fin, [cp], cp[1:-1, 2 * E:]
        wf = torch.full((S * N + 2, E + 4), SENT, device="cuda")
        return pf, part, fin, [wf], wf[1:-1]

    def head_checks(tag, hvd, kd, pd, h, addd):
        pf, part, fin, wf, wpart = h
        res = R.head_bwd(hvd, dld, wd, Cd, kd, pd, part_add=addd, Lc=LcR)
        assert _only(of, out) and _only(pf, part if S > 1 else fin) and _only(wf, wpart), "head_bwd wrote outside its destination"
        rep.check("head_bwd.out_" + tag, out, res["out"])
        rep.check("head_bwd.wpart", wpart[:, :E], res["wpart"])
        rep.check("head_bwd.dlsum", wpart[:, E], res["dlsum"])
        assert bool((wpart[:, E + 1:] == 0).all()), "wpart tail must be [sum dl, 0, 0, 0]"
        assert bool((out[zero_rows] == 0).all())
        sums("head_bwd", part, fin, res)

    snap = lambda h: [out.clone(), h[1].clone(), h[4].clone()]
    same = lambda h, s: torch.equal(out, s[0]) and torch.equal(h[1], s[1]) and torch.equal(h[4], s[2])
    for tag, hvk, drop, again, kd, pd in (("keep", "hv", (keep, 0, P), (keep, 0, P), keepd, P),
                                          ("nodrop", "hv0", (None, 0, 0.0), (None, SEED, 0.0), None, 0.0)):
        hv.copy_(x[hvk].cuda())
        out.fill_(SENT)
        h = new_head()
        add = padd if (S == 1 and kd is not None) else None    # one chunk per sample: once on top of part_add, once without
        ops.hie_head_bwd(hv, dl, w, C, drop, N, L, T, out, h[1], h[4], part_add=add)
        s1 = snap(h)
        head_checks(tag, d3(x[hvk], L), kd, pd, h, paddd if add is not None else None)
        h2 = new_head()
        ops.hie_head_bwd(hv, dl, w, C, again, N, L, T, out, h2[1], h2[4], part_add=add)
        assert same(h2, s1), "head_bwd: a second launch / p = 0 differs (%s)" % tag
        del h2
        if kd is None:
            continue
        if S > 1:                                              # the slab sum on top of another tensor (dque_ = dti + C dtq)
            h[2].fill_(SENT)
            ops.hie_slab_sum(h[1], h[2], add=padd)
            rep.check("slab_sum.out_add", h[2], R.slab_sum(h[1].cpu().double(), x["padd"].double()))
            big = torch.empty((S * MT, 2 * E), device="cuda")
            with pytest.raises(VqfError, match="VQF_E_BADARG"):                      # several chunks: no part_add, no strided part
                ops.hie_head_bwd(hv, dl, w, C, drop, N, L, T, out, h[1], h[4], part_add=padd)
            with pytest.raises(VqfError, match="VQF_E_BADARG"):
                ops.hie_head_bwd(hv, dl, w, C, drop, N, L, T, out, big[:, E:], h[4])
            with pytest.raises(VqfError, match="VQF_E_BADARG"):
                ops.hie_hv_fwd(a, C, V, (None, 0, 0.0), N, L, T, out, big[:, E:])
            with pytest.raises(VqfError, match="VQF_E_BADARG"):
                ops.hie_rank_left(C, V, a, N, L, T, out, big[:, E:])
            assert torch.equal(out, s1[0]), "a refused launch wrote"
            del big
        else:                                                  # without part_add: the same out and wpart, the plain sums
            h0 = new_head()
            ops.hie_head_bwd(hv, dl, w, C, drop, N, L, T, out, h0[1], h0[4])
            rep.check("head_bwd.part", h0[2], R.head_bwd(d3(x[hvk], L), dld, wd, Cd, kd, pd)["part"])
            assert torch.equal(out, s1[0]) and torch.equal(h0[4], s1[2])
            del h0
        del s1
        hp = new_head()                                        # Philox == the same pattern passed as keep, bit for bit
        ops.hie_head_bwd(hv, dl, w, C, (None, SEED, P), N, L, T, out, hp[1], hp[4])
        sp = snap(hp)
        live = (pattern != 0) & (dl != 0)[:, None] & (w != 0)[None, :] & (hv < 1.9) & (hv > -1.9)
        assert not bool(((out != 0) & (pattern == 0)).any()) and not bool(((out == 0) & live).any()), "head_bwd: Philox zero pattern"
        del live
        hk = new_head()
        ops.hie_head_bwd(hv, dl, w, C, (pattern, 0, P), N, L, T, out, hk[1], hk[4])
        assert same(hk, sp), "head_bwd: Philox differs from its pattern passed as keep"
        del hp, hk, sp
    del pattern

    # ---- rank_add: out of place with colpart, without (same bits), in place (same bits)
    def new_colpart():
        if wide:
            cp = torch.full((S * N + 2, 3 * E + 4), SENT, device="cuda")
            return [cp], cp[1:-1, E:2 * E], cp[1:-1, :E]
        fs, (c1, c2) = _views(S * N, E, False)
        return fs, c1, c2

    res = R.rank_add(ad, Cd, d3(x["dti"], T), Lc=LcR)
    out.fill_(SENT)
    cf, cadd, _ = new_colpart()
    ops.hie_rank_add(a, C, dti, N, L, T, out, colpart=cadd)
    assert _only(of, out) and _only(cf, cadd), "rank_add wrote outside its destination"
    rep.check("rank_add.out", out, res["out"])
    rep.check("rank_add.colpart", cadd, res["colpart"])
    del res
    saved = out.clone()
    out.fill_(SENT)
    ops.hie_rank_add(a, C, dti, N, L, T, out)
    assert torch.equal(out, saved) and _only(of, out), "rank_add: colpart=None changes out"
    out.copy_(a)
    cf2, cadd2, _ = new_colpart()
    ops.hie_rank_add(out, C, dti, N, L, T, out, colpart=cadd2)
    assert torch.equal(out, saved) and torch.equal(cadd, cadd2) and _only(of, out), "rank_add: in place differs from out of place"
    del saved, cf, cadd, cf2, cadd2, of, out

    # ---- rank_left
    res = R.rank_left(Cd, Vd, zd, Lc=LcR)
    a.copy_(x["z"].cuda())                                     # z in the column block a held
    of, (out, _) = _views(M, E, wide)                          # dCv: the LEFT half of [dCv | dimg_]
    cf, _, cleft = new_colpart()
    pf, part, fin = new_part()
    ops.hie_rank_left(C, V, a, N, L, T, out, part, colpart=cleft)
    assert _only(of, out) and _only(cf, cleft) and _only(pf, part if S > 1 else fin), "rank_left wrote outside its destination"
    rep.check("rank_left.out", out, res["out"])
    rep.check("rank_left.colpart", cleft, res["colpart"])
    saved, psaved = out.clone(), part.clone()
    sums("rank_left", part, fin, res)
    out.fill_(SENT)
    _, part2, _ = new_part()
    ops.hie_rank_left(C, V, a, N, L, T, out, part2)
    assert torch.equal(out, saved) and torch.equal(part2, psaved), "rank_left: colpart=None / a second launch changes the result"
    rep.flush()


@pytest.mark.parametrize("N,L,E,T", sorted(CASES))
def test_streaming_passes_elementwise_vs_fp64(N, L, E, T):
    """Every ratio err / bound is asserted <= 1 (the measured ones, per pass, shape and output: profiles/hie_stream_parity.txt)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()                       # (what earlier tests of the process still hold)
    for wide in ((True, False) if (N, L, E, T) in BOTH_LAYOUTS else (True,)):
        _run_shape(N, L, E, T, wide)
    used = torch.cuda.max_memory_allocated() - base
    print("hie_stream %s peak device memory %.0f MB" % ((N, L, E, T), used / 1e6))
    assert used < 1e9, used


@pytest.mark.parametrize("N,L,E,T,why", [(2, 20, 96, 7, "E / 4 does not divide 256"), (2, 20, 64, 17, "T > 16"),
                                         (300, 196, 1024, 14, "the (T, E) + (T, L) images exceed 64 KB of LDS")])
def test_unsupported_shapes_are_refused_by_every_pass(N, L, E, T, why):
    vqa = _vqa()
    ops, VqfError = vqa.ops, vqa.lib.VqfError
    assert not ops.hie_stream_supported(N, L, E, T), why
    S = ops.hie_chunks(N, L)
    M, MT = N * L, N * T
    new = lambda *shape: torch.zeros(shape, device="cuda")
    a, out, C, V = new(M, E), new(M, E), new(N, T, L), new(MT, E)            # full-size operands: a wrong `yes` must not write out of bounds
    part, wpart, colpart = new(S, MT, E), new(S * N, E + 4), new(S * N, E)
    with pytest.raises(VqfError, match="VQF_E_UNSUPPORTED"):
        ops.hie_hv_fwd(a, C, V, (None, 0, 0.0), N, L, T, out, part)
    with pytest.raises(VqfError, match="VQF_E_UNSUPPORTED"):
        ops.hie_head_bwd(a, new(M), new(E), C, (None, 0, 0.0), N, L, T, out, part, wpart)
    with pytest.raises(VqfError, match="VQF_E_UNSUPPORTED"):
        ops.hie_rank_add(a, C, V, N, L, T, out, colpart=colpart)
    with pytest.raises(VqfError, match="VQF_E_UNSUPPORTED"):
        ops.hie_rank_left(C, V, a, N, L, T, out, part, colpart=colpart)
    assert float(out.abs().max()) == 0.0 and float(part.abs().max()) == 0.0


def test_slab_sum_on_its_own():
    """vqf_hie_slab_sum: S slabs (+ add) into a strided destination, guard columns untouched, S = 1 .. 25, R * W not a multiple of
    the workgroup"""
    ops = _vqa().ops
    rep = Report("slab_sum", True)
    for S, Rr, W in [(1, 7, 4), (3, 42, 512), (25, 98, 64), (125, 28, 256)]:
        part = _r((S, Rr, W), 50 + S, 2.0).cuda()
        addw = _r((Rr, 2 * W), 60 + S).cuda()
        for add in (None, addw[:, W:]):
            fulls, (_, out) = _views(Rr, W, True)
            ops.hie_slab_sum(part, out, add=add)
            assert _only(fulls, out)
            rep.check("slab_sum.S%d" % S, out, R.slab_sum(part.double().cpu(), None if add is None else add.double().cpu()))
    rep.flush()

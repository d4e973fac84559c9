"""The region-count entry points of csrc/hie.hip (vqf_hie_affinity_regions / _levels_regions, vqf_hie_hv_fwd_regions,
vqf_hie_rank_add_regions, vqf_hie_rank_left_regions, vqf_zero_cols_len) on their own, against the fp64 truncation references of
tests/hie_ladder_regions_ref.py (pinned on the CPU by tests/test_hie_ladder_regions_cpu.py).

Inside the ladder the padded rows hold finite values that no real result may depend on.  Here every case runs with different
contents behind the counts of every input -- seeded values in [-4, 4], then NaN, then 1e30 -- and the outputs must be the same
bits.  Further, per entry point:
  parity      the affinity per level and sample, max |err| / max |ref| at the tolerance tests/test_gpu_len_kernels.py applies to
              vqf_hie_affinity_len (2e-6; 5e-6 with the tanh epilogue); the streaming passes ELEMENT by element within the
              bounds tests/hie_stream_ref.py derives (on the cut operands), as tests/test_gpu_hie_stream.py checks the plain forms;
  zeros       outputs are pre-filled (7.0; the partial slabs with NaN): a padded row or column, the slab and the column partials
              of a chunk wholly behind the count must be exact zeros -- "not written" does not pass;
  counts = L  the bits of the existing entry point; the real rows of `out` are the plain pass's bits at any count;
  two runs    equal bits;
  refusals    a null or misaligned rlens: VQF_E_BADARG, nothing launched.
The measured err / bound of every case: profiles/hie_regions_parity.txt."""
import pytest
import torch

import hie_ladder_regions_ref as RR
import len_kernels_ref as LK
from golden_util import _report_parity
from hie_stream_util import Report, _r, _views, _only, SENT

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILLS = (("rand", 310), (NAN, 320), (1e30, 330))
P_DROP = 0.3


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


def _cu(x):
    return x.float().contiguous().cuda()


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


def _seven(*shape):
    return torch.full(shape, 7.0, device="cuda")


def _pad_cols(rlens, L):
    """(N, L) bool on the GPU: the padded regions"""
    return (torch.arange(L).unsqueeze(0) >= torch.tensor(RR.clamp_counts(rlens, L)).unsqueeze(1)).cuda()


class _Parity:
    def __init__(self, entry, shape):
        self.label, self.items = "hie_regions %-36s %s" % (entry, shape), {}

    def check(self, name, got, ref, tol):
        """ref (samples, ...) fp64: every (level and) sample judged on its own"""
        got = got.detach().cpu().double().reshape(ref.shape)
        errs = [float((got[n] - ref[n]).abs().max() / (ref[n].abs().max() + 1e-30)) for n in range(ref.shape[0])]
        for n, e in enumerate(errs):
            assert e <= tol, (self.label, name, "sample %d" % n, e, tol)
        self.items[name] = max(self.items.get(name, 0.0), max(errs) / tol)

    def flush(self):
        name = max(self.items, key=self.items.get)
        _report_parity(self.label, self.items[name], name, "  " + " ".join("%s=%.3f" % kv for kv in sorted(self.items.items())))


# ---- the affinity -------------------------------------------------------------------------------------------------------------------
def _aff_tol(epi):
    return 5e-6 if epi == 1 else 2e-6                  # tests/test_gpu_len_kernels.py, vqf_hie_affinity_len


def _align(x, y):
    """x (E) with the signs of y (E), in place.  The count-1 sample has T values, with T = 1 a single one, and the per-sample
    max norm then judges one fp32 dot product against itself: a cancelling sum cannot meet a relative 2e-6 in fp32 whatever
    the kernel (its error goes with K u sum|terms|, not with |sum|).  So that sample's question row 0 is sign-aligned with its
    region 0: the value is sum|x||y|, and the criterion there is the K-term relative bound it was set for."""
    x.copy_(x.abs() * torch.where(y < 0, -1.0, 1.0))


def _levels_case(ops, N, L, E, T, counts, lens, epi, combos, rep):
    """vqf_hie_affinity_levels_regions over (G, shared y, pairs) in `combos`, with the row counts `lens` or without"""
    padc = _pad_cols(counts, L)
    for G, shared, pairs in combos:
        assert ops.hie_affinity_levels_supported(N, L, E, T, G, pairs)
        lvy = 0 if shared else E
        x, y = LK.rnd((N, T, 2 * G * E), 130 + pairs, 0.5), LK.rnd((N, L, G * E), 140 + pairs, 0.5)   # level g's X at g 2E, Y at g E (or 0)
        x2, y2 = LK.rnd((N, T, G * E), 150, 0.5), LK.rnd((N, L, G * E + 4), 160, 0.5)
        yprev = LK.rnd((G, N, T, L), 170, 0.9)
        if counts[0] == 1:
            for g in range(G):
                _align(x[0, 0, 2 * g * E:2 * g * E + E], y[0, 0, g * lvy:g * lvy + E])
                _align(x2[0, 0, g * E:(g + 1) * E], y2[0, 0, g * lvy:g * lvy + E])

        def run(rl, fill, seed, ln=lens):
            fy = (lambda t, s, dim=1: t) if fill is None else (lambda t, s, dim=1: RR.fill_rows(t, counts, fill, seed + s, dim))
            fx = (lambda t, s: t) if (fill is None or ln is None) else (lambda t, s: LK.fill_padding(t, ln, "rand", seed + s))
            gx, gy = _cu(fx(x, 0)).view(N * T, -1), _cu(fy(y, 1)).view(N * L, -1)
            gx2 = _cu(fx(x2, 2)).view(N * T, -1) if pairs == 2 else None
            gy2 = _cu(fy(y2, 3)).view(N * L, -1) if pairs == 2 else None
            gp = _cu(torch.stack([fy(yprev[g], 4 + g, 2) for g in range(G)])) if epi == 2 else None
            out = _seven(G, N, T, L)
            ops.hie_affinity_levels(gx, 2 * E, gy, lvy, G, N, L, T, E, x2=gx2, lvx2=E, y2=gy2, lvy2=lvy, epi=epi, yprev=gp, out=out,
                                    lens=None if ln is None else _i32(ln), rlens=None if rl is None else _i32(rl))
            torch.cuda.synchronize()
            return out

        a = run(counts, *FILLS[0])
        for fill, seed in FILLS[1:] + FILLS[:1]:
            assert torch.equal(a, run(counts, fill, seed)), (G, shared, pairs, fill)
        ref = torch.stack([RR.affinity(x[:, :, 2 * g * E:2 * g * E + E], y[:, :, g * lvy:g * lvy + E], counts, lens,
                                       x2=x2[:, :, g * E:(g + 1) * E] if pairs == 2 else None,
                                       y2=y2[:, :, g * lvy:g * lvy + E] if pairs == 2 else None, epi=epi,
                                       yprev=yprev[g] if epi == 2 else None) for g in range(G)])
        rep.check("G%d_%s_pairs%d_%s" % (G, "shared" if shared else "separate", pairs, "rows" if lens else "norows"),
                  a.view(G * N, T, L), ref.view(G * N, T, L), _aff_tol(epi))
        assert bool((a.transpose(2, 3)[:, padc] == 0).all())                    # the padded columns of every level: exact zeros
        if lens is not None:
            padr = (torch.arange(T).unsqueeze(0) >= torch.tensor(LK.clamp_lens(lens, T)).unsqueeze(1)).cuda()
            assert bool((a[:, padr] == 0).all())
        plain = run(None, None, 0)                                               # the _len / plain form
        assert torch.equal(run([L] * N, None, 0), plain)
        live = ~padc.view(1, N, 1, L).expand_as(a)
        assert torch.equal(a[live], plain[live])                                 # the real columns: the existing form's bits


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("E", [32, 288])
@pytest.mark.parametrize("T", [1, 5, 16])
def test_hie_affinity_levels_regions(ops, T, E, epi):
    """L = 20: two 16-column groups, the second partial; counts before, at and behind the group edge.  E = 288: two k slabs."""
    N, L, counts = 5, 20, [1, 15, 16, 17, 20]
    rows = [min(t, T) for t in (T, 1, 3, T - 1 if T > 1 else 1, 2)]
    rep = _Parity("affinity_levels_regions epi %d" % epi, (N, L, E, T))
    combos = [(G, sh, pr) for G in (1, 3) for sh in (True, False) for pr in (1, 2)]
    for lens in (None, rows):
        _levels_case(ops, N, L, E, T, counts, lens, epi, combos, rep)
    rep.flush()


@pytest.mark.parametrize("epi", [0, 1, 2])
def test_hie_affinity_levels_regions_model_shape(ops, epi):
    """L = 196, E = 512: thirteen column groups over one workgroup's waves, the counts of a nearly empty and two nearly full images"""
    N, L, E, T, counts = 3, 196, 512, 14, [5, 196, 195]
    rep = _Parity("affinity_levels_regions epi %d" % epi, (N, L, E, T))
    _levels_case(ops, N, L, E, T, counts, None, epi, [(3, True, 1), (1, False, 2)], rep)
    _levels_case(ops, N, L, E, T, counts, [14, 1, 9], epi, [(3, True, 1), (1, False, 2)], rep)
    rep.flush()


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("T,E", [(5, 32), (16, 288)])
def test_hie_affinity_regions(ops, T, E, epi):
    """vqf_hie_affinity_regions (the dropout instantiation): explicit keep-mask and Philox; the mask of a real element does not
    depend on the counts (its index is that of the padded (N*T, L) tensor)"""
    N, L, counts = 5, 20, [1, 15, 16, 17, 20]
    padc = _pad_cols(counts, L)
    xw, yw = LK.rnd((N, T, 2 * E), 101, 0.5), LK.rnd((N, L, 2 * E), 102, 0.5)
    _align(xw[0, 0], yw[0, 0])                             # (the count-1 sample: see _align)
    yprev = LK.rnd((N, T, L), 103, 0.9)
    keep = (torch.rand((N, T, L), generator=torch.Generator().manual_seed(104)) >= P_DROP).to(torch.uint8)
    rows = [min(t, T) for t in (T, 1, 3, T - 1, 2)]
    rep = _Parity("affinity_regions epi %d" % epi, (N, L, E, T))
    gx = _cu(xw).view(N * T, 2 * E)
    for pairs in (1, 2):
        for lens in (None, rows):
            for mask in (("none",) if epi == 0 else ("keep", "philox")):
                drop = (None, 0, 0.0) if mask == "none" else (keep.cuda(), 0, P_DROP) if mask == "keep" else (None, 555, P_DROP)

                def run(rl, fill, seed, ep=epi, ln=lens):
                    gy = _cu(yw if fill is None else RR.fill_rows(yw, counts, fill, seed)).view(N * L, 2 * E)
                    gp = None if ep != 2 else _cu(yprev if fill is None else RR.fill_rows(yprev, counts, fill, seed + 1, 2))
                    out = _seven(N, T, L)
                    ops.hie_affinity(gx[:, :E], gy[:, :E], N, L, T, x2=gx[:, E:] if pairs == 2 else None,
                                     y2=gy[:, E:] if pairs == 2 else None, epi=ep, yprev=gp, drop=drop, out=out,
                                     lens=None if ln is None else _i32(ln), rlens=None if rl is None else _i32(rl))
                    torch.cuda.synchronize()
                    return out

                k64 = keep if mask == "keep" else None
                if mask == "philox":                    # the mask the plain kernel draws: the zeros of its dropped tanh
                    k64 = (run(None, None, 0, ep=1, ln=None) != 0).to(torch.uint8).cpu()
                a = run(counts, *FILLS[0])
                for fill, seed in FILLS[1:] + FILLS[:1]:
                    assert torch.equal(a, run(counts, fill, seed)), (pairs, mask, fill)
                ref = RR.affinity(xw[:, :, :E], yw[:, :, :E], counts, lens, x2=xw[:, :, E:] if pairs == 2 else None,
                                  y2=yw[:, :, E:] if pairs == 2 else None, epi=epi, yprev=yprev if epi == 2 else None, keep=k64,
                                  p=P_DROP if k64 is not None else 0.0)
                rep.check("pairs%d_%s_%s" % (pairs, mask, "rows" if lens else "norows"), a, ref, _aff_tol(epi))
                assert bool((a.transpose(1, 2)[padc] == 0).all())
                plain = run(None, None, 0)
                assert torch.equal(run([L] * N, None, 0), plain)
                live = ~padc.view(N, 1, L).expand_as(a)
                assert torch.equal(a[live], plain[live])
    rep.flush()


# ---- the streaming passes -----------------------------------------------------------------------------------------------------------
def _stream_inputs(N, L, E, T):
    M, MT = N * L, N * T
    x = dict(a=_r((M, E), 1, 1.5), C=torch.tanh(_r((N, T, L), 2, 3.0)), V=_r((MT, E), 3, 3.0 / T ** 0.5), z=_r((M, E), 4),
             padd=_r((MT, E), 7), dti=_r((MT, E), 8))
    x["keep"] = (torch.rand((M, E), generator=torch.Generator().manual_seed(9)) >= 0.5).to(torch.uint8)
    return x


def _run_stream(ops, N, L, E, T, counts, wide, with_padd=False):
    S = ops.hie_chunks(N, L)
    Lc = (L + S - 1) // S
    assert ops.hie_stream_supported(N, L, E, T) and (L + Lc - 1) // Lc == S
    assert not with_padd or S == 1
    LcR = None if S == 1 else Lc
    M, MT = N * L, N * T
    rows = RR.clamp_counts(counts, L)
    rl = _i32(counts)
    full = _i32([L] * N)
    rep = Report("regions %s%s" % ((N, L, E, T), " padd" if with_padd else ""), wide)
    x = _stream_inputs(N, L, E, T)
    d3 = lambda t, r: t.double().view(N, r, -1)
    Cd, Vd, ad, zd, dtid = x["C"].double(), d3(x["V"], T), d3(x["a"], L), d3(x["z"], L), d3(x["dti"], T)
    keepd, keep = d3(x["keep"], L), x["keep"].cuda()
    paddd = d3(x["padd"], T) if with_padd else None
    padd = x["padd"].cuda() if with_padd else None
    pk = {} if padd is None else {"part_add": padd}
    padrow = _pad_cols(counts, L).view(M)                                       # (N*L) bool: the padded rows
    empty = torch.tensor([[s * Lc >= r for r in rows] for s in range(S)])        # (S, N): chunks wholly behind the count
    if S > 1:
        assert bool(empty.any())
    _, (V, dti) = _views(MT, E, wide)
    V.copy_(x["V"].cuda())
    dti.copy_(x["dti"].cuda())

    def operands(fill, seed):
        """a, z, C with `fill` behind the counts (None: the operands as they are)"""
        f = lambda t, rws, s, dim=1: t if fill is None else RR.fill_rows(t.view(N, rws, -1) if dim == 1 else t, counts, fill, seed + s, dim)
        _, (a, z) = _views(M, E, wide)
        a.copy_(f(x["a"].double(), L, 0).float().view(M, E).cuda())
        z.copy_(f(x["z"].double(), L, 1).float().view(M, E).cuda())
        return a, z, f(x["C"].double(), T, 2, 2).float().contiguous().cuda()

    def new_part():
        fin_f, (_, fin) = _views(MT, E, True)
        if S == 1:
            return fin_f, fin, fin
        pf = torch.full((S * MT + 2, E), SENT, device="cuda")
        pf[1:-1] = NAN                                                          # a slab that is not written stays NaN
        return [pf] + fin_f, pf[1:-1].view(S, MT, E), fin

    def new_colpart():
        fs, (c1, _) = _views(S * N, E, wide)
        return fs, c1

    def sums(name, part, fin, res):
        if S == 1:
            rep.check(name + ".part", fin, res["part"])
            return
        rep.check(name + ".slabs", part.view(S, N, T, E), res["slabs"])
        assert bool((part.view(S, N, T, E)[empty.cuda()] == 0).all()), name + ": the slab of an empty chunk"
        rep.check(name + ".part", fin, res["part"])             # (vqf_hie_slab_sum of the slabs: done in passes())

    def passes(a, z, C, rlens, drop):
        """the three passes -> {name: tensor} (fresh sentinel destinations; every destination checked for stray writes)"""
        got = {}
        of, (_, out) = _views(M, E, wide)
        out.fill_(7.0)
        pf, part, fin = new_part()
        ops.hie_hv_fwd(a, C, V, drop, N, L, T, out, part, **({} if rlens is None else dict(rlens=rlens, **pk)))
        assert _only(of, out) and _only(pf, part if S > 1 else fin), "hv_fwd wrote outside its destination"
        if S > 1:
            ops.hie_slab_sum(part, fin)
        got.update(hv_out=out, hv_part=part, hv_fin=fin)
        of, (_, out) = _views(M, E, wide)
        out.fill_(7.0)
        cf, cp = new_colpart()
        ops.hie_rank_add(a, C, dti, N, L, T, out, colpart=cp, **({} if rlens is None else dict(rlens=rlens)))
        assert _only(of, out) and _only(cf, cp), "rank_add wrote outside its destination"
        got.update(add_out=out, add_col=cp)
        if rlens is not None:                                                   # in place, as the ladder runs it: the same bits
            of2, (_, io) = _views(M, E, wide)
            io.copy_(a)
            cf2, cp2 = new_colpart()
            ops.hie_rank_add(io, C, dti, N, L, T, io, colpart=cp2, rlens=rlens)
            assert torch.equal(io, out) and torch.equal(cp2, cp) and _only(of2, io), "rank_add in place differs"
        of, (out, _) = _views(M, E, wide)
        out.fill_(7.0)
        cf, cp = new_colpart()
        pf, part, fin = new_part()
        ops.hie_rank_left(C, V, z, N, L, T, out, part, colpart=cp, **({} if rlens is None else dict(rlens=rlens, **pk)))
        assert _only(of, out) and _only(cf, cp) and _only(pf, part if S > 1 else fin), "rank_left wrote outside its destination"
        if S > 1:
            ops.hie_slab_sum(part, fin)
        got.update(left_out=out, left_part=part, left_fin=fin, left_col=cp)
        torch.cuda.synchronize()
        return got

    same = lambda p, q: all(torch.equal(p[k], q[k]) for k in p)
    drop = (keep, 0, 0.5)
    a, z, C = operands(*FILLS[0])
    g = passes(a, z, C, rl, drop)
    # ---- element-wise parity, exact zeros behind the counts
    res = RR.hv_fwd(ad, Cd, Vd, counts, keepd, 0.5, Lc=LcR, padd=paddd)
    rep.check("hv_fwd.out", g["hv_out"], res["out"])
    sums("hv_fwd", g["hv_part"], g["hv_fin"], res)
    res = RR.rank_add(ad, Cd, dtid, counts, Lc=LcR)
    rep.check("rank_add.out", g["add_out"], res["out"])
    rep.check("rank_add.colpart", g["add_col"], res["colpart"])
    res = RR.rank_left(Cd, Vd, zd, counts, Lc=LcR, padd=paddd)
    rep.check("rank_left.out", g["left_out"], res["out"])
    rep.check("rank_left.colpart", g["left_col"], res["colpart"])
    sums("rank_left", g["left_part"], g["left_fin"], res)
    for k in ("hv_out", "add_out", "left_out"):
        assert bool((g[k][padrow] == 0).all()), k + ": a padded row is not an exact zero"
    for k in ("add_col", "left_col"):
        assert bool((g[k].reshape(S, N, E)[empty.cuda()] == 0).all()), k + ": the column partials of an empty chunk"
    # ---- what lies behind the counts changes no bit; two runs: equal bits
    for fill, seed in FILLS[1:] + FILLS[:1]:
        assert same(g, passes(*operands(fill, seed), rl, drop)), fill
    # ---- counts = L: the existing entry points' bits (without padd: they have none); the real rows of out at any count
    a0, z0, C0 = operands(None, 0)
    plain = passes(a0, z0, C0, None, drop)
    if not with_padd:
        assert same(plain, passes(a0, z0, C0, full, drop))
    for k in ("hv_out", "add_out", "left_out"):
        assert torch.equal(g[k][~padrow], plain[k][~padrow]), k
    # ---- Philox: the mask of a real element is the plain pass's (its index is that of the padded tensor)
    gp, pp = passes(a, z, C, rl, (None, 1234, 0.5)), passes(a0, z0, C0, None, (None, 1234, 0.5))
    assert torch.equal(gp["hv_out"][~padrow], pp["hv_out"][~padrow]) and bool((gp["hv_out"][padrow] == 0).all())
    assert not torch.equal(gp["hv_out"], g["hv_out"])
    rep.flush()


@pytest.mark.parametrize("T", [3, 14])
@pytest.mark.parametrize("wide", [True, False], ids=["blocks", "contig"])
def test_streaming_regions_chunked(ops, T, wide):
    """seven chunks of eight rows: count 1 leaves six chunks empty, 8 and 9 sit on a chunk edge, 9 splits a row pair"""
    N, L, E = 5, 50, 32
    assert ops.hie_chunks(N, L) > 1
    _run_stream(ops, N, L, E, T, [1, 8, 9, 49, 50], wide)


def test_streaming_regions_model_shape(ops):
    N, L, E, T = 3, 196, 512, 14
    assert ops.hie_chunks(N, L) > 1
    _run_stream(ops, N, L, E, T, [5, 196, 195], True)


@pytest.mark.parametrize("with_padd", [False, True], ids=["plain", "padd"])
def test_streaming_regions_one_workgroup_per_sample(ops, with_padd):
    N, L, E, T = 256, 20, 32, 3
    if torch.cuda.get_device_properties(0).multi_processor_count > N:
        pytest.skip("the device has more compute units than this batch has samples: no one-workgroup-per-sample form here")
    assert ops.hie_chunks(N, L) == 1
    _run_stream(ops, N, L, E, T, [1 + n % 20 for n in range(N)], True, with_padd=with_padd)


def test_counts_outside_the_range_are_clamped(ops):
    """the kernels clamp what they read: -3 and 0 walk no row, L + 9 walks L rows (the host clamps to [1, L] before)"""
    N, L, E, T = 5, 50, 32, 3
    _run_stream(ops, N, L, E, T, [0, -3, L + 9, 17, 50], True)


# ---- zero_cols_len, refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,N,T,L,counts", [(3, 5, 22, 20, [1, 15, 16, 17, 20]), (1, 3, 17, 196, [5, 196, 195]), (3, 1, 1, 1, [1])])
def test_zero_cols_len_is_exact(ops, G, N, T, L, counts):
    x = _r((G, N, T, L), 41, 2.0).cuda()
    x[0, 0, 0, L - 1] = NAN
    keep = ~_pad_cols(counts, L).view(1, N, 1, L)
    ref = torch.where(keep, x, torch.zeros((), device="cuda"))
    buf = torch.full((x.numel() + 8,), SENT, device="cuda")
    y = buf[4:-4].view(G, N, T, L)
    y.copy_(x)
    assert ops.zero_cols_len(y, _i32(counts), T, N, L) is y
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(y, nan=123.0), torch.nan_to_num(ref, nan=123.0))
    assert bool((buf[:4] == SENT).all()) and bool((buf[-4:] == SENT).all())


def test_null_and_misaligned_rlens_are_refused(ops):
    """every new entry point: rlens = NULL is VQF_E_BADARG, a pointer two bytes off alignment too; both before any launch (the
    outputs keep their 7.0).  The other arguments are valid, so a call that got through would stay in bounds."""
    N, T, E, L, G = 2, 3, 32, 3, 1
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    zin, out = torch.zeros(4096, device="cuda"), _seven(4096)
    odd = _i32([1] * 9)[1:]
    z, o, o2 = p(zin), p(out), p(out[2048:])
    calls = {
        "hie_affinity_regions": lambda rp: lib.vqf_hie_affinity_regions(z, E, z, E, None, 0, None, 0, 0, None, None, 0, 0.0, None, rp, N, L,
                                                                        E, T, o, st),
        "hie_affinity_levels_regions": lambda rp: lib.vqf_hie_affinity_levels_regions(z, E, 0, z, E, 0, None, 0, 0, None, 0, 0, G, 0, None,
                                                                                      None, rp, N, L, E, T, o, st),
        "hie_hv_fwd_regions": lambda rp: lib.vqf_hie_hv_fwd_regions(z, E, z, z, E, None, 0, 0.0, rp, N, L, E, T, o, E, o2, E, None, 0, st),
        "hie_rank_add_regions": lambda rp: lib.vqf_hie_rank_add_regions(z, E, z, z, E, rp, N, L, E, T, o, E, None, 0, st),
        "hie_rank_left_regions": lambda rp: lib.vqf_hie_rank_left_regions(z, z, E, z, E, rp, N, L, E, T, o, E, o2, E, None, 0, None, 0, st),
        "zero_cols_len": lambda rp: lib.vqf_zero_cols_len(o, rp, G * N * T, T, N, L, st),
    }
    for name, call in calls.items():
        assert call(None) == -1, name                   # VQF_E_BADARG
        assert call(odd.data_ptr() + 2) == -1, name
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    # with aligned counts the same argument lists are accepted: the refusals above were about rlens, not about another argument
    for name, call in calls.items():
        assert call(p(odd)) == 0, name
    torch.cuda.synchronize()
    # a misaligned row-count pointer next to good column counts is refused as well
    assert lib.vqf_hie_affinity_regions(z, E, z, E, None, 0, None, 0, 0, None, None, 0, 0.0, odd.data_ptr() + 2, p(odd), N, L, E, T, o, st) == -1

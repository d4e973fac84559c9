"""The MFB fusion kernels of csrc/fusion.hip on their own, every entry point of include/vqa_fusion.h "MFB fusion" called raw through
ops._lib() (the ops.mfb_fuse_* wrappers run vqf_l2_group_norm / vqf_scale_rows / vqf_rowdot around the kernel), element by element
against the fp64 reference tests/mfb_fuse_ref.py (pinned on the CPU by tests/test_mfb_fuse_ref_cpu.py).

The backward is tested as the function of its own operands the header defines (dY, Y, inv, coefA, coefB, P, pbias, q, cascade,
keep), not as the derivative of a chain: in those operands it is well conditioned whatever the signs.  Every case runs two data
sets, each with an explicit keep tensor and again with the in-kernel Philox draw (philox_ref.keep16 is the reference's mask):
  random   P, pbias, q, cascade, dY, dzdrop uniform in [-1, 1] (rounded to bf16 in the bf16-P forms), MIXED signs inside every
           pooling window: pooled sums cancel, change sign with the last addition, are small.  p = 0.3.  inv in [0.5, 2],
           coefA = inv, coefB in [-1, 1]; Y of the backward is the kernel forward's own R * inv of that case.
  exact    small integers and signed powers of two, p = 0.5 (scale exactly 2): every term, every pooled sum and every gradient sum
           is an fp32 number in any order (asserted: sum |terms| / granule < 2^24).  Pooled sums cancel to exactly 0 with kept
           elements, others are +-perfect squares, others not (asserted present).  Y = +-powers of two and some +-0.0.  Every output
           must equal the reference; R within the root's 2u, equal on the perfect squares and +0.0 bits on 0.
Bounds of the random set, per element, u = 2^-24, g(k) = (1 + u)^k - 1, the library being built with -ffp-contract=off so that the
roundings can be counted from the source (the k_* functions below, each from the fusion.hip lines it names):
  R        |s - s64| <= d = g(k_pool) A, A = sum |terms| of the pooled sum; the signed root is monotone, so R must lie in
           [ssqrt(s64 - d), ssqrt(s64 + d)], each end widened by 2u of its magnitude (a correctly rounded or 1-ulp sqrtf).  An
           interval, not a relative tolerance: tight where s is large, honest where s cancels or changes sign.  Reported:
           |R - R64| over the larger half-width.  d == 0 and s64 == 0: +0.0 bits.
  rowssq   the fp64 sum of a row's four partials against sum_o |s64|: g(k_pool + O - 1 + 3) sum_o A (any order of O terms, then the
           three additions of the partials); the partials of the waves that own no output are +0.0 bits.
  zdrop    g(k_term) |z64|.
  backward g(k) on the sum |terms| of each output, the k_* below; bf16 dP with fp32 bound b: b + 2^-8 (|ref| + b) -- store20 /
           own_store (:54, :142) round to nearest even onto bf16's 8 significand bits, spacing 2^-7 in [1, 2): half a spacing is
           2^-8 of the value (2^-9 would refuse the correctly rounded fp64 result itself: 1 + 2^-8 is 2^-8 from both neighbours).
           A dropped element and a Y == 0 element without dzdrop have a zero bound: exact zero.
Nothing is excluded from any comparison.  Every output lives in a buffer pre-filled with 7.0 with guard rows in front and behind,
the workspace has a guard behind it, every operand with rows sits between guard rows of NaN and the padded rows of P, dY and Y of
the layout forms hold NaN; every call is made twice and must give the same bits.  The worst err / bound per output is logged
(profiles/mfb_fuse_parity.txt)."""
import math

import pytest
import torch

import mfb_fuse_ref as FR
import reduce_kernels_ref as RR
from golden_util import _report_parity

pytestmark = pytest.mark.gpu

NAN = float("nan")
UNSUPPORTED = -3                                         # include/vqa_fusion.h VQF_E_UNSUPPORTED
GUARD = 2                                                # guard rows in front of and behind every row-shaped buffer
KINDS = ("exact", "random")
MASKS = ("keep", "philox")
PHILOX_SEED = 0x9E3779B97F4A7C15                         # both key words take part
BF16_U = 2.0 ** -8                                       # bf16's unit roundoff: 8 significand bits, round to nearest even


# ---- k: the roundings a term passes, counted from csrc/fusion.hip -------------------------------------------------------------------
def k_term(pbias, cascade, drop):
    """:277 (p + pb) * qq -- the sum rounds only when there is a bias; :281 * cc; :284 * sc (1.0f without dropout)"""
    return 1 + int(pbias) + int(cascade) + int(drop)


def k_pool(kt):
    """:289 (((p0 + p1) + p2) + p3) + p4"""
    return kt + 4


def k_rowssq(kt, O):
    """:291 ssq += a over the thread's four outputs, :305 wave_sum, :318 one partial per wave, added by the consumer: whatever the
    order, a term of a sum of O passes at most O - 1 additions; + 3 for the partials"""
    return k_pool(kt) + (O - 1) + 3


def k_ds():
    """:405 (ca * dy - cb * y) * (hi / ay): two products, the subtraction, the quotient (counted twice: a division one ulp off is
    allowed), the product; hi = 0.5f * inv is exact"""
    return 6


def k_dz(dzdrop, drop):
    """:410 (ds + dzx) * sc"""
    return k_ds() + int(dzdrop) + int(drop)


def k_dp(kz, cascade):
    """:412 dz * qq * cc, :416 dz * qq"""
    return kz + 1 + int(cascade)


def k_dq(kz, pbias, cascade, L):
    """:396 p += pb, :413 dz * p * cc / :417 dz * p, then dq += over the block's rows (:413) and vqf_group_reduce_f32 over the
    blocks (:693): in any order and for any LS a term of a sum of L passes at most L - 1 additions"""
    return kz + int(pbias) + 1 + int(cascade) + (L - 1)


def k_dcascade(kz, pbias):
    """:396, :414 dz * p * qq"""
    return kz + int(pbias) + 2


def k_dbias(kdp, rows):
    """:419 db += dp (or :519 over the image pass's rows), then vqf_colreduce_2stage (:696): a sum of one dP term per question row"""
    return kdp + (rows - 1)


def k_dp_image(drop, group):
    """:506-507 dz = ds * sc; dp += dz * qq over the image's questions"""
    return k_ds() + int(drop) + 1 + (group - 1)


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd.ops


class _Out:
    """an output (rows, cols) in a buffer pre-filled with 7.0, GUARD rows of it in front and behind"""

    def __init__(self, rows, cols, dtype=torch.float32):
        self.buf = torch.full((rows + 2 * GUARD, cols), 7.0, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + rows]

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == 7).all())

    def take(self):
        torch.cuda.synchronize()
        got = self.view.clone()
        self.view.fill_(7.0)
        assert bool((self.buf == 7).all()), "guard rows around an output were written"
        return got.cpu()


class _Ws:
    """a workspace of exactly `nbytes` with 64 guard floats of 7.0 behind it"""

    def __init__(self, nbytes):
        self.nbytes, self.n = int(nbytes), (int(nbytes) + 3) // 4
        self.buf = torch.full((self.n + 64,), 7.0, device="cuda")

    def ok(self):
        torch.cuda.synchronize()
        return bool((self.buf[self.n:] == 7).all())


def _in(x64, dtype=torch.float32):
    """x (rows, cols) fp64 -> the same values on the GPU between GUARD rows of NaN"""
    if x64 is None:
        return None
    x2 = x64.view(1, -1) if x64.dim() == 1 else x64
    buf = torch.full((x2.shape[0] + 2 * GUARD, x2.shape[1]), NAN, dtype=dtype, device="cuda")
    v = buf[GUARD:GUARD + x2.shape[0]]
    v.copy_(x2.to(dtype).cuda())
    return v


def _i32(x):
    return None if x is None else torch.as_tensor(x, dtype=torch.int32).contiguous().cuda()


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), \
            "two calls, different bits: " + k
    return True


def _plus_zero(x):
    return (x == 0) & ~torch.signbit(x)


class _Report:
    def __init__(self, entry, case):
        self.label, self.items, self.equal = "mfb_fuse %-22s %s" % (entry, case), {}, set()

    def _ratio(self, name, ratio):
        worst = float(ratio.max())
        print("%s %s: worst err/bound %.3f" % (self.label, name, worst))
        assert worst <= 1.0, (self.label, name, worst, int(ratio.reshape(-1).argmax()))
        self.items[name] = max(self.items.get(name, 0.0), worst)

    def bound(self, name, got, ref, bound):
        """per element |got - ref| <= bound (a zero bound: equal)"""
        got = got.double().reshape(ref.shape)
        err = (got - ref).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        self._ratio(name, torch.where(bound > 0, err / bound.clamp_min(1e-300),
                                      torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))))

    def equal_values(self, name, got, ref, sumabs, granule, dtype=torch.float32):
        """the exact data set: sum |terms| stays below 2^24 granules, so every order of every sum is exact"""
        assert float(sumabs.max()) / granule < 2 ** 24, (self.label, name, "the exact data set left the exact range")
        assert torch.equal(ref / granule, (ref / granule).round()), (self.label, name, "not a multiple of the granule")
        want = ref.float().to(dtype).reshape(got.shape)
        assert dtype != torch.float32 or torch.equal(want.double(), ref.reshape(got.shape)), (self.label, name, "reference not fp32")
        bad = ~(got == want)
        assert not bool(bad.any()), (self.label, name, "%d of %d elements differ, first at %d: got %r want %r" % (
            int(bad.sum()), bad.numel(), int(bad.reshape(-1).int().argmax()), float(got.reshape(-1)[bad.reshape(-1)][0]),
            float(want.reshape(-1)[bad.reshape(-1)][0])))
        self.equal.add(name)

    def root(self, name, got, s, d):
        """got must lie in [ssqrt(s - d), ssqrt(s + d)], each end widened by 2u of its magnitude; where that is the point 0: +0.0 bits"""
        got = got.double().reshape(s.shape)
        r64, lo, hi = FR.ssqrt(s), FR.ssqrt(s - d), FR.ssqrt(s + d)
        lo, hi = lo - 2 * FR.U * lo.abs(), hi + 2 * FR.U * hi.abs()
        outside = ~((got >= lo) & (got <= hi))
        assert not bool(outside.any()), (self.label, name, "%d of %d roots outside their interval, first at %d" % (
            int(outside.sum()), outside.numel(), int(outside.reshape(-1).int().argmax())))
        half = torch.maximum(hi - r64, r64 - lo)
        point = half == 0
        assert bool(_plus_zero(got[point]).all()), (self.label, name, "a pooled sum of exactly zero must give +0.0")
        self._ratio(name, torch.where(point, torch.zeros_like(half), (got - r64).abs() / half.clamp_min(1e-300)))

    def flush(self):
        name = max(self.items, key=self.items.get)
        _report_parity(self.label, self.items[name], name, "  " + " ".join("%s=%.3f" % kv for kv in sorted(self.items.items()))
                       + "  exact data: equal (%s)" % " ".join(sorted(self.equal)))


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def _spow2(shape, seed):
    """signed powers of two +-2^-1 .. +-2^1"""
    return RR.pow2(shape, seed, -1, 1) * torch.where(RR.ints(shape, seed + 1000, 0, 1) == 0, -1.0, 1.0)


def _case(form, N, L, O, **kw):
    c = dict(form=form, N=N, L=L, O=O, pbias=True, cascade=False, zdrop=False, dzdrop=False, dbias=True, opts={}, U=None, idx=None,
             lens=None, rb=(), fwd=True, nodbias_too=False)
    c.update(kw)
    c["id"] = "%s N%d L%d O%d%s%s%s%s%s%s%s" % (
        form, N, L, O, "" if c["pbias"] else " nopbias", " cascade" if c["cascade"] else "", " zdrop" if c["zdrop"] else "",
        " dzdrop" if c["dzdrop"] else "", " dbias and nodbias" if c["nodbias_too"] else "" if c["dbias"] else " nodbias", " lens" + "_".join(map(str, c["lens"])) if c["lens"] else "",
        "".join(" %s=%s" % kv for kv in sorted(c["opts"].items())))
    return c


def _build(c, kind, mask):
    """the fp64 operands of a case and the reference's keyword arguments"""
    N, L, O, form = c["N"], c["L"], c["O"], c["form"]
    W5 = 5 * O
    grouped, packed, rows, counted = "grouped" in form, "packed" in form, form == "packed_rows", "len" in form
    own = c["U"] if grouped else N
    owner = torch.tensor(c["idx"]) if grouped else torch.arange(N)
    lens_u = None if c["lens"] is None else torch.tensor(c["lens"])                       # per owner, as the kernel gets them
    cnt_u = torch.full((own,), L) if lens_u is None else lens_u.clamp(1, L)
    bf = form == "pbf16"
    seed = 1000 + 7 * O + L

    def val(shape, s, lo=-3, hi=3):
        if kind == "exact":
            return RR.ints(shape, seed + s, lo, hi)
        x = RR.rnd(shape, seed + s)
        return x.to(torch.bfloat16).double() if bf else x

    d = dict(kind=kind, p=0.5 if kind == "exact" else 0.3, own=own, owner=owner, cnt_u=cnt_u, grouped=grouped, packed=packed,
             rows=rows, counted=counted)
    Ppad = val((own * L, W5), 1).view(own, L, W5).clone()
    real_u = torch.arange(L)[None, :] < cnt_u[:, None]
    owned = torch.zeros(own, dtype=torch.bool)
    owned[owner] = True
    if packed:
        d["P"] = Ppad[real_u]
        roff = torch.zeros(own + 1, dtype=torch.int64)
        roff[1:] = torch.cumsum(cnt_u, 0)
        d["roff"] = roff
    else:
        Ppad[~real_u] = NAN                              # a padded row, and every row of an image without a question, is never read
        Ppad[~owned] = NAN
        d["P"] = Ppad.view(own * L, W5)
    d["pbias"] = val((W5,), 2, -2, 2) if c["pbias"] else None
    spow = kind == "exact"
    d["q"] = _spow2((N, W5), seed + 3) if spow else val((N, W5), 3)
    d["cascade"] = (_spow2((N * L, W5), seed + 4) if spow else val((N * L, W5), 4)) if c["cascade"] else None
    d["dzdrop"] = val((N * L, W5), 5) if c["dzdrop"] else None
    if kind == "exact":
        d["inv"], d["coefA"], d["coefB"] = RR.pow2((N,), seed + 6, -1, 1), RR.pow2((N,), seed + 7, -1, 1), _spow2((N,), seed + 8)
    else:
        d["inv"] = (1.25 + 0.75 * RR.rnd((N,), seed + 6)).float().double()
        d["coefA"], d["coefB"] = d["inv"].clone(), RR.rnd((N,), seed + 8)
    if mask == "keep":
        d["keep"] = torch.rand(N * L, W5, generator=torch.Generator().manual_seed(seed + 9)) >= d["p"]
        d["seed"] = 0
    else:
        d["keep"], d["seed"] = FR.philox_keep(N, L, O, PHILOX_SEED, d["p"]), PHILOX_SEED
    # the rows of R / dY / Y: (N L) in the padded coordinates, or the packed rows
    valid = torch.arange(L)[None, :] < cnt_u[owner][:, None]
    d["valid"] = valid
    d["sample_of_row"] = (torch.arange(N)[:, None].expand(N, L)[valid] if rows else torch.arange(N * L) // L)
    d["nrows"] = int(valid.sum()) if rows else N * L
    d["pad_rows"] = None if rows else ~valid.reshape(-1)
    d["dY"] = val((d["nrows"], O), 10)
    if kind == "exact":                                  # Y an operand of its own: +-powers of two, and +-0.0 in a sixth of the elements
        Y = _spow2((d["nrows"], O), seed + 11)
        z = RR.ints(Y.shape, seed + 12, 0, 11)
        Y[z == 0], Y[z == 1] = 0.0, -0.0
        d["Y"] = Y
    d["ref_kw"] = dict(idx=owner if grouped else None, lens=lens_u[owner] if (counted and not packed) else None,
                       roff=d.get("roff"), rows_out=rows)
    return d


def _nan_pad(x, d):
    """the padded rows of a per-row operand hold NaN"""
    if d["pad_rows"] is not None and (d["counted"] or d["packed"]):
        x = x.clone()
        x[d["pad_rows"]] = NAN
    return x


# ---- the raw calls ------------------------------------------------------------------------------------------------------------------
def _gpu_operands(c, d):
    g = dict(P=_in(d["P"], torch.bfloat16 if c["form"] == "pbf16" else torch.float32), pbias=_in(d["pbias"]), q=_in(d["q"]),
             cascade=_in(d["cascade"]), dzdrop=_in(d["dzdrop"]), inv=_in(d["inv"]), coefA=_in(d["coefA"]), coefB=_in(d["coefB"]),
             keep=d["keep"].to(torch.uint8).contiguous().cuda() if d["seed"] == 0 else None)
    owner = d["owner"]
    if d["grouped"]:
        order = torch.sort(owner, stable=True).indices
        off = torch.zeros(d["own"] + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.bincount(owner, minlength=d["own"]), 0)
        g["idx"], g["order"], g["grp_off"] = _i32(owner), _i32(order), _i32(off)
    if d["packed"]:
        g["roff"] = _i32(d["roff"])
    elif d["counted"]:
        lens_u = torch.tensor(c["lens"])
        g["lens_u"], g["lens_q"] = _i32(lens_u), _i32(lens_u[owner])
    return g


def _fwd(ops, c, d, g, ldrb=None):
    """one forward launch -> {R, rowssq (rows, 4), zdrop, Rb} on the CPU"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    N, L, O, form = c["N"], c["L"], c["O"], c["form"]
    R, ssq = _Out(d["nrows"], O), _Out(d["nrows"], 4)
    zd = _Out(N * L, 5 * O) if c["zdrop"] else None
    kp, seed, pd = p(g["keep"]), d["seed"], d["p"]
    U, Rtot = d["own"], d["P"].shape[0]
    res = {}
    if form in ("plain", "bf16dp"):
        rc = lib.vqf_mfb_fuse_fwd(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["cascade"]), kp, seed, pd, N, L, O, p(R.view), p(ssq.view),
                                  p(zd.view) if zd else None, st)
    elif form == "pbf16" and ldrb is None:
        rc = lib.vqf_mfb_fuse_fwd_pbf16(p(g["P"]), p(g["pbias"]), p(g["q"]), kp, seed, pd, N, L, O, p(R.view), p(ssq.view), st)
    elif form == "pbf16":
        Rb = _Out(N * L, ldrb, dtype=torch.bfloat16)
        rc = lib.vqf_mfb_fuse_fwd_pbf16_rb(p(g["P"]), p(g["pbias"]), p(g["q"]), kp, seed, pd, N, L, O, p(R.view), p(Rb.view), ldrb,
                                           p(ssq.view), st)
        res["Rb"] = Rb.take()
    elif form == "len":
        rc = lib.vqf_mfb_fuse_fwd_len(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["lens_q"]), kp, seed, pd, N, L, O, p(R.view), p(ssq.view), st)
    elif form == "grouped":
        rc = lib.vqf_mfb_fuse_fwd_grouped(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["idx"]), kp, seed, pd, N, U, L, O, p(R.view),
                                          p(ssq.view), st)
    elif form == "grouped_len":
        rc = lib.vqf_mfb_fuse_fwd_grouped_len(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["idx"]), p(g["lens_q"]), p(g["lens_u"]), kp, seed,
                                              pd, N, U, L, O, p(R.view), p(ssq.view), st)
    elif form == "packed":
        rc = lib.vqf_mfb_fuse_fwd_packed(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["roff"]), kp, seed, pd, N, Rtot, L, O, p(R.view),
                                         p(ssq.view), st)
    elif form == "grouped_packed":
        rc = lib.vqf_mfb_fuse_fwd_grouped_packed(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["idx"]), p(g["roff"]), kp, seed, pd, N, U, Rtot,
                                                 L, O, p(R.view), p(ssq.view), st)
    else:
        assert form == "packed_rows"
        rc = lib.vqf_mfb_fuse_fwd_packed_rows(p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["roff"]), kp, seed, pd, N, Rtot, L, O, p(R.view),
                                              p(ssq.view), st)
    assert rc == 0, (form, rc)
    res["R"], res["rowssq"] = R.take(), ssq.take()
    if zd:
        res["zdrop"] = zd.take()
    return res


def _bwd(ops, c, d, g, dY, Y, dbias):
    """one backward call -> {dP, dq, dcascade, dbiasP} on the CPU"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    N, L, O, form = c["N"], c["L"], c["O"], c["form"]
    W5 = 5 * O
    U, Rtot = d["own"], d["P"].shape[0]
    dP = _Out(d["P"].shape[0], W5, dtype=torch.bfloat16 if form in ("pbf16", "bf16dp") else torch.float32)
    dq, dc, db = _Out(N, W5), (_Out(N * L, W5) if c["cascade"] else None), _Out(1, W5)
    ws = _Ws(lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O) if d["grouped"] else lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O))
    kp, seed, pd = p(g["keep"]), d["seed"], d["p"]
    pdb = p(db.view) if dbias else None
    head = (p(dY), p(Y), p(g["inv"]), p(g["coefA"]), p(g["coefB"]), p(g["P"]), p(g["pbias"]), p(g["q"]))
    tail = (p(dP.view), p(dq.view), pdb, p(ws.buf), ws.nbytes, st)
    if form == "plain":
        rc = lib.vqf_mfb_fuse_bwd(p(dY), p(g["dzdrop"]), p(Y), p(g["inv"]), p(g["coefA"]), p(g["coefB"]), p(g["P"]), p(g["pbias"]),
                                  p(g["q"]), p(g["cascade"]), kp, seed, pd, N, L, O, p(dP.view), p(dq.view), p(dc.view) if dc else None,
                                  pdb, p(ws.buf), ws.nbytes, st)
    elif form == "pbf16":
        rc = lib.vqf_mfb_fuse_bwd_pbf16(*head, kp, seed, pd, N, L, O, *tail)
    elif form == "bf16dp":
        rc = lib.vqf_mfb_fuse_bwd_bf16dp(*head, kp, seed, pd, N, L, O, *tail)
    elif form == "len":
        rc = lib.vqf_mfb_fuse_bwd_len(*head, p(g["lens_q"]), kp, seed, pd, N, L, O, *tail)
    elif form == "grouped":
        rc = lib.vqf_mfb_fuse_bwd_grouped(*head, p(g["idx"]), p(g["order"]), p(g["grp_off"]), kp, seed, pd, N, U, L, O, *tail)
    elif form == "grouped_len":
        rc = lib.vqf_mfb_fuse_bwd_grouped_len(*head, p(g["idx"]), p(g["order"]), p(g["grp_off"]), p(g["lens_q"]), p(g["lens_u"]), kp, seed,
                                              pd, N, U, L, O, *tail)
    elif form == "packed":
        rc = lib.vqf_mfb_fuse_bwd_packed(*head, p(g["roff"]), kp, seed, pd, N, Rtot, L, O, *tail)
    elif form == "grouped_packed":
        rc = lib.vqf_mfb_fuse_bwd_grouped_packed(*head, p(g["idx"]), p(g["order"]), p(g["grp_off"]), p(g["roff"]), kp, seed, pd, N, U,
                                                 Rtot, L, O, *tail)
    else:
        assert form == "packed_rows"
        rc = lib.vqf_mfb_fuse_bwd_packed_rows(*head, p(g["roff"]), kp, seed, pd, N, Rtot, L, O, *tail)
    assert rc == 0, (form, rc)
    res = dict(dP=dP.take(), dq=dq.take())
    if dc:
        res["dcascade"] = dc.take()
    if dbias:
        res["dbiasP"] = db.take()
    else:
        assert db.untouched(), "dbiasP = NULL, and its buffer was written"
    assert ws.ok(), "the guard behind the workspace was written"
    return res


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _check_fwd(rep, c, d, got, tag):
    N, L, O = c["N"], c["L"], c["O"]
    exact = d["kind"] == "exact"
    ref = FR.fuse_fwd(d["P"], d["pbias"], d["q"], N, L, O, keep=d["keep"], p=d["p"], cascade=d["cascade"], **d["ref_kw"])
    kt = k_term(c["pbias"], c["cascade"], True)
    s, A = ref["s"], ref["A"]
    if exact:                                            # terms are multiples of 1/2: the pooled sums are exact
        assert float(A.max()) * 2 < 2 ** 24 and torch.equal(s * 2, (s * 2).round())
        if s.numel() >= 512:                             # the windows this data set is for
            root = s.abs().sqrt().float().double()
            square = (root * root == s.abs()) & (s != 0)
            assert int(((s == 0) & (A > 0)).sum()) > 0 and int(square.sum()) > 0 and int((~square & (s != 0)).sum()) > 0
            assert int((s < 0).sum()) > 0 and int((s > 0).sum()) > 0
        rep.root(tag + "R_exact_data", got["R"], s, torch.zeros_like(s))
        r32 = FR.ssqrt(s).float()
        square = r32.double() * r32.double() == s.abs()   # the perfect squares and 0: the root's own bits
        assert torch.equal(got["R"].reshape(s.shape)[square], r32[square]), (rep.label, "a perfect square's root is not exact")
        assert bool(_plus_zero(got["R"].reshape(s.shape)[s == 0]).all())
        rep.equal.add(tag + "R_squares")
    else:
        rep.root(tag + "R", got["R"], s, FR.g(k_pool(kt)) * A)
    part = got["rowssq"].double()
    idle = math.ceil(O / 4 / 64)                         # waves idle .. 3 own no output: O / 4 <= 192, 128, 64
    assert bool(_plus_zero(got["rowssq"][:, idle:]).all()), (rep.label, "a wave without an output left a partial that is not +0.0")
    assert bool((got["rowssq"] >= 0).all())
    if exact:
        rep.equal_values(tag + "rowssq", part.sum(1).float(), ref["rowabs"].reshape(-1), ref["rowA"], 0.5)
    else:
        rep.bound(tag + "rowssq", part.sum(1), ref["rowabs"].reshape(-1), FR.g(k_rowssq(kt, O)) * ref["rowA"].reshape(-1))
    if c["zdrop"]:
        z = ref["zdrop"].reshape(N * L, 5 * O)
        if exact:
            rep.equal_values(tag + "zdrop", got["zdrop"], z, z.abs(), 0.5)
        else:
            rep.bound(tag + "zdrop", got["zdrop"], z, FR.g(kt) * z.abs())
    if not d["rows"]:                                    # the padded rows: exact zeros, +0.0
        pad = d["pad_rows"]
        assert bool(_plus_zero(got["R"][pad]).all()) and bool(_plus_zero(got["rowssq"][pad]).all())
    return ref


def _check_bwd(rep, c, d, got, dY, Y, tag):
    N, L, O = c["N"], c["L"], c["O"]
    exact = d["kind"] == "exact"
    ref = FR.fuse_bwd(dY, Y, d["inv"], d["coefA"], d["coefB"], d["P"], d["pbias"], d["q"], N, L, O, keep=d["keep"], p=d["p"],
                      cascade=d["cascade"], dzdrop=d["dzdrop"], **d["ref_kw"])
    kz = k_dz(c["dzdrop"], True)
    kdp = k_dp(kz, c["cascade"])
    real_rows = int(d["valid"].sum())
    if d["grouped"]:
        group = int(torch.bincount(d["owner"]).max())
        kdp_out = k_dp_image(True, group)
        kdb = k_dbias(k_dp_image(True, 1), real_rows)
    else:
        kdp_out, kdb = kdp, k_dbias(kdp, real_rows)
    ks = dict(dP=kdp_out, dq=k_dq(kz, c["pbias"], c["cascade"], L), dcascade=k_dcascade(kz, c["pbias"]), dbiasP=kdb)
    bf16 = got["dP"].dtype == torch.bfloat16
    for name in ("dP", "dq", "dcascade", "dbiasP"):
        if name not in got:
            continue
        r, a = ref[name].reshape(got[name].shape), ref[name + "_abs"].reshape(got[name].shape)
        assert not bool(torch.isnan(got[name]).any()), (rep.label, name, "NaN: a padded row was read")
        if exact:                                        # every term is a multiple of 2^-6 (the docstring of test_fuse counts it)
            rep.equal_values(tag + name, got[name], r, a, 2.0 ** -6, dtype=got[name].dtype)
        else:
            b = FR.g(ks[name]) * a
            if bf16 and name == "dP":
                b = b + BF16_U * (r.abs() + b)
            rep.bound(tag + name, got[name], r, b)
    # exact zeros: a dropped element, and a Y == 0 element without dzdrop (a zero bound above; here spelled out on dP)
    if not d["grouped"]:
        assert bool((got["dP"].double()[ref["dP_abs"] == 0] == 0).all())
    return ref


def _run_case(ops, c, entry):
    rep = _Report(entry, c["id"])
    O = c["O"]
    with ops.options(**c["opts"]):
        for kind in KINDS:
            for mask in MASKS:
                d = _build(c, kind, mask)
                g = _gpu_operands(c, d)
                tag = "" if mask == "keep" else "philox_"
                if c["fwd"]:
                    f = _fwd(ops, c, d, g)
                    assert _same(f, _fwd(ops, c, d, g))
                    _check_fwd(rep, c, d, f, tag)
                    for ldrb in c["rb"]:                 # the bf16 copy: the RNE bits of the kernel's own fp32 R, zero bits in the pad
                        fb = _fwd(ops, c, d, g, ldrb)
                        assert _same(fb, _fwd(ops, c, d, g, ldrb))
                        assert torch.equal(fb["R"], f["R"]) and torch.equal(fb["rowssq"], f["rowssq"])
                        assert torch.equal(fb["Rb"][:, :O].contiguous().view(torch.int16), f["R"].to(torch.bfloat16).view(torch.int16))
                        assert bool((fb["Rb"][:, O:].contiguous().view(torch.int16) == 0).all())
                        rep.equal.add(tag + "R_bf16_ld%d" % ldrb)
                if kind == "exact" or not c["fwd"]:
                    Y = d["Y"] if kind == "exact" else _random_y(d, O)
                else:                                    # the kernel forward's own R * inv
                    Y = (f["R"].double() * d["inv"][d["sample_of_row"]][:, None]).float().double()
                dY, Y = _nan_pad(d["dY"], d), _nan_pad(Y, d)
                gdY, gY = _in(dY), _in(Y)
                b = _bwd(ops, c, d, g, gdY, gY, c["dbias"])
                assert _same(b, _bwd(ops, c, d, g, gdY, gY, c["dbias"]))
                _check_bwd(rep, c, d, b, dY, Y, tag)
                if c["nodbias_too"]:                     # dbiasP = NULL: the same dP / dq bits
                    nb = _bwd(ops, c, d, g, gdY, gY, False)
                    for name in nb:
                        assert torch.equal(nb[name].view(torch.uint8), b[name].view(torch.uint8)), name
    rep.flush()


def _random_y(d, O):
    """Y as an operand of its own (a backward without a forward): 0.25 <= |Y| <= 1.25 and a few +-0.0"""
    y = RR.rnd((d["nrows"], O), 77)
    y = torch.where(y < 0, y - 0.25, y + 0.25).float().double()
    z = RR.ints(y.shape, 78, 0, 15)
    y[z == 0], y[z == 1] = 0.0, -0.0
    return y


# ---- the plain form: O classes, row walks, access forms, optional operands --------------------------------------------------------
FULL = dict(cascade=True, zdrop=True, dzdrop=True)
# O: 4 one thread, three idle waves; 12: 5 O % 8 == 4, rows alternate Philox phase; 260: one active lane in wave 1; 1000: 58 active
# lanes in wave 3, the el < W5 guards of raw_load / own_store trip; 1024: every lane active
O_CLASSES = (4, 12, 260, 1000, 1024)
PLAIN_CASES = [_case("plain", 2, 7, O, **FULL) for O in O_CLASSES]                                     # L = 7, the default splits
PLAIN_CASES += [_case("plain", 2, 7, O, opts=dict(fuse_coal=coal), **FULL) for O in O_CLASSES for coal in (0, 1)]
PLAIN_CASES += [
    _case("plain", 3, 1, 260, **FULL),                                                                   # L = 1: the direct dq, LS == 1
    _case("plain", 2, 33, 260, **FULL),                                                                  # the forward's default split is 2
    # L = 7 in 2 and in 3 blocks: they walk 4 / 3 and 3 / 2 / 2 rows; COAL = 1's prefetch has a next row in some blocks only
    _case("plain", 2, 7, 260, opts=dict(fuse_ls=2, fuse_ls_bwd=2), **FULL),
    _case("plain", 2, 7, 260, opts=dict(fuse_ls=3, fuse_ls_bwd=3), **FULL),
    _case("plain", 2, 7, 1000, opts=dict(fuse_ls=2, fuse_ls_bwd=2, fuse_coal=1), **FULL),
    _case("plain", 2, 7, 1000, opts=dict(fuse_ls=3, fuse_ls_bwd=3, fuse_coal=1), **FULL),
    _case("plain", 2, 7, 260, opts=dict(fuse_ls=3, fuse_ls_bwd=3, fuse_coal=0), **FULL),
    _case("plain", 2, 7, 260, pbias=False, **FULL),
    _case("plain", 2, 7, 260, dzdrop=True, zdrop=True),                                                  # dzdrop without cascade
    _case("plain", 2, 7, 260, nodbias_too=True),                                                         # the image fusion's call
    _case("plain", 2, 7, 1000, nodbias_too=True, **FULL),
    _case("plain", 2, 7, 12, pbias=False, dbias=False),
]


@pytest.mark.parametrize("c", PLAIN_CASES, ids=[c["id"] for c in PLAIN_CASES])
def test_fuse_plain(ops, c):
    """Exact data, backward: coefA dY is a multiple of 1/2 up to 6, coefB Y of 1/4 up to 4, hi / |Y| in 2^-3 .. 2, so dS is a
    multiple of 2^-5 up to 20; + dzdrop (integers up to 3), * 2: dz a multiple of 2^-4 up to 46; q and cascade +-2^-1 .. 2: dP a
    multiple of 2^-6 up to 184, a term of dq / dcascade (|P + pbias| <= 5) a multiple of 2^-5 up to 460 -- equal_values asserts
    that every sum stays below 2^24 granules of 2^-6."""
    if "fuse_ls" in c["opts"]:
        assert c["opts"]["fuse_ls"] <= c["L"] and c["L"] % c["opts"]["fuse_ls"] != 0                     # an uneven walk
    _run_case(ops, c, "fwd/bwd")


# ---- bf16 P / dP ---------------------------------------------------------------------------------------------------------------------
BF16_CASES = [
    # O = 1000: the coalesced access (5 O % 8 == 0); O = 12: 5 O % 8 == 4, the direct access
    _case("pbf16", 2, 7, 1000, rb=(1024, 1000)),         # ldrb = O rounded up to 32, and an ldrb without a pad column
    _case("pbf16", 2, 7, 12, rb=(32, 12)),
    _case("pbf16", 2, 7, 1000, opts=dict(fuse_coal=0)),
    _case("pbf16", 2, 7, 264, pbias=False, dbias=False, rb=(288,)),
    _case("bf16dp", 2, 7, 1000, nodbias_too=True),
    _case("bf16dp", 2, 7, 12),
    _case("bf16dp", 2, 7, 1000, opts=dict(fuse_coal=0)),
]


@pytest.mark.parametrize("c", BF16_CASES, ids=[c["id"] for c in BF16_CASES])
def test_fuse_bf16(ops, c):
    """pbf16: vqf_mfb_fuse_fwd_pbf16 / _fwd_pbf16_rb / _bwd_pbf16 (P and every other operand hold bf16 values); bf16dp: the fp32
    forward and vqf_mfb_fuse_bwd_bf16dp.  dq and dbiasP are fp32 sums of the unrounded values: the fp32 bounds."""
    assert ((5 * c["O"]) % 8 == 0) == (c["O"] != 12)      # fusion.hip:676 / :712: whole 16-byte pieces of bf16, or the direct access
    _run_case(ops, c, "bf16 fwd/bwd")


# ---- the layout forms ---------------------------------------------------------------------------------------------------------------
IDX = [2, 0, 2, 2]                                       # image 1 has no question, image 2 has three
LAYOUT_CASES = []
for O in (260, 12):
    LAYOUT_CASES += [
        # counts 1, L, one in between, and two values outside [1, L] that the kernel clamps; L odd: the image pass's last row pair
        # straddles L
        _case("len", 5, 5, O, lens=[1, 5, 3, 9, 0], nodbias_too=True),
        _case("grouped", 4, 5, O, U=3, idx=IDX),
        _case("grouped_len", 4, 5, O, U=3, idx=IDX, lens=[4, 2, 3]),          # image 2: count 3, its pair (2, 3) straddles the count
        _case("packed", 4, 5, O, lens=[1, 5, 3, 4]),
        _case("grouped_packed", 4, 5, O, U=3, idx=IDX, lens=[4, 2, 3]),
        _case("packed_rows", 4, 5, O, lens=[2, 5, 1, 3]),
    ]
LAYOUT_CASES += [_case("len", 3, 7, 1000, lens=[7, 2, 5], opts=dict(fuse_ls=3, fuse_ls_bwd=3)),          # blocks without a real row
                 _case("grouped_len", 4, 5, 260, U=3, idx=IDX, lens=[4, 2, 3], opts=dict(fuse_coal=0), dbias=False)]


@pytest.mark.parametrize("c", LAYOUT_CASES, ids=[c["id"] for c in LAYOUT_CASES])
def test_fuse_layouts(ops, c):
    """_len, _grouped, _grouped_len, _packed, _grouped_packed, _packed_rows against the same reference through idx / lens / roff.
    The padded rows of P, dY and Y hold NaN and every row of the image without a question too; padded R / dP rows are exact
    zeros; a packed tensor has no row outside its span, and the guard rows around every output keep their 7.0."""
    _run_case(ops, c, "layout fwd/bwd")


# ---- O > 1024: the backward's second trip of the t += 256 loop ---------------------------------------------------------------------
def test_fuse_bwd_O_1028(ops):
    """vqf_mfb_fuse_bwd takes every O % 4 == 0 (fusion.hip:369: threads 0 .. 255 walk t, t + 256 on the direct access), the forward
    refuses O > 1024: Y is an operand, so the case needs no forward."""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    N, L, O = 2, 3, 1028
    R, ssq = _Out(N * L, O), _Out(N * L, 4)
    z = torch.zeros(N * L * 5 * O, device="cuda")
    assert lib.vqf_mfb_fuse_fwd(p(z), None, p(z), None, None, 0, 0.0, N, L, O, p(R.view), p(ssq.view), None, st) == UNSUPPORTED
    assert R.untouched() and ssq.untouched()
    _run_case(ops, _case("plain", N, L, O, fwd=False, **FULL), "bwd O 1028")
    _run_case(ops, _case("plain", N, L, O, fwd=False, dbias=False, opts=dict(fuse_ls_bwd=2)), "bwd O 1028")

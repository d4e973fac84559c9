"""The ten public MFB fusion wrappers of host/ops.py (mfb_fuse_fwd / _bwd and their _grouped, _packed, _packed_rows pairs) against
the 30 launch entry points they reach, at the smallest shapes that tell the forms apart:

  N = 3, L = 7, O = 8 (5 O = 40: the coalesced bf16 access), counts (7, 1, 4): R = 12 packed rows; shared images: U = 2,
  idx = (1, 0, 1), counts per image (7, 4): R = 11; a bf16 P / dP has pad_rows(R) = 32 rows; p_drop = 0.25 from a Philox seed, and
  one case per direction with a keep mask; mixed-sign finite data.

Per entry:
  routing      ops._lib is replaced by a proxy that records the names it is asked for; the sequence (without the *_ws_bytes and
               *_supported queries) is the one written out here;
  marshalling  the same entry is called raw, with the argument list written out by hand on the same inputs, and every output of the
               wrapper has the raw call's bits (torch.equal; no tolerance: same kernel, same operands, and the kernels give the same
               bits on every run).  The bf16 copy of R and a bf16 dP are the wrapper's allocations: their rows behind the real ones
               are +0.0.
The plain entry's variants: cascade + want_zdrop, dzdrop, lin= against the rowdot head, normalise both ways.
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

N, L, O, U, G = 3, 7, 8, 2, 2
W = 5 * O
NL = N * L
COUNTS, R = (7, 1, 4), 12                     # per sample; roff (0, 7, 8, 12)
IDX, COUNTS_U, RU = (1, 0, 1), (7, 4), 11     # per image; roff_u (0, 7, 11); order (1, 0, 2), grp_off (0, 1, 3)
PAD = 32                                      # pad_rows of 12, 11 and 21
LDRB = 32                                     # O rounded up to 32
SEED, P_DROP = 20240607, 0.25

NORM_TAIL = ["vqf_l2_group_norm"]
NORM_TAIL_ROWS = ["vqf_l2_group_norm_packed"]
COEF_HEAD = ["vqf_rowdot", "vqf_l2_norm_bwd_coef"]
COEF_HEAD_LIN = ["vqf_l2_norm_bwd_coef_lin"]
COEF_HEAD_ROWS = ["vqf_rowdot", "vqf_l2_norm_bwd_coef_packed"]
COEF_HEAD_ROWS_LIN = ["vqf_l2_norm_bwd_coef_lin_packed"]


@pytest.fixture(scope="module")
def ops():
    import vqa_amd
    vqa_amd.lib.load()
    assert vqa_amd.ops.pad_rows(R) == vqa_amd.ops.pad_rows(RU) == vqa_amd.ops.pad_rows(NL) == PAD
    return vqa_amd.ops


@pytest.fixture(scope="module")
def D():
    """the operands, made once and never written"""
    g = torch.Generator().manual_seed(7)

    def rnd(*shape, dtype=torch.float32):
        return (torch.rand(shape, generator=g) * 2 - 1).to(dtype).cuda()

    def i32(*v):
        return torch.tensor(v, dtype=torch.int32).cuda()

    d = types.SimpleNamespace()
    d.P, d.Pb = rnd(NL, W), rnd(PAD, W, dtype=torch.bfloat16)              # plain / counted (a bf16 P: 32 rows, 21 of them real)
    d.Pbn = d.Pb[:NL]                                                      # the plain form: a bf16 P of N*L rows
    d.Pp, d.Ppb = rnd(R, W), rnd(PAD, W, dtype=torch.bfloat16)             # packed (12 real rows)
    d.Pu, d.Pup = rnd(U * L, W), rnd(RU, W)                                # shared images: padded and packed
    d.q, d.pbias, d.cascade = rnd(N, W), rnd(W), rnd(NL, W)
    d.dY, d.dYr, d.dzdrop = rnd(NL, O), rnd(R, O), rnd(NL, W)
    d.dl, d.lin, d.dlr, d.linr = rnd(NL, G), rnd(NL, G), rnd(R, G), rnd(R, G)
    d.keep = (torch.rand((NL, W), generator=g) >= P_DROP).to(torch.uint8).cuda()
    d.lens, d.roff = i32(*COUNTS), i32(0, 7, 8, 12)
    d.idx, d.order, d.grp_off = i32(*IDX), i32(1, 0, 2), i32(0, 1, 3)
    d.lens_u, d.lens_q, d.roff_u = i32(*COUNTS_U), i32(*[COUNTS_U[i] for i in IDX]), i32(0, 7, 11)
    return d


class _Route:
    """ops._lib() for the length of a wrapper call: the library, recording the names it is asked for"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _routed(ops, monkeypatch, call):
    """call(ops) with ops._lib recorded -> (its result, the launch entries asked for, in order)"""
    route = _Route(ops._lib())
    with monkeypatch.context() as m:
        m.setattr(ops, "_lib", lambda: route)
        res = call(ops)
    return res, [n for n in route.names if not n.endswith(("_ws_bytes", "_supported"))]


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    torch.cuda.synchronize()
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k)


def _zero_bits(x, what):
    assert x.numel() > 0 and bool((x.contiguous().view(torch.int16) == 0).all()), what + ": not +0.0"


def _f32(*shape):
    return torch.full(shape, 7.0, dtype=torch.float32, device="cuda")


def _bf16(*shape):
    return torch.full(shape, 7.0, dtype=torch.bfloat16, device="cuda")


def _drop(D, mask):
    """(keep, seed, p_drop) of a case: the Philox draw, or the explicit mask"""
    return (D.keep, 0, P_DROP) if mask else (None, SEED, P_DROP)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
def _raw_fwd(ops, entry, D, drop, normalise, extras=False):
    """the entry called raw, then its norm tail -> the wrapper's outputs by name"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    k = (p(drop[0]), drop[1], drop[2])
    rows = R if "packed_rows" in entry else NL
    Y, ssq, Rb, zdrop = _f32(rows, O), _f32(rows * 4), None, None
    if entry.endswith("_rb"):
        Rb = _bf16(NL if entry == "vqf_mfb_fuse_fwd_pbf16_rb" else PAD, LDRB)
    if entry == "vqf_mfb_fuse_fwd":
        zdrop = _f32(NL, W) if extras else None
        args = (p(D.P), p(D.pbias), p(D.q), p(D.cascade if extras else None), *k, N, L, O, p(Y), p(ssq), p(zdrop), st)
    elif entry == "vqf_mfb_fuse_fwd_pbf16":
        args = (p(D.Pbn), p(D.pbias), p(D.q), *k, N, L, O, p(Y), p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_pbf16_rb":
        args = (p(D.Pbn), p(D.pbias), p(D.q), *k, N, L, O, p(Y), p(Rb), LDRB, p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_len":
        args = (p(D.P), p(D.pbias), p(D.q), p(D.lens), *k, N, L, O, p(Y), p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_len_pbf16":
        args = (p(D.Pb), p(D.pbias), p(D.q), p(D.lens), *k, N, L, O, p(Y), p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_len_pbf16_rb":
        args = (p(D.Pb), p(D.pbias), p(D.q), p(D.lens), *k, N, L, O, p(Y), p(Rb), LDRB, PAD, p(ssq), st)
    elif entry in ("vqf_mfb_fuse_fwd_packed", "vqf_mfb_fuse_fwd_packed_rows"):
        args = (p(D.Pp), p(D.pbias), p(D.q), p(D.roff), *k, N, R, L, O, p(Y), p(ssq), st)
    elif entry in ("vqf_mfb_fuse_fwd_packed_pbf16", "vqf_mfb_fuse_fwd_packed_rows_pbf16"):
        args = (p(D.Ppb), p(D.pbias), p(D.q), p(D.roff), *k, N, R, L, O, p(Y), p(ssq), st)
    elif entry in ("vqf_mfb_fuse_fwd_packed_pbf16_rb", "vqf_mfb_fuse_fwd_packed_rows_pbf16_rb"):
        args = (p(D.Ppb), p(D.pbias), p(D.q), p(D.roff), *k, N, R, L, O, p(Y), p(Rb), LDRB, PAD, p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_grouped":
        args = (p(D.Pu), p(D.pbias), p(D.q), p(D.idx), *k, N, U, L, O, p(Y), p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_grouped_len":
        args = (p(D.Pu), p(D.pbias), p(D.q), p(D.idx), p(D.lens_q), p(D.lens_u), *k, N, U, L, O, p(Y), p(ssq), st)
    elif entry == "vqf_mfb_fuse_fwd_grouped_packed":
        args = (p(D.Pup), p(D.pbias), p(D.q), p(D.idx), p(D.roff_u), *k, N, U, RU, L, O, p(Y), p(ssq), st)
    assert getattr(lib, entry)(*args) == 0, entry
    norm, inv = _f32(N), _f32(N)
    out = dict(Y=Y, norm=norm, inv=inv)
    if rows == R:
        out["rowinv"] = _f32(R)
        assert lib.vqf_l2_group_norm_packed(p(ssq), p(D.roff), N, R, L, p(norm), p(inv), p(out["rowinv"]), st) == 0
        if normalise:
            assert lib.vqf_scale_rows(p(Y), p(out["rowinv"]), R, 1, O, p(Y), st) == 0
    else:
        assert lib.vqf_l2_group_norm(p(ssq), N, 4 * L, p(norm), p(inv), st) == 0
        if normalise:
            assert lib.vqf_scale_rows(p(Y), p(inv), NL, L, O, p(Y), st) == 0
    if Rb is not None:
        out["Rb"] = Rb
    if entry == "vqf_mfb_fuse_fwd":
        out["zdrop"] = zdrop
    return out


def _wrap_fwd(ops, entry, D, drop, normalise, extras=False):
    """the entry through its public wrapper -> its outputs by name"""
    kw = dict(keep=drop[0], seed=drop[1], p_drop=drop[2], pbias=D.pbias, normalise=normalise)
    rb = [] if entry.endswith("_rb") else None
    zdrop = ()
    if entry == "vqf_mfb_fuse_fwd":
        res = ops.mfb_fuse_fwd(D.P, D.q, N, L, O, cascade=D.cascade if extras else None, want_zdrop=extras, **kw)
        res, zdrop = res[:3], res[3:]
    elif entry in ("vqf_mfb_fuse_fwd_pbf16", "vqf_mfb_fuse_fwd_pbf16_rb"):
        res = ops.mfb_fuse_fwd(D.Pbn, D.q, N, L, O, r_bf16=rb, **kw)
        assert res[3] is None
        res = res[:3]
    elif entry == "vqf_mfb_fuse_fwd_len":
        res = ops.mfb_fuse_fwd(D.P, D.q, N, L, O, lens=D.lens, **kw)[:3]
    elif entry in ("vqf_mfb_fuse_fwd_len_pbf16", "vqf_mfb_fuse_fwd_len_pbf16_rb"):
        res = ops.mfb_fuse_fwd(D.Pb, D.q, N, L, O, lens=D.lens, regions_bf16=True, r_bf16=rb, **kw)[:3]
    elif entry == "vqf_mfb_fuse_fwd_packed":
        res = ops.mfb_fuse_fwd_packed(D.Pp, D.q, D.roff, N, L, O, **kw)
    elif entry in ("vqf_mfb_fuse_fwd_packed_pbf16", "vqf_mfb_fuse_fwd_packed_pbf16_rb"):
        res = ops.mfb_fuse_fwd_packed(D.Ppb, D.q, D.roff, N, L, O, R=R, regions_bf16=True, r_bf16=rb, **kw)
    elif entry == "vqf_mfb_fuse_fwd_packed_rows":
        res = ops.mfb_fuse_fwd_packed_rows(D.Pp, D.q, D.roff, N, L, O, **kw)
    elif entry in ("vqf_mfb_fuse_fwd_packed_rows_pbf16", "vqf_mfb_fuse_fwd_packed_rows_pbf16_rb"):
        res = ops.mfb_fuse_fwd_packed_rows(D.Ppb, D.q, D.roff, N, L, O, R=R, regions_bf16=True, r_bf16=rb, **kw)
    elif entry == "vqf_mfb_fuse_fwd_grouped":
        res = ops.mfb_fuse_fwd_grouped(D.Pu, D.q, D.idx, N, U, L, O, **kw)
    elif entry == "vqf_mfb_fuse_fwd_grouped_len":
        res = ops.mfb_fuse_fwd_grouped(D.Pu, D.q, D.idx, N, U, L, O, lens=(D.lens_q, D.lens_u), **kw)
    elif entry == "vqf_mfb_fuse_fwd_grouped_packed":
        res = ops.mfb_fuse_fwd_packed(D.Pup, D.q, D.roff_u, N, L, O, idx=D.idx, **kw)
    out = dict(zip(("Y", "norm", "inv", "rowinv"), res))
    assert len(out) == len(res)
    if rb is not None:
        assert len(rb) == 1
        out["Rb"] = rb[0]
    if entry == "vqf_mfb_fuse_fwd":
        out["zdrop"], = zdrop
    return out


# entry -> (the route behind it, the real rows of the bf16 copy)
FWD = {
    "vqf_mfb_fuse_fwd": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_pbf16": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_pbf16_rb": (NORM_TAIL, NL),
    "vqf_mfb_fuse_fwd_len": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_len_pbf16": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_len_pbf16_rb": (NORM_TAIL, NL),
    "vqf_mfb_fuse_fwd_packed": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_packed_pbf16": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_packed_pbf16_rb": (NORM_TAIL, NL),
    "vqf_mfb_fuse_fwd_packed_rows": (NORM_TAIL_ROWS, None),
    "vqf_mfb_fuse_fwd_packed_rows_pbf16": (NORM_TAIL_ROWS, None),
    "vqf_mfb_fuse_fwd_packed_rows_pbf16_rb": (NORM_TAIL_ROWS, R),
    "vqf_mfb_fuse_fwd_grouped": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_grouped_len": (NORM_TAIL, None),
    "vqf_mfb_fuse_fwd_grouped_packed": (NORM_TAIL, None),
}


def _check_fwd(ops, monkeypatch, D, entry, normalise, mask=False, extras=False):
    tail, rb_real = FWD[entry]
    drop = _drop(D, mask)
    got, names = _routed(ops, monkeypatch, lambda o: _wrap_fwd(o, entry, D, drop, normalise, extras))
    assert names == [entry] + tail + ["vqf_scale_rows"] * normalise
    _same(got, _raw_fwd(ops, entry, D, drop, normalise, extras), entry)
    if rb_real is not None:
        assert tuple(got["Rb"].shape) == (NL if entry == "vqf_mfb_fuse_fwd_pbf16_rb" else PAD, LDRB)
        _zero_bits(got["Rb"][:, O:], entry + ": pad columns of the bf16 copy")
        if got["Rb"].shape[0] > rb_real:
            _zero_bits(got["Rb"][rb_real:], entry + ": rows of the bf16 copy behind the real ones")


@pytest.mark.parametrize("entry", list(FWD))
def test_forward_entry_through_its_wrapper(ops, monkeypatch, D, entry):
    _check_fwd(ops, monkeypatch, D, entry, normalise=not entry.endswith("_rb"))     # the copy of R comes with normalise=False


def test_forward_plain_variants(ops, monkeypatch, D):
    _check_fwd(ops, monkeypatch, D, "vqf_mfb_fuse_fwd", normalise=False)
    _check_fwd(ops, monkeypatch, D, "vqf_mfb_fuse_fwd", normalise=True, mask=True)
    _check_fwd(ops, monkeypatch, D, "vqf_mfb_fuse_fwd", normalise=True, extras=True)
    _check_fwd(ops, monkeypatch, D, "vqf_mfb_fuse_fwd_packed_rows_pbf16", normalise=False, mask=True)
    # a request for the bf16 copy that the plain form cannot serve falls back, quietly, to the entry without it
    rb = []
    res, names = _routed(ops, monkeypatch, lambda o: o.mfb_fuse_fwd(D.Pbn, D.q, N, L, O, seed=SEED, p_drop=P_DROP, pbias=D.pbias,
                                                                  normalise=True, r_bf16=rb))
    assert names == ["vqf_mfb_fuse_fwd_pbf16", "vqf_l2_group_norm", "vqf_scale_rows"] and rb == []
    _same(dict(zip(("Y", "norm", "inv"), res[:3])), _raw_fwd(ops, "vqf_mfb_fuse_fwd_pbf16", D, _drop(D, False), True), "fallback")


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def _fwd_of(ops, entry, D, drop, lin):
    """Y, norm, inv of the forward the backward entry belongs to (inputs of the case: made by the wrapper, compared nowhere)"""
    fwd = entry.replace("_bwd", "_fwd").replace("_bf16dp", "")
    out = _wrap_fwd(ops, fwd, D, drop, normalise=lin is None)
    return out["Y"], out["norm"], out["inv"]


def _raw_bwd(ops, entry, D, drop, Y, norm, inv, lin=None, extras=False, dbias=True):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    k = (p(drop[0]), drop[1], drop[2])
    rows = "packed_rows" in entry
    dY = D.dYr if rows else D.dY
    cA, cB = _f32(N), _f32(N)
    if lin is not None and rows:
        unit = _f32(N)
        assert lib.vqf_l2_norm_bwd_coef_lin_packed(p(lin[0]), p(lin[1]), G, p(D.roff), p(norm), p(inv), N, R, L, p(cA), p(cB), p(unit),
                                                   st) == 0
        inv = unit
    elif lin is not None:
        unit = _f32(N)
        assert lib.vqf_l2_norm_bwd_coef_lin(p(lin[0]), p(lin[1]), G, p(norm), p(inv), N, L, p(cA), p(cB), p(unit), st) == 0
        inv = unit
    elif rows:
        rowdot = _f32(R)
        assert lib.vqf_rowdot(p(Y), p(dY), R, O, p(rowdot), st) == 0
        assert lib.vqf_l2_norm_bwd_coef_packed(p(rowdot), p(D.roff), p(norm), p(inv), N, R, L, p(cA), p(cB), st) == 0
    else:
        rowdot = _f32(NL)
        assert lib.vqf_rowdot(p(Y), p(dY), NL, O, p(rowdot), st) == 0
        assert lib.vqf_l2_norm_bwd_coef(p(rowdot), p(norm), p(inv), N, L, p(cA), p(cB), st) == 0
    grouped = "_grouped" in entry
    nbytes = lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O) if grouped else lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O)
    ws = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
    dq, db = _f32(N, W), _f32(W) if dbias else None
    head = (p(dY), p(Y), p(inv), p(cA), p(cB))
    tail = (p(dq), p(db), p(ws), ws.numel(), st)
    dc = None
    if entry == "vqf_mfb_fuse_bwd":
        dP, dc = _f32(NL, W), _f32(NL, W) if extras else None
        args = (p(dY), p(D.dzdrop if extras else None), p(Y), p(inv), p(cA), p(cB), p(D.P), p(D.pbias), p(D.q),
                p(D.cascade if extras else None), *k, N, L, O, p(dP), p(dq), p(dc), p(db), p(ws), ws.numel(), st)
    elif entry == "vqf_mfb_fuse_bwd_pbf16":
        dP = _bf16(NL, W)
        args = (*head, p(D.Pbn), p(D.pbias), p(D.q), *k, N, L, O, p(dP), *tail)
    elif entry == "vqf_mfb_fuse_bwd_bf16dp":
        dP = _bf16(NL, W)
        args = (*head, p(D.P), p(D.pbias), p(D.q), *k, N, L, O, p(dP), *tail)
    elif entry == "vqf_mfb_fuse_bwd_len":
        dP = _f32(NL, W)
        args = (*head, p(D.P), p(D.pbias), p(D.q), p(D.lens), *k, N, L, O, p(dP), *tail)
    elif entry == "vqf_mfb_fuse_bwd_len_pbf16":
        dP = _bf16(PAD, W)
        args = (*head, p(D.Pb), p(D.pbias), p(D.q), p(D.lens), *k, N, L, O, p(dP), PAD, *tail)
    elif entry == "vqf_mfb_fuse_bwd_len_bf16dp":
        dP = _bf16(PAD, W)
        args = (*head, p(D.P), p(D.pbias), p(D.q), p(D.lens), *k, N, L, O, p(dP), PAD, *tail)
    elif entry in ("vqf_mfb_fuse_bwd_packed", "vqf_mfb_fuse_bwd_packed_rows"):
        dP = _f32(R, W)
        args = (*head, p(D.Pp), p(D.pbias), p(D.q), p(D.roff), *k, N, R, L, O, p(dP), *tail)
    elif entry in ("vqf_mfb_fuse_bwd_packed_pbf16", "vqf_mfb_fuse_bwd_packed_rows_pbf16"):
        dP = _bf16(PAD, W)
        args = (*head, p(D.Ppb), p(D.pbias), p(D.q), p(D.roff), *k, N, R, L, O, p(dP), PAD, *tail)
    elif entry in ("vqf_mfb_fuse_bwd_packed_bf16dp", "vqf_mfb_fuse_bwd_packed_rows_bf16dp"):
        dP = _bf16(PAD, W)
        args = (*head, p(D.Pp), p(D.pbias), p(D.q), p(D.roff), *k, N, R, L, O, p(dP), PAD, *tail)
    elif entry == "vqf_mfb_fuse_bwd_grouped":
        dP = _f32(U * L, W)
        args = (*head, p(D.Pu), p(D.pbias), p(D.q), p(D.idx), p(D.order), p(D.grp_off), *k, N, U, L, O, p(dP), *tail)
    elif entry == "vqf_mfb_fuse_bwd_grouped_len":
        dP = _f32(U * L, W)
        args = (*head, p(D.Pu), p(D.pbias), p(D.q), p(D.idx), p(D.order), p(D.grp_off), p(D.lens_q), p(D.lens_u), *k, N, U, L, O, p(dP),
                *tail)
    elif entry == "vqf_mfb_fuse_bwd_grouped_packed":
        dP = _f32(RU, W)
        args = (*head, p(D.Pup), p(D.pbias), p(D.q), p(D.idx), p(D.order), p(D.grp_off), p(D.roff_u), *k, N, U, RU, L, O, p(dP), *tail)
    assert getattr(lib, entry)(*args) == 0, entry
    out = dict(dP=dP, dq=dq, db=db)
    if entry in ("vqf_mfb_fuse_bwd", "vqf_mfb_fuse_bwd_pbf16", "vqf_mfb_fuse_bwd_bf16dp", "vqf_mfb_fuse_bwd_len",
                 "vqf_mfb_fuse_bwd_len_pbf16", "vqf_mfb_fuse_bwd_len_bf16dp"):
        out["dc"] = dc
    return out


def _wrap_bwd(ops, entry, D, drop, Y, norm, inv, lin=None, extras=False, dbias=True):
    kw = dict(keep=drop[0], seed=drop[1], p_drop=drop[2], pbias=D.pbias, want_dbias=dbias, lin=lin)
    bf = dict(dp_bf16=True, regions_bf16=True, dp_rows=PAD)
    if entry == "vqf_mfb_fuse_bwd":
        res = ops.mfb_fuse_bwd(D.dY, Y, norm, inv, D.P, D.q, N, L, O, cascade=D.cascade if extras else None,
                               dzdrop=D.dzdrop if extras else None, **kw)
    elif entry == "vqf_mfb_fuse_bwd_pbf16":
        res = ops.mfb_fuse_bwd(D.dY, Y, norm, inv, D.Pbn, D.q, N, L, O, dp_bf16=True, **kw)
    elif entry == "vqf_mfb_fuse_bwd_bf16dp":
        res = ops.mfb_fuse_bwd(D.dY, Y, norm, inv, D.P, D.q, N, L, O, dp_bf16=True, **kw)
    elif entry == "vqf_mfb_fuse_bwd_len":
        res = ops.mfb_fuse_bwd(D.dY, Y, norm, inv, D.P, D.q, N, L, O, lens=D.lens, **kw)
    elif entry == "vqf_mfb_fuse_bwd_len_pbf16":                            # dp_rows left to its default: the rows of P
        res = ops.mfb_fuse_bwd(D.dY, Y, norm, inv, D.Pb, D.q, N, L, O, lens=D.lens, dp_bf16=True, regions_bf16=True, **kw)
    elif entry == "vqf_mfb_fuse_bwd_len_bf16dp":
        res = ops.mfb_fuse_bwd(D.dY, Y, norm, inv, D.P, D.q, N, L, O, lens=D.lens, **bf, **kw)
    elif entry == "vqf_mfb_fuse_bwd_packed":
        res = ops.mfb_fuse_bwd_packed(D.dY, Y, norm, inv, D.Pp, D.q, D.roff, N, L, O, **kw)
    elif entry == "vqf_mfb_fuse_bwd_packed_pbf16":                         # dp_rows left to its default: the rows of P
        res = ops.mfb_fuse_bwd_packed(D.dY, Y, norm, inv, D.Ppb, D.q, D.roff, N, L, O, R=R, dp_bf16=True, regions_bf16=True, **kw)
    elif entry == "vqf_mfb_fuse_bwd_packed_bf16dp":
        res = ops.mfb_fuse_bwd_packed(D.dY, Y, norm, inv, D.Pp, D.q, D.roff, N, L, O, **bf, **kw)
    elif entry == "vqf_mfb_fuse_bwd_packed_rows":
        res = ops.mfb_fuse_bwd_packed_rows(D.dYr, Y, norm, inv, D.Pp, D.q, D.roff, N, L, O, **kw)
    elif entry == "vqf_mfb_fuse_bwd_packed_rows_pbf16":
        res = ops.mfb_fuse_bwd_packed_rows(D.dYr, Y, norm, inv, D.Ppb, D.q, D.roff, N, L, O, R=R, **bf, **kw)
    elif entry == "vqf_mfb_fuse_bwd_packed_rows_bf16dp":
        res = ops.mfb_fuse_bwd_packed_rows(D.dYr, Y, norm, inv, D.Pp, D.q, D.roff, N, L, O, **bf, **kw)
    elif entry == "vqf_mfb_fuse_bwd_grouped":
        res = ops.mfb_fuse_bwd_grouped(D.dY, Y, norm, inv, D.Pu, D.q, D.idx, D.order, D.grp_off, N, U, L, O, **kw)
    elif entry == "vqf_mfb_fuse_bwd_grouped_len":
        res = ops.mfb_fuse_bwd_grouped(D.dY, Y, norm, inv, D.Pu, D.q, D.idx, D.order, D.grp_off, N, U, L, O, lens=(D.lens_q, D.lens_u),
                                       **kw)
    elif entry == "vqf_mfb_fuse_bwd_grouped_packed":
        res = ops.mfb_fuse_bwd_packed(D.dY, Y, norm, inv, D.Pup, D.q, D.roff_u, N, L, O, grp=(D.idx, D.order, D.grp_off), **kw)
    if len(res) == 4:
        return dict(dP=res[0], dq=res[1], dc=res[2], db=res[3])
    return dict(zip(("dP", "dq", "db"), res))


# entry -> (the route in front of it, (rows of a bf16 dP, the real ones of them))
BWD = {
    "vqf_mfb_fuse_bwd": (COEF_HEAD, None),
    "vqf_mfb_fuse_bwd_pbf16": (COEF_HEAD, (NL, None)),                     # the plain form: dP like P
    "vqf_mfb_fuse_bwd_bf16dp": (COEF_HEAD, (NL, None)),
    "vqf_mfb_fuse_bwd_len": (COEF_HEAD, None),
    "vqf_mfb_fuse_bwd_len_pbf16": (COEF_HEAD, (PAD, NL)),
    "vqf_mfb_fuse_bwd_len_bf16dp": (COEF_HEAD, (PAD, NL)),
    "vqf_mfb_fuse_bwd_packed": (COEF_HEAD, None),
    "vqf_mfb_fuse_bwd_packed_pbf16": (COEF_HEAD, (PAD, R)),
    "vqf_mfb_fuse_bwd_packed_bf16dp": (COEF_HEAD, (PAD, R)),
    "vqf_mfb_fuse_bwd_packed_rows": (COEF_HEAD_ROWS, None),
    "vqf_mfb_fuse_bwd_packed_rows_pbf16": (COEF_HEAD_ROWS, (PAD, R)),
    "vqf_mfb_fuse_bwd_packed_rows_bf16dp": (COEF_HEAD_ROWS, (PAD, R)),
    "vqf_mfb_fuse_bwd_grouped": (COEF_HEAD, None),
    "vqf_mfb_fuse_bwd_grouped_len": (COEF_HEAD, None),
    "vqf_mfb_fuse_bwd_grouped_packed": (COEF_HEAD, None),
}


def _check_bwd(ops, monkeypatch, D, entry, mask=False, lin=None, head=None, extras=False, dbias=True):
    drop = _drop(D, mask)
    Y, norm, inv = _fwd_of(ops, entry, D, drop, lin)
    got, names = _routed(ops, monkeypatch, lambda o: _wrap_bwd(o, entry, D, drop, Y, norm, inv, lin, extras, dbias))
    assert names == (head or BWD[entry][0]) + [entry]
    _same(got, _raw_bwd(ops, entry, D, drop, Y, norm, inv, lin, extras, dbias), entry)
    if BWD[entry][1] is not None:
        rows, real = BWD[entry][1]
        assert got["dP"].dtype == torch.bfloat16 and tuple(got["dP"].shape) == (rows, W)
        if real is not None:
            _zero_bits(got["dP"][real:], entry + ": rows of dP behind the real ones")


@pytest.mark.parametrize("entry", list(BWD))
def test_backward_entry_through_its_wrapper(ops, monkeypatch, D, entry):
    _check_bwd(ops, monkeypatch, D, entry)


def test_backward_plain_variants(ops, monkeypatch, D):
    _check_bwd(ops, monkeypatch, D, "vqf_mfb_fuse_bwd", mask=True, dbias=False)
    _check_bwd(ops, monkeypatch, D, "vqf_mfb_fuse_bwd", extras=True)                            # cascade and dzdrop
    _check_bwd(ops, monkeypatch, D, "vqf_mfb_fuse_bwd", lin=(D.dl, D.lin), head=COEF_HEAD_LIN)
    _check_bwd(ops, monkeypatch, D, "vqf_mfb_fuse_bwd_packed_rows", lin=(D.dlr, D.linr), head=COEF_HEAD_ROWS_LIN)
    _check_bwd(ops, monkeypatch, D, "vqf_mfb_fuse_bwd_packed_rows_bf16dp", mask=True)

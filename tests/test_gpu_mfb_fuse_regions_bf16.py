"""The bf16 forms of the image fusion on counted and packed regions (include/vqa_fusion.h "The bf16 image projection on counted and
packed regions"; csrc/fusion_regions_bf16.hip over the kernels of csrc/fusion.hip), every entry point called raw, in the way and
with the plumbing of tests/test_gpu_mfb_fuse_kernels.py (imported, not restated: its operands, its two data sets `exact` and `random`
with an explicit keep tensor and with the Philox draw, its guard rows, its per-element fp64 bounds k_*, its b + 2^-8 (|ref| + b) rule
for a bf16 dP).  P holds bf16-representable values where it is stored in bf16; every other operand is what that file makes it.

Per case (N = 3, L = 7, counts 1, L and one between; R = 12 packed and N L = 21 counted, so dP has 32 rows and a zero tail):
  1. forward and backward against the fp64 reference tests/mfb_fuse_ref.py through lens / roff, that file's bounds;
  2. R and rowssq of the bf16-P forward carry the bits of the fp32-P sibling fed the same values;
  3. dq and dbiasP are bit-equal between _pbf16 and _bf16dp (their dP too: the same fp32 values, rounded once);
  4. the _packed / _packed_rows forms are bit-equal to the _len forms on the zero-padded copy (dP: the real rows);
  5. dP rows R .. dP_rows - 1 hold +0.0 bits, the guard rows behind them keep their 7.0, dP_rows = R leaves no tail and the same
     bits, and the padded dP rows of the _len form are +0.0;
  6. the row-padding cast gives ops.cast_bf16's bits on the real rows and +0.0 in the tail.
Every call is made twice and must give the same bits.  The worst err / bound per output is logged
(profiles/mfb_fuse_regions_bf16_parity.txt)."""
import pytest
import torch

import test_gpu_mfb_fuse_kernels as K

pytestmark = pytest.mark.gpu

N, L = 3, 7
COUNTS = [1, 7, 4]                                       # 1, L and one between: R = 12, N L = 21 -- neither a multiple of 32
FORMS = ("len", "packed", "packed_rows")


@pytest.fixture(scope="module")
def ops():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd.ops


def _pad32(r):
    return (r + 31) // 32 * 32


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _equal_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what + ": different bits"


def _fwd(ops, form, c, d, g):
    """one forward launch of the bf16-P entry point of `form` -> {R, rowssq} on the CPU"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    O = c["O"]
    R, ssq = K._Out(d["nrows"], O), K._Out(d["nrows"], 4)
    head = (p(g["P"]), p(g["pbias"]), p(g["q"]))
    drop = (p(g["keep"]), d["seed"], d["p"])
    if form == "len":
        rc = lib.vqf_mfb_fuse_fwd_len_pbf16(*head, p(g["lens_q"]), *drop, N, L, O, p(R.view), p(ssq.view), st)
    else:
        fn = lib.vqf_mfb_fuse_fwd_packed_pbf16 if form == "packed" else lib.vqf_mfb_fuse_fwd_packed_rows_pbf16
        rc = fn(*head, p(g["roff"]), *drop, N, g["Rtot"], L, O, p(R.view), p(ssq.view), st)
    assert rc == 0, (form, rc)
    return dict(R=R.take(), rowssq=ssq.take())


def _bwd(ops, form, c, d, g, dY, Y, p_bf16, dp_rows, dbias=True):
    """one backward call of form + ("_pbf16" | "_bf16dp") with dP_rows = dp_rows -> {dP (dp_rows, 5 O) bf16, dq, dbiasP} on the CPU"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    O = c["O"]
    W5 = 5 * O
    dP, dq, db = K._Out(dp_rows, W5, dtype=torch.bfloat16), K._Out(N, W5), K._Out(1, W5)
    ws = K._Ws(lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O))
    fn = getattr(lib, "vqf_mfb_fuse_bwd_%s_%s" % (form, "pbf16" if p_bf16 else "bf16dp"))
    head = (p(dY), p(Y), p(g["inv"]), p(g["coefA"]), p(g["coefB"]), p(g["P"]), p(g["pbias"]), p(g["q"]))
    tail = (p(dP.view), dp_rows, p(dq.view), p(db.view) if dbias else None, p(ws.buf), ws.nbytes, st)
    if form == "len":
        rc = fn(*head, p(g["lens_q"]), p(g["keep"]), d["seed"], d["p"], N, L, O, *tail)
    else:
        rc = fn(*head, p(g["roff"]), p(g["keep"]), d["seed"], d["p"], N, g["Rtot"], L, O, *tail)
    assert rc == 0, (form, p_bf16, rc)
    res = dict(dP=dP.take(), dq=dq.take())               # (take: the guard rows around dP -- behind its zero tail -- kept their 7.0)
    if dbias:
        res["dbiasP"] = db.take()
    else:
        assert db.untouched()
    assert ws.ok(), "the guard behind the workspace was written"
    return res


def _operands(c, d, p_dtype):
    """K._gpu_operands with P in p_dtype (the values are bf16-representable, so both hold the same numbers)"""
    g = K._gpu_operands(c, d)
    g["P"] = K._in(d["P"], p_dtype)
    g["Rtot"] = d["P"].shape[0]
    return g


def _len_twin(c, d):
    """the counted form of a packed case on the ZERO-padded copy of P: (case, operands d) with the same q, masks and coefficients"""
    cl = dict(c, form="len")
    dl = dict(d, packed=False, rows=False, counted=True)
    P = torch.zeros(N * L, d["P"].shape[1], dtype=torch.float64)
    P[d["valid"].reshape(-1)] = d["P"]
    dl["P"], dl["nrows"], dl["pad_rows"] = P, N * L, ~d["valid"].reshape(-1)
    dl.pop("roff", None)
    return cl, dl


def _scatter(x, d):
    """a per-row operand of the packed_rows form -> the padded coordinates, exact zeros on the padded rows"""
    if not d["rows"]:
        return x
    out = torch.zeros(N * L, x.shape[1], dtype=x.dtype)
    out[d["valid"].reshape(-1)] = x
    return out


def _case(form, O, **kw):
    return K._case(form, N, L, O, lens=COUNTS, **kw)


CASES = [_case(form, O) for form in FORMS for O in K.O_CLASSES]
# the direct access at an O the coalesced one takes, and a walk in three blocks per sample (the count-1 sample: blocks without a row)
CASES += [_case("packed", 1000, opts=dict(fuse_coal=0)), _case("len", 1000, opts=dict(fuse_ls=3, fuse_ls_bwd=3)),
          _case("packed_rows", 1000, opts=dict(fuse_ls=3, fuse_ls_bwd=3, fuse_coal=0))]


# whole 16-byte pieces of the bf16 rows start + l (5 O % 8 == 0: the coalesced access), and the direct access for every other O
assert {(5 * O) % 8 == 0 for O in K.O_CLASSES} == {True, False} and (5 * 12) % 8 != 0 and (5 * 1000) % 8 == 0


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_fuse_regions_bf16(ops, c):
    form, O = c["form"], c["O"]
    rep = K._Report("regions bf16", c["id"])
    with ops.options(**c["opts"]):
        for kind in K.KINDS:
            for mask in K.MASKS:
                d = K._build(c, kind, mask)
                d["P"] = d["P"].to(torch.bfloat16).double()          # P is stored in bf16 (NaN padding stays NaN)
                R = d["P"].shape[0]
                assert R == (12 if d["packed"] else 21) and R % 32 != 0
                rows = _pad32(R)
                gb, gf = _operands(c, d, torch.bfloat16), _operands(c, d, torch.float32)
                tag = "" if mask == "keep" else "philox_"
                # forward: fp64 bounds (1), the fp32-P sibling's bits (2)
                f = _fwd(ops, form, c, d, gb)
                assert K._same(f, _fwd(ops, form, c, d, gb))
                K._check_fwd(rep, c, d, f, tag)
                f32 = K._fwd(ops, c, d, gf)
                _equal_bits(f["R"], f32["R"], "R against the fp32-P sibling")
                _equal_bits(f["rowssq"], f32["rowssq"], "rowssq against the fp32-P sibling")
                if kind == "exact":
                    Y = d["Y"]
                else:
                    Y = (f["R"].double() * d["inv"][d["sample_of_row"]][:, None]).float().double()
                dY, Y = K._nan_pad(d["dY"], d), K._nan_pad(Y, d)
                gdY, gY = K._in(dY), K._in(Y)
                # backward: fp64 bounds (1) on the real rows, the tail and the guards (5), _pbf16 against _bf16dp (3)
                res = {}
                for p_bf16, g in ((True, gb), (False, gf)):
                    b = _bwd(ops, form, c, d, g, gdY, gY, p_bf16, rows)
                    assert K._same(b, _bwd(ops, form, c, d, g, gdY, gY, p_bf16, rows))
                    assert b["dP"].shape[0] == rows and bool((_bits(b["dP"][R:]) == 0).all()), "dP rows R .. dP_rows - 1 must be +0.0"
                    tight = _bwd(ops, form, c, d, g, gdY, gY, p_bf16, R)               # dP_rows = R: no tail, the same bits
                    _equal_bits(tight["dP"], b["dP"][:R], "dP with dP_rows = R")
                    _equal_bits(tight["dq"], b["dq"], "dq with dP_rows = R")
                    K._check_bwd(rep, c, d, dict(b, dP=b["dP"][:R]), dY, Y, tag + ("pbf16_" if p_bf16 else "bf16dp_"))
                    if form == "len":
                        assert bool((_bits(b["dP"][:R][d["pad_rows"]]) == 0).all()), "a padded dP row of the _len form must be +0.0"
                    res[p_bf16] = b
                for name in ("dP", "dq", "dbiasP"):
                    _equal_bits(res[True][name], res[False][name], name + ": _pbf16 against _bf16dp")
                nb = _bwd(ops, form, c, d, gb, gdY, gY, True, rows, dbias=False)       # dbiasP = NULL: the same dP / dq bits
                _equal_bits(nb["dP"], res[True]["dP"], "dP without dbiasP")
                _equal_bits(nb["dq"], res[True]["dq"], "dq without dbiasP")
                # the packed forms against the counted form on the zero-padded copy (4)
                if d["packed"]:
                    cl, dl = _len_twin(c, d)
                    gl = _operands(cl, dl, torch.bfloat16)
                    fl = _fwd(ops, "len", cl, dl, gl)
                    valid = d["valid"].reshape(-1)
                    _equal_bits(f["R"], fl["R"][valid] if d["rows"] else fl["R"], "R against the _len form")
                    _equal_bits(f["rowssq"], fl["rowssq"][valid] if d["rows"] else fl["rowssq"], "rowssq against the _len form")
                    bl = _bwd(ops, "len", cl, dl, gl, K._in(_scatter(dY, d)), K._in(_scatter(Y, d)), True, _pad32(N * L))
                    _equal_bits(res[True]["dP"][:R], bl["dP"][:N * L][valid], "dP against the _len form's real rows")
                    assert bool((_bits(bl["dP"][:N * L][~valid]) == 0).all()) and bool((_bits(bl["dP"][N * L:]) == 0).all())
                    _equal_bits(res[True]["dq"], bl["dq"], "dq against the _len form")
                    _equal_bits(res[True]["dbiasP"], bl["dbiasP"], "dbiasP against the _len form")
    rep.flush()


@pytest.mark.parametrize("R,C", [(12, 24), (21, 2048), (1037, 40), (64, 8), (1, 12)])
def test_cast_rows(ops, R, C):
    """vqf_cast_f32_bf16_rows / ops.cast_bf16(pad_rows_to=32): the bits of ops.cast_bf16 on the real rows (pad columns included), +0.0
    in the tail, nothing behind it; a row count that is a multiple of 32 is the plain call."""
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C)).cuda()
    want = ops.cast_bf16(x)
    got = ops.cast_bf16(x, pad_rows_to=32)
    torch.cuda.synchronize()
    Rp = _pad32(R)
    assert got.shape == (Rp, want.shape[1]) and got.dtype == torch.bfloat16
    _equal_bits(got[:R].cpu(), want.cpu(), "the real rows")
    assert bool((_bits(got[R:].cpu()) == 0).all())
    # raw, into a buffer of 7.0 with guard rows: NaN where the tail will be, so that zeros there were written
    lib, p = ops._lib(), ops._ptr
    out = K._Out(Rp, want.shape[1], dtype=torch.bfloat16)
    out.view[R:] = float("nan")
    for _ in range(2):
        assert lib.vqf_cast_f32_bf16_rows(p(x), R, C, C, p(out.view), want.shape[1], Rp, ops._stream()) == 0
    raw = out.take()
    _equal_bits(raw, got.cpu(), "the raw call")
    assert lib.vqf_cast_f32_bf16_rows(p(x), R, C, C, p(out.view), want.shape[1], R - 1, ops._stream()) == -1      # VQF_E_BADARG
    assert out.untouched()

"""The bf16 copy of R on counted and packed regions (include/vqa_fusion.h "The bf16 co-attention head on the same call forms":
vqf_mfb_fuse_fwd_{len,packed,packed_rows}_pbf16_rb), every entry point called raw with the plumbing of
tests/test_gpu_mfb_fuse_kernels.py (imported: its operands with an explicit keep tensor and with the Philox draw, its guard rows).

N = 3; O = 8 and 40 (neither a multiple of 32: pad columns), L = 5 and 37, counts with 1 and L among them; the packed row count R is 9,
45 (no multiple of 32) and 64 (one); N L is 15 and 111.  Per case, with the copy's buffer pre-filled with NaN between guard rows:
  1. R and rowssq carry the bits of the entry point without _rb on the same operands;
  2. the copy equals R.to(bfloat16) element for element on the real rows;
  3. its pad columns (up to the pitch, which may exceed O rounded up to 32), every row behind a count (len / packed) and the rows
     behind `rows` up to rb_rows hold +0.0 bits; the guard rows keep their fill; rb_rows = rows leaves no tail and the same bits;
  4. with every count equal to L the len form gives the bits of vqf_mfb_fuse_fwd_pbf16_rb;
  5. a refused call (rb_rows below rows, a pitch below the padded width) has written nothing.
Every call is made twice and must give the same bits."""
import pytest
import torch

import test_gpu_mfb_fuse_kernels as K

pytestmark = pytest.mark.gpu

N = 3
FORMS = ("len", "packed", "packed_rows")
BADARG = -1


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


def _operands(c, d):
    g = K._gpu_operands(c, d)
    g["P"] = K._in(d["P"], torch.bfloat16)
    g["Rtot"] = d["P"].shape[0]
    return g


def _call(ops, form, c, d, g, rb=None, expect=0):
    """one forward launch of the bf16-P entry point of `form`; rb = (rb_rows, ldrb): the _rb entry point, the copy pre-filled with NaN
    -> {R, rowssq[, Rb]} on the CPU (expect != 0: the return code, and nothing may have been written)"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    L, O = c["L"], c["O"]
    R, ssq = K._Out(d["nrows"], O), K._Out(d["nrows"], 4)
    head = (p(g["P"]), p(g["pbias"]), p(g["q"]), p(g["lens_q"] if form == "len" else g["roff"]), p(g["keep"]), d["seed"], d["p"])
    dims = (N, L, O) if form == "len" else (N, g["Rtot"], L, O)
    name = "vqf_mfb_fuse_fwd_%s_pbf16%s" % (form, "_rb" if rb else "")
    if rb:
        Rb = K._Out(rb[0], rb[1], dtype=torch.bfloat16)
        rc = getattr(lib, name)(*head, *dims, p(R.view), p(Rb.view), rb[1], rb[0], p(ssq.view), st)
        if expect:
            assert rc == expect, (name, rc)
            assert R.untouched() and ssq.untouched() and Rb.untouched(), name + ": a refused call wrote something"
            return None
        Rb.view.fill_(float("nan"))
        rc = getattr(lib, name)(*head, *dims, p(R.view), p(Rb.view), rb[1], rb[0], p(ssq.view), st)
    else:
        rc = getattr(lib, name)(*head, *dims, p(R.view), p(ssq.view), st)
    assert rc == 0, (name, rc)
    res = dict(R=R.take(), rowssq=ssq.take())
    if rb:
        torch.cuda.synchronize()
        res["Rb"] = Rb.view.clone().cpu()
        Rb.view.fill_(7.0)
        assert Rb.untouched(), "guard rows around the bf16 copy were written"
    return res


def _case(form, O, L, counts, **kw):
    c = K._case(form, N, L, O, lens=counts, **kw)
    return c


SHAPES = [(5, [1, 5, 3]), (37, [1, 37, 7]), (37, [1, 37, 26])]        # R = 9, 45, 64; N L = 15, 111, 111
CASES = [_case(form, O, L, counts) for form in FORMS for O in (8, 40) for L, counts in SHAPES]
# the direct access, and a walk in three blocks per sample (the count-1 sample: blocks without a real row store the zero rows)
CASES += [_case("packed", 40, 37, [1, 37, 7], opts=dict(fuse_coal=0)), _case("len", 40, 37, [1, 37, 7], opts=dict(fuse_ls=3)),
          _case("packed_rows", 8, 37, [1, 37, 26], opts=dict(fuse_ls=3, fuse_coal=0)), _case("len", 8, 5, [1, 5, 3], opts=dict(fuse_coal=1))]


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_fuse_regions_bf16_rb(ops, c):
    form, O, L = c["form"], c["O"], c["L"]
    with ops.options(**c["opts"]):
        for mask in K.MASKS:
            d = K._build(c, "random", mask)
            d["P"] = d["P"].to(torch.bfloat16).double()                      # P is stored in bf16 (NaN padding stays NaN)
            g = _operands(c, d)
            rows = d["nrows"]
            assert rows == (sum(c["lens"]) if form == "packed_rows" else N * L)
            plain = _call(ops, form, c, d, g)
            for ldrb in (_pad32(O), _pad32(O) + 32):
                rb_rows = _pad32(rows) if ldrb == _pad32(O) else rows + 3     # (the tail need not end on a multiple of 32)
                got = _call(ops, form, c, d, g, rb=(rb_rows, ldrb))
                assert K._same(got, _call(ops, form, c, d, g, rb=(rb_rows, ldrb)))
                _equal_bits(got["R"], plain["R"], "R against the form without _rb")                                  # 1
                _equal_bits(got["rowssq"], plain["rowssq"], "rowssq against the form without _rb")
                Rb = got["Rb"]
                assert Rb.shape == (rb_rows, ldrb) and not bool(torch.isnan(Rb.float()).any())
                _equal_bits(Rb[:rows, :O], got["R"].to(torch.bfloat16), "the copy against R.to(bfloat16)")           # 2
                assert bool((_bits(Rb[:, O:]) == 0).all()), "pad columns must be +0.0"                               # 3
                assert bool((_bits(Rb[rows:]) == 0).all()), "the rows behind `rows` must be +0.0"
                if form != "packed_rows":
                    behind = ~d["valid"].reshape(-1)
                    assert int(behind.sum()) == N * L - sum(c["lens"]) > 0
                    assert bool((_bits(Rb[:rows][behind]) == 0).all()), "a row behind a count must be +0.0"
                    assert bool((_bits(got["R"][behind]) == 0).all())
                tight = _call(ops, form, c, d, g, rb=(rows, ldrb))                                                   # no tail
                _equal_bits(tight["Rb"], Rb[:rows], "the copy with rb_rows = rows")
            _call(ops, form, c, d, g, rb=(rows - 1, _pad32(O)), expect=BADARG)                                       # 5
            _call(ops, form, c, d, g, rb=(_pad32(rows), _pad32(O) - 4), expect=BADARG)
            _call(ops, form, c, d, g, rb=(_pad32(rows), O), expect=BADARG)


@pytest.mark.parametrize("O,L", [(8, 5), (40, 37), (1000, 5)])
def test_len_form_at_full_counts_is_the_plain_rb_kernel(ops, O, L):
    """every count equal to L: R, rowssq and the copy carry the bits of vqf_mfb_fuse_fwd_pbf16_rb (whose copy has N L rows)"""
    c = _case("len", O, L, [L] * N)
    cp = K._case("pbf16", N, L, O)
    for mask in K.MASKS:
        d = K._build(c, "random", mask)
        d["P"] = d["P"].to(torch.bfloat16).double()
        g = _operands(c, d)
        ldrb = _pad32(O)
        got = _call(ops, "len", c, d, g, rb=(_pad32(N * L), ldrb))
        want = K._fwd(ops, cp, dict(d, own=N), g, ldrb=ldrb)
        _equal_bits(got["R"], want["R"], "R")
        _equal_bits(got["rowssq"], want["rowssq"], "rowssq")
        _equal_bits(got["Rb"][:N * L], want["Rb"], "the copy")
        assert bool((_bits(got["Rb"][N * L:]) == 0).all())

"""The GEMM kernel families on their own (csrc/gemm_f32.hip, gemm_f32_wave.hip, gemm_f32_n80.hip, gemm_f32_big.hip,
gemm_f32_sample.hip, gemm_bf16.hip and the batched entry), element by element against the fp64 reference tests/gemm_ref.py
(pinned on torch.matmul by tests/test_gemm_ref_cpu.py), at the SMALLEST shapes that reach each path: the workgroup-index remap
with a partial last group, both loader templates with K tails, the smallest K that splits, idle waves, dead sub-tiles.

Every case runs two data sets:
  exact    seeded integers (powers of two for row scales): every product and every partial sum, in any order, is an fp32
           number (max sum |terms| < 2^24 is asserted), so the kernel must return the reference's bits.  A dropped k term, a
           slab counted twice, a bias added per split or a tile stored at the wrong offset cannot hide behind rounding.
  random   fp32 values; per ELEMENT |got - ref| <= (k + 1) 2^-24 sum |terms|.  k is an upper limit on the additions a term
           passes through (k_of below names the source lines it counts from).  u = 2^-24 assumes that the matrix pipe rounds
           each accumulate to nearest; nothing is fitted to the kernels, the worst err / bound is logged
           (profiles/gemm_small_parity.txt).
Every operand with a leading dimension, an offset or a batch stride lives in a buffer of NaN, every output in a buffer of 7.0
with guard floats in front, behind and between the rows of a strided view (the rowscale wrappers allocate their own output:
no guards there); every call is made twice and must give the same bits.  The launchers' routing is restated below and every
case asserts the family (ops.stat deltas: the named family + 1 per call, every other family + 0), the number of splitk_reduce
launches (profiler) and the form the restated rules give.  A case whose route is not reached FAILS; shapes that depend on the
CU count are computed from the device.  Variants of a case (another placement, another library option) that run the same
additions in the same order must give the bits of the case's first run."""
import functools

import numpy as np
import pytest
import torch

import gemm_ref as GR
from golden_util import _report_parity

pytestmark = pytest.mark.gpu

KINDS = ("exact", "random")
WS_BYTES = 192 << 20                          # host/ops.py SPLITK_WS_BYTES: what ops.gemm hands the launcher at least
STAT_OF = {"tile128": "gemm_f32_tile128", "batched": "gemm_f32_tile128", "big": "gemm_f32_big", "wave": "gemm_f32_wave",
           "n80": "gemm_f32_n80", "sample": "gemm_f32_sample", "bf16": "gemm_bf16_tile128"}
STATS = ("gemm_f32_tile128", "gemm_f32_big", "gemm_f32_wave", "gemm_bf16_tile128", "gemm_bf16_big", "gemm_f32_sample", "gemm_f32_n80")
T128 = dict(gemm_f32_big=0, gemm_f32_wave=0, gemm_f32_n80=0)      # pins the 128x128 fp32 kernel
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _cdiv(a, b):
    return -(-a // b)


# ---- the launchers' routing, restated -----------------------------------------------------------------------------------------------
def splitk_chunks(K, slab_k, wanted):
    """gemm_host.h:47-52 vqf_splitk_chunks -> (splits that are not empty, K range of a split)"""
    per = _cdiv(_cdiv(K, slab_k), wanted)
    return _cdiv(K, per * slab_k), per * slab_k


def tile128_splits(tiles, ktiles, M, N, ws_bytes):
    """gemm_host.h:69-83 vqf_tile128_splits: 512 slots, cost = rounds / sp * (1 + 0.01 sp), at least 16 K tiles per split"""
    splits, best = 1, 1e30
    for sp in range(1, 17):
        if ktiles // sp < 16 or sp * M * N * 4 > ws_bytes:
            break
        cost = float((tiles * sp + 511) // 512) / sp * (1.0 + 0.01 * sp)
        if cost < best - 1e-12:
            best, splits = cost, sp
    return splits


def f32_tile128_plan(M, N, K, ws_bytes):
    """gemm_f32.hip:563-572 (the gate at :570) -> (splits, kchunk) of the 128x128x16 kernel"""
    tiles, ktiles, splits = _cdiv(M, 128) * _cdiv(N, 128), _cdiv(K, 16), 1
    if ws_bytes and tiles < 1024 and ktiles >= 32 and not (tiles >= 512 and K <= 1024) and not (192 <= tiles <= 256 and K <= 512):
        splits = tile128_splits(tiles, ktiles, M, N, ws_bytes)
    return splitk_chunks(K, 16, splits)


def bf16_tile128_plan(M, N, K, ws_bytes, rowscale):
    """gemm_bf16.hip:327-331 -> (splits, kchunk) of the 128x128x32 kernel"""
    tiles, ktiles, splits = _cdiv(M, 128) * _cdiv(N, 128), _cdiv(K, 32), 1
    if ws_bytes and not rowscale and tiles < 1024 and ktiles >= 32:
        splits = tile128_splits(tiles, ktiles, M, N, ws_bytes)
    return splitk_chunks(K, 32, splits)


def vec_ok(ld, off, bstride=0):
    """gemm_f32.hip:559-560 and :654-655: 16-byte vector loads of an operand (base `off` floats behind a 16-byte boundary)"""
    return off % 4 == 0 and ld % 4 == 0 and bstride % 4 == 0


def tile128_template(ta, tb, M, N, vecA, vecB):
    """gemm_f32.hip:488-492: the clamped loaders ("fast") need vector operands and, K-major, a row extent % 4 == 0 and >= 4"""
    okA = vecA and (not ta or (M % 4 == 0 and M >= 4))
    okB = vecB and (not tb or (N % 4 == 0 and N >= 4))
    return "fast" if okA and okB else "guarded"


def wave_form(ta, tb, M, N, K, vec, opt):
    """gemm_f32_wave.hip:556-587 vqf_gemm_f32_wave_try -> None (not this kernel) | "plain" | "shb" | "wk4"; opt: the option
    gemm_f32_wave (None: unset)"""
    if opt == 0:                                                                  # :558
        return None
    if ta or M > 1024 or K % 16 or K < 256 or not vec:                            # :559
        return None
    if tb and N % 4:                                                              # :560
        return None
    if _cdiv(M, 128) * _cdiv(N, 128) >= 256:                                      # :562
        return None
    tiles_m, tiles_n = _cdiv(M, 32), _cdiv(N, 64)
    tiles = tiles_m * tiles_n
    nwg1, nwg4 = _cdiv(tiles, 4), tiles
    ok4 = K % 64 == 0 and K // 4 >= 256                                           # :570
    if 192 <= nwg1 <= 256:                                                        # :574
        return "shb" if (tiles_m % 4 == 0 and tiles % 4 == 0 and opt != 1) else "plain"   # :581
    if ok4 and 192 <= nwg4 <= 256:                                                # :575
        return "wk4"
    return None


def n80_takes(ta, tb, M, N, K, other_flags, vec, cus, opt):
    """gemm_f32.hip:618 and gemm_f32_n80.hip:238-256: one round of 128x80 tiles that fills at least 0.8 of the CUs; cus None: False
    where no CU count could make it take the product, else None (needs the CU count)"""
    if ta or tb or opt == 0 or other_flags or K % 128 or K < 512 or not vec or M > 1024:
        return False
    if cus is None:
        return None
    tiles = _cdiv(M, 128) * _cdiv(N, 80)
    return not (tiles > cus or tiles * 10 < cus * 8)


def big_pick_splits(tiles, K, M, N, ws_bytes):
    """gemm_f32_big.hip:660-674 pick_splits"""
    if tiles >= 768:
        return 1
    best, best_cost = 1, 1e30
    for sp in range(1, 33):
        if sp > 1 and (sp * M * N * 4 > ws_bytes or K // sp < 16 * 16):
            break
        rounds = float((tiles * sp + 255) // 256)
        slabs = (K // 16 + sp - 1) // sp
        cost = rounds * slabs * 16 * 0.213 + (sp * float(M) * N * 8.0 / 4.0e6 if sp > 1 else 0.0)
        if cost < best_cost - 1e-9:
            best_cost, best = cost, sp
    return best


def big_applies(ta, tb, M, N, K, acc, ws_bytes, sw):
    """gemm_f32_big.hip:724-745 big_applies; sw: the option gemm_f32_big (1 = default, 2 = wherever the kernel can run, :729)"""
    if sw == 0 or K % 4 or K < 64 or M < 256 or N < 128 or acc:                   # :726
        return False
    if (ta and M % 4) or (tb and N % 4):                                          # :727-728
        return False
    if sw == 2:                                                                   # :729
        return True
    tiles = _cdiv(M, 256) * _cdiv(N, 256)
    if tiles >= 1024:
        return K >= 1536
    if ta and tb and K >= 16384 and tiles * big_pick_splits(tiles, K, M, N, ws_bytes) >= 256:
        return True
    return bool(ta and tb and K >= 4096 and _cdiv(N, 256) * 256 * 100 <= N * 107
                and tiles * big_pick_splits(tiles, K, M, N, ws_bytes) >= 256)


def whole_round_rows(ta, tb, M, N, K, acc, sw, cus):
    """gemm_f32_big.hip:754-766 whole_round_rows: the leading rows whose 256x256 tiles fill whole rounds of the CUs to within 4 %;
    cus None: 0 where no chip of 8 CUs or more could take any, else None (needs the CU count)"""
    if sw == 0 or ta or acc or K % 4 or K < 256 or N < 128 or (tb and N % 4):
        return 0
    tn = _cdiv(N, 256)
    if tn * 256 * 100 > N * 107:
        return 0
    if cus is None:
        return 0 if (M // 256) * tn < 8 else None
    c = cus & ~7
    r = M // 256
    while c >= 8 and r >= 1 and r * tn >= c:
        tiles, rounds = r * tn, _cdiv(r * tn, c)
        if (rounds * c - tiles) * 25 <= rounds * c:
            return r * 256
        r -= 1
    return 0


def bf16_big_applies(ta, tb, M, N, K, acc):
    """gemm_bf16_big.hip:716-725"""
    if K % 32 or M < 256 or N < 128 or acc or (ta and M % 8) or (tb and N % 8):
        return False
    return _cdiv(M, 256) * _cdiv(N, 256) >= 64


class Spec:
    """one launch: the product, its flags, where operands and output lie, the library options, and the route its case names"""
    FIELDS = dict(batch=None, bias=False, relu=False, acc=False, rowscale=0, L=0, a=(0, 0), b=(0, 0), c=(0, 0), sa=0, sb=0, sc=0,
                  opts=None, splitk=True, bf16=False, relu_a=False, form=None, splits=1, reduce=0)

    def __init__(self, fam, ta, tb, M, N, K, **kw):
        self.fam, self.ta, self.tb, self.M, self.N, self.K = fam, int(ta), int(tb), M, N, K
        for name, default in self.FIELDS.items():
            setattr(self, name, kw.pop(name, default))
        assert not kw, kw
        self.opts = dict(self.opts or {})

    def but(self, **kw):
        """a copy with some fields replaced: fam, the flags, the placement (a, b, c: (extra floats per row, floats the base lies
        behind a 16-byte boundary); sa, sb, sc: extra floats per batch stride), opts, splitk, form, splits, reduce"""
        d = {name: getattr(self, name) for name in self.FIELDS}
        d.update(kw)
        fam = d.pop("fam", self.fam)
        return Spec(fam, self.ta, self.tb, self.M, self.N, self.K, **d)

    def data_key(self):
        return (self.ta, self.tb, self.M, self.N, self.K, self.batch, self.bias, self.acc, self.rowscale, self.bf16, self.relu_a, self.relu)

    def lds(self):
        """row pitches (lda, ldb) of the operands as stored"""
        wa = self.M if self.ta else self.K
        wb = self.N if self.tb else self.K
        return wa + self.a[0], wb + self.b[0]

    def __repr__(self):
        flags = "".join(c for c, on in (("b", self.bias), ("r", self.relu), ("a", self.acc), ("s", self.rowscale)) if on)
        return "%s ta%d tb%d %s%dx%dx%d %s" % (self.fam, self.ta, self.tb, "" if self.batch is None else "%dx" % self.batch,
                                              self.M, self.N, self.K, flags or "-")


def route(s, cus=None):
    """-> (family, form, splits, splitk_reduce launches) as the restated rules give them, or None where the rule needs the CU
    count and cus is None.  gemm_f32.hip:597-622 gemm_f32_impl is the order of the fp32 tries."""
    o = s.opts
    if s.fam == "batched":                                                        # gemm_f32.hip:640-660: always the 128x128 kernel
        lda, ldb = s.lds()
        rows_a, rows_b = (s.K if s.ta else s.M), (s.K if s.tb else s.N)
        va = vec_ok(lda, s.a[1], rows_a * lda + s.sa)
        vb = vec_ok(ldb, s.b[1], rows_b * ldb + s.sb)
        return "batched", tile128_template(s.ta, s.tb, s.M, s.N, va, vb), 1, 0
    if s.fam == "sample":                                                         # gemm_f32_sample.hip:323-331 under gemm_f32_sample = 2
        ok = (s.L in (192, 196) and s.M % s.L == 0 and s.N >= 256 and s.N % 256 == 0 and s.K >= 64 and s.K % 16 == 0
              and o.get("gemm_f32_sample") == 2 and not s.acc and not s.ta)
        return ("sample", None, 1, 0) if ok else None
    if s.bf16:
        if o.get("gemm_bf16_big", 1) != 0 and bf16_big_applies(s.ta, s.tb, s.M, s.N, s.K, s.acc):
            return "bf16_big", None, 1, 0
        splits, _ = bf16_tile128_plan(s.M, s.N, s.K, 0 if s.rowscale else WS_BYTES, bool(s.rowscale))
        return "bf16", None, splits, int(splits > 1 and o.get("gemm_splitk_fused", 0) != 1)
    lda, ldb = s.lds()
    va, vb = vec_ok(lda, s.a[1]), vec_ok(ldb, s.b[1])
    ws = WS_BYTES if (s.splitk and not s.rowscale) else 0
    sw_big = o.get("gemm_f32_big", 1)
    if va and vb:                                                                 # gemm_f32.hip:604
        big = big_applies(s.ta, s.tb, s.M, s.N, s.K, s.acc, ws, sw_big)
        if big:
            tiles = _cdiv(s.M, 256) * _cdiv(s.N, 256)
            sp = big_pick_splits(tiles, s.K, s.M, s.N, ws)
            if not (sp > 1 and (s.rowscale or s.K % 16)):                         # gemm_f32_big.hip:848
                splits, _ = splitk_chunks(s.K, 16, sp)
                fused = tiles >= 64 and o.get("gemm_splitk_fused", 1) != 0        # :870
                return "big", None, splits, int(splits > 1 and not fused)
        else:
            rows = whole_round_rows(s.ta, s.tb, s.M, s.N, s.K, s.acc, sw_big, cus)
            if rows is None:
                return None
            if rows:                                                              # (no case of this file is split by rows)
                return "big+tile128", None, 1, 0
        if not s.rowscale:                                                        # gemm_f32.hip:614-618
            form = wave_form(s.ta, s.tb, s.M, s.N, s.K, True, o.get("gemm_f32_wave"))
            if form:
                return "wave", form, 1, 0
            n80 = n80_takes(s.ta, s.tb, s.M, s.N, s.K, s.acc, True, cus, o.get("gemm_f32_n80", 1))
            if n80 is None:
                return None
            if n80:
                return "n80", None, 1, 0
    splits, _ = f32_tile128_plan(s.M, s.N, s.K, ws)
    return "tile128", tile128_template(s.ta, s.tb, s.M, s.N, va, vb), splits, int(splits > 1 and o.get("gemm_splitk_fused", 0) != 1)


def k_of(s):
    """The additions a term passes through, at most.  All kernels add a k's product to the accumulator of its element once
    (gemm_f32.hip:246-251, gemm_f32_wave.hip's 16 MFMAs per slab, gemm_f32_n80.hip, gemm_f32_big.hip, gemm_f32_sample.hip,
    gemm_bf16.hip: v_mfma with the accumulator as C): K.  Split-K adds the slabs one by one (gemm_f32.hip:475, common.h
    vqf_splitk_combine): + splits - 1.  The per-wave kernel's WK = 4 form sums four accumulators through LDS: + 3.  The row scale
    rounds once (gemm_f32.hip:446), the bias and the accumulate add once each (:446, :448)."""
    return s.K + (s.splits - 1) + (3 if s.form == "wk4" else 0) + int(s.bias) + int(s.acc) + int(bool(s.rowscale))


# ---- the case tables (tests/test_gemm_ref_cpu.py walks ALL_CASES: exact range, bound not too tight, routes) ------------------------
ALL_CASES = []


def _case(group, cid, spec, variants=()):
    """variants: (label, Spec, same_bits): same_bits = must equal the first run bit for bit on both data sets ("exact": on the
    integer data only)"""
    c = (group, cid, spec, list(variants))
    ALL_CASES.append(c)
    return c


def _ids(cases):
    return [c[1] for c in cases]


# a. the 128x128 fp32 kernel
REMAP_SHAPES = [("10x3 tiles last group of 2 nwg 30 K 16", 9 * 128 + 5, 2 * 128 + 40, 16), ("10x3 tiles K 48", 9 * 128 + 5, 2 * 128 + 40, 48),
                ("17x1 tiles", 16 * 128 + 3, 100, 16), ("1x17 tiles", 100, 16 * 128 + 3, 16)]
REMAP = [_case("remap", "%s ta%d tb%d" % (n, ta, tb), Spec("tile128", ta, tb, M, N, K, opts=T128,
                                                            form=tile128_template(ta, tb, M, N, True, True)))
         for n, M, N, K in REMAP_SHAPES for ta, tb in LAYOUTS]

KT_M, KT_N = 130, 97          # tile row 0: all four waves' sub-tiles inside (EDGE = false); tile row 1: 2 live rows (EDGE = true)
KTAILS = []
for _K in (1, 7, 15, 16, 17, 31, 33, 51, 68):
    _pad = (-_K) % 4 + 4
    _base = Spec("tile128", 0, 0, KT_M, KT_N, _K, opts=T128, form="fast" if _K % 4 == 0 else "guarded")
    KTAILS.append(_case("ktail", "K %d" % _K, _base, [
        ("views ld % 4 == 0 aligned", _base.but(a=(_pad, 0), b=(_pad, 0), c=(3, 0), form="fast"), True),
        ("base one float off", _base.but(a=(_pad, 1), b=(_pad, 1), c=(0, 1), form="guarded"), True)]))

KMAJOR = []
for _ta, _tb in LAYOUTS[1:]:
    for _n, _M, _N, _form in (("rows % 4 == 0", 132, 72, "fast"), ("rows % 4 != 0", 130, 70, "guarded"), ("rows < 4", 3, 2, "guarded"),
                              ("A rows % 4 == 0 B rows % 4 != 0", 132, 70, "fast" if not _tb else "guarded")):
        _base = Spec("tile128", _ta, _tb, _M, _N, 40, opts=T128, form=_form)
        KMAJOR.append(_case("kmajor", "ta%d tb%d %s" % (_ta, _tb, _n), _base,
                            [("views", _base.but(a=(4, 0), b=(8, 0), c=(1, 0)), True)]))

EDGE_MN = [1, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129]
EDGES = [_case("edge", "M %d N %d ta%d tb%d" % (M, EDGE_MN[(i * 3 + rot) % 11], t, t),
               Spec("tile128", t, t, M, EDGE_MN[(i * 3 + rot) % 11], 24, opts=T128, c=(2, 0),
                    form=tile128_template(t, t, M, EDGE_MN[(i * 3 + rot) % 11], True, True)))
         for rot in (1, 6) for i, M in enumerate(EDGE_MN) for t in (0, 1)]

FLAGS = [_case("flags", "bias %d relu %d accumulate %d" % (bi, re, ac),
               Spec("tile128", 0, 0, 130, 70, 40, opts=T128, bias=bool(bi), relu=bool(re), acc=bool(ac), c=(5, 0), form="fast"))
         for bi in (0, 1) for re in (0, 1) for ac in (0, 1)]

ROWSCALE = [_case("rowscale", "rps %d" % rps, Spec("tile128", 0, 0, 3 * 196 + 5, 200, 64, opts=T128, bias=True, relu=True, rowscale=rps,
                                                   form="fast")) for rps in (196, 1, 600)]

SPLITK = []
for _M, _N, _K in ((128, 128, 512), (130, 70, 520)):
    for _ta, _tb in LAYOUTS:
        _form = tile128_template(_ta, _tb, _M, _N, True, True)
        _base = Spec("tile128", _ta, _tb, _M, _N, _K, opts=T128, bias=True, relu=True, acc=True, c=(3, 0), form=_form, splits=2, reduce=1)
        SPLITK.append(_case("splitk", "%dx%dx%d ta%d tb%d" % (_M, _N, _K, _ta, _tb), _base, [
            ("combined in the launch", _base.but(opts=dict(T128, gemm_splitk_fused=1), reduce=0), True),
            ("splitk=False", _base.but(splitk=False, splits=1, reduce=0), "exact")]))

# b. vqf_gemm_f32_batched: HieCoAtten's per-sample products at small width (T, L, E) = (14, 196, 64) and (22, 100, 512)
BATCHED_SHAPES = [("affinity (0,0) T x L over E", 0, 0, 14, 196, 64), ("(0,1) T x E over L K % 16 = 4", 0, 1, 14, 64, 196),
                  ("(1,1) L x E over T K 14 below one K tile", 1, 1, 196, 64, 14), ("(1,0) L x T over E", 1, 0, 196, 14, 64),
                  ("(0,0) 22 x 100 over 512", 0, 0, 22, 100, 512), ("(0,1) 22 x 512 over 100 four column tiles", 0, 1, 22, 512, 100),
                  ("(1,1) 100 x 512 over 22", 1, 1, 100, 512, 22)]
BATCHED = []
for _n, _ta, _tb, _M, _N, _K in BATCHED_SHAPES:
    for _acc in (False, True):
        for _bn in ((1, 3, 300) if _K <= 64 else (3,)):
            _base = Spec("batched", _ta, _tb, _M, _N, _K, batch=_bn, acc=_acc, form=tile128_template(_ta, _tb, _M, _N, True, True))
            _var = [("column blocks of wider buffers", _base.but(a=(8, 0), b=(4, 0), c=(3, 0), sa=16, sb=8, sc=2 * (_N + 3)), True),
                    ("batch stride not a multiple of 4", _base.but(a=(4, 0), b=(4, 0), sa=2, sb=1, c=(1, 1), form="guarded"), True)]
            BATCHED.append(_case("batched", "%s batch %d accumulate %d" % (_n, _bn, _acc), _base, _var if _bn == 3 else _var[:1]))

# c. the per-wave kernel (default route: no option set)
WAVE_SHAPES_SMALL = [("WK 1 plain 3 row tiles", "plain", 96, (16384, 16384), 256), ("WK 1 plain idle wave ragged", "plain", 90, (16438, 16436), 256),
                     ("WK 1 plain odd N scalar tail", "plain", 96, (16383, None), 256),
                     ("WK 1 shared B", "shb", 128, (12288, 12288), 256), ("WK 1 shared B 32 row tiles", "shb", 1024, (2048, 2048), 256),
                     ("WK 4", "wk4", 32, (12800, 12800), 1024), ("WK 4 ragged", "wk4", 30, (12790, 12788), 1024)]
WAVE = []
for _n, _form, _M, _Ns, _K in WAVE_SHAPES_SMALL:
    for _tb in (0, 1):
        if _Ns[_tb] is None:
            continue
        _plain = Spec("wave", 0, _tb, _M, _Ns[_tb], _K, form=_form)
        _own_b = [("gemm_f32_wave=1 every wave its own B", _plain.but(opts=dict(gemm_f32_wave=1), form="plain"), True)] if _form == "shb" else []
        WAVE.append(_case("wave", "%s tb%d no flags" % (_n, _tb), _plain, _own_b))
        _even = 2 - _Ns[_tb] % 2                                                  # even ldc, 8-byte aligned base: 8-byte c_prefetch / put2
        _acc = _plain.but(bias=True, relu=True, acc=True, c=(_even, 0))
        WAVE.append(_case("wave", "%s tb%d bias relu accumulate" % (_n, _tb), _acc, [
            ("odd ldc", _acc.but(c=(3 - _even, 0)), True), ("base 4 bytes off", _acc.but(c=(_even, 1)), True)]))


# d. the 128x80 kernel: shapes with ceil(M / 128) ceil(N / 80) in [0.8 CUs, CUs], from the device's CU count
def n80_shapes(cus):
    return [("one row tile ragged N", 100, 80 * (cus * 210 // 256) - 3, 512), ("8 row tiles", 1024, 80 * (cus * 28 // 256), 512),
            ("one row tile K 640", 100, 80 * (cus * 210 // 256) - 3, 640)]


def n80_cases(cus):
    out = []
    for n, M, N, K in n80_shapes(cus):
        base = Spec("n80", 0, 0, M, N, K, bias=True, relu=True, relu_a=True, a=(4, 0), b=(8, 0), c=(3, 0))
        off = base.but(fam="tile128", opts=dict(gemm_f32_n80=0), form="fast")
        off.splits, _ = f32_tile128_plan(M, N, K, WS_BYTES)
        off.reduce = int(off.splits > 1)
        out.append(("n80", n, base, [("gemm_f32_n80=0 the 128x128 kernel", off, False)]))
    return out


ALL_CASES.extend(n80_cases(256))              # (the CPU test walks the 256-CU shapes; the GPU test computes its own)

# e. the large-tile fp32 kernel under gemm_f32_big = 2
BIG = []
for _M, _N, _K in ((256, 128, 64), (300, 392, 68), (520, 264, 1036)):
    for _ta, _tb in LAYOUTS:
        _o = dict(gemm_f32_big=2)
        _base = Spec("big", _ta, _tb, _M, _N, _K, opts=_o, splitk=False, bias=True, relu=True, c=(3, 0))
        _var = [("one workgroup per tile", _base.but(opts=dict(_o, gemm_f32_persist=0)), True),
                ("gemm_f32_big=0 the 128x128 kernel", _base.but(fam="tile128", opts=dict(gemm_f32_big=0),
                                                                form=tile128_template(_ta, _tb, _M, _N, True, True)), True)]
        if (_ta, _tb) == (0, 0):
            _var += [("no short-edge path", _base.but(opts=dict(_o, gemm_f32_edge=0)), True),
                     ("no short-edge path one workgroup per tile", _base.but(opts=dict(_o, gemm_f32_edge=0, gemm_f32_persist=0)), True)]
        BIG.append(_case("big", "%dx%dx%d ta%d tb%d" % (_M, _N, _K, _ta, _tb), _base, _var))
BIG.append(_case("big", "split-K 256x256x16384 ta1 tb1 slabs and one reduce",
                 Spec("big", 1, 1, 256, 256, 16384, opts=dict(gemm_f32_big=2), bias=True, relu=True, c=(3, 0), splits=32, reduce=1)))

# f. the per-sample kernel under gemm_f32_sample = 2 (MAXRAG = 1, gemm_f32_sample.hip:34: L = 192 and 192 + 4 MAXRAG = 196)
SAMPLE = []
for _L in (192, 196):
    for _K in (64, 80):
        for _tb in (0, 1):
            for _NS in (1, 3):
                _base = Spec("sample", 0, _tb, _NS * _L, 256, _K, L=_L, opts=dict(gemm_f32_sample=2), bias=True, relu=True, relu_a=True, c=(2, 0))
                SAMPLE.append(_case("sample", "NS %d L %d K %d tb%d" % (_NS, _L, _K, _tb), _base, [
                    ("vqf_gemm_f32 on the same values", _base.but(fam="tile128", opts=dict(gemm_f32_sample=0),
                                                                 form=tile128_template(0, _tb, _NS * _L, 256, True, True)), "exact")]))

# g. the 128x128 bf16 kernel (K-major operands need a row extent % 8 == 0: the ragged shape moves to the next multiple there)
BF16 = []
for _n, _M, _N, _K, _splits in (("8x8x8", 8, 8, 8, 1), ("136x264x72", 136, 264, 72, 1), ("130x70x1032 split-K", 130, 70, 1032, 2)):
    for _ta, _tb in LAYOUTS:
        _Mv, _Nv = (_M if not _ta else _cdiv(_M, 8) * 8), (_N if not _tb else _cdiv(_N, 8) * 8)
        for _fl, _kw in (("no flags", {}), ("accumulate", dict(acc=True)), ("accumulate relu bias", dict(acc=True, relu=True, bias=True))):
            BF16.append(_case("bf16", "%s ta%d tb%d %s" % (_n, _ta, _tb, _fl),
                              Spec("bf16", _ta, _tb, _Mv, _Nv, _K, bf16=True, a=(8, 0), b=(16, 0), c=(3, 0), splits=_splits,
                                   reduce=int(_splits > 1), **_kw)))
BF16_ROWSCALE = [_case("bf16_rowscale", "rps %d" % rps, Spec("bf16", 0, 0, 3 * 196 + 5, 200, 64, bf16=True, bias=True, relu=True, rowscale=rps))
                 for rps in (196, 1)]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd.ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=6)
def reference(kind, key):
    """the data of a case and its fp64 reference, computed once per (data set, product, flags) and shared by its variants"""
    ta, tb, M, N, K, batch, bias, acc, rowscale, bf16, relu_a, relu = key
    seed = 1000 + (M * 31 + N * 17 + K * 7 + ta * 2 + tb + (batch or 0) * 3) % 100000
    d = GR.operands(kind, ta, tb, M, N, K, seed, batch=batch, bias=bias, c0=acc, rowscale=rowscale, bf16=bf16, relu_a=relu_a)
    ref, terms = GR.product(d["A"], d["B"], ta, tb, bias=d["bias"], c0=d["c0"], rowscale=d["rowscale"], rps=rowscale or 1, relu=relu)
    for v in list(d.values()) + [ref, terms]:
        if v is not None:
            v.setflags(write=False)
    return d, ref, terms


class _Placed:
    """x (rows, cols) or (batch, rows, cols) as a GPU view with row pitch cols + pad and batch stride rows * pitch + extra that starts
    `off` elements behind a 16-byte aligned address; every other element of the buffer (16 bytes in front, the pitch's tail, the
    batch stride's tail, 16 bytes behind) holds `fill`"""

    def __init__(self, shape, pad, off, extra, fill, dtype=torch.float32):
        self.lead = len(shape) == 3
        bn, rows, cols = shape if self.lead else (1,) + tuple(shape)
        ld = cols + pad
        bs = rows * ld + extra
        front = 16 // torch.empty((), dtype=dtype).element_size() + off
        self.fill = fill
        self.buf = torch.full((front + bn * bs + 8,), fill, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.v3 = torch.as_strided(self.buf, (bn, rows, cols), (bs, ld, 1), front)
        self.view = self.v3 if self.lead else self.v3[0]

    def put(self, x):
        self.v3.copy_(torch.tensor(x).reshape(self.v3.shape).to(self.buf.dtype))
        return self

    def take(self):
        """the view's content; the rest of the buffer must still hold the fill"""
        torch.cuda.synchronize()
        got = self.v3.clone()
        self.v3.fill_(self.fill)
        assert bool((self.buf == self.fill).all()), "guard floats around the output were written"
        return got.cpu().numpy().reshape(self.view.shape)


def _launches(ops, call):
    """call() with the profiler on -> {kernel id name: launches}"""
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        call()
        torch.cuda.synchronize()
        return {k: v[0] for k, v in ops.prof_report().items()}
    finally:
        ops.prof_reset()
        ops.prof_enable(False)


def _launch(ops, s, d, out):
    """one call through the public wrapper of the spec's entry point, into out.view"""
    dt = torch.bfloat16 if s.bf16 else torch.float32
    A = _Placed(d["A"].shape, s.a[0], s.a[1], s.sa, float("nan"), dt).put(d["A"]).view
    B = _Placed(d["B"].shape, s.b[0], s.b[1], s.sb, float("nan"), dt).put(d["B"]).view
    bias = None if d["bias"] is None else torch.tensor(d["bias"]).cuda()
    rs = None if d["rowscale"] is None else torch.tensor(d["rowscale"]).cuda()

    def call():
        if s.acc:
            out.put(d["c0"])
        ta, tb = bool(s.ta), bool(s.tb)
        if s.batch is not None:
            res = ops.bgemm(A, B, ta=ta, tb=tb, out=out.view, accumulate=s.acc)
        elif s.L:
            res = ops.gemm_rows(A, B, s.L, tb=tb, bias=bias, relu=s.relu, out=out.view)
        elif s.bf16 and s.rowscale:
            res = ops.gemm_bf16_rowscale(A, B, rs, s.rowscale, bias=bias, relu=s.relu)
        elif s.bf16:
            res = ops.gemm_bf16(A, B, ta=ta, tb=tb, bias=bias, relu=s.relu, out=out.view, accumulate=s.acc)
        elif s.rowscale:
            res = ops.gemm_rowscale(A.contiguous(), B.contiguous(), rs, s.rowscale, bias=bias, relu=s.relu)
        else:
            res = ops.gemm(A, B, ta=ta, tb=tb, bias=bias, relu=s.relu, out=out.view, accumulate=s.acc, splitk=s.splitk)
        if res.data_ptr() != out.view.data_ptr():
            out.view.copy_(res)
    return call


def run_spec(ops, cus, s, kind, rep, name):
    """One spec on one data set: the route the spec names is the route the restated rules give and the route the counters show,
    two calls give the same bits, guards intact, exact data: the reference's bits, random data: the bound.  -> the result"""
    assert route(s, cus) == (s.fam, s.form, s.splits, s.reduce), (name, route(s, cus))
    d, ref, terms = reference(kind, s.data_key())
    shape = ref.shape
    out = _Placed(shape, s.c[0], s.c[1], s.sc, 7.0)
    call = _launch(ops, s, d, out)
    with ops.options(**s.opts):
        before = {n: ops.stat(n) for n in STATS}
        counts = _launches(ops, call)
        got = out.take()
        call()
        again = out.take()
        delta = {n: ops.stat(n) - before[n] for n in STATS}
    assert delta == {n: (2 if n == STAT_OF[s.fam] else 0) for n in STATS}, (name, delta)
    assert counts.get("splitk_reduce", 0) == s.reduce, (name, counts)
    assert sum(counts.values()) == 1 + s.reduce, (name, counts)
    assert got.tobytes() == again.tobytes(), (name, "two calls, different bits")
    assert not np.isnan(got).any(), (name, "NaN in the output")
    if kind == "exact":
        assert float(terms.max()) < GR.EXACT_LIMIT, (name, "the exact data set left the exact range")
        nbad, first = GR.same_bits(got, ref)
        assert nbad == 0, (name, "%d of %d elements differ from the fp64 reference, first at %s"
                           % (nbad, got.size, np.unravel_index(first, shape)))
        rep.equal.append(name)
    else:
        worst, at = GR.check(got, ref, terms, k_of(s))
        print("%s %s: k %d worst err/bound %.3f" % (rep.label, name, k_of(s), worst))
        rep.items[name] = worst
        assert worst <= 1.0, (name, worst, np.unravel_index(at, shape))
    return got


class _Report:
    def __init__(self, group, cid):
        self.label, self.items, self.equal = "gemm_small %-13s %s" % (group, cid), {}, []

    def flush(self, k):
        name = max(self.items, key=self.items.get)
        _report_parity(self.label + " k %d" % k, self.items[name], name, "  " + " ".join("%s=%.3f" % (n.replace(" ", "_"), v) for n, v in self.items.items())
                       + "  exact data: equal (%d runs)" % len(self.equal))


def run_case(ops, cus, case):
    group, cid, spec, variants = case
    rep = _Report(group, cid)
    for kind in KINDS:
        first = run_spec(ops, cus, spec, kind, rep, "first")
        for label, v, same in variants:
            got = run_spec(ops, cus, v, kind, rep, label)
            if same is True or same == kind:
                assert got.tobytes() == first.tobytes(), (cid, label, kind, "not the bits of the case's first run")
            else:                             # two kernels, two orders: within the sum of both bounds of the same reference
                _, ref, terms = reference(kind, spec.data_key())
                assert (np.abs(got.astype(np.float64) - first) <= GR.bound(terms, k_of(spec)) + GR.bound(terms, k_of(v))).all(), (cid, label)
    rep.flush(k_of(spec))


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REMAP, ids=_ids(REMAP))
def test_tile128_workgroup_index_remap(ops, cus, case):
    """gemm_f32.hip:394-409: the XCD remap with nwg % 8 != 0 and a last GROUP_M group of fewer than 8 row tiles; a tile computed
    twice or not at all, or stored at another tile's place, shows on the integer data"""
    spec = case[2]
    tiles_m, tiles_n = _cdiv(spec.M, 128), _cdiv(spec.N, 128)
    assert (tiles_m * tiles_n) % 8 != 0 and (tiles_m % 8 != 0 or tiles_m == 1)
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", KTAILS, ids=_ids(KTAILS))
def test_tile128_k_tails_under_both_loader_templates(ops, cus, case):
    """gemm_f32.hip:351-375: K tails (K < BK, K % 16 in 1 .. 15, K % 4 != 0) contiguous, as aligned views (clamped loaders with a
    guarded tail) and one float off (guarded loaders): the k order is the same, so are the bits"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", KMAJOR, ids=_ids(KMAJOR))
def test_tile128_k_major_operands(ops, cus, case):
    """gemm_f32.hip:156-157 clamps a K-major operand's row to R - 4: only with R % 4 == 0 and R >= 4 (:488-489)"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", EDGES, ids=_ids(EDGES))
def test_tile128_edge_sub_tiles(ops, cus, case):
    """gemm_f32.hip:230-234, :423: sub-tiles entirely outside the matrix are skipped, the border ones are guarded in the epilogue"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", FLAGS, ids=_ids(FLAGS))
def test_tile128_epilogue_flags(ops, cus, case):
    """gemm_f32.hip:438-455: bias, then the output's earlier content, then the ReLU, into a row-strided view"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", ROWSCALE, ids=_ids(ROWSCALE))
def test_tile128_rowscale(ops, cus, case):
    """vqf_gemm_f32_rowscale, gemm_f32.hip:446: rowscale[row / rps] on the sum, not on the bias; samples of 196 rows and a short last one"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", SPLITK, ids=_ids(SPLITK))
def test_tile128_split_k_at_the_smallest_k_that_splits(ops, cus, case):
    """gemm_f32.hip:570-587: two K slices + the reduce launch (bias, accumulate and ReLU in the reduce, :466-482), the same slices
    combined in the launch (gemm_splitk_fused = 1: same bits, no reduce launch), and unsplit"""
    spec = case[2]
    splits, kchunk = f32_tile128_plan(spec.M, spec.N, spec.K, WS_BYTES)
    assert splits == 2 and kchunk % 16 == 0 and kchunk < spec.K
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", BATCHED, ids=_ids(BATCHED))
def test_batched_gemm(ops, cus, case):
    """vqf_gemm_f32_batched (gemm_f32.hip:640-660): grid.z = batch over every layout, accumulate, strided views, batch strides that
    disable the vector loaders"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", WAVE, ids=_ids(WAVE))
def test_per_wave_kernel(ops, cus, case):
    """gemm_f32_wave.hip on its default route: the plain WK = 1 form (row tiles not in fours, idle waves in the last workgroup),
    the shared-B form, WK = 4, both c_prefetch / put2 forms under accumulate"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("which", range(3), ids=[n for n, _, _, _ in n80_shapes(256)])
def test_128x80_kernel(ops, cus, which):
    """gemm_f32_n80.hip: one round of 128x80 tiles, per element, and against the 128x128 kernel within the sum of both bounds"""
    case = n80_cases(cus)[which]
    spec = case[2]
    assert cus * 8 <= _cdiv(spec.M, 128) * _cdiv(spec.N, 80) * 10 and _cdiv(spec.M, 128) * _cdiv(spec.N, 80) <= cus
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", BIG, ids=_ids(BIG))
def test_large_tile_kernel_at_small_shapes(ops, cus, case):
    """gemm_f32_big.hip under gemm_f32_big = 2 (:729): one tile with dead columns, ragged tiles with a zero-filled last slab, K
    shorter than the prologue; persistent and one workgroup per tile, with and without the short-edge path: the bits of the
    128x128 kernel.  Deep K on one tile: 32 slabs and one reduce launch (:866-870, fewer than 64 tiles)"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", SAMPLE, ids=_ids(SAMPLE))
def test_per_sample_kernel(ops, cus, case):
    """gemm_f32_sample.hip under gemm_f32_sample = 2: whole and ragged samples, K of four and five slabs, both B layouts"""
    run_case(ops, cus, case)


@pytest.mark.parametrize("case", BF16 + BF16_ROWSCALE, ids=_ids(BF16 + BF16_ROWSCALE))
def test_bf16_tile128_kernel(ops, cus, case):
    """gemm_bf16.hip: every layout, K below one K tile, K tails, split-K, and the VQF_GEMM_ACCUM epilogue (:241) the bf16 LSTM
    recursion uses, into a strided fp32 view; vqf_gemm_bf16_rowscale"""
    run_case(ops, cus, case)

"""The reduction kernels of csrc/reduce.hip and the logit-head kernels of csrc/attention.hip (att_logits_*) on their own, every
code path, element by element against the fp64 reference tests/reduce_kernels_ref.py (pinned on autograd by
tests/test_reduce_kernels_ref_cpu.py).  They sit under every bias gradient, under F.normalize and under the attention heads.

Every case runs two data sets:
  exact    small integers (powers of two for scales): every product and every partial sum, in any order, is an fp32 number
           (sum |terms| < 2^24 is asserted), so the result must be the reference's bits.  A dropped, doubled or misplaced row,
           or a column written by the wrong tile, cannot hide behind rounding.  Where a root or a quotient is taken
           (vqf_l2_group_norm) those outputs get 2^-22 relative: one rounding each, doubled.
  random   fp32 values; per ELEMENT |got - ref| <= (k + 1) 2^-24 sum |terms|, k = the longest chain of additions a term passes
           through as the kernel is written (in the thread, across the LDS slots, through the partial-row reduction; the + 1 is
           the product's rounding).  The k_* functions below count it, each from the source lines it names.  No tolerance is
           fitted to the kernels; the worst err / bound per output is logged (profiles/reduce_kernels_parity.txt).
Every output lives in a buffer pre-filled with 7.0 with guard floats in front and behind (and the workspace has a guard behind
it); every operand with a leading dimension or an offset lives in a buffer of NaN; every call is made twice and must give the
same bits.  The launchers' routing is restated at the top of this file and every case asserts the branch its id names, with the
profiler's launch counts where they tell branches apart.  The refusals assert the exact VQF_E_* code and untouched outputs."""
import math

import pytest
import torch

import reduce_kernels_ref as RR
from golden_util import _report_parity

pytestmark = pytest.mark.gpu

NAN = float("nan")
BADARG, ALIGN, UNSUPPORTED, WORKSPACE = -1, -2, -3, -4      # include/vqa_fusion.h VQF_E_*
KINDS = ("exact", "random")


def _cdiv(a, b):
    return -(-a // b)


# ---- the launchers' routing, restated -----------------------------------------------------------------------------------------------
CS_ROWS, REDUCE_SPLITS, LB_ROWS = 256, 32, 128              # reduce.hip:7, common.h:95 (VQF_REDUCE_SPLITS), attention.hip:89


def cs_rows_vec(M, N, capped=True):
    """reduce.hip:11-16 cs_rows_vec: rows per workgroup of the 16-byte column-sum kernels"""
    tiles_c = (N // 4 + 255) // 256
    rpb = ((M * tiles_c // 512 + 7) // 8) * 8
    cap = 64 if (M > 16384 and capped) else (CS_ROWS if capped else 1 << 30)
    return min(max(rpb, 16), cap)


def att_bwd_rows_per_block(M):
    """attention.hip:90-93 att_bwd_rows_per_block"""
    lb = ((M // 512 + 3) // 4) * 4
    return min(max(lb, 16), LB_ROWS)


def colreduce_branch(J):
    """reduce.hip:305-320 vqf_colreduce_2stage: J <= 2 VQF_REDUCE_SPLITS = 64 -> group_reduce_kernel; J <= 4096 -> colreduce_one_kernel
    (one launch); else group_reduce_stage1_kernel + group_reduce_kernel (two launches).  All under the profiler id group_reduce."""
    return "group_reduce" if J <= 2 * REDUCE_SPLITS else ("colreduce_one" if J <= 4096 else "group_reduce_stage1")


def colsum_route(M, N, ldy, aligned):
    """reduce.hip:334-355 vqf_colsum_f32 (with a sufficient, aligned workspace) -> (kernel route, partial rows, reducer branch)"""
    nb = _cdiv(M, CS_ROWS)
    vec_ok = N % 4 == 0 and ldy % 4 == 0 and aligned                             # :338
    if nb == 1 and not (vec_ok and M >= 64):                                     # :339
        return "scalar_single", 1, None
    if vec_ok:                                                                   # :345
        nbv = _cdiv(M, cs_rows_vec(M, N))
        return "vec", nbv, colreduce_branch(nbv)
    return "scalar_multi", nb, colreduce_branch(nb)


def col_tiles(C):
    """reduce.hip:41-44 / 147-150: per column tile (float4 columns of the tile, CT = next power of two >= them, RS = 256 / CT)"""
    out = []
    for t in range((C // 4 + 255) // 256):
        w = min(256, C // 4 - t * 256)
        CT = 1
        while CT < w:
            CT <<= 1
        out.append((w, CT, 256 // CT))
    return out


# ---- k: the longest chain of additions ----------------------------------------------------------------------------------------------
def k_serial4(n):
    """reduce.hip:24-33 (colsum_partial_kernel) and :119-128 (group_reduce_stage1_kernel): n rows over four accumulators, the < 4 left
    into a0, then (a0 + a1) + (a2 + a3)"""
    return n // 4 + n % 4 + 2


def k_group_reduce(J):
    """reduce.hip:77-81 group_reduce_kernel: two accumulators, a0 + a1"""
    return (J + 1) // 2 + 1


def k_slot8(nt):
    """reduce.hip:52-61 and :94-103: a slot's nt rows, eight per trip into acc[q & 3] (two each), the < 8 left into acc[0], then
    (acc0 + acc1) + (acc2 + acc3)"""
    return 2 * (nt // 8) + nt % 8 + 2


def k_colreduce(J):
    """reduce.hip:305-320 by branch; colreduce_one_kernel: 16 slots of ceil(J / 16) rows (:94-103) folded in slot order (:106-108)"""
    b = colreduce_branch(J)
    if b == "group_reduce":
        return k_group_reduce(J)
    if b == "colreduce_one":
        return k_slot8(_cdiv(J, 16)) + 15
    chunk = _cdiv(J, REDUCE_SPLITS)
    return k_serial4(chunk) + k_group_reduce(_cdiv(J, chunk))


def k_colsum(M, N, ldy, aligned):
    route, nb, _ = colsum_route(M, N, ldy, aligned)
    if route == "scalar_single":
        return k_serial4(M)
    if route == "scalar_multi":
        return k_serial4(CS_ROWS) + k_colreduce(nb)
    rpb = cs_rows_vec(M, N)                                   # the widest chain over the column tiles; slots folded at :64-65
    return max(k_slot8(_cdiv(rpb, RS)) + RS - 1 for _, _, RS in col_tiles(N)) + k_colreduce(nb)


def k_rank1_dbias(M, C):
    """reduce.hip:157-189: an element is w * dp, + dX, * scale (3 roundings); a slot adds its rows one by one (:175, :178), the
    slots are folded in order (:186-187), then the partial rows (:399)"""
    rpb = cs_rows_vec(M, C)
    nb = _cdiv(M, rpb)
    return 3 + max(_cdiv(rpb, RS) + RS - 1 for _, _, RS in col_tiles(C)) + (k_colreduce(nb) if nb > 1 else 0)


def k_wave_row(W, vec):
    """reduce.hip:238-247 (rowdot) and attention.hip:47-73 (att_logits_fwd): a lane adds x0 y0 + x1 y1 + x2 y2 + x3 y3 (3) to its
    accumulator once per 256 columns, or one product per 64 columns on the scalar path; wave_sum: 6 shuffle steps (common.h:187-191)"""
    return (3 + _cdiv(W, 256) if vec else _cdiv(W, 64)) + 6


def k_wave_sum(L):
    """reduce.hip:258-259, :276-277, :293-294: a lane adds every 64th value, then wave_sum"""
    return _cdiv(L, 64) + 6


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd.ops


def _cu(x):
    return None if x is None else x.float().contiguous().cuda()


def _data(kind, shape, seed, scale=1.0):
    return RR.ints(shape, seed) if kind == "exact" else RR.rnd(shape, seed, scale)


def _scales(kind, shape, seed):
    """powers of two, or random values with 0.25 <= |s| <= 1.25"""
    if kind == "exact":
        return RR.pow2(shape, seed)
    s = RR.rnd(shape, seed)
    return (torch.where(s < 0, s - 0.25, s + 0.25)).float().double()


def _in_buffer(x, ld=None, off=0):
    """x (rows, cols) or (n,) fp64 -> the same values as a GPU view with row pitch ld that starts `off` floats behind a 16-byte
    aligned address; the floats in front, between the rows and behind hold NaN"""
    x2 = x.view(1, -1) if x.dim() == 1 else x
    rows, cols = x2.shape
    ld = ld or cols
    buf = torch.full((off + rows * ld + 4,), NAN, device="cuda")
    v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(x2.float().cuda())
    return v


class _Out:
    """an output of `shape` in a buffer pre-filled with 7.0: `off` floats in front (4: 16-byte aligned, 5: one float off), 4 behind"""

    def __init__(self, *shape, off=4, dtype=torch.float32):
        n = math.prod(shape)
        self.buf = torch.full((off + n + 4,), 7.0, dtype=dtype, device="cuda")
        self.view = self.buf[off:off + n].view(*shape)

    def untouched(self):
        return bool((self.buf == 7).all())

    def take(self):
        """the result; the guards still hold 7.0"""
        torch.cuda.synchronize()
        got = self.view.clone()
        self.view.fill_(7.0)
        assert self.untouched(), "guard floats around the output were written"
        return got


class _Ws:
    """a workspace of exactly `nbytes` with 64 guard floats of 7.0 behind it"""

    def __init__(self, nbytes):
        self.nbytes, self.n = int(nbytes), (int(nbytes) + 3) // 4
        self.buf = torch.full((self.n + 64,), 7.0, device="cuda")

    def ok(self):
        return bool((self.buf[self.n:] == 7).all())


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), "two calls, different bits: " + k
    return True


def _launches(ops, call):
    """call() with the profiler on -> (its result, {kernel id name: launches})"""
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        res = call()
        torch.cuda.synchronize()
        counts = {k: v[0] for k, v in ops.prof_report().items()}
    finally:
        ops.prof_reset()
        ops.prof_enable(False)
    return res, counts


REDUCER_LAUNCHES = {None: 0, "group_reduce": 1, "colreduce_one": 1, "group_reduce_stage1": 2}


class _Report:
    def __init__(self, entry, case):
        self.label, self.items, self.equal = "reduce_kernels %-26s %s" % (entry, case), {}, set()

    def bound(self, name, got, ref, bound):
        """per element |got - ref| <= bound (a zero bound: equal)"""
        got = got.detach().cpu().double()
        ref, bound = ref.reshape(got.shape), bound.reshape(got.shape)
        err = (got - ref).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst = float(ratio.max())
        print("%s %s: worst err/bound %.3f" % (self.label, name, worst))
        assert worst <= 1.0, (self.label, name, worst, int(ratio.argmax()))
        self.items[name] = max(self.items.get(name, 0.0), worst)

    def equal_bits(self, name, got, ref, sumabs=None):
        got = got.detach().cpu()
        ref = ref.reshape(got.shape)
        if sumabs is not None:
            assert float(sumabs.max()) < 2 ** 24, (self.label, name, "the exact data set left the exact range")
        assert torch.equal(ref.float().double(), ref), (self.label, name, "reference not an fp32 number")
        bad = got != ref.float()
        assert not bool(bad.any()), (self.label, name, "%d of %d elements differ, first at %d" % (int(bad.sum()), bad.numel(), int(bad.view(-1).int().argmax())))
        self.equal.add(name)

    def check(self, kind, name, got, ref, sumabs, k):
        """exact: the reference's bits; random: (k + 1) 2^-24 sum |terms|"""
        if kind == "exact":
            self.equal_bits(name, got, ref, sumabs)
        else:
            self.bound(name, got, ref, (k + 1) * RR.U * sumabs)

    def flush(self):
        name = max(self.items, key=self.items.get)
        _report_parity(self.label, self.items[name], name, "  " + " ".join("%s=%.3f" % kv for kv in sorted(self.items.items()))
                       + "  exact data: equal (%s)" % " ".join(sorted(self.equal)))


# ---- vqf_colsum_f32 -----------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [
    # id, M, N, ldy (None: N), base offset in floats, route, reducer branch
    ("scalar single block N not a multiple of 4", 200, 37, None, 0, "scalar_single", None),
    ("scalar single block ldy not a multiple of 4 nan padding", 100, 8, 11, 0, "scalar_single", None),
    ("scalar single block base offset one float", 100, 8, None, 1, "scalar_single", None),
    ("scalar single block M below 64", 63, 8, None, 0, "scalar_single", None),
    ("vec nb 1 N 4 one column group short last block group_reduce", 70, 4, None, 0, "vec", "group_reduce"),
    ("vec N 1000 dead threads row walk tail group_reduce", 300, 1000, None, 0, "vec", "group_reduce"),
    ("vec ldy above N nan padding group_reduce", 130, 8, 12, 0, "vec", "group_reduce"),
    ("vec N 512 power of two tile colreduce_one", 5000, 512, None, 0, "vec", "colreduce_one"),
    ("vec N 1100 narrow last tile colreduce_one", 1100, 1100, None, 0, "vec", "colreduce_one"),
    ("vec N 76 eight row slots eight rows in flight colreduce_one", 30000, 76, None, 0, "vec", "colreduce_one"),
    ("vec N 4 M above 16384 rpb capped at 64 colreduce_one", 40000, 4, None, 0, "vec", "colreduce_one"),
    ("scalar multi block N not a multiple of 4 short last block group_reduce", 300, 37, None, 0, "scalar_multi", "group_reduce"),
    ("scalar multi block group_reduce_stage1 two stages", 256 * 4096 + 1, 3, None, 0, "scalar_multi", "group_reduce_stage1"),
]


@pytest.mark.parametrize("case,M,N,ld,off,route,branch", COLSUM_CASES, ids=[c[0] for c in COLSUM_CASES])
def test_colsum(ops, case, M, N, ld, off, route, branch):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    ldy = ld or N
    got_route, nb, got_branch = colsum_route(M, N, ldy, off == 0)
    assert (got_route, got_branch) == (route, branch)
    if route == "vec":                                   # what the id says about the tiles and the row walk
        rpb, tiles = cs_rows_vec(M, N), col_tiles(N)
        assert M % rpb != 0 or "capped" in case or "eight rows" in case          # a short last block
        if "dead threads" in case:
            assert tiles == [(250, 256, 1)] and (M % rpb) % 8 != 0 and M % rpb > 8   # a trip of eight, then the r += RS tail
        if "narrow last tile" in case:
            assert tiles == [(256, 256, 1), (19, 32, 8)]
        if "power of two" in case:
            assert tiles == [(128, 128, 2)]
        if "eight row slots" in case:
            assert tiles == [(19, 32, 8)] and rpb == 64                          # 8 rows per slot: exactly one trip of eight
        if "capped" in case:
            assert cs_rows_vec(M, N, capped=False) > 64 == rpb and tiles == [(1, 1, 256)]
        if "nb 1" in case:
            assert _cdiv(M, CS_ROWS) == 1 and M >= 64
    if route == "scalar_multi":
        assert M % CS_ROWS != 0
    k = k_colsum(M, N, ldy, off == 0)
    rep = _Report("colsum", "(%d, %d) ld %d off %d %s k %d" % (M, N, ldy, off, branch or route, k))
    for kind in KINDS:
        x64 = _data(kind, (M, N), 100 + M % 97)
        x = _in_buffer(x64, ldy, off)

        def run():
            out, ws = _Out(N), _Ws(lib.vqf_colsum_ws_bytes(M, N))
            assert lib.vqf_colsum_f32(p(x), M, N, ldy, p(out.view), p(ws.buf), ws.nbytes, st) == 0
            res = dict(db=out.take())
            assert ws.ok()
            return res

        a, counts = _launches(ops, run)
        assert counts.get("colsum") == 1 and counts.get("group_reduce", 0) == REDUCER_LAUNCHES[branch], counts
        assert _same(a, run())
        ref, sumabs = RR.colsum(x64)
        rep.check(kind, "db", a["db"], ref, sumabs, k)
        if ldy == N and off == 0:                       # the wrapper makes the same call
            assert torch.equal(ops.colsum(_cu(x64)), a["db"])
    rep.flush()


# ---- vqf_group_reduce_f32 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
def test_group_reduce(ops, G):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    rep = _Report("group_reduce", "G %d J 1 2 7 W 1 255 257" % G)
    for J in (1, 2, 7):
        for W in (1, 255, 257):                          # 257: a second workgroup with one live thread
            for kind in KINDS:
                x64 = _data(kind, (G * J, W), 200 + 10 * J + W % 7)
                x = _cu(x64)

                def run():
                    out = _Out(G, W)
                    assert lib.vqf_group_reduce_f32(p(x), G, J, W, p(out.view), st) == 0
                    return dict(out=out.take())

                a = run()
                assert _same(a, run())
                ref, sumabs = RR.group_reduce(x64, G, J)
                rep.check(kind, "J%d_W%d" % (J, W), a["out"], ref, sumabs, k_group_reduce(J))
    rep.flush()


# ---- vqf_relu_bwd_f32 ---------------------------------------------------------------------------------------------------------------
RELU_CASES = [
    # id, M, C, dbias
    ("grid stride second trip size not a multiple of 256 dbias scalar multi block", 4097, 513, True),
    ("no dbias odd size", 5, 7, False),
    ("dbias vec", 300, 512, True),
]


@pytest.mark.parametrize("case,M,C,want_bias", RELU_CASES, ids=[c[0] for c in RELU_CASES])
def test_relu_bwd(ops, case, M, C, want_bias):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    if "second trip" in case:                            # reduce.hip:370-371: at most 8192 workgroups of 256
        assert M * C > 8192 * 256 and (M * C) % 256 != 0 and colsum_route(M, C, C, True)[0] == "scalar_multi"
    k = k_colsum(M, C, C, True)
    rep = _Report("relu_bwd", "(%d, %d) k %d" % (M, C, k))
    for kind in KINDS:
        dx64, y64 = _data(kind, (M, C), 301), _data(kind, (M, C), 302)
        dx64[dx64 == 0] = 2.0                            # a wrongly kept element shows
        y64[0, 0], y64[0, 1], y64[M - 1, C - 1] = -0.0, 0.0, 0.0
        dx, y = _cu(dx64), _cu(y64)

        def run():
            dpre, db, ws = _Out(M, C), _Out(C), _Ws(lib.vqf_colsum_ws_bytes(M, C))
            assert lib.vqf_relu_bwd_f32(p(dx), p(y), M, C, p(dpre.view), p(db.view) if want_bias else None, p(ws.buf), ws.nbytes, st) == 0
            res = dict(dpre=dpre.take())
            if want_bias:
                res["db"] = db.take()
            else:
                torch.cuda.synchronize()
                assert db.untouched()
            assert ws.ok()
            return res

        a = run()
        assert _same(a, run())
        rpre, rdb, sumabs = RR.relu_bwd(dx64, y64)
        rep.equal_bits("dpre_" + kind, a["dpre"], rpre)                            # exactly dX or 0, whatever the data
        assert float(a["dpre"][0, 0]) == 0.0 and float(a["dpre"][0, 1]) == 0.0
        if want_bias:
            rep.check(kind, "db", a["db"], rdb, sumabs, k)
            w = ops.relu_bwd(dx, y)
            assert torch.equal(w[0], a["dpre"]) and torch.equal(w[1], a["db"])
    if want_bias:
        rep.flush()


# ---- vqf_relu_bwd_rank1_f32 ---------------------------------------------------------------------------------------------------------
RANK1_CASES = [
    # id, M, C, L, wts, dbias, in place
    ("C 8 nb 1 dbias written directly", 13, 8, 5, True, True, False),
    ("C 8 nb 3 dbias through ws no second row hasB false", 40, 8, 7, True, True, False),
    ("C 1000 dead threads odd last block in place", 299, 1000, 196, True, True, True),
    ("C 1100 narrow last tile", 50, 1100, 7, True, True, False),
    ("C 2052 three tiles last one column group no wts", 20, 2052, 3, False, True, False),
    ("C 1000 no dbias in place", 37, 1000, 6, True, False, True),
]


@pytest.mark.parametrize("case,M,C,L,with_wts,want_bias,inplace", RANK1_CASES, ids=[c[0] for c in RANK1_CASES])
def test_relu_bwd_rank1(ops, case, M, C, L, with_wts, want_bias, inplace):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    rpb, tiles = cs_rows_vec(M, C), col_tiles(C)
    nb = _cdiv(M, rpb)
    assert rpb % L != 0                                  # m / L changes inside a workgroup and not at its boundary
    if "nb 1" in case:
        assert nb == 1
    if "nb 3" in case:
        assert nb == 3 and tiles == [(2, 2, 128)] and rpb < 128                  # one row per slot: every trip without a second row
    if "dead threads" in case:
        assert tiles == [(250, 256, 1)] and (M % rpb) % 2 == 1 and nb > 1        # the last trip of the last block has no second row
    if "narrow last tile" in case:
        assert tiles == [(256, 256, 1), (19, 32, 8)] and nb > 1
    if "three tiles" in case:
        assert tiles == [(256, 256, 1), (256, 256, 1), (1, 1, 256)] and nb > 1
    k = k_rank1_dbias(M, C)
    rep = _Report("relu_bwd_rank1", "(%d, %d) L %d nb %d k %d%s" % (M, C, L, nb, k, " in place" if inplace else ""))
    for kind in KINDS:
        scale = 2.0 if kind == "exact" else float(torch.tensor(1.0 / 0.7).float())
        dx64 = _data(kind, (M, C), 401)
        y64 = torch.relu(_data(kind, (M, C), 402)) * scale                           # exact zeros: dropped or below the kink
        y64[0, 0] = -0.0
        w64, dp64 = (_data(kind, (M,), 403), _data(kind, (_cdiv(M, L), C), 404)) if with_wts else (None, None)
        dx, y, w, dp = _cu(dx64), _cu(y64), _cu(w64), _cu(dp64)

        def run():
            dpre, db, ws = _Out(M, C), _Out(C), _Ws(lib.vqf_colsum_ws_bytes(M, C))
            src = dx
            if inplace:
                dpre.view.copy_(dx)
                src = dpre.view
            assert lib.vqf_relu_bwd_rank1_f32(p(src), p(y), p(w), p(dp), L, scale, M, C, p(dpre.view), p(db.view) if want_bias else None,
                                              p(ws.buf), ws.nbytes, st) == 0
            res = dict(dpre=dpre.take())
            if want_bias:
                res["db"] = db.take()
            else:
                assert db.untouched()
            assert ws.ok()
            return res

        a, counts = _launches(ops, run)
        assert counts.get("relu_bwd") == 1 and counts.get("group_reduce", 0) == (1 if want_bias and nb > 1 else 0), counts
        assert _same(a, run())
        rpre, mag, rdb, sumabs = RR.relu_bwd_rank1(dx64, y64, w64, dp64, L, scale)
        rep.check(kind, "dpre", a["dpre"], rpre, mag, 2)        # w * dp, + dX, * scale: reduce.hip:165-172
        if want_bias:
            rep.check(kind, "db", a["db"], rdb, sumabs, k)
        if not inplace:
            wr = ops.relu_bwd_rank1(dx, y, w, dp, L, scale, want_bias=want_bias)
            assert torch.equal(wr[0], a["dpre"]) and (not want_bias or torch.equal(wr[1], a["db"]))
    rep.flush()


# ---- vqf_scale_rows / vqf_rowdot ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 4, 252, 256, 260, 1000])
def test_scale_rows_and_rowdot(ops, W):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    M = 7                                                # not a multiple of the four rows of a workgroup
    variants = [(3, 0), (1, 0)] + ([(3, 1)] if W % 4 == 0 else [])      # (L, base offset): L = 3 does not divide M; inv has ceil(M / L) entries
    rep = _Report("scale_rows/rowdot", "(%d, %d)" % (M, W))
    for L, off in variants:
        vec = W % 4 == 0 and off == 0                    # reduce.hip:219, :238: scalar through W % 4 or through the base pointer
        tag = "L%d_%s" % (L, "vec" if vec else "scalar_offset" if W % 4 == 0 else "scalar")
        for kind in KINDS:
            R64, D64 = _data(kind, (M, W), 501 + L), _data(kind, (M, W), 502 + L)
            inv64 = _scales(kind, (_cdiv(M, L),), 503)
            R, D, inv = _in_buffer(R64, off=off), _in_buffer(D64, off=off), _cu(inv64)
            assert R.data_ptr() % 16 == 4 * off

            def run():
                y, yin, rd = _Out(M, W, off=4 + off), _Out(M, W, off=4 + off), _Out(M)
                assert lib.vqf_scale_rows(p(R), p(inv), M, L, W, p(y.view), st) == 0
                yin.view.copy_(R)
                assert lib.vqf_scale_rows(p(yin.view), p(inv), M, L, W, p(yin.view), st) == 0         # in place
                assert lib.vqf_rowdot(p(R), p(D), M, W, p(rd.view), st) == 0
                return dict(y=y.take(), y_inplace=yin.take(), rowdot=rd.take())

            a = run()
            assert _same(a, run()) and torch.equal(a["y"], a["y_inplace"])
            ref = RR.scale_rows(R64, inv64, L)
            rep.check(kind, tag + "_y", a["y"], ref, ref.abs(), 0)                 # one product
            rref, rabs = RR.rowdot(R64, D64)
            rep.check(kind, tag + "_rowdot", a["rowdot"], rref, rabs, k_wave_row(W, vec))
    for kind in KINDS:                                   # one scale for all rows, read on the device
        x64, s64 = _data(kind, (M, W), 510), _scales(kind, (1,), 511)
        got = ops.scale_by_device_scalar(_cu(x64), _cu(s64))
        assert torch.equal(got, ops.scale_by_device_scalar(_cu(x64), _cu(s64)))
        rep.check(kind, "device_scalar", got, x64 * s64, (x64 * s64).abs(), 0)
    rep.flush()


# ---- vqf_l2_group_norm / vqf_l2_norm_bwd_coef / _lin --------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65, 784])
def test_l2_norm_kernels(ops, L):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    N, Z = 5, 2                                          # N not a multiple of the four samples of a workgroup; sample Z is all zero
    rep = _Report("l2_group_norm/_bwd_coef", "N %d L %d" % (N, L))
    big = float(torch.tensor(1.0 / RR.EPS).float())      # 1 / max(0, 1e-12) as fp32
    for kind in KINDS:
        ssq64 = RR.ints((N, L), 601, 0, 3) if kind == "exact" else RR.rnd((N, L), 601).abs()
        ssq64[Z] = 0.0
        ssq = _cu(ssq64.view(-1))

        def run_norm():
            norm, inv = _Out(N), _Out(N)
            assert lib.vqf_l2_group_norm(p(ssq), N, L, p(norm.view), p(inv.view), st) == 0
            return dict(norm=norm.take(), inv=inv.take())

        a = run_norm()
        assert _same(a, run_norm())
        rn, ri, rabs = RR.l2_group_norm(ssq64.view(-1), N, L)
        assert float(a["norm"][Z]) == 0.0 and float(rn[Z]) == 0.0
        k = k_wave_sum(L)
        if kind == "exact":                              # the sum is exact: one rounding each for the root and the quotient, doubled
            assert float(rabs.max()) < 2 ** 24
            rep.bound("norm_exact_data", a["norm"], rn, 2.0 ** -22 * rn)
            rep.bound("inv_exact_data", a["inv"], ri, 2.0 ** -22 * ri)
        else:                                            # sum: (k + 1) u relative (positive terms), halved by the root, + u for the root, + u for the quotient
            rep.bound("norm", a["norm"], rn, ((k + 1) / 2 + 1) * RR.U * rn)
            rep.bound("inv", a["inv"], ri, ((k + 1) / 2 + 2) * RR.U * ri)
        assert abs(float(a["inv"][Z]) / 1e12 - 1) <= 2.0 ** -22

        # the coefficients: norm and inv are inputs (inv a power of two in the exact data set)
        inv64 = _scales(kind, (N,), 602).abs()
        norm64 = (1.0 / inv64).float().double()
        norm64[Z], inv64[Z] = 0.0, big
        gn, gi = _cu(norm64), _cu(inv64)
        for G in (1, 2):
            rd64, dl64, lin64 = _data(kind, (N * L,), 603), _data(kind, (N * L * G,), 604 + G), _data(kind, (N * L * G,), 606 + G)
            rd, dl, lin = _cu(rd64), _cu(dl64), _cu(lin64)

            def run_coef():
                cA, cB, lA, lB, lU = (_Out(N) for _ in range(5))
                assert lib.vqf_l2_norm_bwd_coef(p(rd), p(gn), p(gi), N, L, p(cA.view), p(cB.view), st) == 0
                assert lib.vqf_l2_norm_bwd_coef_lin(p(dl), p(lin), G, p(gn), p(gi), N, L, p(lA.view), p(lB.view), p(lU.view), st) == 0
                return dict(coefA=cA.take(), coefB=cB.take(), lin_coefA=lA.take(), lin_coefB=lB.take(), lin_unit=lU.take())

            c = run_coef()
            assert _same(c, run_coef())
            rA, rB, rBabs = RR.l2_norm_bwd_coef(rd64, norm64, inv64, N, L)
            assert torch.equal(c["coefA"], gi)                                    # a copy of inv, the clamped sample's 1e12 included
            rep.check(kind, "coefB", c["coefB"], rB, rBabs, k_wave_sum(L) + 1)   # the sum, then * inv: reduce.hip:297
            lA, lB, lU, lBabs = RR.l2_norm_bwd_coef_lin(dl64, lin64, G, norm64, inv64, N, L)
            assert bool((c["lin_coefA"] == 1).all()) and bool((c["lin_unit"] == 1).all())
            rep.check(kind, "lin_G%d_coefB" % G, c["lin_coefB"], lB, lBabs, k_wave_sum(L * G) + 2)   # inv * inv, then * the sum: reduce.hip:281
            assert float(c["coefB"][Z]) == 0.0 and float(c["lin_coefB"][Z]) == 0.0
    rep.flush()


# ---- vqf_att_logits_fwd / _fwd_lin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hh", [1, 3, 4, 30, 256, 260, 1028])
def test_att_logits_fwd(ops, Hh):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    M = 7                                                # not a multiple of the four rows of a workgroup
    rep = _Report("att_logits_fwd/_fwd_lin", "(%d, %d)" % (M, Hh))
    for G in (1, 2, 3):
        for off in ((0, 1) if Hh % 4 == 0 else (0,)):    # off 1: hid (and, in a second _lin call, b1 alone) one float off 16 bytes
            for kind in KINDS:
                b1_64, w64, b2_64 = _data(kind, (Hh,), 701, 0.5), _data(kind, (G, Hh), 702), _data(kind, (G,), 703)
                hid64 = torch.relu(_data(kind, (M, Hh), 704) + b1_64).float().double()
                hid64[0, 0] = 0.0
                w2, b2 = _cu(w64), _cu(b2_64)
                hid = _in_buffer(hid64, off=off)
                vec = Hh % 4 == 0 and off == 0           # attention.hip:47
                tag = "G%d_%s" % (G, "vec" if vec else "scalar_offset" if Hh % 4 == 0 else "scalar")
                k = k_wave_row(Hh, vec) + 1              # + b2: attention.hip:76

                def run():
                    lg = _Out(M, G)
                    assert lib.vqf_att_logits_fwd(p(hid), p(w2), p(b2), M, Hh, G, p(lg.view), st) == 0
                    res = dict(logits=lg.take())
                    if G <= 2:
                        for name, h, b1 in (("", hid, _in_buffer(b1_64)), ("_b1_offset", _in_buffer(hid64), _in_buffer(b1_64, off=off))):
                            lg, lin = _Out(M, G), _Out(M, G)
                            assert lib.vqf_att_logits_fwd_lin(p(h), p(w2), p(b2), p(b1), M, Hh, G, p(lg.view), p(lin.view), st) == 0
                            res["lin_logits" + name], res["lin" + name] = lg.take(), lin.take()
                    return res

                a = run()
                assert _same(a, run())
                ref, sumabs = RR.att_logits_fwd(hid64, w64, b2_64)
                rep.check(kind, tag + "_logits", a["logits"], ref, sumabs, k)
                if G <= 2:
                    assert torch.equal(a["lin_logits"], a["logits"])              # the same path, the same bits
                    lref, labs = RR.att_logits_fwd_lin(hid64, w64, b2_64, b1_64)
                    for name in ("", "_b1_offset"):      # hid - b1 is one more rounding: k + 1 (both calls reported under one name)
                        rep.check(kind, tag + "_lin", a["lin" + name], lref, labs, k + 1)
                        rep.check(kind, tag + "_logits", a["lin_logits" + name], ref, sumabs, k)
                if off == 0:
                    assert torch.equal(ops.att_logits_fwd(_cu(hid64), w2, b2), a["logits"])
    rep.flush()


# ---- vqf_att_logits_bwd / _rowscale / _rowscale_obf16 -------------------------------------------------------------------------------
ATT_BWD_CASES = [
    # id, M, Hh, G, relu_mask, rows_per_scale (None: the entry point without rowscale), (hid offset, dhid_pre offset), reducer branch
    ("Hh 2 below 4 scalar M 1 G 1 relu", 1, 2, 1, 1, None, (0, 0), "group_reduce"),
    ("Hh 4 one column group M 5 G 2 relu rowscale rps 1", 5, 4, 2, 1, 1, (0, 0), "group_reduce"),
    ("Hh 30 scalar partial group M 17 G 2 no relu", 17, 30, 2, 0, None, (0, 0), "group_reduce"),
    ("Hh 1024 exactly one chunk M 17 G 1 no relu rowscale rps 3", 17, 1024, 1, 0, 3, (0, 0), "group_reduce"),
    ("Hh 1028 second chunk full group M 37 G 2 relu rowscale rps 3", 37, 1028, 2, 1, 3, (0, 0), "group_reduce"),
    ("Hh 1030 second chunk partial group scalar M 5 G 3 no relu", 5, 1030, 3, 0, None, (0, 0), "group_reduce"),
    ("Hh 2052 third chunk M 17 G 3 no relu", 17, 2052, 3, 0, None, (0, 0), "group_reduce"),
    ("Hh 8 misaligned hid scalar M 17 G 2 relu rowscale rps 3", 17, 8, 2, 1, 3, (1, 0), "group_reduce"),
    ("Hh 8 misaligned dhid_pre scalar M 21 G 1 relu", 21, 8, 1, 1, None, (0, 1), "group_reduce"),
    ("Hh 4 colreduce_one M 1041 short last block G 2 relu rowscale rps 196", 1041, 4, 2, 1, 196, (0, 0), "colreduce_one"),
    ("Hh 4 group_reduce_stage1 M 524289 G 1 relu", 128 * 4096 + 1, 4, 1, 1, None, (0, 0), "group_reduce_stage1"),
]


def _att_bwd_k(M, Hh, G):
    """attention.hip:125-183 and :500: a workgroup adds its lb rows one by one (s: :151, sb: :153, db2: :182), then the nb partial
    rows; an element of dhid_pre is G products added up (:151) and one scale (:164, :168)"""
    lb = att_bwd_rows_per_block(M)
    red = min(lb, M) + k_colreduce(_cdiv(M, lb))
    return dict(dhid_pre=G + 1, dw2=red, db2=red, dbias1=G + red)


def _att_bwd_run(ops, dl, hid, w2, rs, rps, M, Hh, G, relu, dpre_off=0, db1=True):
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    dpre, dw2, db2, dbias1 = _Out(M, Hh, off=4 + dpre_off), _Out(G, Hh), _Out(G), _Out(Hh)
    ws = _Ws(lib.vqf_att_logits_bwd_ws_bytes(M, Hh))
    pb1 = p(dbias1.view) if db1 else None
    if rps is None:
        rc = lib.vqf_att_logits_bwd(p(dl), p(hid), p(w2), M, Hh, G, relu, p(dpre.view), p(dw2.view), p(db2.view), pb1, p(ws.buf), ws.nbytes, st)
    else:
        rc = lib.vqf_att_logits_bwd_rowscale(p(dl), p(hid), p(w2), p(rs), rps, M, Hh, G, relu, p(dpre.view), p(dw2.view), p(db2.view),
                                             pb1, p(ws.buf), ws.nbytes, st)
    assert rc == 0
    res = dict(dhid_pre=dpre.take(), dw2=dw2.take(), db2=db2.take())
    if db1:
        res["dbias1"] = dbias1.take()
    else:
        assert dbias1.untouched()
    assert ws.ok()
    return res


def _att_bwd_inputs(kind, M, Hh, G, relu, rps, seed=800):
    dl64, w64 = _data(kind, (M, G), seed + 1), _data(kind, (G, Hh), seed + 2)
    hid64 = _data(kind, (M, Hh), seed + 3)
    if relu:
        hid64 = torch.relu(hid64)                        # exact zeros
    hid64[0, 0] = 0.0
    rs64 = None if rps is None else _scales(kind, (_cdiv(M, rps),), seed + 4)
    return dl64, hid64, w64, rs64


@pytest.mark.parametrize("case,M,Hh,G,relu,rps,offs,branch", ATT_BWD_CASES, ids=[c[0] for c in ATT_BWD_CASES])
def test_att_logits_bwd(ops, case, M, Hh, G, relu, rps, offs, branch):
    lb = att_bwd_rows_per_block(M)
    nb = _cdiv(M, lb)
    assert colreduce_branch(nb) == branch
    vec = Hh % 4 == 0 and offs == (0, 0)                 # attention.hip:111
    assert vec == ("scalar" not in case)
    chunks, tail = _cdiv(Hh, 1024), Hh % 4               # attention.hip:112-113: the c += 1024 loop, nc = min(4, Hh - c)
    assert ("third chunk" in case) == (chunks == 3) and ("second chunk" in case) == (chunks == 2)
    assert ("partial group" in case or "below 4" in case) == (tail != 0)
    if M > 1:
        assert M % lb != 0 and (M % lb) % 4 != 0         # a short last block whose last trip has fewer than four rows
    if rps is not None and rps > 1:
        assert lb % rps != 0 and rps % lb != 0           # the scale changes inside a workgroup and not at its boundary
    k = _att_bwd_k(M, Hh, G)
    rep = _Report("att_logits_bwd", "(%d, %d) G %d relu %d rps %s nb %d %s k %d" % (M, Hh, G, relu, rps, nb, branch, k["dbias1"]))
    for kind in KINDS:
        dl64, hid64, w64, rs64 = _att_bwd_inputs(kind, M, Hh, G, relu, rps)
        dl, w2, rs = _cu(dl64), _cu(w64), _cu(rs64)
        hid = _in_buffer(hid64, off=offs[0])

        def run():
            return _att_bwd_run(ops, dl, hid, w2, rs, rps, M, Hh, G, relu, offs[1])

        a, counts = _launches(ops, run)
        assert counts.get("att_logits_bwd") == 1 and counts.get("group_reduce") == REDUCER_LAUNCHES[branch], counts
        assert _same(a, run())
        ref = RR.att_logits_bwd(dl64, hid64, w64, relu, rs64, rps or 1)
        for name in ("dhid_pre", "dw2", "db2", "dbias1"):
            rep.check(kind, name, a[name], ref[name], ref[name + "_abs"], k[name])
        if rps is not None and kind == "exact":          # the stored rows are scaled, the three sums are those without a scale
            plain = _att_bwd_run(ops, dl, hid, w2, None, None, M, Hh, G, relu, offs[1])
            for name in ("dw2", "db2", "dbias1"):
                assert torch.equal(plain[name], a[name]), name
            assert not torch.equal(plain["dhid_pre"], a["dhid_pre"])
        if offs == (0, 0) and M < 100000:                # the wrapper makes the same call
            w = ops.att_logits_bwd(dl, _cu(hid64), w2, relu_mask=bool(relu), rowscale=rs, rows_per_scale=rps or 1)
            for got, name in zip(w, ("dhid_pre", "dw2", "db2", "dbias1")):
                assert torch.equal(got, a[name]), name
    rep.flush()


def test_att_logits_bwd_without_dbias1(ops):
    """dbias1 = NULL (split_reduced_row_kernel's d1, attention.hip:191): dw2, db2 and the rows are those of the call with it"""
    M, Hh, G = 21, 260, 2
    for kind in KINDS:
        dl64, hid64, w64, rs64 = _att_bwd_inputs(kind, M, Hh, G, 1, 3, seed=820)
        args = (_cu(dl64), _cu(hid64), _cu(w64), _cu(rs64), 3, M, Hh, G, 1)
        full, without = _att_bwd_run(ops, *args), _att_bwd_run(ops, *args, db1=False)
        assert _same(without, _att_bwd_run(ops, *args, db1=False))
        for name in ("dhid_pre", "dw2", "db2"):
            assert torch.equal(without[name], full[name]), name


def test_att_logits_bwd_obf16(ops):
    """the bf16 rows are the round-to-nearest-even cast of the fp32 entry point's rows; the three sums are its bits"""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    M, Hh, G, rps = 37, 1028, 2, 3
    assert _cdiv(Hh, 1024) == 2 and M % att_bwd_rows_per_block(M) % 4 != 0
    for kind in KINDS:
        dl64, hid64, w64, rs64 = _att_bwd_inputs(kind, M, Hh, G, 1, rps, seed=840)
        dl, hid, w2, rs = _cu(dl64), _cu(hid64), _cu(w64), _cu(rs64)
        f32 = _att_bwd_run(ops, dl, hid, w2, rs, rps, M, Hh, G, 1)

        def run():
            dpre, dw2, db2, db1 = _Out(M, Hh, off=8, dtype=torch.bfloat16), _Out(G, Hh), _Out(G), _Out(Hh)
            ws = _Ws(lib.vqf_att_logits_bwd_ws_bytes(M, Hh))
            assert lib.vqf_att_logits_bwd_rowscale_obf16(p(dl), p(hid), p(w2), p(rs), rps, M, Hh, G, p(dpre.view), p(dw2.view), p(db2.view),
                                                         p(db1.view), p(ws.buf), ws.nbytes, st) == 0
            res = dict(dhid_pre=dpre.take(), dw2=dw2.take(), db2=db2.take(), dbias1=db1.take())
            assert ws.ok()
            return res

        a = run()
        assert _same(a, run())
        assert a["dhid_pre"].dtype == torch.bfloat16 and torch.equal(a["dhid_pre"], f32["dhid_pre"].to(torch.bfloat16))
        for name in ("dw2", "db2", "dbias1"):
            assert torch.equal(a[name], f32[name]), name


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    """the exact VQF_E_* code of every refused call; nothing is launched: every output still holds 7.0.  The other arguments are
    valid and in bounds, so a call that got through would stay inside its buffers."""
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    zin, out, out2 = torch.zeros(1 << 16, device="cuda"), _Out(1 << 16), _Out(1 << 12)
    obf = _Out(1 << 12, off=8, dtype=torch.bfloat16)
    ws = _Ws(1 << 20)
    z, o, o2, w = p(zin), p(out.view), p(out2.view), p(ws.buf)
    odd = ops._ptr(zin[1:])                              # one float off 16 bytes
    M, N = 300, 8                                        # two row blocks
    need = lib.vqf_colsum_ws_bytes(M, N)
    assert colsum_route(M, N, N, True)[1] > 1 and need <= ws.nbytes
    calls = [
        ("colsum ldy < N", BADARG, lambda: lib.vqf_colsum_f32(z, M, N, N - 1, o, w, ws.nbytes, st)),
        ("colsum multi-block without ws", WORKSPACE, lambda: lib.vqf_colsum_f32(z, M, N, N, o, None, 0, st)),
        ("colsum multi-block ws too small", WORKSPACE, lambda: lib.vqf_colsum_f32(z, M, N, N, o, w, need - 4, st)),
        ("relu_bwd_rank1 C % 4", UNSUPPORTED, lambda: lib.vqf_relu_bwd_rank1_f32(z, z, z, z, 7, 1.0, 40, 6, o, o2, w, ws.nbytes, st)),
        ("relu_bwd_rank1 misaligned dX", ALIGN, lambda: lib.vqf_relu_bwd_rank1_f32(odd, z, z, z, 7, 1.0, 40, 8, o, o2, w, ws.nbytes, st)),
        ("relu_bwd_rank1 misaligned dpooled", ALIGN, lambda: lib.vqf_relu_bwd_rank1_f32(z, z, z, odd, 7, 1.0, 40, 8, o, o2, w, ws.nbytes, st)),
        ("relu_bwd_rank1 wts without dpooled", BADARG, lambda: lib.vqf_relu_bwd_rank1_f32(z, z, z, None, 7, 1.0, 40, 8, o, o2, w, ws.nbytes, st)),
        ("relu_bwd_rank1 nb > 1, dbias, no ws", WORKSPACE, lambda: lib.vqf_relu_bwd_rank1_f32(z, z, z, z, 7, 1.0, 40, 8, o, o2, None, 0, st)),
        ("att_logits_fwd G 0", UNSUPPORTED, lambda: lib.vqf_att_logits_fwd(z, z, z, 9, 8, 0, o, st)),
        ("att_logits_fwd G 4", UNSUPPORTED, lambda: lib.vqf_att_logits_fwd(z, z, z, 9, 8, 4, o, st)),
        ("att_logits_fwd_lin G 3", UNSUPPORTED, lambda: lib.vqf_att_logits_fwd_lin(z, z, z, z, 9, 8, 3, o, o2, st)),
        ("att_logits_bwd G 3 relu", UNSUPPORTED, lambda: lib.vqf_att_logits_bwd(z, z, z, 9, 8, 3, 1, o, o2, o2, o2, w, ws.nbytes, st)),
        ("att_logits_bwd G 3 rowscale", UNSUPPORTED,
         lambda: lib.vqf_att_logits_bwd_rowscale(z, z, z, z, 1, 9, 8, 3, 0, o, o2, o2, o2, w, ws.nbytes, st)),
        ("att_logits_bwd rows_per_scale 0", BADARG,
         lambda: lib.vqf_att_logits_bwd_rowscale(z, z, z, z, 0, 9, 8, 2, 1, o, o2, o2, o2, w, ws.nbytes, st)),
        ("att_logits_bwd ws too small", WORKSPACE,
         lambda: lib.vqf_att_logits_bwd(z, z, z, 9, 8, 2, 1, o, o2, o2, o2, w, lib.vqf_att_logits_bwd_ws_bytes(9, 8) - 1, st)),
        ("obf16 G 1", UNSUPPORTED,
         lambda: lib.vqf_att_logits_bwd_rowscale_obf16(z, z, z, z, 1, 9, 8, 1, p(obf.view), o2, o2, o2, w, ws.nbytes, st)),
        ("obf16 Hh % 4", UNSUPPORTED,
         lambda: lib.vqf_att_logits_bwd_rowscale_obf16(z, z, z, z, 1, 9, 6, 2, p(obf.view), o2, o2, o2, w, ws.nbytes, st)),
        ("obf16 destination 4 bytes off 8", ALIGN,
         lambda: lib.vqf_att_logits_bwd_rowscale_obf16(z, z, z, z, 1, 9, 8, 2, p(obf.view[2:]), o2, o2, o2, w, ws.nbytes, st)),
    ]
    assert 1 << 20 >= lib.vqf_att_logits_bwd_ws_bytes(9, 8) and 1 << 20 >= lib.vqf_colsum_ws_bytes(40, 8)
    assert _cdiv(40, cs_rows_vec(40, 8)) > 1
    for name, code, call in calls:
        assert call() == code, name
        torch.cuda.synchronize()
        assert out.untouched() and out2.untouched() and obf.untouched() and ws.ok() and bool((ws.buf == 7).all()), name

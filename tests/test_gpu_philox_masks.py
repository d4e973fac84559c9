"""Every kernel that regenerates a dropout mask in registers, run in Philox mode (keep=None) and held to tests/philox_ref.py -- the
host restatement of philox4x32_10 and of the two index rules (32-bit draw per element: call e >> 2, word e & 3; the fusion's
16-bit draw: call e >> 3, half-word e & 7, low half first) -- for EVERY element, no mismatch tolerated.

Operands make a dropped element the only possible zero (ones, or strictly positive values; tanh arguments > 0, |tanh| < 1 where
the backward multiplies by 1 - t^2), so `out != 0` IS the kernel's mask.  Where the output is one fp32 multiply of the input
(vqf_dropout_f32, vqf_dropout_bt, vqf_embed_dropout_fwd, the fusion's zdrop on ones) the values are compared bit for bit with
x * fp32(1 / (1 - p)); where it carries arithmetic, against the consumer's fp64 reference FED THE HOST MASK under the criterion
that consumer's own test uses (hie_stream_ref (value, bound) pairs; 1e-6 / 1e-5 on the flat tanh kernels; 2e-6 + gemm_tol on the
affinity; 1e-5 on Y / norm and 2e-5 on dP / dq / dbias of the fusion).  Seeds: 0, 77, 2^32 (low key word 0, high word 1) and a
62-bit one, the size host/mfb.py draws; p: 0.5 (threshold 2^31), 0.1 and 0.3 (thresholds that tell an fp32 p from a double one
and are no power of two), 0.25 / 0.1 for the fusion, 0.999 once.  Every launch runs twice and must give equal bits.

A failure names the first differing element as (call, word or half-word, window phase)."""
import functools

import numpy as np
import pytest
import torch

import hie_stream_ref as R
import mfb_regions_ref as RR
import philox_ref as PR
from golden_util import _report_parity
from hie_stream_util import _only, _views, _vqa, SENT
from node_harness import gemm_tol

pytestmark = pytest.mark.gpu

BIG_SEED = 0x1D2C3B4A5F6E7081 & ((1 << 62) - 1)
SEEDS = [pytest.param(0, id="seed0"), pytest.param(77, id="seed77"), pytest.param(1 << 32, id="seed2p32"),
         pytest.param(BIG_SEED, id="seed62bit")]
P32 = [0.5, 0.1, 0.3]
P16 = [0.1, 0.25]
seeds_and_p32 = lambda f: pytest.mark.parametrize("seed", SEEDS)(pytest.mark.parametrize("p", P32)(f))


@pytest.fixture(scope="module")
def ops():
    return _vqa().ops


# ---- operands, host masks, comparisons ----------------------------------------------------------------------------------------------
def _pos(shape, seed, lo=0.1, hi=1.0):
    """seeded fp32 values in [lo, hi] (CPU)"""
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).float()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


def _p64(p):
    return float(np.float32(p))


@functools.lru_cache(maxsize=None)
def _host(bits, n, seed, p):
    """the host mask of n elements, computed once per (rule, n, seed, p): numpy bool, read-only"""
    m = (PR.keep32 if bits == 32 else PR.keep16)(n, seed, p)
    m.setflags(write=False)
    return m


def _mask_t(bits, shape, seed, p):
    return torch.from_numpy(_host(bits, int(np.prod(shape)), seed, p).copy()).view(*shape)


def _scaled(x, keep, p):
    """x * fp32(1 / (1 - p)) where kept, +0 where dropped: the ONE fp32 multiply of the kernels, on the host"""
    v = (x.numpy() * PR.inv_keep(p)).astype(np.float32) * keep.numpy().astype(np.float32)
    return torch.from_numpy(v)


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.uint8)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _twice(fn):
    """fn() -> a tensor or a tuple of tensors / None, freshly allocated: two launches, equal bits; the first is returned"""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, (tuple, list)) else (a,), b if isinstance(b, (tuple, list)) else (b,)):
        assert (x is None and y is None) or _same_bits(x, y), "two launches gave different bits"
    return a


def _assert_mask(kept, host, what, bits=32):
    """kept: bool tensor in the LOGICAL element order (True: the kernel kept the element); host: bool tensor / array of philox_ref"""
    g = kept.detach().contiguous().cpu().numpy().reshape(-1)
    h = (host.numpy() if torch.is_tensor(host) else host).reshape(-1)
    assert g.shape == h.shape, (what, g.shape, h.shape)
    bad = np.flatnonzero(g != h)
    if bad.size:
        e = int(bad[0])
        where = "call %d word %d" % (e >> 2, e & 3) if bits == 32 else \
            "call %d half-word %d (%s half of word %d), window phase %d" % (e >> 3, e & 7, "high" if e & 1 else "low", (e & 7) >> 1, e & 4)
        raise AssertionError("%s: %d of %d elements are not the host mask; first at flat element %d = %s: kernel %s, host %s"
                             % (what, bad.size, g.size, e, where, "kept" if g[e] else "dropped", "kept" if h[e] else "dropped"))


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


class _Report:
    """worst err / bound per output of one consumer and case, printed (and logged on the GPU machine) as golden_util does"""

    def __init__(self, consumer, case):
        self.label, self.items = "philox_masks %-22s %s" % (consumer, case), {}

    def _note(self, name, ratio):
        self.items[name] = max(self.items.get(name, 0.0), ratio)

    def bound(self, name, got, ref_bound):
        """|got - ref| <= bound at every element ((value, bound) pairs of tests/hie_stream_ref.py)"""
        ref, bound = ref_bound
        got = got.detach().contiguous().cpu().double().reshape(ref.shape)
        err = (got - ref).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = tuple(bad.nonzero()[0].tolist())
            raise AssertionError("%s %s: %d of %d elements off; first %s: got %r ref %r bound %r"
                                 % (self.label, name, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(bound[i])))
        pos = bound > 0
        self._note(name, float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0)

    def rel(self, name, got, ref, tol):
        """max |got - ref| / max |ref| <= tol"""
        e = _rel(got, ref)
        print("%s %s: rel err %.2e (tol %.1e)" % (self.label, name, e, tol))
        assert e <= tol, (self.label, name, e, tol)
        self._note(name, e / tol)

    def flush(self):
        name = max(self.items, key=self.items.get)
        _report_parity(self.label, self.items[name], name, "  " + " ".join("%s=%.3f" % kv for kv in sorted(self.items.items())))


def _case(shape, seed, p):
    return "%s seed=%#x p=%g" % (tuple(shape), seed, p)


# ---- vqf_dropout_f32 ------------------------------------------------------------------------------------------------------------------
def _dropout_exact(ops, shape, seed, p):
    x = _pos(shape, 11)
    keep = _mask_t(32, shape, seed, p)
    y = _twice(lambda: ops.dropout(x.cuda(), seed=seed, p_drop=p))
    _assert_mask(y != 0, keep, "dropout %s" % _case(shape, seed, p))
    assert _same_bits(y.cpu(), _scaled(x, keep, p)), "dropout: a kept element is not x * fp32(1 / (1 - p))"


@seeds_and_p32
def test_dropout(ops, seed, p):
    for shape in ((4,), (300, 64)):
        _dropout_exact(ops, shape, seed, p)


@pytest.mark.parametrize("seed", SEEDS)
def test_dropout_p_0_999(ops, seed):
    """threshold 4290672384: above 2^31 (a signed compare keeps nearly everything) with low bits set"""
    _dropout_exact(ops, (300, 64), seed, 0.999)
    assert 0 < int(_host(32, 300 * 64, seed, 0.999).sum()) < 100


def test_dropout_grid_stride_second_trip(ops):
    """n = 4 (16384 x 256) + 4 x 37 elements: the launch is capped at 16384 workgroups of 256 threads, so the first 37 threads
    take a second trip of the grid-stride loop; the whole mask, the tail included, is the host's"""
    seed, p = BIG_SEED, 0.3
    per_trip = 4 * 16384 * 256
    n = per_trip + 4 * 37
    ones = torch.ones(n, device="cuda")
    y = _twice(lambda: ops.dropout(ones, seed=seed, p_drop=p))
    ik = float(PR.inv_keep(p))
    assert bool(((y == 0) | (y == ik)).all())
    kept = (y != 0).cpu()
    del y, ones
    tail = PR.keep32(4 * 37 + 4096, seed, p, first=per_trip - 4096)
    _assert_mask(kept[per_trip - 4096:], tail, "dropout: the last 4096 elements of the first trip and the second trip")
    _assert_mask(kept, _host(32, n, seed, p), "dropout n = %d" % n)


# ---- vqf_tanh_dropout_fwd / _bwd (flat): 1e-6 / 1e-5 as tests/test_gpu_hie_modules.py --------------------------------------------------
def _tanh_operands(shape):
    """a, b > 0 (tanh(a + b) in (0.15, 0.91), tanh(a) in (0.1, 0.77)); dy > 0"""
    return _pos(shape, 21), _pos(shape, 22, 0.05, 0.5), _pos(shape, 23)


def _stored_y(t64, keep, p):
    """what the forward stores for the tanh values t64: fp32(t) * fp32(1 / (1 - p)) where kept -> (y fp32, fp32(t) as fp64)"""
    t32 = t64.float()
    return _scaled(t32, keep, p), t32.double()


@seeds_and_p32
def test_tanh_dropout_flat(ops, seed, p):
    for shape in ((4,), (300, 64)):
        rep = _Report("tanh_dropout_fwd/_bwd", _case(shape, seed, p))
        a, b, dy = _tanh_operands(shape)
        keep = _mask_t(32, shape, seed, p)
        sc = keep.double() / (1.0 - _p64(p))
        for tag, bb in (("ab", b), ("a", None)):
            y = _twice(lambda: ops.tanh_dropout_fwd(a.cuda(), None if bb is None else bb.cuda(), seed=seed, p_drop=p))
            _assert_mask(y != 0, keep, "tanh_dropout_fwd(%s) %s" % (tag, _case(shape, seed, p)))
            arg = a.double() + (0 if bb is None else bb.double())
            rep.rel("fwd_" + tag, y, torch.tanh(arg) * sc, 1e-6)
        ys, t = _stored_y(torch.tanh(a.double() + b.double()), keep, p)
        dx = _twice(lambda: ops.tanh_dropout_bwd(dy.cuda(), ys.cuda(), seed=seed, p_drop=p))
        _assert_mask(dx != 0, keep, "tanh_dropout_bwd %s" % _case(shape, seed, p))
        rep.rel("bwd", dx, dy.double() * sc * (1 - t * t), 1e-5)
        rep.flush()


# ---- vqf_tanh_dropout_fwd2d / _bwd2d: the index is r * W + c of the logical (R, W), whatever the row strides ------------------------------
@seeds_and_p32
def test_tanh_dropout_2d_strided(ops, seed, p):
    for shape in ((7, 4), (5, 12), (98, 64)):
        Rr, W = shape
        rep = _Report("tanh_dropout_fwd2d/_bwd2d", _case(shape, seed, p))
        a, b, dy = _tanh_operands(shape)
        keep = _mask_t(32, shape, seed, p)
        _, (aw, bw) = _views(Rr, W, True)                     # column blocks of one wider sentinel buffer
        aw.copy_(a.cuda())
        bw.copy_(b.cuda())
        assert aw.stride(0) == 2 * W

        def fwd():
            fulls, (_, out) = _views(Rr, W, True)
            ops.tanh_dropout_fwd2d(aw, bw, None, seed, p, out=out)
            assert _only(fulls, out), "fwd2d wrote outside its destination"
            return out.contiguous()
        y = _twice(fwd)
        _assert_mask(y != 0, keep, "tanh_dropout_fwd2d %s" % _case(shape, seed, p))
        rep.bound("fwd", y, R.tanh_dropout_fwd2d(a.double(), b.double(), keep.double(), _p64(p)))
        ys, _ = _stored_y(torch.tanh(a.double() + b.double()), keep, p)
        _, (dyw, yw) = _views(Rr, W, True)
        dyw.copy_(dy.cuda())
        yw.copy_(ys.cuda())

        def bwd():
            fulls, (_, dx) = _views(Rr, W, True)
            ops.tanh_dropout_bwd2d(dyw, yw, None, seed, p, out=dx)
            assert _only(fulls, dx), "bwd2d wrote outside its destination"
            return dx.contiguous()
        dx = _twice(bwd)
        _assert_mask(dx != 0, keep, "tanh_dropout_bwd2d %s" % _case(shape, seed, p))
        rep.bound("bwd", dx, R.tanh_dropout_bwd2d(dy.double(), ys.double(), keep.double(), _p64(p)))
        rep.flush()


# ---- vqf_dropout_bt / _len: the index is (b * T + t) * H + h whatever the layouts ---------------------------------------------------------
@seeds_and_p32
def test_dropout_bt_layouts_and_lens(ops, seed, p):
    for (B, T, H), lens in (((3, 5, 8), [1, 5, 3]), ((2, 22, 64), [22, 17])):
        x = _pos((B, T, H), 31)
        keep = _mask_t(32, (B, T, H), seed, p)
        want = _scaled(x, keep, p)
        real = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[:, :, None].expand(B, T, H)
        want_len = torch.where(real, want, torch.zeros_like(want))
        for layout in ("time_major_in", "time_major_out"):
            for ln, exp in ((None, want), (lens, want_len)):
                def run():
                    if layout == "time_major_in":
                        gx, out = x.permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2), torch.full((B, T, H), 7.0, device="cuda")
                    else:
                        gx, out = x.cuda(), torch.full((T, B, H), 7.0, device="cuda").permute(1, 0, 2)
                    gl = None if ln is None else torch.tensor(ln, dtype=torch.int32).cuda()
                    ops.dropout_bt(gx, out, None, seed, p, lens=gl)
                    return out.contiguous()
                y = _twice(run)
                what = "dropout_bt %s lens=%s %s" % (layout, ln, _case((B, T, H), seed, p))
                _assert_mask(y != 0, keep & real if ln is not None else keep, what)
                assert _same_bits(y.cpu(), exp), what + ": a kept element is not x * fp32(1 / (1 - p)) / a padded row is not zero"


# ---- vqf_embed_dropout_fwd / _bwd: the flat (T, E) index; E % 4 != 0 is the element-by-element path --------------------------------------
@seeds_and_p32
def test_embed_dropout(ops, seed, p):
    for Tn, V, E in ((5, 3, 4), (77, 20, 1024), (13, 5, 7)):
        rep = _Report("embed_dropout_fwd/_bwd", _case((Tn, V, E), seed, p))
        W, dout = _pos((V, E), 41), _rand((Tn, E), 42)
        ids = torch.randint(0, V, (Tn,), generator=torch.Generator().manual_seed(43))
        keep = _mask_t(32, (Tn, E), seed, p)
        out = _twice(lambda: ops.embed_dropout_fwd(W.cuda(), ids.cuda(), None, seed, p))
        what = "embed_dropout_fwd %s" % _case((Tn, V, E), seed, p)
        _assert_mask(out != 0, keep, what)
        assert _same_bits(out.cpu(), _scaled(W[ids], keep, p)), what + ": a kept element is not W[id] * fp32(1 / (1 - p))"
        dW = _twice(lambda: ops.embed_dropout_bwd(dout.cuda(), ids.cuda(), V, None, seed, p))
        rep.bound("dW", dW, R.embed_dropout_bwd(dout.double(), ids, V, keep.double(), _p64(p)))
        # every token its own id: a row of dW is ONE token's dout * scale -- the backward's mask, element by element
        perm = torch.randperm(Tn, generator=torch.Generator().manual_seed(44))
        dpos = _pos((Tn, E), 45)
        dW1 = _twice(lambda: ops.embed_dropout_bwd(dpos.cuda(), perm.cuda(), Tn, None, seed, p))
        _assert_mask(dW1[perm.cuda()] != 0, keep, "embed_dropout_bwd %s" % _case((Tn, Tn, E), seed, p))
        assert _same_bits(dW1.cpu()[perm], _scaled(dpos, keep, p))
        rep.flush()


# ---- vqf_hie_affinity, epilogues 1 and 2: the flat (N, T, L) index; N T L % 4 != 0 is keep1's own ground ---------------------------------
@seeds_and_p32
def test_hie_affinity_epilogues(ops, seed, p):
    for N, L, E, T in ((2, 50, 64, 5), (3, 17, 32, 5)):
        assert ops.hie_affinity_supported(N, L, E, T, 2)
        if (N, L, E, T) == (3, 17, 32, 5):
            assert N * T * L % 4 != 0
        rep = _Report("hie_affinity epi 1/2", _case((N, L, E, T), seed, p))
        # positive operands scaled so that the sums stay in about (0.2, 2.5): tanh neither 0 nor 1
        widex = (_pos((N * T, 2 * E), 51) * (2.0 / E)).float().cuda()
        widey = _pos((N * L, 2 * E), 52).cuda()
        x1, x2, y1, y2 = widex[:, :E], widex[:, E:], widey[:, :E], widey[:, E:]
        d = lambda t, rows: t.double().cpu().reshape(N, rows, E)
        s1 = torch.einsum("nte,nle->ntl", d(x1, T), d(y1, L))
        s2 = s1 + torch.einsum("nte,nle->ntl", d(x2, T), d(y2, L))
        assert float(s1.min()) > 0.05 and float(s2.max()) < 4.0
        keep = _mask_t(32, (N, T, L), seed, p)
        sc = keep.double() / (1.0 - _p64(p))
        smax = float(s1.abs().max())
        f = _twice(lambda: ops.hie_affinity(x1, y1, N, L, T, epi=1, drop=(None, seed, p)))
        _assert_mask(f != 0, keep, "hie_affinity epi 1 %s" % _case((N, L, E, T), seed, p))
        rep.rel("epi1", f, torch.tanh(s1) * sc, 2e-6 + gemm_tol(E) * smax)
        b = _twice(lambda: ops.hie_affinity(x1, y1, N, L, T, x2=x2, y2=y2, epi=2, yprev=f, drop=(None, seed, p)))
        _assert_mask(b != 0, keep, "hie_affinity epi 2 %s" % _case((N, L, E, T), seed, p))
        rep.rel("epi2", b, s2 * sc * (1 - torch.tanh(s1) ** 2), 1e-5 + 2 * gemm_tol(E) * smax)
        rep.flush()


# ---- vqf_hie_hv_fwd, vqf_hie_head_bwd (keep4v): the flat (N L, E) index of `out`, whatever its row stride --------------------------------
HIE_SHAPES = [(3, 24, 4, 5, False), (3, 24, 8, 16, False), (2, 7, 128, 14, True)]      # (N, L, E, T, one chunk per sample?)


@seeds_and_p32
def test_hie_stream_hv_fwd_and_head_bwd(ops, seed, p):
    for N, L, E, T, one in HIE_SHAPES:
        assert ops.hie_stream_supported(N, L, E, T)
        S = ops.hie_chunks(N, L)
        Lc = (L + S - 1) // S
        assert (S == 1) == one, (S, "the shape no longer reaches the chunking it is there for")
        LcR = None if S == 1 else Lc
        M, MT = N * L, N * T
        rep = _Report("hie_hv_fwd/head_bwd", _case((N, L, E, T), seed, p))
        a, C, V = _pos((M, E), 61), _pos((N, T, L), 62), (_pos((MT, E), 63) * (1.0 / T)).float()
        dl, w = _pos((M,), 64), _pos((E,), 65)
        keep = _mask_t(32, (M, E), seed, p)
        d3 = lambda t, rows: t.double().view(N, rows, -1)
        _, (aw, hvw) = _views(M, E, True)                       # [a | hv] like [Cv | img_]
        aw.copy_(a.cuda())
        Cg, Vg = C.cuda(), V.cuda()
        new_part = lambda: torch.full((MT, E) if S == 1 else (S, MT, E), SENT, device="cuda")

        def fwd():
            fulls, (_, out) = _views(M, E, True)
            ops.hie_hv_fwd(aw, Cg, Vg, (None, seed, p), N, L, T, out, new_part())
            assert _only(fulls, out), "hv_fwd wrote outside its destination"
            return out.contiguous()
        out = _twice(fwd)
        _assert_mask(out != 0, keep, "hie_hv_fwd %s" % _case((N, L, E, T), seed, p))
        rep.bound("hv_fwd.out", out, R.hv_fwd(d3(a, L), C.double(), d3(V, T), d3(keep, L), _p64(p), Lc=LcR)["out"])

        # head_bwd reads the STORED Hv = tanh * keep / (1 - p); |tanh| <= 0.95 keeps 1 - t^2 away from 0
        t64 = torch.sign(_rand((M, E), 66) + 1e-3).double() * _pos((M, E), 67, 0.05, 0.95).double()
        hv, _ = _stored_y(t64, keep, p)
        hvw.copy_(hv.cuda())

        def head():
            fulls, (_, o) = _views(M, E, True)
            wpart = torch.full((S * N, E + 4), SENT, device="cuda")
            ops.hie_head_bwd(hvw, dl.cuda(), w.cuda(), Cg, (None, seed, p), N, L, T, o, new_part(), wpart)
            assert _only(fulls, o), "head_bwd wrote outside its destination"
            return o.contiguous()
        o = _twice(head)
        _assert_mask(o != 0, keep, "hie_head_bwd %s" % _case((N, L, E, T), seed, p))
        rep.bound("head_bwd.out", o, R.head_bwd(d3(hv, L), dl.double().view(N, L), w.double(), C.double(), d3(keep, L), _p64(p),
                                                Lc=LcR)["out"])
        rep.flush()


# ---- the fusion kernels: a 16-bit draw per element of the (N L, 5 O) product ------------------------------------------------------------
FUSE_SHAPES = [pytest.param(2, 3, 12, id="N2_L3_O12_rows_alternate_phase"), pytest.param(3, 20, 1000, id="N3_L20_O1000"),
               pytest.param(2, 1, 8, id="N2_L1_O8")]
_FUSE = {}


def _fuse_operands(rows, N, L, O_):
    """strictly positive P and bias, q of one sign per pooling window (a pooled sum is a sum of five terms of one sign), any dY"""
    W5 = 5 * O_
    gsign = torch.sign(_rand((N, O_), 156) + 1e-3).repeat_interleave(5, 1)
    return dict(P=_pos((rows, W5), 150), pb=_pos((W5,), 157), q=_pos((N, W5), 151) * gsign, dY=_rand((N * L, O_), 154))


def _fuse_reference(N, L, O_, seed, p, bf16=False, idx=None, U=None):
    """fp64 Y, norm, dP, dq, db of the fusion with the HOST mask; once per case.  Also checks, on the CPU, that the exact-mask
    assertions are sound: a pooled sum is zero only where all five of its elements are dropped, and the gradient of every kept
    element is non-zero (so that dP == 0 <=> dropped)."""
    key = (N, L, O_, seed, p, bf16, None if idx is None else tuple(idx))
    if key in _FUSE:
        return _FUSE[key]
    W5 = 5 * O_
    c = _fuse_operands((U if U is not None else N) * L, N, L, O_)
    keep = _mask_t(16, (N * L, W5), seed, p)
    Pv = c["P"].to(torch.bfloat16).float() if bf16 else c["P"]
    P, pb, q = (t.double().clone().requires_grad_() for t in (Pv, c["pb"], c["q"]))
    it = None if idx is None else torch.tensor(idx)
    Rr, Y, norm, _ = RR.fuse_ref(P, pb, q, torch.full((N,), L), N, L, O_, keep=keep, p=_p64(p), idx=it, U=U)
    (Y * c["dY"].double()).sum().backward()
    all_dropped = ~keep.view(N * L, O_, 5).any(2)
    assert torch.equal(Rr.detach() == 0, all_dropped), "a pooled sum is zero although one of its elements is kept"
    assert all(bool(torch.isfinite(g).all()) for g in (P.grad, q.grad, pb.grad))
    kept_any = keep.view(N, L, W5)
    if idx is not None:
        kept_any = torch.zeros((U, L, W5), dtype=torch.bool)
        for n, u in enumerate(idx):
            kept_any[u] |= keep.view(N, L, W5)[n]
    assert torch.equal(P.grad.view(-1, L, W5) != 0, kept_any), "the fp64 gradient of a kept element is zero"
    c.update(keep=keep, kept_any=kept_any.reshape(-1, W5), Y=Y.detach(), norm=norm.detach(), dP=P.grad, dq=q.grad, db=pb.grad)
    _FUSE[key] = c
    return c


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", P16)
@pytest.mark.parametrize("N,L,O_", FUSE_SHAPES)
def test_mfb_fuse_fwd_bwd(ops, N, L, O_, seed, p):
    W5 = 5 * O_
    if O_ == 12:
        assert W5 % 8 == 4                                    # consecutive rows start in alternate window phases
    c = _fuse_reference(N, L, O_, seed, p)
    case = _case((N, L, O_), seed, p)
    g = {k: c[k].cuda() for k in ("P", "pb", "q", "dY")}
    ones_p, ones_q = torch.ones((N * L, W5), device="cuda"), torch.ones((N, W5), device="cuda")
    first = None
    for coal in (0, 1, None):                                 # direct loads / LDS-transposed with prefetch / the default
        rep = _Report("mfb_fuse_fwd/_bwd", "%s fuse_coal=%s" % (case, coal))
        with ops.options(fuse_coal=coal):
            z1 = _twice(lambda: ops.mfb_fuse_fwd(ones_p, ones_q, N, L, O_, seed=seed, p_drop=p, want_zdrop=True)[3])
            Y, norm, inv, z = _twice(lambda: ops.mfb_fuse_fwd(g["P"], g["q"], N, L, O_, seed=seed, p_drop=p, pbias=g["pb"],
                                                             want_zdrop=True))
            dP, dq, _, db = _twice(lambda: ops.mfb_fuse_bwd(g["dY"], Y, norm, inv, g["P"], g["q"], N, L, O_, seed=seed, p_drop=p,
                                                           want_dbias=True, pbias=g["pb"]))
        _assert_mask(z1 != 0, c["keep"], "mfb_fuse_fwd zdrop on ones %s coal=%s" % (case, coal), bits=16)
        assert _same_bits(z1.cpu(), _scaled(torch.ones(N * L, W5), c["keep"], p)), "zdrop on ones is not fp32(1 / (1 - p)) where kept"
        _assert_mask(z != 0, c["keep"], "mfb_fuse_fwd zdrop %s coal=%s" % (case, coal), bits=16)
        rep.rel("Y", Y, c["Y"], 1e-5)
        rep.rel("norm", norm, c["norm"], 1e-5)
        assert bool((dP[~c["keep"].cuda()] == 0).all()), "dP is not zero at an element the host mask drops"
        _assert_mask(dP != 0, c["keep"], "mfb_fuse_bwd dP %s coal=%s" % (case, coal), bits=16)
        rep.rel("dP", dP, c["dP"], 2e-5)
        rep.rel("dq", dq, c["dq"], 2e-5)
        rep.rel("dbias", db, c["db"], 2e-5)
        rep.flush()
        res = (z1, z, Y, dP, dq, db)
        if first is None:
            first = res
        else:
            assert all(_same_bits(x, y) for x, y in zip(first, res)), "the access form changes a bit (fuse_coal=%s)" % coal


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", P16)
def test_mfb_fuse_bf16_projection(ops, seed, p):
    """bf16 P and bf16 dP (the bf16 mode of the image fusion).  The reference takes the bf16-rounded P.  dq / dbias are fp32
    outputs: 2e-5.  dP is ROUNDED to bf16 on store: a round-to-nearest bf16 is within 2^-9 of the value, so each element must
    lie within 2^-8 |ref| (twice that) + the 2e-5 max|ref| the fp32 arithmetic in front of the rounding is allowed."""
    N, L, O_ = 3, 20, 1000
    c = _fuse_reference(N, L, O_, seed, p, bf16=True)
    case = _case((N, L, O_), seed, p)
    g = {k: c[k].cuda() for k in ("pb", "q", "dY")}
    Pb = c["P"].to(torch.bfloat16).cuda()
    first = None
    for coal in (0, 1, None):
        rep = _Report("mfb_fuse bf16 P / dP", "%s fuse_coal=%s" % (case, coal))
        with ops.options(fuse_coal=coal):
            Y, norm, inv, _ = _twice(lambda: ops.mfb_fuse_fwd(Pb, g["q"], N, L, O_, seed=seed, p_drop=p, pbias=g["pb"]))
            dP, dq, _, db = _twice(lambda: ops.mfb_fuse_bwd(g["dY"], Y, norm, inv, Pb, g["q"], N, L, O_, seed=seed, p_drop=p,
                                                           want_dbias=True, pbias=g["pb"], dp_bf16=True))
        assert dP.dtype == torch.bfloat16
        rep.rel("Y", Y, c["Y"], 1e-5)
        rep.rel("norm", norm, c["norm"], 1e-5)
        assert bool((dP[~c["keep"].cuda()] == 0).all()), "dP is not zero at an element the host mask drops"
        _assert_mask(dP != 0, c["keep"], "mfb_fuse_bwd bf16 dP %s coal=%s" % (case, coal), bits=16)
        ref = c["dP"]
        rep.bound("dP", dP.float(), (ref, ref.abs() * 2.0 ** -8 + 2e-5 * float(ref.abs().max())))
        rep.rel("dq", dq, c["dq"], 2e-5)
        rep.rel("dbias", db, c["db"], 2e-5)
        rep.flush()
        res = (Y, dP, dq, db)
        if first is None:
            first = res
        else:
            assert all(_same_bits(x, y) for x, y in zip(first, res)), "the access form changes a bit (fuse_coal=%s)" % coal


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", P16)
def test_mfb_fuse_grouped(ops, seed, p):
    """N questions over U shared images: the mask index is the QUESTION row n L + l.  The image-owned backward sums dz q over an
    image's questions, each under its own host mask: dP is zero exactly where every question of the image drops the element."""
    import importlib
    grouping = importlib.import_module(_vqa().__name__ + ".host.grouping")
    U, N, L, O_, index = 2, 5, 4, 8, [1, 0, 0, 1, 0]
    c = _fuse_reference(N, L, O_, seed, p, idx=index, U=U)
    case = _case((U, N, L, O_), seed, p)
    rep = _Report("mfb_fuse_*_grouped", case)
    g = {k: c[k].cuda() for k in ("P", "pb", "q", "dY")}
    i32, order, off = grouping._group_index(torch.tensor(index).cuda(), U)
    assert ops.mfb_fuse_grouped_supported(N, U, L, O_)
    Y, norm, inv = _twice(lambda: ops.mfb_fuse_fwd_grouped(g["P"], g["q"], i32, N, U, L, O_, seed=seed, p_drop=p, pbias=g["pb"]))
    rep.rel("Y", Y, c["Y"], 1e-5)
    rep.rel("norm", norm, c["norm"], 1e-5)
    # the forward's mask itself: on ones R^2 of an output is (number of kept elements of its window) * fp32(1 / (1 - p))
    ones_p, ones_q = torch.ones((U * L, 5 * O_), device="cuda"), torch.ones((N, 5 * O_), device="cuda")
    R1 = _twice(lambda: ops.mfb_fuse_fwd_grouped(ones_p, ones_q, i32, N, U, L, O_, seed=seed, p_drop=p, normalise=False)[0])
    count = torch.round(R1.double().cpu() ** 2 / float(PR.inv_keep(p)))
    assert torch.equal(count, c["keep"].view(N * L, O_, 5).sum(2).double()), "grouped forward: kept elements per pooling window"
    dP, dq, db = _twice(lambda: ops.mfb_fuse_bwd_grouped(g["dY"], Y, norm, inv, g["P"], g["q"], i32, order, off, N, U, L, O_, seed=seed,
                                                         p_drop=p, want_dbias=True, pbias=g["pb"]))
    assert bool((dP[~c["kept_any"].cuda()] == 0).all()), "dP is not zero where every question of the image drops the element"
    _assert_mask(dP != 0, c["kept_any"], "mfb_fuse_bwd_grouped dP %s" % case, bits=16)
    rep.rel("dP", dP, c["dP"], 2e-5)
    rep.rel("dq", dq, c["dq"], 2e-5)
    rep.rel("dbias", db, c["db"], 2e-5)
    rep.flush()


# ---- the saturation contract of vqf_tanh_fast (csrc/common.h), through vqf_tanh_dropout_fwd at p = 0 -----------------------------------------
def test_tanh_fast_saturates_without_nan(ops):
    """"e -> 0 gives -1, a huge e is cut off at +1 before inf * 0": exactly +-1 at +-inf, NaN only at NaN, and everywhere else
    within the bound tests/hie_stream_ref.py attaches to this kernel (2e-7 absolute + the roundings of argument and value)"""
    mags = [0.0, 1e-8, 1e-4, 0.5, 8.3, 8.4, 20.0, 44.0, 88.0, float("inf")]
    vals = [s * m for m in mags for s in (1.0, -1.0)] + [float("nan"), 0.25, 0.25, 0.25]       # 24 elements: whole groups of four
    x = torch.tensor(vals, dtype=torch.float32)
    y = _twice(lambda: ops.tanh_dropout_fwd(x.cuda(), None, None, 0, 0.0)).cpu()
    fin = torch.isfinite(x)
    rep = _Report("vqf_tanh_fast", "saturation vector")
    rep.bound("tanh", y[fin], tuple(t[fin] for t in R.tanh_dropout_fwd2d(x.double(), None)))
    rep.flush()
    inf = torch.isinf(x)
    assert torch.equal(y[inf], torch.sign(x[inf])), "tanh(+-inf) must be exactly +-1"
    assert bool(torch.isnan(y[torch.isnan(x)]).all()) and int(torch.isnan(y).sum()) == 1, "NaN at NaN and nowhere else"
    assert bool((y[fin].abs() <= 1.0).all())


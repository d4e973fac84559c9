"""vqf_lstm_seq_fwd / vqf_lstm_seq_bwd (csrc/lstm.hip) and vqf_lstm_cell_fwd / _bwd (csrc/lstm_cell.hip) on their own, per step and
per ELEMENT against the fp64 references of tests/lstm_seq_ref.py (bounds derived there; tests/test_lstm_seq_ref_cpu.py shows that
honest fp32 arithmetic sits at a few 1e-3 of them and a single misrouted operand far outside).

Matrix: H in {256, 512, 768, 1024} (every template instance) x B in {1, 16, 17, 32} (both batch halves; the owner-thread boundary
at exactly one wave and at one wave plus four threads) x {fp32, bf16}, plus B = 31 at H = 1024; S = 5, the smallest length at
which each of the two fragment buffers is rewritten and then read again.  One data set per H, generated at B = 32 from a seeded CPU
generator (xw +-1.5, W_hh +-1.25 / sqrt(H) so that the recurrent term weighs as much as xw at every width, dhs +-1; W_hh is not
pre-rounded in bf16 mode): a smaller B takes its first rows, so that runs at different B can be compared bit for bit.

Forward: teacher-forced -- step s of the reference starts from the KERNEL'S stored hs[s-1], cs[s-1].  Backward: independent of the
forward kernel -- gates and cs come from the fp64 reference rounded to fp32; step s takes the kernel's stored dgates[s+1] and the
fp64 cell-gradient carry with its bound.  Every element of every stored output must be within its bound; bf16 mode under the SAME
fp32-accumulation bounds (the reference rounds the same operands).  References run in fp64 on the GPU.
Bitwise: rows do not mix and the k order does not depend on B (row independence), the workspace is fully rewritten before it is
read (0xFF-filled, or left over from another B), two runs give the same bits.  Whole-sequence drift: one free-running (48, 17, 1024)
case per mode against the free-running reference, norm-relative, under node_harness's figures for this recursion.
Guards and refusals go through the C entry points; only refusals that return before any launch are exercised."""
import ctypes
import functools

import pytest
import torch

import lstm_seq_ref as LR
from node_harness import BENIGN_TOL_BF16, LSTM_SEQ_TOL_F32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 5
CASES = [(H, B) for H in (256, 512, 768, 1024) for B in (1, 16, 17, 32)] + [(1024, 31)]
MODES = [pytest.param(False, id="fp32"), pytest.param(True, id="bf16")]
E_BADARG, E_ALIGN, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


def _mode(bf16):
    return "bf16" if bf16 else "fp32"


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ratio(got, val, bnd):
    err = (got.double() - val).abs()
    return torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


class _Worst:
    """the worst err / bound of a case with the output and step it belongs to; every element is asserted as it comes"""

    def __init__(self, entry, mode, shape):
        self.label = "lstm_seq %s %s (%s)" % (entry, mode, ",".join(str(v) for v in shape))
        self.worst, self.where = 0.0, "-"
        self.worst_prod, self.where_prod = None, "-"

    def check(self, name, step, got, ref, product=False):
        """product: the step holds a recurrent product (the first forward and the last backward step have none: there the
        activations' accuracy alone sets the ratio)"""
        val, bnd = ref
        ratio = _ratio(got, val, bnd)
        w = float(ratio.max())
        where = "%s, step %d" % (name, step)
        assert w <= 1.0, (self.label, where, w, "element %d" % int(ratio.argmax()), "%d elements outside" % int((ratio > 1).sum()))
        if w >= self.worst:
            self.worst, self.where = w, where
        if product and (self.worst_prod is None or w >= self.worst_prod):
            self.worst_prod, self.where_prod = w, where

    def report(self):
        line = "%s worst err/bound %.3f (%s)" % (self.label, self.worst, self.where)
        if self.worst_prod is not None:
            line += "; over the steps with a product %.4f (%s)" % (self.worst_prod, self.where_prod)
        print(line)


@functools.lru_cache(maxsize=None)
def _data(H, S_=S, Bmax=32):
    g = torch.Generator().manual_seed(7000 + H + S_)
    r = lambda *s: torch.rand(s, generator=g) * 2 - 1
    xw, w, dhs = r(S_, Bmax, 4 * H) * 1.5, r(4 * H, H) * (1.25 / H ** 0.5), r(S_, Bmax, H)
    return xw.to(DEV), w.to(DEV), dhs.to(DEV)


def _rows(t, B):
    return t[:, :B].contiguous()


@functools.lru_cache(maxsize=None)
def _ref_states(H, bf16):
    """the backward's stored operands: gates and cs of the fp64 free-running forward at B = 32, rounded to fp32"""
    xw, w, _ = _data(H)
    _, cs, gates = LR.seq_fwd(xw.double(), w.double(), bf16)
    return gates.float(), cs.float()


@functools.lru_cache(maxsize=None)
def _fwd(H, B, bf16):
    import vqa_amd
    xw, w, _ = _data(H)
    return vqa_amd.ops.lstm_seq_fwd(_rows(xw, B), w, bf16=bf16)


@functools.lru_cache(maxsize=None)
def _bwd(H, B, bf16):
    import vqa_amd
    _, w, dhs = _data(H)
    gates, cs = _ref_states(H, bf16)
    return vqa_amd.ops.lstm_seq_bwd(_rows(dhs, B), _rows(gates, B), _rows(cs, B), w, bf16=bf16)


def _check_fwd(tag, xw, w, hs, cs, gates, bf16):
    w64 = w.double()
    for s in range(xw.shape[0]):
        ref = LR.step_fwd(xw[s].double(), w64, hs[s - 1].double() if s else None, cs[s - 1].double() if s else None, bf16)
        tag.check("gates", s, gates[s], ref["gates"], s > 0)
        tag.check("cs", s, cs[s], ref["c"], s > 0)
        tag.check("hs", s, hs[s], ref["h"], s > 0)


def _check_bwd(tag, dhs, gates, cs, w, dg, bf16):
    w64 = w.double()
    dc = dcb = None
    for s in range(dhs.shape[0] - 1, -1, -1):
        last = s == dhs.shape[0] - 1
        ref = LR.step_bwd(dhs[s].double(), None if last else dg[s + 1].double(), w64, gates[s].double(), cs[s].double(),
                          cs[s - 1].double() if s else None, dc, dcb, bf16)
        tag.check("dgates", s, dg[s], ref["dG"], not last)
        dc, dcb = ref["dc_out"], ref["dc_out_bound"]
    return dc, dcb


# ---- 1. every step, every element ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("H,B", CASES)
def test_forward_steps_teacher_forced(vqa, H, B, bf16):
    xw, w, _ = _data(H)
    xw = _rows(xw, B)
    hs, cs, gates = _fwd(H, B, bf16)
    tag = _Worst("fwd", _mode(bf16), (S, B, H))
    _check_fwd(tag, xw, w, hs, cs, gates, bf16)
    tag.report()
    if bf16:
        hs0, cs0, g0 = _fwd(H, B, False)
        # step 0 has no recurrent product: the fp32 kernel's bits; overall the bf16 kernel really ran
        assert _same_bits(hs[0], hs0[0]) and _same_bits(cs[0], cs0[0]) and _same_bits(gates[0], g0[0])
        assert not torch.equal(hs, hs0)


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("H,B", CASES)
def test_backward_steps_from_reference_states(vqa, H, B, bf16):
    _, w, dhs = _data(H)
    gates, cs = _ref_states(H, bf16)
    dhs, gates, cs = _rows(dhs, B), _rows(gates, B), _rows(cs, B)
    dg = _bwd(H, B, bf16)
    tag = _Worst("bwd", _mode(bf16), (S, B, H))
    _check_bwd(tag, dhs, gates, cs, w, dg, bf16)
    tag.report()
    if bf16:
        d0 = vqa.ops.lstm_seq_bwd(dhs, gates, cs, w)         # the fp32 kernel on the same stored operands
        assert _same_bits(dg[-1], d0[-1]) and not torch.equal(dg, d0)


# ---- 2. bitwise properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("H", [256, 1024])
def test_rows_are_independent_of_the_batch(vqa, H, bf16):
    big = _fwd(H, 32, bf16) + (_bwd(H, 32, bf16),)
    for B in (17, 1):
        small = _fwd(H, B, bf16) + (_bwd(H, B, bf16),)
        for name, a, b in zip(("hs", "cs", "gates", "dgates"), big, small):
            assert _same_bits(_rows(a, B), b), (name, "rows 0..%d of the B = 32 run are not the B = %d run" % (B - 1, B))


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("H", [256, 1024])
def test_workspace_content_and_run_order_do_not_matter(vqa, H, bf16):
    ops = vqa.ops
    xw, w, dhs = _data(H)
    gates, cs = _ref_states(H, bf16)
    nbytes = int(vqa.lib.load().vqf_lstm_seq_ws_bytes(32, H))
    ws = ops.workspace(torch.device(DEV), nbytes)

    def fwd(B):
        return list(ops.lstm_seq_fwd(_rows(xw, B), w, bf16=bf16))

    def bwd(B):
        return [ops.lstm_seq_bwd(_rows(dhs, B), _rows(gates, B), _rows(cs, B), w, bf16=bf16)]

    def run(before):
        """forward, then backward, at B = 3, each right after before()"""
        outs = []
        for call in (fwd, bwd):
            before(call)
            assert ops.workspace(torch.device(DEV), nbytes) is ws      # the buffer the call below gets
            outs += call(3)
        return outs

    base = run(lambda call: ws.zero_())
    junk = run(lambda call: ws.fill_(0xFF))                            # NaN bit patterns in fp32 and in bf16
    after = run(lambda call: call(32))                                 # rows 3..31 of both fragment images hold the B = 32 run's
    again = run(lambda call: None)
    for name, a, b, c, d in zip(("hs", "cs", "gates", "dgates"), base, junk, after, again):
        assert torch.isfinite(a).all(), name
        assert _same_bits(a, b), (name, "depends on what the workspace held")
        assert _same_bits(a, c), (name, "depends on the run before")
        assert _same_bits(c, d), (name, "two consecutive runs differ")


# ---- 3. whole-sequence drift --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", MODES)
def test_free_running_sequence_stays_within_the_recursion_tolerance(vqa, bf16):
    Sd, B, H = 48, 17, 1024
    xw, w, dhs = _data(H, Sd, B)
    hs, cs, gates = vqa.ops.lstm_seq_fwd(xw, w, bf16=bf16)
    dg = vqa.ops.lstm_seq_bwd(dhs, gates, cs, w, bf16=bf16)
    hs64, cs64, g64 = LR.seq_fwd(xw.double(), w.double(), bf16)
    dg64 = LR.seq_bwd(dhs.double(), g64, cs64, w.double(), bf16)
    tol = BENIGN_TOL_BF16 if bf16 else LSTM_SEQ_TOL_F32
    rel = {n: float((a.double() - b).norm() / b.norm()) for n, a, b in (("hs", hs, hs64), ("cs", cs, cs64), ("gates", gates, g64), ("dgates", dg, dg64))}
    print("lstm_seq drift %s (%d,%d,%d) norm-relative to the free-running fp64 reference: %s (tolerance %.0e)"
          % (_mode(bf16), Sd, B, H, " ".join("%s %.2e" % kv for kv in rel.items()), tol))
    for n, e in rel.items():
        assert e <= tol, (n, e, tol)


# ---- 4. guards and refusals through the C entry points -------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Guarded:
    """an interior, 16-byte-aligned slice of a buffer pre-filled with 7.0, 256 floats of margin on each side"""
    MARGIN = 256

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * self.MARGIN,), 7.0, device=DEV)
        self.t = self.buf[self.MARGIN:self.MARGIN + n]
        assert self.t.data_ptr() % 16 == 0

    def margins_intact(self):
        return bool((self.buf[:self.MARGIN] == 7.0).all() and (self.buf[self.MARGIN + self.n:] == 7.0).all())

    def fully_written(self):
        return not bool((self.t == 7.0).any())

    def untouched(self):
        return bool((self.buf == 7.0).all())


@pytest.mark.parametrize("bf16", MODES)
@pytest.mark.parametrize("B,H", [(17, 256), (32, 1024)])
def test_outputs_are_written_completely_and_nothing_beyond(vqa, B, H, bf16):
    lib = vqa.lib.load()
    xw, w, dhs = _data(H)
    xw, dhs = _rows(xw, B), _rows(dhs, B)
    gates_in, cs_in = (_rows(t, B) for t in _ref_states(H, bf16))
    nb = int(lib.vqf_lstm_seq_ws_bytes(B, H))
    ws = vqa.ops.workspace(torch.device(DEV), nb)
    hs, cs, gates = _Guarded(S * B * H), _Guarded(S * B * H), _Guarded(S * B * 4 * H)
    dg, carry = _Guarded(S * B * 4 * H), _Guarded(B * H)
    flags = 1 if bf16 else 0
    rc = lib.vqf_lstm_seq_fwd(_p(xw), _p(w), S, B, H, _p(hs.t), _p(cs.t), _p(gates.t), flags, _p(ws), nb, _stream())
    assert rc == 0
    rc = lib.vqf_lstm_seq_bwd(_p(dhs), _p(gates_in), _p(cs_in), _p(w), S, B, H, _p(dg.t), _p(carry.t), flags, _p(ws), nb, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, gd in (("hs", hs), ("cs", cs), ("gates", gates), ("dgates", dg), ("dc_carry", carry)):
        assert gd.margins_intact(), (name, "written outside its extent")
        assert gd.fully_written(), (name, "an element was left unwritten")
    # and the guarded run computed what the plain one did
    for a, b in zip((hs, cs, gates), _fwd(H, B, bf16)):
        assert _same_bits(a.t.view(b.shape), b)
    assert _same_bits(dg.t.view(S, B, 4 * H), _bwd(H, B, bf16))
    # dc_carry, the one output the backward does not store per step: what step 0 leaves, against the fp64 carry and its bound
    dc, dcb = _check_bwd(_Worst("bwd", _mode(bf16), (S, B, H)), dhs, gates_in, cs_in, w, dg.t.view(S, B, 4 * H), bf16)
    tag = _Worst("bwd_carry", _mode(bf16), (S, B, H))
    tag.check("dc_carry", 0, carry.t.view(B, H), (dc, dcb), True)
    tag.report()


def test_refusals_return_before_any_launch(vqa):
    lib = vqa.lib.load()
    B, H = 17, 256
    nB = 33                                                      # buffers sized for the largest B named below
    xw_g, dhs_g = _Guarded(S * nB * 4 * H + 4), _Guarded(S * nB * H)
    w = _data(H)[1]
    gin, cin = torch.zeros(S * nB * 4 * H, device=DEV), torch.zeros(S * nB * H, device=DEV)
    hs, cs, gates = _Guarded(S * nB * H), _Guarded(S * nB * H), _Guarded(S * nB * 4 * H)
    dg, carry = _Guarded(S * nB * 4 * H + 4), _Guarded(nB * H)
    nb = int(lib.vqf_lstm_seq_ws_bytes(B, H))
    # vqf_lstm_seq_ws_bytes is the backward's need; the forward checks its own, smaller one: packed W_hh + its two fragment images
    # (lstm.hip's header comment, hf: [half][kc][lane][4])
    nb_fwd = 4 * (4 * H * H + 2 * 2 * (H // 16) * 64 * 4)
    assert nb_fwd < nb
    assert lib.vqf_lstm_seq_ws_bytes(33, H) == 0 and lib.vqf_lstm_seq_ws_bytes(B, 128) == 0
    ws = _Guarded(nb // 4)

    def fwd(S_=S, B_=B, H_=H, xw=xw_g.t, ws_bytes=nb):
        return lib.vqf_lstm_seq_fwd(_p(xw), _p(w), S_, B_, H_, _p(hs.t), _p(cs.t), _p(gates.t), 0, _p(ws.t), ws_bytes, _stream())

    def bwd(S_=S, B_=B, H_=H, dgates=dg.t, ws_bytes=nb):
        return lib.vqf_lstm_seq_bwd(_p(dhs_g.t), _p(gin), _p(cin), _p(w), S_, B_, H_, _p(dgates), _p(carry.t), 0, _p(ws.t), ws_bytes, _stream())

    for call in (fwd, bwd):
        assert call(S_=0) == E_BADARG
        assert call(B_=33) == E_UNSUPPORTED and call(H_=128) == E_UNSUPPORTED
    assert fwd(ws_bytes=nb_fwd - 1) == E_WORKSPACE and bwd(ws_bytes=nb - 1) == E_WORKSPACE
    assert fwd(xw=xw_g.t[1:]) == E_ALIGN                          # 4 bytes off a 16-byte boundary
    assert bwd(dgates=dg.t[1:]) == E_ALIGN
    torch.cuda.synchronize()
    for name, gd in (("hs", hs), ("cs", cs), ("gates", gates), ("dgates", dg), ("dc_carry", carry), ("ws", ws)):
        assert gd.untouched(), (name, "a refused call wrote to it")


# ---- 5. the point-wise cell kernels on their own -------------------------------------------------------------------------------
CELL_SHAPES = [(1, 4), (3, 20), (7, 148), (512, 1024)]           # (7, 148): B H / 4 = 259, one block plus three threads


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_fwd_every_element(vqa, B, H):
    g = torch.Generator().manual_seed(B * 31 + H)
    r = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(DEV)
    pre, c_prev = r(B, 4 * H) * 3.0, r(B, H) * 2.0
    tag = _Worst("cell_fwd", "fp32", (1, B, H))
    for step, cp in enumerate((None, c_prev)):
        gates, c, h = pre.clone(), torch.full((B, H), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
        vqa.ops.lstm_cell_fwd(gates, cp, c, h)
        ref = LR.cell_fwd(pre.double(), None if cp is None else cp.double())
        tag.check("gates (in place)", step, gates, ref["gates"])
        tag.check("c", step, c, ref["c"])
        tag.check("h", step, h, ref["h"])
    tag.report()


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_bwd_every_element_and_the_first_step_ignores_the_carry(vqa, B, H):
    g = torch.Generator().manual_seed(B * 37 + H)
    r = lambda *s: (torch.rand(s, generator=g) * 2 - 1).to(DEV)
    c_prev, dhs, dh_carry, dc_given = r(B, H) * 2.0, r(B, H), r(B, H), r(B, H)
    fw = LR.cell_fwd((r(B, 4 * H) * 3.0).double(), c_prev.double())
    gates, c_t = fw["gates"][0].float(), fw["c"][0].float()        # stored operands, independent of the forward kernel
    tag = _Worst("cell_bwd", "fp32", (1, B, H))
    step = 0
    for cp in (None, c_prev):
        for dhc in (None, dh_carry):
            for first in (True, False):
                carry = torch.full((B, H), float("nan"), device=DEV) if first else dc_given.clone()
                dG = torch.full((B, 4 * H), float("nan"), device=DEV)
                vqa.ops.lstm_cell_bwd(dhs, dhc, gates, c_t, cp, first, carry, dG)
                ref = LR.cell_bwd(dhs.double(), None if dhc is None else dhc.double(), gates.double(), c_t.double(),
                                  None if cp is None else cp.double(), dc_given.double(), first)
                assert torch.isfinite(dG).all() and torch.isfinite(carry).all(), (cp is None, dhc is None, first)
                tag.check("dG", step, dG, ref["dG"])
                tag.check("dc_carry", step, carry, (ref["dc_out"], ref["dc_out_bound"]))
                step += 1
    tag.report()


def test_cell_kernels_refuse_a_width_that_is_no_multiple_of_four(vqa):
    lib = vqa.lib.load()
    B, H = 3, 6
    mk = lambda n: _Guarded(n)
    gates, c, h, dG, carry = mk(B * 4 * H), mk(B * H), mk(B * H), mk(B * 4 * H), mk(B * H)
    z = torch.zeros(B * 4 * H, device=DEV)
    assert lib.vqf_lstm_cell_fwd(_p(gates.t), None, B, H, _p(c.t), _p(h.t), _stream()) == E_UNSUPPORTED
    assert lib.vqf_lstm_cell_bwd(_p(z), None, _p(z), _p(z), None, 1, B, H, _p(carry.t), _p(dG.t), _stream()) == E_UNSUPPORTED
    torch.cuda.synchronize()
    for gd in (gates, c, h, dG, carry):
        assert gd.untouched()

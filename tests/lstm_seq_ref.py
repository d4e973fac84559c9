"""fp64 references, with an ELEMENT-WISE error bound per output, of ONE step of the LSTM sequence kernels (vqf_lstm_seq_fwd /
vqf_lstm_seq_bwd, csrc/lstm.hip) and of the point-wise cell kernels (vqf_lstm_cell_fwd / _bwd, csrc/lstm_cell.hip).  Plain torch,
written from the formulas of include/vqa_fusion.h and the header comment of lstm.hip, not from the kernel bodies.  Every function
takes fp64 tensors (the fp32 operands of the kernel, widened exactly) and returns {output name: (value, bound)}: a kernel passes
when |got - value| <= bound at EVERY element.

Teacher forcing.  A sequence kernel stores every step's hs, cs, gates (forward) and dgates (backward), and a step's only
non-pointwise work is one product with K = H (forward) or K = 4H (backward).  step_fwd / step_bwd therefore take the KERNEL'S OWN
previous step (h_prev, c_prev; dG_next) as exact operands: rounding does not compound along the recursion, and a stale or swapped
fragment buffer shows at the step where it happens.  The one quantity the backward does not store per step, the cell-gradient
carry, is carried by the caller in fp64 together with its bound.

Modes.  R(.) is the identity in fp32 mode and round-to-nearest-even to bf16 in bf16 mode (node_harness.bf): there W_hh and the
recurrent operand (h / dG) enter the product as bf16, exactly representable in fp32, and the accumulation stays fp32 -- the
reference rounds the same operands, so the SAME fp32-accumulation bound holds in both modes.  PyTorch gate order i, f, g, o.

The bounds (u = 2^-23: twice the fp32 unit roundoff, so that any order of summation and any split into partial sums is covered;
ACT = 2e-7: the project's absolute accuracy figure of a device exponential-based activation, hie_stream_ref.TANH_ABS):
  * pre = xw + R(h) R(W)^T, a sum of K + 1 terms in any order:     (K + 3) u (|xw| + |R h| |R W|^T), the abs-sum evaluated next to
                                                                   the sum; the first step has no product: pre = xw exactly, bound 0
  * sigmoid(pre), |sigmoid'| <= 1/4:                               bound_pre / 4 + ACT + u |value|
  * tanh(pre), |tanh'| <= 1:                                       bound_pre + ACT + u |value|
  * a product x y of bounded factors (first order):                |y| bound_x + |x| bound_y + u |x y|
  * c = f c_prev + i g (c_prev is a stored fp32 value: exact):     |c_prev| bound_f + |g| bound_i + |i| bound_g + 2 u (|f c_prev| + |i g|)
                                                                   (u per product, and the sum's rounding is relative to |c| <= the abs-sum)
  * h = o tanh(c):                                                 |tanh c| bound_o + |o| bound_tanh(c) + u |h|, bound_tanh(c) by the tanh rule
  * dh = dhs + R(dG_next) R(W), K = 4H:                            (4H + 3) u (|dhs| + |R dG| |R W|); the last step: dh = dhs exactly
  * t = tanh(c) of a stored c:                                     bound_t = ACT + u |t|
  * 1 - t^2: the square and the subtraction each round a quantity <= 1, ABSOLUTELY:   2 |t| bound_t + 2 u
    (the cancellation makes the error absolute in a quantity <= 1, as in hie_stream_ref); 1 - g^2 of a stored gate: 2 u
  * dc = dc_in + dh o (1 - t^2):                                   bound_dc_in + |o (1 - t^2)| bound_dh + |dh o| bound_(1 - t^2)
                                                                   + 2 u |dh o (1 - t^2)| + u (|dc_in| + |dh o (1 - t^2)|)
  * dG_i = dc g i (1 - i), dG_f = dc c_prev f (1 - f):             |the other factors| bound_dc + 4 u |value|  (three products, one difference)
  * dG_g = dc i (1 - g^2):                                         |i (1 - g^2)| bound_dc + 2 u |dc i| + 2 u |value|
  * dG_o = dh t o (1 - o):                                         |t o (1 - o)| bound_dh + |dh o (1 - o)| bound_t + 4 u |value|
  * dc_out = dc f:                                                 f bound_dc + u |dc_out|; f < 1, so the carried bound grows at most
                                                                   linearly in S
Shapes: xw_s, gates (B, 4H); h, c, dhs_s (B, H); w_hh (4H, H)."""
import torch

from node_harness import bf

U = 2.0 ** -23
ACT = 2e-7


def R(x, bf16):
    return bf(x) if bf16 else x


def _sigmoid(pre, pre_b):
    v = torch.sigmoid(pre)
    return v, pre_b / 4 + ACT + U * v.abs()


def _tanh(pre, pre_b):
    v = torch.tanh(pre)
    return v, pre_b + ACT + U * v.abs()


def _cell(pre, pre_b, c_prev):
    """the point-wise part of a forward step from the pre-activations (B, 4H) and their bound"""
    pi, pf, pg, po = pre.chunk(4, dim=1)
    bi, bf_, bg, bo = pre_b.chunk(4, dim=1) if torch.is_tensor(pre_b) else (pre_b,) * 4
    (i, ib), (f, fb), (g, gb), (o, ob) = _sigmoid(pi, bi), _sigmoid(pf, bf_), _tanh(pg, bg), _sigmoid(po, bo)
    ig = i * g
    if c_prev is None:
        c, cb = ig, g.abs() * ib + i.abs() * gb + U * ig.abs()
    else:
        fc = f * c_prev
        c = fc + ig
        cb = c_prev.abs() * fb + g.abs() * ib + i.abs() * gb + 2 * U * (fc.abs() + ig.abs())
    t, tb = _tanh(c, cb)
    h = o * t
    hb = t.abs() * ob + o.abs() * tb + U * h.abs()
    return {"gates": (torch.cat((i, f, g, o), 1), torch.cat((ib, fb, gb, ob), 1)), "c": (c, cb), "h": (h, hb)}


def step_fwd(xw_s, w_hh, h_prev, c_prev, bf16=False):
    """One forward step given the previous step's stored (h, c) (None at the first step) -> gates (activated), c, h"""
    H = w_hh.shape[1]
    if h_prev is None:
        pre, pre_b = xw_s, torch.zeros_like(xw_s)
    else:
        hr, wr = R(h_prev, bf16), R(w_hh, bf16)
        pre = xw_s + hr @ wr.t()
        pre_b = (H + 3) * U * (xw_s.abs() + hr.abs() @ wr.abs().t())
    return _cell(pre, pre_b, c_prev)


def _cell_bwd(dh, dhb, gates_s, c_s, c_prev, dc_in, dc_in_b):
    """the point-wise part of a backward step from dh and its bound; dc_in None: no carry yet"""
    i, f, g, o = gates_s.chunk(4, dim=1)
    t = torch.tanh(c_s)
    tb = ACT + U * t.abs()
    om = 1.0 - t * t
    omb = 2 * t.abs() * tb + 2 * U
    p = dh * o * om
    pb = (o * om).abs() * dhb + (dh * o).abs() * omb + 2 * U * p.abs()
    if dc_in is None:
        dc, dcb = p, pb
    else:
        dc = dc_in + p
        dcb = dc_in_b + pb + U * (dc_in.abs() + p.abs())
    cp = torch.zeros_like(c_s) if c_prev is None else c_prev
    d0 = dc * g * i * (1.0 - i)
    d0b = (g * i * (1.0 - i)).abs() * dcb + 4 * U * d0.abs()
    d1 = dc * cp * f * (1.0 - f)
    d1b = (cp * f * (1.0 - f)).abs() * dcb + 4 * U * d1.abs()
    og = 1.0 - g * g
    d2 = dc * i * og
    d2b = (i * og).abs() * dcb + 2 * U * (dc * i).abs() + 2 * U * d2.abs()
    d3 = dh * t * o * (1.0 - o)
    d3b = (t * o * (1.0 - o)).abs() * dhb + (dh * o * (1.0 - o)).abs() * tb + 4 * U * d3.abs()
    dc_out = dc * f
    return {"dG": (torch.cat((d0, d1, d2, d3), 1), torch.cat((d0b, d1b, d2b, d3b), 1)),
            "dc_out": dc_out, "dc_out_bound": dcb * f + U * dc_out.abs()}


def step_bwd(dhs_s, dG_next, w_hh, gates_s, c_s, c_prev, dc_in, dc_in_bound, bf16=False):
    """One backward step given the next step's stored dG (None at the last step) and the fp64 cell-gradient carry with its bound
    (None at the last step) -> dG (the four pre-activation gradients, with bound), dc_out, dc_out_bound"""
    H = w_hh.shape[1]
    if dG_next is None:
        dh, dhb = dhs_s, torch.zeros_like(dhs_s)
    else:
        gr, wr = R(dG_next, bf16), R(w_hh, bf16)
        dh = dhs_s + gr @ wr
        dhb = (4 * H + 3) * U * (dhs_s.abs() + gr.abs() @ wr.abs())
    return _cell_bwd(dh, dhb, gates_s, c_s, c_prev, dc_in, dc_in_bound)


def seq_fwd(xw, w_hh, bf16=False):
    """The free-running whole sequence: h and c are the reference's own -> hs, cs (S, B, H), gates (S, B, 4H)"""
    hs, cs, gs = [], [], []
    h = c = None
    for s in range(xw.shape[0]):
        r = step_fwd(xw[s], w_hh, h, c, bf16)
        h, c = r["h"][0], r["c"][0]
        hs.append(h), cs.append(c), gs.append(r["gates"][0])
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def seq_bwd(dhs, gates, cs, w_hh, bf16=False):
    """The free-running backward over stored gates / cs: dG and the carry are the reference's own -> dgates (S, B, 4H)"""
    S = dhs.shape[0]
    out = [None] * S
    dG = dc = dcb = None
    for s in range(S - 1, -1, -1):
        r = step_bwd(dhs[s], dG, w_hh, gates[s], cs[s], cs[s - 1] if s else None, dc, dcb, bf16)
        dG, dc, dcb = r["dG"][0], r["dc_out"], r["dc_out_bound"]
        out[s] = dG
    return torch.stack(out)


def cell_fwd(pre, c_prev):
    """vqf_lstm_cell_fwd: pre-activations (B, 4H) as given -> gates (activated), c, h"""
    return _cell(pre, torch.zeros_like(pre), c_prev)


def cell_bwd(dhs_t, dh_carry, gates, c_t, c_prev, dc_in, first):
    """vqf_lstm_cell_bwd: dh = dhs_t (+ dh_carry); first: the carry dc_in is NOT read (whatever it holds) -> dG, dc_out"""
    if dh_carry is None:
        dh, dhb = dhs_t, torch.zeros_like(dhs_t)
    else:
        dh, dhb = dhs_t + dh_carry, U * (dhs_t.abs() + dh_carry.abs())
    if first:
        return _cell_bwd(dh, dhb, gates, c_t, c_prev, None, None)
    return _cell_bwd(dh, dhb, gates, c_t, c_prev, dc_in, torch.zeros_like(dc_in))

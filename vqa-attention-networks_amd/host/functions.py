"""torch.autograd.Function per fused stage of the hot path.

Each Function's forward/backward is a short sequence of C-ABI launches on the
current HIP stream; no torch arithmetic op touches the big tensors.

  LinearFn     a4, a10      nn.Linear / 1x1 conv          (mfb.py:92,137 ...)
  AttHeadFn    a3, a7+a8    attention MLP -> 2 logits -> softmax -> glimpse sums
  ImgFuseFn    a5+a6        image projection + MFB fusion over the 196 regions
  FinalMfbFn   a9           the (N,5000) x (N,5000) MFB block(s)
"""
import torch

from . import ops


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _w2d(w):
    """(out,in,1,1) conv weight or (out,in) linear weight -> contiguous (out,in) view."""
    return _c(w.reshape(w.shape[0], -1))


def _bf16_ok(*dims):
    """bf16 GEMM entry point: every extent that becomes a K or a K-major row extent must be a multiple of 8."""
    return all(d % 8 == 0 for d in dims)


class EmbedTanhFn(torch.autograd.Function):
    """que_embedded = tanh(word_embedding(questions))   (mfb.py:68, mhb_coAtt.py:69): gather + tanh in one launch, and a
    deterministic one-launch weight gradient (csrc/embed.hip) instead of torch's sort-based embedding backward.
    lens ((N,) int32, ids (N, Tq); HieCoAttenLadder): the tokens at positions >= lens[n] are padding -- zero rows, no gradient."""

    @staticmethod
    def forward(ctx, ids, weight, tanh=True, time_major=False, lens=None):
        ids = ids.contiguous()
        out = ops.embed_tanh_fwd(_c(weight), ids, tanh, time_major, lens=lens)
        ctx.save_for_backward(ids, out if tanh else None)
        ctx.V, ctx.tm, ctx.lens = weight.shape[0], bool(time_major), lens
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, out = ctx.saved_tensors
        return None, ops.embed_tanh_bwd(_c(dout), out, ids, ctx.V, ctx.tm, lens=ctx.lens), None, None, None


def _plain_embedding(embedding, ids):
    w = embedding.weight
    return (w.is_cuda and w.dtype == torch.float32 and ids.is_cuda and ids.dtype == torch.int64 and embedding.padding_idx is None
            and embedding.max_norm is None and not embedding.sparse and not embedding.scale_grad_by_freq and w.shape[1] <= 1024)


def embed_tanh(embedding, ids, time_major=False):
    """tanh(embedding(ids)) on the HIP path when the nn.Embedding is a plain lookup (no padding_idx / max_norm / sparse grads /
    frequency scaling) with an fp32 GPU weight of width <= 1024; torch otherwise.  time_major: ids (N,Tq) -> (Tq,N,E), the layout
    the batch-major LSTM consumes (the lookup writes it directly: no transposing copy)."""
    if _plain_embedding(embedding, ids):
        return EmbedTanhFn.apply(ids, embedding.weight, True, bool(time_major) and ids.dim() == 2)
    y = torch.tanh(embedding(ids))
    return y.transpose(0, 1).contiguous() if time_major and ids.dim() == 2 else y


def embed(embedding, ids):
    """embedding(ids) (hieCoAtten.py:27, networks.py:23,56, mhb_coAtt.py:181) on the HIP path under the same conditions."""
    if _plain_embedding(embedding, ids):
        return EmbedTanhFn.apply(ids, embedding.weight, False, False)
    return embedding(ids)


class NormLink:
    """F.normalize folded into its consumer (mfb.py:105-109: fusion_normed is consumed by co_att_conv1 alone).

    The producer (ImgFuseFn / MfbFuseFn) hands on R, the signed square roots WITHOUT the per-sample 1/norm, and leaves
    inv = 1 / max(||R_n||, eps) and L here; the consumer (the co-attention AttHeadFn) applies inv in the epilogue of its
    conv GEMM (vqf_gemm_f32_rowscale), scales its stored hidden-layer gradient by it so that dW1 and the gradient it
    returns (dYs = dY / norm) need no further pass, and leaves (dlogits, lin) here, from which the producer's backward gets
    sum(Y * dY) per sample.  Saves the scale_rows pass (forward) and the rowdot pass (backward) over the (N*L, 1000)
    tensors.  One link per forward call; only valid while the producer's output has exactly this one consumer.
    Where the producer's output holds the packed rows (RegionLayout.rows) the scale is per ROW: inv is rowinv (R,) -- 1/norm of each
    row's sample, written by vqf_l2_group_norm_packed -- and L is 1; the consumer's calls do not change.
    want_xb: the consumer's request for the producer's bf16 copy of R on a REGION layout (the models' regions_bf16_coatt: the head
    behind the link runs in bf16).  On a plain tensor a bf16 P always leaves the copy; on a region layout only when asked, so that
    regions_bf16 alone keeps its launches."""
    __slots__ = ("inv", "L", "lin", "xb", "want_xb")

    def __init__(self, want_xb=False):
        self.inv, self.L, self.lin, self.xb = None, 0, None, None    # xb: the producer's bf16 copy of R (K padded to 32), bf16 modes
        self.want_xb = bool(want_xb)


class _Dense:
    """The dense layer LinearFn, FinalMfbFn and both forms of AttHeadFn share: y = x W^T (+ b)(relu) in fp32, or with bf16
    operands / fp32 accumulate (bias, ReLU and every reduction stay fp32).  bf16 needs every extent in `dims` -- those that
    become a K or a K-major row extent -- to be a multiple of 8, else the layer stays fp32 (_bf16_ok).  operand() is the cast
    (columns zero-padded to pad_to: 8, or 32 for the K of the attention head's first layer; a tensor that already is bf16 is
    taken as it is); fwd / dx / dw are the three products on operands as operand() returned them, which is what a backward
    saves, and one operand(dy) serves dx and dw.  Every step is one launch, so a node with two layers (FinalMfbFn) keeps its launch order.
    kw: the explicit extents of a site whose operands are padded (K=, N=) and out= / accumulate=."""
    __slots__ = ("bf16",)

    def __init__(self, bf16, dims=()):
        self.bf16 = bool(bf16) and _bf16_ok(*dims)

    def operand(self, t, pad_to=8, pad_rows_to=None):
        """pad_rows_to: the rows zero-padded as well (ops.cast_bf16): an operand of a weight gradient whose K is a region layout's row count"""
        return ops.cast_bf16(t, pad_to, pad_rows_to) if (self.bf16 and t.dtype != torch.bfloat16) else t

    def fwd(self, x, w, bias=None, relu=False, scale=None, **kw):
        """scale: (rowscale, rows per scale), the epilogue of the head behind a NormLink"""
        if scale is not None:
            return (ops.gemm_bf16_rowscale if self.bf16 else ops.gemm_rowscale)(x, w, *scale, bias=bias, relu=relu, **kw)
        return (ops.gemm_bf16 if self.bf16 else ops.gemm)(x, w, bias=bias, relu=relu, **kw)

    def dx(self, dy, w, **kw):
        """dX = dY W   (M,K)"""
        return (ops.gemm_bf16 if self.bf16 else ops.gemm)(dy, w, tb=True, **kw)

    def dw(self, dy, x, like):
        """dW = dY^T X   (N,K) in the parameter's shape, without the pad columns of a padded x"""
        g = (ops.gemm_bf16 if self.bf16 else ops.gemm)(dy, x, ta=True, tb=True)
        cin = like[0].numel()
        return (g if g.shape[1] == cin else g[:, :cin].contiguous()).view_as(like)


class LinearFn(torch.autograd.Function):
    """y = x @ W^T + b  (optionally relu).  x (M,K), W (N,K).
    bf16 (gemm_dtype "bf16-all"): bf16 operands / fp32 accumulate in the forward, the dgrad and the weight gradient (_Dense)."""

    @staticmethod
    def forward(ctx, x, w, b, relu=False, bf16=False):
        x, w2 = _c(x), _w2d(w)
        d = _Dense(bf16, dims=(x.shape[0], x.shape[1], w2.shape[0]))
        x, wo = d.operand(x), d.operand(w2)
        y = d.fwd(x, wo, b, relu)
        ctx.save_for_backward(x, w, y if relu else None, wo if d.bf16 else None)
        ctx.has_bias, ctx.relu, ctx.bf16 = b is not None, relu, d.bf16
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, wb = ctx.saved_tensors
        d = _Dense(ctx.bf16)
        dy = _c(dy)
        db = None
        if ctx.relu:
            dy, db = ops.relu_bwd(dy, y, want_bias=ctx.has_bias)
        elif ctx.has_bias and ctx.needs_input_grad[2]:
            db = ops.colsum(dy)
        dy = d.operand(dy)
        dx = d.dx(dy, wb if d.bf16 else _w2d(w)) if ctx.needs_input_grad[0] else None
        dw = d.dw(dy, x, w) if ctx.needs_input_grad[1] else None
        return dx, dw, db, None, None


class Linear2Fn(torch.autograd.Function):
    """y = [x1 | x2] @ W^T + b without materialising the concatenation (mhb_coAtt.py:147-148,213-214: the two final MFB blocks
    are concatenated along the feature axis and fed to the classifier).  x1 (M,K1), x2 (M,K2), W (N, K1+K2): two products into
    one output (the second accumulates), the weight's column blocks read in place as row-strided operands; the backward hands
    each block its own contiguous gradient and writes the weight gradient's column blocks in place."""

    @staticmethod
    def forward(ctx, x1, x2, w, b):
        x1, x2 = _c(x1), _c(x2)
        w2 = _w2d(w)
        K1 = x1.shape[1]
        y = ops.gemm(x1, w2[:, :K1], bias=b)
        ops.gemm(x2, w2[:, K1:], out=y, accumulate=True)
        ctx.save_for_backward(x1, x2, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, w = ctx.saved_tensors
        w2 = _w2d(w)
        dy = _c(dy)
        K1 = x1.shape[1]
        dx1 = ops.gemm(dy, w2[:, :K1], tb=True) if ctx.needs_input_grad[0] else None
        dx2 = ops.gemm(dy, w2[:, K1:], tb=True) if ctx.needs_input_grad[1] else None
        dw = None
        if ctx.needs_input_grad[2]:
            dw = torch.empty_like(w2)
            ops.gemm(dy, x1, ta=True, tb=True, out=dw[:, :K1])
            ops.gemm(dy, x2, ta=True, tb=True, out=dw[:, K1:])
            dw = dw.view_as(w)
        db = ops.colsum(dy) if (ctx.has_bias and ctx.needs_input_grad[3]) else None
        return dx1, dx2, dw, db


class JoinRowsFn(torch.autograd.Function):
    """cat((v, q), 0) where v and q already ARE the two row blocks of `buf` (their producers wrote them there): returns buf,
    hands each block its contiguous half of the gradient (hieCoAtten.py:52)."""

    @staticmethod
    def forward(ctx, v, q, buf):
        n = v.shape[0]
        if v.data_ptr() != buf.data_ptr() or q.data_ptr() != buf[n:].data_ptr() or buf.shape[0] != n + q.shape[0]:
            raise ops._l.VqfError("JoinRowsFn: v and q must be the row blocks of buf")
        ctx.n = n
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        return g[:ctx.n], g[ctx.n:], None


# ---------------------------------------------------------------------------------------------
# One dispatcher pair per kernel family that knows where the image rows are (grouping.RegionLayout: shared images, region
# counts, packed rows).  Each picks the ops.* wrapper of the layout and is the only place that does; layout None is the plain
# tensor and takes the calls it always took.  Image tensors behind a layout other than the plain one are fp32 -- but for P and dP of
# the un-grouped layouts (the models' regions_bf16): the wrappers pick the bf16 entry points by P.dtype and dp_bf16, a bf16 P / dP has
# ops.pad_rows(layout.R) rows (the weight gradient's K, zero behind the layout.R real ones).
# ---------------------------------------------------------------------------------------------
def _fuse_fwd(P, q, layout, N, L, O, link, **kw):
    """The MFB fusion over the regions (ops.mfb_fuse_fwd / _grouped / _packed / _packed_rows; kw: keep, seed, p_drop, pbias)
    -> (Y, norm, inv, rb, (scale, rows per scale)): with a link Y is R without 1/norm, rb holds the bf16 copy of R a bf16 P's kernel
    wrote beside it (on a region layout only where the link asks for it, want_xb: ops.pad_rows(rows of Y) rows, zero behind the real
    ones), and the last pair is what the link's consumer scales Y's rows by -- (inv, L), or (rowinv, 1) where Y holds the packed rows
    (layout.rows)."""
    if layout is not None and P.dtype == torch.bfloat16:                  # un-grouped (the nodes refuse bf16 with shared images)
        kw["regions_bf16"] = True
    rb = [] if (link is not None and P.dtype == torch.bfloat16 and (layout is None or (link.want_xb and not layout.grouped))) else None
    if layout is not None and layout.rows:
        Y, norm, inv, rowinv = ops.mfb_fuse_fwd_packed_rows(P, q, layout.roff, N, L, O, normalise=link is None, R=layout.R,
                                                            **(kw if rb is None else dict(kw, r_bf16=rb)))
        return Y, norm, inv, rb, (rowinv, 1)
    if layout is not None and layout.packed:
        return ops.mfb_fuse_fwd_packed(P, q, layout.roff, N, L, O, idx=layout.idx, normalise=link is None, R=layout.R,
                                       **(kw if rb is None else dict(kw, r_bf16=rb))) + (rb, None)
    if layout is not None and layout.grouped:
        return ops.mfb_fuse_fwd_grouped(P, q, layout.idx, N, layout.U, L, O, normalise=link is None,
                                        lens=(layout.lens_q, layout.lens_u) if layout.counted else None, **kw) + (None, None)
    Y, norm, inv, _ = ops.mfb_fuse_fwd(P, q, N, L, O, normalise=link is None, r_bf16=rb,
                                       lens=None if layout is None else layout.lens_q, **kw)
    return Y, norm, inv, rb, None


def _fuse_bwd(dY, Y, norm, inv, P, q, layout, N, L, O, dp_bf16=False, **kw):
    """-> (dP in P's layout -- summed per image where the images are shared --, dq, dbias); kw: keep, seed, p_drop, pbias, lin"""
    if layout is not None and dp_bf16:                                    # un-grouped (the nodes refuse bf16 with shared images)
        kw.update(regions_bf16=True, dp_bf16=True, dp_rows=ops.pad_rows(layout.R))
    if layout is not None and layout.rows:
        return ops.mfb_fuse_bwd_packed_rows(dY, Y, norm, inv, P, q, layout.roff, N, L, O, want_dbias=True, R=layout.R, **kw)
    if layout is not None and layout.packed:
        return ops.mfb_fuse_bwd_packed(dY, Y, norm, inv, P, q, layout.roff, N, L, O, grp=layout.grp, want_dbias=True, R=layout.R,
                                       **kw)
    if layout is not None and layout.grouped:
        return ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, *layout.grp, N, layout.U, L, O, want_dbias=True,
                                        lens=(layout.lens_q, layout.lens_u) if layout.counted else None, **kw)
    kw.setdefault("dp_bf16", dp_bf16)
    dP, dq, _, dbi = ops.mfb_fuse_bwd(dY, Y, norm, inv, P, q, N, L, O, want_dbias=True,
                                      lens=None if layout is None else layout.lens_q, **kw)
    return dP, dq, dbi


def _unit_sums(feat, G, layout):
    """The pooling under unit weights, per OWNER of the rows (the images, shared or not): feat (U, S, C), or (R, C) packed
    -> (wts, sums (U, G*C)) over each owner's real regions."""
    U, S = (feat.shape[0], feat.shape[1]) if layout is None else (layout.U, layout.L)
    zeros = torch.zeros((U * S, G), dtype=torch.float32, device=feat.device)          # the logits: ignored under unit weights
    if layout is not None and layout.packed:
        return ops.glimpse_pool_fwd_packed(feat, zeros, layout.roff, U, S, True)
    return ops.glimpse_pool_fwd(feat, zeros, True, lens=None if layout is None else layout.lens_u)


def _pool_fwd(feat, logits, unit, layout):
    """softmax over a sample's positions + glimpse sums (ops.glimpse_pool_fwd / _grouped / _packed) -> (wts (N, G, S), pooled (N, G*C)).
    feat (N, S, C); with shared images (U, S, C); packed (R, C).  Shared images under unit weights: the region sums of each IMAGE
    (the unit pooling on the image tensor), one row block per question; there are no weights to keep."""
    if layout is None:
        return ops.glimpse_pool_fwd(feat, logits, unit)
    if layout.grouped and unit:
        return None, ops.row_block_gather(_unit_sums(feat, logits.shape[1], layout)[1], layout.idx)
    if layout.rows:                   # logits (R, G) on the packed rows
        return ops.glimpse_pool_fwd_packed_rows(feat, logits, layout.roff, layout.N, layout.L, unit)
    if layout.packed:
        return ops.glimpse_pool_fwd_packed(feat, logits, layout.roff, layout.N, layout.L, unit, idx=layout.idx)
    if layout.grouped:
        return ops.glimpse_pool_fwd_grouped(feat, logits, layout.idx, lens=layout.lens_q)
    return ops.glimpse_pool_fwd(feat, logits, unit, lens=layout.lens_q)


def _pool_bwd(dpooled, feat, wts, unit, need_dfeat, layout, dwts=None):
    """-> (dlogits (N*S, G), dfeat in feat's layout or None): with shared images dfeat sums each image's questions."""
    if layout is None:
        return ops.glimpse_pool_bwd(dpooled, feat, wts, unit, need_dfeat, dwts=dwts)
    if layout.grouped and unit:       # d(pooled)/d(logits) == 0 under unit weights: the exact zeros the unit kernel writes
        G = dpooled.shape[1] // feat.shape[-1]
        return torch.zeros((layout.N * layout.L, G), dtype=torch.float32, device=dpooled.device), None
    if layout.rows and not need_dfeat:        # dlogits (R, G) on the packed rows
        return ops.glimpse_pool_bwd_packed_rows(dpooled, feat, wts, layout.roff, unit, dwts=dwts), None
    if layout.rows:
        raise ops._l.VqfError("the co-attention head on the packed rows pools a feature tensor that is data (no dfeat)")
    if layout.packed and need_dfeat:
        return ops.glimpse_pool_bwd_packed_dfeat(dpooled, feat, wts, layout.roff, unit, grp=layout.grp, dwts=dwts)
    if layout.packed:
        return ops.glimpse_pool_bwd_packed(dpooled, feat, wts, layout.roff, unit, idx=layout.idx, dwts=dwts), None
    if layout.grouped:
        return ops.glimpse_pool_bwd_grouped(dpooled, feat, wts, *layout.grp, need_dfeat, dwts=dwts, lens=layout.lens_q)
    return ops.glimpse_pool_bwd(dpooled, feat, wts, unit, need_dfeat, dwts=dwts, lens=layout.lens_q)


def _guided_fwd(xh, gp, w, layout, N, S):
    """The guided attention logits over the image rows (ops.guided_logits_fwd / _grouped / _packed): xh (N*S, G*E); with shared
    images (U*S, G*E); packed (R, G*E) -> logits (N*S, G)."""
    if layout.packed:
        return ops.guided_logits_fwd_packed(xh, gp, w, layout.roff, N, S, idx=layout.idx)
    if layout.grouped:
        return ops.guided_logits_fwd_grouped(xh, gp, w, layout.idx, N, layout.U, S)
    return ops.guided_logits_fwd(xh, gp, w, N, S)


def _guided_bwd(dlogits, xh, gp, w, layout, N, S):
    """-> (dxh in xh's layout -- summed per image where the images are shared --, dgp (N, G*E), dw (G, E))"""
    if layout.packed:
        return ops.guided_logits_bwd_packed(dlogits, xh, gp, w, layout.roff, N, S, grp=layout.grp)
    if layout.grouped:
        return ops.guided_logits_bwd_grouped(dlogits, xh, gp, w, layout.order, layout.grp_off, N, layout.U, S)
    return ops.guided_logits_bwd(dlogits, xh, gp, w, N, S)


class AttHeadFn(torch.autograd.Function):
    """Attention MLP + glimpse pooling.

    x    (N*S, Cin)  MLP input  (question side: the LSTM states; image side: fusion_normed)
    feat (N, S, C)   what the glimpses pool (LSTM states / the image tensor)
    w1,b1 [wm,bm] w2,b2: conv1 (+ "multilayer" conv) + conv2 -> 2 logits
    unit_softmax: reproduce mfb.py:84,118 (softmax over the singleton axis == 1)
    same_src: the CALLER's statement that x is feat.view(N*S, C) of the same autograd tensor (the question head pools the very
        tensor its MLP reads, mfb.py:73-89): the backward then adds the MLP's input gradient onto the pooling's in the GEMM
        epilogue and returns ONE gradient (for feat; None for x) instead of leaving two for autograd to add.  Never inferred
        from pointers: an alias with a different autograd history must keep its own gradient.
    layout: None (the question head; the plain image tensor), or the grouping.RegionLayout of the image head -- fp32 feat that is
        data (no gradient), never the MLP's own source; bf16 (the models' regions_bf16_coatt) only where no images are shared: the
        first layer's three products then run as on a plain tensor, but both bf16 operands of its weight gradient -- x and d1 --
        have ops.pad_rows(rows) rows, exact zeros behind the real ones (K % 32 == 0: _img_proj / _img_wgrad's rule), while the
        forward and dx keep M = the real rows.  Shared images: feat is (U, S, C), x stays (N*S, Cin) per question, and
        question n pools the rows of image idx[n] (under unit_softmax the per-image region sums, gathered).  Region counts: the
        softmax runs over the first lens_q[n] positions (unit_softmax: weight 1 there), the weights beyond are exact zeros and so
        are their dlogits, so the MLP's backward adds nothing for padded rows.  Packed rows: feat is (R, C), the real rows of every
        image, read through roff; x, the logits and the weights stay (N, L, .) padded.  Packed rows behind the fusion too
        (layout.rows): x is (R, Cin), so the hidden layers, the logits and every gradient of the MLP are (R, .) -- the products run
        with M (or K) = R --, and only the weights stay (N, G, L), exact zeros behind each count.  (_pool_fwd / _pool_bwd pick the kernels.)
    returns pooled (N, 2C); the attention weights (N,2,S) are kept on ctx.
    """

    @staticmethod
    def forward(ctx, x, feat, w1, b1, wm, bm, w2, b2, unit_softmax, bf16=False, link=None, same_src=False, layout=None):
        x = _c(x)
        feat = _c(feat)
        ctx.same_src = bool(same_src)
        ctx.layout = layout
        if layout is not None and ((bool(bf16) and layout.grouped) or ctx.same_src or feat.dtype != torch.float32
                                   or ctx.needs_input_grad[1] or feat.dim() != (2 if layout.packed else 3)):
            raise ops._l.VqfError("AttHeadFn: a region layout (shared images, region counts, packed rows) is fp32 only where images are "
                                  "shared, for an fp32 feature tensor that is data -- (R, C) when packed -- and never the MLP's own source")
        if ctx.same_src and (x.numel() != feat.numel() or x.shape[-1] != feat.shape[-1] or x.dtype != feat.dtype):
            raise ops._l.VqfError("AttHeadFn: same_src needs x = feat.view(N*S, C)")
        ctx.link = link = link if (link is not None and link.inv is not None) else None
        if link is not None and (wm is not None or b1 is None):
            raise ops._l.VqfError("AttHeadFn: a NormLink needs the single-hidden-layer head with a bias")
        # bf16 operands, fp32 accumulate (BASELINE config 3), K padded to a multiple of 32; the entry point wants the hidden width
        # and, for the dgrad's N = C_in columns, the input width to be multiples of 8, else the head stays fp32
        w1_2 = _w2d(w1)
        d = _Dense(bf16, dims=w1_2.shape)
        ctx.bf16 = d.bf16
        rows = x.shape[0]
        ctx.pad = pad = ops.K_PAD_ROWS if (d.bf16 and layout is not None) else None    # the row padding of the weight gradient's operands
        hid2 = lin = None
        if link is not None:
            # x is the UN-NORMALISED fusion output: 1/norm of the sample (link.inv) rides in the conv GEMM's epilogue, and the logit
            # kernel also returns the part of each logit that is linear in x (NormLink).  bf16: the producer's own bf16 copy of x
            # is the operand where it left one of the padded shape
            w1o = d.operand(w1_2, 32)
            if d.bf16:
                xb, link.xb = link.xb, None
                x = xb if (xb is not None and xb.shape == (ops.pad_rows(rows) if pad else rows, w1o.shape[1])) else d.operand(x, 32, pad)
            hid1 = d.fwd(x, w1o, b1, True, scale=(link.inv, link.L), **({"K": x.shape[1], "M": rows} if d.bf16 else {}))
            logits, lin = ops.att_logits_fwd_lin(hid1, _w2d(w2), b2, b1)
        else:
            x, w1o = d.operand(x, 32, pad), d.operand(w1_2, 32)      # the backward only needs the operand
            hid1 = d.fwd(x, w1o, b1, True, **({"K": x.shape[1], "M": rows} if d.bf16 else {}))
            hid2 = ops.gemm(hid1, _w2d(wm), bias=bm, relu=True) if wm is not None else None
            logits = ops.att_logits_fwd(hid2 if hid2 is not None else hid1, _w2d(w2), b2)
        wts, pooled = _pool_fwd(feat, logits, unit_softmax, layout)
        # x: the first layer's operand; wm, hid2: the "multilayer" conv (never with a link); lin: link only; w1b: w1's bf16 copy (bf16
        # only).  (tests/node_harness.py reads the kernel's ReLU decisions from hid1 by position)
        ctx.save_for_backward(x, feat, w1, wm, w2, hid1, hid2, wts, lin, w1o if d.bf16 else None)
        ctx.unit = bool(unit_softmax)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        x, feat, w1, wm, w2, hid1, hid2, wts, lin, w1b = ctx.saved_tensors
        d = _Dense(ctx.bf16)
        dlogits, dfeat = _pool_bwd(_c(dpooled), feat, wts, ctx.unit, ctx.needs_input_grad[1], ctx.layout)
        dwm = dbm = None
        if ctx.link is not None:
            link = ctx.link
            obf = d.bf16 and hid1.shape[1] % 8 == 0 and w2.shape[0] == 2          # the kernel stores bf16 rows itself: no cast launch
            d1, dw2, db2, db1 = ops.att_logits_bwd(dlogits, hid1, _w2d(w2), relu_mask=True, rowscale=link.inv,
                                                   rows_per_scale=link.L, out_bf16=obf,   # stored rows already times 1/norm
                                                   pad_rows_to=ctx.pad if obf else None)
            link.lin = (dlogits, lin)                                               # -> sum(Y * dY) in the producer's backward
        elif hid2 is not None:
            dm, dw2, db2, dbm = ops.att_logits_bwd(dlogits, hid2, _w2d(w2), relu_mask=True)
            dwm = ops.gemm(dm, hid1, ta=True, tb=True).view_as(wm)
            d1, db1 = ops.relu_bwd(ops.gemm(dm, _w2d(wm), tb=True), hid1, want_bias=True)
        else:
            d1, dw2, db2, db1 = ops.att_logits_bwd(dlogits, hid1, _w2d(w2), relu_mask=True)
        # the first layer: dw1 = d1^T x and dx = d1 w1 (with a link d1 carries 1/norm, so dx = dY / norm)
        d1 = d.operand(d1, 8, ctx.pad)
        dw1 = d.dw(d1, x, w1)
        w1o = w1b if d.bf16 else _w2d(w1)
        dx = None
        if ctx.same_src and dfeat is not None and ctx.link is None and not d.bf16:
            d.dx(d1, w1o, out=dfeat.view(x.shape), accumulate=True)     # dfeat += dx: one gradient for the shared source
        elif ctx.needs_input_grad[0]:
            dx = d.dx(d1, w1o, **({"N": w1[0].numel(), "M": hid1.shape[0]} if d.bf16 else {}))
        return dx, dfeat, dw1, db1, dwm, dbm, dw2.view_as(w2), db2, None, None, None, None, None


def _arm_link(link, inv, L, xb=None):
    """producer side of a NormLink: publish 1/norm and the row-group size for the consumer's GEMM epilogue (and, in the bf16 modes,
    the bf16 copy of R the fusion kernel wrote beside the fp32 one: the consumer's GEMM operand without a cast pass)"""
    if link is not None:
        link.inv, link.L, link.lin, link.xb = inv, L, None, (xb[0] if xb else None)
    return link


def _take_lin(link):
    """producer's backward: the consumer's (dlogits, lin), exactly once"""
    if link is None:
        return None
    if link.lin is None:
        raise ops._l.VqfError("NormLink: the fusion output's consumer has not run its backward (the un-normalised output "
                              "of ImgFuseFn / MfbFuseFn may only feed the co-attention AttHeadFn it was linked to)")
    lin, link.lin = link.lin, None
    return lin


def _fuse_node_fwd(ctx, P, pbias, q, keep, seed, p_drop, N, L, link, layout):
    """The forward MfbFuseFn and ImgFuseFn share behind the projection P: the fusion, the link, what the backward needs on ctx"""
    O = P.shape[1] // ops.POOL_K
    Y, norm, inv, rb, scale = _fuse_fwd(P, q, layout, N, L, O, link, keep=keep, seed=seed, p_drop=p_drop, pbias=pbias)
    ctx.link = _arm_link(link, *(scale or (inv, L)), rb)
    ctx.layout, ctx.seed, ctx.p_drop, ctx.dims = layout, seed, p_drop, (N, L, O)
    return Y, norm, inv


def _fuse_node_bwd(ctx, dY, Y, norm, inv, P, q, keep, pbias, dp_bf16):
    """-> (dP, dq, dbias): the shared backward of the fusion"""
    N, L, O = ctx.dims
    return _fuse_bwd(_c(dY), Y, norm, inv, P, q, ctx.layout, N, L, O, dp_bf16=dp_bf16, keep=keep, seed=ctx.seed, p_drop=ctx.p_drop,
                     pbias=pbias, lin=_take_lin(ctx.link))


def _img_proj(img, wi, bf16, bias=None, store_bf16=True, out=None, pad_k=False):
    """a5, the one place that forms P = img W^T (+ bias): img (., ., D) flattened to rows -> (P, the 2-D image operand as the GEMM
    consumed it, which is what the weight gradient takes).  bf16: bf16 storage of the image tensor (a bf16 batch is used as it
    is, no per-step cast) and of the weight, fp32 accumulation; with store_bf16 P itself is STORED in bf16 when the large-tile
    kernel applies and ImgFuseFn.BF16_P allows (half the bytes of the largest tensor of the step in the GEMM epilogue, the
    fusion forward and the fusion backward).
    pad_k (bf16 on a region layout, whose row count R is whatever the counts add up to): the bf16 image operand comes back with
    ops.pad_rows(R) rows, exact zeros behind the R real ones, so that the weight gradient's K is a multiple of 32 and takes the
    large-tile kernel; the product keeps M = R, and a bf16 P has the padded row count too (zero rows no kernel reads: the gradient
    autograd hands back for it is the padded dP).  Where R is a multiple of 32 this is the call without pad_k."""
    img = _c(img)
    img2 = img.view(-1, img.shape[-1])
    if not bf16:
        return ops.gemm(img2, _w2d(wi), bias=bias, out=out), img2
    R = img2.shape[0]
    if img2.dtype != torch.bfloat16:
        img2 = ops.cast_bf16(img2, pad_rows_to=ops.K_PAD_ROWS if pad_k else None)
    wb = ops.cast_bf16(_w2d(wi))
    P = None
    if store_bf16 and ImgFuseFn.BF16_P:
        if img2.shape[0] != R:
            Pp = torch.empty((img2.shape[0], wb.shape[0]), dtype=torch.bfloat16, device=img2.device)
            if ops.gemm_bf16(img2, wb, bias=bias, M=R, out=Pp[:R], out_bf16=True) is not None:
                Pp[R:].zero_()
                P = Pp
        else:
            P = ops.gemm_bf16(img2, wb, bias=bias, out_bf16=True)
    if P is None:
        P = ops.gemm_bf16(img2, wb, bias=bias, M=R)
    return P, img2


def _img_wgrad(dP, img2, wi):
    """The projection's weight gradient dW = dP^T img2, K = the rows of P, for img2 as _img_proj returned it: a bf16 image operand
    takes dP in bf16 -- as the fusion's backward wrote it (no cast pass), or cast here (to img2's rows where _img_proj padded them:
    both operands' tails are exact zeros)."""
    dP = _c(dP)
    if img2.dtype == torch.bfloat16:
        if dP.dtype != torch.bfloat16:
            dP = ops.cast_bf16(dP, pad_rows_to=ops.K_PAD_ROWS if img2.shape[0] != dP.shape[0] else None)
        if dP.shape[0] != img2.shape[0]:
            raise ops._l.VqfError("image projection weight gradient: dP has %d rows, the bf16 image operand %d" % (dP.shape[0], img2.shape[0]))
        return ops.gemm_bf16(dP, img2, ta=True, tb=True).view_as(wi)
    return ops.gemm(dP, img2, ta=True, tb=True).view_as(wi)


def _cu_bracket(cu_limit):
    """cu_limit > 0: the persistent large-tile GEMMs inside the block leave the other CUs to kernels of other streams (library
    option gemm_cu_limit).  0: the option is left alone, so a limit the user set with ops.set_option / VQF_GEMM_CU_LIMIT applies."""
    return ops.options(gemm_cu_limit=cu_limit) if cu_limit else ops.options()


class ImgFuseFn(torch.autograd.Function):
    """a5+a6: P = img W^T + b;  Y = L2norm_n(ssqrt(pool5(dropout(P * q[n])))).

    img (N,L,D) data (no gradient), wi (5000,D[,1,1]), bi (5000), q (N,5000)
    -> Y (N*L, 1000), row m = n*L + l   (the reference's fusion_normed is the
    (N,1000,L,1) permutation of the same values, mfb.py:103-106).
    layout (None, or the grouping.RegionLayout of img; img itself fp32; bf16 -- the models' regions_bf16 -- only where no images are
    shared: bf16 operands for the projection and its weight gradient, dP and, where the large-tile GEMM applies, P stored in bf16,
    both operands of the weight gradient zero-padded to K % 32 == 0 rows).  Shared images: img is (U, L, D); the projection and its weight
    gradient run on U*L rows, the fusion reads P through idx and its backward sums dP per image.  Region counts: sample n has
    lens_q[n] real regions; the projection and its weight gradient still run over every row, the fusion reads no padded row of P
    and hands back exact zero dP rows there, so finite padding cancels in the weight gradient.  Packed rows: img is (1, R, D), the
    real rows of every image one after the other; the projection and its weight gradient run on the R real rows (P and dP are
    (R, 5000)); Y stays (N*L, 1000) with exact zero rows beyond each count -- unless layout.rows, where Y and dY are (R, 1000) too.
    (_fuse_fwd / _fuse_bwd pick the kernels.)
    """

    BF16_P = True      # bf16 mode: store P in bf16 when the large-tile GEMM applies (A/B switch)

    @staticmethod
    def forward(ctx, img, wi, bi, q, keep, seed, p_drop, bf16=False, link=None, layout=None):
        img, q = _c(img), _c(q)
        N, L = (img.shape[0], img.shape[1]) if layout is None else (layout.N, layout.L)
        ctx.bf16 = bool(bf16)
        if layout is not None and ((ctx.bf16 and layout.grouped) or img.dtype != torch.float32):
            raise ops._l.VqfError("ImgFuseFn: a region layout (shared images, region counts, packed rows) takes fp32 features, and "
                                  "shared images are fp32 only")
        # once per image where they are shared; packed: the real rows only
        P, img2 = _img_proj(img, wi, ctx.bf16, bias=bi, pad_k=layout is not None)
        Y, norm, inv = _fuse_node_fwd(ctx, P, None, q, keep, seed, p_drop, N, L, link, layout)
        ctx.save_for_backward(img2, wi, q, P, Y, norm, inv, keep)
        return Y

    @staticmethod
    def backward(ctx, dY):
        img2, wi, q, P, Y, norm, inv, keep = ctx.saved_tensors
        dP, dq, dbi = _fuse_node_bwd(ctx, dY, Y, norm, inv, P, q, keep, None, ctx.bf16)   # bf16: dP comes back in bf16
        return None, _img_wgrad(dP, img2, wi), dbi, dq, None, None, None, None, None, None


class ImgProjFn(torch.autograd.Function):
    """a5 alone: P0 = img W^T (NO bias: the bias is added inside the fusion kernel).  Split from the
    fusion so that the module can run this GEMM -- 86 % of the forward FLOPs, independent of the
    question path -- on a side stream; autograd then runs its weight-gradient GEMM on that same
    stream, concurrently with the question-side backward and the gradient all-reduce."""

    @staticmethod
    def forward(ctx, img, wi, bf16=False, pad_k=False):
        # (this node hands on an fp32 P0 in the bf16 mode too; pad_k: _img_proj)
        P0, img2 = _img_proj(img, wi, bool(bf16), store_bf16=False, pad_k=pad_k)
        ctx.save_for_backward(img2, wi)
        return P0

    @staticmethod
    def backward(ctx, dP):
        img2, wi = ctx.saved_tensors
        return None, _img_wgrad(dP, img2, wi), None, None


class ImgProjDeferFn(torch.autograd.Function):
    """fp32 image projection whose NODE exists before its PRODUCT: forward() only allocates P0 and returns it; fill() issues the
    GEMM into that buffer later (a raw write the autograd graph does not see).  The one-stream form wants the node created
    FIRST (a node created first runs its backward last: the 14 ms weight gradient then hides the other gradients' all-reduce)
    but the product issued AFTER the question encoder: the projection is then not the kernel right behind the previous step's
    weight-gradient GEMM and Adam -- two back-to-back 14 ms MFMA-bound launches made the second one run 1.4 % slower (same box:
    14.67 vs 14.47 ms, `profiles/r03_all_configs.log`; forward-only steps reach 14.23)."""

    @staticmethod
    def forward(ctx, img, wi):
        img = _c(img)
        N, L, D = img.shape
        ctx.save_for_backward(img.view(N * L, D), wi)
        return torch.empty((N * L, wi.shape[0]), dtype=torch.float32, device=img.device)

    @staticmethod
    def fill(P0, img, wi):
        _img_proj(img, wi, False, out=P0.detach())

    @staticmethod
    def backward(ctx, dP):
        img2, wi = ctx.saved_tensors
        return None, _img_wgrad(dP, img2, wi)


def img_project(img, wi, bf16, cu_limit=0, pad_k=False):
    """a5 without an autograd node: P0 = img W^T (no bias), fp32 or -- bf16 operands -- STORED in bf16 when the large-tile
    kernel applies (_img_proj; pad_k as there).  Returns (P0, img2d as the GEMM consumed it).  cu_limit: _cu_bracket."""
    with _cu_bracket(cu_limit):
        return _img_proj(img, wi, bf16, pad_k=pad_k)


class ImgProjLateFn(torch.autograd.Function):
    """The autograd node of an image projection whose product was ALREADY computed (img_project, issued at the very start
    of the forward on a side stream).  Created late -- right before the fusion node that consumes P0 -- so that autograd runs
    its backward (the weight-gradient GEMM, 14 ms in fp32) right after the fusion's backward and BEFORE the question-side
    backward is issued: on its own stream it then overlaps the LSTM backward.  (A node created first runs last.)
    dP arrives in P0's dtype: fp32, or bf16 straight from vqf_mfb_fuse_bwd_pbf16 (no cast pass)."""

    @staticmethod
    def forward(ctx, P0, img2, wi, cu_limit=0):
        ctx.save_for_backward(img2, wi)
        ctx.cu_limit = cu_limit
        return P0.view_as(P0)

    @staticmethod
    def backward(ctx, dP):
        img2, wi = ctx.saved_tensors
        with _cu_bracket(ctx.cu_limit):
            return None, None, _img_wgrad(dP, img2, wi), None


class MfbFuseFn(torch.autograd.Function):
    """a6: Y = L2norm_n(ssqrt(pool5(dropout((P0 + bias) * q[n])))) for the L regions of each sample.
    P0 fp32, or bf16 (then dP is handed back in bf16 too: the bf16 mode's projection storage).
    layout (None, or the grouping.RegionLayout of the projected image tensor; a bf16 P0 only where no images are shared, and then
    with ops.pad_rows(layout.R) rows, as dP), as in ImgFuseFn.  Shared images: P0 is
    (U*L, 5000) and dP comes back (U*L, 5000), summed over each image's questions, so the projection node behind it (ImgProjFn /
    ImgProjDeferFn / ImgProjLateFn) runs its weight gradient with K = U*L.  Region counts: no padded row of P0 is read, the padded
    rows of dP are exact zeros.  Packed rows: P0 and dP are (R, 5000), the real rows."""

    @staticmethod
    def forward(ctx, P0, bi, q, keep, seed, p_drop, N, L, link=None, layout=None):
        P0, q = _c(P0), _c(q)
        if layout is not None and P0.dtype != torch.float32 and (layout.grouped or P0.shape[0] != ops.pad_rows(layout.R)):
            raise ops._l.VqfError("MfbFuseFn: shared images are fp32 only, and a bf16 projection on a region layout has the rows of "
                                  "the layout rounded up to a multiple of %d; got a %s projection of %d rows"
                                  % (ops.K_PAD_ROWS, P0.dtype, P0.shape[0]))
        Y, norm, inv = _fuse_node_fwd(ctx, P0, bi, q, keep, seed, p_drop, N, L, link, layout)
        ctx.save_for_backward(P0, bi, q, Y, norm, inv, keep)
        return Y

    @staticmethod
    def backward(ctx, dY):
        P0, bi, q, Y, norm, inv, keep = ctx.saved_tensors
        dP, dq, dbi = _fuse_node_bwd(ctx, dY, Y, norm, inv, P0, q, keep, bi, P0.dtype == torch.bfloat16)
        return dP, dbi, dq, None, None, None, None, None, None, None


class _Fork:
    """Run a block of launches on a second stream beside the caller's (two independent ~100-us products of a final MFB block:
    each leaves a third of the chip's issue slots idle in its prologue, tail and slab reduce).  with _Fork(dev) as f: ... launches
    on the side stream ...; f.join(*tensors_made_there) makes the caller's stream wait and tells the allocator who reads them."""
    _streams = {}

    def __init__(self, device):
        self.cur = torch.cuda.current_stream(device)
        self.side = _Fork._streams.get(device)
        if self.side is None:
            self.side = _Fork._streams[device] = torch.cuda.Stream(device=device)
        self.side.wait_stream(self.cur)
        self._ctx = torch.cuda.stream(self.side)

    def __enter__(self):
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)

    def join(self, *tensors):
        self.cur.wait_stream(self.side)
        for t in tensors:
            if t is not None:
                t.record_stream(self.cur)


class FinalMfbFn(torch.autograd.Function):
    """a9: y = L2norm_row(ssqrt(pool5(dropout((qa Wq^T + bq) * (va Wv^T + bv))))), (N,1000).

    cascade (N,5000) optional third factor and want_zdrop: MHB's high-order block
    (mhb_coAtt.py:201-211) reuses this stage.
    """

    TWO_STREAMS = False    # A/B: the question-side and image-side products (and their gradients) on two streams

    @staticmethod
    def forward(ctx, qa, va, wq, bq, wv, bv, keep, seed, p_drop, cascade=None, want_zdrop=False, bf16=False):
        qa, va = _c(qa), _c(va)
        N = qa.shape[0]
        O = wq.shape[0] // ops.POOL_K
        d = _Dense(bf16, dims=(N, qa.shape[1], va.shape[1], wq.shape[0]))      # "bf16-all": both projections with bf16 operands
        qa, va, wqo, wvo = d.operand(qa), d.operand(va), d.operand(_w2d(wq)), d.operand(_w2d(wv))
        if FinalMfbFn.TWO_STREAMS and not d.bf16:          # the image-side product beside the question-side one
            with _Fork(qa.device) as f:
                vv = d.fwd(va, wvo, bv)
            qq = d.fwd(qa, wqo, bq)
            f.join(vv)
        else:
            qq, vv = d.fwd(qa, wqo, bq), d.fwd(va, wvo, bv)
        if cascade is not None:
            cascade = _c(cascade)
        y, norm, inv, zdrop = ops.mfb_fuse_fwd(vv, qq, N, 1, O, keep=keep, seed=seed, p_drop=p_drop,
                                               cascade=cascade, want_zdrop=want_zdrop)
        ctx.save_for_backward(qa, va, wq, wv, qq, vv, y, norm, inv, keep, cascade, *((wqo, wvo) if d.bf16 else (None, None)))
        ctx.seed, ctx.p_drop, ctx.dims, ctx.bf16 = seed, p_drop, (N, O), d.bf16
        if want_zdrop:
            return y, zdrop
        return y

    @staticmethod
    def backward(ctx, dy, dz=None):
        qa, va, wq, wv, qq, vv, y, norm, inv, keep, cascade, wqb, wvb = ctx.saved_tensors
        N, O = ctx.dims
        dvv, dqq, dcasc, _ = ops.mfb_fuse_bwd(_c(dy), y, norm, inv, vv, qq, N, 1, O, keep=keep,
                                              seed=ctx.seed, p_drop=ctx.p_drop, cascade=cascade,
                                              dzdrop=None if dz is None else _c(dz))
        d = _Dense(ctx.bf16)
        dqo, dvo = d.operand(dqq), d.operand(dvv)
        wqo, wvo = (wqb, wvb) if d.bf16 else (_w2d(wq), _w2d(wv))
        need_q, need_v = ctx.needs_input_grad[:2]
        if FinalMfbFn.TWO_STREAMS and not d.bf16:          # each side's three launches together, the image side's on the second stream
            with _Fork(dqq.device) as f:
                dva, dwv, dbv = (d.dx(dvo, wvo) if need_v else None), d.dw(dvo, va, wv), ops.colsum(dvv)
            dqa, dwq, dbq = (d.dx(dqo, wqo) if need_q else None), d.dw(dqo, qa, wq), ops.colsum(dqq)
            f.join(dva, dwv, dbv)
        else:
            dqa = d.dx(dqo, wqo) if need_q else None
            dva = d.dx(dvo, wvo) if need_v else None
            dwq, dwv = d.dw(dqo, qa, wq), d.dw(dvo, va, wv)
            dbq, dbv = ops.colsum(dqq), ops.colsum(dvv)
        return dqa, dva, dwq, dbq, dwv, dbv, None, None, None, dcasc, None, None


# ---------------------------------------------------------------------------------------------
# stages used by HieCoAtten (hieCoAtten.py) and modules.py / networks.py
# ---------------------------------------------------------------------------------------------
class DropoutFn(torch.autograd.Function):
    """F.dropout with an in-kernel Philox mask (or an explicit uint8 keep-mask)."""

    @staticmethod
    def forward(ctx, x, keep, seed, p_drop):
        x = _c(x)
        ctx.keep, ctx.seed, ctx.p = keep, seed, p_drop
        return ops.dropout(x, keep=keep, seed=seed, p_drop=p_drop)

    @staticmethod
    def backward(ctx, dy):
        return ops.dropout(_c(dy), keep=ctx.keep, seed=ctx.seed, p_drop=ctx.p), None, None, None


class DropoutBTFn(torch.autograd.Function):
    """The LSTM-output dropout (mfb.py:70, mhb_coAtt.py:75): x (B, T, H), any strides on the first two axes (MFB hands in the
    transposed view of its time-major LSTM states) -> CONTIGUOUS dropout(x); the gradient goes back in x's own layout, so the
    (T, B, H) <-> (B, T, H) re-layouts of both directions ride in the two dropout passes instead of torch copy kernels.
    lens ((B,) int32; HieCoAttenLadder's sentence level): rows t >= lens[b] are zero in the output, and so is their gradient."""

    @staticmethod
    def forward(ctx, x, keep, seed, p_drop, lens=None):
        ctx.keep, ctx.seed, ctx.p, ctx.lens = keep, seed, p_drop, lens
        ctx.in_strides = (x.stride(0), x.stride(1))
        return ops.dropout_bt(x, torch.empty(x.shape, dtype=torch.float32, device=x.device), keep, seed, p_drop, lens=lens)

    @staticmethod
    def backward(ctx, dy):
        B, T, H = dy.shape
        if dy.stride(2) != 1 or dy.stride(0) % 4 or dy.stride(1) % 4 or dy.data_ptr() % 16:
            dy = dy.contiguous()           # an offset view or odd strides: the kernel wants 16-byte rows
        sb, st = ctx.in_strides
        if st > sb and sb == H and st == B * H:                     # x was the transposed view of a contiguous (T, B, H) tensor
            dx = torch.empty((T, B, H), dtype=torch.float32, device=dy.device).transpose(0, 1)
        else:
            dx = torch.empty((B, T, H), dtype=torch.float32, device=dy.device)
        ops.dropout_bt(dy, dx, ctx.keep, ctx.seed, ctx.p, lens=ctx.lens)
        return dx, None, None, None, None


def lstm_out_dropout(module, x, seeds, tag="l"):
    """dropout_l / lstm_dropout of the reference modules on the HIP path: rate = the nn.Dropout's p in train mode, 0 in eval
    (then the pass only makes x contiguous); an explicit (B*T, H) keep-mask under `tag` replaces the in-kernel Philox draw."""
    if x.dim() == 3 and x.is_cuda and x.dtype == torch.float32 and x.stride(2) == 1 and x.shape[2] % 4 == 0 \
            and all(s % 4 == 0 for s in x.stride()[:2]) and x.data_ptr() % 16 == 0:
        keep, seed, rate = seeds.draw(tag, module.training, float(module.p) if module.training else 0.0)   # (rate 0 draws nothing)
        if rate <= 0.0 and keep is None and x.is_contiguous():
            return x
        return DropoutBTFn.apply(x, keep, seed, rate)
    return module(x).contiguous()


class TanhDropFn(torch.autograd.Function):
    """y = dropout(tanh(a [+ b]))   (hieCoAtten.py:32-33,38-39,45-46)."""

    @staticmethod
    def forward(ctx, a, b, keep, seed, p_drop):
        a = _c(a)
        b = None if b is None else _c(b)
        y = ops.tanh_dropout_fwd(a, b, keep=keep, seed=seed, p_drop=p_drop)
        ctx.save_for_backward(y)
        ctx.keep, ctx.seed, ctx.p, ctx.has_b = keep, seed, p_drop, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = ops.tanh_dropout_bwd(_c(dy), y, keep=ctx.keep, seed=ctx.seed, p_drop=ctx.p)
        return dx, (dx if ctx.has_b else None), None, None, None


class TanhDropUnpackFn(torch.autograd.Function):
    """y (U*L, E) = dropout(tanh(z)) laid out padded, from z (R, E) packed rows and roff (U + 1) int32 (HieCoAttenLadder on a
    PackedRegions): the tanh / dropout pass is where the layout changes.  Padded rows of y are exact zeros; the masks are those of
    TanhDropFn on the padded tensor.  Backward: dz (R, E), the real rows only (vqf_tanh_dropout_pack_bwd)."""

    @staticmethod
    def forward(ctx, z, roff, U, L, keep, seed, p_drop):
        z = _c(z)
        y = ops.tanh_dropout_unpack_fwd(z, roff, U, L, keep=keep, seed=seed, p_drop=p_drop)
        ctx.save_for_backward(y, roff)
        ctx.keep, ctx.seed, ctx.p, ctx.dims = keep, seed, p_drop, (U, z.shape[0], L)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, roff = ctx.saved_tensors
        U, R, L = ctx.dims
        dz = ops.tanh_dropout_pack_bwd(_c(dy), y, roff, U, R, L, keep=ctx.keep, seed=ctx.seed, p_drop=ctx.p)
        return dz, None, None, None, None, None, None


class TanhDropPackedFn(torch.autograd.Function):
    """y (R, E) = dropout(tanh(z)) with BOTH sides packed (HieCoAttenLadder(packed_coatt=True) on a PackedRegions): the rows of
    TanhDropUnpackFn without the padded layout.  The masks stay those of the padded tensor (keep (U*L, E), Philox index
    (u*L + l)*E + c), so row start + l holds the bits of TanhDropUnpackFn's row u*L + l.  Backward: dz (R, E)."""

    @staticmethod
    def forward(ctx, z, roff, U, L, keep, seed, p_drop):
        y = ops.tanh_dropout_packed_fwd(_c(z), roff, U, L, keep=keep, seed=seed, p_drop=p_drop)
        ctx.save_for_backward(y, roff)
        ctx.keep, ctx.seed, ctx.p, ctx.dims = keep, seed, p_drop, (U, L)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, roff = ctx.saved_tensors
        U, L = ctx.dims
        dz = ops.tanh_dropout_packed_bwd(_c(dy), y, roff, U, L, keep=ctx.keep, seed=ctx.seed, p_drop=ctx.p)
        return dz, None, None, None, None, None, None


class GateFn(torch.autograd.Function):
    """y = tanh(a) * sigmoid(b): the gate of Nonlinear_layer (modules.py:103-109), one launch each way."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        ctx.save_for_backward(a, b)
        return ops.gate_tanh_sigmoid_fwd(a, b)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        return ops.gate_tanh_sigmoid_bwd(_c(dy), a, b)


class BmmFn(torch.autograd.Function):
    """Batched C_b = Aop_b @ Bop_b^T on the fp32 MFMA GEMM.

    ta=False: a is (B,M,K), ta=True: a is (B,K,M); tb=False: b is (B,N,K), tb=True: b is (B,K,N).
    """

    @staticmethod
    def forward(ctx, a, b, ta, tb):
        a, b = _c(a), _c(b)
        ctx.save_for_backward(a, b)
        ctx.ta, ctx.tb = ta, tb
        return ops.bgemm(a, b, ta=ta, tb=tb)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = _c(dc)
        ta, tb = ctx.ta, ctx.tb
        da = db = None
        if ctx.needs_input_grad[0]:
            if not ta:      # dA (B,M,K) = dC (M,N) x Bop (N,K)
                da = ops.bgemm(dc, b, ta=False, tb=not tb)
            else:           # dA (B,K,M) = Bop^T (K,N) x dC^T (N,M)
                da = ops.bgemm(b, dc, ta=not tb, tb=False)
        if ctx.needs_input_grad[1]:
            if not tb:      # dB (B,N,K) = dC^T (N,M) x Aop (M,K)
                db = ops.bgemm(dc, a, ta=True, tb=not ta)
            else:           # dB (B,K,N) = Aop^T (K,M) x dC (M,N)
                db = ops.bgemm(a, dc, ta=not ta, tb=True)
        return da, db, None, None


class AttPoolFn(torch.autograd.Function):
    """logits = x W^T + b (G rows, no hidden layer), softmax over the S positions of a sample,
    pooled[n] = sum_s wts[n,g,s] feat[n,s,:].  Returns (pooled (N,G*C), wts (N,G,S)), both
    differentiable (hieCoAtten.py:40-42,47-49 and :55; modules.py:60-65; networks.py:64-66).
    x (N*S, Cin), feat (N,S,C), w (G,Cin), b (G)."""

    @staticmethod
    def forward(ctx, x, feat, w, b, pooled_out=None):
        """pooled_out: a contiguous (N, G*C) buffer (a row block of a larger one) the pooled vectors are written into"""
        x, feat = _c(x), _c(feat)
        w2 = _w2d(w)
        logits = ops.att_logits_fwd(x, w2, b)
        wts, pooled = ops.glimpse_pool_fwd(feat, logits, False, pooled_out=pooled_out)
        ctx.save_for_backward(x, feat, w, wts)
        # (pooled_out is written as raw memory, like ImgProjDeferFn.fill: the output is a fresh view of it, autograd sees no
        #  in-place operation on the buffer)
        return (pooled.view_as(pooled) if pooled_out is not None else pooled), wts

    @staticmethod
    def backward(ctx, dpooled, dwts):
        x, feat, w, wts = ctx.saved_tensors
        dlogits, dfeat = ops.glimpse_pool_bwd(_c(dpooled), feat, wts, False, ctx.needs_input_grad[1],
                                              dwts=None if dwts is None else _c(dwts))
        dx, dw, db, _ = ops.att_logits_bwd(dlogits, x, _w2d(w), relu_mask=False)
        return (dx if ctx.needs_input_grad[0] else None), dfeat, dw.view_as(w), db, None


def _hie_hv_ti(Vh, C, Qh, drop, N, L, T, Hv, ti, stream, rlens=None):
    """One co-attention level's image side: Hv = dropout(tanh(Vh + C^T Qh)) and the T-row sums ti = C Vh, written into Hv
    (N*L, E) and ti (N*T, E).  Vh, Hv, Qh may be column blocks of wider buffers; C (N, T, L).  stream: ONE pass over Vh
    (csrc/hie.hip) -- one workgroup per sample writes the final sums; small batches cut a sample into S chunks whose
    partial slabs a second launch sums.  Otherwise the batched-GEMM form.
    rlens ((N,) int32 region counts or None; HieCoAttenLadder; C comes with zero columns at l >= rlens[n]): the streaming pass
    stops at the count and writes zero Hv rows behind it (vqf_hie_hv_fwd_regions); the batched-GEMM form needs nothing -- its
    padded Hv rows are finite and never used."""
    E = Vh.shape[1]
    if stream:
        rk = {} if rlens is None else {"rlens": rlens}
        S = ops.hie_chunks(N, L)
        if S == 1:
            ops.hie_hv_fwd(Vh, C, Qh, drop, N, L, T, Hv, ti, **rk)
        else:
            part = torch.empty((S, N * T, E), dtype=torch.float32, device=Vh.device)
            ops.hie_hv_fwd(Vh, C, Qh, drop, N, L, T, Hv, part, **rk)
            ops.hie_slab_sum(part, ti)
    else:
        tq = ops.bgemm(C, Qh.view(N, T, E), ta=True, tb=True).view(N * L, E)                # C^T Qh
        ops.tanh_dropout_fwd2d(Vh, tq, *drop, out=Hv)
        ops.bgemm(C, Vh.view(N, L, E), ta=False, tb=True, out=ti.view(N, T, E))             # C Vh


def _hie_dc(dti, Vh, Qh, dtq, C, drop, N, L, T, aff, out=None, lens=None, rlens=None):
    """One level's gradient of the affinity's pre-activation: (dti Vh^T + Qh dtq^T) through the backward of
    C = dropout(tanh(.)), (N, T, L).  aff: ONE pass over Vh and dtq (vqf_hie_affinity, two pairs); otherwise two batched
    products and the element-wise backward.  Reads dtq: call it before dtq is updated in place.
    lens ((N,) int32, no dropout; HieCoAttenLadder): the rows t >= lens[n] of the result are zero (the affinity's epilogue, or
    the element-wise backward's row test: no extra pass).
    rlens ((N,) int32 region counts; HieCoAttenLadder): the columns l >= rlens[n] of the result are zero -- dti . Vh[l] of a padded
    region is not zero by arithmetic -- in the affinity's epilogue (vqf_hie_affinity_regions), or by vqf_zero_cols_len behind the
    element-wise backward."""
    if aff:
        rk = {} if rlens is None else {"rlens": rlens}
        return ops.hie_affinity(dti, Vh, N, L, T, x2=Qh, y2=dtq, epi=2, yprev=C, drop=drop, out=out, lens=lens, **rk)
    E = Vh.shape[1]
    dC = ops.bgemm(dti.view(N, T, E), Vh.view(N, L, E), out=out)
    ops.bgemm(Qh.view(N, T, E), dtq.view(N, L, E), out=dC, accumulate=True)
    if lens is not None:
        if drop[0] is not None or drop[2] != 0.0:
            raise ops._l.VqfError("_hie_dc: lens without dropout on C only")
        ops.tanh_bwd_rows_len(dC, C, lens, N, T, out=dC)
    else:
        ops.tanh_dropout_bwd(dC.view(N * T, L), C.view(N * T, L), *drop, out=dC.view(N * T, L))
    if rlens is not None:
        ops.zero_cols_len(dC, rlens, T, N, L)
    return dC


def _hie_bwd_bgemm(C, dC, dti, dtq, V, Cq, dQh, dCq, dV, N, L, T, dv_accumulate):
    """The batched-GEMM form of one level's remaining backward products (the streaming passes' A/B partner):
    dQh += C dtq;  dtq += C^T dti (in place: dtq becomes dVh);  dCq = dC V;  dV = (dV +) dC^T Cq."""
    E = V.shape[1]
    ops.bgemm(C, dtq.view(N, L, E), ta=False, tb=True, out=dQh.view(N, T, E), accumulate=True)
    ops.bgemm(C, dti.view(N, T, E), ta=True, tb=True, out=dtq.view(N, L, E), accumulate=True)
    ops.bgemm(dC, V.view(N, L, E), ta=False, tb=True, out=dCq.view(N, T, E))
    ops.bgemm(dC, Cq.view(N, T, E), ta=True, tb=True, out=dV.view(N, L, E), accumulate=dv_accumulate)


class HieCoreFn(torch.autograd.Function):
    """HieCoAtten's ladder from the raw inputs to cat((v, q), 0).view(N, -1) (hieCoAtten.py:25-53) as ONE autograd node with a
    hand-ordered backward, so that
      * fc_Wbv and fc_Wv, both applied to `img` (:30,35), are ONE product with the concatenated (2E, E) weight -- [Cv | img_] =
        img [Wbv; Wv]^T, a (N*L, 2E) buffer whose halves the later stages consume in place (row-strided operands) -- and the
        question side likewise ([Cq | que_] = que [Wbv; Wq]^T: :31 applies fc_Wbv to the question too);
      * their input gradients are ONE product with K = 2E over the gradient buffer [dCv | dimg_], which the batched products
        and the tanh backward fill in place (VQF_GEMM_ACCUM where two consumers meet): no gradient-accumulation adds of the
        (N*L, E) tensors, one weight-gradient product per side;
      * the attention pool's gradient into `img` -- the rank-1 term av[n,l] * dv[n,:] -- is never materialised: the backward of
        dropout(relu(img_emb(.))) adds it on the fly (vqf_relu_bwd_rank1_f32);
      * v and q land in the two halves of one (2N, E) buffer: the reference's cat is a view.
    drops: {tag: (keep mask | None, seed, p)} for 'img', 'que', 'C', 'Hv', 'Hq' (the always-on functional dropouts).
    Returns (x (N, 2E), av (N,1,L), aq (N,1,T)), all differentiable."""

    STREAM = True      # the tiny-T stages as streaming passes (csrc/hie.hip) where supported; False: batched GEMMs + element-wise (A/B)
    AFFINITY = True    # Cq Cv^T and its gradient on vqf_hie_affinity (needs STREAM); False: batched GEMMs + element-wise (A/B)

    @staticmethod
    def forward(ctx, imgf, ids, w_emb, b_emb, w_que, wbv, bbv, wv, bv, wq, bq, whv, bhv, whq, bhq, drops):
        imgf, ids = _c(imgf), ids.contiguous()
        N, L, D = imgf.shape
        T = ids.shape[1]
        E = w_emb.shape[0]
        M, MT = N * L, N * T
        dev = imgf.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        # :25-26  img = dropout(relu(img_emb(img_features)))   (ReLU in the GEMM epilogue, the dropout in place)
        # (per-sample tiles where the library takes the shape: 256 samples x 196 regions = one workgroup per CU, csrc/gemm_f32_sample.hip)
        img = ops.gemm_rows(imgf.view(M, D), _c(w_emb), L, bias=b_emb, relu=True)
        ops.dropout(img, *drops["img"], out=img)
        # :27-28  que = dropout(que_emb(que_features))
        if E % 4 == 0 and E <= 1024:
            que = ops.embed_dropout_fwd(_c(w_que), ids, *drops["que"])           # lookup + dropout in one launch
        else:
            que = ops.embed_tanh_fwd(_c(w_que), ids, False).view(MT, E)
            ops.dropout(que, *drops["que"], out=que)
        # :30-31,35-36  the four E x E layers as two products with concatenated weights
        Wi, bi, Wq2, bq2 = new(2 * E, E), new(2 * E), new(2 * E, E), new(2 * E)
        ops.multi_copy([(_c(wbv), Wi[:E]), (_c(wv), Wi[E:]), (bbv, bi[:E]), (bv, bi[E:]),
                        (_c(wbv), Wq2[:E]), (_c(wq), Wq2[E:]), (bbv, bq2[:E]), (bq, bq2[E:])])
        CI = ops.gemm_rows(img, Wi, L, bias=bi)               # (M, 2E)  = [Cv | img_]
        CQ = ops.gemm(que, Wq2, bias=bq2)                     # (MT, 2E) = [Cq | que_]
        # :32-33  C = dropout(tanh(Cq Cv^T))   (N,T,L)
        stream = HieCoreFn.STREAM and ops.hie_stream_supported(N, L, E, T)
        aff = stream and HieCoreFn.AFFINITY and ops.hie_affinity_supported(N, L, E, T, 2)
        if aff:                  # one pass over Cv on 16x16x4 MFMAs, tanh + dropout in its epilogue (csrc/hie.hip)
            C3 = ops.hie_affinity(CQ[:, :E], CI[:, :E], N, L, T, epi=1, drop=drops["C"])
        else:
            C3 = ops.bgemm(CQ[:, :E].view(N, T, E), CI[:, :E].view(N, L, E))
            ops.tanh_dropout_fwd(C3.view(MT, L), None, *drops["C"], out=C3.view(MT, L))
        # :38-42  Hv = dropout(tanh(img_ + C^T que_)), av = softmax_L(Whv Hv), v = av^T img;  :45  ti = C img_
        Hv, ti = new(M, E), new(MT, E)
        _hie_hv_ti(CI[:, E:], C3, CQ[:, E:], drops["Hv"], N, L, T, Hv, ti, stream)
        xcat = new(2 * N, E)
        av, _ = ops.glimpse_pool_fwd(img.view(N, L, E), ops.att_logits_fwd(Hv, _w2d(whv), bhv), False, pooled_out=xcat[:N])
        # :45-49  Hq = dropout(tanh(que_ + C img_)), aq = softmax_T(Whq Hq), q = aq^T que
        Hq = ops.tanh_dropout_fwd2d(CQ[:, E:], ti, *drops["Hq"], out=ti)
        aq, _ = ops.glimpse_pool_fwd(que.view(N, T, E), ops.att_logits_fwd(Hq, _w2d(whq), bhq), False, pooled_out=xcat[N:])
        ctx.save_for_backward(imgf, ids, img, que, Wi, Wq2, CI, CQ, C3, Hv, Hq, av, aq, whv, whq)
        ctx.drops, ctx.dims, ctx.V, ctx.stream, ctx.aff = drops, (N, L, T, D, E), w_que.shape[0], stream, aff
        # an output nobody differentiates (av / aq under a loss on x: solver.py:84-91) arrives as None in the backward, not as a
        # zero tensor torch has to fill and the pooling kernels have to read
        ctx.set_materialize_grads(False)
        return xcat.view(N, 2 * E), av, aq                    # :52-53: cat((v, q), 0).view(N, -1) is a view of xcat

    @staticmethod
    def backward(ctx, dx, dav, daq):
        imgf, ids, img, que, Wi, Wq2, CI, CQ, C3, Hv, Hq, av, aq, whv, whq = ctx.saved_tensors
        N, L, T, D, E = ctx.dims
        M, MT = N * L, N * T
        drops = ctx.drops
        dev = imgf.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        if dx is None:
            dx = torch.zeros((N, 2 * E), dtype=torch.float32, device=dev)
        dxcat = _c(dx).view(2 * N, E)
        dv, dq = dxcat[:N], dxcat[N:]
        dCI, dCQ = new(M, 2 * E), new(MT, 2 * E)              # [dCv | dimg_], [dCq | dque_]
        # question-side head: q = aq^T que, aq = softmax(Whq Hq), Hq = dropout(tanh(que_ + ti))
        dlq, dque = ops.glimpse_pool_bwd(dq, que.view(N, T, E), aq, False, True, dwts=None if daq is None else _c(daq))
        dHq, dwhq, dbhq, _ = ops.att_logits_bwd(dlq, Hq, _w2d(whq), relu_mask=False)
        if not ctx.stream:
            ops.tanh_dropout_bwd2d(dHq, Hq, *drops["Hq"], out=dCQ[:, E:])      # d(que_ + ti): first term of dque_ ...
        dti = ops.tanh_dropout_bwd2d(dHq, Hq, *drops["Hq"], out=dHq)           # ... and, untouched by the sums below, dti (7 MB)
        # image-side head
        dlv, _ = ops.glimpse_pool_bwd(dv, img.view(N, L, E), av, False, False, dwts=None if dav is None else _c(dav))
        if ctx.stream:
            # dtq = d(img_ + tq) straight from the logit gradient (dHv = dlv (x) whv is never written), C dtq and dlv^T Hv on the way
            S = ops.hie_chunks(N, L)
            # one buffer of partial rows, one per workgroup: [colsum dCv | colsum dimg_ | dl^T Hv | sum dl | 0 0 0]; its column
            # sums are the bias gradient of [fc_Wbv; fc_Wv] (no column-sum pass over the 205 MB gradient buffer) and d fc_Whv
            cpart = new(S * N, 3 * E + 4)
            part, wpart = (None if S == 1 else new(S, MT, E)), cpart[:, 2 * E:]
            if S == 1:           # dque_ = dti + C dtq written by the pass itself (one workgroup per sample)
                ops.hie_head_bwd(Hv, dlv.view(M), whv.view(E), C3, drops["Hv"], N, L, T, dCI[:, E:], dCQ[:, E:], wpart, part_add=dti)
            else:
                ops.hie_head_bwd(Hv, dlv.view(M), whv.view(E), C3, drops["Hv"], N, L, T, dCI[:, E:], part, wpart)
            # dC = dti img_^T + que_ dtq^T and the backward of C = dropout(tanh(Cq Cv^T))
            dC3 = _hie_dc(dti, CI[:, E:], CQ[:, E:], dCI[:, E:], C3, drops["C"], N, L, T, ctx.aff)
            if S > 1:
                ops.hie_slab_sum(part, dCQ[:, E:], add=dti)                        # dque_ = dti + C dtq
            ops.hie_rank_add(dCI[:, E:], C3, dti, N, L, T, dCI[:, E:], colpart=cpart[:, E:2 * E])      # dimg_ = dtq + C^T dti (dtq's own uses are above)
            # dCv = dC^T Cq,  dCq = dC Cv   (one pass over Cv)
            if S == 1:
                ops.hie_rank_left(dC3, CQ[:, :E], CI[:, :E], N, L, T, dCI[:, :E], dCQ[:, :E], colpart=cpart[:, :E])      # dCq straight into its column block
            else:
                ops.hie_rank_left(dC3, CQ[:, :E], CI[:, :E], N, L, T, dCI[:, :E], part, colpart=cpart[:, :E])
                ops.hie_slab_sum(part, dCQ[:, :E])
        else:
            dHv, dwhv, dbhv, _ = ops.att_logits_bwd(dlv, Hv, _w2d(whv), relu_mask=False)
            ops.tanh_dropout_bwd2d(dHv, Hv, *drops["Hv"], out=dCI[:, E:])          # d(img_ + tq), first term of dimg_
            del dHv
            # tq = C^T que_, ti = C img_, C = dropout(tanh(Cq Cv^T)):  dC, then dque_ += C dtq;  dimg_ += C^T dti;  dCq = dC Cv;
            # dCv = dC^T Cq
            dC3 = _hie_dc(dti, CI[:, E:], CQ[:, E:], dCI[:, E:], C3, drops["C"], N, L, T, False)
            _hie_bwd_bgemm(C3, dC3, dti, dCI[:, E:], CI[:, :E], CQ[:, :E], dCQ[:, E:], dCQ[:, :E], dCI[:, :E], N, L, T, False)
        # the concatenated layers: one input-gradient product (K = 2E), one weight-gradient product and one column sum per side
        dimg = ops.gemm_rows(dCI, Wi, L, tb=True)                              # (M, E); the pool's rank-1 term is added below
        ops.gemm(dCQ, Wq2, tb=True, out=dque.view(MT, E), accumulate=True)     # on top of the pool's gradient into que
        dWi, dWq2 = ops.gemm(dCI, img, ta=True, tb=True), ops.gemm(dCQ, que, ta=True, tb=True)
        if ctx.stream:
            csum = ops.colsum(cpart)
            dbi, dwhv, dbhv = csum[:2 * E], csum[2 * E:3 * E], csum[3 * E:3 * E + 1]
        else:
            dbi = ops.colsum(dCI)
        dbq2 = ops.colsum(dCQ)
        dwbv, dbbv = new(E, E), new(E)
        ops.multi_add([(dWi[:E], dWq2[:E], dwbv), (dbi[:E], dbq2[:E], dbbv)])  # fc_Wbv serves both sides (:30-31)
        # img = dropout(relu(img_emb(.))): mask, 1 / (1 - p) and the pool's av[n,l] * dv[n,:] in one pass, in place
        keep_i, _, p_i = drops["img"]
        scale = 1.0 / (1.0 - p_i) if (keep_i is not None or p_i > 0.0) else 1.0
        dpre, db_emb = ops.relu_bwd_rank1(dimg, img, av.view(M), dv, L, scale, want_bias=True, out=dimg)
        dw_emb = ops.gemm(dpre, imgf.view(M, D), ta=True, tb=True)
        dque2 = dque.view(MT, E)
        if E % 4 == 0 and E <= 1024:
            dw_que = ops.embed_dropout_bwd(dque2, ids, ctx.V, *drops["que"])     # dropout's backward inside the segment sums
        else:
            ops.dropout(dque2, *drops["que"], out=dque2)
            dw_que = ops.embed_tanh_bwd(dque2, None, ids, ctx.V)
        return (None, None, dw_emb, db_emb, dw_que, dwbv, dbbv, dWi[E:], dbi[E:], dWq2[E:], dbq2[E:],
                dwhv.view_as(whv), dbhv, dwhq.view_as(whq), dbhq, None)


class SoftmaxRowsFn(torch.autograd.Function):
    """softmax over the last axis of a 2-D tensor (modules.py:91-92)."""

    @staticmethod
    def forward(ctx, x):
        y = ops.softmax_rows_fwd(_c(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.softmax_rows_bwd(_c(dy), y)


class LogSoftmaxRowsFn(torch.autograd.Function):
    """log_softmax over the last axis of the 2-D logits: the classifier tail of MHBCoAtt / MHB (mhb_coAtt.py:149-151,215-217)."""

    @staticmethod
    def forward(ctx, x):
        y = ops.log_softmax_rows_fwd(_c(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.log_softmax_rows_bwd(_c(dy), y)


def _bias_sum(b_ih, b_hh):
    """b_ih + b_hh of an nn.LSTM (one library launch; torch for anything the launch does not take)"""
    if b_ih is None:
        return None
    if b_ih.is_cuda and b_ih.dtype == torch.float32 and b_ih.is_contiguous() and b_hh.is_contiguous():
        out = torch.empty_like(b_ih)
        ops.multi_add([(b_ih.detach(), b_hh.detach(), out)])
        return out
    return b_ih + b_hh


def _copy_of(t):
    """a second tensor with t's values (b_hh's gradient beside b_ih's), one library launch"""
    if t is None:
        return None
    if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous():
        out = torch.empty_like(t)
        ops.multi_copy([(t, out)])
        return out
    return t.clone()


def _lstm_in_proj(x2, w_ih, bias, bf16_proj):
    """Input projection of a whole sequence, x2 (S*B, I) @ w_ih^T (+ b_ih + b_hh).  bf16_proj (gemm_dtype "bf16-all"):
    bf16 operands, columns zero-padded to a multiple of 8 by the cast (I = 300 -> 304); returns the casts for the
    backward."""
    if not bf16_proj:
        return ops.gemm(x2, _c(w_ih), bias=bias), None, None
    xb, wb = ops.cast_bf16(x2), ops.cast_bf16(_c(w_ih))
    return ops.gemm_bf16(xb, wb, bias=bias), xb, wb


def _lstm_in_proj_bwd(dgb, xb, wb, I, need_dx):
    """dX = dG W_ih and dW_ih = dG^T X with the bf16 operands of _lstm_in_proj (padded columns come back as zeros)."""
    dx = ops.gemm_bf16(dgb, wb, tb=True)[:, :I].contiguous() if need_dx else None
    dw = ops.gemm_bf16(dgb, xb, ta=True, tb=True)[:, :I].contiguous()
    return dx, dw


def _lstm_flag(bf16):
    """The Lstm*Fn precision flag (mfb._lstm_bf16) -> (bf16 operands in the recurrent products, "bf16-all": also in the input
    projection and the weight gradients): False -> (False, False), True -> (True, False), "all" -> (True, True)."""
    return bool(bf16), bf16 == "all"


def _lstm_param_grads(ctx, dg, dgb, hh_bf16):
    """The tail both LSTM nodes' backward share, from the gate gradients dg (S,B,4H) of the whole sequence: dX, dW_ih (bf16
    operands where the forward's input projection had them, ctx.bf16_proj), dW_hh = sum_t dG_t^T h_{t-1} (bf16 operands where the
    node says so, hh_bf16), the bias gradient and its copy for b_hh.  dgb: dg as (S*B, 4H) bf16, or None where neither needs it.
    -> the node's six gradients."""
    x, w_ih, w_hh, hs, _, _, xb, wb = ctx.saved_tensors
    S, B, I = x.shape
    H = w_hh.shape[1]
    dg2 = dg.view(S * B, 4 * H)
    if ctx.bf16_proj:
        dx, dw_ih = _lstm_in_proj_bwd(dgb, xb, wb, I, ctx.needs_input_grad[0])
    else:
        dx = ops.gemm(dg2, _c(w_ih), tb=True) if ctx.needs_input_grad[0] else None
        dw_ih = ops.gemm(dg2, x.view(S * B, I), ta=True, tb=True)
    if S == 1:
        dw_hh = torch.zeros_like(w_hh)
    elif hh_bf16:                        # bf16 modes: the 60-GFLOP recurrent weight gradient takes bf16 operands too
        dw_hh = ops.gemm_bf16(dgb[B:], ops.cast_bf16(hs[:-1].reshape((S - 1) * B, H)), ta=True, tb=True)
    else:
        dw_hh = ops.gemm(dg[1:].reshape((S - 1) * B, 4 * H), hs[:-1].reshape((S - 1) * B, H), ta=True, tb=True)
    db = ops.colsum(dg2) if ctx.has_bias else None
    return (dx.view(S, B, I) if dx is not None else None), dw_ih, dw_hh, db, _copy_of(db), None


class LstmSeqFn(torch.autograd.Function):
    """Single-layer LSTM over dim 0 of x (S,B,I) -> hs (S,B,H), zero initial state.

    For small per-step batches B (MHBCoAtt's batch-axis recursion, mhb_coAtt.py:72-74: S = N, B = T):
    input projection and all weight gradients are MFMA GEMMs over the whole sequence; the recursion
    itself is one fused kernel launch per step (vqf_lstm_seq_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, bf16=False):
        x = _c(x)
        S, B, I = x.shape
        H = w_hh.shape[1]
        bias = _bias_sum(b_ih, b_hh)
        ctx.bf16, all_ = _lstm_flag(bf16)
        ctx.bf16_proj = all_ and H % 8 == 0
        xw, xb, wb = _lstm_in_proj(x.view(S * B, I), w_ih, bias, ctx.bf16_proj)
        xw = xw.view(S, B, 4 * H)
        hs, cs, gates = ops.lstm_seq_fwd(xw, _c(w_hh), bf16=ctx.bf16)
        ctx.save_for_backward(x, w_ih, w_hh, hs, cs, gates, xb, wb)
        ctx.has_bias = b_ih is not None
        return hs

    @staticmethod
    def backward(ctx, dhs):
        _, _, w_hh, _, cs, gates, _, _ = ctx.saved_tensors
        H = w_hh.shape[1]
        dg = ops.lstm_seq_bwd(_c(dhs), gates, cs, _c(w_hh), bf16=ctx.bf16)                # (S,B,4H)
        dgb = ops.cast_bf16(dg.view(-1, 4 * H)) if ctx.bf16 and H % 8 == 0 else None      # one cast serves every bf16 gradient product
        return _lstm_param_grads(ctx, dg, dgb, dgb is not None)


class LstmBatchFn(torch.autograd.Function):
    """Single-layer LSTM over dim 0 of x (T,B,I) -> hs (T,B,H), zero initial state, for LARGE per-step
    batches (the question encoder in its regular orientation, mfb.py:68-70: T = 14 steps of the N-row
    minibatch).  Input projection, the T recurrent products (accumulating into the projection) and all weight
    gradients are MFMA GEMMs; one point-wise kernel per step does the rest (vqf_lstm_cell_fwd / _bwd).
    bf16=True (bf16 mode): the recurrent products take bf16 operands (W_hh cast once, h_t / dG_t per step),
    fp32 accumulation; gates, cell state and every stored tensor stay fp32."""

    FUSED_STEP = True      # fp32: a step's recurrent product and its cell stage in one launch where supported (A/B switch)

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, bf16=False):
        x = _c(x)
        T, B, I = x.shape
        H = w_hh.shape[1]
        bias = _bias_sum(b_ih, b_hh)
        rec, all_ = _lstm_flag(bf16)
        ctx.bf16 = rec and H % 8 == 0
        ctx.bf16_proj = ctx.bf16 and all_
        whh = ops.cast_bf16(_c(w_hh)) if ctx.bf16 else _c(w_hh)
        gates, xb, wb = _lstm_in_proj(x.view(T * B, I), w_ih, bias, ctx.bf16_proj)
        gates = gates.view(T, B, 4 * H)                     # pre-activations -> activated in place
        hs = torch.empty((T, B, H), dtype=torch.float32, device=x.device)
        cs = torch.empty_like(hs)
        fused = LstmBatchFn.FUSED_STEP and not ctx.bf16 and ops.lstm_step_supported(B, H)
        for t in range(T):
            if t > 0 and fused:                 # product + cell in ONE launch (bit-identical to the two below; csrc/gemm_f32_wave.hip)
                ops.lstm_step_fwd(hs[t - 1], whh, gates[t], cs[t - 1], cs[t], hs[t])
                continue
            if t > 0:                                                               # += h_{t-1} W_hh^T
                if ctx.bf16:
                    ops.gemm_bf16(ops.cast_bf16(hs[t - 1]), whh, out=gates[t], accumulate=True)
                else:
                    ops.gemm(hs[t - 1], whh, out=gates[t], accumulate=True)
            ops.lstm_cell_fwd(gates[t], cs[t - 1] if t else None, cs[t], hs[t])
        ctx.save_for_backward(x, w_ih, w_hh, hs, cs, gates, xb, wb)
        ctx.has_bias = b_ih is not None
        return hs

    @staticmethod
    def backward(ctx, dhs):
        x, _, w_hh, _, cs, gates, _, _ = ctx.saved_tensors
        T, B, _ = x.shape
        H = w_hh.shape[1]
        dhs = _c(dhs)
        whh = ops.cast_bf16(_c(w_hh)) if ctx.bf16 else _c(w_hh)
        dG = torch.empty_like(gates)
        dc = torch.empty((B, H), dtype=torch.float32, device=x.device)
        dh = None
        for t in range(T - 1, -1, -1):
            ops.lstm_cell_bwd(dhs[t], dh, gates[t], cs[t], cs[t - 1] if t else None, t == T - 1, dc, dG[t])
            if t > 0:                                                               # dG_t W_hh  (B,H)
                dh = ops.gemm_bf16(ops.cast_bf16(dG[t]), whh, tb=True) if ctx.bf16 else ops.gemm(dG[t], whh, tb=True)
        dGb = ops.cast_bf16(dG.view(T * B, 4 * H)) if ctx.bf16_proj else None
        return _lstm_param_grads(ctx, dG, dGb, ctx.bf16_proj and B % 8 == 0)


class UnitPoolFn(torch.autograd.Function):
    """pooled[n, g*C + c] = sum_s feat[n, s, c] for g < G: the glimpse sums under mfb.py:84,118's
    singleton-axis softmax (weights == 1), without the attention MLP in front (MFB's `pruned` mode).
    layout (None, or the grouping.RegionLayout of an image tensor; fp32 feat): one sum per OWNER of the rows -- per image, (U, G*C),
    where the images are shared -- over its real regions (s < lens_u[u]; packed: feat is (R, C) data, the rows roff gives it)."""

    @staticmethod
    def forward(ctx, feat, G, layout=None):
        feat = _c(feat)
        if layout is not None and layout.packed and (feat.dim() != 2 or ctx.needs_input_grad[0]):
            raise ops._l.VqfError("UnitPoolFn: packed rows are a 2-D feature tensor that is data")
        wts, pooled = _unit_sums(feat, G, layout)
        ctx.save_for_backward(feat, wts)
        ctx.layout = layout
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        feat, wts = ctx.saved_tensors
        _, dfeat = ops.glimpse_pool_bwd(_c(dpooled), feat, wts, True, True, lens=None if ctx.layout is None else ctx.layout.lens_u)
        return dfeat, None, None


class DeadParamsFn(torch.autograd.Function):
    """Identity on `out` that hands EXACT-ZERO gradients to parameters whose contribution is provably
    dead (what the reference's autograd computes for them, the long way round)."""

    @staticmethod
    def forward(ctx, out, *params):
        ctx.meta = [(p.shape, p.dtype, p.device) for p in params]
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        return (g,) + tuple(torch.zeros(sh, dtype=dt, device=dv) for sh, dt, dv in ctx.meta)

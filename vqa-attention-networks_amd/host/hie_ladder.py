"""HieCoAttenLadder: the word / phrase / sentence hierarchical co-attention model (Lu et al. 2016, "Hierarchical
Question-Image Co-Attention for Visual Question Answering") on the HIP path.

The reference has no code for it (its HieCoAtten, host/hieCoAtten.py, is the word level alone); the
equations below are the specification, restated line by line in tests/hie_ladder_ref.py:

    V   = drop(tanh(img_emb(img)))                       (N, L, E)
    Qw  = drop(tanh(word_emb(ids)))                      (N, T, E)
    u_k[t] = b_k + sum_{j<k, t+j<T} W_k[:, :, j] Qw[t+j]  k = 1, 2, 3   (right zero padding)
    Qp  = max_k tanh(u_k)
    Qs  = sent_lstm(Qp)                                  zero initial state, all T outputs
    per level i, Q in (Qw, Qp, Qs):
        C = tanh((Q Wb^T) V^T);  Vh = V Wv^T;  Qh = Q Wq^T
        Hv = tanh(Vh + C^T Qh);  Hq = tanh(Qh + C Vh)
        av_i = softmax_L(Hv whv^T);  aq_i = softmax_T(Hq whq^T)
        v_i = sum_l av_i[l] V[l];  q_i = sum_t aq_i[t] Q[t]
    h_w = tanh(ans_w(drop(q_0 + v_0)));  h_p = tanh(ans_p(drop([q_1 + v_1, h_w])))
    h_s = tanh(ans_s(drop([q_2 + v_2, h_p])));  logits = ans_h(drop(h_s))

`drop` is dropout with rate drop_p in train mode only.

Alternating co-attention (coatt="alternating"; the paper's second mechanism, section 3.3).  The per-level block above becomes
three attention steps, each with its own weights; with A(X, g; Wx, bx, Wg, wh) for X (N, S, E) and g (N, E) or absent:

    Xh = X Wx^T + bx;  H = tanh(Xh + (g Wg^T)[:, None, :])  (absent g: H = tanh(Xh));  a = softmax_S(H wh^T);  x^ = sum_s a[s] X[s]
    per level i, Q in (Qw, Qp, Qs):
        s_i = A(Q, none)          (sum_x, sum_h)                 the question summary
        v_i, av_i = A(V, s_i)     (img_x, img_g, img_h)          the image attended under the summary
        q_i, aq_i = A(Q, v_i)     (que_x, que_g, que_h)          the question attended under the attended image

v_i, q_i, av_i, aq_i feed the same answer MLP; everything before the levels is unchanged.  With q_length the softmax of steps 1
and 3 runs over t < len[n] (exact zeros beyond); Xh of a padded row is bx, not zero, but the row enters nothing: its weight
is an exact zero, and in the backward its dlogit is an exact zero out of vqf_glimpse_pool_bwd_len, so its dXh row, and its part
of dgp and dwh, are zero by arithmetic.  H is never stored (vqf_guided_logits_fwd / _bwd, csrc/hie_ladder_alt.hip).

Question lengths.  forward(img, ids, q_length) -- the call form of the reference's training loop (solver.py:84-89,
model.forward(i, q, q_l)) -- takes the loader's (N,) lengths (data_loader.py:34,45; questions are padded on the right up to
T words, utils.py:185-196).  With valid[n, t] = t < len[n] (len clamped to [1, T] on the device, never read on the host):

    Qw  = valid * drop(tanh(word_emb(ids)))
    u_k[t] = b_k + sum_{j<k, t+j<len[n]} W_k[:, :, j] Qw[t+j]           (the window stops at the real end)
    Qp  = valid * max_k tanh(u_k)
    Qs  = valid * sent_lstm(Qp)                                         (causal: real steps never see padding)
    per level: C[t, :] = 0 for padded t (Cq and Qh have no bias, so zero Q rows give it); aq = softmax over t < len[n] only,
               exactly 0 elsewhere; q_i = sum_{t<len} aq[t] Q[t]; the image side unchanged in form

so a padded batch gives, sample by sample, what the unmasked model gives on that sample alone cut to its own length: the
padding ids do not matter, the padding id's embedding row gets no gradient, and every gradient of a padded row (dQw, dQp,
dQs, dC, dHq, the phrase taps' dZ) is an exact zero.  The lengths ride in the passes that stream these tensors anyway (the
*_len entry points of include/vqa_fusion.h): no extra launch, no torch op on an (N*T, E) or (N, T, L) tensor.  q_length=None
is the unmasked model: a padding id is then an ordinary word of the vocabulary at every level (as in HieCoAtten).

Shared images.  forward(img (U, L, D), ids (N, T), q_length, img_index (N,)) -- VQA asks several questions about each image --
is the model above on img[img_index] with everything question-independent computed once per IMAGE: V = drop(tanh(img_emb(img)))
is (U*L, E) (one dropout mask per image: the questions of an image see the same dropped V), and its gradient is the sum over
the image's questions.  The index is never read on the host: _group_index clamps it to [0, U - 1] and derives, on the device,
order (the questions sorted by image, a stable sort) and grp_off (U + 1 group bounds); the kernels clamp again what they read.
  * alternating mode: the image side STAYS at U -- VX = V [img_x]^T + b is (U*L, 3E), the step-2 passes are the grouped entry
    points (vqf_guided_logits_fwd_grouped / _bwd_grouped, vqf_glimpse_pool_fwd_grouped / _bwd_grouped): a question reads its
    image's rows in the forward, and in the backward a workgroup owns a tile of one image's rows and walks that image's questions
    in `order` (fixed summation order, no atomics, the same bits on every run; an image without a question gets exact zeros).
    No (N*L, .) tensor exists on the image side; the products run on U*L rows.
  * parallel mode: V is computed at U and expanded to (N*L, E) by one row-block gather (vqf_row_block_gather; backward
    vqf_row_block_group_sum, the same fixed-order sum); LadderCoattFn is unchanged.  Sharing Vh and teaching the affinity /
    rank-T streaming kernels the index is out of scope: only img_emb and the tanh / dropout pass are saved there.
img_index=None is the (N, L, D) model, bit for bit: the same code path, no extra launch.

Region counts.  forward((img (N, L, D), img_length (N,)), ids, ...) -- the pair data_loader.pad_region_features builds from
detector-box features, as MFB / MHBCoAtt take it; with img_index the pair is (img (U, L, D), img_length (U,)), one count per
image, and the per-question counts lens_q = lens_u[idx] are one gather on the device.  With rvalid[n, l] = l < len_img[n] (the
counts clamped to [1, L] on the device, never read on the host) the result of sample n is the model on the first len_img[n]
regions of its image alone:
    both modes: av_i = softmax over the real regions, exact zeros elsewhere; v_i sums the real rows; every gradient row of a
        padded region (dV, dVh, dVX) is an exact zero, so img_emb learns nothing from padding, and the padded rows of img may
        hold any finite values without changing an output or gradient bit.
    parallel:   C_i[t, l] = 0 and dC_i[t, l] = 0 for padded l.  dC = (dti Vh^T + Qh dtq^T)(1 - C^2) is NOT zero there by
        arithmetic (dti . Vh[l] != 0): the affinity's epilogue masks it (vqf_hie_affinity_regions / _levels_regions).  Hq, ti,
        dQh and dCq then sum the real regions only: the streaming passes walk min(chunk end, count) rows, read nothing behind
        the count and store zero Hv / dVh rows there (vqf_hie_hv_fwd_regions, _rank_add_regions, _rank_left_regions), so the
        image-side traffic of the affinity and rank-T passes goes with sum(counts) instead of N L.  T > 16 (batched GEMMs):
        vqf_zero_cols_len on C after the tanh and on dC; nothing else on that route needs the counts but the pooling.
    alternating: only step 2's pooling changes (vqf_glimpse_pool_fwd_len / _bwd_len; with img_index the _grouped_len forms with
        lens_q); the guided-logits backward gives a zero dXh row for a zero dlogits row.  Host wiring, no kernel of its own.
q_length, img_index, coatt and img_length combine freely.  Dropout masks, explicit or Philox, keep their element indices
(row, col) over the padded (. * L, E) tensor: the masks of real elements do not depend on the counts.  The img_emb / Vh / VX
products and the logit heads run on all rows; their padded results are never used.  A plain tensor or (img, None) is the
model without counts, bit for bit: no extra launch, the same code route.

Packed regions.  forward(PackedRegions(rows (R, D), offsets, max_regions = L), ids, ...) -- what data_loader.pack_region_features builds:
every image's real regions, never padded; offsets (N + 1,), or (U + 1,) per image with img_index -- is, by definition, the model on
(packed.unpack(), ids, ...): the region-count call above.  img_emb runs on the R real rows (so does its weight gradient), and the
tanh / dropout pass that follows anyway is where the layout changes: vqf_tanh_dropout_unpack_fwd reads (R, E) and writes V as
(U*L, E) with exact zero rows behind each count, its backward (vqf_tanh_dropout_pack_bwd) returns dZ (R, E) without reading a padded
row -- as many launches as the pair call, no extra pass over an (N*L, .) tensor.  Dropout indices stay those of the padded tensor
(set_keep_masks(img=...) stays (U*L, E)); the counts are offsets[1:] - offsets[:-1] through the same clamp as img_length, and from V
on the code is that of the region-count call (RegionLayout.padded(): the same layout with counts in place of the offsets; the
*_regions / *_len kernels, RowBlockGatherFn and the grouping).  offsets is never read
on the host; the kernels clamp what it holds (include/vqa_fusion.h).  The Vh / VX products, the affinity and the rank-T passes stay
padded (N*L rows), as in the region-count call; fp32 only.

Packed co-attention rows.  HieCoAttenLadder(coatt="alternating", packed_coatt=True) -- opt-in, default off -- keeps the whole image
side of the alternating levels on the R real rows when it is handed a PackedRegions: V stays (R, E) (vqf_tanh_dropout_packed_fwd /
_bwd: both sides packed, the masks still those of the padded (U*L, E) tensor), VX = V [img_x]^T + b and dVX are (R, 3E), step 2 runs on
vqf_guided_logits_fwd_packed / _bwd_packed and vqf_glimpse_pool_fwd_packed / _bwd_packed_dfeat (their grouped forms with img_index),
dV is (R, E), and dV += dVX wimg and dwimg = dVX^T V are products on R rows.  The result is still, by definition, the model on
(packed.unpack(), ...): av (N, 3, L) with exact zeros behind each count, the same parameters and state_dict, offsets never read on
the host.  Against packed_coatt=False only the summation order of dwimg (and of the products' K splits) differs, so the two agree
to rounding, not bit for bit.  What stays padded or untouched: the question side (QX and everything over (N*T, .)), parallel mode
(its Vh product, affinity and rank-T passes: packed_coatt=True raises ValueError there), bf16, and the HieCoAtten class.  With a
plain tensor or the pair the keyword changes nothing: the same code path, bit for bit.

Where the image rows are -- the index, the counts, the offsets of the four paragraphs above -- travels from forward() to the nodes
as ONE grouping.RegionLayout, made by mfb.region_layout with every refusal of the call form; padded() and per_question() follow V
through the unpacking pass and the row-block gather, and functions._guided_fwd / _pool_fwd (and their backwards) pick step 2's kernels.

Stages (every product and every pass over an (N*L, .) or (N*T, .) tensor runs in libvqa_fusion.so):
  * img_emb / word embedding: LinearFn + TanhDropFn, EmbedTanhFn + DropoutFn;
  * phrase level (PhraseFn): the six conv taps as one GEMM, then vqf_phrase_ngram_fwd / _bwd (csrc/hie_ladder.hip);
  * sentence level: LstmBatchFn, its (N, T) <-> (T, N) re-layouts in DropoutBTFn passes at rate 0;
  * the three co-attention levels (LadderCoattFn): one Vh product for all levels, one multi-level affinity pass over V
    (vqf_hie_affinity_levels), the streaming Hv / Hq passes of csrc/hie.hip per level on column blocks, one G = 3 image-side
    pooling over V;
  * alternating mode (LadderAltCoattFn) instead: one product V [img_x_0; img_x_1; img_x_2]^T, one product per level
    Q_i [sum_x_i; que_x_i]^T, the guided-logits passes (one G = 3 launch over the image rows, one launch per level and step
    over the question rows), the same pooling kernels, (N, E) products for the guidance rows;
  * the answer MLP: LinearFn, TanhDropFn, DropoutFn; torch does its O(N E) adds and concatenations.
"""
import torch
import torch.nn as nn

from . import ops
from .functions import (_c, _hie_hv_ti, _hie_dc, _hie_bwd_bgemm, _guided_fwd, _guided_bwd, _pool_fwd, _pool_bwd, EmbedTanhFn, LinearFn,
                        DropoutFn, TanhDropFn, TanhDropUnpackFn, TanhDropPackedFn, DropoutBTFn, LstmBatchFn)
from .grouping import _group_index, PackedRegions    # (importable from here as before)
from .lib import VqfError
from .mfb import _DropSeeds, region_layout

_NODROP = (None, 0, 0.0)


class PhraseFn(torch.autograd.Function):
    """Qp = max_k tanh(conv_k(Qw) + b_k) over the n-gram sizes k = 1, 2, 3 (right zero padding).  qw (N*T, E) contiguous;
    w_k (E, E, k), b_k (E) the nn.Conv1d parameters.  Forward: Z = qw Wcat^T with the six taps stacked (one GEMM), then one
    streaming pass (vqf_phrase_ngram_fwd) that also records the winning k.  Backward: dZ gathered from the winners
    (vqf_phrase_ngram_bwd), dqw and dWcat as GEMMs, the bias gradients as column sums of dZ.
    lens ((N,) int32 or None): the windows stop at lens[n], padded rows of Qp and of dZ are zero (the *_len kernels)."""

    @staticmethod
    def forward(ctx, qw, w1, b1, w2, b2, w3, b3, N, T, lens=None):
        E = qw.shape[1]
        wcat = torch.cat([w1[:, :, 0], w2[:, :, 0], w2[:, :, 1], w3[:, :, 0], w3[:, :, 1], w3[:, :, 2]], 0).contiguous()
        bcat = torch.cat([b1, b2, b3], 0).contiguous()
        Z = ops.gemm(qw, wcat)                                     # (N*T, 6E)
        qp, idx = ops.phrase_ngram_fwd(Z, bcat, N, T, lens=lens)
        ctx.save_for_backward(qw, wcat, qp, idx)
        ctx.dims, ctx.lens = (N, T, E), lens
        return qp

    @staticmethod
    def backward(ctx, dqp):
        qw, wcat, qp, idx = ctx.saved_tensors
        N, T, E = ctx.dims
        dZ = ops.phrase_ngram_bwd(_c(dqp), qp, idx, N, T, lens=ctx.lens)
        dqw = ops.gemm(dZ, wcat, tb=True)                         # (N*T, E)
        dW = ops.gemm(dZ, qw, ta=True, tb=True)                   # (6E, E)
        db = ops.colsum(dZ)
        dw1 = dW[:E].unsqueeze(2).contiguous()
        dw2 = torch.stack([dW[E:2 * E], dW[2 * E:3 * E]], 2)
        dw3 = torch.stack([dW[3 * E:4 * E], dW[4 * E:5 * E], dW[5 * E:6 * E]], 2)
        return dqw, dw1, db[:E], dw2, db[E:2 * E], dw3, db[3 * E:4 * E], None, None, None


class RowBlockGatherFn(torch.autograd.Function):
    """(U*L, E) -> (N*L, E): question n's rows are image idx[n]'s (vqf_row_block_gather); backward: the sum over each image's
    questions in `order` (vqf_row_block_group_sum; zeros for an image without a question)."""

    @staticmethod
    def forward(ctx, V, idx, order, grp_off, L):
        U, E = V.shape[0] // L, V.shape[1]
        ctx.save_for_backward(order, grp_off)
        ctx.dims = (U, L, E)
        return ops.row_block_gather(V.view(U, L * E), idx).view(idx.shape[0] * L, E)

    @staticmethod
    def backward(ctx, dV):
        order, grp_off = ctx.saved_tensors
        U, L, E = ctx.dims
        return ops.row_block_group_sum(_c(dV).view(order.shape[0], L * E), order, grp_off).view(U * L, E), None, None, None, None


class LadderCoattFn(torch.autograd.Function):
    """The three parallel co-attention levels over ONE image tensor.  V (N*L, E), q0 / q1 / q2 (N*T, E) contiguous;
    weights: for each level (Wb, Wv, Wq (E, E), whv, whq (1, E)).  Returns (vcat (N, 3E) = [v_0 | v_1 | v_2], q_0, q_1, q_2
    (N, E), av (N, 3, L), aq_0, aq_1, aq_2 (N, 1, T)).

    Forward: Vh = V [Wv_0; Wv_1; Wv_2]^T (one product, (N*L, 3E)); [Cq_i | Qh_i] = Q_i [Wb_i; Wq_i]^T into one (N*T, 6E)
    buffer; C_i = tanh(Cq_i V^T) for the three levels in one pass over V (vqf_hie_affinity_levels); per level Hv_i and the
    T-row sums ti_i = C_i Vh_i in one streaming pass over Vh_i (vqf_hie_hv_fwd), Hq_i = tanh(Qh_i + ti_i); the image-side
    logits of all levels with a block-diagonal (3, 3E) weight and ONE G = 3 pooling pass over V.  Where the streaming
    passes do not take the shape (T > 16) the T-row products run on the batched GEMM and the element-wise kernels.
    Backward: the same stages in reverse; dC_i = (dti_i Vh_i^T + Qh_i dtq_i^T)(1 - C_i^2) in one affinity pass (all levels
    in one launch where the LDS holds them, one launch per level otherwise).
    lens ((N,) int32 or None; q0 / q1 / q2 come with zero rows at t >= lens[n]): the question-side poolings take the softmax
    over the real words, and the dC stage writes zero rows for the padded ones on every route -- with those, every other
    stage's padded rows are zero by its own arithmetic (bias-free products of zero rows, tanh(0) = 0).
    layout (the grouping.RegionLayout of V: one image per question here, so only its counts matter; rlens below = layout.lens_q,
    (N,) int32 or None: the real regions of each sample's L; V's padded rows hold finite values that must not matter):
    the *_regions forms of the affinity and of the streaming passes -- zero columns of C and dC, zero rows of Hv and dVh behind
    the count, nothing read there -- and the image-side pooling over the real regions (vqf_glimpse_pool_fwd_len / _bwd_len);
    on the batched-GEMM route vqf_zero_cols_len on C and dC, which makes every other padded term a product with an exact zero."""

    STREAM = True      # the T-row stages as streaming passes where supported; False: batched GEMMs + element-wise (A/B)

    @staticmethod
    def forward(ctx, V, q0, q1, q2, N, L, T, lens, layout, *w):
        E = V.shape[1]
        rlens = layout.lens_q
        lk = {} if lens is None else {"lens": lens}
        rk = {} if rlens is None else {"rlens": rlens}
        M, MT = N * L, N * T
        dev = V.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        Q = (q0, q1, q2)
        Wb, Wv, Wq, whv, whq = ([_c(w[5 * g + i]) for g in range(3)] for i in range(5))
        wv_cat = torch.cat(Wv, 0).contiguous()                                      # (3E, E)
        wq2 = [torch.cat([Wb[g], Wq[g]], 0).contiguous() for g in range(3)]         # (2E, E) each
        wblk = torch.zeros((3, 3 * E), dtype=torch.float32, device=dev)             # block-diagonal head weight
        for g in range(3):
            wblk[g, g * E:(g + 1) * E] = whv[g].view(E)
        zb3, zb1 = torch.zeros(3, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
        Vh = ops.gemm_rows(V, wv_cat, L)                                            # (M, 3E) = [Vh_0 | Vh_1 | Vh_2]
        CQ = new(MT, 6 * E)                                                         # [Cq_0 | Qh_0 | Cq_1 | Qh_1 | Cq_2 | Qh_2]
        for g in range(3):
            ops.gemm(Q[g], wq2[g], out=CQ[:, 2 * g * E:(2 * g + 2) * E])
        stream = LadderCoattFn.STREAM and ops.hie_stream_supported(N, L, E, T)
        if stream and ops.hie_affinity_levels_supported(N, L, E, T, 3, 1):
            C = ops.hie_affinity_levels(CQ, 2 * E, V, 0, 3, N, L, T, E, epi=1, **rk)      # (3, N, T, L), V read once
        else:
            C = new(3, N, T, L)
            for g in range(3):
                ops.bgemm(CQ[:, 2 * g * E:(2 * g + 1) * E].view(N, T, E), V.view(N, L, E), out=C[g])
            ops.tanh_dropout_fwd(C.view(3 * MT, L), None, *_NODROP, out=C.view(3 * MT, L))
            if rlens is not None:
                ops.zero_cols_len(C, rlens, T, N, L)
        Hv = new(M, 3 * E)
        Hq = new(3, MT, E)                                                          # ti_i first, then Hq_i in place
        for g in range(3):
            Qh_g, ti_g = CQ[:, (2 * g + 1) * E:(2 * g + 2) * E], Hq[g]
            _hie_hv_ti(Vh[:, g * E:(g + 1) * E], C[g], Qh_g, _NODROP, N, L, T, Hv[:, g * E:(g + 1) * E], ti_g, stream, **rk)
            ops.tanh_dropout_fwd2d(Qh_g, ti_g, *_NODROP, out=ti_g)
        av, vcat = ops.glimpse_pool_fwd(V.view(N, L, E), ops.att_logits_fwd(Hv, wblk, zb3), False,
                                        **({} if rlens is None else {"lens": rlens}))                 # (N, 3, L), (N, 3E)
        aq, qo = [], []
        for g in range(3):
            a_g, q_g = ops.glimpse_pool_fwd(Q[g].view(N, T, E), ops.att_logits_fwd(Hq[g], whq[g], zb1), False, **lk)
            aq.append(a_g)
            qo.append(q_g)
        ctx.save_for_backward(V, q0, q1, q2, wv_cat, wq2[0], wq2[1], wq2[2], wblk, whq[0], whq[1], whq[2], Vh, CQ, C, Hv, Hq, av,
                              aq[0], aq[1], aq[2])
        ctx.dims, ctx.stream, ctx.lens, ctx.rlens = (N, L, T, E), stream, lens, rlens
        ctx.set_materialize_grads(False)
        return (vcat, qo[0], qo[1], qo[2], av, aq[0], aq[1], aq[2])

    @staticmethod
    def backward(ctx, dvcat, dq0, dq1, dq2, dav, daq0, daq1, daq2):
        (V, q0, q1, q2, wv_cat, wq0, wq1, wq2_, wblk, whq0, whq1, whq2, Vh, CQ, C, Hv, Hq, av, aq0, aq1, aq2) = ctx.saved_tensors
        N, L, T, E = ctx.dims
        M, MT = N * L, N * T
        dev = V.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        Q, wq2, whq, aq = (q0, q1, q2), (wq0, wq1, wq2_), (whq0, whq1, whq2), (aq0, aq1, aq2)
        dq, daq = (dq0, dq1, dq2), (daq0, daq1, daq2)
        stream, lens, rlens = ctx.stream, ctx.lens, ctx.rlens
        lk = {} if lens is None else {"lens": lens}
        rk = {} if rlens is None else {"rlens": rlens}
        dCQ = new(MT, 6 * E)                                                        # [dCq_0 | dQh_0 | ...]
        dti = new(MT, 3 * E)
        dQ, dwhq = [], []
        # question side: q_i = aq_i^T Q_i, aq_i = softmax(whq_i Hq_i), Hq_i = tanh(Qh_i + ti_i)
        for g in range(3):
            dqg = _c(dq[g]) if dq[g] is not None else zeros(N, E)
            dl, dQg = ops.glimpse_pool_bwd(dqg, Q[g].view(N, T, E), aq[g], False, True,
                                           dwts=None if daq[g] is None else _c(daq[g]), **lk)
            dHq, dw, _, _ = ops.att_logits_bwd(dl, Hq[g], whq[g], relu_mask=False)
            ops.tanh_dropout_bwd2d(dHq, Hq[g], *_NODROP, out=dti[:, g * E:(g + 1) * E])   # d(Qh_i + ti_i)
            if not stream:
                ops.tanh_dropout_bwd2d(dHq, Hq[g], *_NODROP, out=dCQ[:, (2 * g + 1) * E:(2 * g + 2) * E])
            dQ.append(dQg.view(MT, E))
            dwhq.append(dw)
        # image side: one G = 3 pooling backward over V, the block-diagonal head, Hv_i = tanh(Vh_i + tq_i)
        dvc = _c(dvcat) if dvcat is not None else zeros(N, 3 * E)
        dlv, dV = ops.glimpse_pool_bwd(dvc, V.view(N, L, E), av, False, True, dwts=None if dav is None else _c(dav),
                                       **({} if rlens is None else {"lens": rlens}))
        dV = dV.view(M, E)
        dHv, dwblk, _, _ = ops.att_logits_bwd(dlv, Hv, wblk, relu_mask=False)
        dVh = ops.tanh_dropout_bwd2d(dHv, Hv, *_NODROP, out=dHv)                   # dtq_i = d(Vh_i + tq_i); dVh_i below
        dC = new(3, N, T, L)
        if stream and ops.hie_affinity_levels_supported(N, L, E, T, 3, 2):
            ops.hie_affinity_levels(dti, E, Vh, E, 3, N, L, T, E, x2=CQ[:, E:], lvx2=2 * E, y2=dVh, lvy2=E, epi=2, yprev=C, out=dC,
                                    **lk, **rk)
        else:                      # per level (E = 512: three levels x two pairs exceed the LDS: one two-pair launch each)
            aff = stream and ops.hie_affinity_supported(N, L, E, T, 2)
            for g in range(3):
                _hie_dc(dti[:, g * E:(g + 1) * E], Vh[:, g * E:(g + 1) * E], CQ[:, (2 * g + 1) * E:(2 * g + 2) * E],
                        dVh[:, g * E:(g + 1) * E], C[g], _NODROP, N, L, T, aff, out=dC[g], **lk, **rk)
        if stream:
            S = ops.hie_chunks(N, L)
            part, scratch = new(S, MT, E), new(M, E)
        for g in range(3):
            cq_g, qh_g = CQ[:, 2 * g * E:(2 * g + 1) * E], CQ[:, (2 * g + 1) * E:(2 * g + 2) * E]
            dcq_g, dqh_g = dCQ[:, 2 * g * E:(2 * g + 1) * E], dCQ[:, (2 * g + 1) * E:(2 * g + 2) * E]
            dti_g, dtq_g = dti[:, g * E:(g + 1) * E], dVh[:, g * E:(g + 1) * E]
            if stream:
                ops.hie_rank_left(C[g], dti_g, dtq_g, N, L, T, scratch, part, **rk)  # C dtq (the T-row sums)
                ops.hie_slab_sum(part, dqh_g, add=dti_g)                            # dQh = dti + C dtq
                ops.hie_rank_add(dtq_g, C[g], dti_g, N, L, T, dtq_g, **rk)          # dVh = dtq + C^T dti   (in place)
                ops.hie_rank_left(dC[g], cq_g, V, N, L, T, scratch, part, **rk)     # dCq = dC V  (T-row sums over V)
                ops.hie_slab_sum(part, dcq_g)
                ops.hie_rank_add(dV, dC[g], cq_g, N, L, T, dV, **rk)                # dV += dC^T Cq   (in place)
            else:
                _hie_bwd_bgemm(C[g], dC[g], dti_g, dtq_g, V, cq_g, dqh_g, dcq_g, dV, N, L, T, True)
        # the concatenated layers: dV += dVh [Wv_0; Wv_1; Wv_2], one weight-gradient product; per level the [Wb; Wq] pair
        ops.gemm(dVh, wv_cat, tb=True, out=dV, accumulate=True)
        dwv = ops.gemm(dVh, V, ta=True, tb=True)                                   # (3E, E)
        grads = []
        for g in range(3):
            blk = dCQ[:, 2 * g * E:(2 * g + 2) * E]
            ops.gemm(blk, wq2[g], tb=True, out=dQ[g], accumulate=True)
            dwq2 = ops.gemm(blk, Q[g], ta=True, tb=True)                           # (2E, E) = [dWb; dWq]
            grads += [dwq2[:E], dwv[g * E:(g + 1) * E], dwq2[E:], dwblk[g:g + 1, g * E:(g + 1) * E].contiguous(), dwhq[g]]
        return (dV, dQ[0], dQ[1], dQ[2], None, None, None, None, None, *grads)


class LadderAltCoattFn(torch.autograd.Function):
    """The three alternating co-attention levels over ONE image tensor (the module docstring's A steps).  V (N*L, E),
    q0 / q1 / q2 (N*T, E) contiguous; weights: for each level (sum_x.weight (E, E), sum_x.bias (E), sum_h.weight (1, E),
    img_x.weight, img_x.bias, img_g.weight (E, E), img_h.weight, que_x.weight, que_x.bias, que_g.weight, que_h.weight).
    Returns what LadderCoattFn returns: (vcat (N, 3E), q_0, q_1, q_2 (N, E), av (N, 3, L), aq_0, aq_1, aq_2 (N, 1, T)).

    Forward: VX = V [img_x_0; img_x_1; img_x_2]^T + b (one product, (N*L, 3E)); [sum_i | que_i] = Q_i [sum_x_i; que_x_i]^T + b
    into one (N*T, 6E) buffer; step 1 per level: guided logits without guidance over the sum_i block, pooling over Q_i -> s_i;
    step 2: the guidance rows s_i img_g_i^T (N, 3E), ONE G = 3 guided-logits pass over VX and ONE G = 3 pooling pass over V;
    step 3 per level: v_i que_g_i^T, guided logits over the que_i block, pooling over Q_i.
    Backward: step 3 -> step 2 -> step 1 through the guidance-row gradients dgp; the guided-logits backward writes dXh straight
    into the (N*T, 6E) / (N*L, 3E) operands of the weight- and input-gradient products; the bias gradients are column sums of
    the (N, .) dgp.  lens ((N,) int32 or None; q0 / q1 / q2 come with zero rows at t >= lens[n]): the question-side poolings
    take the softmax over the real words and give zero dlogits for the padded ones.
    layout (the grouping.RegionLayout of V; step 2 runs on functions._guided_fwd / _pool_fwd and their backwards, which pick the
    kernels).  Region counts: step 2's pooling runs over the real regions (the question's count lens_q = lens_u[idx] where the images
    are shared); its zero dlogits rows give zero dVX rows out of the guided-logits backward.  Host wiring only: no kernel of this
    mode knows the counts but the pooling.  Shared images: V is (U*L, E) -- VX stays (U*L, 3E), step 2 runs on the grouped entry
    points (question n reads image idx[n]'s rows; dV and dVX sum each image's questions in `order`).  Packed rows
    (HieCoAttenLadder(packed_coatt=True)): the image side on the PACKED rows -- V is (R, E), VX = V [img_x]^T + b and dVX are (R, 3E),
    dV is (R, E); step 2 runs on the packed entry points (their grouped forms where the images are shared), which take the counts
    from roff; av stays (N, 3, L) with exact zeros behind each count.  The dV += dVX wimg and dwimg products run on R rows."""

    PER_LEVEL = 11

    @staticmethod
    def forward(ctx, V, q0, q1, q2, N, L, T, lens, layout, *w):
        E = V.shape[1]
        lk = {} if lens is None else {"lens": lens}
        Vf = V if layout.packed else V.view(layout.U, L, E)                         # what step 2's pooling reads
        MT = N * T
        dev = V.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        Q = (q0, q1, q2)
        (sum_x, sum_b, sum_h, img_x, img_b, img_g, img_h, que_x, que_b, que_g, que_h) = \
            ([_c(w[LadderAltCoattFn.PER_LEVEL * g + i]) for g in range(3)] for i in range(LadderAltCoattFn.PER_LEVEL))
        wimg = torch.cat(img_x, 0).contiguous()                                     # (3E, E)
        bimg = torch.cat(img_b, 0).contiguous()
        whimg = torch.cat(img_h, 0).contiguous()                                    # (3, E)
        wq2 = [torch.cat([sum_x[g], que_x[g]], 0).contiguous() for g in range(3)]   # (2E, E) each
        bq2 = [torch.cat([sum_b[g], que_b[g]], 0).contiguous() for g in range(3)]
        if layout.packed:
            VX = ops.gemm(V, wimg, bias=bimg)                                       # (R, 3E): the real rows only
        else:
            VX = ops.gemm_rows(V, wimg, L, bias=bimg)                               # (U*L, 3E) = [img_0 | img_1 | img_2]
        QX = new(MT, 6 * E)                                                         # [sum_0 | que_0 | sum_1 | que_1 | sum_2 | que_2]
        for g in range(3):
            ops.gemm(Q[g], wq2[g], bias=bq2[g], out=QX[:, 2 * g * E:(2 * g + 2) * E])
        # step 1: the question summaries
        asum, s = [], []
        for g in range(3):
            lg = ops.guided_logits_fwd(QX[:, 2 * g * E:(2 * g + 1) * E], None, sum_h[g], N, T)
            a_g, s_g = ops.glimpse_pool_fwd(Q[g].view(N, T, E), lg, False, **lk)
            asum.append(a_g)
            s.append(s_g)
        # step 2: the image under the summaries, all levels in one pass over VX and one over V
        gpv = new(N, 3 * E)
        for g in range(3):
            ops.gemm(s[g], img_g[g], out=gpv[:, g * E:(g + 1) * E])
        av, vcat = _pool_fwd(Vf, _guided_fwd(VX, gpv, whimg, layout, N, L), False, layout)               # (N, 3, L), (N, 3E)
        # step 3: the question under the attended image
        gpq = new(3, N, E)
        aq, qo = [], []
        for g in range(3):
            ops.gemm(vcat[:, g * E:(g + 1) * E], que_g[g], out=gpq[g])
            lg = ops.guided_logits_fwd(QX[:, (2 * g + 1) * E:(2 * g + 2) * E], gpq[g], que_h[g], N, T)
            a_g, q_g = ops.glimpse_pool_fwd(Q[g].view(N, T, E), lg, False, **lk)
            aq.append(a_g)
            qo.append(q_g)
        ctx.save_for_backward(V, q0, q1, q2, wimg, whimg, VX, QX, gpv, gpq, vcat, av, *wq2, *sum_h, *img_g, *que_g, *que_h, *s, *asum,
                              *aq)
        ctx.dims, ctx.lens, ctx.layout = (N, L, T, E), lens, layout
        ctx.set_materialize_grads(False)
        return (vcat, qo[0], qo[1], qo[2], av, aq[0], aq[1], aq[2])

    @staticmethod
    def backward(ctx, dvcat, dq0, dq1, dq2, dav, daq0, daq1, daq2):
        t = ctx.saved_tensors
        V, q0, q1, q2, wimg, whimg, VX, QX, gpv, gpq, vcat, av = t[:12]
        wq2, sum_h, img_g, que_g, que_h, s, asum, aq = (t[12 + 3 * i:15 + 3 * i] for i in range(8))
        N, L, T, E = ctx.dims
        layout = ctx.layout
        Vf = V if layout.packed else V.view(layout.U, L, E)
        MT = N * T
        dev = V.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        Q, dq, daq = (q0, q1, q2), (dq0, dq1, dq2), (daq0, daq1, daq2)
        lens = ctx.lens
        lk = {} if lens is None else {"lens": lens}
        dQX = new(MT, 6 * E)                                                       # [dsum_0 | dque_0 | ...]
        dvc = dvcat.clone(memory_format=torch.contiguous_format) if dvcat is not None else zeros(N, 3 * E)               # dv_i: the answer MLP's plus step 3's
        dQ, g3 = [], []
        # step 3: q_i = aq_i^T Q_i, aq_i = softmax(que_h_i tanh(que_i + v_i que_g_i^T))
        for g in range(3):
            blk = slice(g * E, (g + 1) * E)
            dqg = _c(dq[g]) if dq[g] is not None else zeros(N, E)
            dl, dQg = ops.glimpse_pool_bwd(dqg, Q[g].view(N, T, E), aq[g], False, True,
                                           dwts=None if daq[g] is None else _c(daq[g]), **lk)
            _, dgp, dwh = ops.guided_logits_bwd(dl, QX[:, (2 * g + 1) * E:(2 * g + 2) * E], gpq[g], que_h[g], N, T,
                                                out=dQX[:, (2 * g + 1) * E:(2 * g + 2) * E])
            ops.gemm(dgp, que_g[g], tb=True, out=dvc[:, blk], accumulate=True)      # dv_i += dgp que_g_i
            g3.append((ops.colsum(dgp), ops.gemm(dgp, vcat[:, blk], ta=True, tb=True), dwh))   # que_x.bias, que_g, que_h
            dQ.append(dQg.view(MT, E))
        # step 2: one G = 3 pooling backward over V, one G = 3 guided-logits backward over VX
        # (dV and dVX come back in V's and VX's layout: packed rows, or each shared image's questions summed in `order`)
        dlv, dV = _pool_bwd(dvc, Vf, av, False, True, layout, dwts=None if dav is None else _c(dav))
        dVX, dgpv, dwhimg = _guided_bwd(dlv, VX, gpv, whimg, layout, N, L)
        dV = dV.view(V.shape[0], E)
        dbimg = ops.colsum(dgpv)
        ops.gemm(dVX, wimg, tb=True, out=dV, accumulate=True)                      # dV += dVX [img_x_0; img_x_1; img_x_2]
        dwimg = ops.gemm(dVX, V, ta=True, tb=True)                                 # (3E, E)
        # step 1: s_i = asum_i^T Q_i; then the [sum_x_i; que_x_i] pair's products
        grads, dQ1 = [], []
        for g in range(3):
            blk = slice(g * E, (g + 1) * E)
            ds = ops.gemm(dgpv[:, blk], img_g[g], tb=True)                          # (N, E)
            dimg_g = ops.gemm(dgpv[:, blk], s[g], ta=True, tb=True)
            dl, dQ1g = ops.glimpse_pool_bwd(ds, Q[g].view(N, T, E), asum[g], False, True, **lk)
            _, dgp, dwsum_h = ops.guided_logits_bwd(dl, QX[:, 2 * g * E:(2 * g + 1) * E], None, sum_h[g], N, T,
                                                    out=dQX[:, 2 * g * E:(2 * g + 1) * E])
            pair = dQX[:, 2 * g * E:(2 * g + 2) * E]
            ops.gemm(pair, wq2[g], tb=True, out=dQ[g], accumulate=True)
            dwq2 = ops.gemm(pair, Q[g], ta=True, tb=True)                           # (2E, E) = [dsum_x; dque_x]
            dQ1.append(dQ1g.view(MT, E))
            grads += [dwq2[:E], ops.colsum(dgp), dwsum_h, dwimg[blk], dbimg[blk], dimg_g, dwhimg[g:g + 1], dwq2[E:], g3[g][0],
                      g3[g][1], g3[g][2]]
        ops.multi_add([(dQ[g], dQ1[g], dQ[g]) for g in range(3)])                   # dQ_i: step 3's + the pair's + step 1's
        return (dV, dQ[0], dQ[1], dQ[2], None, None, None, None, None, *grads)


class _Coatt(nn.Module):
    """One level's co-attention weights (no biases: a bias inside the softmax cancels, and Wb / Wv / Wq are bias-free)."""

    def __init__(self, E):
        super(_Coatt, self).__init__()
        self.Wb = nn.Linear(E, E, bias=False)
        self.Wv = nn.Linear(E, E, bias=False)
        self.Wq = nn.Linear(E, E, bias=False)
        self.whv = nn.Linear(E, 1, bias=False)
        self.whq = nn.Linear(E, 1, bias=False)


class _CoattAlt(nn.Module):
    """One level's alternating co-attention weights: the three attention steps (question summary, image, question), each a
    projection with a bias (*_x), a bias-free guidance projection (*_g; the summary step has no guidance) and a head (*_h; a
    bias inside the softmax cancels)."""

    def __init__(self, E):
        super(_CoattAlt, self).__init__()
        self.sum_x = nn.Linear(E, E)
        self.sum_h = nn.Linear(E, 1, bias=False)
        self.img_x = nn.Linear(E, E)
        self.img_g = nn.Linear(E, E, bias=False)
        self.img_h = nn.Linear(E, 1, bias=False)
        self.que_x = nn.Linear(E, E)
        self.que_g = nn.Linear(E, E, bias=False)
        self.que_h = nn.Linear(E, 1, bias=False)


COATT_MODES = ("parallel", "alternating")


class HieCoAttenLadder(nn.Module):
    """forward(img_features (N, L, img_size) fp32 GPU, que_features (N, T) int64 GPU, q_length=None, img_index=None)
    -> (logits (N, output_size), av (N, 3, L), aq (N, 3, T)); levels ordered word, phrase, sentence.

    img_index: (N,) int64 or int32 on the questions' device; img_features is then (U, L, img_size) for any U >= 1 and question n
    looks at image img_index[n] (any order, repeated indices, images without a question, N < U and N > U).  Values are clamped
    to [0, U - 1] on the device; the index is never read on the host.  The question-independent image work runs once per image
    (module docstring, "Shared images"); in train mode the 'img' dropout mask is drawn once per image, over (U*L, E): the
    questions of one image see the same dropped V.  In parallel mode only img_emb and its tanh / dropout pass are shared
    (sharing Vh and the affinity / rank-T passes is out of scope).  None: today's (N, L, img_size) model, bit for bit.

    q_length: (N,) int64 or int32 on the same GPU, the real words of each right-padded question (the loader's q_l; the
    reference's training loop calls model.forward(i, q, q_l)).  Padding is then masked at every level: the result of a sample
    does not depend on the pad width or the padding ids, aq has exact zeros at the padded positions, the padding id's embedding
    row gets no gradient.  Values are clamped to [1, T] on the device; the lengths are never read on the host.  None: no masking
    (every id is a word), bit for bit the two-argument model.

    coatt: "parallel" (the default: the affinity form of the module docstring) or "alternating" (the paper's alternating
    co-attention: question summary -> image attention -> question attention per level; self.coatt then holds three modules
    with sum_x, sum_h, img_x, img_g, img_h, que_x, que_g, que_h).  Anything else raises ValueError; coatt_mode holds the string.
    Inputs, outputs, masking and the dropout sites are the same in both modes.

    img_features may be the pair (img, img_length): img_length (N,) -- (U,) with img_index, one count per image -- int64 or int32
    on the questions' device, the real regions of each right-padded image (data_loader.pad_region_features).  Padded regions
    are then masked at every level (module docstring, "Region counts"): av has exact zeros there, the padded rows of img may
    hold any finite values.  Values are clamped to [1, L] on the device and never read on the host.  A tensor or (img, None):
    no masking, bit for bit today's model.  A pair of another arity, counts of a wrong dtype, shape or device raise VqfError.

    img_features may be a PackedRegions(rows (R, img_size), offsets, max_regions) (grouping.PackedRegions; what
    data_loader.pack_region_features builds): the real regions of every image, never padded; offsets (N + 1,) -- (U + 1,) with
    img_index -- int64 or int32 on the questions' device, never read on the host; max_regions a Python int L in [1, 1024].  The
    result is this model on (packed.unpack(), ...), the pair call, with av (N, 3, L) and exact zeros behind each count; img_emb
    and its weight gradient run on the R real rows (module docstring, "Packed regions").  A malformed object, rows on another
    device or of another channel count, more than 65535 images or R >= 2^29 raise VqfError before the first launch.

    packed_coatt (constructor keyword, default False; stored as self.packed_coatt): True keeps the image side of the ALTERNATING
    levels on the R packed rows when forward is handed a PackedRegions (V, VX = V [img_x]^T + b, dVX and dV have R rows; module
    docstring, "Packed co-attention rows").  It is the same model -- the same parameters and state_dict, av (N, 3, L) with exact
    zeros behind each count, set_keep_masks(img=...) still (U*L, E) -- and agrees with False to rounding (the dwimg sum runs over R
    rows instead of U*L).  With a plain tensor or the pair it changes nothing, bit for bit.  True with coatt="parallel" raises
    ValueError at construction: there is nothing to keep packed there.  Shapes outside vqf_guided_logits_packed_supported raise
    VqfError before the first launch.

    The image features are data (img_features.requires_grad raises), fp32 on the GPU: CPU tensors and bf16 features raise
    VqfError -- there is no CPU fallback.  Dropout (rate drop_p) is active in train mode only;
    set_keep_masks() supplies explicit uint8 keep-masks for the tests, otherwise the kernels draw Philox masks."""

    def __init__(self, block_num=196, word_num=22, img_size=2048, vocab_size=15881, embed_size=512, hidden_size=1024,
                 output_size=3000, drop_p=0.5, coatt="parallel", packed_coatt=False):
        super(HieCoAttenLadder, self).__init__()
        if coatt not in COATT_MODES:
            raise ValueError("HieCoAttenLadder: coatt must be one of %s, got %r" % (", ".join(COATT_MODES), coatt))
        if packed_coatt and coatt != "alternating":
            raise ValueError("HieCoAttenLadder: packed_coatt=True needs coatt='alternating' (parallel mode has no image-side pass "
                             "that runs on packed rows), got coatt=%r" % (coatt,))
        self.coatt_mode = coatt
        self.packed_coatt = bool(packed_coatt)
        E = embed_size
        self.img_emb = nn.Linear(img_size, E)
        self.word_emb = nn.Embedding(vocab_size, E)
        self.phrase_uni = nn.Conv1d(E, E, 1)
        self.phrase_bi = nn.Conv1d(E, E, 2)
        self.phrase_tri = nn.Conv1d(E, E, 3)
        self.sent_lstm = nn.LSTM(E, E, batch_first=True)
        self.coatt = nn.ModuleList([(_Coatt if coatt == "parallel" else _CoattAlt)(E) for _ in range(3)])
        self.ans_w = nn.Linear(E, E)
        self.ans_p = nn.Linear(2 * E, E)
        self.ans_s = nn.Linear(2 * E, hidden_size)
        self.ans_h = nn.Linear(hidden_size, output_size)
        self.drop_p = drop_p
        self._seeds = _DropSeeds()

    def set_keep_masks(self, **masks):
        """Test hook: uint8 keep-masks 'img' (N*L, E) ((U*L, E) with img_index: one mask per image; the same padded shape for a PackedRegions), 'word' (N*T, E), 'ans_w' (N, E), 'ans_p' (N, 2E), 'ans_s' (N, 2E),
        'ans_h' (N, hidden_size); used in train mode in place of the in-kernel draws."""
        self._seeds.keep = masks

    def _draw(self, tag):
        """(keep, seed, rate) of one dropout site: one draw per tag and call, the same order always; masks count in train mode only"""
        return self._seeds.draw(tag if self.training else None, self.training, self.drop_p)

    def _drop(self, x, tag):
        keep, seed, rate = self._draw(tag)
        if keep is None and rate <= 0.0:
            return x
        return DropoutFn.apply(_c(x), keep, seed, rate)

    def _is_data(self, img, que_features):
        """region_layout's refusals about the tensors themselves: the features are fp32 data on the GPU, the ids int64"""
        if not img.is_cuda or not que_features.is_cuda:
            raise VqfError("HieCoAttenLadder needs GPU tensors (the HIP extension is the only path; no CPU fallback)")
        if img.dtype != torch.float32:
            raise VqfError("HieCoAttenLadder takes fp32 img_features (got %s)" % img.dtype)
        if img.requires_grad:
            raise VqfError("HieCoAttenLadder: img_features are data (no gradient into the image features)")
        if que_features.dtype != torch.int64:
            raise VqfError("HieCoAttenLadder takes int64 word ids")

    def _limits(self, T, who, N, U, L, R, D, grouped, counted, packed):
        """region_layout's refusals about the shapes this model's kernels take; none needs a GPU"""
        E, alt = self.img_emb.out_features, self.coatt_mode == "alternating"
        if packed and D != self.img_emb.in_features:
            raise VqfError("%s: PackedRegions.rows must have img_size = %d channels, got %s" % (who, self.img_emb.in_features, (R, D)))
        if packed and not ops.tanh_dropout_unpack_supported(U, R, L, E):
            raise VqfError("%s: PackedRegions takes 1 <= images <= 65535, 1 <= R < 2^29 rows, max_regions <= 1024 and "
                           "embed_size %% 4 == 0 (got images=%d, R=%d, max_regions=%d, E=%d)" % (who, U, R, L, E))
        if E % 32 or not ops.phrase_ngram_supported(T, E) or L > 1024 or T > 1024:
            raise VqfError("HieCoAttenLadder: embed_size %% 32 == 0, T <= 32 and L <= 1024 are supported (got E=%d, T=%d, L=%d)"
                           % (E, T, L))
        if alt and not (ops.guided_logits_supported(N, L, E, 3) and ops.guided_logits_supported(N, T, E, 1)):
            raise VqfError("HieCoAttenLadder(coatt='alternating'): embed_size %% 32 == 0, embed_size <= 1024, L <= 1024 and "
                           "N <= 65535 are supported (got E=%d, L=%d, T=%d, N=%d)" % (E, L, T, N))
        if packed and self.packed_coatt and not (ops.guided_logits_packed_supported(N, U, R, L, E, 3) and
                                                 ops.glimpse_pool_grouped_supported(N, U, L, E, 3)):
            raise VqfError("HieCoAttenLadder(packed_coatt=True): embed_size %% 32 == 0, embed_size <= 1024, max_regions <= 1024, "
                           "N <= 65535, 1 <= images <= 65535 and 1 <= R < 2^29 are supported (got E=%d, L=%d, N=%d, images=%d, R=%d)"
                           % (E, L, N, U, R))
        if grouped and not ((ops.guided_logits_grouped_supported(N, U, L, E, 3) and ops.glimpse_pool_grouped_supported(N, U, L, E, 3))
                            if alt else ops.row_block_supported(N, U, L * E)):
            raise VqfError("HieCoAttenLadder(img_index): 1 <= U <= 65535 images and N <= 65535 questions are supported "
                           "(got U=%d, N=%d, L=%d, E=%d)" % (U, N, L, E))

    def forward(self, img_features, que_features, q_length=None, img_index=None):
        if not torch.is_tensor(que_features) or que_features.dim() != 2:
            raise VqfError("HieCoAttenLadder takes (N, T) int64 word ids")
        T = que_features.shape[1]
        img_features, layout = region_layout("HieCoAttenLadder", img_features, que_features, img_index,
                                             lambda t: self._is_data(t, que_features), lambda *dims: self._limits(T, *dims))
        N, U, L = layout.N, layout.U, layout.L
        E = self.img_emb.out_features
        alt = self.coatt_mode == "alternating"
        MT = N * T
        lens = None
        if q_length is not None:
            if not torch.is_tensor(q_length) or q_length.dtype not in (torch.int64, torch.int32):
                raise VqfError("HieCoAttenLadder: q_length must be an int64 or int32 tensor")
            if tuple(q_length.shape) != (N,):
                raise VqfError("HieCoAttenLadder: q_length must have shape (N,) = (%d,), got %s" % (N, tuple(q_length.shape)))
            if q_length.device != que_features.device:
                raise VqfError("HieCoAttenLadder: q_length must be on the questions' device (%s), got %s"
                               % (que_features.device, q_length.device))
            lens = q_length.clamp(1, T).to(torch.int32).contiguous()            # O(N), on the device: nothing is read back
        # V = drop(tanh(img_emb(img))): (U*L, E), once per image; from a PackedRegions the product runs on the R real rows
        drop = self._draw("img")
        V = LinearFn.apply(_c(img_features).view(layout.R, -1), self.img_emb.weight, self.img_emb.bias, False)
        if not layout.packed:
            V = TanhDropFn.apply(V, None, *drop)
        elif self.packed_coatt:            # V stays (R, E): the masks of the padded tensor on the real rows
            V = TanhDropPackedFn.apply(V, layout.roff, U, L, *drop)
        else:                              # the tanh / dropout pass lays V out padded, (U*L, E) with zero padded rows
            V = TanhDropUnpackFn.apply(V, layout.roff, U, L, *drop)
            layout = layout.padded()
        if layout.grouped and not alt:
            V = RowBlockGatherFn.apply(V, *layout.grp, L)                                            # (N*L, E)
            layout = layout.per_question()
        # Qw = drop(tanh(word_emb(ids)))
        qw = EmbedTanhFn.apply(que_features, self.word_emb.weight, True, False, lens).view(MT, E)
        qw = self._drop(qw, "word")
        # phrase level
        qp = PhraseFn.apply(qw, self.phrase_uni.weight, self.phrase_uni.bias, self.phrase_bi.weight, self.phrase_bi.bias,
                            self.phrase_tri.weight, self.phrase_tri.bias, N, T, lens)
        # sentence level: the HIP LSTM over time-major rows (the re-layouts are dropout passes at rate 0)
        lstm = self.sent_lstm
        xt = DropoutBTFn.apply(qp.view(N, T, E).transpose(0, 1), None, 0, 0.0)            # (T, N, E) contiguous
        hs = LstmBatchFn.apply(xt, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, False)
        qs = DropoutBTFn.apply(hs.transpose(0, 1), None, 0, 0.0, lens).view(MT, E)      # (N*T, E), zero rows past the last word
        # the three co-attention levels
        if alt:
            w = [p_ for c in self.coatt for p_ in (c.sum_x.weight, c.sum_x.bias, c.sum_h.weight, c.img_x.weight, c.img_x.bias,
                                                   c.img_g.weight, c.img_h.weight, c.que_x.weight, c.que_x.bias, c.que_g.weight,
                                                   c.que_h.weight)]
            vcat, q0, q1, q2, av, aq0, aq1, aq2 = LadderAltCoattFn.apply(V, _c(qw), _c(qp), qs, N, L, T, lens, layout, *w)
        else:
            w = [p_ for c in self.coatt for p_ in (c.Wb.weight, c.Wv.weight, c.Wq.weight, c.whv.weight, c.whq.weight)]
            vcat, q0, q1, q2, av, aq0, aq1, aq2 = LadderCoattFn.apply(V, _c(qw), _c(qp), qs, N, L, T, lens, layout, *w)
        v0, v1, v2 = vcat[:, :E], vcat[:, E:2 * E], vcat[:, 2 * E:]
        th = lambda x: TanhDropFn.apply(x, None, None, 0, 0.0)
        lin = lambda x, m: LinearFn.apply(_c(x), m.weight, m.bias, False)
        h_w = th(lin(self._drop(q0 + v0, "ans_w"), self.ans_w))
        h_p = th(lin(self._drop(torch.cat([q1 + v1, h_w], 1), "ans_p"), self.ans_p))
        h_s = th(lin(self._drop(torch.cat([q2 + v2, h_p], 1), "ans_s"), self.ans_s))
        logits = lin(self._drop(h_s, "ans_h"), self.ans_h)
        aq = torch.cat([aq0, aq1, aq2], 1)                                              # (N, 3, T): 3 N T floats
        return logits, av, aq

"""MHBCoAtt and MHB on the HIP fusion path (reference interface: mhb_coAtt.py).

MHBCoAtt keeps the reference's behaviour, including the LSTM that is built
with batch_first=True but fed (T,N,.) and therefore recurs over the minibatch
axis (mhb_coAtt.py:27-36,72-74); set `fix_lstm_orientation=True` to opt out.
"""
import torch
import torch.nn as nn

from . import ops
from .functions import (LinearFn, Linear2Fn, AttHeadFn, FinalMfbFn, LstmSeqFn, LstmBatchFn, LogSoftmaxRowsFn, NormLink, embed_tanh,
                        embed, lstm_out_dropout)
from .mfb import (_DropSeeds, _image_is_data, _SideStream, _lstm_bf16, batch_first_lstm, warn_once, fusion_region_layout, regions_bf16_on,
                  regions_bf16_coatt_check, project_aside, join_or_fuse)


class MHBCoAtt(nn.Module):
    def __init__(self, cfg):
        super(MHBCoAtt, self).__init__()
        self.cfg = cfg
        self.word_embedding = nn.Embedding(cfg.q_vocab_size, cfg.emb_dim)
        lstm_in = cfg.emb_dim * 2 if cfg.glove else cfg.emb_dim
        self.lstm = nn.LSTM(input_size=lstm_in, hidden_size=cfg.hidden_dim,
                            num_layers=cfg.num_layers, batch_first=True)
        self.dropout_l = nn.Dropout(p=0.3)
        self.ques_att_conv1 = nn.Conv2d(cfg.hidden_dim, 512, [1, 1])
        self.ques_att_conv2 = nn.Conv2d(512, 2, [1, 1])
        self.ques_proj1 = nn.Linear(2 * cfg.hidden_dim, 5000)
        self.img_conv1d = nn.Conv2d(cfg.img_feature_channel, 5000, [1, 1])
        self.dropout_m = nn.Dropout(p=0.1)
        self.co_att_conv1 = nn.Conv2d(1000, 512, [1, 1])
        self.co_att_conv2 = nn.Conv2d(512, 2, [1, 1])
        self.ques_proj2 = nn.Linear(2 * cfg.hidden_dim, 5000)
        self.ques_proj3 = nn.Linear(2 * cfg.hidden_dim, 5000)
        self.img_proj2 = nn.Linear(2 * cfg.img_feature_channel, 5000)
        self.img_proj3 = nn.Linear(2 * cfg.img_feature_channel, 5000)
        self.linear_pred = nn.Linear(2000, cfg.a_vocab_size)
        self.fix_lstm_orientation = False
        self.gemm_dtype = "fp32"          # or "bf16" (BASELINE config 3), see MFB.gemm_dtype
        # the batch-axis recursion as one fused HIP kernel per step instead of nn.LSTM (MIOpen spends
        # ~35 ms per step on 512 sequential tiny steps); same arithmetic, see csrc/lstm.hip
        self.use_hip_lstm = True
        self.overlap_streams = True       # img_conv1d on a side stream, see MFB.overlap_streams
        self.fuse_bf16_dp = True          # see MFB.fuse_bf16_dp
        self.fold_norm = True             # see MFB.fold_norm
        self.packed_coatt = False         # see MFB.packed_coatt
        self.regions_bf16 = False         # see MFB.regions_bf16
        self.regions_bf16_coatt = False   # see MFB.regions_bf16_coatt
        self.side_cu_limit = 0            # see MFB.side_cu_limit
        self.side_bf16 = False            # see MFB.side_bf16
        self._side = _SideStream()
        self._seeds = _DropSeeds()

    def set_keep_masks(self, **masks):
        self._seeds.keep = masks

    def forward(self, img_features, questions, glove_matrix=None, is_training=True, img_index=None):
        """img_index: see MFB.forward -- img_features (U, L, D) are the images the N questions share; the batch-axis LSTM
        recursion runs over the questions in the caller's order, untouched.
        Region counts: see MFB.forward -- img_features may be the pair (img, img_length), one count per image ((N,), or (U,) with
        img_index; fp32 only); the fusion's norm and
        the co-attention softmax run over each image's real regions.  The padded rows of img_features must be FINITE: the
        projection and its weight gradient still run over them, and they cancel only because their dP rows are exact zeros.
        Packed regions: see MFB.forward -- img_features may be a PackedRegions(rows, offsets, max_regions) (fp32 only): the real
        regions of every image, never padded; the result is this model on (packed.unpack(), ...).
        packed_coatt = True (an attribute, default False): see MFB.forward -- with a PackedRegions and no img_index the co-attention
        head runs on the R real rows as well; refused (VqfError) together with img_index, no effect on the other call forms.
        regions_bf16 = True (an attribute, default False): see MFB.forward -- with gemm_dtype "fp32", a PackedRegions or the pair
        (img, img_length) and no img_index, img_conv1d and its weight gradient take bf16 operands with fp32 accumulation and dP
        (and P, where the large-tile bf16 GEMM applies) is stored in bf16; the question side, the co-attention head, the pooling,
        the norms, the masks and the loss stay fp32.  Refused (VqfError) together with img_index and for a channel count that is
        no multiple of 8; no effect on a plain tensor.
        regions_bf16_coatt = True (an attribute, default False): see MFB.forward -- on exactly the calls where regions_bf16 takes
        effect, co_att_conv1's forward, input gradient and weight gradient take bf16 operands with fp32 accumulation too, as
        gemm_dtype "bf16-att" runs them on a plain tensor; everything else stays as under regions_bf16.  Refused (VqfError, before
        the first launch) on a PackedRegions or a pair (img, img_length) where regions_bf16 does not apply (regions_bf16 = False, or
        a gemm_dtype other than "fp32"); no effect on a plain tensor."""
        coatt_regions = bool(self.regions_bf16_coatt)
        regions_bf16_coatt_check("MHBCoAtt", img_features, img_index, self.gemm_dtype,
                                 self.regions_bf16 and self.img_conv1d.out_channels, coatt_regions)
        img_features, img3, L, layout = fusion_region_layout("MHBCoAtt", img_features, questions, img_index, self.gemm_dtype,
                                                             self.packed_coatt, self.regions_bf16 and self.img_conv1d.out_channels)
        N = questions.shape[0]
        bf16_regions = regions_bf16_on(self.regions_bf16, self.gemm_dtype, layout)
        coatt_regions = coatt_regions and bf16_regions
        bf16_img = bf16_regions or self.gemm_dtype in ("bf16", "bf16-img", "bf16-all")
        bf16_all = self.gemm_dtype == "bf16-all"          # also ques_proj*, img_proj*, the question-attention conv
        proj = project_aside(self, img3, bf16_img, bf16_regions)
        que_embedded = embed_tanh(self.word_embedding, questions)            # (N,T,E)
        if self.cfg.glove:
            assert glove_matrix is not None, 'glove should not be NoneType.'
            que_embedded = torch.cat((que_embedded, glove_matrix), dim=2)
        if self.fix_lstm_orientation:
            lstm_o = batch_first_lstm(self.lstm, que_embedded, self.use_hip_lstm, _lstm_bf16(self.gemm_dtype))   # (N,T,H)
            ques_feature = lstm_out_dropout(self.dropout_l, lstm_o, self._seeds)
        elif (self.use_hip_lstm and self.lstm.num_layers == 1 and que_embedded.is_cuda
              and ops.lstm_seq_supported(que_embedded.shape[1], self.cfg.hidden_dim)):
            # batch_first LSTM fed (T,N,.): sequence axis = N, per-step batch = T  (mhb_coAtt.py:72-74).
            # (N,T,.) is already (S,B,.) for the sequence kernel and its output (N,T,H) is the
            # reference's lstm_o.permute(1,0,2).
            hs = LstmSeqFn.apply(que_embedded, self.lstm.weight_ih_l0, self.lstm.weight_hh_l0,
                                 self.lstm.bias_ih_l0, self.lstm.bias_hh_l0,
                                 _lstm_bf16(self.gemm_dtype))     # bf16 modes: bf16 operands in the recurrent product
            ques_feature = lstm_out_dropout(self.dropout_l, hs, self._seeds)        # mhb_coAtt.py:75
        else:
            if self.use_hip_lstm:
                warn_once("lstm_seq", "MHBCoAtt's batch-axis LSTM recursion runs on nn.LSTM (MIOpen: one tiny step per "
                          "sample, ~35 ms per 512-sample step), not on the HIP LstmSeqFn, which covers one layer, "
                          "tokens per question <= 32 and hidden_dim in {256, 512, 768, 1024} (got T=%d, H=%d, layers=%d)"
                          % (que_embedded.shape[1], self.cfg.hidden_dim, self.lstm.num_layers))
            lstm_o, _ = self.lstm(que_embedded.permute(1, 0, 2))             # (T,N,H), recurs over N
            ques_feature = lstm_out_dropout(self.dropout_l, lstm_o.permute(1, 0, 2), self._seeds)   # (N,T,H) contiguous
        T, H = ques_feature.shape[1], ques_feature.shape[2]

        qa = AttHeadFn.apply(ques_feature.view(N * T, H), ques_feature,
                             self.ques_att_conv1.weight, self.ques_att_conv1.bias, None, None,
                             self.ques_att_conv2.weight, self.ques_att_conv2.bias, False, bf16_all, None, True)
        qp = LinearFn.apply(qa, self.ques_proj1.weight, self.ques_proj1.bias, False, bf16_all)
        pm = self.dropout_m.p
        coatt_bf16 = coatt_regions or self.gemm_dtype in ("bf16", "bf16-att", "bf16-all")
        link = NormLink(want_xb=coatt_regions) if self.fold_norm else None
        Y = join_or_fuse(self, proj, img3, qp, self._seeds.draw('m1', self.training, pm), bf16_img, N, L, link, layout)
        va = AttHeadFn.apply(Y, img_features, self.co_att_conv1.weight, self.co_att_conv1.bias, None, None,
                             self.co_att_conv2.weight, self.co_att_conv2.bias, False, coatt_bf16, link, False, layout)
        ys = []
        for tag, qpj, ipj in (('m2', self.ques_proj2, self.img_proj2), ('m3', self.ques_proj3, self.img_proj3)):
            ys.append(FinalMfbFn.apply(qa, va, qpj.weight, qpj.bias, ipj.weight, ipj.bias, *self._seeds.draw(tag, self.training, pm),
                                       None, False, bf16_all))
        # :147-148  linear_pred(cat((att_normed_2, att_normed_3), 1)): the concatenation is never materialised
        logits = Linear2Fn.apply(ys[0], ys[1], self.linear_pred.weight, self.linear_pred.bias)
        return LogSoftmaxRowsFn.apply(logits)                                # :149-151 (implicit dim = 1 on the 2-D logits)


class MHB(nn.Module):
    """Mean-pooled image x last valid LSTM state, two cascaded MFB blocks (mhb_coAtt.py:153-217).

    The reference class cannot run as shipped (hard .cuda() at :176 is harmless
    here, but :214 names an undefined `mhb_22`); this follows the evident
    intent `mhb_12` (:213).
    """

    def __init__(self, cfg):
        super(MHB, self).__init__()
        self.model_name = cfg.model_name
        self.cfg = cfg
        self.mean_pool = nn.AvgPool2d((14, 14))
        self.Embedding = nn.Embedding(cfg.q_vocab_size, cfg.emb_dim)
        self.LSTM = nn.LSTM(input_size=cfg.emb_dim, hidden_size=cfg.hidden_dim, num_layers=1,
                            batch_first=False)
        self.linear_q_1 = nn.Linear(cfg.hidden_dim, 5000)
        self.linear_q_2 = nn.Linear(cfg.hidden_dim, 5000)
        self.linear_i_1 = nn.Linear(cfg.img_feature_channel, 5000)
        self.linear_i_2 = nn.Linear(cfg.img_feature_channel, 5000)
        self.lstm_dropout = nn.Dropout(0.3)
        self.mfb_dropout = nn.Dropout(0.1)
        self.linear_out = nn.Linear(2000, cfg.a_vocab_size)
        self.use_hip_lstm = True          # LSTM recursion on the HIP path (functions.LstmBatchFn) instead of MIOpen
        self._seeds = _DropSeeds()

    def set_keep_masks(self, **masks):
        self._seeds.keep = masks

    def forward(self, img_feature, questions, q_length):
        batch_size, max_len = questions.size()
        # AvgPool2d(14,14) over the (N,C,14,14) view == mean over the 196 regions   :178-180
        # (the glimpse kernel with unit weights sums the regions; fp32 or bf16 feature storage)
        img3 = img_feature.reshape(batch_size, -1, self.cfg.img_feature_channel)
        _image_is_data(img3, "bf16")
        img3 = img3 if img3.is_contiguous() else img3.contiguous()
        L = img3.shape[1]
        _, i_sum = ops.glimpse_pool_fwd(img3, torch.zeros((batch_size * L, 1), device=img3.device), True)
        i_mean = i_sum * (1.0 / L)
        q_embedded = embed(self.Embedding, questions).permute(1, 0, 2)              # (T,N,E)  :181-182
        if (self.use_hip_lstm and q_embedded.is_cuda and self.LSTM.num_layers == 1 and not self.LSTM.bidirectional
                and self.LSTM.hidden_size % 4 == 0):
            lstm_outs = LstmBatchFn.apply(q_embedded.contiguous(), self.LSTM.weight_ih_l0, self.LSTM.weight_hh_l0,
                                          self.LSTM.bias_ih_l0, self.LSTM.bias_hh_l0)       # (T,N,H)
        else:
            if self.use_hip_lstm:
                warn_once("lstm_mhb", "MHB's LSTM runs on nn.LSTM (MIOpen), not on the HIP LstmBatchFn (one layer, "
                          "unidirectional, hidden_size % 4 == 0, GPU input)")
            lstm_outs, _ = self.LSTM(q_embedded)                             # (T,N,H)
        idx = (q_length.to(torch.long) - 1).to(lstm_outs.device)
        lstm_out = lstm_outs[idx, torch.arange(batch_size, device=lstm_outs.device)]   # :185-186
        lstm_out = lstm_out_dropout(self.lstm_dropout, lstm_out.unsqueeze(1), self._seeds).squeeze(1)      # :188
        pm = self.mfb_dropout.p
        mhb_1, z1 = FinalMfbFn.apply(lstm_out, i_mean, self.linear_q_1.weight, self.linear_q_1.bias, self.linear_i_1.weight,
                                     self.linear_i_1.bias, *self._seeds.draw('m1', self.training, pm), None, True)     # :190-199
        mhb_2 = FinalMfbFn.apply(lstm_out, i_mean, self.linear_q_2.weight, self.linear_q_2.bias, self.linear_i_2.weight,
                                 self.linear_i_2.bias, *self._seeds.draw('m2', self.training, pm), z1, False)          # :201-211
        # :213-214  linear_out(cat((mhb_1, mhb_2), 1)) without the concatenated tensor (:214 names mhb_22: see the class docstring)
        logits = Linear2Fn.apply(mhb_1, mhb_2, self.linear_out.weight, self.linear_out.bias)
        return LogSoftmaxRowsFn.apply(logits)                                # :215-217

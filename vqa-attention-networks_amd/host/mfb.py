"""MFB-baseline model on the HIP fusion path.

Mirrors the reference interface (mfb.py:6-140): `MFB(cfg)`,
`forward(img_features, questions, is_training=True) -> logits (N, a_vocab_size)`,
identical state_dict keys/shapes, so it drops into solver.py / train_models.py.
The question encoder's embedding lookup + tanh (mfb.py:68, csrc/embed.hip), its LSTM
recursion and everything from the question attention to the logits run in
libvqa_fusion.so (`use_hip_lstm = False` puts the LSTM back on nn.LSTM / MIOpen), dropout_l
(mfb.py:70) included (`vqf_dropout_bt`: the nn.Dropout module only carries the rate).
"""
import torch
import torch.nn as nn

from . import ops
from .lib import VqfError
from .grouping import check_img_index, check_img_length, check_packed_regions, PackedRegions, RegionLayout
from .functions import (LinearFn, AttHeadFn, ImgFuseFn, ImgProjFn, ImgProjLateFn, ImgProjDeferFn, MfbFuseFn, FinalMfbFn,
                        LstmBatchFn, UnitPoolFn, DeadParamsFn, NormLink, img_project, embed_tanh, lstm_out_dropout)


def _image_is_data(img, gemm_dtype="fp32"):
    """The image grid features are input data on this path (no d/d-image kernels: SURVEY 8a, a5),
    and they must live on the GPU: there is no CPU fallback.  A bf16 feature tensor (bf16 storage,
    data_loader.FeatureStager(bf16=True)) is accepted when the image projection runs in bf16."""
    if not img.is_cuda:
        raise VqfError("vqa fusion modules need GPU tensors (HIP extension is the only path; no CPU fallback)")
    if img.dtype == torch.bfloat16:
        if gemm_dtype not in ("bf16", "bf16-img", "bf16-all"):
            raise VqfError("bf16 img_features need model.gemm_dtype = 'bf16', 'bf16-img' or 'bf16-all'; "
                           "the fp32 path takes fp32 features")
        if img.shape[-1] % 8:
            raise VqfError("bf16 img_features: the channel count must be a multiple of 8")
    elif img.dtype != torch.float32:
        raise VqfError("img_features must be fp32 or bf16, got %s" % img.dtype)
    if img.requires_grad:
        raise VqfError("img_features.requires_grad=True: the HIP fusion path treats the image tensor as "
                       "data and does not produce its gradient")


def split_region_features(who, img_features):
    """The region-count call form: img_features given as the pair (img (N, L, D), img_length (N,)) -> (img, img_length); a plain
    tensor -> (img, None).  forward() keeps its parameter list (the positional call forms are pinned); the counts travel with
    the features they describe, as data_loader.pad_region_features returns them."""
    if isinstance(img_features, (tuple, list)):
        if any(isinstance(t, PackedRegions) for t in img_features):
            raise VqfError("%s: a PackedRegions carries its own counts and is passed on its own, not inside a pair (img, img_length)"
                           % who)
        if len(img_features) != 2 or not torch.is_tensor(img_features[0]):
            raise VqfError("%s: img_features must be a tensor or the pair (img (N, L, D), img_length (N,)), got a %s of %d"
                           % (who, type(img_features).__name__, len(img_features)))
        return img_features[0], img_features[1]
    return img_features, None


def _fusion_limits(who, N, U, L, R, D, grouped, counted, packed):
    """region_layout's `limits` of MFB / MHBCoAtt: the shapes their grouped, region-count and packed fusion kernels take."""
    if packed:
        if not (1 <= N <= 65535 and ops.mfb_fuse_packed_supported(N, U, R, L, 1000) and ops.glimpse_pool_grouped_supported(N, U, L, D, 2)
                and (not grouped or ops.row_block_supported(N, U, 2 * D))):
            raise VqfError("%s: PackedRegions needs at most 65535 questions and images and a channel count that is a multiple of 4 "
                           "(got U=%d, N=%d, R=%d, L=%d, D=%d)" % (who, U, N, R, L, D))
        return
    if grouped and not (ops.mfb_fuse_grouped_supported(N, U, L, 1000) and ops.glimpse_pool_grouped_supported(N, U, L, D, 2)
                        and ops.row_block_supported(N, U, 2 * D)):
        raise VqfError("%s: img_index needs L <= 1024 regions and a channel count that is a multiple of 4 (got U=%d, N=%d, L=%d, "
                       "D=%d)" % (who, U, N, L, D))
    if counted and L > 1024:
        raise VqfError("%s: img_length needs L <= 1024 regions (got L=%d)" % (who, L))


def region_layout(who, img_features, questions, img_index, is_data, limits, gemm_dtype="fp32"):
    """The one place that turns a call form into what the nodes take: img_features a tensor (U, L, D), the pair (img, img_length) or
    a PackedRegions, each with or without img_index -> (img (U, L, D) or rows (R, D), grouping.RegionLayout).  Every refusal of the
    form is raised here, before the first launch: those of the arguments themselves (grouping.check_*), the fp32-only ones
    (gemm_dtype: the grouped, region-count and packed kernels have no bf16 form), the model's own about the feature tensor
    (is_data(t): device, dtype, no gradient) and about the shapes its kernels take (limits(who, N, U, L, R, D, grouped, counted,
    packed)).  The index, the counts and the offsets are converted on the device and never read on the host (the kernels clamp
    what they hold).  Without img_index there is one image per question: the layout's N is U."""
    dev = questions.device
    if isinstance(img_features, PackedRegions):
        packed = img_features
        if gemm_dtype != "fp32":
            raise VqfError("%s: PackedRegions is fp32 only (the packed fusion kernels have no bf16 form); got gemm_dtype=%r"
                           % (who, gemm_dtype))
        N = questions.shape[0]
        U = N if img_index is None else (packed.offsets.numel() - 1 if torch.is_tensor(packed.offsets) else -1)
        check_packed_regions(who, packed, U, dev)
        rows, L = packed.rows, packed.max_regions
        if rows.device != dev:
            raise VqfError("%s: PackedRegions.rows must be on the questions' device (%s), got %s" % (who, dev, rows.device))
        limits(who, N, U, L, rows.shape[0], rows.shape[1], img_index is not None, False, True)
        is_data(rows)
        if img_index is not None:
            check_img_index(who, img_index, N, U, dev)
        return rows.contiguous(), RegionLayout(N, U, L, img_index, None, packed.offsets, rows.shape[0])
    img, img_length = split_region_features(who, img_features)
    is_data(img)
    U, L, D = img.shape
    N = U if img_index is None else questions.shape[0]
    if (img_index is not None or img_length is not None) and (gemm_dtype != "fp32" or img.dtype != torch.float32):
        raise VqfError("%s: %s is fp32 only (the %s fusion kernels have no bf16 form); got gemm_dtype=%r and %s img_features"
                       % ((who,) + (("img_index", "grouped") if img_index is not None else ("img_length", "region-count"))
                          + (gemm_dtype, img.dtype)))
    if img_index is not None:
        check_img_index(who, img_index, N, U, dev)
    if img_length is not None:
        check_img_length(who, img_length, U, dev)
    limits(who, N, U, L, U * L, D, img_index is not None, img_length is not None, False)
    return img, RegionLayout(N, U, L, img_index, img_length)


def regions_bf16_applies(who, img_features, img_index, gemm_dtype, regions_bf16):
    """The models' regions_bf16 attribute on one call -> whether the image projection of this call runs in bf16.  regions_bf16: False,
    or the projection's output width 5*O (True stands for the models' 5000).  It applies with gemm_dtype "fp32" (any other value
    keeps its own meaning and its own refusals) to a PackedRegions or a pair (img, img_length) with counts; a plain tensor is not
    touched.  Its two refusals are raised here, before anything looks at a device: together with img_index (the grouped fusion
    backward has an image-owned pass of its own, which stays fp32), and a channel count D or a width 5*O that is no multiple of 8
    (the bf16 GEMM entry's extents)."""
    if not regions_bf16 or gemm_dtype != "fp32":
        return False
    if isinstance(img_features, PackedRegions):
        feat = img_features.rows
    elif isinstance(img_features, (tuple, list)) and len(img_features) == 2 and img_features[1] is not None:
        feat = img_features[0]
    else:
        return False
    if img_index is not None:
        raise VqfError("%s: regions_bf16 = True does not take img_index (the fusion backward over shared images is fp32 only); set "
                       "regions_bf16 = False for batches whose questions share images" % who)
    W5 = 5000 if regions_bf16 is True else int(regions_bf16)
    D = feat.shape[-1] if torch.is_tensor(feat) and feat.dim() >= 2 else 8         # (not a feature tensor: region_layout says so)
    if D % 8 or W5 % 8:
        raise VqfError("%s: regions_bf16 = True needs a channel count D and a projection width 5*O that are multiples of 8 (the bf16 "
                       "GEMM's extents); got D=%d, 5*O=%d" % (who, D, W5))
    return True


def regions_bf16_on(regions_bf16, gemm_dtype, layout):
    """regions_bf16_applies behind fusion_region_layout, which has made its refusals: read off the nodes' layout"""
    return bool(regions_bf16) and gemm_dtype == "fp32" and layout is not None and not layout.grouped and \
        (layout.packed or layout.counted)


def regions_bf16_coatt_check(who, img_features, img_index, gemm_dtype, regions_bf16, regions_bf16_coatt):
    """The models' regions_bf16_coatt attribute on one call, in front of fusion_region_layout (regions_bf16: as regions_bf16_applies
    takes it, whose own refusals speak first, with their texts).  The attribute rides on regions_bf16: on a region form -- a
    PackedRegions or the pair (img, img_length) with counts -- where regions_bf16 does not apply (it is False, or gemm_dtype is not
    "fp32") the call is refused here, before anything looks at a device, instead of running the head in fp32 behind the user's
    back.  A plain tensor is not touched, and without the attribute nothing is looked at."""
    if not regions_bf16_coatt or regions_bf16_applies(who, img_features, img_index, gemm_dtype, regions_bf16):
        return
    if isinstance(img_features, PackedRegions) or (isinstance(img_features, (tuple, list)) and len(img_features) == 2
                                                   and img_features[1] is not None):
        raise VqfError("%s: regions_bf16_coatt = True needs regions_bf16 = True and gemm_dtype \"fp32\" on a PackedRegions or the pair "
                       "(img, img_length): the bf16 co-attention head on a region layout runs behind the bf16 image projection "
                       "only; set regions_bf16 = True, or regions_bf16_coatt = False" % who)


def fusion_region_layout(who, img_features, questions, img_index, gemm_dtype, packed_coatt=False, regions_bf16=False):
    """MFB / MHBCoAtt's call of region_layout -> (img (U, L, D) or rows (R, D), the 3-D tensor the projection nodes flatten -- rows
    as (1, R, D) --, L, the nodes' layout: None for the plain tensor, whose path takes nothing extra).
    packed_coatt (the models' attribute): a PackedRegions without img_index gets the layout whose rows BEHIND the fusion are packed
    too (RegionLayout.packed_rows()); with img_index it is refused here, in front of every other check and of the first launch (a
    question's rows would be those of its image, and their total is a shape that would have to be read on the host); for a plain
    tensor or the pair (img, img_length) it changes nothing.
    regions_bf16 (the models' attribute, as regions_bf16_applies takes it): that function's two refusals are raised here, behind the
    one above and in front of everything else; the layout itself does not change (the models ask regions_bf16_on)."""
    if packed_coatt and img_index is not None and isinstance(img_features, PackedRegions):
        raise VqfError("%s: packed_coatt = True does not take img_index (the co-attention head on the packed rows has one image per "
                       "question); set packed_coatt = False for batches whose questions share images" % who)
    regions_bf16_applies(who, img_features, img_index, gemm_dtype, regions_bf16)
    img, layout = region_layout(who, img_features, questions, img_index, lambda t: _image_is_data(t, gemm_dtype), _fusion_limits,
                                gemm_dtype)
    if packed_coatt:
        layout = layout.packed_rows()
    return img, (img.unsqueeze(0) if layout.packed else img), layout.L, (None if layout.plain else layout)


_warned = set()


def warn_once(key, msg):
    """One log line per process and reason when a module leaves the HIP path for a torch/MIOpen op
    (the answer stays the same, the speed does not: MHBCoAtt's batch-axis recursion costs ~35 ms per step there)."""
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn("vqa fusion path: " + msg, RuntimeWarning, stacklevel=3)


def _lstm_bf16(gemm_dtype):
    """LSTM precision flag of the functions.Lstm*Fn: False (fp32), True ("bf16": bf16 operands in the recurrent
    products) or "all" ("bf16-all": also in the input projection and the weight gradients)."""
    return "all" if gemm_dtype == "bf16-all" else gemm_dtype == "bf16"


def hip_batch_lstm_ok(lstm, x_is_cuda_fp32, use_hip=True):
    """whether batch_first_lstm runs the recursion on the HIP path (functions.LstmBatchFn)"""
    return bool(use_hip and x_is_cuda_fp32 and lstm.num_layers == 1 and not lstm.bidirectional and lstm.proj_size == 0
                and lstm.hidden_size % 4 == 0)


def batch_first_lstm(lstm, x, use_hip=True, bf16=False, time_major_in=False):
    """nn.LSTM(batch_first=True) forward of x (N,T,E) -> (N,T,H) with zero initial state (mfb.py:69).  The
    recursion runs on the HIP path (MFMA GEMMs + one point-wise kernel per step, functions.LstmBatchFn) with
    the nn.LSTM module's own parameters; anything it does not cover (several layers, bidirectional,
    projections) stays on nn.LSTM.  time_major_in: x arrives as (T,N,E) (embed_tanh(time_major=True))."""
    if hip_batch_lstm_ok(lstm, x.is_cuda and x.dtype == torch.float32, use_hip):
        hs = LstmBatchFn.apply(x if time_major_in else x.transpose(0, 1).contiguous(), lstm.weight_ih_l0, lstm.weight_hh_l0,
                               lstm.bias_ih_l0 if lstm.bias else None, lstm.bias_hh_l0 if lstm.bias else None, bf16)
        return hs.transpose(0, 1)
    if time_major_in:
        x = x.transpose(0, 1).contiguous()
    if use_hip:
        warn_once("lstm_batch", "question-encoder LSTM runs on nn.LSTM (MIOpen), not on the HIP LstmBatchFn: it needs "
                  "a GPU fp32 input, one layer, unidirectional, no projection, hidden_size %% 4 == 0 (got layers=%d, "
                  "bidirectional=%s, proj=%d, hidden=%d, dtype=%s)" % (lstm.num_layers, lstm.bidirectional,
                                                                      lstm.proj_size, lstm.hidden_size, x.dtype))
    out, _ = lstm(x)
    return out


class _SideStream:
    """Runs the image projection on a second HIP stream (one per device, created lazily)."""

    def __init__(self):
        self.streams = {}

    def project(self, img, conv, bf16, same_stream=False, cu_limit=0, pad_k=False):
        dev = img.device
        if same_stream:
            # the projection stays its own autograd node but runs on the caller's stream: created first, its
            # backward (the weight-gradient GEMM) is the LAST node autograd runs, so every other gradient bucket
            # is already being all-reduced (on RCCL's stream) while that 15 ms GEMM computes
            if not bf16 and _SideStream.DEFER and img.dtype == torch.float32:
                # ... and its PRODUCT is issued by join(), behind the question encoder (functions.ImgProjDeferFn)
                return ("defer", ImgProjDeferFn.apply(img, conv.weight), img, conv.weight), None
            return ImgProjFn.apply(img, conv.weight, bf16, pad_k), None
        # a second stream: the product is computed NOW, without an autograd node; join() creates the node late, so that
        # its backward (the weight gradient) is issued early in the backward pass (functions.ImgProjLateFn) and overlaps
        # the question-side backward the way the product overlaps the question-side forward
        side = self.streams.get(dev)
        if side is None:
            side = self.streams[dev] = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(dev)
        side.wait_stream(cur)                    # inputs / weights produced on the caller's stream
        with torch.cuda.stream(side), torch.no_grad():
            P0, img2 = img_project(img, conv.weight, bf16, cu_limit, pad_k)
        return (P0, img2, conv.weight, cu_limit), side

    DEFER = True       # one-stream form: issue the projection's product behind the question encoder (A/B switch)

    @staticmethod
    def join(P0, side):
        if side is None:
            if isinstance(P0, tuple) and P0[0] == "defer":
                _, P, img, w = P0
                with torch.no_grad():
                    ImgProjDeferFn.fill(P, img, w)
                return P
            return P0
        P0, img2, w, cu_limit = P0
        with torch.cuda.stream(side):            # the node's stream = the stream its backward will run on
            P = ImgProjLateFn.apply(P0, img2, w, cu_limit)
        cur = torch.cuda.current_stream(P.device)
        cur.wait_stream(side)
        P0.record_stream(cur)                    # allocated on the side stream, consumed here
        img2.record_stream(cur)
        return P


class _DropSeeds:
    """Per-call dropout seeds for the in-kernel Philox masks (train mode)."""

    def __init__(self):
        self.keep = {}      # optional externally supplied uint8 keep-masks (parity tests)

    def next(self, training, p):
        if not training or p <= 0.0:
            return 0, 0.0
        # one 63-bit seed per call from torch's CPU generator: reproducible under manual_seed
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()), p

    def draw(self, tag, training, p):
        """One dropout site's arguments -> (keep, seed, rate): the explicit keep-mask under `tag` if the test gave one, else one
        seed from the stream (next); the rate is p with a mask, else the drawn rate (0 outside training).  One call = one draw,
        with or without a mask, so the seed stream does not depend on the masks."""
        seed, rate = self.next(training, p)
        keep = self.keep.get(tag)
        return keep, seed, (p if keep is not None else rate)


def project_aside(model, img3, bf16_img, pad_k=False):
    """MFB / MHBCoAtt: start a5 first -- it only needs the image and its weights -- as its own node (model._side: on the side
    stream, or on the caller's for overlap_streams = "same-stream") -> what join_or_fuse takes, or None for projection + fusion in
    one node (ImgFuseFn).  The bf16 modes keep the one node (fuse_bf16_dp): its backward hands dP to the weight-gradient GEMM in
    bf16 without an fp32 round trip, which is worth more than the stream overlap; a real second stream -- overlap_streams is
    True -- with side_bf16 keeps the bf16 hand-off too (MfbFuseFn takes / returns bf16).  pad_k: the bf16 projection of a region
    layout (regions_bf16), whose operands of the weight gradient are zero-padded to K % 32 == 0 rows (functions._img_proj)."""
    ov = model.overlap_streams
    if not ov or (bf16_img and model.fuse_bf16_dp and not (ov is True and model.side_bf16)):
        return None
    return model._side.project(img3, model.img_conv1d, bf16_img, ov == "same-stream", model.side_cu_limit, pad_k)


def join_or_fuse(model, proj, img3, qp, drop, bf16_img, N, L, link, layout):
    """a5+a6: the MFB fusion over the regions behind project_aside's projection (joined here), or projection + fusion as one node;
    drop = (keep, seed, rate).  -> Y (N*L, 1000); with a link the un-normalised R"""
    conv = model.img_conv1d
    if proj is not None:
        return MfbFuseFn.apply(model._side.join(*proj), conv.bias, qp, *drop, N, L, link, layout)
    return ImgFuseFn.apply(img3, conv.weight, conv.bias, qp, *drop, bf16_img, link, layout)


class MFB(nn.Module):
    def __init__(self, cfg):
        super(MFB, self).__init__()
        self.cfg = cfg
        self.word_embedding = nn.Embedding(cfg.q_vocab_size, cfg.emb_dim)
        self.lstm = nn.LSTM(input_size=cfg.emb_dim, hidden_size=cfg.hidden_dim,
                            num_layers=cfg.num_layers, batch_first=True)
        self.dropout_l = nn.Dropout(p=0.3)
        self.multilayer = cfg.model_name == 'mfb-multilayer'
        self.ques_att_conv1 = nn.Conv2d(cfg.hidden_dim, 1024, [1, 1])
        if self.multilayer:
            self.ques_att_multiconv = nn.Conv2d(1024, 512, [1, 1])
            self.ques_att_conv2 = nn.Conv2d(512, 2, [1, 1])
        else:
            self.ques_att_conv2 = nn.Conv2d(1024, 2, [1, 1])
        self.ques_proj1 = nn.Linear(2 * cfg.hidden_dim, 5000)
        self.img_conv1d = nn.Conv2d(cfg.img_feature_channel, 5000, [1, 1])
        self.dropout_m = nn.Dropout(p=0.1)      # its .p is the rate of the in-kernel Philox masks
        self.co_att_conv1 = nn.Conv2d(1000, 1024, [1, 1])
        if self.multilayer:
            self.co_att_multiconv = nn.Conv2d(1024, 512, [1, 1])
            self.co_att_conv2 = nn.Conv2d(512, 2, [1, 1])
        else:
            self.co_att_conv2 = nn.Conv2d(1024, 2, [1, 1])
        self.ques_proj2 = nn.Linear(2 * cfg.hidden_dim, 5000)
        self.img_proj2 = nn.Linear(2 * cfg.img_feature_channel, 5000)
        self.linear_pred = nn.Linear(1000, cfg.a_vocab_size)
        # reference_compat: mfb.py:84,118 run both softmaxes over a singleton axis (weights == 1)
        self.unit_softmax = True
        # Execution mode under unit_softmax.  False ("faithful", default and the benchmarked one): every op
        # the reference's autograd executes is executed.  True ("pruned"): with attention weights == 1 the
        # glimpses are plain sums, so both attention MLPs, ques_proj1, img_conv1d and the fusion over the
        # regions cannot influence the logits and their 12 parameter tensors get exactly-zero gradients;
        # the pruned mode skips that work (96 % of the FLOPs) and returns bit-identical logits and gradients.
        self.pruned = False
        # "fp32" (default, parity 1e-4) or "bf16": bf16 operands / fp32 accumulate for the two large
        # GEMM families (img_conv1d and co_att_conv1, 96 % of the FLOPs); everything else stays fp32.
        # "bf16-all": additionally ques_proj1, the final blocks' ques_proj* / img_proj* and the question-attention
        # conv take bf16 operands (forward, dgrad and weight gradient), and so do the LSTM's input projection (K = 300
        # zero-padded to 304 by the cast) with its two gradients and the recurrent weight gradient; the classifier, the
        # fusion / attention / normalisation arithmetic, the LSTM's gates and state and every reduction stay fp32
        self.gemm_dtype = "fp32"
        # True: run img_conv1d (and, through autograd, its weight gradient) on a side stream, concurrently
        # with the question encoder / question attention (and their backward + gradient all-reduce).
        # "same-stream": the projection is its own autograd node on the caller's stream (its weight gradient
        # then runs last in the backward, behind which the other buckets' all-reduce hides); one compute stream.
        # False: projection + fusion as one node (ImgFuseFn).
        self.overlap_streams = True
        # question encoder's LSTM recursion on the HIP path instead of nn.LSTM / MIOpen (same parameters)
        self.use_hip_lstm = True
        # bf16 mode: one autograd node for projection + fusion, whose backward writes dP in bf16 for the
        # weight-gradient GEMM (no 2 GB fp32 round trip, no cast pass); takes precedence over the overlap
        self.fuse_bf16_dp = True
        # F.normalize (mfb.py:105) folded into co_att_conv1's GEMM epilogue: fusion_normed is never written and neither the
        # scale pass nor the sum(Y * dY) pass of its backward runs (functions.NormLink).  fp32 co-attention, single hidden
        # layer only; False materialises fusion_normed as round 2 did
        self.fold_norm = True
        # True: on a PackedRegions (without img_index) everything between the fusion and the pooling -- the fusion's output, co_att_conv1
        # (and the multilayer conv) with their hidden layers and gradients, the logits -- holds the R real rows only; nothing of N*L
        # rows is allocated.  Same parameters, same masks, the result of packed_coatt = False up to summation order inside the GEMMs.
        # No effect on a plain tensor, on the pair (img, img_length) or in the pruned mode; refused together with img_index.
        self.packed_coatt = False
        # True: on a PackedRegions or the pair (img, img_length), without img_index and with gemm_dtype "fp32", img_conv1d and its weight
        # gradient take bf16 operands with fp32 accumulation, dP is stored in bf16 and so is P where the large-tile bf16 GEMM applies
        # (gemm_dtype "bf16-img" on the region layouts; parity 3e-2).  The rows are cast per step; everything else -- the question
        # side, the co-attention head, the pooling, the norms, the masks, the loss -- stays fp32, and the dropout masks are those of
        # the fp32 form.  No effect on a plain tensor or with any other gemm_dtype; refused together with img_index, and for a
        # channel count that is no multiple of 8.
        self.regions_bf16 = False
        # True (with regions_bf16 = True, on the calls where that one takes effect): co_att_conv1's three products -- the forward, dx =
        # d1 W1 and dW1 = d1^T x -- take bf16 operands with fp32 accumulation too, exactly as gemm_dtype "bf16-att" runs them on a
        # plain tensor: the 1/norm row scale in the GEMM epilogue, the fusion kernel's own bf16 copy of R as the operand, the hidden
        # gradient stored in bf16.  The multilayer conv, the logits, the softmax, the pooling, the norms, biases, ReLU and every
        # reduction stay fp32; masks and parameters do not change.  On a region form where regions_bf16 does not apply (it is False,
        # or another gemm_dtype) the call raises VqfError; no effect on a plain tensor or in the pruned mode.
        self.regions_bf16_coatt = False
        # overlap_streams = True only: the persistent image-projection GEMMs use at most this many CUs (a multiple of 8; 0 =
        # all), which leaves the others to the question-side kernels of the main stream (library option gemm_cu_limit)
        self.side_cu_limit = 0
        # bf16 modes keep projection + fusion in ONE node on the caller's stream by default (fuse_bf16_dp); side_bf16 = True
        # lets overlap_streams = True put the bf16 projection on the second stream as well (bf16 P in, bf16 dP out of
        # MfbFuseFn): worth it where the question side is long and idle, i.e. MHBCoAtt's 512-step LSTM recursion
        self.side_bf16 = False
        self._side = _SideStream()
        self._seeds = _DropSeeds()

    # -- helpers -----------------------------------------------------------
    def _mc(self, name):
        m = getattr(self, name, None) if self.multilayer else None
        return (m.weight, m.bias) if m is not None else (None, None)

    def set_keep_masks(self, **masks):
        """Test hook: explicit uint8 keep-masks 'm1' (N*L,5000), 'm2' (N,5000) instead of Philox."""
        self._seeds.keep = masks

    def _forward_pruned(self, img_features, ques_feature, layout=None):
        """The live part of the reference graph when both softmaxes are over a singleton axis."""
        pm = self.dropout_m.p
        qa = UnitPoolFn.apply(ques_feature, 2)                             # (N, 2H)   mfb.py:85-89 with weights 1
        self._seeds.next(self.training, pm)                                # the regions' dropout draw (unused, keeps the stream)
        # (N, 2D)   mfb.py:119-123 with weights 1 (img_length: on the real regions; per image when the images are shared)
        # (packed rows: one sum per owner of the row offsets -- per image when the images are shared)
        va = UnitPoolFn.apply(img_features, 2, layout)
        if layout is not None and layout.grouped:                          # per image (U, 2D), one row block per question
            va = ops.row_block_gather(va, layout.idx)
        y = FinalMfbFn.apply(qa, va, self.ques_proj2.weight, self.ques_proj2.bias,
                             self.img_proj2.weight, self.img_proj2.bias, *self._seeds.draw('m2', self.training, pm))
        out = LinearFn.apply(y, self.linear_pred.weight, self.linear_pred.bias)
        dead = [self.ques_att_conv1, self.ques_att_conv2, self.ques_proj1, self.img_conv1d, self.co_att_conv1,
                self.co_att_conv2]
        if self.multilayer:
            dead += [self.ques_att_multiconv, self.co_att_multiconv]
        params = [t for m in dead for t in (m.weight, m.bias) if t.requires_grad]
        return DeadParamsFn.apply(out, *params) if params and torch.is_grad_enabled() else out

    def forward(self, img_features, questions, is_training=True, img_index=None):
        """img_index (None, or (N,) int64 / int32 on the questions' device): img_features holds the U images the batch's N
        questions share, and question n looks at image img_index[n] (any order, repeats, images without a question).  The
        result is this model on img_features[img_index]; img_conv1d and its weight gradient run once per image.
        Region counts: img_features may be the PAIR (img, img_length) -- what data_loader.pad_region_features returns, moved to
        the GPU -- with img_length an int64 / int32 tensor on the questions' device, one count per image ((N,), or (U,) with
        img_index; fp32 only): img is right-padded to L regions (detector boxes) and image i has img_length[i] real ones, clamped
        to [1, L] on the device.  A plain tensor, or (img, None), is the existing path.
        The result is this model on the first img_length[i] regions of each image: the fusion's L2
        norm, the co-attention softmax (under unit_softmax: the region sum) and every gradient run over the real regions, and
        no padded row of the projection is read.  The padded rows of img_features may hold any FINITE values: img_conv1d and
        its weight gradient still run over all L rows and the padding cancels because its dP rows are exact zeros -- a NaN or
        Inf in a padded row would reach img_conv1d's weight gradient.  data_loader.pad_region_features builds such a batch.
        Packed regions: img_features may be a PackedRegions(rows, offsets, max_regions) -- what data_loader.pack_region_features
        returns, moved to the GPU with .to(device): rows (R, D) fp32 are every image's real regions, one image after the other,
        never padded; offsets (N + 1,), or (U + 1,) per image with img_index, int64 / int32 on the questions' device; max_regions a
        Python int L in [1, 1024], at least the largest count (fp32 only).  The result is this model on (packed.unpack(), ...),
        the region-count call; img_conv1d and its weight gradient run on the R real rows only.
        packed_coatt = True (an attribute, default False): with a PackedRegions and no img_index the co-attention head runs on the R
        real rows as well -- the fusion's output, co_att_conv1's input, hidden layer and gradients, the logits -- and only the
        attention weights keep their (N, 2, L) shape, exact zeros behind each count.  The result is still this model on
        (packed.unpack(), ...), with the dropout masks of the default form.  Together with img_index it raises VqfError; for a plain
        tensor, the pair (img, img_length) and the pruned mode it changes nothing.
        regions_bf16 = True (an attribute, default False): with gemm_dtype "fp32", a PackedRegions or the pair (img, img_length) and
        no img_index, img_conv1d and its weight gradient take bf16 operands with fp32 accumulation (the fp32 rows are cast per
        step), dP is stored in bf16, and so is P where the large-tile bf16 GEMM applies -- gemm_dtype "bf16-img" on the region
        layouts, within 3e-2 of the fp32 form.  Everything else stays fp32: the question side, the co-attention head, the pooling,
        the norms, the loss; the dropout masks are those of the fp32 form.  Together with img_index, or with a channel count that is
        no multiple of 8, it raises VqfError; a plain tensor is not touched, and any other gemm_dtype keeps its meaning.
        regions_bf16_coatt = True (an attribute, default False): on exactly the calls where regions_bf16 takes effect, co_att_conv1's
        forward, input gradient and weight gradient take bf16 operands with fp32 accumulation as well, as gemm_dtype "bf16-att" runs
        them on a plain tensor (within 3e-2 of regions_bf16 alone).  The multilayer conv, the logits, the masked softmax, the
        pooling, the norms, the question side, the final blocks and the loss stay fp32; masks, parameters and the (N, 2, L)
        attention weights with exact zeros behind each count do not change.  On a PackedRegions or a pair (img, img_length) where
        regions_bf16 does not apply -- regions_bf16 = False, or a gemm_dtype other than "fp32" -- it raises VqfError before the first
        launch (no silent fp32 head); a plain tensor and the pruned mode are not touched."""
        coatt_regions = bool(self.regions_bf16_coatt) and not (self.pruned and self.unit_softmax)
        regions_bf16_coatt_check("MFB", img_features, img_index, self.gemm_dtype, self.regions_bf16 and self.img_conv1d.out_channels,
                                 coatt_regions)
        img_features, img3, L, layout = fusion_region_layout("MFB", img_features, questions, img_index, self.gemm_dtype,
                                                             self.packed_coatt, self.regions_bf16 and self.img_conv1d.out_channels)
        bf16_regions = regions_bf16_on(self.regions_bf16, self.gemm_dtype, layout)
        coatt_regions = coatt_regions and bf16_regions
        bf16_img = bf16_regions or self.gemm_dtype in ("bf16", "bf16-img", "bf16-all")
        bf16_all = self.gemm_dtype == "bf16-all"          # also ques_proj*, img_proj*, the question-attention conv
        # a5 starts first where it is its own node; the pruned mode has no projection
        proj = None if (self.pruned and self.unit_softmax) else project_aside(self, img3, bf16_img, bf16_regions)
        # a2: question encoder                                               mfb.py:68-70
        # (the lookup writes (T,N,E) directly when the recursion runs on the HIP path: no transposing copy in between)
        tm = questions.dim() == 2 and hip_batch_lstm_ok(self.lstm, questions.is_cuda and self.word_embedding.weight.dtype == torch.float32,
                                                        self.use_hip_lstm)
        que_embedded = embed_tanh(self.word_embedding, questions, time_major=tm)
        lstm_o = batch_first_lstm(self.lstm, que_embedded, self.use_hip_lstm, _lstm_bf16(self.gemm_dtype), time_major_in=tm)
        ques_feature = lstm_out_dropout(self.dropout_l, lstm_o, self._seeds)   # (N,T,H) contiguous; mfb.py:70
        N, T, H = ques_feature.shape
        if self.pruned and self.unit_softmax:
            return self._forward_pruned(img_features, ques_feature, layout)

        # a3: question attention                                             mfb.py:73-89
        wm, bm = self._mc('ques_att_multiconv')
        qa = AttHeadFn.apply(ques_feature.view(N * T, H), ques_feature,
                             self.ques_att_conv1.weight, self.ques_att_conv1.bias, wm, bm,
                             self.ques_att_conv2.weight, self.ques_att_conv2.bias, self.unit_softmax, bf16_all, None, True)
        # a4: ques_proj1                                                     mfb.py:92-93
        qp = LinearFn.apply(qa, self.ques_proj1.weight, self.ques_proj1.bias, False, bf16_all)
        # a5+a6: image projection + MFB fusion over the regions             mfb.py:95-106
        pm = self.dropout_m.p
        coatt_bf16 = coatt_regions or self.gemm_dtype in ("bf16", "bf16-att", "bf16-all")
        link = NormLink(want_xb=coatt_regions) if (self.fold_norm and not self.multilayer) else None
        Y = join_or_fuse(self, proj, img3, qp, self._seeds.draw('m1', self.training, pm), bf16_img, N, L, link, layout)
        # a7+a8: co-attention over the regions                               mfb.py:109-123
        # (with a link Y is the un-normalised R and 1/norm rides in co_att_conv1's GEMM epilogue)
        wm, bm = self._mc('co_att_multiconv')
        va = AttHeadFn.apply(Y, img_features, self.co_att_conv1.weight, self.co_att_conv1.bias, wm, bm,
                             self.co_att_conv2.weight, self.co_att_conv2.bias, self.unit_softmax, coatt_bf16, link, False, layout)
        # a9: final MFB block                                                mfb.py:126-135
        y = FinalMfbFn.apply(qa, va, self.ques_proj2.weight, self.ques_proj2.bias, self.img_proj2.weight, self.img_proj2.bias,
                             *self._seeds.draw('m2', self.training, pm), None, False, bf16_all)
        # a10: classifier; the reference computes a softmax and discards it  mfb.py:137-140
        return LinearFn.apply(y, self.linear_pred.weight, self.linear_pred.bias)

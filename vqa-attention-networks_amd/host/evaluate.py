"""The solver's evaluation tail on the HIP path: prediction, accuracy, validation totals, top-k answers.

The reference's loop goes on after the criterion (solver.py:96-101, and the same lines in val(), :146-153):
    pred = F.softmax(logits, dim=1); pred = pred.max(1)[1]
    a = a.max(1)[1]                                   # mhb / mhb_coAtt only
    acc = (pred == a).float().mean(); total_acc += (pred == a).sum(dtype=torch.float32)
The arg-max of a softmax is the arg-max of its input, so none of this needs a pass of its own: with the cross-entropy
criterion the prediction and the hit count ride in the loss kernel's row pass (ops.ce_loss_pred), with the KL criterion one
row pass over log-probs and soft targets follows the loss (ops.answer_match_rows); a validation epoch accumulates on the
device and is read back once.  Ties go to the lowest index and a NaN row predicts its first NaN, as torch.max does.
"""
import torch

from . import ops
from .lib import VqfError
from .train_step import BCEWithLogitsLoss, CrossEntropyLoss, KLDivLoss, _KlDivLossFn, _bce_scale, _bce_target, _times


class _CeLossPredFn(torch.autograd.Function):
    """_CeLossFn of train_step.py (the same loss and gradient bits) that also returns the prediction and the accuracy"""

    @staticmethod
    def forward(ctx, logits, target):
        acc = torch.empty(1, dtype=torch.float32, device=logits.device)
        loss, d, pred = ops.ce_loss_pred(logits.contiguous(), target, want_grad=logits.requires_grad, acc=acc)
        ctx.save_for_backward(d)
        acc = acc.view(())
        ctx.mark_non_differentiable(pred, acc)
        return loss.view(()), pred, acc

    @staticmethod
    def backward(ctx, g, _gpred, _gacc):
        (d,) = ctx.saved_tensors
        return _times(d, g), None


class _BceLossPredFn(torch.autograd.Function):
    """_BceLossFn of train_step.py (the same loss and gradient bits) that also returns the prediction and the mean soft score"""

    @staticmethod
    def forward(ctx, logits, target, per_row):
        want_grad = logits.requires_grad      # of the incoming tensor, as in _BceLossFn
        logits = logits.contiguous()
        acc = torch.empty(1, dtype=torch.float32, device=logits.device)
        loss, d, pred, _ = ops.bce_logits_loss(logits, _bce_target(target), _bce_scale(logits, per_row), want_grad=want_grad,
                                               acc=acc)
        ctx.save_for_backward(d)
        acc = acc.view(())
        ctx.mark_non_differentiable(pred, acc)
        return loss.view(()), pred, acc

    @staticmethod
    def backward(ctx, g, _gpred, _gacc):
        (d,) = ctx.saved_tensors
        return _times(d, g), None, None


def loss_and_accuracy(criterion, logits, a):
    """solver.py:91 and :96-101 in one call -> (loss, pred, acc).

    loss: the differentiable scalar `criterion(logits, a)` gives (same bits, same gradient bits); pred (N,) int64; acc a
    0-dim fp32 GPU tensor, hits / counted rows (rows with target -100 do not count; no counted row: NaN, like the mean of an
    empty tensor).  pred and acc are not differentiable.  `criterion` is this package's CrossEntropyLoss (a (N,) int64),
    KLDivLoss (a (N, A) soft targets, compared through a.max(1)[1] as solver.py:100 does) or BCEWithLogitsLoss (a (N, A) soft
    scores or a SoftAnswers; acc is then the mean soft score a[n, pred[n]] of the predicted answers, the VQA accuracy, from
    the loss kernel's own row pass); anything else raises."""
    if isinstance(criterion, BCEWithLogitsLoss):
        return _BceLossPredFn.apply(logits, a, criterion.reduction == "batchmean")
    if isinstance(criterion, CrossEntropyLoss):
        return _CeLossPredFn.apply(logits, a)
    if isinstance(criterion, KLDivLoss):
        loss = _KlDivLossFn.apply(logits, a)
        acc = torch.empty(1, dtype=torch.float32, device=logits.device)
        pred, _, _ = ops.answer_match_rows(logits.detach().contiguous(), a.contiguous(), want_score=False, acc=acc)
        return loss, pred, acc.view(())
    raise VqfError("loss_and_accuracy: criterion must be vqa_amd.CrossEntropyLoss, vqa_amd.KLDivLoss or "
                   "vqa_amd.BCEWithLogitsLoss, got %s (there is no torch route)" % type(criterion).__name__)


class Evaluator:
    """val() of solver.py:119-178 without a host read per batch.

        ev = Evaluator(criterion)
        for batch in loader: ev.update(model(...), a)        # device-side accumulation, no synchronisation
        r = ev.result()                                        # ONE device-to-host copy

    result() -> {"correct": int, "rows": int, "accuracy": correct / rows, "loss_mean": the mean loss over all rows seen,
    "loss_last": the last batch's loss (what val() returns in training mode)}, plus "vqa_score" with the KL criterion: the
    mean soft score target[n, pred[n]] of the predicted answers.  With no row seen the means are NaN.

    `accuracy` differs from solver.py:177 on purpose: the reference divides the hits by len(loader) * batch_size, which counts
    rows a short last batch does not have; here the divisor is the rows actually seen (with the cross-entropy criterion: the
    rows whose target is not -100).  loss_mean weights every batch by its rows.
    The totals are three device scalars (hits and rows as int64, sums as float64) per process; summing them over the ranks of a
    multi-GPU run (one all-reduce of the buffer) is left to the caller.

    With BCEWithLogitsLoss (a: (N, A) soft scores or a SoftAnswers) update() is ONE call of the loss kernel, and result() ->
    {"rows", "vqa_score": the mean soft score of the predicted answers, "accuracy": the same number (one key for every
    criterion), "loss_mean", "loss_last"}; there is no "correct": a soft score is not a hit count.  Its totals live in a buffer
    of their own (rows int64 | score sum, loss sum float64 | last loss fp32)."""

    def __init__(self, criterion):
        if not isinstance(criterion, (CrossEntropyLoss, KLDivLoss, BCEWithLogitsLoss)):
            raise VqfError("Evaluator: criterion must be vqa_amd.CrossEntropyLoss, vqa_amd.KLDivLoss or "
                           "vqa_amd.BCEWithLogitsLoss, got %s (there is no torch route)" % type(criterion).__name__)
        self.soft = isinstance(criterion, KLDivLoss)
        self.bce = isinstance(criterion, BCEWithLogitsLoss)
        self._per_row = self.bce and criterion.reduction == "batchmean"
        self._buf = None

    def _bce_views(self, device):
        # four 8-byte slots: rows (int64) | score sum, loss sum (float64) | last loss (fp32)
        if self._buf is None or self._buf.device != device:
            self._buf = torch.zeros(4, dtype=torch.int64, device=device)
        b = self._buf
        return b[0:1], b[1:2].view(torch.float64), b[2:3].view(torch.float64), b[3:4].view(torch.float32)[0:1]

    def _views(self, device):
        # one buffer of five 8-byte slots: hits, rows (int64) | loss sum, score sum (float64) | last loss (fp32)
        if self._buf is None or self._buf.device != device:
            self._buf = torch.zeros(5, dtype=torch.int64, device=device)
        b = self._buf
        return b[0:2], b[2:3].view(torch.float64), b[3:4].view(torch.float64), b[4:5].view(torch.float32)[0:1]

    @torch.no_grad()
    def update(self, logits, a):
        logits = logits.detach().contiguous()
        if self.bce:
            ops._chk(logits)       # a CPU tensor is refused before the totals are placed on its device
            scale = _bce_scale(logits, self._per_row)
            rows, score_sum, loss_sum, last = self._bce_views(logits.device)
            ops.bce_logits_loss(logits, _bce_target(a), scale, want_grad=False, want_pred=False, rows=rows, score_sum=score_sum,
                                loss_sum=loss_sum, accumulate=True, loss_out=last)
            return
        counts, loss_sum, score_sum, last = self._views(logits.device)
        if self.soft:
            a = a.contiguous()
            ops.kldiv_loss(logits, a, want_grad=False, loss_out=last)
            ops.answer_match_rows(logits, a, want_score=False, counts=counts, score_sum=score_sum, loss=last,
                                  loss_sum=loss_sum, accumulate=True)
        else:
            ops.ce_loss_pred(logits, a, want_grad=False, want_pred=False, counts=counts, loss_sum=loss_sum,
                             accumulate=True, loss_out=last)

    def reset(self):
        if self._buf is not None:
            self._buf.zero_()

    def result(self):
        if self.bce:
            h = self._buf.cpu() if self._buf is not None else torch.zeros(4, dtype=torch.int64)
            rows, nan = int(h[0]), float("nan")
            score = float(h[1:2].view(torch.float64)[0]) / rows if rows else nan
            return {"rows": rows, "vqa_score": score, "accuracy": score,
                    "loss_mean": float(h[2:3].view(torch.float64)[0]) / rows if rows else nan,
                    "loss_last": float(h[3:4].view(torch.float32)[0]) if rows else nan}
        h = self._buf.cpu() if self._buf is not None else torch.zeros(5, dtype=torch.int64)
        correct, rows = int(h[0]), int(h[1])
        nan = float("nan")
        r = {"correct": correct, "rows": rows, "accuracy": correct / rows if rows else nan,
             "loss_mean": float(h[2:3].view(torch.float64)[0]) / rows if rows else nan,
             "loss_last": float(h[4:5].view(torch.float32)[0]) if rows else nan}
        if self.soft:
            r["vqa_score"] = float(h[3:4].view(torch.float64)[0]) / rows if rows else nan
        return r


def topk_answers(logits, k=5):
    """logits (N, A) fp32 (or log-probs: their softmax is the same distribution) -> (ids (N, k) int64, probs (N, k) fp32), the
    k most likely answers of every row with their softmax probabilities, most likely first.  A (W, k) the kernel does not
    take raises VqfError."""
    x = logits.detach()
    if x.dim() == 2 and x.stride(1) != 1:
        x = x.contiguous()
    return ops.topk_rows(x, k, mode=1)


def predict(model, img, q, q_length=None, k=5, **fwd_kwargs):
    """'What are the k most likely answers, and how sure is the model?' -> (ids (N, k) int64, probs (N, k) fp32).
    Runs `model` in eval() mode (dropout off) under torch.no_grad() and puts its `training` flag back; q_length is passed
    only when given; HieCoAtten / HieCoAttenLadder return (logits, attention maps...): the first element is used.
    Further keyword arguments go to the model's forward: predict(model, img (U, L, D), q (N, T), q_length, img_index=idx) asks
    HieCoAttenLadder N questions about U shared images (idx (N,): the image of each question); predict(model, (img, img_length),
    q) asks MFB / MHBCoAtt / HieCoAttenLadder about right-padded region features (img_length: the real regions of each image);
    predict(model, PackedRegions(rows, offsets, max_regions), q) asks MFB / MHBCoAtt / HieCoAttenLadder about region features that were never padded."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            args = (img, q) if q_length is None else (img, q, q_length)
            out = model(*args, **fwd_kwargs)
    finally:
        model.train(was_training)
    if isinstance(out, (tuple, list)):
        out = out[0]
    return topk_answers(out, k)

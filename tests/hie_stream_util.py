"""Shared helpers of the element-wise kernel tests (tests/test_gpu_hie_stream.py, tests/test_gpu_hie_small_kernels.py): seeded fp32
operands, sentinel-filled destination buffers with guard rows / columns, and the per-element comparison against a (value, bound)
pair of tests/hie_stream_ref.py with its worst err / bound reported the way golden_util._report_parity does."""
import torch

from golden_util import _report_parity

SENT = -777.25


def _vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


def _r(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


def _views(rows, W, wide, n=2):
    """n (rows, W) destinations / operands: column blocks of ONE (rows + 2, n W) sentinel buffer (wide), or n contiguous buffers,
    each with a guard row above and below -> (buffers, views)"""
    if wide:
        full = torch.full((rows + 2, n * W), SENT, device="cuda")
        return [full], [full[1:-1, j * W:(j + 1) * W] for j in range(n)]
    fulls = [torch.full((rows + 2, W), SENT, device="cuda") for _ in range(n)]
    return fulls, [f[1:-1] for f in fulls]


def _only(fulls, *views):
    """nothing but `views` changed in the sentinel buffers"""
    saved = [v.clone() for v in views]
    for v in views:
        v.fill_(SENT)
    ok = all(bool((f == SENT).all()) for f in fulls)
    for v, s in zip(views, saved):
        v.copy_(s)
    return ok


class Report:
    def __init__(self, shape, wide):
        self.tag, self.worst = "%s %s" % (shape, "blocks" if wide else "contig"), {}

    def check(self, name, got, ref_bound):
        ref, bound = ref_bound
        got = got.detach().contiguous().cpu().double().reshape(ref.shape)
        err = (got - ref).abs()
        bad = ~(err <= bound)                                  # (a NaN fails)
        if bool(bad.any()):
            idx = bad.nonzero()[:6].tolist()
            raise AssertionError("%s %s: %d of %d elements off; first (index, got, ref, bound): %s" % (
                self.tag, name, int(bad.sum()), bad.numel(),
                [(i, float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]))
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
        self.worst[name] = max(self.worst.get(name, 0.0), ratio)

    def flush(self):
        for pass_ in sorted({k.split(".")[0] for k in self.worst}):
            items = {k: v for k, v in self.worst.items() if k.split(".")[0] == pass_}
            name = max(items, key=items.get)
            _report_parity("hie_stream %-10s %s" % (pass_, self.tag), items[name], name,
                           "  " + " ".join("%s=%.3f" % (k.split(".", 1)[1], v) for k, v in sorted(items.items())))

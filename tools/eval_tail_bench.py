"""The solver's evaluation tail (solver.py:91, 96-101) on the MI355X: the fused route against the route it replaces.

    python tools/eval_tail_bench.py [--repeats 9] [--inner 200] [--out FILE]

For (N, A) = (512, 5000) and (256, 3000), in ONE process, alternating the two routes inside every repeat:

  ce tail     fused : ops.ce_loss_pred  -- loss, dlogits, pred and acc from the loss kernel's row pass (2 launches)
              parent: ops.ce_loss, then the four torch ops of solver.py:96-101
                      (F.softmax, .max(1)[1], ==, .float().mean())
  kl tail     fused : ops.kldiv_loss + ops.answer_match_rows           (the soft-target models)
              parent: ops.kldiv_loss, then F.softmax, .max(1)[1], a.max(1)[1], ==, .float().mean()
  top-5       fused : ops.topk_rows(k=5, mode=1)
              torch : torch.topk(F.softmax(x, dim=1), 5)

A sample is the device time of `inner` back-to-back calls between two events, divided by `inner`: the calls are enqueued eagerly,
as the solver enqueues them, so a route made of many short launches also pays the launch gaps it causes.  Every route is warmed
up first; the table gives the median over the repeats and their spread (min .. max).  The expectation checked at the end:
the fused route's median is not above the parent route's median by more than the parent's own spread.
Bytes: the fused ce tail adds no pass over the logits (the arg-max rides in the loss kernel's own row pass); the parent's
tail adds a softmax (read + write), a max (read) and two short passes over (N,) vectors."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vqa_amd  # noqa: E402


def _sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # microseconds per call


def _ab(routes, repeats, inner):
    """routes: {name: fn}; alternates them inside every repeat -> {name: [us per call] * repeats}"""
    for fn in routes.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            out[k].append(_sample(fn, inner))
    return out


def _row(name, v):
    return "  %-34s median %8.2f us   min %8.2f   max %8.2f" % (name, statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_tail_bench.py measures on the MI355X; no GPU found")
    vqa_amd.build()
    ops = vqa_amd.ops
    dev = "cuda:0"
    lines, verdicts = [], {}

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("eval tail on %s, torch %s; %d repeats x %d calls per sample" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                       args.repeats, args.inner))
    for N, A in ((512, 5000), (256, 3000)):
        g = torch.Generator().manual_seed(N + A)
        logits = (torch.randn(N, A, generator=g) * 2).to(dev)
        hard = torch.randint(0, A, (N,), generator=g).to(dev)
        logp = torch.log_softmax(logits, dim=1)
        soft = torch.softmax(torch.randn(N, A, generator=g), dim=1).to(dev)
        acc = torch.empty(1, dtype=torch.float32, device=dev)

        def ce_fused():
            return ops.ce_loss_pred(logits, hard, want_grad=True, acc=acc)

        def ce_parent():
            loss, d = ops.ce_loss(logits, hard, want_grad=True)
            pred = F.softmax(logits, dim=1)
            pred = pred.max(1)[1]
            return loss, d, pred, (pred == hard).float().mean()

        def kl_fused():
            loss, d = ops.kldiv_loss(logp, soft, want_grad=True)
            return loss, d, ops.answer_match_rows(logp, soft, want_score=False, acc=acc)

        def kl_parent():
            loss, d = ops.kldiv_loss(logp, soft, want_grad=True)
            pred = F.softmax(logp, dim=1)
            pred = pred.max(1)[1]
            a = soft.max(1)[1]
            return loss, d, pred, (pred == a).float().mean()

        def topk_fused():
            return ops.topk_rows(logits, 5, mode=1)

        def topk_torch():
            return torch.topk(F.softmax(logits, dim=1), 5)

        # the routes agree before they are timed
        _, d0, p0, a0 = ce_parent()
        _, d1, p1 = ce_fused()
        assert torch.equal(p0, p1) and torch.equal(d0, d1) and abs(acc.item() - a0.item()) < 1e-7
        _, _, pk, ak = kl_parent()
        _, _, (pf, _, _) = kl_fused()
        assert torch.equal(pk, pf) and abs(acc.item() - ak.item()) < 1e-7
        ti, tv = topk_torch()[1], topk_torch()[0]
        fi, fv = topk_fused()
        assert torch.equal(ti, fi) and ((tv - fv).abs() / tv).max().item() < 1e-4

        say()
        say("N = %d, A = %d (logits %.1f MB)" % (N, A, N * A * 4 / 1e6))
        for title, pair in (("ce tail", {"fused: ce_loss_pred": ce_fused, "parent: ce_loss + 4 torch ops": ce_parent}),
                            ("kl tail", {"fused: kldiv + answer_match_rows": kl_fused, "parent: kldiv + 5 torch ops": kl_parent}),
                            ("top-5", {"fused: topk_rows(mode=1)": topk_fused, "torch: topk(softmax)": topk_torch})):
            res = _ab(pair, args.repeats, args.inner)
            (fk, fvs), (pk_, pvs) = res.items()
            say(" %s" % title)
            say(_row(fk, fvs))
            say(_row(pk_, pvs))
            spread = max(pvs) - min(pvs)
            ok = statistics.median(fvs) <= statistics.median(pvs) + spread
            verdicts["%s N=%d A=%d" % (title, N, A)] = {"fused_us": statistics.median(fvs), "other_us": statistics.median(pvs),
                                                        "other_spread_us": spread, "fused_not_slower": ok}
            say("  -> fused / other = %.2f; other route's spread %.2f us; fused not slower beyond it: %s"
                % (statistics.median(fvs) / statistics.median(pvs), spread, "yes" if ok else "NO"))
    say()
    say(json.dumps({"eval_tail_bench": verdicts}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

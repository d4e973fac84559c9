"""BCE-with-logits on soft answers on the MI355X: this package's two target forms against the torch route they replace.

    python tools/soft_loss_bench.py [--rounds 2] [--repeats 7] [--inner 200] [--out FILE]

N = 512, A in {1000, 3000}, K = 10 slots; ONE process, the forms alternating inside every repeat:

  dense   ops.bce_logits_loss(logits, target (N, A))      loss + dlogits + pred + score + this call's mean score (2 launches)
  sparse  ops.bce_logits_loss(logits, SoftAnswers)        the same, the target as (N, K) ids + scores
  torch   F.binary_cross_entropy_with_logits, its backward to the logits (autograd.grad), argmax, gather, mean
  copy    host-to-device: the dense (N, A) fp32 target from pinned memory against SoftAnswers.to(device) from pinned memory

A sample is the device time of `inner` back-to-back calls between two events, divided by `inner`: the calls are enqueued eagerly,
as a solver enqueues them, so a route made of several short launches also pays the gaps between them.  Every route is warmed up
first.  A round gives the median over its repeats; the table prints the median of the rounds' medians and every round's median.

This is not a step-time feature: the row pass moves 2 N A 4 bytes (12.3 MB at N = 512, A = 3000), a few microseconds at the HBM
rates DESIGN.md quotes, so launches dominate.  That expectation is DERIVED from shapes; what this tool prints is MEASURED."""
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


def _rounds(routes, rounds, repeats, inner):
    """routes: {name: fn}; alternates them inside every repeat -> {name: [median us per call of each round]}"""
    for fn in routes.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for _ in range(rounds):
        samples = {k: [] for k in routes}
        for _ in range(repeats):
            for k, fn in routes.items():
                samples[k].append(_sample(fn, inner))
        for k in routes:
            out[k].append(statistics.median(samples[k]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_loss_bench.py measures on the MI355X; no GPU found")
    vqa_amd.build()
    ops = vqa_amd.ops
    dev = "cuda:0"
    lines, result = [], {}

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("soft-answer loss on %s, torch %s; %d rounds x %d repeats x %d calls per sample"
        % (torch.cuda.get_device_name(0), torch.__version__, args.rounds, args.repeats, args.inner))
    N, K = 512, 10
    for A in (1000, 3000):
        g = torch.Generator().manual_seed(A)
        logits = (torch.randn(N, A, generator=g) * 2).to(dev)
        ids = torch.stack([torch.randperm(A, generator=g)[:K] for _ in range(N)])
        scores = torch.tensor([0.3, 0.6, 0.9, 1.0])[torch.randint(0, 4, (N, K), generator=g)]
        soft_host = vqa_amd.SoftAnswers(ids.pin_memory(), scores.pin_memory())
        dense_host = vqa_amd.SoftAnswers(ids, scores).dense(A).pin_memory()
        soft, dense = soft_host.to(dev), dense_host.to(dev)
        acc = torch.empty(1, dtype=torch.float32, device=dev)
        c = 1.0 / (N * A)
        xg = logits.clone().requires_grad_(True)

        def pkg_dense():
            return ops.bce_logits_loss(logits, dense, c, acc=acc)

        def pkg_sparse():
            return ops.bce_logits_loss(logits, soft, c, acc=acc)

        def torch_route():
            loss = F.binary_cross_entropy_with_logits(xg, dense)
            (d,) = torch.autograd.grad(loss, xg)
            pred = torch.argmax(logits, dim=1)
            return loss, d, pred, dense.gather(1, pred.unsqueeze(1)).mean()

        def copy_dense():
            return dense_host.to(dev, non_blocking=True)

        def copy_sparse():
            return soft_host.to(dev, non_blocking=True)

        # the routes agree before they are timed
        l0, d0, p0, a0 = torch_route()
        for fn in (pkg_dense, pkg_sparse):
            l1, d1, p1, _ = fn()
            assert torch.equal(p0, p1) and abs(acc.item() - a0.item()) < 1e-6
            assert abs(l1.item() - l0.item()) < 1e-5 * abs(l0.item()) and (d1 - d0).abs().max().item() < 1e-5 * c

        say()
        say("N = %d, A = %d, K = %d (logits %.1f MB, dense target %.1f MB, SoftAnswers %.3f MB)"
            % (N, A, K, N * A * 4 / 1e6, N * A * 4 / 1e6, N * K * 12 / 1e6))
        res = _rounds({"package, dense target": pkg_dense, "package, SoftAnswers": pkg_sparse,
                       "torch: bce + grad + argmax + gather + mean": torch_route,
                       "H2D copy, dense target (pinned)": copy_dense, "H2D copy, SoftAnswers (pinned)": copy_sparse},
                      args.rounds, args.repeats, args.inner)
        for k, v in res.items():
            say("  %-46s median %8.2f us   rounds: %s" % (k, statistics.median(v), "  ".join("%.2f" % r for r in v)))
        result["A=%d" % A] = {k: statistics.median(v) for k, v in res.items()}
    say()
    say(json.dumps({"soft_loss_bench": result}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Region counts (forward((img, img_length), ...)): what the fusion kernels and the train step cost with right-padded region features.

    python tools/mfb_regions_bench.py [--batch 512] [--regions 100] [--steps 8] [--warmup 3] [--repeats 5] [--plain-only]
                                      [--models mfb,mhbcoatt] [--out profiles/mfb_regions_bench.txt]

Kernel part (N = --batch, L = --regions, O = 1000, fp32, Philox dropout 0.1): mfb_fuse_fwd / mfb_fuse_bwd
  without lens, with lens = L everywhere, and with counts drawn uniformly from 10 .. L (seed 1), each as the median of --repeats
  windows of --steps launches (device events) with the spread (max - min) of the windows, and as achieved GB/s over the bytes of
  its REAL rows (fwd: P read + R written; bwd: P, dY, Y read + dP written).  The expectation under test: time ~ sum(counts).
  --plain-only runs the legs without lens only: that part uses nothing this feature added, so the same file run from a checkout
  of the commit before it gives the yardstick the "without lens" figures have to agree with (within the spread).
Model part: the train step (bench.py's: forward, loss, backward, the project's Adam) of MFB (live softmax) and MHBCoAtt on the
  same padded tensor with the counts, forward((img, img_length), ...), beside the plain tensor.
"""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vqa_amd  # noqa: E402

D, H, E, T, V, A, O = 2048, 1024, 300, 14, 1000, 1000, 1000


def windows(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    w = []
    for _ in range(max(1, repeats)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        w.append(a.elapsed_time(b) / steps)
    return sorted(w)[len(w) // 2], max(w) - min(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", default="mfb,mhbcoatt")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, L, dev = a.batch, a.regions, "cuda:0"
    ops = vqa_amd.ops
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("region counts: fusion kernels and train step   N=%d L=%d O=%d fp32   %s" % (N, L, O, torch.cuda.get_device_name(0)))
    say("  median of %d windows of %d launches / steps after %d warm-up; spread = max - min of the windows" % (a.repeats, a.steps, a.warmup))
    g = torch.Generator().manual_seed(1)
    counts = torch.randint(10, L + 1, (N,), generator=g)
    P = torch.rand(N * L, 5 * O, generator=g).to(dev)
    q = (torch.rand(N, 5 * O, generator=g) - 0.5).to(dev)
    pb = torch.rand(5 * O, generator=g).to(dev)
    dY = (torch.rand(N * L, O, generator=g) - 0.5).to(dev)
    legs = [("without lens", None, N * L)]
    if not a.plain_only:
        legs += [("lens = L", torch.full((N,), L, dtype=torch.int32, device=dev), N * L),
                 ("lens ~ U[10, %d]" % L, counts.to(torch.int32).to(dev), int(counts.sum()))]
    say()
    say("sum(counts) / (N L) = %.3f" % (float(counts.sum()) / (N * L)))
    say("%-18s  fwd ms (spread)   GB/s real rows   bwd ms (spread)   GB/s real rows" % "mfb_fuse")
    base = None
    for name, lens, rows in legs:
        kw = dict(seed=7, p_drop=0.1, pbias=pb)
        if lens is not None:
            kw["lens"] = lens
        Y, norm, inv, _ = ops.mfb_fuse_fwd(P, q, N, L, O, **kw)
        f_ms, f_sp = windows(lambda: ops.mfb_fuse_fwd(P, q, N, L, O, normalise=False, **kw), a.steps, a.warmup, a.repeats)
        b_ms, b_sp = windows(lambda: ops.mfb_fuse_bwd(dY, Y, norm, inv, P, q, N, L, O, want_dbias=True, **kw), a.steps, a.warmup, a.repeats)
        fb, bb = rows * (5 * O + O) * 4, rows * (2 * 5 * O + 2 * O) * 4
        say("%-18s  %7.3f (%.3f)   %8.0f         %7.3f (%.3f)   %8.0f" % (name, f_ms, f_sp, fb / f_ms / 1e6, b_ms, b_sp, bb / b_ms / 1e6))
        if base is None:
            base = (f_ms, b_ms)
        else:
            say("%-18s  time / without lens: fwd %.3f  bwd %.3f   (rows / (N L) = %.3f)" % ("", f_ms / base[0], b_ms / base[1], rows / (N * L)))
    say("  (the forward is timed without the scale pass, the backward with its rowdot / coefficient passes and the bias reduce in front"
        " and behind: fixed costs that do not shrink with the counts)")
    del P, dY
    torch.cuda.empty_cache()
    if not a.plain_only:
        say()
        say("%-9s  with counts ms/step (spread)   plain ms/step (spread)   counts / plain" % "train step")
        for name in a.models.split(","):
            cfg = types.SimpleNamespace(q_vocab_size=V, a_vocab_size=A, emb_dim=E, hidden_dim=H, num_layers=1, glove=False,
                                        model_name="mfb" if name == "mfb" else "mhb_coAtt", img_feature_channel=D, img_feature_dim=L)
            torch.manual_seed(0)
            model = (vqa_amd.MFB if name == "mfb" else vqa_amd.MHBCoAtt)(cfg)
            for n_, p_ in model.named_parameters():
                if n_.find("bias") == -1 and p_.dim() > 1:
                    torch.nn.init.xavier_uniform_(p_)
            model = model.to(dev).train()
            if name == "mfb":
                model.unit_softmax = False
            ids = torch.randint(1, V, (N, T), generator=g).to(dev)
            target = (torch.randint(0, A, (N,), generator=g) if name == "mfb" else torch.softmax(torch.randn(N, A, generator=g), 1)).to(dev)
            img = torch.rand(N, L, D, generator=g).to(dev)
            crit = vqa_amd.CrossEntropyLoss() if name == "mfb" else vqa_amd.KLDivLoss()
            opt = vqa_amd.Adam(model.parameters(), lr=1e-4)
            res = []
            for il in (counts.to(dev), None):
                def step():
                    opt.zero_grad(set_to_none=True)
                    crit(model(img if il is None else (img, il), ids), target).backward()
                    opt.step()
                res.append(windows(step, a.steps, a.warmup, a.repeats))
            say("%-9s  %9.3f (%.3f)            %9.3f (%.3f)       %6.3f" % (name, res[0][0], res[0][1], res[1][0], res[1][1], res[0][0] / res[1][0]))
            del model, opt, img
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

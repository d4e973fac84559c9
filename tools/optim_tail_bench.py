"""The optimizer tail of a train step: gradient-norm clipping + the update, on the parameter set of the bench.py headline model.

    python tools/optim_tail_bench.py [--forms a,b,c,d,e,f] [--steps 200] [--warmup 20] [--rounds 2] [--max-norm 0.25]
                                     [--out profiles/optim_tail_bench.txt]

Setup: one fp32 GPU tensor per parameter of MFB(bench.full_cfg()) (the shapes only: no forward runs here), seeded values and
seeded gradients, every form on its own copy.  The forms named in --forms run ALTERNATELY in one process (form a's window,
form b's window, ..., --rounds times) after --warmup steps of each; a window is --steps calls between two device events.
Reported per form: the median window (us / call), the spread (max - min) of its windows.
  a   torch.nn.utils.clip_grad_norm_ + vqa_amd.Adam.step()
  b   vqa_amd.clip_grad_norm_ + vqa_amd.Adam.step()              (norm, scale, update: three kinds of launches)
  c   vqa_amd.Adam(max_grad_norm=M).step()                       (norm, update)
  d   vqa_amd.Adam.step()                                        (the plain update: nothing this tool measures is new in it)
  e   torch.nn.utils.clip_grad_norm_ + torch.optim.Adamax.step()
  f   vqa_amd.Adamax(max_grad_norm=M).step()
--forms d uses nothing newer than vqa_amd.Adam: the same file run from a checkout of an earlier commit gives the yardstick the plain
path has to stay inside.  Derived from the bytes per element (Adam 16 read + 12 written, the norm 4 read): c - d = 4/28 of d; the
tool prints that beside the measurement.  A kernel trace, to see where a larger surplus goes, is taken in a run of its own.
Needs the GPU: there is no other path."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import vqa_amd  # noqa: E402

FORMS = ("a", "b", "c", "d", "e", "f")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-norm", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    forms = a.forms.split(",")
    assert forms and all(f in FORMS for f in forms)
    if not torch.cuda.is_available():
        raise SystemExit("optim_tail_bench.py needs the GPU (the HIP path is the only one)")
    dev, M = "cuda:0", a.max_norm
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    shapes = [tuple(p.shape) for p in vqa_amd.MFB(bench.full_cfg()).parameters()]
    elems = sum(int(torch.Size(s).numel()) for s in shapes)
    say("optimizer tail on the MFB headline parameter set   %d tensors, %d elements (%.1f MB fp32)   %s"
        % (len(shapes), elems, elems * 4 / 1e6, torch.cuda.get_device_name(0)))
    say("  forms %s alternating, %d rounds of one window of %d calls each after %d warm-up calls; spread = max - min of a form's windows"
        % (a.forms, a.rounds, a.steps, a.warmup))

    def make(form):
        g = torch.Generator().manual_seed(7)
        ps = []
        for s in shapes:
            p = torch.nn.Parameter(((torch.rand(s, generator=g) - 0.5) * 0.1).to(dev))
            p.grad = ((torch.rand(s, generator=g) - 0.5) * 0.02).to(dev)
            ps.append(p)
        if form in ("a", "b", "d"):
            opt = vqa_amd.Adam(ps, lr=1e-4)
        elif form == "c":
            opt = vqa_amd.Adam(ps, lr=1e-4, max_grad_norm=M)
        elif form == "e":
            opt = torch.optim.Adamax(ps, lr=1e-4)
        else:
            opt = vqa_amd.Adamax(ps, lr=1e-4, max_grad_norm=M)
        if form in ("a", "e"):
            def call():
                torch.nn.utils.clip_grad_norm_(ps, M)
                opt.step()
        elif form == "b":
            def call():
                vqa_amd.clip_grad_norm_(ps, M)
                opt.step()
        else:
            call = opt.step
        return call

    calls = {f: make(f) for f in forms}
    for f in forms:
        for _ in range(a.warmup):
            calls[f]()
    torch.cuda.synchronize()
    w = {f: [] for f in forms}
    for _ in range(max(1, a.rounds)):
        for f in forms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                calls[f]()
            t1.record()
            torch.cuda.synchronize()
            w[f].append(1e3 * t0.elapsed_time(t1) / a.steps)
    say()
    say("form  us/call median (spread)   windows")
    med = {}
    for f in forms:
        s = sorted(w[f])
        med[f] = 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])
        say("%-4s  %9.1f (%.1f)          %s" % (f, med[f], s[-1] - s[0], " ".join("%.1f" % x for x in w[f])))
    say()
    for x, y in (("c", "a"), ("b", "a"), ("f", "e")):
        if x in med and y in med:
            say("%s - %s = %.1f us / call, per round: %s   (%s / %s = %.3f)"
                % (x, y, med[x] - med[y], " ".join("%.1f" % (p - q) for p, q in zip(w[x], w[y])), x, y, med[x] / med[y]))
    if "c" in med and "d" in med:
        say("c - d = %.1f us / call measured, per round: %s; derived from the bytes (4 / 28 of d) = %.1f us"
            % (med["c"] - med["d"], " ".join("%.1f" % (p - q) for p, q in zip(w["c"], w["d"])), med["d"] * 4 / 28))
    if "d" in med:
        say("d moves 28 bytes per element: %.2f TB/s" % (28.0 * elems / (med["d"] * 1e-6) / 1e12))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

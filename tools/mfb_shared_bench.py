"""Train step of MFB and MHBCoAtt (fp32) with shared images: forward(img (U, L, D), questions, img_index) beside the same
model called without an index on the pre-gathered tensor img[img_index], in the same process on the same device.

    python tools/mfb_shared_bench.py [--batch 512] [--questions-per-image 1,2,4,8] [--models mfb,mhbcoatt] [--steps 8]
                                     [--warmup 3] [--repeats 5] [--out profiles/mfb_shared_bench.txt] [--json OUT]

The step is bench.py's: forward, loss, backward, the project's Adam.  N stays --batch; for Q questions per image U = N / Q and
img_index = arange(N) // Q shuffled with a fixed seed (Q = 1: every question its own image, through the index -- what the
second backward pass costs when nothing is shared).  Each line is the median of --repeats windows of --steps steps (device
events) after --warmup steps, with the spread (max - min) of the windows: the run-to-run figure to hold a difference against.
After the table: the library profiler's times of the fusion kernels in one extra step of each form, with the bandwidth their
HBM-unique bytes (from the shapes) amount to."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vqa_amd  # noqa: E402

L, D, H, E, T, V, A, O = 196, 2048, 1024, 300, 14, 1000, 1000, 1000


def make_model(name, dev):
    cfg = types.SimpleNamespace(q_vocab_size=V, a_vocab_size=A, emb_dim=E, hidden_dim=H, num_layers=1, glove=False,
                                model_name="mfb" if name == "mfb" else "mhb_coAtt", img_feature_channel=D, img_feature_dim=L)
    torch.manual_seed(0)
    model = (vqa_amd.MFB if name == "mfb" else vqa_amd.MHBCoAtt)(cfg)
    for n, p in model.named_parameters():
        if n.find("bias") == -1 and p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    return model.to(dev).train()


def timed(model, name, img, ids, target, img_index, steps, warmup, repeats):
    crit = vqa_amd.CrossEntropyLoss() if name == "mfb" else vqa_amd.KLDivLoss()
    opt = vqa_amd.Adam(model.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        out = model(img, ids, img_index=img_index)
        crit(out, target).backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(max(1, repeats)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / steps)
    ops = vqa_amd.ops
    ops.prof_reset()
    ops.prof_enable(True)
    step()
    torch.cuda.synchronize()
    ops.prof_enable(False)
    return sorted(windows)[len(windows) // 2], max(windows) - min(windows), windows, ops.prof_report()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--questions-per-image", default="1,2,4,8")
    ap.add_argument("--models", default="mfb,mhbcoatt")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    N, dev = a.batch, "cuda:0"
    qs = [int(x) for x in a.questions_per_image.split(",")]
    if any(q < 1 or N % q for q in qs):
        ap.error("every --questions-per-image value must divide --batch")
    lines, results = [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("MFB / MHBCoAtt fp32 train step with shared images   N=%d L=%d D=%d H=%d T=%d   %s" % (N, L, D, H, T, torch.cuda.get_device_name(0)))
    say("  median of %d windows of %d steps after %d warm-up steps; spread = max - min of the windows" % (a.repeats, a.steps, a.warmup))
    one = N * L * 5 * O * 4
    for name in a.models.split(","):
        model = make_model(name, dev)
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(1, V, (N, T), generator=g).to(dev)
        target = (torch.randint(0, A, (N,), generator=g) if name == "mfb" else torch.softmax(torch.randn(N, A, generator=g), 1)).to(dev)
        say()
        say("%-9s  Q    U   img_index ms/step (spread)   None on img[idx] ms/step (spread)   shared / None   QA pairs/s shared" % name)
        for Q in qs:
            U = N // Q
            index = (torch.arange(N) // Q)[torch.randperm(N, generator=torch.Generator().manual_seed(2))].to(dev)
            img = torch.rand(U, L, D, generator=torch.Generator().manual_seed(3)).to(dev)
            ms_s, sp_s, w_s, k_s = timed(model, name, img, ids, target, index, a.steps, a.warmup, a.repeats)
            gathered = img[index].contiguous()
            ms_n, sp_n, w_n, k_n = timed(model, name, gathered, ids, target, None, a.steps, a.warmup, a.repeats)
            del gathered
            torch.cuda.empty_cache()
            say("%-9s %2d  %4d   %9.3f (%.3f)            %9.3f (%.3f)                  %6.3f          %8.0f"
                % ("", Q, U, ms_s, sp_s, ms_n, sp_n, ms_s / ms_n, N / ms_s * 1e3))
            results.append(dict(model=name, Q=Q, U=U, shared_ms=ms_s, shared_spread_ms=sp_s, shared_windows=w_s, none_ms=ms_n,
                                none_spread_ms=sp_n, none_windows=w_n, kernels_shared=k_s, kernels_none=k_n))
        del model
        torch.cuda.empty_cache()
    say()
    say("fusion kernels in one profiled step (event brackets add a few us per launch; mfb_fuse_fwd / mfb_fuse_bwd include the")
    say("final blocks' (N, 5000) launches, ~0.01 ms each).  GB = HBM-unique bytes from the shapes:")
    say("  fwd: P (U*L, 5000) read + R (N*L, 1000) written;  bwd question-owned pass: P read + dY, Y read;")
    say("  bwd image-owned pass: dY, Y read + dP (U*L, 5000) written;  plain bwd: P, dY, Y read + dP written.")
    for r in results:
        U, ks, kn = r["U"], r["kernels_shared"], r["kernels_none"]
        pu, ry = U * L * 5 * O * 4, N * L * O * 4

        def bw(k, name, nbytes):
            t = k.get(name, (0, 0.0))[1]
            return "%-18s %7.3f ms %5.2f TB/s" % (name, t, nbytes / t / 1e9 if t > 0 else 0.0)
        say("  %-8s Q=%d shared: %s | %s | %s" % (r["model"], r["Q"], bw(ks, "mfb_fuse_fwd", pu + ry), bw(ks, "mfb_fuse_bwd", pu + 2 * ry),
                                                  bw(ks, "mfb_fuse_bwd_image", pu + 2 * ry)))
        say("  %-8s Q=%d None:   %s | %s" % (r["model"], r["Q"], bw(kn, "mfb_fuse_fwd", one + ry), bw(kn, "mfb_fuse_bwd", 2 * one + 2 * ry)))
        for nm in ("gemm_f32_a0b0(fwd)", "gemm_f32_a1b1(wgrad)"):
            say("             %-22s shared %8.3f ms   None %8.3f ms" % (nm, ks.get(nm, (0, 0.0))[1], kn.get(nm, (0, 0.0))[1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(results, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()

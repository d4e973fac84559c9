"""Packed region features (forward(PackedRegions, ...)): what the MFB train step costs when the loader never pads.

    python tools/mfb_packed_bench.py [--batch 512] [--regions 100] [--steps 6] [--warmup 3] [--rounds 2]
                                     [--forms packed-rows-bf16-coatt,packed-bf16-coatt,packed-rows-bf16,packed-bf16,packed-rows,packed,pair,plain]
                                     [--out profiles/mfb_packed_bench.txt]

Setup: N = --batch, L = --regions, D = 2048, the counts of tools/mfb_regions_bench.py (uniform in 10 .. L, seed 1), MFB with the
live softmax, fp32, the train step of bench.py (forward, loss, backward, the project's Adam).  The forms named in --forms run
ALTERNATELY in one process (form A's window, form B's window, ..., --rounds times) after --warmup steps of each; a window is
--steps steps between two device events.  Reported per form: the median window (ms / step), the spread (max - min) of its windows,
the rows the projection runs on and rows / (N L).
  packed   forward(PackedRegions(rows (R, D), offsets, L), q): the projection and its weight gradient on R = sum(counts) rows
  packed-rows   the same call with model.packed_coatt = True: the fusion's output and the co-attention head on the R rows as well
  packed-bf16 / packed-rows-bf16   those two with model.regions_bf16 = True: img_conv1d and its weight gradient with bf16 operands,
           P and dP stored in bf16 (the rows are cast per step); everything else fp32
  packed-bf16-coatt / packed-rows-bf16-coatt   those two with model.regions_bf16_coatt = True as well: co_att_conv1's forward, input
           gradient and weight gradient with bf16 operands too (the fusion kernel's own bf16 copy of R, the hidden gradient stored in bf16)
  pair     forward((img (N, L, D), img_length), q): the same batch, zero-padded
  plain    forward(img, q): the padded tensor without counts (a different result: every padded row counts as a region)
--forms pair,plain uses nothing the packed form added: the same file run from a checkout of the commit before it gives the
yardstick (and, run twice, the run-to-run spread) those two forms have to stay inside.
The two projection launches come from a kernel trace in a run of its own (one form per run, e.g. --forms packed --rounds 1).
After the windows: the peak of torch's allocator over one step of each form (above what is allocated before the step), and, with
both packed forms named, the largest difference of their logits on the timed batch in eval mode (summation order inside the GEMMs);
with packed and packed-bf16 named, the same for those two (bf16 rounding of the projection's operands and of P); with packed-bf16 and
packed-bf16-coatt named, for those two (bf16 rounding of co_att_conv1's operands).
"""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vqa_amd  # noqa: E402

D, H, E, T, V, A = 2048, 1024, 300, 14, 1000, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--forms", default="packed,pair,plain")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, L, dev = a.batch, a.regions, "cuda:0"
    forms = a.forms.split(",")
    assert forms and all(f in ("packed-rows-bf16-coatt", "packed-bf16-coatt", "packed-rows-bf16", "packed-bf16", "packed-rows", "packed",
                               "pair", "plain") for f in forms)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(1)
    counts = torch.randint(10, L + 1, (N,), generator=g)
    R = int(counts.sum())
    say("packed region features: MFB train step (live softmax, fp32)   N=%d L=%d D=%d   %s" % (N, L, D, torch.cuda.get_device_name(0)))
    say("  forms %s alternating, %d rounds of one window of %d steps each after %d warm-up steps; spread = max - min of a form's windows"
        % (a.forms, a.rounds, a.steps, a.warmup))
    say("  R = sum(counts) = %d, N L = %d, R / (N L) = %.3f" % (R, N * L, R / (N * L)))
    cfg = types.SimpleNamespace(q_vocab_size=V, a_vocab_size=A, emb_dim=E, hidden_dim=H, num_layers=1, glove=False, model_name="mfb",
                                img_feature_channel=D, img_feature_dim=L)
    torch.manual_seed(0)
    model = vqa_amd.MFB(cfg)
    for n_, p_ in model.named_parameters():
        if n_.find("bias") == -1 and p_.dim() > 1:
            torch.nn.init.xavier_uniform_(p_)
    model = model.to(dev).train()
    model.unit_softmax = False
    ids = torch.randint(1, V, (N, T), generator=g).to(dev)
    target = torch.randint(0, A, (N,), generator=g).to(dev)
    valid = torch.arange(L)[None, :] < counts[:, None]
    img = (torch.rand(N, L, D, generator=g) * valid[:, :, None]).to(dev)               # zero-padded, as pad_region_features makes it
    feats = {"pair": (img, counts.to(dev)), "plain": img}
    packed_forms = ("packed", "packed-rows", "packed-bf16", "packed-rows-bf16", "packed-bf16-coatt", "packed-rows-bf16-coatt")
    rows_of = {"pair": N * L, "plain": N * L, **{f: R for f in packed_forms}}
    if any(f in forms for f in packed_forms):
        off = torch.zeros(N + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(counts, 0)
        feats.update(dict.fromkeys(packed_forms, vqa_amd.PackedRegions(img[valid.to(dev)].contiguous(), off.to(dev), L)))
    crit = vqa_amd.CrossEntropyLoss()
    opt = vqa_amd.Adam(model.parameters(), lr=1e-4)

    def step(f):
        model.packed_coatt = f.startswith("packed-rows")
        model.regions_bf16 = "-bf16" in f
        model.regions_bf16_coatt = f.endswith("-coatt")
        opt.zero_grad(set_to_none=True)
        crit(model(feats[f], ids), target).backward()
        opt.step()

    for f in forms:
        for _ in range(a.warmup):
            step(f)
    torch.cuda.synchronize()
    w = {f: [] for f in forms}
    for _ in range(max(1, a.rounds)):
        for f in forms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                step(f)
            t1.record()
            torch.cuda.synchronize()
            w[f].append(t0.elapsed_time(t1) / a.steps)
    say()
    say("%-22s  ms/step median (spread)   windows                      projection rows   rows / (N L)" % "form")
    med = {}
    for f in forms:
        s = sorted(w[f])
        med[f] = 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])
        say("%-22s  %9.3f (%.3f)          %-28s %9d        %.3f" % (f, med[f], s[-1] - s[0], " ".join("%.3f" % x for x in w[f]), rows_of[f],
                                                                   rows_of[f] / (N * L)))
    if "packed" in med and "pair" in med:
        say("packed / pair = %.3f" % (med["packed"] / med["pair"]))
    if "packed-rows" in med and "packed" in med:
        say("packed-rows - packed = %.3f ms / step, per round: %s" % (med["packed-rows"] - med["packed"],
                                                                     " ".join("%.3f" % (x - y) for x, y in zip(w["packed-rows"], w["packed"]))))
    for f in ("packed", "packed-rows"):
        if f in med and f + "-bf16" in med:
            say("%s-bf16 / %s = %.3f (%.3f ms / step less), per round: %s"
                % (f, f, med[f + "-bf16"] / med[f], med[f] - med[f + "-bf16"],
                   " ".join("%.3f" % (y - x) for x, y in zip(w[f + "-bf16"], w[f]))))
    for f in ("packed-bf16", "packed-rows-bf16"):
        if f in med and f + "-coatt" in med:
            say("%s-coatt / %s = %.3f (%.3f ms / step less), per round: %s"
                % (f, f, med[f + "-coatt"] / med[f], med[f] - med[f + "-coatt"],
                   " ".join("%.3f" % (y - x) for x, y in zip(w[f + "-coatt"], w[f]))))
    say()
    for f in forms:                                   # the allocator's peak over one step, above what the step starts from
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(f)
        torch.cuda.synchronize()
        say("%-22s  peak memory of one step above its start: %.1f MB" % (f, (torch.cuda.max_memory_allocated() - base) / 1e6))
    if "packed-rows" in forms and "packed" in forms:
        model.eval()
        with torch.no_grad():
            model.packed_coatt = False
            o0 = model(feats["packed"], ids)
            model.packed_coatt = True
            o1 = model(feats["packed"], ids)
        say("logits, eval mode: max |packed-rows - packed| / max |packed| = %.2e" % float((o1 - o0).abs().max() / o0.abs().max()))
    if "packed-bf16" in forms and "packed" in forms:
        model.eval()
        with torch.no_grad():
            model.packed_coatt, model.regions_bf16 = False, False
            o0 = model(feats["packed"], ids)
            model.regions_bf16 = True
            o1 = model(feats["packed"], ids)
        say("logits, eval mode: max |packed-bf16 - packed| / max |packed| = %.2e" % float((o1 - o0).abs().max() / o0.abs().max()))
    if "packed-bf16-coatt" in forms and "packed-bf16" in forms:
        model.eval()
        with torch.no_grad():
            model.packed_coatt, model.regions_bf16, model.regions_bf16_coatt = False, True, False
            o0 = model(feats["packed"], ids)
            model.regions_bf16_coatt = True
            o1 = model(feats["packed"], ids)
        say("logits, eval mode: max |packed-bf16-coatt - packed-bf16| / max |packed-bf16| = %.2e"
            % float((o1 - o0).abs().max() / o0.abs().max()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

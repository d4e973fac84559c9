"""Train step of HieCoAttenLadder (host/hie_ladder.py) at config 4's shapes: forward, CE loss, backward, the project's Adam.

    python tools/hie_ladder_bench.py [--batch 256] [--steps 20] [--warmup 5] [--lengths] [--coatt parallel|alternating] [--json OUT]
                                     [--questions-per-image Q] [--repeats R] [--no-context] [--regions MIN,MAX] [--blocks L]
                                     [--packed [--rounds K] [--forms packed-rows,packed,pair,plain]]

Prints ms / step and QA pairs / s (device events around the timed steps), the step's FLOP count from the shapes with its
MFMA floor at 157.3 TF/s (fp32 MFMA peak of the MI355X) and the fraction reached, the library profiler's per-kernel table
of one extra step, and config 4's single-level HieCoAtten at the same shapes in the same process for context.
--lengths: the masked step, forward(img, ids, q_length) with seeded question lengths in [3, T] (the products stay dense N*T
rows: the FLOP count is the unmasked step's).
--coatt alternating: the alternating co-attention model (its own FLOP table), and after it the streaming yardsticks of its
image side in the same process: vqf_guided_logits_fwd / _bwd over the (N*L, 3E) projection beside vqf_att_logits_fwd over a
tensor of the same size (the parallel mode's Hv pass: the same bytes read) and a device copy of that many bytes.
--questions-per-image Q: the shared-image call, forward(img (U, L, D), ids, q_length, img_index): N stays --batch, U = N / Q,
img_index = arange(N) // Q shuffled with a fixed seed (Q = 1: every question its own image, through the index).  The FLOP table
stays the per-question model's (what the step would cost without sharing).  --repeats R: R timed windows of --steps steps; the
line reports their median and the spread (max - min), the run-to-run figure to hold differences against.  --no-context: skip
the streaming yardsticks and the HieCoAtten step.
--regions MIN,MAX: the region-count call, forward((img, img_length), ...) with seeded counts in [MIN, MAX] (one per image, clipped
to the run's L; MIN = MAX = L times the masked code route at full counts).  The line adds sum(counts) / (images L), the bound
on what the image-side affinity and rank-T passes can save (their traffic goes with sum(counts)); the products and the logit
heads stay dense, and the FLOP table is the dense step's.  --blocks L: regions per image (default 196).
--packed (with --regions): the three call forms of ONE batch in one process -- forward(PackedRegions(rows, offsets, L), ...) with the
real rows of the same images, the pair (img, img_length) and the plain tensor -- on one model, alternating: --rounds K rounds (default
2) of packed, pair, plain in that order, each --repeats windows of --steps steps after --warmup steps of that form.  Prints every
round's median and spread per form, the median over all windows per form, packed against pair, and from one profiled step per form the
launch count and the img_emb launches (the projection M = rows, N = E, K = img and its weight gradient M = E, N = img, K = rows: R rows
packed, U L otherwise) beside the tanh / dropout passes.  --forms: a subset, in the order to run (pair,plain runs on a tree without the
packed form).  packed-rows (alternating only): the packed batch on the same model with packed_coatt=True -- the image side of the
levels on the R rows too; the profiled step then also lists the VX-family products by their row count.  Every form's line adds the
peak torch.cuda.max_memory_allocated of one step."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vqa_amd  # noqa: E402

PEAK_TFS = 157.3


def ladder_flops(N, L, D, E, T, H, O):
    """multiply-add pairs x 2 of the step's products (forward + input gradients + weight gradients); the image features are
    data (no input gradient for img_emb)"""
    M, MT = N * L, N * T
    f = {
        "img_emb (fwd + wgrad)": 2 * 2 * M * D * E,
        "Vh = V [Wv0;Wv1;Wv2]^T (fwd + dgrad + wgrad)": 3 * 2 * M * E * 3 * E,
        "[Cq|Qh] per level (x3)": 3 * 3 * 2 * MT * E * 2 * E,
        "phrase taps Z (x3)": 3 * 2 * MT * E * 6 * E,
        "sentence LSTM (x3)": 3 * 2 * 2 * MT * E * 4 * E,
        "affinity + rank-T passes": 3 * (2 + 2 * 2 + 2 + 2 + 2 + 2 + 2) * MT * L * E,
        "answer MLP (x3)": 3 * 2 * N * (E * E + 2 * E * E + 2 * E * H + H * O),
    }
    return f, sum(f.values())


def ladder_alt_flops(N, L, D, E, T, H, O):
    """the alternating step: the products as above, the (N, E) guidance-row products, and the streaming passes' VALU work
    (guided logits: a dot product forward, the gradient row and two sums backward; the poolings likewise)"""
    M, MT = N * L, N * T
    rows = M * 3 * E + 2 * 3 * MT * E                                  # elements the attention steps stream: image + 2 x 3 question
    f = {
        "img_emb (fwd + wgrad)": 2 * 2 * M * D * E,
        "VX = V [img_x0;img_x1;img_x2]^T (fwd + dgrad + wgrad)": 3 * 2 * M * E * 3 * E,
        "[sum|que] per level (x3)": 3 * 3 * 2 * MT * E * 2 * E,
        "phrase taps Z (x3)": 3 * 2 * MT * E * 6 * E,
        "sentence LSTM (x3)": 3 * 2 * 2 * MT * E * 4 * E,
        "guidance rows s img_g^T, v que_g^T (x3)": 3 * 6 * 2 * N * E * E,
        "guided-logits passes (VALU, fwd 2 + bwd 6 / element)": 8 * rows,
        "pooling passes (VALU, fwd 2 + bwd 4 / element)": 6 * (M * 3 * E + 2 * 3 * MT * E),
        "answer MLP (x3)": 3 * 2 * N * (E * E + 2 * E * E + 2 * E * H + H * O),
    }
    return f, sum(f.values())


def stream_yardsticks(N, L, E, reps=20):
    """image-side guided logits beside att_logits_fwd on a tensor of the same size and a copy of the same bytes, device events
    around `reps` back-to-back launches after a warm-up; bytes from the shapes: fwd reads (M, 3E); bwd reads it and writes it"""
    ops = vqa_amd.ops
    dev = "cuda:0"
    M = N * L
    g = torch.Generator().manual_seed(3)
    x = ((torch.rand(M, 3 * E, generator=g) * 2 - 1) * 1.5).to(dev)
    gp = (torch.rand(N, 3 * E, generator=g) * 2 - 1).to(dev)
    w = ((torch.rand(3, E, generator=g) * 2 - 1) * 0.1).to(dev)
    wblk = torch.zeros(3, 3 * E, device=dev)
    for i in range(3):
        wblk[i, i * E:(i + 1) * E] = w[i]
    zb = torch.zeros(3, device=dev)
    dl = (torch.rand(M, 3, generator=g) * 2 - 1).to(dev)
    dst = torch.empty_like(x)
    nbytes = x.numel() * 4

    def run(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    rows = [("att_logits_fwd (M, 3E) block-diagonal head", run(lambda: ops.att_logits_fwd(x, wblk, zb)), nbytes),
            ("guided_logits_fwd (M, 3E), G = 3", run(lambda: ops.guided_logits_fwd(x, gp, w, N, L)), nbytes),
            ("guided_logits_bwd (M, 3E), G = 3 (+ its reductions)", run(lambda: ops.guided_logits_bwd(dl, x, gp, w, N, L, out=dst)), 2 * nbytes),
            ("hbm_copy of (M, 3E)", run(lambda: ops.hbm_copy(x, dst)), 2 * nbytes)]
    print("  streaming yardsticks, M = %d, 3E = %d (%.0f MB per pass over the tensor; each includes its launch, %d back to back):"
          % (M, 3 * E, nbytes / 1e6, reps))
    for name, ms, b in rows:
        print("    %-52s %7.3f ms  %6.2f TB/s  %.3f of 8 TB/s" % (name, ms, b / ms / 1e9, b / ms / 1e9 / 8.0))
    return {name: {"ms": ms, "bytes": b} for name, ms, b in rows}


def timed(model, img, ids, target, steps, warmup, q_len=None, img_index=None, repeats=1, img_length=None):
    crit = vqa_amd.CrossEntropyLoss()
    opt = vqa_amd.Adam(model.parameters(), lr=1e-4)
    if img_length is not None:
        img = (img, img_length)

    def step():
        opt.zero_grad(set_to_none=True)
        if img_index is not None:
            out = model(img, ids, q_len, img_index=img_index)
        else:
            out = model(img, ids) if q_len is None else model(img, ids, q_len)
        loss = crit(out[0], target)
        loss.backward()
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
    ms = sorted(windows)[len(windows) // 2]
    ops = vqa_amd.ops
    ops.prof_reset()
    ops.prof_enable(True)
    step()
    torch.cuda.synchronize()
    ops.prof_enable(False)
    timed.windows = windows
    return ms, ops.prof_report()


def compare_forms(model, img, ids, target, q_len, img_index, img_length, forms, steps, warmup, rounds, repeats):
    """--packed: the call forms of one batch on one model and one optimizer, alternating -> {form: {"rounds": [[ms per window]],
    "launches": n, "kernels": prof_report(), "img_emb": {...}}}"""
    ops = vqa_amd.ops
    U, L, D = img.shape
    E = model.img_emb.out_features
    feats = {"plain": img, "pair": (img, img_length)}
    rows_of = {"plain": U * L, "pair": U * L}
    if "packed" in forms or "packed-rows" in forms:
        off = torch.zeros(U + 1, dtype=torch.int64, device=img.device)
        off[1:] = torch.cumsum(img_length.to(torch.int64), 0)
        real = torch.arange(L, device=img.device).unsqueeze(0) < img_length.unsqueeze(1)
        rows = img[real].contiguous()                                  # (R, D): the real rows, one image after the other
        feats["packed"] = feats["packed-rows"] = vqa_amd.PackedRegions(rows, off, L)
        rows_of["packed"] = rows_of["packed-rows"] = rows.shape[0]
    crit = vqa_amd.CrossEntropyLoss()
    opt = vqa_amd.Adam(model.parameters(), lr=1e-4)

    def step(f, form=None):
        model.packed_coatt = form == "packed-rows"                     # the keyword of the constructor: read by forward
        opt.zero_grad(set_to_none=True)
        if img_index is not None:
            out = model(f, ids, q_len, img_index=img_index)
        else:
            out = model(f, ids) if q_len is None else model(f, ids, q_len)
        crit(out[0], target).backward()
        opt.step()

    res = {f: {"rounds": [], "rows": rows_of[f]} for f in forms}
    for _ in range(rounds):
        for f in forms:
            for _ in range(warmup):
                step(feats[f], f)
            torch.cuda.synchronize()
            windows = []
            for _ in range(max(1, repeats)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    step(feats[f], f)
                b.record()
                torch.cuda.synchronize()
                windows.append(a.elapsed_time(b) / steps)
            res[f]["rounds"].append(windows)
    for f in forms:                                                    # one profiled step per form, after the timing
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step(feats[f], f)
        torch.cuda.synchronize()
        res[f]["peak_bytes"] = torch.cuda.max_memory_allocated()
        ops.prof_reset()
        ops.prof_enable(True)
        step(feats[f], f)
        torch.cuda.synchronize()
        ops.prof_enable(False)
        kern = ops.prof_report()
        M = rows_of[f]
        Mc = M if f == "packed-rows" else U * L                        # rows of the VX-family products of the alternating levels
        res[f]["vx"] = {"VX fwd (M=%d, N=%d, K=%d)" % (Mc, 3 * E, E): ops.prof_gemm(0, 0, Mc, 3 * E, E),
                        "dV += dVX W (M=%d, N=%d, K=%d)" % (Mc, E, 3 * E): ops.prof_gemm(0, 1, Mc, E, 3 * E),
                        "dW = dVX^T V (M=%d, N=%d, K=%d)" % (3 * E, E, Mc): ops.prof_gemm(1, 1, 3 * E, E, Mc)}
        gemms = [k for k in kern if k.startswith("gemm_f32_")]
        res[f]["kernels"] = kern
        res[f]["launches"] = sum(n for n, _ in kern.values())
        res[f]["img_emb"] = {"fwd (M=%d, N=%d, K=%d)" % (M, E, D): [ops.prof_shape(k, M, E, D) + (k,) for k in gemms if ops.prof_shape(k, M, E, D)[0]],
                             "wgrad (M=%d, N=%d, K=%d)" % (E, D, M): [ops.prof_shape(k, E, D, M) + (k,) for k in gemms if ops.prof_shape(k, E, D, M)[0]]}
    return res


def print_forms(res, forms, steps):
    med = lambda v: sorted(v)[len(v) // 2]
    for f in forms:
        for i, w in enumerate(res[f]["rounds"]):
            print("  %-11s round %d  median %.3f ms  spread %.3f ms  windows %s  launches/step %d  peak %.1f MB"
                  % (f, i + 1, med(w), max(w) - min(w), " ".join("%.3f" % x for x in w), res[f]["launches"], res[f]["peak_bytes"] / 1e6))
    allw = {f: [x for w in res[f]["rounds"] for x in w] for f in forms}
    print("  median over all windows (of %d steps): %s" % (steps, "   ".join("%s %.3f ms" % (f, med(allw[f])) for f in forms)))
    if "packed" in forms and "pair" in forms:
        p, q = med(allw["packed"]), med(allw["pair"])
        print("  packed against pair: %+.3f ms (%+.2f %%); rows of the img_emb products: %d packed, %d padded (%.3f)"
              % (p - q, (p / q - 1) * 100, res["packed"]["rows"], res["pair"]["rows"], res["packed"]["rows"] / res["pair"]["rows"]))
    if "packed-rows" in forms and "packed" in forms:
        p, q = med(allw["packed-rows"]), med(allw["packed"])
        print("  packed-rows against packed: %+.3f ms (%+.2f %%); peak memory of one step %.1f MB against %.1f MB"
              % (p - q, (p / q - 1) * 100, res["packed-rows"]["peak_bytes"] / 1e6, res["packed"]["peak_bytes"] / 1e6))
    print("  one profiled step per form (ms; event brackets add a few us per launch):")
    for f in forms:
        k = res[f]["kernels"]
        print("    %s:" % f)
        for what, hits in res[f]["img_emb"].items():
            for n, ms, name in hits:
                print("      img_emb %-32s %-22s %d launch  %7.3f ms" % (what, name, n, ms))
        for what, (n, ms) in res[f]["vx"].items():
            print("      %-46s %d launch  %7.3f ms" % (what, n, ms))
        for name in ("tanh_dropout_fwd", "tanh_dropout_bwd", "tanh_dropout_unpack_fwd", "tanh_dropout_pack_bwd", "tanh_dropout_packed_fwd",
                     "tanh_dropout_packed_bwd", "guided_logits_fwd", "guided_logits_bwd", "glimpse_pool_fwd", "glimpse_pool_bwd",
                     "glimpse_dfeat_grouped", "splitk_reduce", "colsum"):
            if name in k:
                print("      %-28s %4d launches  %7.3f ms" % (name, k[name][0], k[name][1]))
        print("      %-28s %4d launches  %7.3f ms" % ("all kernels", res[f]["launches"], sum(t for _, t in k.values())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lengths", action="store_true", help="time the masked step: seeded question lengths in [3, T]")
    ap.add_argument("--coatt", choices=("parallel", "alternating"), default="parallel", help="the co-attention mechanism of the levels")
    ap.add_argument("--json", default=None)
    ap.add_argument("--questions-per-image", type=int, default=0, metavar="Q",
                    help="shared images: U = batch / Q images, img_index = arange(N) // Q shuffled (seed 2); 0: no index")
    ap.add_argument("--repeats", type=int, default=1, help="timed windows; the median and the spread (max - min) are reported")
    ap.add_argument("--no-context", action="store_true", help="skip the streaming yardsticks and the HieCoAtten step")
    ap.add_argument("--regions", default=None, metavar="MIN,MAX", help="region counts: seeded img_length in [MIN, MAX] per image (seed 4)")
    ap.add_argument("--blocks", type=int, default=196, metavar="L", help="regions per image")
    ap.add_argument("--packed", action="store_true", help="with --regions: time the packed, pair and plain forms alternating in one process")
    ap.add_argument("--rounds", type=int, default=2, help="--packed: rounds of the forms")
    ap.add_argument("--forms", default="packed,pair,plain", help="--packed: the forms to time, in order")
    a = ap.parse_args()
    N, L, D, E, T, H, O, V = a.batch, a.blocks, 2048, 512, 14, 1024, 1000, 15881
    dev = "cuda:0"
    torch.manual_seed(0)
    Q = a.questions_per_image
    if Q < 0 or (Q and N % Q):
        ap.error("--questions-per-image must divide --batch")
    U = N // Q if Q else N
    img_index = None
    if Q:
        img_index = (torch.arange(N) // Q)[torch.randperm(N, generator=torch.Generator().manual_seed(2))].to(dev)
    img = torch.rand(U, L, D, device=dev)
    ids = torch.randint(0, V, (N, T), device=dev)
    target = torch.randint(0, O, (N,), device=dev)
    ladder = vqa_amd.HieCoAttenLadder(block_num=L, word_num=T, img_size=D, vocab_size=V, embed_size=E, hidden_size=H,
                                      output_size=O, **({} if a.coatt == "parallel" else {"coatt": a.coatt})).to(dev).train()
    q_len = None
    if a.lengths:
        q_len = torch.randint(3, T + 1, (N,), generator=torch.Generator().manual_seed(1)).to(dev)
    img_length, share = None, None
    if a.regions:
        try:
            lo, hi = (int(v) for v in a.regions.split(","))
        except ValueError:
            ap.error("--regions takes MIN,MAX")
        if not 1 <= lo <= hi:
            ap.error("--regions: 1 <= MIN <= MAX")
        lo, hi = min(lo, L), min(hi, L)
        img_length = torch.randint(lo, hi + 1, (U,), generator=torch.Generator().manual_seed(4)).to(dev)
        per_q = img_length if img_index is None else img_length[img_index]
        share = float(per_q.float().sum()) / (N * L)
    if a.packed:
        forms = [f for f in a.forms.split(",") if f]
        if not a.regions or not forms or any(f not in ("packed-rows", "packed", "pair", "plain") for f in forms):
            ap.error("--packed needs --regions MIN,MAX and --forms out of packed-rows,packed,pair,plain")
        if "packed-rows" in forms and a.coatt != "alternating":
            ap.error("--forms packed-rows needs --coatt alternating")
        res = compare_forms(ladder, img, ids, target, q_len, img_index, img_length, forms, a.steps, a.warmup, a.rounds, a.repeats)
        print("HieCoAttenLadder (coatt=%s) train step, call forms of one batch  B=%d U=%d L=%d img=%d E=%d T=%d%s"
              % (a.coatt, N, U, L, D, E, T, "  question lengths in [3, %d]" % T if a.lengths else ""))
        print("  region counts in [%d, %d]: sum(counts) / (N L) = %.3f" % (lo, hi, share))
        print_forms(res, forms, a.steps)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump({"coatt": a.coatt, "regions": a.regions, "blocks": L, "counts_share": share, "forms": res}, open(a.json, "w"), indent=1)
        return
    ms, kern = timed(ladder, img, ids, target, a.steps, a.warmup, q_len, img_index, a.repeats, img_length)
    windows = list(timed.windows)
    launches = sum(n for n, _ in kern.values())
    parts, flops = (ladder_flops if a.coatt == "parallel" else ladder_alt_flops)(N, L, D, E, T, H, O)
    floor_ms = flops / (PEAK_TFS * 1e12) * 1e3
    print("HieCoAttenLadder (coatt=%s) train step  B=%d L=%d img=%d E=%d T=%d hidden=%d out=%d%s"
          % (a.coatt, N, L, D, E, T, H, O, "  question lengths in [3, %d], mean %.1f" % (T, float(q_len.float().mean())) if a.lengths else ""))
    if Q:
        print("  shared images: %d questions per image, U = %d images, img_index shuffled" % (Q, U))
    if a.regions:
        print("  region counts in [%d, %d]: sum(counts) / (N L) = %.3f (the bound on the affinity and rank-T passes' traffic)" % (lo, hi, share))
    print("  %.3f ms/step   %.0f QA pairs/s   (median of %d windows of %d steps, spread %.3f ms; %d library launches per step)"
          % (ms, N / ms * 1e3, len(windows), a.steps, max(windows) - min(windows), launches))
    print("  %.3f TFLOP/step:" % (flops / 1e12))
    for k, v in parts.items():
        print("    %-56s %7.1f GFLOP" % (k, v / 1e9))
    print("  MFMA floor at %.1f TF/s: %.3f ms   fraction reached %.3f" % (PEAK_TFS, floor_ms, floor_ms / ms))
    print("  per kernel (one profiled step; event brackets add a few us per launch):")
    for k, (n, t) in sorted(kern.items(), key=lambda kv: -kv[1][1]):
        print("    %-28s %4d launches  %8.3f ms" % (k, n, t))
    del ladder
    torch.cuda.empty_cache()
    yard, ms4 = None, None
    if not a.no_context:
        yard = stream_yardsticks(N, L, E) if a.coatt == "alternating" else None
        hie = vqa_amd.HieCoAtten(block_num=L, word_num=T, img_size=D, vocab_size=V, embed_size=E, output_size=O).to(dev).train()
        ms4, _ = timed(hie, torch.rand(N, L, D, device=dev) if Q else img, ids, target, a.steps, a.warmup)
        print("config 4 HieCoAtten (word level only) at the same shapes: %.3f ms/step   %.0f QA pairs/s" % (ms4, N / ms4 * 1e3))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump({"coatt": a.coatt, "questions_per_image": Q, "images": U, "windows_ms": windows, "spread_ms": max(windows) - min(windows),
                   "launches_per_step": launches, "regions": a.regions, "blocks": L, "counts_share": share, "yardsticks": yard, "lengths": bool(a.lengths), "ms_per_step": ms, "qa_per_s": N / ms * 1e3, "tflop_per_step": flops / 1e12, "floor_ms": floor_ms,
                   "fraction_of_floor": floor_ms / ms, "kernels": kern, "hiecoatten_ms_per_step": ms4}, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()

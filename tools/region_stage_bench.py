"""Packed region features from pinned host memory (RegionStager): what the MFB train step costs PCIe-inclusive.

    python tools/region_stage_bench.py [--batch 512] [--regions 100] [--steps 6] [--warmup 3] [--rounds 2]
                                       [--out profiles/region_stager_bench.txt]

Setup: the batch of tools/mfb_packed_bench.py (N = --batch, L = --regions, D = 2048, counts uniform in 10 .. L, seed 1), MFB with
the live softmax, fp32, forward + loss + backward + the project's Adam.  The forms run ALTERNATELY in one process (--rounds windows
of --steps steps each, after --warmup steps of each); a window is a host clock around steps that end in a device synchronise, since
half of what is measured is host work.  Reported per form: the mean of the two middle windows (the median), the spread
(max - min), and the difference to `resident` of the same run.
  resident       forward(PackedRegions) on a batch that lives in HBM (the yardstick)
  staged32       RegionStager(storage="fp32", depth 2): next(), the step, then host_slot() / commit() of the next batch with the
                 slot's rows left as they are (only the counts are written): the copies, the waits and the stager's own host work
  staged16       the same with storage="fp16" (half the bytes over PCIe, the widening kernel behind the copy)
  staged32+fill  as staged32, and the host also copies the batch's rows into the pinned slot first (stands for the loader's np.load)
  staged16+fill  the same for fp16 (the host copy reads fp16 rows)
  pack.to        pack_region_features(list).to(device) per step: np.concatenate into pageable memory, then a blocking copy
Then a timeline: one more window for resident / staged32 / staged16, twice, with device events around every step (compute stream)
and every commit (copy stream) -- where the copies sit, whether a step waits for them, which steps take longer -- and the plain
windows of those three once more behind it.  Then, on their own: the H2D rate out of the pinned slot, what one commit keeps the copy
stream busy for, and the kernel's passes beside vqf_hbm_copy moving the same number of bytes (read + written) in the same process.
"""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vqa_amd  # noqa: E402

D, H, E, T, V, A = 2048, 1024, 300, 14, 1000, 1000


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, L, dev = a.batch, a.regions, torch.device("cuda", 0)
    ops = vqa_amd.ops
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(1)
    counts = torch.randint(10, L + 1, (N,), generator=g)
    R = int(counts.sum())
    say("RegionStager: MFB train step (live softmax, fp32) fed from pinned host memory   N=%d L=%d D=%d   %s"
        % (N, L, D, torch.cuda.get_device_name(0)))
    say("  R = sum(counts) = %d rows: %.1f MB as fp32, %.1f MB as fp16 (the padded pair: %.1f MB); R / (N L) = %.3f"
        % (R, R * D * 4 / 1e6, R * D * 2 / 1e6, N * L * D * 4 / 1e6, R / (N * L)))
    say("  forms alternating, %d rounds of one window of %d steps each after %d warm-up steps; spread = max - min of a form's windows"
        % (a.rounds, a.steps, a.warmup))
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
    rows32 = torch.rand(R, D, generator=g).numpy()
    rows16 = rows32.astype(np.float16)
    cnt = counts.numpy().astype(np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)])
    per_image = [rows32[off[u]:off[u + 1]] for u in range(N)]           # what a loader holds: one (K_u, D) array per image
    resident = vqa_amd.pack_region_features(per_image)
    resident = vqa_amd.PackedRegions(resident.rows, resident.offsets, L).to(dev)
    crit = vqa_amd.CrossEntropyLoss()
    opt = vqa_amd.Adam(model.parameters(), lr=1e-4)

    def step(x):
        opt.zero_grad(set_to_none=True)
        crit(model(x, ids), target).backward()
        opt.step()

    stagers = {s: vqa_amd.RegionStager(N, channels=D, max_regions=L, max_rows=R, device=dev, storage=s, depth=2) for s in ("fp32", "fp16")}
    fill_s, fill_n = {}, {}

    def put(storage, fill):
        st = stagers[storage]
        rows, c = st.host_slot()
        if fill:
            t0 = time.perf_counter()
            np.copyto(rows[:R], rows16 if storage == "fp16" else rows32)
            fill_s[storage] = fill_s.get(storage, 0.0) + time.perf_counter() - t0
            fill_n[storage] = fill_n.get(storage, 0) + 1
        c[:N] = cnt
        st.commit(N)

    def staged(storage, fill):
        def run(steps):
            put(storage, True)                       # primes the pipeline (outside the window: run() is called once before timing)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                x, _ = stagers[storage].next()
                step(x)                              # the GPU works on batch k ...
                put(storage, fill)                   # ... while the host ships batch k + 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            stagers[storage].next()                  # drain
            return dt
        return run

    def plain(feats_of):
        def run(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(feats_of())
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return run

    def pack_to():
        p = vqa_amd.pack_region_features(per_image)
        return vqa_amd.PackedRegions(p.rows, p.offsets, L).to(dev)

    forms = [("resident", plain(lambda: resident)), ("staged32", staged("fp32", False)), ("staged16", staged("fp16", False)),
             ("staged32+fill", staged("fp32", True)), ("staged16+fill", staged("fp16", True)), ("pack.to", plain(pack_to))]
    for _, run in forms:
        run(a.warmup)
    fill_s.clear()
    fill_n.clear()
    w = {f: [] for f, _ in forms}
    for _ in range(max(1, a.rounds)):
        for f, run in forms:
            w[f].append(run(a.steps) / a.steps * 1e3)
    say()
    say("%-14s  ms/step median (spread)   windows                 minus resident" % "form")
    med = {}
    for f, _ in forms:
        s = sorted(w[f])
        med[f] = 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])
    for f, _ in forms:
        s = sorted(w[f])
        say("%-14s  %9.3f (%.3f)          %-22s  %+8.3f" % (f, med[f], s[-1] - s[0], " ".join("%.3f" % x for x in w[f]), med[f] - med["resident"]))
    for s in ("fp32", "fp16"):
        say("host copy into the pinned slot (%s): %.2f ms per batch (one thread)" % (s, fill_s[s] / fill_n[s] * 1e3))

    # where the difference to `resident` sits: one more window per form, with device events around each step (compute stream) and
    # around each commit (copy stream)
    def ev(stream=None):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream if stream is not None else torch.cuda.current_stream(dev))
        return e

    def timeline(storage):
        st = stagers.get(storage)
        if st is not None:
            put(storage, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base, rec = ev(), []
        for _ in range(a.steps):
            x = resident if st is None else st.next()[0]        # next(): the compute stream waits for the batch's event
            s0 = ev()
            step(x)
            s1 = ev()
            c0 = c1 = None
            if st is not None:
                c0 = ev(st.copy_stream)                            # the copy stream is idle: this is when the host got here
                put(storage, False)
                c1 = ev(st.copy_stream)
            rec.append((s0, s1, c0, c1))
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        if st is not None:
            st.next()
        t = base.elapsed_time
        busy = sum(s0.elapsed_time(s1) for s0, s1, _, _ in rec)
        say("  %s: host clock %.3f ms / step; on the GPU first start %.3f, last end %.3f, the steps themselves %.3f ms / step"
            % ("resident" if st is None else "staged, %s slots" % storage, host_ms / a.steps, t(rec[0][0]), t(rec[-1][1]), busy / a.steps))
        for k, (s0, s1, c0, c1) in enumerate(rec):
            line = "    step %d on the GPU %8.3f .. %8.3f = %7.3f ms" % (k, t(s0), t(s1), s0.elapsed_time(s1))
            if c0 is not None:
                line += ";  copies (+ kernel) of batch %d %8.3f .. %8.3f = %6.3f ms" % (k + 1, t(c0), t(c1), c0.elapsed_time(c1))
            say(line)

    say()
    say("timeline (ms since the window's first event; one more window of %d steps per form, twice):" % a.steps)
    for _ in range(2):
        for s in (None, "fp32", "fp16"):
            timeline(s)

    say()
    say("plain windows once more, behind the instrumented ones (ms / step, minus resident of this round):")
    again = {f: run(a.steps) / a.steps * 1e3 for f, run in forms[:3]}
    say("  " + "   ".join("%s %.3f (%+.3f)" % (f, v, v - again["resident"]) for f, v in again.items()))

    say()
    say("on their own (device events, 10 iterations each after one warm-up call):")
    for s, esz in (("fp32", 4), ("fp16", 2)):
        sl = stagers[s]._slots[0]
        dst = torch.empty((R, D), dtype=sl["host"].dtype, device=dev)
        ms = timed(lambda: dst.copy_(sl["host"][:R], non_blocking=True), 10)
        say("  H2D from the pinned slot, %s: %.1f MB in %.3f ms = %.1f GB/s" % (s, R * D * esz / 1e6, ms, R * D * esz / ms / 1e6))
    for s in ("fp32", "fp16"):
        for form in ("packed", "padded"):
            st = vqa_amd.RegionStager(N, channels=D, max_regions=L, max_rows=R, device=dev, storage=s, form=form, depth=1)
            busy = []
            for _ in range(4):
                rows, c = st.host_slot()
                c[:N] = cnt
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st.copy_stream)
                st.commit(N)
                e1.record(st.copy_stream)
                torch.cuda.synchronize()
                st.next()
                busy.append(e0.elapsed_time(e1))
            say("  one commit on the copy stream, %s %s: %.3f ms (copies + kernel, nothing else running)" % (s, form, min(busy[1:])))
    droff = torch.from_numpy(off.astype(np.int32)).to(dev)
    d32, d16 = torch.from_numpy(rows32).to(dev), torch.from_numpy(rows16).to(dev)
    passes = [("widen fp16 -> packed", lambda: ops.region_rows_stage(d16), R * D * 6),
              ("copy fp32 -> packed", lambda: ops.region_rows_stage(d32), R * D * 8),
              ("fp32 -> padded", lambda: ops.region_rows_stage(d32, droff, L), R * D * 4 + N * L * D * 4),
              ("fp16 -> padded", lambda: ops.region_rows_stage(d16, droff, L), R * D * 2 + N * L * D * 4)]
    for name, fn, nbytes in passes:
        half = nbytes // 2 // 16 * 16
        src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        src.zero_()
        ms_k, ms_c = timed(fn, 10), timed(lambda: ops.hbm_copy(src, dst), 10)
        say("  %-20s %7.1f MB read + written: %.4f ms = %6.1f GB/s;  vqf_hbm_copy of as many bytes: %.4f ms = %6.1f GB/s"
            % (name, nbytes / 1e6, ms_k, nbytes / ms_k / 1e6, ms_c, 2 * half / ms_c / 1e6))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

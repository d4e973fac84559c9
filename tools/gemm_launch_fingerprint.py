#!/usr/bin/env python3
"""Fingerprint of the GEMM launchers (csrc/gemm_f32*.hip, gemm_bf16*.hip): a fixed table of products with seeded operands through
ops.gemm, gemm_rowscale, gemm_rows, bgemm, gemm_bf16, gemm_bf16_rowscale and lstm_step_fwd, under the default options and under
each option value that selects another launch statement.  Per case one line: the launches counted per kernel family (ops.stat
deltas, in the order of ops.STATS) and the sha256 of the output.  The summation order of a product depends on its splits and
K chunks, so equal hashes pin them; two commits that differ only in how the launchers are written must print the same bytes.

    python tools/gemm_launch_fingerprint.py [--out fp.txt]
    rocprofv3 --kernel-trace -d DIR -- python tools/gemm_launch_fingerprint.py       # the ordered (kernel, grid, workgroup, LDS) list

One process, well under a minute on an MI355X; the table makes every GEMM launch statement of the seven files execute (the record with
the kernel list is profiles/gemm_launch_fingerprint.txt; the fp32 -> bf16 cast of gemm_bf16.hip is no GEMM and is not in it)."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqa_amd import ops                                                                  # noqa: E402

DEV = "cuda:0"


def U(shape, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.rand(shape, generator=g, device=DEV) * 2 - 1).to(dtype)


def operands(ta, tb, M, N, K, dtype=torch.float32):
    return U((K, M) if ta else (M, K), 11, dtype), U((K, N) if tb else (N, K), 12, dtype)


def gemm(ta, tb, M, N, K, **kw):
    a, b = operands(ta, tb, M, N, K)
    return ops.gemm(a, b, ta=bool(ta), tb=bool(tb), bias=U((N,), 13), **kw)


def gemm_unaligned(ta, tb, M, N, K):
    """operands 4 bytes off a 16-byte boundary: the guarded loaders of the 128x128 kernel"""
    a = U((K, M + 1) if ta else (M, K + 1), 11)[:, 1:]
    b = U((K, N + 1) if tb else (N, K + 1), 12)[:, 1:]
    return ops.gemm(a, b, ta=bool(ta), tb=bool(tb), relu=True)


def gemm_accum(ta, tb, M, N, K):
    a, b = operands(ta, tb, M, N, K)
    return ops.gemm(a, b, ta=bool(ta), tb=bool(tb), out=U((M, N), 14), accumulate=True)


def rowscale(M, N, K, rps):
    a, b = operands(0, 0, M, N, K)
    return ops.gemm_rowscale(a, b, U(((M + rps - 1) // rps,), 15), rps, bias=U((N,), 13), relu=True)


def rows(tb, NS, L, N, K):
    a, b = operands(0, tb, NS * L, N, K)
    return ops.gemm_rows(a, b, L, tb=bool(tb), bias=U((N,), 13), relu=True)


def bgemm(ta, tb, Bn, M, N, K):
    return ops.bgemm(U((Bn, K, M) if ta else (Bn, M, K), 11), U((Bn, K, N) if tb else (Bn, N, K), 12), ta=bool(ta), tb=bool(tb))


def bf16(ta, tb, M, N, K, **kw):
    a, b = operands(ta, tb, M, N, K, torch.bfloat16)
    return ops.gemm_bf16(a, b, ta=bool(ta), tb=bool(tb), bias=U((N,), 13), **kw)


def bf16_rowscale(M, N, K, rps):
    a, b = operands(0, 0, M, N, K, torch.bfloat16)
    return ops.gemm_bf16_rowscale(a, b, U(((M + rps - 1) // rps,), 15), rps, bias=U((N,), 13), relu=True)


def lstm_step(B, H):
    gates, c_out, h_out = U((B, 4 * H), 16), torch.empty((B, H), device=DEV), torch.empty((B, H), device=DEV)
    ops.lstm_step_fwd(U((B, H), 11), U((4 * H, H), 12) * 0.05, gates, U((B, H), 17), c_out, h_out)
    return torch.cat([gates, c_out, h_out], dim=1)


LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
CASES = []      # (name, options, function, arguments)


def case(name, fn, *args, **options):
    CASES.append((name, options, fn, args))


# ---- fp32 large-tile kernel (gemm_f32_big.hip).  gemm_f32_big = 2 reaches it with small products: every layout in every loop form,
# a zero-filled last K slab (K % 16 != 0) and a short last column tile
for ta, tb in LAYOUTS:
    for loop in (0, 1, 2):
        case("f32big/small/%d%d/loop%d" % (ta, tb, loop), gemm, ta, tb, 520, 392, 200, gemm_f32_big=2, gemm_f32_loop=loop)
    # the stream-K tail (real routing: 392 tiles = 1.53 rounds) and the same products without it
    case("f32big/streamk/%d%d" % (ta, tb), gemm, ta, tb, 50176, 512, 512, gemm_f32_streamk=1)
case("f32big/1024tiles/K1536", gemm, 0, 0, 8192, 8192, 1536)
case("f32big/1024tiles/K1536/relu", gemm, 0, 1, 8192, 8192, 1536, relu=True)
for name, opts in (("default", {}), ("persist0", dict(gemm_f32_persist=0)), ("cu128", dict(gemm_cu_limit=128)), ("edge0", dict(gemm_f32_edge=0))):
    case("f32big/N5000/" + name, gemm, 0, 0, 13312, 5000, 1536, **opts)                  # 52 x 20 tiles, 136 live columns in the last
for name, opts in (("default", {}), ("fused0", dict(gemm_splitk_fused=0)), ("order1", dict(gemm_splitk_order=1)),
                   ("persist0", dict(gemm_f32_persist=0))):
    case("f32big/wgrad64/" + name, gemm, 1, 1, 4096, 1024, 7168, **opts)                  # 64 tiles x 4 splits, combined in the launch
case("f32big/wgrad16", gemm, 1, 1, 1024, 1024, 50176)                                     # 16 tiles x 16 splits + the reduce launch
case("f32big/wgrad16/order1", gemm, 1, 1, 1024, 1024, 50176, gemm_splitk_order=1)
# the whole-rounds row split of a mid-size product: 128 row tiles here, the other rows on the 128x128 kernel
case("f32/rounds/50176x512", gemm, 0, 0, 50176, 512, 512)
case("f32/rounds/50176x512/tb", gemm, 0, 1, 50176, 512, 512)
case("f32/rounds/50176x512/rounds0", gemm, 0, 0, 50176, 512, 512, gemm_f32_rounds=0)
case("f32/rounds/50176x512/rowscale", rowscale, 50176, 512, 512, 196)
case("f32/rowscale/big", rowscale, 8192, 8192, 1536, 196)
case("f32/rowscale/small", rowscale, 300, 136, 72, 7)
# ---- per-wave kernel (gemm_f32_wave.hip): its four forms, both B layouts
for tb in (0, 1):
    for name, opts in (("shb6", {}), ("own", dict(gemm_f32_wave=1)), ("shb12", dict(gemm_f32_wave=3)), ("off", dict(gemm_f32_wave=0))):
        case("f32wave/%s/tb%d" % (name, tb), gemm, 0, tb, 512, 4096, 1024, **opts)
    case("f32wave/k4/tb%d" % tb, gemm, 0, tb, 256, 2048, 1024)
    case("f32wave/accum/tb%d" % tb, gemm_accum, 0, tb, 512, 4096, 1024)
# ---- one-round 128x80 tiles (gemm_f32_n80.hip) and what takes the product without it: the 128x128 kernel's split-K, both combines
for name, opts in (("default", {}), ("n80=0", dict(gemm_f32_n80=0)), ("n80=0/fused1", dict(gemm_f32_n80=0, gemm_splitk_fused=1)),
                   ("cu128", dict(gemm_cu_limit=128))):
    case("f32n80/512x5000x2048/" + name, gemm, 0, 0, 512, 5000, 2048, **opts)
case("lstm_step/n80", lstm_step, 512, 1024)
case("lstm_step/wave", lstm_step, 512, 1024, gemm_f32_n80=0)
case("lstm_step/wave/H256", lstm_step, 128, 256)
# ---- per-sample tiles (gemm_f32_sample.hip)
for tb in (0, 1):
    case("f32sample/tb%d" % tb, rows, tb, 64, 196, 512, 512)
    case("f32sample/tb%d/cu128" % tb, rows, tb, 64, 196, 512, 512, gemm_cu_limit=128)
    case("f32sample/tb%d/off" % tb, rows, tb, 64, 196, 512, 512, gemm_f32_sample=0)
# ---- 128x128 kernel (gemm_f32.hip): every layout with the fast and with the guarded loaders, split-K, the batched form
for ta, tb in LAYOUTS:
    case("f32tile/fast/%d%d" % (ta, tb), gemm, ta, tb, 200, 136, 72, gemm_f32_big=0)
    case("f32tile/guarded/%d%d" % (ta, tb), gemm_unaligned, ta, tb, 200, 136, 72)
    case("f32tile/odd/%d%d" % (ta, tb), gemm, ta, tb, 201, 135, 71)
    case("f32tile/splitk/%d%d" % (ta, tb), gemm, ta, tb, 512, 384, 8192, gemm_f32_big=0, gemm_f32_wave=0)
    case("f32tile/batched/%d%d" % (ta, tb), bgemm, ta, tb, 3, 200, 136, 72)
case("f32tile/nosplitk", gemm, 1, 1, 512, 384, 8192, gemm_f32_big=0, splitk=False)
# ---- bf16 large-tile kernels (gemm_bf16_big.hip): pp16 / pp / lockstep / loop 3, rowscale, bf16 output, split-K
for ta, tb in LAYOUTS:
    for loop in (1, 0, 3):
        case("bf16big/%d%d/loop%d" % (ta, tb, loop), bf16, ta, tb, 2048, 2048, 1024, gemm_bf16_loop=loop)
case("bf16big/persist0", bf16, 0, 0, 2048, 5000, 1024, gemm_bf16_persist=0)
case("bf16big/cu128", bf16, 0, 0, 8192, 5000, 1024, gemm_cu_limit=128)
case("bf16big/rowscale", bf16_rowscale, 4096, 2048, 1024, 196)
case("bf16big/rowscale/loop0", bf16_rowscale, 4096, 2048, 1024, 196, gemm_bf16_loop=0)
case("bf16big/out_bf16", bf16, 0, 0, 2048, 2048, 1024, out_bf16=True)
for name, opts in (("default", {}), ("fused0", dict(gemm_splitk_fused=0)), ("order1", dict(gemm_splitk_order=1)), ("big0", dict(gemm_bf16_big=0))):
    case("bf16big/wgrad64/" + name, bf16, 1, 1, 4096, 1024, 7168, **opts)
# ---- bf16 128x128 kernel (gemm_bf16.hip)
for ta, tb in LAYOUTS:
    case("bf16tile/%d%d" % (ta, tb), bf16, ta, tb, 200, 136, 72)
    case("bf16tile/splitk/%d%d" % (ta, tb), bf16, ta, tb, 512, 384, 8192)
case("bf16tile/splitk/fused1", bf16, 1, 1, 512, 384, 8192, gemm_splitk_fused=1)
case("bf16tile/rowscale", bf16_rowscale, 304, 136, 72, 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    lines = []
    for name, options, fn, fargs in CASES:
        if args.only and args.only not in name:
            continue
        kw = {k: v for k, v in options.items() if k not in ops.OPTIONS}
        before = [ops.stat(s) for s in ops.STATS]
        with ops.options(**{k: v for k, v in options.items() if k in ops.OPTIONS}):
            out = fn(*fargs, **kw)
            torch.cuda.synchronize()
        delta = [ops.stat(s) - b for s, b in zip(ops.STATS, before)]
        assert sum(delta) > 0, name
        raw = out.contiguous().view(torch.uint8).cpu().numpy().tobytes()
        lines.append("%-40s %s %s %s" % (name, ",".join(map(str, delta)), "%s:%s" % (tuple(out.shape), str(out.dtype)[6:]),
                                         hashlib.sha256(raw).hexdigest()))
        del out
    text = "families: " + " ".join(ops.STATS) + "\n" + "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

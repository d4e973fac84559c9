"""tests/gemm_ref.py and the checker of tests/test_gpu_gemm_small.py without a GPU: the fp64 reference against torch.matmul on
every option, the integer data set of every GPU case inside the exact range, the bound (k + 1) 2^-24 sum |terms| not too tight
(plain fp32 arithmetic on the CPU stays inside it on every random case), the checker rejecting each of a list of subtly wrong
results, and the restated routing rules giving every case the family its table names."""
import numpy as np
import pytest
import torch

import gemm_ref as GR
import test_gpu_gemm_small as G


def _specs():
    """(group, case id, label, spec) of every first run and variant of the GPU file's tables"""
    for group, cid, spec, variants in G.ALL_CASES:
        yield group, cid, "first", spec
        for label, v, _ in variants:
            yield group, cid, label, v


def _unique_products():
    seen, out = set(), []
    for group, cid, label, s in _specs():
        if s.data_key() not in seen:
            seen.add(s.data_key())
            out.append((group, cid, s))
    return out


PRODUCTS = _unique_products()


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 3])
@pytest.mark.parametrize("ta,tb", G.LAYOUTS)
def test_product_equals_torch_matmul_fp64(ta, tb, batch):
    M, N, K = 37, 21, 29
    for bias in (False, True):
        for c0 in (False, True):
            for rps, row0 in ((0, 0), (1, 0), (7, 0), (7, 5), (100, 0)):
                for relu in (False, True):
                    d = GR.operands("random", ta, tb, M, N, K, 11, batch=batch, bias=bias, c0=c0, rowscale=rps)
                    if rps:                                                       # enough scales for rows row0 .. row0 + M - 1
                        d["rowscale"] = GR.uniform((-(-(M + row0) // rps),), 12) + 2.0
                    ref, terms = GR.product(d["A"], d["B"], ta, tb, bias=d["bias"], c0=d["c0"], rowscale=d["rowscale"], rps=rps or 1,
                                            row0=row0, relu=relu)
                    a, b = torch.from_numpy(d["A"]).double(), torch.from_numpy(d["B"]).double()
                    a = a.transpose(-1, -2) if ta else a
                    b = b if tb else b.transpose(-1, -2)
                    want, wabs = torch.matmul(a, b), torch.matmul(a.abs(), b.abs())
                    if rps:
                        sc = torch.from_numpy(d["rowscale"]).double()[(row0 + torch.arange(M)) // rps][:, None]
                        want, wabs = want * sc, wabs * sc.abs()
                    for t in (d["bias"], d["c0"]):
                        if t is not None:
                            want, wabs = want + torch.from_numpy(t).double(), wabs + torch.from_numpy(t).double().abs()
                    if relu:
                        want = torch.relu(want)
                    assert ref.shape == ((M, N) if batch is None else (batch, M, N)) and ref.dtype == np.float64
                    assert np.allclose(ref, want.numpy(), rtol=1e-13, atol=1e-13) and np.allclose(terms, wabs.numpy(), rtol=1e-13, atol=1e-13)
                    assert (np.abs(ref) <= terms * (1 + 1e-12)).all()


def test_bf16_rounding_helpers():
    x = GR.uniform((4096,), 3)
    assert np.array_equal(GR.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert (np.abs(GR.bf16_trunc(x)) <= np.abs(x)).all() and (np.abs(GR.bf16_trunc(x) - x) <= np.abs(x) * 2.0 ** -7).all()
    ints = GR.ints((64, 64), 5, 8)
    assert np.array_equal(GR.bf16_round(ints), ints)


def test_bound_formula():
    t = np.array([[2.0, 0.0]])
    assert np.array_equal(GR.bound(t, 7), 8 * 2.0 ** -24 * t) and np.array_equal(GR.bound(t, 7, u=2.0 ** -23), 8 * 2.0 ** -23 * t)
    assert GR.check(np.float32([[2.0, 0.0]]), np.array([[2.0, 0.0]]), t, 7) == (0.0, 0)
    assert GR.check(np.float32([[2.0, 1e-30]]), np.array([[2.0, 0.0]]), t, 7) == (float("inf"), 1)      # a zero bound: equal or rejected
    assert GR.check(np.float32([[float("nan"), 0.0]]), np.array([[2.0, 0.0]]), t, 7)[0] == float("inf")


# ---- the GPU file's data ------------------------------------------------------------------------------------------------------------
def test_every_exact_case_stays_in_the_exact_range():
    worst = 0.0
    for group, cid, s in PRODUCTS:
        d, ref, terms = G.reference("exact", s.data_key())
        assert float(terms.max()) < GR.EXACT_LIMIT, (group, cid)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), (group, cid, "reference not an fp32 number")
        for name in ("A", "B"):                                                   # every value depends on its position
            assert np.unique(d[name]).size >= 5, (group, cid, name)
        assert np.array_equal(GR.bf16_round(d["A"]), d["A"]) and np.array_equal(GR.bf16_round(d["B"]), d["B"])
        worst = max(worst, float(terms.max()))
    print("exact data: %d products, largest sum |terms| %.0f = 2^%.1f" % (len(PRODUCTS), worst, np.log2(worst)))


def _fp32_whole(d, s):
    """the product in plain fp32 on the CPU: torch.float32 matmul, then the epilogue one fp32 operation at a time"""
    a, b = torch.tensor(d["A"]), torch.tensor(d["B"])
    a = a.transpose(-1, -2) if s.ta else a
    b = b if s.tb else b.transpose(-1, -2)
    v = torch.matmul(a, b)
    if s.rowscale:
        v = v * torch.tensor(d["rowscale"])[torch.arange(s.M) // s.rowscale][:, None]
    if s.bias:
        v = v + torch.tensor(d["bias"])
    if s.acc:
        v = v + torch.tensor(d["c0"])
    return (torch.relu(v) if s.relu else v).numpy()


def _fp32_chain(d, s, rows, cols):
    """a block of the product as a sequential np.float32 chain over k (each product rounded, each addition rounded: no fused
    multiply-add), then the epilogue"""
    a, b = GR.operand(d["A"], s.ta), GR.operand(d["B"], s.tb)
    if s.batch is not None:
        a, b = a[-1], b[-1]
    a, b = np.ascontiguousarray(a[rows]), np.ascontiguousarray(b[cols])
    acc = np.zeros((len(rows), len(cols)), dtype=np.float32)
    for k in range(s.K):
        acc = acc + a[:, k, None] * b[None, :, k]
    assert acc.dtype == np.float32
    if s.rowscale:
        acc = acc * d["rowscale"][rows // s.rowscale][:, None]
    if s.bias:
        acc = acc + d["bias"][cols]
    if s.acc:
        c0 = d["c0"] if s.batch is None else d["c0"][-1]
        acc = acc + c0[np.ix_(rows, cols)]
    return np.maximum(acc, np.float32(0)) if s.relu else acc


def test_the_bound_is_not_too_tight_for_plain_fp32_arithmetic():
    """a kernel that adds K products in fp32, in whatever order, has to be able to pass: torch's fp32 matmul on the whole output and
    a sequential fp32 chain on a sampled 8 x 8 block, on every random case with the case's own k"""
    worst_whole = worst_chain = 0.0
    for group, cid, s in PRODUCTS:
        d, ref, terms = G.reference("random", s.data_key())
        k = G.k_of(s)
        whole, _ = GR.check(_fp32_whole(d, s), ref, terms, k)
        rng = np.random.default_rng(s.M + s.N + s.K)
        rows = np.sort(rng.choice(s.M, size=min(8, s.M), replace=False))
        cols = np.sort(rng.choice(s.N, size=min(8, s.N), replace=False))
        r2, t2 = (ref, terms) if s.batch is None else (ref[-1], terms[-1])
        chain, _ = GR.check(_fp32_chain(d, s, rows, cols), r2[np.ix_(rows, cols)], t2[np.ix_(rows, cols)], k)
        print("cpu fp32 %-13s %-60s k %5d  torch.float32 matmul err/bound %.3f  np.float32 chain err/bound %.3f" % (group, cid, k, whole, chain))
        assert whole <= 1.0 and chain <= 1.0, (group, cid, whole, chain)
        worst_whole, worst_chain = max(worst_whole, whole), max(worst_chain, chain)
    print("cpu fp32 worst over %d products: matmul %.3f, chain %.3f" % (len(PRODUCTS), worst_whole, worst_chain))


# ---- the checker rejects subtly wrong results ---------------------------------------------------------------------------------------
MUT_M, MUT_N, MUT_K, MUT_SPLITS, MUT_CHUNK = 130, 70, 520, 2, 272     # the ragged split-K case of the GPU file: 272 + 248, tail of 8


def _mut_data(kind, acc=False, relu=False):
    d = GR.operands(kind, 0, 0, MUT_M, MUT_N, MUT_K, 77, bias=True, c0=acc)
    ref, terms = GR.product(d["A"], d["B"], 0, 0, bias=d["bias"], c0=d["c0"], relu=relu)
    return d, ref, terms, MUT_K + (MUT_SPLITS - 1) + 1 + int(acc)


def _rejected(kind, got, ref, terms, k):
    if kind == "exact":
        return GR.same_bits(got, ref)[0] > 0
    return GR.check(got, ref, terms, k)[0] > 1.0


def _accepted(kind, got, ref, terms, k):
    return not _rejected(kind, got, ref, terms, k)


def _drop_one_term(d, ref):
    a, b = d["A"].astype(np.float64), d["B"].astype(np.float64)
    i, j = 71, 33
    k = int(np.argmax(np.abs(a[i]) * np.abs(b[j]) > 0))       # the first k of that element whose term is not zero
    assert a[i, k] * b[j, k] != 0
    got = ref.copy()
    got[i, j] -= a[i, k] * b[j, k]
    return got


def _swap_rows(d, ref):
    got = ref.copy()
    got[[5, 6]] = got[[6, 5]]
    return got


def _bias_per_split(d, ref):
    return ref + (MUT_SPLITS - 1) * d["bias"].astype(np.float64)


def _shift_sub_tile(d, ref):
    got = ref.copy()
    got[:, 32:64] = ref[:, 31:63]
    return got


def _tail_twice(d, ref):
    a, b = d["A"].astype(np.float64), d["B"].astype(np.float64)
    k0 = MUT_K - MUT_K % 16
    assert 0 < MUT_K - k0 < 16
    return ref + a[:, k0:] @ b[:, k0:].T


MUTATIONS = [("one k term dropped from one element", _drop_one_term), ("two rows swapped inside a tile", _swap_rows),
             ("bias added once per split", _bias_per_split), ("one 32-column sub-tile shifted by one column", _shift_sub_tile),
             ("the last K-tail slab taken twice", _tail_twice)]


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("name,mutate", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_checker_rejects(name, mutate, kind):
    d, ref, terms, k = _mut_data(kind)
    good = ref.astype(np.float32)
    assert _accepted(kind, good, ref, terms, k)
    bad = mutate(d, ref).astype(np.float32)
    changed = int((bad != good).sum())
    assert changed > 0
    assert _rejected(kind, bad, ref, terms, k), name
    print("mutation %-48s %-6s rejected (%d of %d elements changed)" % (name, kind, changed, good.size))


def test_checker_rejects_relu_before_the_accumulate():
    d, ref, terms, k = _mut_data("exact", acc=True, relu=True)
    assert _accepted("exact", ref.astype(np.float32), ref, terms, k)
    pre, _ = GR.product(d["A"], d["B"], 0, 0, bias=d["bias"], relu=True)
    bad = (pre + d["c0"]).astype(np.float32)
    assert _rejected("exact", bad, ref, terms, k)
    print("mutation %-48s exact  rejected (%d of %d elements changed)" % ("ReLU before the accumulate", int((bad != ref).sum()), bad.size))


def test_checker_rejects_operands_truncated_to_bf16_where_the_bound_can_see_it():
    """Truncating both operands to bf16 leaves each product ~2^-8 relative off, a sum of K of them ~sqrt(K) 2^-9 rms|ab|; the bound is
    (K + 1) 2^-24 K mean|ab|.  For every K of the fp32 random cases: where the first exceeds the second on the case's
    distributions the checker must reject such a result; the other K are listed."""
    ks = sorted({s.K for _, _, s in PRODUCTS if not s.bf16})
    seen, blind = [], []
    for K in ks:
        d = GR.operands("random", 0, 0, 64, 64, K, 5)
        ref, terms = GR.product(d["A"], d["B"], 0, 0)
        ab = np.abs(d["A"].astype(np.float64)[:, None, :] * d["B"].astype(np.float64)[None, :, :])
        est, bnd = np.sqrt(K) * 2.0 ** -9 * np.sqrt((ab ** 2).mean()), (K + 1) * GR.U * K * ab.mean()
        got, _ = GR.product(GR.bf16_trunc(d["A"]), GR.bf16_trunc(d["B"]), 0, 0)
        worst, _ = GR.check(got.astype(np.float32), ref, terms, K)
        print("bf16-truncated operands K %5d: estimate %.2e bound %.2e -> worst err/bound %.1f" % (K, est, bnd, worst))
        if est > bnd:
            assert worst > 1.0, K
            seen.append(K)
        else:
            blind.append(K)
    assert seen, "no K at which the bound sees bf16 operands"
    print("bf16-truncated operands: rejected at K in %s; not asserted at K in %s (the estimate is inside the bound)" % (seen, blind))


# ---- the routing restatement --------------------------------------------------------------------------------------------------------
def test_restated_routing_gives_every_case_its_family():
    needs_cus = []
    for group, cid, label, s in _specs():
        want = (s.fam, s.form, s.splits, s.reduce)
        got = G.route(s, None)
        if got is None:
            needs_cus.append((group, cid, label))
        else:
            assert got == want, (group, cid, label, got, want)
        assert G.route(s, 256) == want, (group, cid, label, G.route(s, 256), want)          # the tables hold the 256-CU shapes
    print("routes: %d runs; %d need the CU count: %s" % (sum(1 for _ in _specs()), len(needs_cus), sorted({c[:2] for c in needs_cus})))
    assert {c[0] for c in needs_cus} <= {"n80", "wave"}


def test_restated_split_plans():
    """the split decisions the GPU file's ids name, from the restated cost models"""
    assert G.f32_tile128_plan(128, 128, 512, G.WS_BYTES) == (2, 256) and G.f32_tile128_plan(128, 128, 496, G.WS_BYTES)[0] == 1
    assert G.f32_tile128_plan(130, 70, 520, G.WS_BYTES) == (2, 272) and G.f32_tile128_plan(130, 70, 520, 0)[0] == 1
    assert G.bf16_tile128_plan(130, 70, 1032, G.WS_BYTES, False) == (2, 544) and G.bf16_tile128_plan(130, 70, 1032, 0, True)[0] == 1
    assert G.big_pick_splits(1, 16384, 256, 256, G.WS_BYTES) == 32 and G.splitk_chunks(16384, 16, 32) == (32, 512)
    assert (MUT_SPLITS, MUT_CHUNK) == G.f32_tile128_plan(MUT_M, MUT_N, MUT_K, G.WS_BYTES)
    for cus in (64, 104, 256, 304):                        # the 128x80 shapes land in [0.8 CUs, CUs] on other chips as well
        for _, M, N, K in G.n80_shapes(cus):
            tiles = -(-M // 128) * -(-N // 80)
            assert cus * 8 <= tiles * 10 and tiles <= cus, (cus, M, N)

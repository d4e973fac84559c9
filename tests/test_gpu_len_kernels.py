"""The twelve length-masked entry points (include/vqa_fusion.h: vqf_embed_tanh_fwd_len / _bwd_len, vqf_phrase_ngram_fwd_len /
_bwd_len, vqf_dropout_bt_len, vqf_glimpse_pool_fwd_len / _bwd_len and their _grouped_len forms, vqf_hie_affinity_len /
_levels_len, vqf_tanh_bwd_rows_len) on their own, against the fp64 truncation reference tests/len_kernels_ref.py (pinned on the
masked model restatement by tests/test_len_kernels_ref_cpu.py).

Inside the models the padding is already zero when it reaches these kernels, so a kernel that read it would give the same bits
there.  Here every case runs twice with different contents in the padded rows of every input: first values that would do the
most damage if read (+ 50 in the phrase kernels' Z, + 30 in the pool's logits, seeded values in [-4, 4] elsewhere), then NaN
wherever the header calls the rows unread.  The outputs of the two runs must be the same bits.  Further, per entry point:
  parity      per SAMPLE (per level and sample for the affinity) against the reference, max |err| / max |ref| of that sample, at
              the tolerance the project applies to the unmasked kernel (cited at each check);
  zeros       every output is pre-filled with 7.0: a padded output row must be an exact zero, "not written" does not pass;
  lens = T    the bits of the entry point without lens (vqf_tanh_bwd_rows_len has none: the bits of vqf_tanh_dropout_bwd with
              p = 0, the flat kernel the ladder runs there when it has no lengths);  two runs: equal bits;
  clamping    (the kernels that clamp: phrase, pool, tanh_bwd_rows) lengths 0 and T + 5 give the bits of 1 and T;
  refusals    a null lens: VQF_E_BADARG; a lens pointer two bytes off alignment: a non-zero code, nothing launched.
Shapes: the smallest at which each loop tail can go wrong (see the parameter lists)."""
import pytest
import torch

import len_kernels_ref as LR
from golden_util import _report_parity

pytestmark = pytest.mark.gpu

NAN = float("nan")
P_DROP = 0.3


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


@pytest.fixture(scope="module")
def grouping(vqa):
    import importlib
    return importlib.import_module(vqa.__name__ + ".host.grouping")


def _cu(x):
    return x.float().contiguous().cuda()


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


def _seven(*shape, dtype=torch.float32):
    return torch.full(shape, 7, dtype=dtype, device="cuda")


def _pad_mask(lens, T):
    """(N, T) bool on the GPU: the padded positions"""
    return (torch.arange(T).unsqueeze(0) >= torch.tensor(LR.clamp_lens(lens, T)).unsqueeze(1)).cuda()


def _zero_rows(x, pad):
    """x (N, T, ...): every padded row an exact zero (a NaN or a 7.0 left from the pre-fill fails)"""
    return bool((x[pad] == 0).all())


def _out_of_range(lens, T):
    """the lengths with a 1 replaced by 0 and a T by T + 5: what the clamping kernels must treat as 1 and T"""
    out = [0 if l == 1 else l for l in lens]
    for i in reversed(range(len(lens))):
        if lens[i] == T:
            out[i] = T + 5
            break
    assert out != list(lens)
    return out


def _same(a, b):
    """two result dicts: the same bits under every key (None == None)"""
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    return True


class _Report:
    """per-sample parity; the worst err / tolerance per output is printed (and logged on the GPU machine) as golden_util does"""

    def __init__(self, entry, shape):
        self.label, self.items = "len_kernels %-32s %s" % (entry, shape), {}

    def parity(self, name, got, ref, tol):
        """ref (samples, ...) fp64: every sample judged on its own"""
        got = got.detach().cpu().double().reshape(ref.shape)
        errs = [float((got[n] - ref[n]).abs().max() / (ref[n].abs().max() + 1e-30)) for n in range(ref.shape[0])]
        print("%s %s: worst err/tol %.3f, per sample err %s" % (self.label, name, max(errs) / tol, " ".join("%.1e" % e for e in errs)))
        for n, e in enumerate(errs):
            assert e <= tol, (self.label, name, "sample %d" % n, e, tol)
        self.items[name] = max(self.items.get(name, 0.0), max(errs) / tol)

    def flush(self):
        name = max(self.items, key=self.items.get)
        _report_parity(self.label, self.items[name], name, "  " + " ".join("%s=%.3f" % kv for kv in sorted(self.items.items())))


# ---- phrase_ngram_fwd_len / _bwd_len ------------------------------------------------------------------------------------------------
def _wide(x2d, ld):
    """x (rows, W) as the first W columns of a (rows, ld) buffer"""
    buf = torch.full((x2d.shape[0], ld), 9.0, device="cuda")
    buf[:, :x2d.shape[1]] = x2d
    return buf[:, :x2d.shape[1]]


@pytest.mark.parametrize("N,T,E,lens", LR.PHRASE_CASES, ids=["N6_T7_E8_window_cut_at_1_and_2", "N3_T32_E64", "N2_T1_E64"])
def test_phrase_ngram_len(ops, N, T, E, lens):
    ldz, ldq = 6 * E + 4, E + 4                       # rows as column blocks of wider buffers
    Z, bias, dQp = LR.phrase_inputs(N, T, E)
    gb, pad = _cu(bias), _pad_mask(lens, T)
    qjunk = LR.rnd((N, T, E), 77, 4.0)

    def run(ln, Zf, dQf, qfill):
        """forward, then the backward on the kernel's own Qp and idx (whose padded Qp rows get `qfill` first)"""
        gl = None if ln is None else _i32(ln)
        qbuf, idx, zbuf = _seven(N * T, ldq), _seven(N * T, E, dtype=torch.uint8), _seven(N * T, ldz)
        ops.phrase_ngram_fwd(_wide(_cu(Zf).view(N * T, 6 * E), ldz), gb, N, T, out=qbuf[:, :E], idx=idx, lens=gl)
        qp = qbuf[:, :E].contiguous()
        if qfill is not None:
            fill = _cu(qjunk) if qfill == "rand" else torch.full((N, T, E), qfill, device="cuda")
            qbuf[:, :E] = torch.where(pad[:, :, None], fill, qp.view(N, T, E)).view(N * T, E)
        ops.phrase_ngram_bwd(_wide(_cu(dQf).view(N * T, E), ldq), qbuf[:, :E], idx, N, T, out=zbuf[:, :6 * E], lens=gl)
        torch.cuda.synchronize()
        assert bool((qbuf[:, E:] == 7).all()) and bool((zbuf[:, 6 * E:] == 7).all())            # nothing beyond the rows' columns
        return dict(Qp=qp, idx=idx, dZ=zbuf[:, :6 * E].contiguous())

    Zhot = LR.fill_padding(Z, lens, 50.0)             # + 50 would win any maximum
    a = run(lens, Zhot, LR.fill_padding(dQp, lens, "rand", 5), "rand")
    b = run(lens, LR.fill_padding(Z, lens, NAN), LR.fill_padding(dQp, lens, NAN), NAN)
    assert _same(a, b)
    assert _same(a, run(lens, Zhot, LR.fill_padding(dQp, lens, "rand", 5), "rand"))
    rep = _Report("phrase_ngram_fwd_len/_bwd_len", (N, T, E))
    rqp, ridx, clear = LR.phrase_fwd(Zhot, bias, lens)
    rep.parity("Qp", a["Qp"], rqp, 1e-6)                                  # test_gpu_hie_ladder.test_phrase_ngram_kernels: 1e-6
    idx = a["idx"].cpu().long().view(N, T, E)
    real = int((~pad).sum()) * E
    excluded = int((~clear).sum())
    print("phrase idx: %d of %d real elements within %.0e of a tie" % (excluded, real, LR.IDX_GAP))
    assert excluded <= LR.IDX_CAP * real
    assert torch.equal(idx[clear], ridx[clear])
    assert _zero_rows(a["Qp"].view(N, T, E), pad) and bool((a["idx"].view(N, T, E)[pad] == 3).all())
    # backward, given the kernel's own Qp and winners
    rdz = LR.phrase_bwd(dQp, a["Qp"].cpu().double().view(N, T, E), idx, lens)
    rep.parity("dZ", a["dZ"], rdz, 1e-6)                                  # test_phrase_ngram_kernels: 1e-6
    assert _zero_rows(a["dZ"].view(N, T, 6 * E), pad)
    db, dbr = ops.colsum(a["dZ"]).cpu().double(), rdz.view(N * T, 6 * E).sum(0)
    for c0 in (0, E, 3 * E):                                              # the taps (1, 0), (2, 0), (3, 0): the bias gradients, 2e-5
        rep.parity("colsum_tap%d" % c0, db[c0:c0 + E].view(1, E), dbr[c0:c0 + E].view(1, E), 2e-5)
    rep.flush()
    # lens = T: the bits of the entry points without lens
    assert _same(run([T] * N, Z, dQp, None), run(None, Z, dQp, None))
    # 0 and T + 5 act as 1 and T
    assert _same(a, run(_out_of_range(lens, T), Zhot, LR.fill_padding(dQp, lens, "rand", 5), "rand"))


# ---- tanh_bwd_rows_len --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,L,lens", [(4, 5, 7, [2, 5, 1, 3]), (2, 22, 50, [22, 17])],
                         ids=["N4_T5_L7_groups_straddle_rows", "N2_T22_L50_batched_gemm_route"])
def test_tanh_bwd_rows_len(ops, N, T, L, lens):
    dy, y, pad = LR.rnd((N, T, L), 31), LR.rnd((N, T, L), 32, 0.9), _pad_mask(lens, T)

    def run(ln, fill, inplace):
        gd, gy = _cu(LR.fill_padding(dy, lens, fill, 6)), _cu(LR.fill_padding(y, lens, fill, 7))
        out = gd if inplace else _seven(N, T, L)
        ops.tanh_bwd_rows_len(gd, gy, _i32(ln), N, T, out=out)
        torch.cuda.synchronize()
        return dict(dx=out)

    rep = _Report("tanh_bwd_rows_len", (N, T, L))
    a = run(lens, "rand", False)
    for inplace in (False, True):
        assert _same(a, run(lens, "rand", inplace)) and _same(a, run(lens, NAN, inplace))
        assert _same(a, run(_out_of_range(lens, T), "rand", inplace))
    rep.parity("dx", a["dx"], LR.tanh_bwd_rows(dy, y, lens), 1e-6)         # three fp32 roundings
    assert _zero_rows(a["dx"], pad)
    rep.flush()
    # lens = T: the flat kernel the ladder runs without lengths (functions._hie_dc)
    flat = ops.tanh_dropout_bwd(_cu(dy).view(N * T, L), _cu(y).view(N * T, L), None, 0, 0.0)
    gd, gy = _cu(dy), _cu(y)
    assert torch.equal(ops.tanh_bwd_rows_len(gd, gy, _i32([T] * N), N, T, out=_seven(N, T, L)).view(N * T, L), flat)


# ---- dropout_bt_len -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["keep", "philox"])
@pytest.mark.parametrize("layout", ["time_major_in", "time_major_out"])
def test_dropout_bt_len(ops, layout, mask):
    B, T, H, lens = 4, 6, 8, [1, 6, 3, 5]
    x, pad = LR.rnd((B, T, H), 41), _pad_mask(lens, T)
    keep = (torch.rand((B, T, H), generator=torch.Generator().manual_seed(42)) >= P_DROP).to(torch.uint8)
    kw = dict(keep=keep.cuda(), p_drop=P_DROP) if mask == "keep" else dict(seed=977, p_drop=P_DROP)

    def run(ln, xf):
        """-> y as a contiguous (B, T, H) tensor; the time-major side is a permuted view of a (T, B, H) buffer"""
        if layout == "time_major_in":
            gx, out = _cu(xf.permute(1, 0, 2)).permute(1, 0, 2), _seven(B, T, H)
        else:
            gx, out = _cu(xf), _seven(T, B, H).permute(1, 0, 2)
        assert ops.dropout_bt(gx, out, lens=None if ln is None else _i32(ln), **kw) is out
        torch.cuda.synchronize()
        return dict(y=out.contiguous())

    if mask == "philox":       # the mask the plain kernel draws, read off ones
        keep = (run(None, torch.ones(B, T, H, dtype=torch.float64))["y"] != 0).to(torch.uint8).cpu()
    a = run(lens, LR.fill_padding(x, lens, "rand", 8))
    assert _same(a, run(lens, LR.fill_padding(x, lens, NAN))) and _same(a, run(lens, LR.fill_padding(x, lens, "rand", 8)))
    rep = _Report("dropout_bt_len %s %s" % (layout, mask), (B, T, H))
    rep.parity("y", a["y"], LR.dropout_bt(x, keep, P_DROP, lens), 1e-6)    # test_gpu_hie_modules.test_dropout_and_tanh_dropout_kernels: 1e-6
    rep.flush()
    assert _zero_rows(a["y"], pad)
    plain = run(None, x)
    assert torch.equal(a["y"][~pad], plain["y"][~pad])                     # the real rows: vqf_dropout_bt's bits
    assert _same(run([T] * B, x), plain)
    assert float((a["y"][~pad] == 0).float().mean()) > 0.1                 # the mask did drop something


# ---- embed_tanh_fwd_len / _bwd_len --------------------------------------------------------------------------------------------------
def test_embed_tanh_len(ops):
    V, E = 50, 7                                       # the smallest (V, E) of test_gpu_kernels.test_embed_tanh_fwd_bwd_vs_torch_fp64
    N, Tq, lens = 5, 7, [1, 7, 3, 6, 2]
    LONE, NEVER = 11, 5                                # LONE occurs at padded positions only, NEVER nowhere
    g = torch.Generator().manual_seed(51)
    W = torch.randn((V, E), generator=g).double()
    ids = torch.randint(0, V, (N, Tq), generator=g)
    ids[(ids == LONE) | (ids == NEVER)] = 6
    pad_c = _pad_mask(lens, Tq).cpu()
    shared = int(ids[1, 2])                            # a real word of sample 1 that the padding repeats
    kinds = torch.tensor([LONE, shared, -1, V])
    ids[pad_c] = kinds[torch.arange(int(pad_c.sum())) % 4]
    assert int((ids[~pad_c] == LONE).sum()) == 0 and int((ids[pad_c] == shared).sum()) > 0
    dout, pad = LR.rnd((N, Tq, E), 52), pad_c.cuda()
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    gW, gids = _cu(W), ids.cuda()

    def run(ln, seed):
        """the forward; the backward with seeded finite values in the padded rows of dout and out (the header promises nothing
        about NaN there)"""
        gl = _i32(ln)
        out, dW = _seven(N, Tq, E), _seven(V, E)
        assert lib.vqf_embed_tanh_fwd_len(ptr(gW), ptr(gids), ptr(gl), N, Tq, V, E, ptr(out), st) == 0
        gd = _cu(LR.fill_padding(dout, ln, "rand", seed))
        go = _cu(LR.fill_padding(out.cpu().double(), ln, "rand", seed + 1))
        assert lib.vqf_embed_tanh_bwd_len(ptr(gd), ptr(go), ptr(gids), ptr(gl), N, Tq, V, E, ptr(dW), st) == 0
        torch.cuda.synchronize()
        return dict(out=out, dW=dW)

    a = run(lens, 9)
    assert _same(a, run(lens, 19)) and _same(a, run(lens, 9))
    assert torch.equal(a["out"], ops.embed_tanh_fwd(gW, gids, lens=_i32(lens)))                  # the wrapper: the same call
    assert torch.equal(a["dW"], ops.embed_tanh_bwd(_cu(dout), a["out"], gids, V, lens=_i32(lens)))
    rep = _Report("embed_tanh_fwd_len/_bwd_len", (N, Tq, V, E))
    rep.parity("out", a["out"], LR.embed_fwd(W, ids, lens), 2e-6)          # test_embed_tanh_fwd_bwd_vs_torch_fp64: 2e-6
    assert _zero_rows(a["out"], pad)
    # (dW has no sample axis: the whole tensor, 2e-6 max(1, sqrt(T / V) / 4) = 2e-6 at T = 35 tokens, and row by row below)
    rdW = LR.embed_bwd(dout, a["out"].cpu().double(), ids, lens, V)
    rep.parity("dW", a["dW"], rdW.view(1, V, E), 2e-6)
    rep.flush()
    assert float(a["dW"][LONE].abs().max()) == 0.0 and float(a["dW"][NEVER].abs().max()) == 0.0
    assert float(rdW[shared].abs().max()) > 0.0
    got = a["dW"].cpu().double()
    assert float((got[shared] - rdW[shared]).abs().max()) <= 2e-6 * float(rdW.abs().max())     # the real contributions only
    # lens = Tq: the bits of the entry points without lens (ids outside [0, V) select no row there either)
    full = run([Tq] * N, 9)
    out = ops.embed_tanh_fwd(gW, gids)
    assert torch.equal(full["out"], out)
    assert torch.equal(full["dW"], ops.embed_tanh_bwd(_cu(dout), out, gids, V))


# ---- glimpse_pool_fwd_len / _bwd_len and the grouped forms --------------------------------------------------------------------------
def _pool_fwd(ops, feat, logits, lens, idx, dims, unit):
    N, U, S, C, G = dims
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    wts, pooled = _seven(N, G, S), _seven(N, G * C)
    if idx is None and lens is None:
        rc = lib.vqf_glimpse_pool_fwd(p(feat), p(logits), N, S, C, G, unit, p(wts), p(pooled), st)
    elif idx is None:
        rc = lib.vqf_glimpse_pool_fwd_len(p(feat), p(logits), p(lens), N, S, C, G, unit, p(wts), p(pooled), st)
    elif lens is None:
        rc = lib.vqf_glimpse_pool_fwd_grouped(p(feat), p(logits), p(idx[0]), N, U, S, C, G, p(wts), p(pooled), st)
    else:
        rc = lib.vqf_glimpse_pool_fwd_grouped_len(p(feat), p(logits), p(idx[0]), p(lens), N, U, S, C, G, p(wts), p(pooled), st)
    assert rc == 0
    return wts, pooled


def _pool_bwd(ops, dp, dwx, feat, wts, lens, idx, dims, unit, want_dfeat):
    N, U, S, C, G = dims
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    dl = _seven(N * S, G)
    df = _seven(*feat.shape) if want_dfeat else None
    if idx is None and lens is None:
        rc = lib.vqf_glimpse_pool_bwd(p(dp), p(dwx), p(feat), p(wts), N, S, C, G, unit, p(dl), p(df), st)
    elif idx is None:
        rc = lib.vqf_glimpse_pool_bwd_len(p(dp), p(dwx), p(feat), p(wts), p(lens), N, S, C, G, unit, p(dl), p(df), st)
    elif lens is None:
        rc = lib.vqf_glimpse_pool_bwd_grouped(p(dp), p(dwx), p(feat), p(wts), p(idx[0]), p(idx[1]), p(idx[2]), N, U, S, C, G, p(dl), p(df), st)
    else:
        rc = lib.vqf_glimpse_pool_bwd_grouped_len(p(dp), p(dwx), p(feat), p(wts), p(idx[0]), p(idx[1]), p(idx[2]), p(lens), N, U, S, C, G,
                                                  p(dl), p(df), st)
    assert rc == 0
    return dl, df


def _pool_run(ops, ln, feat, logits, dwx, dp, idx, dims, unit):
    """the forward and the four backwards (with / without dfeat: the general and the register path; with / without dwts_extra),
    wts from the kernel's own forward; every output pre-filled with 7.0"""
    gl = None if ln is None else _i32(ln)
    gf, glg, gdx = _cu(feat), _cu(logits).view(-1, dims[4]), _cu(dwx.transpose(1, 2))
    res = {}
    res["wts"], res["pooled"] = _pool_fwd(ops, gf, glg, gl, idx, dims, unit)
    for want_dfeat in (True, False):
        for extra in (True, False):
            dl, df = _pool_bwd(ops, dp, gdx if extra else None, gf, res["wts"], gl, idx, dims, unit, want_dfeat)
            res["dl_%d%d" % (want_dfeat, extra)], res["df_%d%d" % (want_dfeat, extra)] = dl, df
    torch.cuda.synchronize()
    return res


POOL_CASES = [
    # U, N, S, C, G, lens (U: counts per image), index, unit_softmax
    pytest.param(None, 7, 14, 64, 3, [1, 2, 3, 4, 5, 13, 14], None, 0, id="wide_N7_S14_C64_G3_Sv_around_the_unroll_of_4"),
    pytest.param(None, 3, 9, 6, 1, [1, 9, 5], None, 0, id="scalar_path_C6"),
    pytest.param(None, 9, 196, 512, 3, [1, 7, 8, 9, 15, 16, 17, 195, 196], None, 0, id="row_slots_RS8_S196_C512_G3"),
    pytest.param(None, 5, 64, 256, 1, [1, 16, 17, 33, 64], None, 0, id="row_slots_RS16_S64_C256_G1"),
    pytest.param(None, 7, 14, 64, 3, [1, 2, 3, 4, 5, 13, 14], None, 1, id="wide_unit_softmax"),
    pytest.param(3, 9, 20, 64, 2, [7, 20, 1], [2, 0, 0, 2, 0, 2, 0, 0, 0], 0, id="grouped_U3_N9_S20_image0_six_questions_image1_unused"),
    pytest.param(2, 5, 196, 512, 2, [195, 1], [1, 0, 0, 1, 0], 0, id="grouped_row_slots_U2_N5_S196_C512"),
]


@pytest.mark.parametrize("U,N,S,C,G,lens,index,unit", POOL_CASES)
def test_glimpse_pool_len(ops, grouping, U, N, S, C, G, lens, index, unit):
    dims = (N, U or 0, S, C, G)
    shared = U is not None
    it = torch.tensor(index) if shared else None
    idx = grouping._group_index(it.cuda(), U) if shared else None
    lens_q = [lens[u] for u in index] if shared else lens                       # per question; lens: per feature block
    feat, logits = LR.rnd((U or N, S, C), 61), LR.rnd((N, S, G), 62, 2.0)
    dwx, dp = LR.rnd((N, S, G), 63), _cu(LR.rnd((N, G * C), 64))                 # dwts_extra in the (N, S, G) layout until the call
    pad, pad_f = _pad_mask(lens_q, S), _pad_mask(lens, S)

    def run(ln, ffill, lfill, seed):
        """ffill None: the operands as they are"""
        if ffill is None:
            return _pool_run(ops, ln, feat, logits, dwx, dp, idx, dims, unit)
        return _pool_run(ops, ln, LR.fill_padding(feat, lens, ffill, seed), LR.fill_padding(logits, lens_q, lfill, seed + 1),
                         LR.fill_padding(dwx, lens_q, ffill, seed + 2), dp, idx, dims, unit)

    a = run(lens_q, "rand", 30.0, 70)                  # + 30 in the padded logits would take the whole softmax
    assert _same(a, run(lens_q, NAN, NAN, 80)) and _same(a, run(lens_q, "rand", 30.0, 70))
    assert _same(a, run(_out_of_range(lens_q, S), "rand", 30.0, 70))
    if C % 4 == 0:                                     # the wrappers make the same calls
        gf, gl = _cu(LR.fill_padding(feat, lens, "rand", 70)), _i32(lens_q)
        glg = _cu(LR.fill_padding(logits, lens_q, 30.0, 71)).view(N * S, G)
        gdx = _cu(LR.fill_padding(dwx, lens_q, "rand", 72).transpose(1, 2))
        if shared:
            w, po = ops.glimpse_pool_fwd_grouped(gf, glg, idx[0], lens=gl)
            dl, df = ops.glimpse_pool_bwd_grouped(dp, gf, w, idx[0], idx[1], idx[2], True, dwts=gdx, lens=gl)
        else:
            w, po = ops.glimpse_pool_fwd(gf, glg, bool(unit), lens=gl)
            dl, df = ops.glimpse_pool_bwd(dp, gf, w, bool(unit), True, dwts=gdx, lens=gl)
        assert torch.equal(w, a["wts"]) and torch.equal(po, a["pooled"]) and torch.equal(dl, a["dl_11"]) and torch.equal(df, a["df_11"])

    rep = _Report("glimpse_pool%s_len%s" % ("_grouped" if shared else "", " unit" if unit else ""), (U, N, S, C, G))
    rw, rp = LR.pool_fwd(feat, logits, lens_q, unit=bool(unit), idx=it)
    rep.parity("wts", a["wts"], rw, 1e-6)              # test_gpu_hie_ladder.test_glimpse_pool_and_logits_g3: wts, pooled, dfeat 1e-6 ...
    rep.parity("pooled", a["pooled"], rp, 1e-6)
    wts = a["wts"].transpose(1, 2)                     # (N, S, G)
    assert _zero_rows(wts, pad)
    if not unit:
        assert float((a["wts"].double().sum(2) - 1).abs().max()) <= 1e-5
    w64 = a["wts"].cpu().double()
    for extra in (True, False):
        rdl, rdf = LR.pool_bwd(dp.cpu().double(), dwx.transpose(1, 2) if extra else None, feat, w64, lens_q, unit=bool(unit), idx=it, U=U)
        for want_dfeat in (True, False):
            tag = "%d%d" % (want_dfeat, extra)
            dl = a["dl_" + tag].view(N, S, G)
            rep.parity("dlogits_" + tag, dl, rdl, 1e-5)                        # ... and dlogits 1e-5
            assert _zero_rows(dl, pad)
            if want_dfeat:
                rep.parity("dfeat_" + tag, a["df_" + tag], rdf, 1e-6)
                assert _zero_rows(a["df_" + tag], pad_f)                       # (grouped: beyond the image's count; the unused image)
            else:
                assert a["df_" + tag] is None
    if shared:
        for u in range(U):
            if u not in index:
                assert float(a["df_11"][u].abs().max()) == 0.0 and float(a["df_10"][u].abs().max()) == 0.0
    rep.flush()
    # lens = S: the bits of the entry points without lens
    assert _same(run([S] * N, None, None, 0), run(None, None, None, 0))


def test_glimpse_pool_grouped_len_identity_index(ops, grouping):
    """under the identity index the grouped forms run the plain forms' kernels for wts, pooled and dlogits: the same bits; dfeat is
    the per-image sum kernel's (another association), 1e-6"""
    N, S, C, G, lens = 5, 20, 64, 2, [7, 20, 1, 16, 17]
    idx = grouping._group_index(torch.arange(N).cuda(), N)
    feat, logits, dwx = (LR.fill_padding(LR.rnd(s, 65 + i, 2.0 if i == 1 else 1.0), lens, f, 90 + i)
                         for i, (s, f) in enumerate((((N, S, C), "rand"), ((N, S, G), 30.0), ((N, S, G), "rand"))))
    dp = _cu(LR.rnd((N, G * C), 68))
    plain = _pool_run(ops, lens, feat, logits, dwx, dp, None, (N, 0, S, C, G), 0)
    grouped = _pool_run(ops, lens, feat, logits, dwx, dp, idx, (N, N, S, C, G), 0)
    rep = _Report("glimpse_pool_grouped_len identity", (N, S, C, G))
    for k in plain:
        if k.startswith("df_1"):
            rep.parity(k, grouped[k], plain[k].cpu().double(), 1e-6)
            assert _zero_rows(grouped[k], _pad_mask(lens, S))
        else:
            assert _same({k: plain[k]}, {k: grouped[k]})
    rep.flush()


# ---- hie_affinity_len ---------------------------------------------------------------------------------------------------------------
def _aff_tol(epi):
    return 5e-6 if epi == 1 else 2e-6                  # test_gpu_hie_ladder.test_hie_affinity_levels: 2e-6, 5e-6 with the fast tanh


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("N,L,E,T,lens", [(4, 37, 32, 5, [1, 5, 3, 4]), (3, 16, 64, 16, [16, 15, 1])],
                         ids=["N4_L37_E32_T5_three_row_groups_last_partial", "N3_L16_E64_T16"])
def test_hie_affinity_len(ops, N, L, E, T, lens, epi):
    pad = _pad_mask(lens, T)
    xw, yw = LR.rnd((N, T, 2 * E), 101, 0.5), LR.rnd((N, L, 2 * E), 102, 0.5)   # [x1 | x2], [y1 | y2]: column blocks of wider buffers
    yprev = LR.rnd((N, T, L), 103, 0.9)
    keep = (torch.rand((N, T, L), generator=torch.Generator().manual_seed(104)) >= P_DROP).to(torch.uint8)
    gy = _cu(yw).view(N * L, 2 * E)
    rep = _Report("hie_affinity_len epi %d" % epi, (N, L, E, T))
    for pairs in (1, 2):
        for mask in (("none",) if epi == 0 else ("keep", "philox")):
            drop = (None, 0, 0.0) if mask == "none" else (keep.cuda(), 0, P_DROP) if mask == "keep" else (None, 555, P_DROP)

            def run(ln, fill, seed, ep=epi):
                gx = _cu(xw if ln is None else LR.fill_padding(xw, lens, fill, seed)).view(N * T, 2 * E)
                gp = None if ep != 2 else _cu(yprev if ln is None else LR.fill_padding(yprev, lens, fill, seed + 1))
                out = _seven(N, T, L)
                ops.hie_affinity(gx[:, :E], gy[:, :E], N, L, T, x2=gx[:, E:] if pairs == 2 else None, y2=gy[:, E:] if pairs == 2 else None,
                                 epi=ep, yprev=gp, drop=drop, out=out, lens=None if ln is None else _i32(ln))
                torch.cuda.synchronize()
                return dict(out=out)

            k64 = None
            if mask == "keep":
                k64 = keep
            elif mask == "philox":      # the mask the plain kernel draws: the zeros of its dropped tanh
                k64 = (run(None, None, 0, ep=1)["out"] != 0).to(torch.uint8).cpu()
            a = run(lens, "rand", 110)
            assert _same(a, run(lens, NAN, 120)) and _same(a, run(lens, "rand", 110))
            ref = LR.affinity(xw[:, :, :E], yw[:, :, :E], lens, x2=xw[:, :, E:] if pairs == 2 else None, y2=yw[:, :, E:] if pairs == 2 else None,
                              epi=epi, yprev=yprev if epi == 2 else None, keep=k64, p=P_DROP if k64 is not None else 0.0)
            rep.parity("pairs%d_%s" % (pairs, mask), a["out"], ref, _aff_tol(epi))
            assert _zero_rows(a["out"], pad)
            plain = run(None, None, 0)
            assert torch.equal(a["out"][~pad], plain["out"][~pad])             # the real rows: vqf_hie_affinity's bits
            assert _same(run([T] * N, None, 0), plain)
    rep.flush()


# ---- hie_affinity_levels_len --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_y", "separate_y"])
@pytest.mark.parametrize("G", [1, 3])
def test_hie_affinity_levels_len(ops, G, shared, epi):
    N, L, E, T, lens = 3, 20, 32, 14, [14, 1, 9]
    pad = _pad_mask(lens, T)
    lvy = 0 if shared else E
    rep = _Report("hie_affinity_levels_len G %d %s epi %d" % (G, "shared" if shared else "separate", epi), (N, L, E, T))
    for pairs in (1, 2):
        assert ops.hie_affinity_levels_supported(N, L, E, T, G, pairs)
        x, y = LR.rnd((N, T, 2 * G * E), 130 + pairs, 0.5), LR.rnd((N, L, G * E), 140 + pairs, 0.5)   # level g's X at g 2E, Y at g E (or 0)
        x2, y2 = LR.rnd((N, T, G * E), 150, 0.5), LR.rnd((N, L, G * E + 4), 160, 0.5)
        yprev = LR.rnd((G, N, T, L), 170, 0.9)
        gy, gy2 = _cu(y).view(N * L, -1), _cu(y2).view(N * L, -1) if pairs == 2 else None

        def run(ln, fill, seed):
            f = (lambda t, s: t) if ln is None else (lambda t, s: LR.fill_padding(t, lens, fill, seed + s))
            gx = _cu(f(x, 0)).view(N * T, -1)
            gx2 = _cu(f(x2, 1)).view(N * T, -1) if pairs == 2 else None
            gp = _cu(torch.stack([f(yprev[g], 2 + g) for g in range(G)])) if epi == 2 else None
            out = _seven(G, N, T, L)
            ops.hie_affinity_levels(gx, 2 * E, gy, lvy, G, N, L, T, E, x2=gx2, lvx2=E, y2=gy2, lvy2=lvy, epi=epi, yprev=gp, out=out,
                                    lens=None if ln is None else _i32(ln))
            torch.cuda.synchronize()
            return dict(out=out), gx, gx2, gp

        a = run(lens, "rand", 180)[0]
        assert _same(a, run(lens, NAN, 190)[0]) and _same(a, run(lens, "rand", 180)[0])
        ref = torch.stack([LR.affinity(x[:, :, 2 * g * E:2 * g * E + E], y[:, :, g * lvy:g * lvy + E], lens,
                                       x2=x2[:, :, g * E:(g + 1) * E] if pairs == 2 else None,
                                       y2=y2[:, :, g * lvy:g * lvy + E] if pairs == 2 else None, epi=epi,
                                       yprev=yprev[g] if epi == 2 else None) for g in range(G)])
        rep.parity("pairs%d" % pairs, a["out"].view(G * N, T, L), ref.view(G * N, T, L), _aff_tol(epi))    # per level and sample
        for g in range(G):
            assert _zero_rows(a["out"][g], pad), g
        assert _same(run([T] * N, None, 0)[0], run(None, None, 0)[0])           # lens = T: vqf_hie_affinity_levels' bits
        if G == 1:                                                             # the same kernel as vqf_hie_affinity_len: the same bits
            _, gx, gx2, gp = run(lens, "rand", 180)
            one = ops.hie_affinity(gx[:, :E], gy[:, :E], N, L, T, x2=None if gx2 is None else gx2[:, :E],
                                   y2=None if gy2 is None else gy2[:, :E], epi=epi, yprev=gp, out=_seven(N, T, L), lens=_i32(lens))
            assert torch.equal(one.view(-1), a["out"].view(-1))
    rep.flush()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_null_and_misaligned_lens_are_refused(ops):
    """every entry point: lens = NULL is VQF_E_BADARG, a lens pointer two bytes off alignment a non-zero code; both before any
    launch (the outputs keep their 7.0).  The other arguments are valid, so a call that got through would stay in bounds."""
    N, T, E, L, G, U, V = 2, 3, 32, 3, 1, 2, 9
    lib, p, st = ops._lib(), ops._ptr, ops._stream()
    zin, out = torch.zeros(4096, device="cuda"), _seven(4096)
    ids, i32 = torch.zeros(N * T, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    u8 = torch.zeros(N * T * E, dtype=torch.uint8, device="cuda")
    odd = _i32([1] * 9)[1:]                             # 4-byte aligned; + 2 bytes below is not
    z, o, i = p(zin), p(out), p(i32)
    calls = {
        "embed_tanh_fwd_len": lambda lp: lib.vqf_embed_tanh_fwd_len(z, p(ids), lp, N, T, V, E, o, st),
        "embed_tanh_bwd_len": lambda lp: lib.vqf_embed_tanh_bwd_len(z, z, p(ids), lp, N, T, V, E, o, st),
        "phrase_ngram_fwd_len": lambda lp: lib.vqf_phrase_ngram_fwd_len(z, 6 * E, z, lp, N, T, E, o, E, p(u8), st),
        "phrase_ngram_bwd_len": lambda lp: lib.vqf_phrase_ngram_bwd_len(z, E, z, E, p(u8), lp, N, T, E, o, 6 * E, st),
        "dropout_bt_len": lambda lp: lib.vqf_dropout_bt_len(z, T * E, E, None, 0, 0.0, lp, N, T, E, o, T * E, E, st),
        "glimpse_pool_fwd_len": lambda lp: lib.vqf_glimpse_pool_fwd_len(z, z, lp, N, T, E, G, 0, o, p(out[2048:]), st),
        "glimpse_pool_bwd_len": lambda lp: lib.vqf_glimpse_pool_bwd_len(z, None, z, z, lp, N, T, E, G, 0, o, p(out[2048:]), st),
        "glimpse_pool_fwd_grouped_len": lambda lp: lib.vqf_glimpse_pool_fwd_grouped_len(z, z, i, lp, N, U, T, E, G, o, p(out[2048:]), st),
        "glimpse_pool_bwd_grouped_len": lambda lp: lib.vqf_glimpse_pool_bwd_grouped_len(z, None, z, z, i, i, i, lp, N, U, T, E, G, o,
                                                                                       p(out[2048:]), st),
        "hie_affinity_len": lambda lp: lib.vqf_hie_affinity_len(z, E, z, E, None, 0, None, 0, 0, None, None, 0, 0.0, lp, N, L, E, T, o, st),
        "hie_affinity_levels_len": lambda lp: lib.vqf_hie_affinity_levels_len(z, E, 0, z, E, 0, None, 0, 0, None, 0, 0, G, 0, None, lp,
                                                                              N, L, E, T, o, st),
        "tanh_bwd_rows_len": lambda lp: lib.vqf_tanh_bwd_rows_len(z, z, lp, N, T, 4, o, st),
    }
    assert len(calls) == 12
    for name, call in calls.items():
        assert call(None) == -1, name                   # VQF_E_BADARG
        assert call(odd.data_ptr() + 2) != 0, name
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    # with an aligned lens the same argument lists are accepted: the refusals above were about lens, not about another argument
    for name, call in calls.items():
        assert call(p(odd)) == 0, name
    torch.cuda.synchronize()

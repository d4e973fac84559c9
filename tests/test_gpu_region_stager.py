"""RegionStager and vqf_region_rows_stage: packed region features from pinned host slots to the tensors the models take.

Every comparison is bit-exact: the kernel copies fp32 rows or widens fp16 rows (exact for every fp16 value), the stager moves
bytes, and the models see the same tensors whichever way those arrived."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import mfb_packed_ref as PR
import test_gpu_hie_ladder_packed as HL
import test_gpu_mfb_regions as TR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.5
# the smallest and the largest fp16 subnormal, +-0, +-65504 (the largest finite value), +-inf
SPECIALS = np.array([0x0001, 0x03FF, 0x8001, 0x83FF, 0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00], dtype=np.uint16).view(np.float16)


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rows(R, D, dtype, seed):
    g = np.random.default_rng(seed)
    return ((g.random((R, D), dtype=np.float32) * 1.9 + 0.1) * (g.integers(0, 2, (R, D)) * 2 - 1).astype(np.float32)).astype(dtype)


def _padded_ref(rows32, spans, L):
    """numpy: rows32 (R, D) fp32 placed at u*L + l by (start, cnt) spans, +0.0 behind every count"""
    out = np.zeros((len(spans), L, rows32.shape[1]), dtype=np.float32)
    for u, (start, cnt) in enumerate(spans):
        out[u, :cnt] = rows32[start:start + cnt]
    return out


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------
# the smallest shape; odd counts; D % 8 != 0 (fp16 rows only 8-byte aligned); D = 2048 with counts 1, L - 1 and L, where an image is
# more than the 64 x 256 vectors one trip of the grid-stride loop covers; L = 1024 at the narrowest D
KCASES = [(1, 1, 4, [1]), (3, 5, 8, [5, 1, 3]), (4, 7, 68, [7, 2, 1, 6]), (5, 50, 2048, [50, 1, 17, 49, 2]), (2, 1024, 4, [1024, 1])]


@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("U,L,D,counts", KCASES, ids=["U%d_L%d_D%d" % c[:3] for c in KCASES])
def test_kernel_is_bit_equal_to_numpy(ops, U, L, D, counts, dtype, form):
    R = sum(counts)
    src = _rows(R, D, dtype, U * 100 + L)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    if dtype is np.float16:              # first / last element of the first / last real row of every image
        k = 0
        for u in range(U):
            for r in (off[u], off[u + 1] - 1):
                for c in (0, D - 1):
                    src[r, c] = SPECIALS[k % len(SPECIALS)]
                    k += 1
        src[0, :4], src[R - 1, -4:] = SPECIALS[:4], SPECIALS[4:8]          # and all ten in every case, whatever U is
        src[0, -1], src[R - 1, 0] = SPECIALS[8], SPECIALS[9]
    want = src.astype(np.float32)
    dsrc = torch.from_numpy(src).to(DEV)
    if form == "packed":
        out = torch.full((R, D), float("nan"), device=DEV)
        got = ops.region_rows_stage(dsrc, out=out)
        assert ops.region_rows_stage(dsrc).shape == (R, D)
    else:
        out = torch.full((U, L, D), float("nan"), device=DEV)
        got = ops.region_rows_stage(dsrc, torch.from_numpy(off).to(DEV), L, out=out)
        want = _padded_ref(want, [(int(off[u]), counts[u]) for u in range(U)], L)
        pad = np.ones((U, L), dtype=bool)
        for u in range(U):
            pad[u, :counts[u]] = False
        assert (_bits(got.cpu().numpy())[pad] == 0).all()                  # +0.0, the sign bit included
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))


# The categories of test_gpu_hie_ladder_packed.py::BAD_OFFSETS at U = 5, L = 20, R = 51 -- negative, decreasing, beyond R, count 0,
# count > L, all at once --, every entry at most L = 20 rows outside [0, R], so that with L guard rows on each side even an access
# that ignored the clamp would stay inside the allocations.
GU, GL, GD, GCOUNTS = 5, 20, 64, [1, 20, 19, 7, 4]
BAD_OFFSETS = [("well_formed", None),
               ("negative", [-20, -7, 5, 9, 30, 51]),
               ("decreasing", [0, 20, 12, 3, 3, 51]),
               ("beyond_R", [0, 40, 52, 60, 71, 51]),
               ("count_zero", [0, 1, 1, 21, 21, 21]),
               ("counts_above_L", [0, 25, 26, 51, 30, 71])]


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name,offs", BAD_OFFSETS, ids=[b[0] for b in BAD_OFFSETS])
def test_guard_rows_stay_untouched_whatever_the_offsets_hold(vqa, name, offs, dtype):
    U, L, D, R, G = GU, GL, GD, sum(GCOUNTS), GL
    good = np.concatenate([[0], np.cumsum(GCOUNTS)]).tolist()
    offs = good if offs is None else offs
    assert all(-L <= o <= R + L for o in offs)
    tdt = torch.float16 if dtype is np.float16 else torch.float32
    sbuf = torch.full((R + 2 * G, D), SENTINEL, dtype=tdt, device=DEV)      # src and dst are slices of larger allocations
    src = _rows(R, D, dtype, 5)
    sbuf[G:G + R] = torch.from_numpy(src).to(DEV)
    before = sbuf.clone()
    dbuf = torch.full((U * L + 2 * G, D), SENTINEL, device=DEV)
    roff = torch.tensor(offs, dtype=torch.int32, device=DEV)
    lib = vqa.lib.load()
    esz = 2 if dtype is np.float16 else 4
    rc = lib.vqf_region_rows_stage(ctypes.c_void_p(sbuf.data_ptr() + G * D * esz), int(dtype is np.float16),
                                   ctypes.c_void_p(roff.data_ptr()), U, R, L, D, ctypes.c_void_p(dbuf.data_ptr() + G * D * 4),
                                   vqa.ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    guard = torch.full((G, D), SENTINEL, device=DEV)
    assert torch.equal(dbuf[:G], guard) and torch.equal(dbuf[G + U * L:], guard) and torch.equal(sbuf, before)
    spans = PR.clamped_spans(torch.tensor(offs), R, L)
    for start, cnt in spans:
        assert 0 <= start and 1 <= cnt <= L and start + cnt <= R
    want = _padded_ref(src.astype(np.float32), spans, L)
    got = dbuf[G:G + U * L].view(U, L, D).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    for u in range(U):                                                     # the owners with well-formed offsets keep their bits
        if offs[u] == good[u] and offs[u + 1] == good[u + 1]:
            assert spans[u] == (good[u], GCOUNTS[u]) and np.array_equal(got[u, :GCOUNTS[u]], src[good[u]:good[u + 1]].astype(np.float32))


def test_refusals_through_ops(vqa, ops):
    E = vqa.VqfError
    z = lambda *s, **k: torch.zeros(s, device=DEV, **k)
    roff = torch.tensor([0, 2, 5], dtype=torch.int32, device=DEV)
    assert ops.region_rows_stage(z(5, 8), roff, 3).shape == (2, 3, 8)
    with pytest.raises(E, match="D"):
        ops.region_rows_stage(z(5, 6))                                     # D = 6
    with pytest.raises(E, match="L"):
        ops.region_rows_stage(z(5, 8), roff, 1025)                         # L = 1025
    with pytest.raises(E, match="U"):
        ops.region_rows_stage(z(5, 8), roff[:1], 3)                        # U = 0
    with pytest.raises(E, match="ALIGN"):
        ops.region_rows_stage(z(41)[1:].view(5, 8))                        # fp32 rows 4 bytes off a 16-byte boundary
    with pytest.raises(E, match="ALIGN"):
        ops.region_rows_stage(z(42, dtype=torch.float16)[2:].view(5, 8))   # fp16 rows 4 bytes off an 8-byte boundary
    with pytest.raises(E, match="ALIGN"):
        ops.region_rows_stage(z(5, 8), out=z(41)[1:].view(5, 8))
    with pytest.raises(E, match="roff"):
        ops.region_rows_stage(z(5, 8), roff, 3, out=z(3, 3, 8))            # a roff of the wrong length for the result
    with pytest.raises(E, match="roff"):
        ops.region_rows_stage(z(5, 8), roff.to(torch.int64), 3)
    with pytest.raises(E, match="roff"):
        ops.region_rows_stage(z(5, 8), roff.view(1, 3), 3)
    with pytest.raises(E, match="L"):
        ops.region_rows_stage(z(5, 8), roff)                               # the padded form without L
    with pytest.raises(E):
        ops.region_rows_stage(torch.zeros(5, 8))                           # no CPU path
    with pytest.raises(E):
        ops.region_rows_stage(z(5, 8).to(torch.bfloat16))


# ---- the stager ------------------------------------------------------------------------------------------------------------------------
SU, SL, SD, SROWS = 6, 9, 24, 30
# five batches of different U and R: one image; exactly max_rows with max_images; counts 1 and L; ...
SBATCHES = [[4, 9, 1], [7], [9, 1, 9, 2, 8, 1], [1, 1], [3, 9, 9, 5]]
_SFEATS = {}


def _sfeats(k, counts, D=SD):
    """the host features of stager batch k, computed once and never modified"""
    if k not in _SFEATS:
        g = np.random.default_rng(1000 + k)
        _SFEATS[k] = [((g.random((c, D), dtype=np.float32) * 2 - 1) * 3).astype(np.float32) for c in counts]
    return _SFEATS[k]


def _rounded(feats, storage):
    return [f.astype(np.float16).astype(np.float32) for f in feats] if storage == "fp16" else feats


def _check_batch(vqa, got, feats, storage, form, L):
    ref = vqa.pack_region_features(_rounded(feats, storage))
    if form == "packed":
        assert isinstance(got, vqa.PackedRegions) and got.max_regions == L and isinstance(got.max_regions, int)
        assert got.rows.dtype == torch.float32 and got.offsets.dtype == torch.int32
        assert torch.equal(got.rows.cpu(), ref.rows) and torch.equal(got.offsets.cpu(), ref.offsets.to(torch.int32))
    else:
        img, length = got
        wimg, wlen = vqa.PackedRegions(ref.rows, ref.offsets, L).unpack()
        assert img.dtype == torch.float32 and length.dtype == torch.int32
        assert torch.equal(img.cpu(), wimg) and torch.equal(length.cpu(), wlen.to(torch.int32))
        assert not bool(torch.signbit(img).logical_and(img == 0).any())    # +0.0 padding (the features hold no zero)


@pytest.mark.parametrize("route", ["submit", "host_slot"])
@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("depth", [2, 3])
def test_stager_keeps_order_and_content(vqa, depth, storage, form, route):
    assert sum(SBATCHES[2]) == SROWS and len(SBATCHES[2]) == SU
    st = vqa.RegionStager(SU, channels=SD, max_regions=SL, max_rows=SROWS, storage=storage, form=form, depth=depth)

    def put(k):
        feats = _sfeats(k, SBATCHES[k])
        if route == "submit":
            return st.submit(feats)
        rows, counts = st.host_slot()
        assert rows.shape == (SROWS, SD) and rows.dtype == (np.float16 if storage == "fp16" else np.float32)
        assert counts.shape == (SU,) and counts.dtype == np.int32
        r = 0
        for u, f in enumerate(feats):
            rows[r:r + len(f)] = f
            counts[u] = len(f)
            r += len(f)
        st.commit(len(feats))

    outs = []
    put(0)
    for k in range(5):
        if k + 1 < 5:
            put(k + 1)                               # batch k + 1 is queued before batch k is consumed
        feats, idx = st.next()
        assert idx is None
        if form == "packed":
            feats.rows.mul_(1.0)                     # some work on the compute stream
        outs.append(feats)                           # all five are held until the end: fresh allocations, not the slots
    torch.cuda.synchronize()
    for k in range(5):
        _check_batch(vqa, outs[k], _sfeats(k, SBATCHES[k]), storage, form, SL)


@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_one_shot_form(vqa, storage, form):
    feats = _sfeats(0, SBATCHES[0])
    got, idx = vqa.stage_regions(feats, storage=storage, form=form)
    assert idx is None
    _check_batch(vqa, got, feats, storage, form, max(SBATCHES[0]))


IDS = ["b", "a", "a", "c", "b", "a", "c"]                                  # repeats in scattered order: 3 distinct images of 7


def test_shared_images_stage_only_the_distinct_ones(vqa):
    first, index = vqa.group_batch(IDS)
    per_image = _sfeats(2, SBATCHES[2])[:3]
    order = {"b": 0, "a": 1, "c": 2}
    per_question = [per_image[order[i]] for i in IDS]
    st = vqa.RegionStager(3, channels=SD, max_regions=SL, max_questions=7)
    st.submit(per_question, IDS)
    got, idx = st.next()
    assert idx.dtype == torch.int64 and idx.device.type == "cuda" and torch.equal(idx.cpu(), index)
    assert first.tolist() == [0, 1, 3]
    _check_batch(vqa, got, per_image, "fp32", "packed", SL)                # three images' rows, not seven
    got1, idx1 = vqa.stage_regions(per_question, IDS)
    assert torch.equal(idx1.cpu(), index) and torch.equal(got1.rows, got.rows) and got1.max_regions == 9
    # more questions than max_questions, ids that do not match the features
    with pytest.raises(ValueError):
        vqa.RegionStager(3, channels=SD, max_regions=SL, max_questions=6).submit(per_question, IDS)
    with pytest.raises(ValueError):
        st.submit(per_question, IDS[:6])


def test_errors_leave_the_stager_usable(vqa):
    E = vqa.VqfError
    st = vqa.RegionStager(3, channels=SD, max_regions=SL, max_rows=12, depth=1)
    good = _sfeats(3, SBATCHES[3])
    with pytest.raises(E):
        st.next()                                                           # nothing committed
    with pytest.raises(E):
        st.commit(1)                                                        # commit() without host_slot()
    bad = [[], [np.zeros((0, SD), np.float32)], [np.zeros((2, SD + 4), np.float32)], [np.ones((SL + 1, SD), np.float32)],
           [np.ones((7, SD), np.float32), np.ones((6, SD), np.float32)], [np.ones((1, SD), np.float32)] * 4]
    for feats in bad:
        with pytest.raises(ValueError):
            st.submit(feats)
    for images, counts, index in ((0, [1, 1, 1], None), (4, [1, 1, 1], None), (2, [1, 0, 1], None), (2, [1, SL + 1, 1], None),
                                  (3, [5, 5, 5], None), (2, [1, 1, 1], [0, 2]), (2, [1, 1, 1], [0, -1]), (2, [1, 1, 1], [0] * 4),
                                  (2, [1, 1, 1], [0.0, 1.0])):
        rows, cnt = st.host_slot()
        cnt[:] = counts
        with pytest.raises(ValueError):
            st.commit(images, index)
    st.submit(good)                                                         # the single slot is still free after every refusal
    with pytest.raises(E):
        st.host_slot()                                                      # ... and now in flight
    with pytest.raises(E):
        st.submit(good)
    got, _ = st.next()
    _check_batch(vqa, got, good, "fp32", "packed", SL)
    st.submit(good)
    _check_batch(vqa, st.next()[0], good, "fp32", "packed", SL)


# ---- the staged batch feeds the models -------------------------------------------------------------------------------------------------
def _host_features(img, counts):
    """(U, L, D) GPU tensor + counts -> the loader's list of (K_u, D) numpy arrays"""
    return [img[u, :int(c)].cpu().numpy().copy() for u, c in enumerate(counts.tolist())]


def _staged_calls(vqa, call, feats, L, idx):
    """call(features, img_index) on every storage x form of the stager against the same call on the tensors moved by .to(DEV)"""
    for storage in ("fp32", "fp16"):
        ref = vqa.pack_region_features(_rounded(feats, storage))
        ref = vqa.PackedRegions(ref.rows, ref.offsets, L)
        want_packed = call(ref.to(DEV), idx)
        uimg, ulen = ref.unpack()
        want_pair = call((uimg.to(DEV), ulen.to(DEV)), idx)
        for form, want in (("packed", want_packed), ("padded", want_pair)):
            st = vqa.RegionStager(len(feats), channels=feats[0].shape[1], max_regions=L, max_questions=16, storage=storage, form=form)
            st.commit(vqa.data_loader.pack_into(*st.host_slot(), feats), None if idx is None else idx.cpu())
            staged, sidx = st.next()
            assert (sidx is None) == (idx is None) and (idx is None or torch.equal(sidx, idx))
            got = call(staged, sidx)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (storage, form)


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("mhb", [False, True], ids=["mfb", "mhbcoatt"])
def test_staged_batch_feeds_mfb_and_mhbcoatt(vqa, mhb, shared):
    model, img, counts, q, tgt, idx = TR._model(vqa, TR.MHB3 if mhb else TR.MFB3, mhb, shared)
    model.set_keep_masks()
    model.eval()

    def call(features, index):
        with torch.no_grad():
            return (model.forward(features, q) if index is None else model.forward(features, q, img_index=index),)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # MHBCoAtt's question LSTM at this hidden width runs on nn.LSTM
        _staged_calls(vqa, call, _host_features(img, counts), img.shape[1], idx)


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("coatt", HL.MODES)
def test_staged_batch_feeds_the_ladder(vqa, coatt, shared):
    U, N, T, L, E, D = (3, 7, 14, 50, 64, 96) if shared else (5, 5, 14, 50, 64, 96)
    m = HL._model(vqa, L, E, D, coatt).eval()
    packed, ids, lens, counts = HL._inputs(vqa, U, N, L, D, T, counts=HL._shared_counts(L) if shared else None)
    idx = torch.tensor(HL.SHARED_IDX, device=DEV) if shared else None
    off = packed.offsets.tolist()
    feats = [packed.rows[off[u]:off[u + 1]].cpu().numpy().copy() for u in range(U)]

    def call(features, index):
        with torch.no_grad():
            return HL._call(m, features, ids, lens, index)

    _staged_calls(vqa, call, feats, L, idx)


def test_questions_that_share_images_equal_the_per_question_call(vqa):
    """submit(per-question features, image_ids): the model call on the staged distinct images with the staged img_index against the
    call on the per-question features (one image per question, no index)"""
    model, img, counts, q, tgt, idx = TR._model(vqa, TR.MFB3, False, True)
    model.set_keep_masks()
    model.eval()
    per_image = _host_features(img, counts)
    ids = ["img%d" % i for i in TR.INDEX]
    per_question = [per_image[i] for i in TR.INDEX]
    first, index = vqa.group_batch(ids)
    L = img.shape[1]
    st = vqa.RegionStager(len(ids), channels=img.shape[2], max_regions=L)
    st.submit(per_question, ids)
    st.submit(per_question)
    staged, sidx = st.next()
    every, none = st.next()
    assert none is None and torch.equal(sidx.cpu(), index) and staged.offsets.numel() == len(first) + 1 == 3
    assert every.offsets.numel() == len(ids) + 1
    with torch.no_grad():
        a = model.forward(staged, q, img_index=sidx)
        b = model.forward(every, q)
    print("shared vs per-question: max abs diff %.3e, max |b| %.3e" % (float((a - b).abs().max()), float(b.abs().max())))
    assert torch.equal(a, b)


def test_no_host_read_between_next_and_the_forward(vqa, monkeypatch):
    """the guards of test_gpu_hie_ladder_packed.py::test_structure around next() + the model forward"""
    U, N, T, L, E, D = 3, 7, 14, 50, 64, 96
    m = HL._model(vqa, L, E, D, "parallel").eval()
    packed, ids, lens, counts = HL._inputs(vqa, U, N, L, D, T, counts=HL._shared_counts(L))
    off = packed.offsets.tolist()
    feats = [packed.rows[off[u]:off[u + 1]].cpu().numpy().copy() for u in range(U)]
    stagers = [vqa.RegionStager(U, channels=D, max_regions=L, max_questions=N, storage=s, form=f)
               for s in ("fp32", "fp16") for f in ("packed", "padded")]
    for st in stagers:
        st.commit(vqa.data_loader.pack_into(*st.host_slot(), feats), HL.SHARED_IDX)
    torch.cuda.synchronize()

    def guard(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("a GPU tensor was read on the host (Tensor.%s)" % name)
            return real(self, *a, **k)
        return f

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize between next() and the forward")

    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, guard(name))
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    outs = []
    with torch.no_grad():
        for st in stagers:
            staged, sidx = st.next()
            outs.append(m(staged, ids, lens, sidx)[0])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs)

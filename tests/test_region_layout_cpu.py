"""grouping.RegionLayout -- where the image rows of a batch are, for the fusion, attention and ladder nodes -- and mfb.region_layout,
the one place that turns a call form (a tensor, the pair (img, img_length), a PackedRegions, each with or without img_index) into
one: every field of the six forms against hand-written values, the two transformations the ladder uses, and each refusal the three
models raise from the helpers that moved there, with the text they always had.  Plain torch on CPU tensors."""
import importlib

import pytest
import torch

INDEX, U, N, L = [2, 0, 2, 2, 0], 3, 5, 7              # image 1 has no question
IDX, ORDER, GRP_OFF = [2, 0, 2, 2, 0], [1, 4, 0, 2, 3], [0, 2, 2, 5]
COUNTS, LENS_U, LENS_Q = [0, 99, 3], [1, 7, 3], [3, 1, 3, 3, 1]
OFFSETS, PADDED_LENS = [0, 7, 8, 12], [7, 1, 4]


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    return vqa_amd


@pytest.fixture(scope="module")
def gr(vqa):
    return importlib.import_module(vqa.__name__ + ".host.grouping")


def _is(t, want, dtype=torch.int32):
    return torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous() and t.tolist() == want


def _grouped_fields(lay):
    assert _is(lay.idx, IDX) and _is(lay.order, ORDER) and _is(lay.grp_off, GRP_OFF)
    assert lay.grouped and lay.grp[0] is lay.idx and lay.grp[1] is lay.order and lay.grp[2] is lay.grp_off and len(lay.grp) == 3


def _ungrouped_fields(lay):
    assert lay.idx is None and lay.order is None and lay.grp_off is None and lay.grp is None and not lay.grouped


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_the_six_forms_field_by_field(gr, dtype):
    t = lambda x: torch.tensor(x, dtype=dtype)
    plain = gr.RegionLayout(N, N, L)
    assert (plain.N, plain.U, plain.L, plain.R) == (5, 5, 7, 35) and plain.plain and not (plain.counted or plain.packed)
    _ungrouped_fields(plain)
    assert plain.lens_u is None and plain.lens_q is None and plain.roff is None
    assert plain.padded() is plain

    counts = gr.RegionLayout(U, U, L, img_length=t(COUNTS))
    assert (counts.N, counts.U, counts.L, counts.R) == (3, 3, 7, 21) and counts.counted and not (counts.plain or counts.packed)
    _ungrouped_fields(counts)
    assert _is(counts.lens_u, LENS_U) and counts.lens_q is counts.lens_u and counts.roff is None      # clamped to [1, L]

    index = gr.RegionLayout(N, U, L, img_index=t(INDEX))
    assert (index.N, index.U, index.L, index.R) == (5, 3, 7, 21) and not (index.plain or index.counted or index.packed)
    _grouped_fields(index)
    assert index.lens_u is None and index.lens_q is None and index.roff is None

    both = gr.RegionLayout(N, U, L, img_index=t(INDEX), img_length=t(COUNTS))
    assert (both.N, both.U, both.L, both.R) == (5, 3, 7, 21) and both.counted and not (both.plain or both.packed)
    _grouped_fields(both)
    assert _is(both.lens_u, LENS_U) and _is(both.lens_q, LENS_Q) and both.roff is None                # lens_q = lens_u[idx]

    packed = gr.RegionLayout(U, U, L, offsets=t(OFFSETS), R=12)
    assert (packed.N, packed.U, packed.L, packed.R) == (3, 3, 7, 12) and packed.packed and not (packed.plain or packed.counted)
    _ungrouped_fields(packed)
    assert packed.lens_u is None and packed.lens_q is None and _is(packed.roff, OFFSETS)              # the counts ride in roff

    pidx = gr.RegionLayout(N, U, L, img_index=t(INDEX), offsets=t(OFFSETS), R=12)
    assert (pidx.N, pidx.U, pidx.L, pidx.R) == (5, 3, 7, 12) and pidx.packed and not (pidx.plain or pidx.counted)
    _grouped_fields(pidx)
    assert pidx.lens_u is None and pidx.lens_q is None and _is(pidx.roff, OFFSETS)

    # padded(): the same batch after the rows were laid out padded
    p = packed.padded()
    assert (p.N, p.U, p.L, p.R) == (3, 3, 7, 21) and p.roff is None and p.counted and not p.packed
    assert _is(p.lens_u, PADDED_LENS) and p.lens_q is p.lens_u
    _ungrouped_fields(p)
    p = pidx.padded()
    assert (p.N, p.U, p.L, p.R) == (5, 3, 7, 21) and p.roff is None and p.counted and not p.packed
    assert _is(p.lens_u, PADDED_LENS) and _is(p.lens_q, [4, 7, 4, 4, 7])
    _grouped_fields(p)
    assert p.idx is pidx.idx and packed.roff is not None                                              # the source is untouched

    # per_question(): behind the ladder's row-block gather
    pq = both.per_question()
    assert (pq.N, pq.U, pq.L, pq.R) == (5, 5, 7, 35) and pq.lens_u is pq.lens_q and pq.lens_q is both.lens_q and pq.roff is None
    _ungrouped_fields(pq)
    pq = index.per_question()
    assert pq.plain and pq.U == pq.N == 5


def test_a_layout_is_immutable_and_has_no_dict(gr):
    lay = gr.RegionLayout(N, U, L, img_index=torch.tensor(INDEX))
    with pytest.raises(AttributeError):
        lay.N = 3
    with pytest.raises(AttributeError):
        lay.extra = 1
    assert not hasattr(lay, "__dict__")


def test_nothing_reads_a_tensor_on_the_host(gr):
    """meta tensors have no values: whatever called .item() / .tolist() / .cpu() on one would raise"""
    m = lambda n: torch.empty(n, dtype=torch.int64, device="meta")
    lay = gr.RegionLayout(N, U, L, img_index=m(N), img_length=m(U))
    assert lay.idx.device.type == "meta" and tuple(lay.lens_q.shape) == (N,) and tuple(lay.grp_off.shape) == (U + 1,)
    assert lay.grouped and lay.counted and not lay.packed and lay.grp is not None
    assert tuple(lay.per_question().lens_u.shape) == (N,)
    lay = gr.RegionLayout(N, U, L, img_index=m(N), offsets=m(U + 1), R=12)
    assert lay.roff.dtype == torch.int32 and lay.roff.device.type == "meta"
    p = lay.padded()
    assert tuple(p.lens_u.shape) == (U,) and tuple(p.lens_q.shape) == (N,) and p.lens_q.dtype == torch.int32


def test_the_helpers_keep_their_names_and_results(vqa, gr):
    hl = importlib.import_module(vqa.__name__ + ".host.hie_ladder")
    mfb = importlib.import_module(vqa.__name__ + ".host.mfb")
    assert hl._group_index is gr._group_index and callable(mfb.split_region_features) and vqa.PackedRegions is gr.PackedRegions
    idx, order, off = gr._group_index(torch.tensor(INDEX), U)
    assert _is(idx, IDX) and _is(order, ORDER) and _is(off, GRP_OFF)
    lens_q, lens_u = gr._region_lens(torch.tensor(COUNTS), L, idx)
    assert _is(lens_u, LENS_U) and _is(lens_q, LENS_Q) and _is(gr._region_lens(torch.tensor(COUNTS), L), LENS_U)


# ---- the refusals that moved into mfb.region_layout --------------------------------------------------------------------------------
def _models(vqa):
    import types
    cfg = types.SimpleNamespace(q_vocab_size=20, a_vocab_size=6, emb_dim=8, hidden_dim=16, num_layers=1, model_name="mfb", glove=False,
                                img_feature_channel=12, img_feature_dim=L, batch_size=N)
    ladder = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=32, hidden_size=10, output_size=6)
    cfg2 = types.SimpleNamespace(**dict(vars(cfg), model_name="mhb_coAtt"))
    return [("MFB", vqa.MFB(cfg)), ("MHBCoAtt", vqa.MHBCoAtt(cfg2)), ("HieCoAttenLadder", ladder)]


def test_moved_refusals_keep_type_and_text(vqa, gr):
    mfb = importlib.import_module(vqa.__name__ + ".host.mfb")
    q = torch.ones(N, 4, dtype=torch.long)
    img = torch.zeros(U, L, 12)
    ok = lambda *a: None
    lay = lambda feats, idx=None, **kw: mfb.region_layout("WHO", feats, q, idx, ok, ok, **kw)
    idx = torch.tensor(INDEX)
    # the happy path on CPU tensors: the checks need no GPU
    t, layout = lay((img, torch.tensor(COUNTS)), idx)
    assert t is img and _is(layout.lens_q, LENS_Q) and layout.grouped and (layout.N, layout.U, layout.L, layout.R) == (5, 3, 7, 21)
    t, layout = lay(torch.zeros(N, L, 12))
    assert layout.plain and (layout.N, layout.U) == (5, 5)
    # img_index: dtype, shape, device
    for bad, what in ((idx.float(), "WHO: img_index must be an int64 or int32 tensor, got torch.float32"), (INDEX, "img_index must be an int64 or int32 tensor, got list"),
                      (idx[:4], r"img_index must have shape \(N,\) = \(5,\), got \(4,\)"), (idx.view(-1, 1), r"img_index must have shape \(N,\)"),
                      (idx.to("meta"), r"img_index must be on the questions' device \(cpu\), got meta")):
        with pytest.raises(vqa.VqfError, match=what):
            lay(img, bad)
    # img_length: dtype, shape (one count per image: U with img_index), device
    cnt = torch.tensor(COUNTS)
    for bad, what in ((cnt.float(), "WHO: img_length must be an int64 or int32 tensor, got torch.float32"), (COUNTS, "img_length must be an int64 or int32 tensor, got list"),
                      (torch.ones(N, dtype=torch.long), r"img_length must have shape \(3,\) \(one region count per image\), got \(5,\)"),
                      (cnt.to("meta"), r"img_length must be on the questions' device \(cpu\), got meta")):
        with pytest.raises(vqa.VqfError, match=what):
            lay((img, bad), idx)
    # a pair of another arity; a PackedRegions inside a pair
    rows = torch.zeros(12, 12)
    good = vqa.PackedRegions(rows, torch.tensor(OFFSETS), L)
    for bad in ((img,), (img, cnt, 3), (None, cnt)):
        with pytest.raises(vqa.VqfError, match="img_features must be a tensor or the pair"):
            lay(bad, idx)
    for bad in ((good, cnt), (good, None), [good, good]):
        with pytest.raises(vqa.VqfError, match="a PackedRegions carries its own counts and is passed on its own, not inside a pair"):
            lay(bad, idx)
    # offsets: dtype, shape (one more than the images), device; max_regions out of range; rows
    t, layout = lay(good, idx)
    assert t.shape == (12, 12) and layout.packed and layout.grouped and _is(layout.roff, OFFSETS) and layout.R == 12
    P = vqa.PackedRegions
    off = torch.tensor(OFFSETS)
    for bad, what in ((P(rows, off.float(), L), "PackedRegions.offsets must be an int64 or int32 tensor, got torch.float32"),
                      (P(rows, OFFSETS, L), "PackedRegions.offsets must be an int64 or int32 tensor, got list"),
                      (P(rows, off.view(-1, 1), L), r"PackedRegions.offsets must have shape \(4,\) \(one more than the images\), got \(4, 1\)"),
                      (P(rows, off.to("meta"), L), r"PackedRegions.offsets must be on the questions' device \(cpu\), got meta"),
                      (P(rows, off, 0), r"PackedRegions.max_regions must be a Python int in \[1, 1024\], got 0"),
                      (P(rows, off, 1025), "PackedRegions.max_regions must be a Python int in .* got 1025"),
                      (P(rows, off, 7.0), "PackedRegions.max_regions must be a Python int"),
                      (P(rows.double(), off, L), r"PackedRegions.rows must be a 2-D fp32 tensor \(R, D\) with R >= 1"),
                      (P(rows.to("meta"), off, L), r"PackedRegions.rows must be on the questions' device \(cpu\), got meta")):
        with pytest.raises(vqa.VqfError, match=what):
            lay(bad, idx)
    with pytest.raises(vqa.VqfError, match=r"PackedRegions.offsets must have shape \(6,\)"):          # without img_index: one owner per question
        lay(good)
    # fp32 only, whatever the model
    for dt in ("bf16", "bf16-img", "bf16-all", "bf16-att"):
        with pytest.raises(vqa.VqfError, match="WHO: PackedRegions is fp32 only.*%s" % dt):
            lay(good, idx, gemm_dtype=dt)
        with pytest.raises(vqa.VqfError, match="WHO: img_index is fp32 only.*%s" % dt):
            lay(img, idx, gemm_dtype=dt)
        with pytest.raises(vqa.VqfError, match="WHO: img_length is fp32 only.*%s" % dt):
            lay((img, cnt), gemm_dtype=dt)
    # the models' own refusals run inside, before anything is made on the device
    def no(*a):
        raise vqa.VqfError("model says no")
    with pytest.raises(vqa.VqfError, match="model says no"):
        mfb.region_layout("WHO", img, q, None, no, ok)
    with pytest.raises(vqa.VqfError, match="model says no"):
        mfb.region_layout("WHO", good, q, idx, ok, no)


def test_each_model_raises_them_under_its_own_name(vqa):
    """once per model and helper, through forward(): CPU tensors, so a call that passes the moved checks ends at 'GPU tensors'"""
    q = torch.ones(N, 4, dtype=torch.long)
    img, cnt, idx = torch.zeros(U, L, 12), torch.tensor(COUNTS), torch.tensor(INDEX)
    good = vqa.PackedRegions(torch.zeros(12, 12), torch.tensor(OFFSETS), L)
    for who, model in _models(vqa):
        call = lambda feats, index=None: model(feats, q, img_index=index)
        with pytest.raises(vqa.VqfError, match="%s: a PackedRegions carries its own counts" % who):
            call((good, cnt), idx)
        with pytest.raises(vqa.VqfError, match="%s: img_features must be a tensor or the pair" % who):
            call((img, cnt, 3), idx)
        with pytest.raises(vqa.VqfError, match=r"%s: PackedRegions.offsets must have shape \(6,\)" % who):
            call(good)
        with pytest.raises(vqa.VqfError, match="%s: PackedRegions.max_regions must be a Python int" % who):
            call(vqa.PackedRegions(good.rows, good.offsets, 1025), idx)
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            call(good, idx)
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            call((img, cnt), idx)

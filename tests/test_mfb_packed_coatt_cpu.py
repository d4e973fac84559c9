"""MFB / MHBCoAtt packed_coatt (the co-attention head on the packed rows), the part that needs no GPU: the address arithmetic of the
packed-rows kernels restated in Python against mfb_packed_ref.clamped_spans (every address any offsets can produce lies inside its
tensor), the derived layout, the refusal together with img_index (raised in front of every other check), the new entry points in the
header, the binding table and the built library, and the error codes they return before any launch.
"""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import mfb_packed_ref as PR
from cases import MFB_CASES, MHBCOATT_CASES, make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


# ---- the address arithmetic ----------------------------------------------------------------------------------------------------------
def _span(off, s, L, R):
    """vqf_packed_span (csrc/common.h), as the kernels compute it"""
    a, b = off[s], off[s + 1]
    st = min(max(a, 0), R - 1)
    return st, min(max(b - a, 1), min(L, R - st))


def _addresses(off, N, L, R, O, G):
    """Every element index the packed-rows kernels form, per tensor: {name: (extent, [indices])}.  Restated from csrc/fusion.hip
    (PROWS), csrc/reduce.hip (*_packed) and csrc/attention.hip (LPK); LS walks do not change which rows a sample touches."""
    acc = {k: [] for k in ("Y", "rowssq", "rowinv", "logits", "keep_row")}
    for n in range(N):
        st, cnt = _span(off, n, L, R)
        for l in range(cnt):
            acc["Y"] += [(st + l) * O, (st + l) * O + O - 1]                         # R / Y / dY rows, first and last element
            acc["rowssq"] += [4 * (st + l) + w for w in range(4)]                    # fusion forward stores, group norm loads
            acc["rowinv"].append(st + l)
            acc["logits"] += [(st + l) * G + g for g in range(G)]                    # pooling loads / dlogits stores
            acc["keep_row"].append(n * L + l)                                        # keep / Philox stay padded
        # the reducers' flat walks: i < 4 cnt from 4 start; i < cnt G from start G
        assert 4 * st + 4 * cnt - 1 == acc["rowssq"][-1] and st * G + cnt * G - 1 == acc["logits"][-1]
    ext = dict(Y=R * O, rowssq=4 * R, rowinv=R, logits=R * G, keep_row=N * L)
    return {k: (ext[k], v) for k, v in acc.items()}


OFFSETS = [
    ("valid", [0, 1, 21, 40, 47, 51], 5, 20),
    ("count_0_and_above_L", [0, 0, 22, 41, 48, 52], 5, 20),                      # test_packed_fuse_clamps_what_the_offsets_hold's anomalies
    ("count_0", [0, 0, 1], 2, 1),
    ("count_above_L", [0, 3, 4], 2, 1),
    ("negative_and_beyond_R", [-7, 3, 900, 2, 2], 4, 20),
    ("decreasing", [40, 30, 20, 10, 0], 4, 196),
    ("all_at_the_end", [51, 51, 51, 60], 3, 20),
]


@pytest.mark.parametrize("name,off,N,L", OFFSETS, ids=[o[0] for o in OFFSETS])
def test_every_packed_rows_address_lies_inside_its_tensor(name, off, N, L):
    R = max(1, off[-1]) if name in ("valid", "count_0_and_above_L", "count_0", "count_above_L") else 52
    spans = PR.clamped_spans(torch.tensor(off), R, L)
    assert spans == [_span(off, s, L, R) for s in range(N)]                       # the restatement is the reference's rule
    assert all(0 <= st and 1 <= cn <= L and st + cn <= R for st, cn in spans)
    for O, G in ((1000, 2), (8, 1)):
        for k, (extent, idx) in _addresses(off, N, L, R, O, G).items():
            assert idx and min(idx) >= 0 and max(idx) < extent, (k, min(idx), max(idx), extent)
    if name == "valid":                                                            # ... and on valid offsets every row has one owner
        rows = sorted(r for st, cn in spans for r in range(st, st + cn))
        assert rows == list(range(R))


# ---- the layout -----------------------------------------------------------------------------------------------------------------------
def test_packed_rows_is_a_derived_layout(vqa):
    gr = importlib.import_module(vqa.__name__ + ".host.grouping")
    off = torch.tensor([0, 4, 11, 12])
    packed = gr.RegionLayout(3, 3, 7, offsets=off, R=12)
    assert packed.packed and not packed.rows
    rows = packed.packed_rows()
    assert rows.rows and rows.packed and not (rows.grouped or rows.counted or rows.plain)
    assert (rows.N, rows.U, rows.L, rows.R) == (3, 3, 7, 12) and rows.roff is packed.roff and rows.offsets is packed.offsets
    assert rows.packed_rows() is rows and not packed.rows                          # the source is untouched
    assert rows.padded().counted and not rows.padded().rows
    # only a packed layout without shared images has the form
    for lay in (gr.RegionLayout(3, 3, 7), gr.RegionLayout(3, 3, 7, img_length=torch.tensor([4, 7, 1])),
                gr.RegionLayout(5, 3, 7, img_index=torch.tensor([0, 2, 0, 1, 2]), offsets=off, R=12)):
        assert lay.packed_rows() is lay and not lay.rows
    meta = gr.RegionLayout(3, 3, 7, offsets=torch.empty(4, dtype=torch.int64, device="meta"), R=12).packed_rows()
    assert meta.rows and meta.roff.device.type == "meta"                           # nothing read on the host


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def _features(counts, D, seed=3):
    rng = np.random.RandomState(seed)
    return [rng.randn(k, D) for k in counts]


@pytest.mark.parametrize("mhb", [False, True], ids=["mfb", "mhbcoatt"])
def test_packed_coatt_is_an_attribute_and_refuses_img_index(vqa, mhb):
    case = MHBCOATT_CASES[1] if mhb else MFB_CASES[2]
    cfg = make_cfg(case)
    cls = vqa.MHBCoAtt if mhb else vqa.MFB
    model = cls(cfg)
    assert model.packed_coatt is False
    keys = list(model.state_dict().keys())
    model.packed_coatt = True
    assert list(model.state_dict().keys()) == keys                                # same parameters, same state_dict
    D = cfg.img_feature_channel
    good = vqa.pack_region_features(_features((3, 10, 1, 7), D))
    q7 = torch.ones(7, case["T"], dtype=torch.long)
    idx = torch.tensor([2, 0, 0, 3, 0, 2, 1])
    with pytest.raises(vqa.VqfError, match="packed_coatt.*img_index") as e:        # in front of every other check: no GPU needed
        model(good, q7, img_index=idx)
    assert ("MHBCoAtt" if mhb else "MFB") in str(e.value)
    # without img_index, and with it on the other call forms, the attribute refuses nothing: the next check speaks
    q4 = torch.ones(4, case["T"], dtype=torch.long)
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(good, q4)
    img, lens = vqa.pad_region_features(_features((3, 10, 1, 7), D))
    for form in (img, (img, lens)):
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            model(form, q7, img_index=idx)
    # bf16 is still refused for any PackedRegions, with the existing message
    model.gemm_dtype = "bf16"
    with pytest.raises(vqa.VqfError, match="PackedRegions is fp32 only.*bf16"):
        model(good, q4)
    model.gemm_dtype, model.packed_coatt = "fp32", False
    with pytest.raises(vqa.VqfError, match="GPU tensors"):                        # the default form takes img_index as before
        model(good, q7, img_index=idx)


def test_the_attribute_is_documented(vqa):
    assert "packed_coatt" in vqa.MFB.forward.__doc__ and "packed_coatt" in vqa.MHBCoAtt.forward.__doc__
    assert "img_index" in vqa.MFB.forward.__doc__.split("packed_coatt", 1)[1]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ["vqf_mfb_fuse_fwd_packed_rows", "vqf_mfb_fuse_bwd_packed_rows", "vqf_l2_group_norm_packed", "vqf_l2_norm_bwd_coef_packed",
       "vqf_l2_norm_bwd_coef_lin_packed", "vqf_glimpse_pool_fwd_packed_rows", "vqf_glimpse_pool_bwd_packed_rows"]


def test_header_binding_table_and_library_agree_on_the_packed_rows_forms_within_abi_7(vqa):
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name in NEW:
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(vqa.lib.SIGNATURES[name][1]) == len(decl.split(",")), name
    # the rows forms take the arguments of their *_packed siblings
    for a, b in (("vqf_mfb_fuse_fwd_packed_rows", "vqf_mfb_fuse_fwd_packed"), ("vqf_mfb_fuse_bwd_packed_rows", "vqf_mfb_fuse_bwd_packed"),
                 ("vqf_glimpse_pool_fwd_packed_rows", "vqf_glimpse_pool_fwd_packed"),
                 ("vqf_glimpse_pool_bwd_packed_rows", "vqf_glimpse_pool_bwd_packed")):
        assert vqa.lib.SIGNATURES[a] == vqa.lib.SIGNATURES[b], a
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7
    for name in NEW:
        assert hasattr(vqa.ops, name[4:]), name                                   # and each has its wrapper


def test_packed_rows_argument_checks_need_no_gpu(vqa):
    lib = vqa.lib.load()
    fake = 4096                                   # never dereferenced: every call below is refused first
    BADARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    fwd = lib.vqf_mfb_fuse_fwd_packed_rows
    assert fwd(fake, None, fake, None, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None) == BADARG                 # null roff
    assert fwd(fake, None, fake, fake + 2, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None) == BADARG             # misaligned roff
    assert fwd(fake, None, fake, fake, None, 0, 0.0, 2, 0, 3, 8, fake, fake, None) == BADARG                 # R = 0
    assert fwd(fake, None, fake, fake, None, 0, 0.0, 2, 5, 3, 10, fake, fake, None) == UNSUPPORTED           # O % 4
    assert fwd(fake, None, fake, fake, None, 0, 0.0, 2, 5, 2000, 8, fake, fake, None) == UNSUPPORTED         # L > 1024
    assert fwd(fake, None, fake, fake, None, 0, 0.0, 2, 5, 3, 8, None, fake, None) == BADARG                 # no output
    bwd = lib.vqf_mfb_fuse_bwd_packed_rows
    head = (fake, fake, fake, fake, fake, fake, None, fake)
    assert bwd(*head, None, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    assert bwd(*head, fake + 2, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    assert bwd(*head, fake, None, 0, 0.0, 2, -1, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    assert bwd(*head, fake, None, 0, 0.0, 2, 5, 3, 10, fake, fake, None, fake, 1 << 30, None) == UNSUPPORTED
    need = lib.vqf_mfb_fuse_bwd_ws_bytes(2, 3, 8)
    assert need > 0
    assert bwd(*head, fake, None, 0, 0.0, 2, 5, 3, 8, fake, fake, fake, fake, need - 4, None) == WORKSPACE   # short (dbiasP wanted)
    assert bwd(*head, fake, None, 0, 0.0, 2, 5, 3, 8, fake, fake, fake, None, need, None) == WORKSPACE
    gn = lib.vqf_l2_group_norm_packed
    assert gn(fake, None, 2, 5, 3, fake, fake, fake, None) == BADARG
    assert gn(fake, fake + 2, 2, 5, 3, fake, fake, fake, None) == BADARG
    assert gn(fake, fake, 2, 0, 3, fake, fake, fake, None) == BADARG
    assert gn(fake, fake, 0, 5, 3, fake, fake, fake, None) == BADARG
    assert gn(fake, fake, 2, 5, 3, fake, fake, None, None) == BADARG                                          # rowinv is an output
    co = lib.vqf_l2_norm_bwd_coef_packed
    assert co(fake, None, fake, fake, 2, 5, 3, fake, fake, None) == BADARG
    assert co(fake, fake + 1, fake, fake, 2, 5, 3, fake, fake, None) == BADARG
    assert co(fake, fake, fake, fake, 2, 0, 3, fake, fake, None) == BADARG
    cl = lib.vqf_l2_norm_bwd_coef_lin_packed
    assert cl(fake, fake, 2, None, fake, fake, 2, 5, 3, fake, fake, fake, None) == BADARG
    assert cl(fake, fake, 2, fake + 2, fake, fake, 2, 5, 3, fake, fake, fake, None) == BADARG
    assert cl(fake, fake, 2, fake, fake, fake, 2, 0, 3, fake, fake, fake, None) == BADARG
    assert cl(fake, fake, 0, fake, fake, fake, 2, 5, 3, fake, fake, fake, None) == BADARG
    pf, pb = lib.vqf_glimpse_pool_fwd_packed_rows, lib.vqf_glimpse_pool_bwd_packed_rows
    assert pf(fake, fake, None, None, 2, 2, 5, 3, 8, 2, 0, fake, fake, None) == BADARG
    assert pf(fake, fake, None, fake + 2, 2, 2, 5, 3, 8, 2, 0, fake, fake, None) == BADARG
    assert pf(fake, fake, None, fake, 2, 2, 0, 3, 8, 2, 0, fake, fake, None) == BADARG
    assert pf(fake, fake, fake, fake, 2, 2, 5, 3, 8, 2, 0, fake, fake, None) == BADARG                        # idx given
    assert pf(fake, fake, None, fake, 2, 3, 5, 3, 8, 2, 0, fake, fake, None) == BADARG                        # U = N
    assert pf(fake, fake, None, fake, 2, 2, 5, 3, 6, 2, 0, fake, fake, None) == UNSUPPORTED                   # C % 4
    assert pf(fake, fake, None, fake, 2, 2, 5, 2000, 8, 2, 0, fake, fake, None) == UNSUPPORTED                # S > 1024
    assert pb(fake, None, fake, fake, None, None, 2, 2, 5, 3, 8, 2, 0, fake, None) == BADARG
    assert pb(fake, None, fake, fake, fake, fake, 2, 2, 5, 3, 8, 2, 0, fake, None) == BADARG                  # idx given
    assert pb(fake, None, fake, fake, None, fake, 2, 2, 5, 3, 8, 4, 0, fake, None) == UNSUPPORTED             # G
    assert pf(fake, fake, None, fake, 2, 2, 5, 3, 8, 3, 0, fake, fake, None) == UNSUPPORTED                   # G = 3: the ladder's, not here
    assert pb(fake, None, fake, fake, None, fake, 2, 2, 5, 3, 8, 3, 0, fake, None) == UNSUPPORTED

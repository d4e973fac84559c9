"""RegionStager's host half without a GPU: pack_into fills plain numpy buffers to what pack_region_features holds, refuses what it
must, and the class / one-shot form are exported and raise VqfError on a machine without a GPU."""
import numpy as np
import pytest
import torch

import recipe


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    return vqa_amd


def _features(counts, D, salt=3):
    return [recipe.sym_tensor((k, D), 3.0, recipe.name_seed("regions", salt + 10 * u)) for u, k in enumerate(counts)]


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
def test_pack_into_fills_the_buffers_like_pack_region_features(vqa, dtype):
    counts, D = [7, 1, 20, 3], 12
    feats = _features(counts, D)
    rows = np.full((sum(counts) + 5, D), -7.0, dtype=dtype)
    cnt = np.full(6, -1, dtype=np.int32)
    assert vqa.data_loader.pack_into(rows, cnt, feats, 20) == 4
    ref = vqa.pack_region_features([f.astype(dtype).astype(np.float32) for f in feats])
    R = sum(counts)
    assert rows.dtype == dtype and np.array_equal(rows[:R].astype(np.float32), ref.rows.numpy())
    assert np.array_equal(rows[R:], np.full((5, D), -7.0, dtype=dtype))            # nothing behind the last row is touched
    off = np.concatenate([[0], np.cumsum(cnt[:4])])
    assert np.array_equal(off, ref.offsets.numpy()) and cnt[4] == -1 and cnt[5] == -1
    if dtype is np.float16:                                                           # the cast is numpy's round to nearest even
        assert not np.array_equal(rows[:R].astype(np.float32), np.concatenate(feats, 0))
    # exactly full buffers are taken
    rows2, cnt2 = np.zeros((R, D), dtype=dtype), np.zeros(4, dtype=np.int32)
    assert vqa.data_loader.pack_into(rows2, cnt2, feats) == 4 and np.array_equal(rows2, rows[:R]) and cnt2.tolist() == counts


def test_pack_into_refusals_write_nothing(vqa):
    D = 8
    rows, cnt = np.full((30, D), 5.0, dtype=np.float32), np.full(3, 9, dtype=np.int32)
    good = _features([4, 2], D)
    bad = {"empty list": [],
           "K_i = 0": [good[0], np.zeros((0, D), np.float32)],
           "not 2-D": [good[0], np.zeros(D, np.float32)],
           "mixed D": [good[0], np.zeros((2, D + 4), np.float32)],
           "another D than the buffer": _features([4, 2], D + 4),
           "K_i above max_regions": _features([4, 11], D),
           "sum beyond the buffer": _features([10, 10, 10], D) + _features([1], D),
           "more images than counts": _features([1, 1, 1, 1], D)}
    for name, feats in bad.items():
        with pytest.raises(ValueError):
            vqa.data_loader.pack_into(rows, cnt, feats, 10)
        assert (rows == 5.0).all() and (cnt == 9).all(), name
    assert vqa.data_loader.pack_into(rows, cnt, _features([10, 10, 10], D), 10) == 3          # exactly at every limit


def test_stager_needs_a_gpu(vqa, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(vqa.VqfError, match="GPU"):
        vqa.RegionStager(4, channels=8, max_regions=5)
    with pytest.raises(vqa.VqfError, match="GPU"):
        vqa.stage_regions(_features([2, 3], 8))


def test_exports_and_argument_checks(vqa):
    assert vqa.RegionStager is vqa.data_loader.RegionStager and vqa.stage_regions is vqa.data_loader.stage_regions
    assert vqa.pack_into is vqa.data_loader.pack_into
    for kw in (dict(storage="bf16"), dict(form="grid"), dict(depth=0), dict(max_regions=0), dict(max_regions=1025)):
        with pytest.raises(ValueError):
            vqa.RegionStager(4, channels=8, **kw)
    ops = vqa.ops
    assert ops.region_rows_stage_supported(1, 1, 1, 4) and ops.region_rows_stage_supported(65535, (1 << 29) - 1, 1024, 65536)
    for U, R, L, D in ((0, 1, 1, 4), (65536, 1, 1, 4), (1, 0, 1, 4), (1, 1 << 29, 1, 4), (1, 1, 0, 4), (1, 1, 1025, 4), (1, 1, 1, 6),
                       (1, 1, 1, 0), (1, 1, 1, 65540)):
        assert not ops.region_rows_stage_supported(U, R, L, D)


def test_entry_point_is_bound_and_named(vqa):
    vqa.build()
    lib = vqa.lib.load()
    assert len(vqa.lib.SIGNATURES["vqf_region_rows_stage"][1]) == 9
    names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
    assert "region_rows_stage" in names
    # the argument checks run before any launch: they need no GPU
    f = lib.vqf_region_rows_stage
    a = 1 << 20                                             # a 16-byte aligned address that is never dereferenced
    assert f(None, 0, None, 1, 1, 1, 4, a, None) == -1 and f(a, 0, None, 1, 1, 1, 4, None, None) == -1
    assert f(a, 0, a + 2, 1, 1, 1, 4, a, None) == -1 and f(a, 0, None, 0, 1, 1, 4, a, None) == -1
    assert f(a, 0, None, 1, 1, 1, 0, a, None) == -1
    assert f(a, 0, None, 1, 1, 1, 6, a, None) == -3 and f(a, 0, None, 1, 1, 1025, 4, a, None) == -3
    assert f(a, 0, None, 65536, 1, 1, 4, a, None) == -3 and f(a, 0, None, 1, 1 << 29, 1, 4, a, None) == -3
    assert f(a, 0, None, 1, 1, 1, 65540, a, None) == -3
    assert f(a, 0, None, 1, 1, 1, 4, a + 8, None) == -2 and f(a + 8, 0, None, 1, 1, 1, 4, a, None) == -2
    assert f(a + 4, 1, None, 1, 1, 1, 4, a, None) == -2

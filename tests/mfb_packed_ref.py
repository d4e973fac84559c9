"""TEST INFRASTRUCTURE ONLY: the packed layout of region features (forward(PackedRegions(rows, offsets, max_regions), ...)), in torch.

rows holds every owner's real rows, one owner after the other; owner i has rows offsets[i] .. offsets[i + 1] - 1.  The model's
result on a PackedRegions is, by definition, its result on the zero-padded batch with the counts offsets[1:] - offsets[:-1]
(tests/mfb_regions_ref.py), so the only thing restated here is the change of layout -- independently of PackedRegions.unpack
and data_loader.pack_region_features, which tests/test_mfb_packed_cpu.py pins against these helpers.
"""
import torch


def offsets_of(counts):
    """counts (N,) -> offsets (N + 1,) int64 on the counts' device: 0, c0, c0 + c1, ..."""
    counts = torch.as_tensor(counts).to(torch.int64)
    off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    off[1:] = torch.cumsum(counts, 0)
    return off


def pack_rows(padded, counts):
    """padded (N, L, ...) and counts (N,) in [1, L] -> rows (sum counts, ...): the first counts[i] rows of every owner, in order"""
    counts = [int(c) for c in torch.as_tensor(counts).tolist()]
    assert len(counts) == padded.shape[0] and all(1 <= c <= padded.shape[1] for c in counts)
    return torch.cat([padded[i, :c] for i, c in enumerate(counts)], 0).contiguous()


def unpack_rows(rows, offsets, L, fill=0.0):
    """rows (R, ...) and offsets (N + 1,) -> (padded (N, L, ...) with `fill` beyond each count, counts (N,) int64)"""
    off = [int(o) for o in torch.as_tensor(offsets).tolist()]
    N = len(off) - 1
    assert off[0] == 0 and off[-1] == rows.shape[0] and all(1 <= off[i + 1] - off[i] <= L for i in range(N))
    out = torch.full((N, L) + tuple(rows.shape[1:]), fill, dtype=rows.dtype, device=rows.device)
    for i in range(N):
        out[i, :off[i + 1] - off[i]] = rows[off[i]:off[i + 1]]
    return out, torch.tensor([off[i + 1] - off[i] for i in range(N)], dtype=torch.int64)


def clamped_spans(offsets, R, L):
    """What the packed kernels make of ANY offsets (include/vqa_fusion.h "Packed region features"): per owner (start, cnt) with
    start = clamp(off[s], 0, R - 1) and cnt = clamp(off[s + 1] - off[s], 1, min(L, R - start))."""
    off = [int(o) for o in torch.as_tensor(offsets).tolist()]
    spans = []
    for s in range(len(off) - 1):
        start = min(max(off[s], 0), R - 1)
        spans.append((start, min(max(off[s + 1] - off[s], 1), min(L, R - start))))
    return spans

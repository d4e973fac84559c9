"""Refusals of the region-aware entry points (csrc/fusion.hip, attention.hip, hie_ladder_alt.hip, hie.hip), and their PRECEDENCE.

Table-driven: for every entry point one valid-looking call (aligned fake addresses, never dereferenced: every call made here is
refused before a launch), broken in one way at a time and in pairs of those ways.  A pair pins which of two refusals speaks first.
The expected codes (tests/golden/region_entry_refusals.json, read by `recorded`: case name -> integer code, nothing else) were recorded
from the build in front of the host-side VqfRegions refactor, on a machine without a GPU; a broken call that build ACCEPTED (it went
on to a launch) is not in the file, and is never made here.  The parameter names and types come from include/vqa_fusion.h, so a fault is named by
the parameter it breaks:  `idx=0` null, `idx+2` / `P+4` misaligned by so many bytes, `N=0`, `U=3`, `idx=set` (a pointer the valid call
leaves NULL), `ws_bytes-4`, `p_drop=1`;  `A&B` is the pair, B applied after A (it only matters where both break one parameter).
"""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "region_entry_refusals.json")
FAKE = 1 << 20                      # 16-byte aligned, never dereferenced
REFUSALS = (-1, -2, -3, -4)         # VQF_E_BADARG, _ALIGN, _UNSUPPORTED, _WORKSPACE

# ---- the valid-looking calls: values by parameter name, per family; None = a pointer the call leaves NULL ------------------------
FUSE = dict(N=2, U=2, R=5, L=3, O=8, ldrb=8, p_drop=0.0, seed=0, keep=None, cascade=None, dcascade=None, dzdrop=None, zdrop=None)
POOL = dict(N=2, U=2, R=5, S=3, C=8, G=2, unit_softmax=0, dwts_extra=None)
GUIDED = dict(N=2, U=2, R=5, S=3, E=32, G=2, ldx=64, lddx=64)
HIE = dict(N=2, L=3, E=32, T=4, lda=32, ldv=32, ldo=32, ldp=32, ldz=32, ldpa=32, ldcp=32, ldh=32, ldw=36, p_drop=0.0, seed=0, keep=None)
AFF = dict(N=2, L=3, E=32, T=4, G=2, epi=2, ldx1=64, ldy1=64, ldx2=64, ldy2=64, ldx_level1=32, ldy_level1=32, ldx_level2=32,
           ldy_level2=32, p_drop=0.0, seed=0, keep=None)
# entry point -> (base values, {parameter: value} of this entry point alone, pairs?)   pairs: every entry point that takes an index,
# count or offset array; the forms without one share the launch functions and are held by their single faults
ENTRIES = {}
for _n in ("fwd_grouped", "bwd_grouped", "fwd_len", "bwd_len", "fwd_grouped_len", "bwd_grouped_len", "fwd_packed", "bwd_packed",
           "fwd_packed_rows", "bwd_packed_rows", "fwd_grouped_packed", "bwd_grouped_packed"):
    ENTRIES["vqf_mfb_fuse_" + _n] = (FUSE, {}, True)
for _n in ("fwd", "fwd_pbf16", "fwd_pbf16_rb", "bwd", "bwd_pbf16", "bwd_bf16dp"):
    ENTRIES["vqf_mfb_fuse_" + _n] = (FUSE, {}, False)
for _n in ("fwd_len", "bwd_len", "fwd_grouped", "bwd_grouped", "fwd_grouped_len", "bwd_grouped_len", "fwd_packed", "bwd_packed",
           "bwd_packed_dfeat"):
    ENTRIES["vqf_glimpse_pool_" + _n] = (POOL, {}, True)
for _n in ("fwd_packed_rows", "bwd_packed_rows"):
    ENTRIES["vqf_glimpse_pool_" + _n] = (POOL, {"idx": None}, True)
for _n in ("fwd", "bwd", "fwd_bf16", "bwd_bf16"):
    ENTRIES["vqf_glimpse_pool_" + _n] = (POOL, {}, False)
ENTRIES["vqf_row_block_gather"] = (dict(N=2, U=2, blk=8), {}, True)
ENTRIES["vqf_row_block_group_sum"] = (dict(N=2, U=2, blk=8), {}, True)
for _n in ("fwd_grouped", "bwd_grouped", "fwd_packed", "bwd_packed"):
    ENTRIES["vqf_guided_logits_" + _n] = (GUIDED, {}, True)
for _n in ("fwd", "bwd"):
    ENTRIES["vqf_guided_logits_" + _n] = (GUIDED, {}, False)
for _n in ("hv_fwd_regions", "rank_add_regions", "rank_left_regions"):
    ENTRIES["vqf_hie_" + _n] = (HIE, {}, True)
for _n in ("hv_fwd", "head_bwd", "rank_add", "rank_left"):
    ENTRIES["vqf_hie_" + _n] = (HIE, {}, False)
ENTRIES["vqf_zero_cols_len"] = (dict(rows=8, rows_per_sample=4, N=2, L=3), {}, True)
for _n in ("affinity_len", "affinity_regions", "affinity_levels_len", "affinity_levels_regions"):
    ENTRIES["vqf_hie_" + _n] = (AFF, {}, True)
for _n in ("affinity", "affinity_levels"):
    ENTRIES["vqf_hie_" + _n] = (AFF, {}, False)

# the unsupported shapes, by parameter (where an entry point has it)
SHAPES = dict(U=3, O=10, S=2000, G=4, E=40, C=6, T=17, blk=6, epi=3)
WS_QUERY = {"vqf_mfb_fuse": ("vqf_mfb_fuse_bwd_grouped_ws_bytes", "NULO", "vqf_mfb_fuse_bwd_ws_bytes", "NLO"),
            "vqf_guided_logits": ("vqf_guided_logits_bwd_grouped_ws_bytes", "NUSEG", "vqf_guided_logits_bwd_ws_bytes", "NSEG")}


def declarations():
    """{entry point: [(type, name), ...]} from include/vqa_fusion.h"""
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(?:int|size_t)\s+(vqf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = [re.match(r"\s*(.*?)\s*(\w+)\s*$", a, flags=re.S).groups() for a in args.split(",")]
    return out


def _kind(ctype, name):
    if "*" in ctype:
        if name == "stream":
            return "stream"
        return "index" if ("int*" in ctype.replace(" ", "") or name == "keep") else "data"      # keep: the 4-byte mask words
    return "float" if ctype == "float" else "size"


def cases(lib, entry, params):
    """[(case name, argument tuple)] for one entry point: the single faults, then (where ENTRIES asks) the pairs"""
    base_by_name, own, pairs = ENTRIES[entry]
    base, faults = {}, []
    for ctype, name in params:
        kind = _kind(ctype, name)
        if kind == "stream":
            base[name] = None
        elif kind in ("index", "data"):
            base[name] = None if {**base_by_name, **own}.get(name, FAKE) is None else FAKE      # (fuse_fwd's output is named R too)
        elif name != "ws_bytes":
            base[name] = base_by_name[name]
    if "ws_bytes" in [n for _, n in params]:
        family = [f for f in WS_QUERY if entry.startswith(f)][0]
        grouped, gargs, plain, pargs = WS_QUERY[family]
        if entry.endswith("_packed") and family == "vqf_guided_logits":
            fn, names = "vqf_guided_logits_bwd_packed_ws_bytes", "NUSEG"
        else:
            fn, names = (grouped, gargs) if "grp_off" in base else (plain, pargs)
        base["ws_bytes"] = getattr(lib, fn)(*[base[c] for c in names])
        assert base["ws_bytes"] > 0
    for ctype, name in params:
        kind = _kind(ctype, name)
        if kind in ("index", "data"):
            off = 2 if kind == "index" else 4
            if base[name] is None:
                faults += [(name + "=set", {name: FAKE}), ("%s+%d" % (name, off), {name: FAKE + off})]
            else:
                faults += [(name + "=0", {name: None}), ("%s+%d" % (name, off), {name: FAKE + off})]
        elif name == "ws_bytes":
            faults.append(("ws_bytes-4", {name: base[name] - 4}))
        elif name == "p_drop":
            faults.append(("p_drop=1", {name: 1.0}))
        elif kind == "size" and name != "seed":
            faults.append((name + "=0", {name: 0}))
            if name in SHAPES or (name == "L" and "O" in base):
                faults.append(("%s=%d" % (name, SHAPES.get(name, 2000)), {name: SHAPES.get(name, 2000)}))
    order = [n for _, n in params]
    out, seen = [], {tuple(base[n] for n in order)}

    def add(label, changed):
        args = tuple({**base, **changed}[n] for n in order)
        if args not in seen:
            seen.add(args)
            out.append((label, args))
    for label, ch in faults:
        add(label, ch)
    if pairs:
        for la, a in faults:
            for lb, b in faults:
                if la != lb:
                    add(la + "&" + lb, {**a, **b})
    return out


@pytest.fixture(scope="module")
def lib():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd.lib.load()


def recorded(rec):
    """{case name: code} of one entry point's record.  `single`[i] is faults[i] alone and `pairs`[i][j] is faults[i]&faults[j]: the
    digit d is the code -d, '.' a call that is not in the table (accepted, or the same arguments as an earlier case)"""
    f = rec["faults"]
    out = {f[i]: -int(c) for i, c in enumerate(rec["single"]) if c != "."}
    out.update({f[i] + "&" + f[j]: -int(c) for i, row in enumerate(rec["pairs"]) for j, c in enumerate(row) if c != "."})
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {entry: recorded(rec) for entry, rec in json.load(f).items()}


def test_the_table_covers_every_entry_point_that_takes_an_index_array(golden):
    decl = declarations()
    src = {f: open(os.path.join(ROOT, "vqa-attention-networks_amd", "csrc", f + ".hip")).read()
           for f in ("fusion", "attention", "hie_ladder_alt", "hie")}
    for name, params in decl.items():
        if any(re.search(r"\b%s\s*\(" % name, s) for s in src.values()) and any("int*" in t.replace(" ", "") for t, _ in params):
            assert name in ENTRIES and ENTRIES[name][2], name
    assert sorted(golden) == sorted(ENTRIES)
    for entry, want in golden.items():
        assert want and all(type(c) is int and c in REFUSALS for c in want.values()), entry
        assert any("&" in k for k in want) == ENTRIES[entry][2], entry


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_refusal_and_its_precedence_is_what_it_was(lib, golden, entry):
    table = dict(cases(lib, entry, declarations()[entry]))
    want = golden[entry]
    assert set(want) <= set(table), sorted(set(want) - set(table))[:5]
    fn = getattr(lib, entry)
    wrong = {k: (fn(*table[k]), c) for k, c in want.items()}       # only calls the recorded build refused: none reaches a launch
    wrong = {k: v for k, v in wrong.items() if v[0] != v[1]}
    assert not wrong, (len(wrong), sorted(wrong.items())[:12])

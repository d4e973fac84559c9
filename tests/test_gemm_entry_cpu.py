"""The GEMM entry points' answers that need no device (csrc/gemm_f32*.hip, gemm_bf16*.hip): routing queries and refusals.

Table-driven, like test_region_entry_refusals_cpu.py.  The expected values (tests/golden/gemm_entry.json) were recorded from the
build in front of the host-side GEMM launch refactor (csrc/gemm_host.h), on a machine without a GPU.  Only what does not depend on
the CU count is here, so the file holds on a machine with a GPU as well:
  * vqf_gemm_f32_ws_bytes / vqf_gemm_bf16_ws_bytes (big_applies and pick_splits of the large-tile kernels) over a grid of
    (ta, tb, M, N, K) -- the project's shapes and the neighbours of every routing threshold -- under the options that change them;
  * vqf_lstm_step_supported over B and H;
  * vqf_gemm_f32_big_rows where big_applies decides (the result is M) or whole_round_rows refuses before it asks for the CU count
    (ta, K < 256, N < 128, a ragged last column tile, an operand that is no multiple of 4) -- a mid-size shape gives 0 without a device and its
    whole-rounds block with one, and is left out;
  * the refusals of vqf_gemm_f32, _rowscale, _batched, vqf_gemm_bf16, _rowscale, vqf_gemm_f32_sample and vqf_lstm_step_fwd: one
    valid-looking call (aligned fake addresses, never dereferenced), broken in one way at a time and in pairs of those ways; a pair
    pins which of two refusals speaks first.  EVERY call made here is refused before a launch: a fault is a change of the arguments
    that the entry point refuses whatever the device, and the valid call itself is never made.
"""
import itertools
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_entry.json")
FAKE = 1 << 20                      # 16-byte aligned, never dereferenced
REFUSALS = (-1, -2, -3, -4)         # VQF_E_BADARG, _ALIGN, _UNSUPPORTED, _WORKSPACE
ACCUM, OUT_BF16 = 2, 4

# ---- the queries ---------------------------------------------------------------------------------------------------------------
# (M, N, K), each under all four (ta, tb)
SHAPES = [
    (100352, 5000, 2048), (5000, 2048, 100352), (1024, 1024, 100352), (4096, 1024, 7168), (512, 5000, 2048), (1024, 512, 50176),
    (50176, 512, 512), (50176, 1024, 1024),                                  # mid-size (HieCoAtten)
    (8192, 8192, 1536), (8192, 8192, 1532), (7936, 8448, 1536), (7936, 8448, 1532), (8192, 8192, 1024),      # 1024 / 1023 tiles, K 1536 / 1532
    (5000, 2048, 16384), (5000, 2048, 16380), (4096, 1024, 4096), (4096, 1024, 4092),                        # K 16384 / 16380, 4096 / 4092
    (4096, 1916, 7168), (4096, 1912, 7168), (4096, 300, 7168),                                               # the 107 % ragged-column rule
    (2048, 2048, 2048), (1792, 2304, 2048), (2048, 2048, 50176), (1792, 2304, 50176), (2048, 1792, 50176),   # 64 / 63 / 56 tiles (bf16)
    (4098, 1024, 7168), (4100, 1024, 7168), (4096, 1026, 7168), (4096, 1028, 7168),                          # M, N no multiples of 4 / 8
    (256, 128, 64), (255, 128, 64), (256, 127, 64), (256, 128, 60), (256, 128, 255), (64, 64, 64),           # the smallest the kernels take
]
GRID = [(ta, tb) + s for s in SHAPES for ta in (0, 1) for tb in (0, 1)]
WS_OPTIONS = ["", "gemm_f32_big=0", "gemm_f32_big=2", "gemm_bf16_big=0"]
ROWS_OPTIONS = ["", "gemm_f32_big=0", "gemm_f32_big=2", "gemm_f32_rounds=0"]
LSTM_OPTIONS = ["", "gemm_f32_wave=0", "gemm_f32_wave=1"]
LSTM_BH = [(B, H) for B in (0, 64, 128, 130, 256, 512) for H in (0, 128, 256, 264, 272, 512, 1024)]


def rows_is_device_free(ta, tb, M, N, K, value):
    """a vqf_gemm_f32_big_rows answer that cannot depend on the CU count (the module docstring)"""
    ragged = ((N + 255) // 256) * 256 * 100 > N * 107
    return value == M or ta or K < 256 or N < 128 or ragged or K % 4 != 0 or (tb and N % 4 != 0)


class with_option:
    """'name=value' (or '') set for the block, and put back"""

    def __init__(self, spec):
        self.spec = spec

    def __enter__(self):
        from vqa_amd import ops
        if self.spec:
            name, value = self.spec.split("=")
            self.name, self.prev = name, ops.set_option(name, int(value))

    def __exit__(self, *exc):
        from vqa_amd import ops
        if self.spec:
            ops.set_option(self.name, self.prev)
        return False


def queries(lib):
    """{query: {option: [values]}} of the library in front of us; big_rows holds None where the answer needs a device"""
    out = {"f32_ws_bytes": {}, "bf16_ws_bytes": {}, "big_rows": {}, "lstm_step_supported": {}}
    for o in WS_OPTIONS:
        with with_option(o):
            out["f32_ws_bytes"][o] = [int(lib.vqf_gemm_f32_ws_bytes(*g)) for g in GRID]
            out["bf16_ws_bytes"][o] = [int(lib.vqf_gemm_bf16_ws_bytes(*g)) for g in GRID]
    for o in ROWS_OPTIONS:
        with with_option(o):
            vals = [int(lib.vqf_gemm_f32_big_rows(*g)) for g in GRID]
            free = o in ("gemm_f32_big=0", "gemm_f32_rounds=0")      # whole_round_rows answers 0 before anything else
            out["big_rows"][o] = [v if free or rows_is_device_free(*g, v) else None for g, v in zip(GRID, vals)]
    for o in LSTM_OPTIONS:
        with with_option(o):
            out["lstm_step_supported"][o] = [int(lib.vqf_lstm_step_supported(B, H)) for B, H in LSTM_BH]
    return out


# ---- the refusals --------------------------------------------------------------------------------------------------------------
# entry point -> (the valid-looking call by parameter name (pointers not named: FAKE, None: left NULL), [(fault, {parameter: value})])
GEMM = dict(ta=0, tb=0, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, bias=None, flags=0, ws=None, ws_bytes=0, stream=None)
NULLS = [("A=0", {"A": None}), ("B=0", {"B": None}), ("C=0", {"C": None})]
SIZES = [("M=0", {"M": 0}), ("N=0", {"N": 0}), ("K=-1", {"K": -1}), ("lda=0", {"lda": 0}), ("ldb=-8", {"ldb": -8}), ("ldc=56", {"ldc": 56})]
SCALE = [("rowscale=0", {"rowscale": None}), ("rows_per_scale=0", {"rows_per_scale": 0}), ("flags=accum", {"flags": ACCUM}),
         ("flags=accum|relu", {"flags": ACCUM | 1})]
BF16 = [("A+8", {"A": FAKE + 8}), ("B+2", {"B": FAKE + 2}), ("lda=68", {"lda": 68}), ("ldb=76", {"ldb": 76}), ("K=60", {"K": 60}),
        ("ta=1,K=60", {"ta": 1, "K": 60}), ("ta=1,M=60", {"ta": 1, "M": 60}), ("ta=1,M=4", {"ta": 1, "M": 4}),
        ("tb=1,N=60", {"tb": 1, "N": 60}), ("flags=out_bf16", {"flags": OUT_BF16})]
SAMPLE = dict(tb=0, NS=128, L=196, N=512, K=512, lda=512, ldb=512, ldc=512, bias=None, flags=0, stream=None)
LSTM = dict(B=128, H=256, stream=None)
ENTRIES = {
    "vqf_gemm_f32": (GEMM, NULLS + SIZES),
    "vqf_gemm_f32_rowscale": (dict(GEMM, rows_per_scale=4), NULLS + SIZES + SCALE),
    "vqf_gemm_f32_batched": (dict(GEMM, batch=2, strideA=4096, strideB=4096, strideC=4096),
                             NULLS + SIZES + [("batch=0", {"batch": 0}), ("batch=65536", {"batch": 65536})]),
    "vqf_gemm_bf16": (GEMM, NULLS + SIZES + BF16),
    "vqf_gemm_bf16_rowscale": (dict(GEMM, rows_per_scale=4), NULLS + SIZES + BF16 + SCALE),
    "vqf_gemm_f32_sample": (SAMPLE, NULLS + [
        ("lda=508", {"lda": 508}), ("ldb=508", {"ldb": 508}), ("ldc=508", {"ldc": 508}), ("tb=1,ldb=508", {"tb": 1, "ldb": 508}),
        ("NS=0", {"NS": 0}), ("L=100", {"L": 100}), ("L=198", {"L": 198}), ("L=204", {"L": 204}), ("N=300", {"N": 300, "ldc": 512}),
        ("K=48", {"K": 48}), ("K=500", {"K": 500}), ("flags=accum", {"flags": ACCUM}), ("A+4", {"A": FAKE + 4}), ("B+8", {"B": FAKE + 8}),
        ("C+4", {"C": FAKE + 4}), ("lda=514", {"lda": 514}), ("ldb=518", {"ldb": 518}), ("ldc=513", {"ldc": 513})]),
    "vqf_lstm_step_fwd": (LSTM, [
        ("h_prev=0", {"h_prev": None}), ("w_hh=0", {"w_hh": None}), ("gates=0", {"gates": None}), ("c_out=0", {"c_out": None}),
        ("h_out=0", {"h_out": None}), ("B=0", {"B": 0}), ("H=-16", {"H": -16}), ("B=100", {"B": 100}), ("H=128", {"H": 128}),
        ("H=264", {"H": 264}), ("h_prev+4", {"h_prev": FAKE + 4}), ("w_hh+8", {"w_hh": FAKE + 8}), ("gates+4", {"gates": FAKE + 4}),
        ("c_prev+4", {"c_prev": FAKE + 4}), ("c_out+12", {"c_out": FAKE + 12}), ("h_out+4", {"h_out": FAKE + 4})]),
}


def declarations():
    """{entry point: [parameter name, ...]} from include/vqa_fusion.h"""
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: [re.match(r".*?(\w+)\s*$", a, flags=re.S).group(1) for a in args.split(",")]
            for name, args in re.findall(r"\b(?:int|size_t)\s+(vqf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def cases(entry, order):
    """[(case name, argument tuple)]: the single faults, then every pair that breaks two different sets of parameters"""
    base, faults = ENTRIES[entry]
    base = {n: base.get(n, FAKE) for n in order}
    out = [(label, tuple({**base, **ch}[n] for n in order)) for label, ch in faults]
    for (la, a), (lb, b) in itertools.combinations(faults, 2):
        if not set(a) & set(b):
            out.append((la + "&" + lb, tuple({**base, **a, **b}[n] for n in order)))
    assert all(args != tuple(base[n] for n in order) for _, args in out)
    return out


@pytest.fixture(scope="module")
def lib():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd.lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("query", ["f32_ws_bytes", "bf16_ws_bytes", "big_rows", "lstm_step_supported"])
def test_every_routing_query_answers_what_it_did(lib, golden, query):
    from vqa_amd import ops
    touched = sorted({o.split("=")[0] for o in WS_OPTIONS + ROWS_OPTIONS + LSTM_OPTIONS if o})
    before = [ops.get_option(n) for n in touched]
    got, want = queries(lib)[query], golden["queries"][query]
    assert [ops.get_option(n) for n in touched] == before
    assert sorted(got) == sorted(want)
    table = LSTM_BH if query == "lstm_step_supported" else GRID
    for o in want:
        assert len(want[o]) == len(table)
        wrong = [(o, g, a, b) for g, a, b in zip(table, got[o], want[o]) if b is not None and a != b]
        assert not wrong, (len(wrong), wrong[:8])
    if query != "lstm_step_supported":      # the table does decide something: both answers occur under the default options
        assert any(v for v in want[""]) and any(v == 0 for v in want[""])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_refusal_and_its_precedence_is_what_it_was(lib, golden, entry):
    table = dict(cases(entry, declarations()[entry]))
    want = golden["refusals"][entry]
    assert sorted(want) == sorted(table)       # every case of the table was refused by the recorded build, none is accepted
    assert all(type(c) is int and c in REFUSALS for c in want.values())
    fn = getattr(lib, entry)
    wrong = {k: (fn(*table[k]), c) for k, c in want.items()}
    wrong = {k: v for k, v in wrong.items() if v[0] != v[1]}
    assert not wrong, (len(wrong), sorted(wrong.items())[:12])


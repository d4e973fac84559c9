"""host/ops.py: the table of the MFB fusion's 30 launch entry points and the two marshallers, without a GPU.

The marshallers are pure: a key and the operands in, (entry name, positional arguments) out.  Here every operand is a string that
names itself, so the argument tuple can be read against the parameter names of the entry's prototype in include/vqa_fusion.h (the
header's text is the reference: host/lib.py's ctypes table holds types only, and is written by hand as well).
"""
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH = re.compile(r"vqf_mfb_fuse_(fwd|bwd)(?!.*(_ws_bytes|_supported)$)")
# the header's parameter names that differ from the marshallers' operand names
ALIAS = {"P_bf16": "P", "dP_bf16": "dP", "lens": "lens0", "lens_q": "lens0", "lens_u": "lens1"}
SCALARS = ("N", "U", "R", "L", "O", "ldrb", "rb_rows", "dP_rows")


@pytest.fixture(scope="module")
def ops():
    import vqa_amd
    return vqa_amd.ops


@pytest.fixture(scope="module")
def signatures():
    import vqa_amd
    return vqa_amd.lib.SIGNATURES


@pytest.fixture(scope="module")
def prototypes():
    """{entry point: [(type, name), ...]} from include/vqa_fusion.h"""
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(?:int|size_t)\s+(vqf_mfb_fuse_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = [re.match(r"\s*(.*?)\s*(\w+)\s*$", a, flags=re.S).groups() for a in args.split(",")]
    return out


def marshal(ops, key):
    """the key's marshaller on operands that name themselves -> (entry, args)"""
    fwd = "P pbias q keep seed p_drop N L O Rout rowssq stream".split()
    bwd = "dY Y inv coefA coefB P pbias q keep seed p_drop N L O dP dq dbiasP ws ws_bytes stream".split()
    if key[0] == "fwd":
        return ops._fuse_fwd_args(key, *fwd, cascade="cascade", zdrop="zdrop", idx="idx", lens=("lens0", "lens1")[:_n_lens(key)],
                                  roff="roff", U="U", R="R", R_bf16="R_bf16", ldrb="ldrb", rb_rows="rb_rows")
    return ops._fuse_bwd_args(key, *bwd, dzdrop="dzdrop", cascade="cascade", dcascade="dcascade", idx="idx", order="order",
                              grp_off="grp_off", lens=("lens0", "lens1")[:_n_lens(key)], roff="roff", U="U", R="R", dP_rows="dP_rows")


def _n_lens(key):
    return (2 if key[1] else 1) if key[2] == "len" else 0


def every_key():
    return list(itertools.product(("fwd", "bwd"), (False, True), ("plain", "len", "packed", "rows"),
                                  ("f32", "pbf16", "bf16dp", "pbf16_f32dp"), (False, True)))


def test_the_table_holds_exactly_the_librarys_launch_entries(ops, signatures, prototypes):
    names = list(ops._FUSE_ENTRIES.values())
    want = sorted(n for n in signatures if LAUNCH.match(n))
    assert len(want) == 30 and sorted(n for n in prototypes if LAUNCH.match(n)) == want
    assert sorted(names) == want                                         # none twice, none missing
    assert sum(k[0] == "fwd" for k in ops._FUSE_ENTRIES) == 15 and all(n.startswith("vqf_mfb_fuse_" + k[0])
                                                                     for k, n in ops._FUSE_ENTRIES.items())


def test_every_name_is_written_once_in_ops(ops):
    """outside docstrings and comments: the table is the only place that spells an entry's name"""
    import ast
    src = open(ops.__file__).read()
    strings = [n.value for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
    attrs = [n.attr for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Attribute)]
    for name in ops._FUSE_ENTRIES.values():
        assert strings.count(name) == 1 and attrs.count(name) == 0, name


def test_every_key_marshals_to_its_entrys_prototype(ops, signatures, prototypes):
    for key, name in ops._FUSE_ENTRIES.items():
        entry, args = marshal(ops, key)
        assert entry == name
        assert len(args) == len(signatures[name][1]) == len(prototypes[name]), name
        for a, (ctype, pname) in zip(args, prototypes[name]):
            if pname == "R" and "*" in ctype:                            # the plain and counted forwards call their output R
                pname = "Rout"
            assert a == ALIAS.get(pname, pname), (name, args)
        ints = [pname for ctype, pname in prototypes[name] if ctype == "int"]
        assert [a for a in args if a in SCALARS] == ints, name            # each scalar where the header names it, and no other


def test_a_key_outside_the_table_is_refused(ops):
    import vqa_amd
    outside = [k for k in every_key() if k not in ops._FUSE_ENTRIES]
    assert len(outside) == len(every_key()) - 30
    for key in outside:
        with pytest.raises(vqa_amd.VqfError):
            marshal(ops, key)
    rules = {("fwd", True, "packed", "pbf16", False): "un-grouped",       # grouped with bf16
             ("bwd", True, "len", "bf16dp", False): "un-grouped",
             ("fwd", False, "len", "f32", True): "r_bf16 needs a bf16 P",   # r_bf16 with an fp32 P
             ("bwd", False, "packed", "pbf16_f32dp", False): "a bf16 P comes with a bf16 dP",
             ("fwd", True, "rows", "f32", False): "un-grouped"}           # packed rows with idx
    for key, why in rules.items():
        with pytest.raises(vqa_amd.VqfError, match=why):
            ops._fuse_entry(key, "mfb_fuse_x")

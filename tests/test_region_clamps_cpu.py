"""The memory-safety clamps of the region forms (csrc/common.h: vqf_packed_span, vqf_region_owner, vqf_region_count,
vqf_group_range, vqf_group_member) against their statement in Python: tools/region_clamp_check.cpp, built here without the
sanitizers, prints one table line per case of its exhaustive walk (and checks the guarantees and vqf_drop itself)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def clamp(v, lo, hi):
    return max(lo, min(v, hi))


def span(Rtot, S, a, b):
    row0 = clamp(a, 0, Rtot - 1)
    return row0, clamp(b - a, 1, min(S, Rtot - row0))


# kind -> rule(inputs as the program printed them) -> expected outputs; the last `nout` numbers of a line are the outputs
RULES = {
    "span": (2, lambda Rtot, S, a, b: span(Rtot, S, a, b)),                       # roff[u], roff[u + 1] = a, b
    "owner": (1, lambda U, n, *idx: (clamp(idx[n], 0, U - 1),)),                  # the whole idx array is on the line
    "count": (1, lambda S, n, *lens: (clamp(lens[n], 1, S),)),
    "range": (2, lambda N, a, b: (clamp(a, 0, N), clamp(b, clamp(a, 0, N), N))),
    "member": (1, lambda N, je, j, *order: (clamp(order[min(j, je - 1)], 0, N - 1),)),     # the whole order array (je entries)
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build tools/region_clamp_check.cpp with")
    exe = str(tmp_path_factory.mktemp("clamps") / "region_clamp_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "region_clamp_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines()


def test_program_passes_its_own_checks(table):
    assert table[-1].startswith("OK: ") and table[-1].endswith(" 0 failures")
    assert not [ln for ln in table if ln.startswith("FAILED")]


def test_every_table_line_is_the_python_rule(table):
    seen = dict.fromkeys(RULES, 0)
    for ln in table[:-1]:
        kind, *nums = ln.split()
        nout, rule = RULES[kind]
        nums = [int(x) for x in nums]
        if kind == "member":
            assert len(nums) == 3 + nums[1] + 1, ln
        assert tuple(nums[-nout:]) == tuple(rule(*nums[:-nout])), ln
        seen[kind] += 1
    # the walk is the exhaustive one: Rtot 1..5 x S 1..4 x (a, b) in [-3, Rtot + 3]^2 spans, and so on
    assert seen["span"] == sum(4 * (r + 7) ** 2 for r in range(1, 6))
    assert seen["owner"] == seen["count"] == 4 * 3 * 12
    assert seen["range"] == sum((n + 7) ** 2 for n in range(1, 5))
    assert seen["member"] == sum((je + 3) * (n + 7) for n in range(1, 5) for je in range(1, n + 1))

#!/usr/bin/env python3
"""The device-code record of csrc/*.hip that a refactor is read against (profiles/*_codeobj.txt); needs no GPU.

    python tools/codeobj_record.py [--csrc DIR] [--work DIR] [file.hip ...] > listing.txt

Each file (default: every .hip of the csrc directory) is compiled with the Makefile's flags plus --offload-device-only
--no-gpu-bundle-output (a gfx950 ELF).  Per kernel, sorted by name: symbol size (llvm-readelf -s), .vgpr_count / .sgpr_count /
.group_segment_fixed_size / .private_segment_fixed_size (llvm-readelf --notes) and the first 12 hex digits of the sha256 of the
kernel's own bytes; a kernel is written as its name and template arguments, the parameter list left off.  Per file, last, the
sha256 and size of its .text section (llvm-objcopy -O binary --only-section=.text).  Run it on two checkouts (--csrc) and diff."""
import argparse
import hashlib
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")


def run(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, check=True, **kw).stdout


def makefile_flags(csrc):
    txt = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", txt, re.M).group(1)
    return re.search(r"^CXXFLAGS\s*:=\s*(.*)$", txt, re.M).group(1).replace("$(ARCH)", arch).split()


def short_names(mangled):
    # c++filt does not know DF16b (__bf16): demangle it as `half` (Dh; neither is a substitution candidate) and rename
    out = run(["c++filt"], input="\n".join(m.replace("DF16b", "Dh") for m in mangled)).split("\n")
    names = {}
    for m, d in zip(mangled, out):
        d = re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "").replace("half", "__bf16"))
        depth = 0
        for i, ch in enumerate(d):
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                d = d[:i]
                break
        names[m] = d.replace(", ", ",")
    return names


def record(csrc, work, flags, f):
    elf = os.path.join(work, f + ".elf")
    run([os.path.join(ROCM, "bin", "hipcc")] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c", f, "-o", elf], cwd=csrc)
    size, addr = {}, {}
    for ln in run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", elf]).splitlines():
        p = ln.split()
        if len(p) >= 8 and p[3] == "FUNC":
            size[p[7]], addr[p[7]] = int(p[2]), int(p[1], 16)
    kern = {}
    for rec in re.split(r"\n\s+- \.agpr_count", run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf]))[1:]:
        get = lambda key: re.search(r"\n\s+\.%s:\s+'?([^\s']+)'?" % key, rec).group(1)
        kern[get("name")] = tuple(int(get(k)) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size",
                                                        "private_segment_fixed_size"))
    text0 = int(re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+)", run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", elf])).group(1), 16)
    raw = os.path.join(work, f + ".text")
    run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", elf, raw])
    text = open(raw, "rb").read()
    names = short_names(sorted(kern))
    lines = []
    for m in sorted(kern, key=lambda m: names[m]):
        code = text[addr[m] - text0:addr[m] - text0 + size[m]]
        lines.append("%s %s size=%d vgpr=%d sgpr=%d lds=%d scratch=%d code=%s"
                     % ((f, names[m], size[m]) + kern[m] + (hashlib.sha256(code).hexdigest()[:12],)))
    lines.append("%s .text sha256=%s bytes=%d" % (f, hashlib.sha256(text).hexdigest(), len(text)))
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(HERE), "vqa-attention-networks_amd", "csrc"))
    ap.add_argument("--work", default=None, help="directory for the ELFs (default: a temporary one)")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    files = a.files or sorted(f for f in os.listdir(a.csrc) if f.endswith(".hip"))
    flags = makefile_flags(a.csrc)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as ex:
        work = a.work or tmp
        os.makedirs(work, exist_ok=True)
        for lines in ex.map(lambda f: record(a.csrc, work, flags, f), files):
            print("\n".join(lines))

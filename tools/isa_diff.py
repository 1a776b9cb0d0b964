#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel for kernel.

For a change that only moves kernels between translation units: every kernel unit of both
trees (the Makefile's lists in doorman_amd/csrc: the kernel units and the runtime's host units) is compiled to device assembly with the
product's flags, the output is cut per function symbol, compiler-numbered local labels
are renumbered per function (so a function's index in its unit does not matter), and
the instruction text, the .amdhsa_* descriptor, the resource symbols and comment block
(registers, scratch, LDS, occupancy) and the code-object metadata entry are compared as
text.  No GPU is needed.

    tools/isa_diff.py PARENT_TREE NEW_TREE [--out profiles/split_isa.md] [--jobs 16]

Exit status 0: the same symbols with identical text on both sides.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def units(tree):
    """The tree's kernel units: what its Makefile lists, or every .hip file (a tree from before the list);
    then the runtime's host units: the Makefile's list, or dm_runtime.cpp alone (a tree from before that list)."""
    d = os.path.join(tree, "doorman_amd", "csrc")

    def listed(target):
        r = subprocess.run(["make", "-s", "--no-print-directory", target], cwd=d, capture_output=True, text=True)
        return r.stdout.split() if r.returncode == 0 else None

    fs = listed("print-units") or sorted(f for f in os.listdir(d) if f.endswith(".hip"))
    return d, fs + (listed("print-host-units") or ["dm_runtime.cpp"])


def compile_unit(d, f, out):
    cmd = [HIPCC] + FLAGS + (["-x", "hip"] if f.endswith(".cpp") else []) + ["-o", out, f]
    subprocess.run(cmd, cwd=d, check=True, stderr=subprocess.DEVNULL)
    return out


def strip(line):
    line = line.split(";", 1)[0].rstrip()
    s = line.strip()
    if not s or s.startswith((".file", ".loc", ".ident")):
        return None
    return s


def renumber(lines):
    """Compiler-numbered local labels -> numbers by first appearance within the function."""
    seen = {}

    def sub(m):
        key = (m.group(1), m.group(2))
        if key not in seen:
            seen[key] = sum(1 for k in seen if k[0] == m.group(1))
        return ".L%s#%d%s" % (m.group(1), seen[key], m.group(3) or "")

    return [LABEL.sub(sub, l) for l in lines]


def parse(path):
    """{symbol: {"text", "descriptor", "resources", "metadata"}} of one unit's assembly."""
    raw = open(path).read().split("\n")
    funcs, meta = {}, {}
    i = 0
    while i < len(raw):
        m = re.match(r"\s*\.type\s+(\S+),@function", raw[i])
        if m:
            sym = m.group(1)
            text, desc, res = [], [], []
            i += 1
            in_desc = False
            while i < len(raw) and not re.match(r"\s*\.size\s+%s," % re.escape(sym), raw[i]):
                s = strip(raw[i])
                if s is not None:
                    if s.startswith(".amdhsa_kernel "):
                        in_desc = True
                    (desc if in_desc else text).append(s)
                    if s == ".end_amdhsa_kernel":
                        in_desc = False
                i += 1
            i += 1
            # the function's resource symbols and the compiler's summary (a comment block)
            while i < len(raw) and not re.match(r"\s*\.(text|type|protected|globl|weak|amdgpu_metadata)\b", raw[i]) \
                    and not re.match(r"\s*\.section\s+\.text", raw[i]):
                s = raw[i].strip()
                if s.startswith(".set " + sym + ".") or re.match(
                        r"; (TotalNumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|LDSByteSize|Occupancy|codeLenInByte)",
                        s):
                    res.append(s)
                i += 1
            funcs[sym] = {"text": renumber(text), "descriptor": desc, "resources": res, "kernel": bool(desc)}
            continue
        if raw[i].strip() == "amdhsa.kernels:":
            i += 1
            entry = None
            while i < len(raw) and (raw[i].startswith("  ") or not raw[i].strip()):
                if raw[i].startswith("  - "):
                    entry = []
                    meta[len(meta)] = entry
                if entry is not None:
                    entry.append(raw[i].rstrip())
                i += 1
            continue
        i += 1
    for entry in meta.values():
        name = next(l.split(":", 1)[1].strip() for l in entry if l.strip().startswith(".name:"))
        funcs[name]["metadata"] = entry
    return funcs


def build(tree, tmp, jobs):
    d, fs = units(tree)
    os.makedirs(tmp)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        outs = list(ex.map(lambda f: compile_unit(d, f, os.path.join(tmp, f + ".s")), fs))
    allf, per_unit = {}, {}
    for f, o in zip(fs, outs):
        fn = parse(o)
        per_unit[f] = sum(1 for v in fn.values() if v["kernel"])
        for sym, v in fn.items():
            if sym in allf and allf[sym] != v:
                raise SystemExit("%s: %s is emitted twice, differently" % (tree, sym))
            allf[sym] = v
    return allf, per_unit


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        pf, pu = build(a.parent, os.path.join(tmp, "parent"), a.jobs)
        nf, nu = build(a.new, os.path.join(tmp, "new"), a.jobs)
    lines = ["# Device code, parent against new: kernel for kernel", "",
             "Every kernel unit compiled with `hipcc " + " ".join(FLAGS) + "`",
             "(the runtime's `.cpp` units with `-x hip`), cut per function symbol, comments and `.file`/`.loc`/`.ident`",
             "dropped, local labels renumbered per function (`tools/isa_diff.py PARENT NEW`).", "",
             "| tree | unit | kernels |", "|---|---|---|"]
    for name, u in (("parent", pu), ("new", nu)):
        lines += ["| %s | `%s` | %d |" % (name, f, n) for f, n in u.items()]
        lines.append("| %s | **all** | **%d** |" % (name, sum(u.values())))
    diffs = []
    for sym in sorted(set(pf) | set(nf)):
        if sym not in nf:
            diffs.append("`%s`: only in the parent" % sym)
        elif sym not in pf:
            diffs.append("`%s`: only in the new tree" % sym)
        else:
            parts = [k for k in ("text", "descriptor", "resources", "metadata") if pf[sym].get(k) != nf[sym].get(k)]
            if parts:
                diffs.append("`%s`: differs in %s" % (sym, ", ".join(parts)))
    nk = sum(1 for v in pf.values() if v["kernel"])
    lines += ["", "Function symbols: %d in the parent (%d kernels, %d device functions out of line), %d in the new tree."
              % (len(pf), nk, len(pf) - nk, len(nf)),
              "Instructions compared: %d lines." % sum(len(v["text"]) for v in pf.values()), ""]
    if diffs:
        lines += ["Differences:", ""] + ["- " + d for d in diffs]
    else:
        lines.append("Every symbol is on both sides with identical instruction text, `.amdhsa_*` descriptor, "
                     "resource figures (VGPRs, SGPRs, AGPRs, scratch, LDS, occupancy, code length) and metadata entry.")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())

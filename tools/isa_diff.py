#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel for kernel.

For a change that only moves kernels between translation units: every kernel unit of both
trees (the Makefile's lists in doorman_amd/csrc: the kernel units and the runtime's host units) is compiled to device assembly with the
product's flags, the output is cut per function symbol, compiler-numbered local labels
are renumbered per function (so a function's index in its unit does not matter), and
the instruction text, the .amdhsa_* descriptor, the resource symbols and comment block
(registers, scratch, LDS, occupancy) and the code-object metadata entry are compared as
text.  No GPU is needed.

    tools/isa_diff.py PARENT_TREE NEW_TREE [--out profiles/split_isa.md] [--jobs 16] [--map FILE]

For a change that also renames kernels (several kernels restated as builds of one template),
--map FILE pairs a parent symbol with its successor.  Each line of the file is

    OLD-SYMBOL-REGEX NEW-SYMBOL-REGEX [text]

both matched against whole mangled names; the second may use the first's groups (\1 ...), and
must match exactly one symbol of the new tree.  Both names are replaced by a placeholder in
text, descriptor, resource symbols and metadata before the comparison.  One allowance is made
for a pair: the successor may take more kernel arguments, appended to the parent's.  Then the
kernel-argument segment grows by some delta, and only what follows from that may differ: the
segment's size in the descriptor and the metadata, the metadata's entries for the appended
arguments, the offsets of the hidden arguments behind them (each moved by delta), and in the
text an immediate that is such an offset (the same instruction with the immediate moved by
delta, at or beyond the parent's explicit arguments).  Every line so allowed is counted in
the report.  `text` marks a pair (or, with the same name on both sides, a kernel) whose
instruction text may differ: its VGPRs, AGPRs, scratch and LDS may not grow nor its occupancy
fall, and the report lists its figures and line counts on both sides.

Exit status 0: the same symbols (up to the map) with identical text on both sides (up to the
allowance), and no `text` kernel worse off.
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


PH = "@SYM"
IMM = re.compile(r"\b(0x[0-9a-fA-F]+|\d+)\b")


def figure(v, name):
    """One of the compiler's summary figures (its comment block after the function)."""
    for l in v["resources"]:
        m = re.match(r"; %s: (\d+)" % name, l)
        if m:
            return int(m.group(1))
    return None


def meta_split(entry):
    """A metadata entry -> (its lines outside .args and the segment size, [argument blocks], segment size)."""
    rest, args, size, cur, in_args = [], [], None, None, False
    for l in entry:
        t = l.strip()
        if t == ".args:":
            in_args = True
        elif in_args and l.startswith("      "):
            if t.startswith("- "):
                cur = []
                args.append(cur)
            cur.append(t[2:] if t.startswith("- ") else t)
        else:
            in_args = False
            m = re.match(r"\.kernarg_segment_size:\s*(\d+)", t)
            if m:
                size = int(m.group(1))
            else:
                rest.append(l)
    return rest, args, size


def arg_offset(block):
    return next(int(l.split(":")[1]) for l in block if l.startswith(".offset:"))


def shifted(block, delta):
    return [".offset:         %d" % (arg_offset(block) + delta) if l.startswith(".offset:") else l for l in block]


def is_hidden(block):
    return any(l.startswith(".value_kind:") and "hidden_" in l for l in block)


def compare_pair(pv, nv, psym, nsym):
    """(parts that differ beyond the allowance, lines the allowance covered) for a parent symbol and its successor."""
    def named(v, k, sym):
        return [l.replace(sym, PH) for l in v.get(k) or []]

    bad, allowed = [], 0
    delta, explicit_end = 0, 0
    pm, nm = named(pv, "metadata", psym), named(nv, "metadata", nsym)
    if pm or nm:
        prest, pargs, psize = meta_split(pm)
        nrest, nargs, nsize = meta_split(nm)
        delta = (nsize or 0) - (psize or 0)
        pe = [a for a in pargs if not is_hidden(a)]
        ph = [a for a in pargs if is_hidden(a)]
        ne = [a for a in nargs if not is_hidden(a)]
        nh = [a for a in nargs if is_hidden(a)]
        explicit_end = max([arg_offset(a) for a in pe] + [0])
        if delta == 0:
            if pm != nm:
                bad.append("metadata")
        elif delta < 0 or prest != nrest or ne[:len(pe)] != pe or [shifted(a, delta) for a in ph] != nh:
            bad.append("metadata")
        else:
            allowed += 1 + len(ne) - len(pe) + len(ph)
    pd, nd = named(pv, "descriptor", psym), named(nv, "descriptor", nsym)
    for a, b in zip(pd, nd):
        if a != b:
            if delta and a.startswith(".amdhsa_kernarg_size") and b.startswith(".amdhsa_kernarg_size"):
                allowed += 1
            elif "descriptor" not in bad:
                bad.append("descriptor")
    if len(pd) != len(nd):
        bad.append("descriptor")
    if named(pv, "resources", psym) != named(nv, "resources", nsym):
        bad.append("resources")
    pt, nt = named(pv, "text", psym), named(nv, "text", nsym)
    if len(pt) != len(nt):
        bad.append("text")
    else:
        for a, b in zip(pt, nt):
            if a == b:
                continue
            ok = False
            if delta:  # one immediate, moved by delta, at or beyond the parent's explicit arguments
                for m in IMM.finditer(b):
                    v = int(m.group(1), 0) - delta
                    if v > explicit_end:
                        for fmt in ("0x%x", "%d"):
                            ok = ok or b[:m.start()] + fmt % v + b[m.end():] == a
            if ok:
                allowed += 1
            elif "text" not in bad:
                bad.append("text")
    return bad, allowed


def read_map(path):
    rules = []
    for l in open(path):
        f = l.split("#", 1)[0].split()
        if f:
            rules.append((re.compile(f[0]), f[1], len(f) > 2 and f[2] == "text"))
    return rules


def pair_up(pf, nf, rules):
    """{parent symbol: (new symbol, text may differ)} for the symbols the map speaks of."""
    pairs = {}
    for sym in sorted(pf):
        for old, new, loose in rules:
            m = old.fullmatch(sym)
            if not m:
                continue
            want = re.compile(re.sub(r"\\(\d)", lambda g: re.escape(m.group(int(g.group(1)))), new))
            hits = [s for s in nf if want.fullmatch(s)]
            if len(hits) != 1:
                raise SystemExit("map: %s has %d successors by %s" % (sym, len(hits), new))
            pairs[sym] = (hits[0], loose)
            break
    return pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--map", help="pairs of renamed symbols (the module's docstring has the format)")
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
    pairs = pair_up(pf, nf, read_map(a.map)) if a.map else {}
    succ = {n for n, _ in pairs.values()}
    diffs, loose_rows, renamed, allowed = [], [], 0, 0
    for sym in sorted(set(pf) | set(nf)):
        if sym in pairs:
            new, loose = pairs[sym]
            bad, n_ok = compare_pair(pf[sym], nf[new], sym, new)
            renamed += sym != new
            allowed += n_ok
            if loose:
                fig = [(k, figure(pf[sym], k), figure(nf[new], k))
                       for k in ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")]
                worse = [k for k, x, y in fig if x is not None and (y < x if k == "Occupancy" else y > x)]
                loose_rows.append("| `%s` | `%s` | %s | %d / %d | %s |" % (
                    sym, new if new != sym else "=", " | ".join("%s / %s" % (x, y) for _, x, y in fig),
                    len(pf[sym]["text"]), len(nf[new]["text"]), "same" if "text" not in bad else "differs"))
                if worse:
                    diffs.append("`%s` -> `%s`: worse in %s" % (sym, new, ", ".join(worse)))
            elif bad:
                diffs.append("`%s` -> `%s`: differs in %s" % (sym, new, ", ".join(bad)))
        elif sym in succ and sym not in pf:
            continue
        elif sym not in nf:
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
    if a.map:
        lines += ["With `--map %s`: %d parent symbols are compared with a successor of another name, both names"
                  % (a.map, renamed),
                  "replaced by `%s`; %d lines differ only by what the allowance covers (a longer kernel-argument"
                  % (PH, allowed),
                  "segment: its size, the appended arguments' metadata, the hidden arguments' offsets).", ""]
    if loose_rows:
        lines += ["Kernels whose text may differ (the map's `text` mark), parent / new:", "",
                  "| parent | new | VGPRs | AGPRs | scratch | LDS | occupancy | lines | text |", "|---|---|---|---|---|---|---|---|---|"]
        lines += loose_rows + [""]
    if diffs:
        lines += ["Differences:", ""] + ["- " + d for d in diffs]
    else:
        lines.append("Every %ssymbol is on both sides with identical instruction text, `.amdhsa_*` descriptor, "
                     "resource figures (VGPRs, SGPRs, AGPRs, scratch, LDS, occupancy, code length) and metadata entry%s."
                     % ("other " if loose_rows else "", ", up to the allowance" if a.map else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())

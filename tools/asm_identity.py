#!/usr/bin/env python3
"""usage: tools/asm_identity.py <a.s> <b.s> [--rename FILE]

Is the device code of build b that of build a?  Both files are engine.hip compiled device-only to assembly with the flags of
ctucopy_amd/build.py plus `--offload-device-only -S`.  Every function of b (kernels and what was not inlined) is compared with a's
function of the same symbol, one to one:
  * the instruction text from the symbol's label to its end, with the function index taken out of the local labels (.LBB<n>_,
    .Lfunc_end<n>, and the loop comments that repeat them) and the .Ltmp<n> labels numbered by first
    appearance, runs of blanks as one, and the function's own symbol replaced by <self>;
  * the descriptor - the .amdhsa_* lines, the .set <symbol>.* resource lines, and the kernel's entry in the metadata (register counts,
    spill counts, LDS, scratch, kernarg layout).
--rename FILE: lines of `<symbol in a> <symbol in b>` for kernels whose template arguments changed.
Functions only in a are listed (the caller says why nothing reaches them); functions only in b, and every difference, fail the run.
The tool diffs; it looks for no particular instruction.  Exit status 0: every function of b is a's."""
import difflib
import re
import shutil
import subprocess
import sys

FUNC_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
LBB = re.compile(r"(?:\.L|\b)BB\d+_")  # .LBB<n>_<m> labels, and BB<n>_<m> in the comments that name a loop's header
LFUNC = re.compile(r"\.Lfunc_(begin|end)\d+")
LTMP = re.compile(r"\.Ltmp\d+")
META_KEEP = (".agpr_count", ".group_segment_fixed_size", ".kernarg_segment_align", ".kernarg_segment_size", ".max_flat_workgroup_size",
             ".private_segment_fixed_size", ".sgpr_count", ".sgpr_spill_count", ".uses_dynamic_stack", ".vgpr_count", ".vgpr_spill_count",
             ".wavefront_size", ".offset", ".size", ".value_kind", ".address_space", ".actual_access")


def parse(path):
    """{symbol: (text lines, descriptor lines)}"""
    lines = open(path, errors="replace").read().split("\n")
    funcs, meta = {}, {}
    i, n = 0, len(lines)
    while i < n:
        m = FUNC_TYPE.match(lines[i])
        if not m:
            if lines[i].startswith("amdhsa.kernels:"):
                meta = parse_meta(lines, i + 1)
                break
            i += 1
            continue
        sym = m.group(1)
        text, desc = [], []
        i += 1
        in_desc = False
        while i < n and not LFUNC.match(lines[i].strip().rstrip(":")):
            s = lines[i].strip()
            if s.startswith(".amdhsa_kernel"):
                in_desc = True
            elif s.startswith(".end_amdhsa_kernel"):
                in_desc = False
            elif in_desc:
                desc.append(s)
            elif s and not s.startswith(".section") and not s.startswith(".p2align"):
                text.append(s)
            i += 1
        # the resource lines behind the function's end, up to the next function
        while i < n and not lines[i].lstrip().startswith(".globl") and not FUNC_TYPE.match(lines[i]) and not lines[i].lstrip().startswith(".amdgpu_metadata"):
            s = lines[i].strip()
            if s.startswith(".set " + sym + "."):
                desc.append(s)
            i += 1
        tmp = {}

        def ltmp(mm):
            return tmp.setdefault(mm.group(0), ".Ltmp#%d" % len(tmp))

        norm = lambda s: LTMP.sub(ltmp, LFUNC.sub(r".Lfunc_\1", LBB.sub("BB_", re.sub(r"\s+", " ", s)))).replace(sym, "<self>")
        funcs[sym] = ([norm(s) for s in text], [norm(s) for s in desc])
    for sym, rows in meta.items():
        if sym in funcs:
            funcs[sym][1].extend(r.replace(sym, "<self>") for r in rows)
    return funcs


def parse_meta(lines, i):
    """{kernel symbol: the kept lines of its metadata entry}"""
    out, cur, name = {}, [], None
    while i < len(lines) and not lines[i].lstrip().startswith(".end_amdgpu_metadata"):
        ln = lines[i]
        if ln.startswith("  - ") or not ln.startswith("  "):  # the next kernel's entry, or the end of the list
            if name:
                out[name] = cur
            cur, name = [], None
            if not ln.startswith("  - "):
                break
        s = ln.strip().lstrip("- ").strip()
        if s.startswith(".name:"):
            name = s.split(":", 1)[1].strip()
        elif s.split(":")[0] in META_KEEP:
            cur.append("meta " + re.sub(r"\s+", " ", s))
        i += 1
    if name:
        out[name] = cur
    return out


def demangle(syms):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not syms:
        return {s: s for s in syms}
    got = subprocess.run([tool], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    return {s: (got[k] if k < len(got) and got[k] else s) for k, s in enumerate(syms)}


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    rename = {}
    if "--rename" in argv:
        for ln in open(argv[argv.index("--rename") + 1]):
            if ln.strip() and not ln.startswith("#"):
                old, new = ln.split()
                rename[new] = old
    a, b = parse(argv[1]), parse(argv[2])
    kern = lambda f: sum(1 for v in f.values() if any(r.startswith("meta ") for r in v[1]))
    print("a: %s: %d functions, %d kernels, %d instruction lines" % (argv[1], len(a), kern(a), sum(len(v[0]) for v in a.values())))
    print("b: %s: %d functions, %d kernels, %d instruction lines" % (argv[2], len(b), kern(b), sum(len(v[0]) for v in b.values())))
    same, bad, used = 0, [], set()
    for sym, (text, desc) in b.items():
        old = rename.get(sym, sym)
        if old not in a:
            bad.append((sym, "only in b", []))
            continue
        used.add(old)
        diff = []
        for what, x, y in (("text", a[old][0], text), ("descriptor", a[old][1], desc)):
            if x != y:
                diff += ["  " + what + ": " + d for d in list(difflib.unified_diff(x, y, "a", "b", lineterm="", n=1))[:40]]
        if diff:
            bad.append((sym, "differs", diff))
        else:
            same += 1
    names = demangle([s for s, _, _ in bad] + [s for s in a if s not in used] + list(rename) + list(rename.values()))
    for new, old in rename.items():
        print("renamed: %s\n      -> %s" % (names[old], names[new]))
    print("identical (instruction text and descriptor): %d of b's %d functions" % (same, len(b)))
    for sym, why, diff in bad:
        print("%s: %s" % (why.upper(), names[sym]))
        print("\n".join(diff))
    only_a = [s for s in a if s not in used]
    print("only in a: %d" % len(only_a))
    for s in only_a:
        print("  " + names[s])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of one HIP object file, symbol by symbol.

    tools/codeobj_diff.py PARENT.o NEW.o [--arch gfx950]

Unbundles the device code object of each file (llvm-objdump --offloading), disassembles it, cuts the listing at every
`<symbol>:` line, drops the trailing `// address: encoding` column and compares the instruction streams per symbol;
then compares each kernel's metadata from the code object's notes (register counts, segment sizes, kernarg size, maximum
workgroup size).  Prints the symbol counts, the order of the symbols where it differs, and every difference; exit status 0
only when the symbol sets, every stream and every kernel's metadata are identical.  For refactors that move device code
between files without meaning to change it."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
             ".kernarg_segment_align", ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()


def unbundle(obj, arch, work):
    """-> path of the device ELF for `arch` inside the host object `obj`"""
    d = os.path.join(work, os.path.basename(obj) + ".d")
    os.makedirs(d)
    local = os.path.join(d, "obj.o")
    shutil.copy(obj, local)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", "obj.o", cwd=d)
    found = [f for f in glob.glob(os.path.join(d, "*")) if f != local and arch in os.path.basename(f)]
    assert len(found) == 1, "expected one %s code object in %s, found %s" % (arch, obj, found)
    return found[0]


def streams(elf):
    """-> ({symbol: [instruction text]}, [symbols in file order])"""
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", elf)
    out, order, cur = {}, [], None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:\s*$", line)
        if m:
            cur = m.group(1)
            order.append(cur)
            out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        out[cur].append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line).strip())
    return out, order


def metadata(elf):
    """-> {kernel symbol: {key: value}} from the AMDGPU metadata note"""
    text = run(os.path.join(LLVM, "llvm-readelf"), "--notes", elf)
    out, cur = {}, {}
    for line in text.split("\n"):
        m = re.match(r"^\s*(?:- )?(\.[a-z_]+):\s*(.*?)\s*$", line)
        if not m:
            continue
        if re.match(r"^  - \.", line):                      # the first key of the next kernel's record
            if ".symbol" in cur:
                out[cur[".symbol"]] = cur
            cur = {}
        cur[m.group(1)] = m.group(2).strip("'\"")
    if ".symbol" in cur:
        out[cur[".symbol"]] = cur
    return {k[:-3] if k.endswith(".kd") else k: {q: v.get(q) for q in META_KEYS} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="codeobj_diff_")
    try:
        ea, eb = unbundle(args.parent, args.arch, os.path.join(work, "a")), unbundle(args.new, args.arch, os.path.join(work, "b"))
        (sa, oa), (sb, ob) = streams(ea), streams(eb)
        ma, mb = metadata(ea), metadata(eb)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    bad = 0
    print("symbols with code: parent %d, new %d" % (len(sa), len(sb)))
    for s in sorted(set(sa) ^ set(sb)):
        print("  only in %s: %s" % ("parent" if s in sa else "new", s))
        bad += 1
    print("instructions: parent %d, new %d" % (sum(map(len, sa.values())), sum(map(len, sb.values()))))
    print("symbol order in the file: %s" % ("identical" if oa == ob else "differs (%d of %d symbols at another position)" %
                                             (sum(1 for i, s in enumerate(oa) if i >= len(ob) or ob[i] != s), len(oa))))
    differing = 0
    for s in sorted(set(sa) & set(sb)):
        if sa[s] == sb[s]:
            continue
        differing += 1
        lines = [(i, x, y) for i, (x, y) in enumerate(zip(sa[s], sb[s])) if x != y]
        print("  DIFFERS %s: %d / %d instructions, %d lines differ; first:" % (s, len(sa[s]), len(sb[s]), len(lines)))
        for i, x, y in lines[:4]:
            print("    [%d] parent: %s\n    [%d] new:    %s" % (i, x, i, y))
    print("instruction streams compared: %d, differing: %d" % (len(set(sa) & set(sb)), differing))
    print("kernels with metadata: parent %d, new %d" % (len(ma), len(mb)))
    mdiff = 0
    for s in sorted(set(ma) | set(mb)):
        if ma.get(s) != mb.get(s):
            mdiff += 1
            print("  METADATA DIFFERS %s:\n    parent %s\n    new    %s" % (s, ma.get(s), mb.get(s)))
    print("kernel metadata compared (%s): %d, differing: %d" % (", ".join(k.lstrip(".") for k in META_KEYS), len(set(ma) & set(mb)), mdiff))
    bad += differing + mdiff
    print("RESULT: %s" % ("identical device code" if not bad else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of one HIP object file - or of two sets of them - symbol by symbol.

    tools/codeobj_diff.py PARENT.o NEW.o [--arch gfx950]
    tools/codeobj_diff.py --parent PARENT.o [...] --new NEW1.o NEW2.o [...]      (one file split into several, or the reverse)

With several objects on a side their symbols are taken together, and a kernel (a symbol with a kernel descriptor) that
occurs in more than one object of a side is reported: it would exist twice on the device.  An object without device code
(a host-only source) is named and adds nothing, so all of csrc/Makefile's objects can be given.
Unbundles the device code object of each file (llvm-objdump --offloading), disassembles it, cuts the listing at every
`<symbol>:` line, drops the trailing `// address: encoding` column and the padding behind a symbol's last instruction, and compares the instruction streams per symbol;
then compares each kernel's metadata from the code object's notes (register counts, segment sizes, kernarg size, maximum
workgroup size).  Prints the symbol counts, the order of the symbols where it differs, and every difference; exit status 0
only when the symbol sets, every stream and every kernel's metadata are identical and no kernel is defined twice.  For refactors that move device code
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
PADDING = ("s_nop 0", "s_code_end", "...")
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
    assert len(found) <= 1, "expected one %s code object in %s, found %s" % (arch, obj, found)
    return found[0] if found else None      # a host-only source (no kernel) has none


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
    for s in out.values():          # what follows a symbol's last instruction up to the next symbol is padding, not code: its
        while s and s[-1] in PADDING:       # length depends on which symbol comes next, or on being the last of the object
            s.pop()
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


def side(name, objs, arch, work):
    """-> (streams, order, metadata, problems) of the objects of one side taken together"""
    sa, order, ma, bad = {}, [], {}, 0
    for i, obj in enumerate(objs):
        elf = unbundle(obj, arch, os.path.join(work, name, str(i)))
        if elf is None:
            print("  no %s device code in %s: %s" % (arch, name, os.path.basename(obj)))
            continue
        s, o = streams(elf)
        m = metadata(elf)
        for k in sorted(set(m) & set(ma)):
            print("  KERNEL DEFINED TWICE in %s: %s (again in %s)" % (name, k, obj))
            bad += 1
        for k in sorted(set(s) & set(sa)):
            if k not in m and s[k] != sa[k]:
                print("  DIFFERS WITHIN %s: %s (in %s)" % (name, k, obj))
                bad += 1
        sa.update(s)
        ma.update(m)
        order += o
    return sa, order, ma, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("objects", nargs="*", help="PARENT.o NEW.o (the single-object form)")
    ap.add_argument("--parent", nargs="+", default=[])
    ap.add_argument("--new", nargs="+", default=[])
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    if len(args.objects) == 2 and not args.parent and not args.new:
        args.parent, args.new = args.objects[:1], args.objects[1:]
    elif args.objects or not args.parent or not args.new:
        ap.error("give PARENT.o NEW.o, or --parent ... --new ...")
    work = tempfile.mkdtemp(prefix="codeobj_diff_")
    try:
        sa, oa, ma, dup_a = side("parent", args.parent, args.arch, work)
        sb, ob, mb, dup_b = side("new", args.new, args.arch, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    bad = dup_a + dup_b
    print("objects: parent %d, new %d; kernels defined twice: parent %d, new %d" % (len(args.parent), len(args.new), dup_a, dup_b))
    print("symbols with code: parent %d, new %d" % (len(sa), len(sb)))
    for s in sorted(set(sa) ^ set(sb)):
        print("  only in %s: %s" % ("parent" if s in sa else "new", s))
        bad += 1
    print("instructions: parent %d, new %d" % (sum(map(len, sa.values())), sum(map(len, sb.values()))))
    print("symbol order in the file(s): %s" % ("identical" if oa == ob else "differs (%d of %d symbols at another position)" %
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

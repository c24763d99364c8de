#!/usr/bin/env python3
"""Inventory of the kernel instantiations libacimg.so ships, against tests/golden/kernel_inventory.json and the add-on files
tests/golden/kernel_inventory_<feature>.json beside it (same record format; the kernels of later features).

Every __global__ function the library can launch has one host stub (`__device_stub__<name>`), so the stub symbols of
the built library are the list of instantiations.  Only symbol NAMES are read (llvm-nm -C of the ROCm tree, else
nm -C); no device code, no assembly.  A name is normalised to template name plus arguments: `acimg::` qualifiers, the
return type and the parameter list go, e.g.

    void acimg::__device_stub__wgrad_halo_kernel<1, 10>(acimg::WgradHaloParams)   ->   wgrad_halo_kernel<1, 10>

and the same function normalises the `Kernel_Name` column of a `rocprofv3 --kernel-trace` CSV, which is how the
fixture's `tests` lists were filled ("Kernel inventory").

    python tools/kernel_inventory.py                    build, compare with the fixture, exit 1 on a difference
    python tools/kernel_inventory.py --list             build, print the normalised names
    python tools/kernel_inventory.py --update MAP.json  build, rewrite the fixture: one record per instantiation of the
                                                        built library, `tests` / `seen` taken from MAP.json
                                                        ({kernel: {"tests": [...], "seen": "trace"}}) where it has the
                                                        kernel, kept from the old fixture otherwise
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_inventory.json")
STUB = "__device_stub__"


def _top_level_cut(s, ch):
    """index of the first `ch` outside every <...>, or -1"""
    depth = 0
    for i, c in enumerate(s):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == ch and depth == 0:
            return i
    return -1


def normalise(name):
    """demangled kernel or stub name -> `template<arguments>` (see the module docstring)"""
    s = name.strip()
    if s.endswith(".kd"):
        s = s[:-3]
    s = s.replace("(anonymous namespace)::", "").replace(STUB, "").replace("acimg::", "")
    cut = _top_level_cut(s, "(")
    if cut >= 0:
        s = s[:cut]
    s = s.strip()
    while True:                                  # the return type: everything up to the last top-level blank
        cut = _top_level_cut(s, " ")
        if cut < 0:
            break
        s = s[cut + 1:]
    return s.replace("> >", ">>").replace("> >", ">>")


def _nm():
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm"),
                 os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")):
        if os.path.exists(cand):
            return cand
    return shutil.which("llvm-nm") or shutil.which("nm") or "nm"


def library_kernels(lib_path):
    """sorted normalised names of every kernel instantiation with a host stub in lib_path"""
    out = subprocess.run([_nm(), "-C", lib_path], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    names = set()
    for line in out.splitlines():
        if STUB not in line:
            continue
        parts = line.split(None, 2)              # address, type letter, demangled name
        names.add(normalise(parts[-1]))
    return sorted(names)


def addon_paths():
    """tests/golden/kernel_inventory_<feature>.json, sorted: the records of kernels added after the fixture was filled from
    a trace.  A change that adds kernels adds a file of its own beside the fixture and leaves the fixture as it is."""
    return sorted(glob.glob(os.path.join(os.path.dirname(FIXTURE), "kernel_inventory_*.json")))


def load_fixture(path=FIXTURE):
    """the records of `path`; of the fixture itself (the default): followed by those of its add-on files"""
    with open(path) as f:
        records = json.load(f)
    if path == FIXTURE:
        for extra in addon_paths():
            with open(extra) as f:
                records += json.load(f)
    return records


def write_fixture(records, path=FIXTURE):
    records = sorted(records, key=lambda r: r["kernel"])
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in records) + "\n]\n")


def compare(built, records):
    """(new, gone): instantiations the library has and the fixture lacks, and the reverse"""
    have = {r["kernel"] for r in records}
    return sorted(set(built) - have), sorted(have - set(built))


def build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    return entry.build()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--update", metavar="MAP.json")
    args = ap.parse_args(argv)
    built = library_kernels(build())
    if args.list:
        print("\n".join(built))
        return 0
    if args.update:
        with open(args.update) as f:
            found = json.load(f)
        old = {r["kernel"]: r for r in load_fixture()} if os.path.exists(FIXTURE) else {}
        elsewhere = {r["kernel"] for extra in addon_paths() for r in load_fixture(extra)}
        records = []
        for k in built:
            if k in elsewhere:                   # its record lives in an add-on file and stays there
                continue
            rec = dict(old.get(k, {"kernel": k, "tests": [], "seen": "reading"}))
            if k in found:
                rec["tests"], rec["seen"] = sorted(found[k]["tests"]), found[k]["seen"]
            records.append(rec)
        write_fixture(records)
    new, gone = compare(built, load_fixture())
    print("%d kernel instantiations in the library, %d records in the fixture" % (len(built), len(load_fixture())))
    for k in new:
        print("new (no record):", k)
    for k in gone:
        print("gone (record without a kernel):", k)
    return 1 if new or gone else 0


if __name__ == "__main__":
    sys.exit(main())

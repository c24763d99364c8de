"""Every kernel instantiation libacimg.so ships is named in tests/golden/kernel_inventory.json together with the GPU tests that
launch it (tools/kernel_inventory.py; DESIGN.md "Kernel inventory").  Host symbol names only: nothing here looks at device
code, and no GPU module is imported - the named tests are looked up in the syntax tree of their file."""
import ast
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_inventory as inv  # noqa: E402

LIB = os.path.join(ROOT, "acoustic-image-generation_amd", "acimg", "lib", "libacimg.so")


@pytest.fixture(scope="module")
def records():
    return inv.load_fixture()


def test_normalise():
    n = inv.normalise
    assert n("void acimg::__device_stub__wgrad_halo_kernel<1, 10>(acimg::WgradHaloParams)") == "wgrad_halo_kernel<1, 10>"
    assert n("void acimg::igemm_split3_kernel<128, 64, 2, 2, 256, acimg::SplitF16, 3>(acimg::IgemmParams)") == \
        "igemm_split3_kernel<128, 64, 2, 2, 256, SplitF16, 3>"
    assert n("acimg::__device_stub__adam_kernel(float*, float const*, float*, float*, long, float)") == "adam_kernel"
    assert n("void acimg::batch_frame_kernel<HIP_vector_type<float, 4u> >(float const*, int)") == \
        n("void acimg::batch_frame_kernel<HIP_vector_type<float, 4u>>(float const*, int) [clone .kd]") == \
        "batch_frame_kernel<HIP_vector_type<float, 4u>>"


def test_library_and_fixture_name_the_same_instantiations(records):
    if not os.path.exists(LIB):
        pytest.fail("libacimg.so is not built: run __graft_entry__.build() first")
    kernels = [r["kernel"] for r in records]
    assert len(kernels) == len(set(kernels)), "a kernel has two records"
    new, gone = inv.compare(inv.library_kernels(LIB), records)
    assert not new and not gone, (
        "the library's kernel instantiations differ from tests/golden/kernel_inventory.json\n"
        "  new (add a record that names the GPU test which launches it): %s\n"
        "  gone (remove the record): %s" % (new, gone))


def test_every_record_names_its_tests(records):
    for r in records:
        assert set(r) <= {"kernel", "tests", "seen", "unreachable"} and r["seen"] in ("trace", "reading"), r
        assert r["tests"] or r.get("unreachable"), "%s: no test launches it and no reason is given" % r["kernel"]
        if "unreachable" in r:
            assert not r["tests"] and len(r["unreachable"]) > 20, r


def test_every_named_test_exists(records):
    functions = {}
    for r in records:
        for t in r["tests"]:
            path, _, func = t.partition("::")
            assert func and path.startswith("tests/") and path.endswith("_gpu.py"), t
            if path not in functions:
                with open(os.path.join(ROOT, path)) as f:
                    tree = ast.parse(f.read())
                functions[path] = {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
            assert func in functions[path], "%s names %s, which %s does not define" % (r["kernel"], func, path)

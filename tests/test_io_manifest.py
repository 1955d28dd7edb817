"""Coverage guard for csrc/io/, the rule of tests/test_kernel_manifest.py applied to the subdirectory: every __global__ kernel there has an
entry naming the test file that reaches it and the hook through which it does; the test file must name that hook."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_IO = os.path.join(ROOT, "streamvoiceanon_amd", "csrc", "io")

IO = "test_gpu_io.py"
MANIFEST = {
    "io_resample_in_kernel": (IO, "test_resample"),
    "io_resample_out_kernel": (IO, "test_resample"),
}


def kernels_in_source():
    found = {}
    for fn in sorted(os.listdir(CSRC_IO)):
        if not fn.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC_IO, fn)) as f:
            src = f.read()
        names = re.findall(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", src)
        assert len(names) == len(re.findall(r"\b__global__\b", src)), (fn, "a __global__ this test cannot name")
        for n in names:
            found[n] = fn
    return found


def test_every_io_kernel_has_a_test_that_names_its_hook():
    found = kernels_in_source()
    assert sorted(found) == sorted(MANIFEST), "kernels of csrc/io/ and the manifest differ: %s vs %s" % (sorted(found), sorted(MANIFEST))
    for k, (fn, hook) in MANIFEST.items():
        path = os.path.join(ROOT, "tests", fn)
        assert os.path.isfile(path), (k, fn)
        with open(path) as f:
            assert hook in f.read(), "%s: %s does not name %s" % (k, fn, hook)


def test_the_hook_launches_both_kernels():
    """sva_test_resample reaches the kernels through their launchers, and nothing outside csrc/io/ launches them except the adaptor"""
    with open(os.path.join(CSRC_IO, "io_hooks.hip")) as f:
        hooks = f.read()
    assert "launch_io_resample_in(" in hooks and "launch_io_resample_out(" in hooks
    with open(os.path.join(CSRC_IO, "resample.hip")) as f:
        src = f.read()
    for k in MANIFEST:
        assert re.search(r"hipLaunchKernelGGL\(\s*%s\b" % k, src), k
    with open(os.path.join(ROOT, "streamvoiceanon_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "io/resample.hip" in mk and "io/io_hooks.hip" in mk

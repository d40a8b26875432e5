"""The co-residency budget of the served pendulum pair, read from the built library's code-object metadata (no GPU, no instruction is
looked at): one wave of rollout_served_kernel and one of env_server_kernel share a SIMD's 512 vector registers, allocated in blocks
of 8, or the server's waves wait until the rollout waves have finished and every replica falls back -- same results, none of the speed
(tests/test_gpu_env_server.py: test_every_replica_is_served_at_the_bench_size sees that on a GPU; this sees it in the build).
Scratch: the server has none (a wave with scratch takes part in the launch's scratch set-up: the two kernels then no longer start
together), and the rollout kernel's stays within what it has had since the server landed: 80 bytes in the specialised instantiations,
96 in the generic one."""
import glob
import os
import re
import shutil
import subprocess

import pytest

LLVM_DIRS = ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin")
SPECS = ("NS_15SpecPendulumTcAILi0EEE", "NS_15SpecPendulumTcAILi1EEE", "NS_15SpecPendulumTcAILi3EEE", "NS_8SpecNoneE")
FIELDS = (".vgpr_count", ".agpr_count", ".private_segment_fixed_size")


def _tool(name, *args, cwd=None):
    d = next((d for d in LLVM_DIRS if os.path.exists(os.path.join(d, name))), None)
    assert d, f"{name} not found under /opt/rocm (the tools the build itself uses)"
    return subprocess.run([os.path.join(d, name)] + list(args), cwd=cwd, capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def kernel_metadata(grlx, tmp_path_factory):
    """{kernel symbol: {field: value}} over every gfx950 code object of the library (as tools/kernel_isa_diff.py reads them)"""
    tmp = str(tmp_path_factory.mktemp("code_objects"))
    shutil.copy(grlx.capi.lib_path(), os.path.join(tmp, "lib.so"))
    _tool("llvm-objdump", "--offloading", "lib.so", cwd=tmp)          # writes lib.so.<n>.<target> next to the input
    meta = {}
    for co in sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950"))):
        cur, kcol = None, 0
        for ln in _tool("llvm-readelf", "--notes", co).split("\n"):
            m = re.match(r"\s*(?:- )?(\.\w+):\s+(.*)$", ln)
            if not m:
                continue
            col = ln.index(".")
            if ln.lstrip().startswith("- .agpr_count"):
                cur, kcol = {}, col                                   # first key of a kernel's entry (the keys are sorted)
            if cur is None or col != kcol:
                continue                                              # (an argument's keys sit deeper)
            if m.group(1) in FIELDS:
                cur[m.group(1)] = int(m.group(2))
            if m.group(1) == ".name":
                meta[m.group(2).strip("'\"")] = cur
    assert len(meta) > 20, "no kernel metadata found in the library"
    return meta


def _round8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("spec", SPECS)
def test_the_pair_fits_one_simd(kernel_metadata, spec):
    server = kernel_metadata[f"_ZN4grlx17env_server_kernelILi0ELi3E{spec}EEvNS_9DevParamsE"]
    rollout = kernel_metadata[f"_ZN4grlx21rollout_served_kernelILi3E{spec}EEvNS_9DevParamsEi"]
    print(f"{spec}: server {server}, rollout {rollout}")
    # (.vgpr_count is the unified total: vector + accumulation registers)
    assert server[".vgpr_count"] >= server[".agpr_count"] and rollout[".vgpr_count"] > 256
    total = _round8(server[".vgpr_count"]) + _round8(rollout[".vgpr_count"])
    assert total <= 512, f"{spec}: {rollout['.vgpr_count']} + {server['.vgpr_count']} registers, {total} in blocks of 8"
    assert server[".private_segment_fixed_size"] == 0, f"{spec}: the server has scratch"
    assert rollout[".private_segment_fixed_size"] <= (96 if spec == "NS_8SpecNoneE" else 80), f"{spec}: the rollout kernel's scratch grew"

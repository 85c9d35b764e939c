"""Kernel metadata of qvit_col2im_quant_backward in the built library: twelve instantiations (index type x mode x
arm), none of them with scratch, the streaming ones within the register budget of eight waves per SIMD. Read from
the gfx950 code objects inside libqvit_hip.so with the LLVM tools that ship beside hipcc (llvm-objdump unbundles,
llvm-readelf prints the AMDGPU metadata note); runs without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from quantized_vit_amd import build

KERNEL = "col2im_quant_backward_kernel"


def _llvm(tool):
    root = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))
    for cand in (os.path.join(root, "llvm", "bin", tool), os.path.join(root, "lib", "llvm", "bin", tool),
                 shutil.which(tool)):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError(f"{tool} not found beside hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: {metadata key: int}} of the new kernel's instantiations."""
    tmp = tmp_path_factory.mktemp("code_objects")
    lib = shutil.copy(build.build(), tmp / "libqvit_hip.so")          # llvm-objdump extracts beside its input
    subprocess.run([_llvm("llvm-objdump"), "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp)
    found = {}
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([_llvm("llvm-readelf"), "--notes", str(tmp / f)], check=True, capture_output=True,
                               text=True).stdout
        for entry in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", entry)
            if name and KERNEL in name.group(1):
                found[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return found


def test_every_instantiation_has_zero_scratch(kernels):
    """Fails without the feature: the library has no such kernel."""
    assert len(kernels) == 12, sorted(kernels)
    for index in ("Ii", "Il"):                       # int, long
        for mode in ("Li0E", "Li1E", "Li2E"):        # fold only, linear, nonlinear
            for arm in ("Lb1E", "Lb0E"):             # 16-byte arm, scalar arm
                assert sum(f"{KERNEL}{index}{mode}{arm}" in n for n in kernels) == 1, (index, mode, arm)
    for name, meta in kernels.items():
        print(name, {k: meta[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
                                          "group_segment_fixed_size")})
        assert meta["private_segment_fixed_size"] == 0, name
        assert meta["group_segment_fixed_size"] <= 96, name           # block_sum3's 4 x 3 doubles, nothing else
        if "Li2E" not in name:                                        # (the nonlinear quantizer's log / exp take more)
            assert meta["vgpr_count"] <= 64, name

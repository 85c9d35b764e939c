"""Kernel metadata of qvit_quant_error in the built library: eight instantiations of quant_error_kernel (quantizer
type x arm x index type) and the fold kernel, none of them with scratch, with the LDS and VGPR figures DESIGN.md
section 23 records. Read from the gfx950 code objects inside libqvit_hip.so with the LLVM tools that ship beside hipcc
(llvm-objdump unbundles, llvm-readelf prints the AMDGPU metadata note); runs without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from quantized_vit_amd import build

MAIN, FOLD = "quant_error_kernel", "quant_error_fold_kernel"
MAIN_LDS = 16 * 4 * 3 * 8 + 16 * 4    # the reduction slots of 16 candidates x 4 waves, and 16 saturation codes
FOLD_LDS = 4 * 3 * 8
# VGPRs of the 16-byte arm and of the scalar arm (the larger index type), linear / nonlinear
VGPR_MAX = {("Lb0E", "Lb1E"): 136, ("Lb1E", "Lb1E"): 176, ("Lb0E", "Lb0E"): 88, ("Lb1E", "Lb0E"): 120}


def _llvm(tool):
    root = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))
    for cand in (os.path.join(root, "llvm", "bin", tool), os.path.join(root, "lib", "llvm", "bin", tool),
                 shutil.which(tool)):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError(f"{tool} not found beside hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: {metadata key: int}} of the kernels of quant_error.hip."""
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
            if name and (MAIN in name.group(1) or FOLD in name.group(1)):
                found[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return found


def test_every_instantiation_has_zero_scratch(kernels):
    """Fails without the feature: the library has no such kernels."""
    assert len(kernels) == 9, sorted(kernels)
    assert sum(FOLD in n for n in kernels) == 1
    for nonlinear in ("Lb0E", "Lb1E"):
        for vec in ("Lb0E", "Lb1E"):
            for index in ("i", "l"):                     # int, long
                assert sum(f"{MAIN}I{nonlinear}{vec}{index}E" in n for n in kernels) == 1, (nonlinear, vec, index)
    for name, meta in kernels.items():
        print(name, {k: meta[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
                                          "group_segment_fixed_size")})
        assert meta["private_segment_fixed_size"] == 0, name
        assert meta.get("vgpr_spill_count", 0) == 0, name    # (48 candidate uniforms: a few SGPRs park in VGPR lanes)
        if FOLD in name:
            assert meta["group_segment_fixed_size"] == FOLD_LDS and meta["vgpr_count"] <= 32, name
            continue
        assert meta["group_segment_fixed_size"] == MAIN_LDS, name
        key = next(k for k in VGPR_MAX if f"{MAIN}I{k[0]}{k[1]}" in name)
        assert meta["vgpr_count"] <= VGPR_MAX[key], name     # at least two (nonlinear 16-byte arm) .. five waves per SIMD

"""Kernel metadata of the uint8 image input in the built library: six instantiations of im2col_u8_kernel (index type x
arm) and two of u8_normalize_kernel, none of them with scratch, each with exactly its table in LDS. Read from the
gfx950 code objects inside libqvit_hip.so with the LLVM tools that ship beside hipcc (llvm-objdump unbundles,
llvm-readelf prints the AMDGPU metadata note); runs without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from quantized_vit_amd import build

IM2COL, NORMALIZE = "im2col_u8_kernel", "u8_normalize_kernel"
CODE_TABLE_BYTES = 16 * 256          # int8 [16][256]
VALUE_TABLE_BYTES = 16 * 1024        # fp32 [16][256]
LDS_EXTRA = 0                        # the kernels declare the table and nothing else


def _llvm(tool):
    root = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))
    for cand in (os.path.join(root, "llvm", "bin", tool), os.path.join(root, "lib", "llvm", "bin", tool),
                 shutil.which(tool)):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError(f"{tool} not found beside hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: {metadata key: int}} of the two kernels' instantiations."""
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
            if name and (IM2COL in name.group(1) or NORMALIZE in name.group(1)):
                found[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return found


def test_every_instantiation_has_zero_scratch(kernels):
    """Fails without the feature: the library has no such kernels."""
    assert len(kernels) == 8, sorted(kernels)
    for index in ("Ii", "Il"):                       # int, long
        for arm in ("Li0E", "Li1E", "Li2E"):         # scalar, NCHW 16-byte, NHWC C == 3
            assert sum(f"{IM2COL}{index}{arm}" in n for n in kernels) == 1, (index, arm)
        assert sum(f"{NORMALIZE}{index}E" in n for n in kernels) == 1, index
    for name, meta in kernels.items():
        print(name, {k: meta[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
                                          "group_segment_fixed_size")})
        assert meta["private_segment_fixed_size"] == 0, name
        table = CODE_TABLE_BYTES if IM2COL in name else VALUE_TABLE_BYTES
        assert meta["group_segment_fixed_size"] <= table + LDS_EXTRA, name
        assert meta["vgpr_count"] <= 64, name        # eight waves per SIMD: these kernels stream

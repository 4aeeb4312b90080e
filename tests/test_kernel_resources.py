"""Register, scratch and LDS budgets of the colour blend kernels, read from the built library's code-object metadata (no GPU needed).

A 1080p frame has 8 160 tiles and the chip 8 192 wave slots at eight waves per SIMD: the tile-wave colour kernels run every tile of the frame in ONE
resident round only while a wave needs at most 64 VGPRs, no scratch and at most 5 KB of LDS.  Past any of the three the frame takes a second round
(+16 %, docs/EXPERIMENTS.md section 7).  The limits are the hardware's (512 VGPRs per SIMD lane / 8 waves, 160 KB of LDS per CU / 32 waves), not the
kernels' present figures.

Only the metadata notes are read (llvm-readelf --notes on the gfx950 code objects embedded in libibgs_rast.so); the instruction stream is not looked at.
The last test asks the host's choice of the colour backward's atomic path for P Gaussians (ibgs_grad_acc_offsets_fit32): 32-bit row offsets while
P * 64 bytes fit 32 unsigned bits, 64-bit addresses beyond."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

from ibgs_amd import _lib

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
BUDGET = {"vgpr_count": 64, "private_segment_fixed_size": 0, "group_segment_fixed_size": 5120}
KERNELS = {          # mangled name -> what it is
    "_ZN4ibgs23render_bwd_color_kernelENS_9BwdParamsE": "render_bwd_color_kernel",
    "_ZN4ibgs29render_bwd_color_noabs_kernelENS_9BwdParamsE": "render_bwd_color_noabs_kernel",
    "_ZN4ibgs17render_fwd_kernelILi0ELi4ELi4EEEvNS_9FwdParamsE": "render_fwd_kernel<0, 4, 4>",
}


def gfx950_code_objects(lib_path):
    """The device code objects of every translation unit: hipcc leaves one uncompressed offload bundle per unit in the library."""
    blob = open(lib_path, "rb").read()
    out = []
    for m in re.finditer(re.escape(MAGIC), blob):
        p = m.start()
        (n,) = struct.unpack_from("<Q", blob, p + len(MAGIC))
        o = p + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, o)
            o += 24
            triple = blob[o:o + tlen].decode()
            o += tlen
            if "gfx950" in triple and size > 0:
                out.append(blob[p + off:p + off + size])
    return out


def kernel_metadata(lib_path):
    """{kernel name: {field: int}} from the AMDGPU metadata notes of every code object."""
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(gfx950_code_objects(lib_path)):
            path = os.path.join(tmp, "unit%d.co" % i)
            with open(path, "wb") as f:
                f.write(co)
            text = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
            for entry in re.split(r"\n  - ", text):
                name = re.search(r"\.name:\s+(\S+)", entry)
                if not name:
                    continue
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s+(\d+)", entry)}
    return meta


@pytest.fixture(scope="module")
def metadata(built_lib):
    if not os.path.exists(READELF):
        pytest.fail("llvm-readelf of the ROCm toolchain not found at %s" % READELF)
    return kernel_metadata(_lib.LIB_PATH)


@pytest.mark.parametrize("mangled", sorted(KERNELS), ids=lambda m: KERNELS[m])
def test_colour_blend_kernels_fit_one_resident_round(metadata, mangled):
    assert mangled in metadata, "%s not found in the library's code objects (%d kernels read)" % (KERNELS[mangled], len(metadata))
    m = metadata[mangled]
    print("\n%s: %s" % (KERNELS[mangled], m))
    assert m["vgpr_count"] <= BUDGET["vgpr_count"], m
    assert m["private_segment_fixed_size"] == BUDGET["private_segment_fixed_size"], m
    assert m["group_segment_fixed_size"] <= BUDGET["group_segment_fixed_size"], m


def test_atomic_path_selection_by_arena_size(built_lib):
    """Rows are 64 bytes: the last row of P Gaussians starts at (P - 1) * 64, and every offset into the arena fits 32 unsigned bits iff P <= 2^26.
    The function alone is asked -- no arena of that size is allocated."""
    fit = built_lib.ibgs_grad_acc_offsets_fit32
    assert fit(1 << 26) == 1
    assert fit((1 << 26) + 1) == 0
    assert fit(0) == 1 and fit(1) == 1 and fit(1000000) == 1
    assert fit(1 << 31) == 0 and fit(-1) == 0

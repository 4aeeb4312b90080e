"""The workgroup reduce / scan helpers the geometry units share (csrc/block_ops.h): the order of the deterministic f64 sums bit for bit against a host
walk of the stated tree, min / max with infinities, and the exclusive scans at every (threads, type) the units use: tests/csrc/test_block_ops.hip, built
with hipcc and run on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_block_ops_match_their_host_restatements(tmp_path):
    exe = str(tmp_path / "tbo")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-I", os.path.join(ROOT, "ibgs_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "csrc", "test_block_ops.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "block ops ok" in r.stdout, r.stdout + r.stderr

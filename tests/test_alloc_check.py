"""The device-allocation registry and the staged replacement of capacity growth (csrc/dev_alloc.h) on the CPU: the
stand-alone program csrc/alloc_check.cpp links them with malloc-backed raw functions under ASan + UBSan and checks the
bytes bookkeeping (with and without guards, zero counts), a committed stage, a stage abandoned at each of its five
allocations (bytes and the live set as before, no leak, no double free) and destroy with live entries."""
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "scalecube-cluster_amd" / "csrc"


def test_alloc_check_builds_and_passes(tmp_path):
    exe = tmp_path / "alloc_check"
    subprocess.check_call(["make", "-s", "-C", str(CSRC), "alloc_check", f"ALLOC_CHECK={exe}"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "alloc_check ok" in r.stdout

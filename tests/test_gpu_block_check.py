"""The block Gram-Schmidt and streaming kernels one by one on the GPU:
tests/native/block_check (built by __graft_entry__.build()) calls each
kt::launch_* of kt_gemm_ts.hip, kt_colbatch.hip, kt_tsqr.hip (sum_slabs,
poly4) and the small streaming kernels of kt_kernels.hip and compares with
exact-integer / long double references, a-priori bounds, NaN padding and
output sentinels.  The program runs once; each group is one test."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "block_check", "block_check")
GROUPS = ["gram", "combine", "chol_rinv", "fro_colmax_scale", "colbatch", "streaming"]


@pytest.fixture(scope="module")
def device_run():
    """(process, parsed JSON line or None, the enumeration's case counts); one
    fresh process, no retry."""
    assert os.path.exists(CHECK), "tests/native/block_check/block_check is not built (__graft_entry__.build())"
    c = subprocess.run([CHECK, "--count"], capture_output=True, text=True, timeout=60)
    assert c.returncode == 0, (c.returncode, c.stdout, c.stderr)
    # the enumeration --host runs (tests/test_block_check_host.py holds --host to it)
    counts = {g: v["cases"] for g, v in json.loads(c.stdout.strip().splitlines()[-1])["groups"].items()}
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:], r.stderr[-2000:])
    try:
        out = json.loads(r.stdout.strip().splitlines()[-1])
    except (IndexError, ValueError):
        out = None
    return r, out, counts


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_block_kernels_match_references(device_run, group):
    """No failed case in the group, and as many cases as the host run has
    (none skipped on the device).  A HIP error or a signal fails every group."""
    r, out, counts = device_run
    assert out is not None, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "hip_error" not in out and r.returncode in (0, 1), (r.returncode, out.get("hip_error"), r.stderr[-2000:])
    assert out["mode"] == "device"
    g = out["groups"][group]
    print(group, "cases", g["cases"], "seconds", g["seconds"], "wall", out["wall_s"])
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group] and g["cases"] > 0, (g["cases"], counts[group])

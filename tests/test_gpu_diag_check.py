"""The diag / entries kernels one by one on the GPU: tests/native/diag_check
(built by __graft_entry__.build()) calls launch_diag_qtz, launch_diag_sum_parts,
launch_diag_start, launch_diag_combine(_y), launch_diag_finish, launch_diag_d0,
launch_entries_accumulate and launch_entries_e0 of kt_diag.hip in every (P, KP)
form their switches admit, and launch_weighted_sum_tab and launch_unit_start of
kt_adapt.hip, and compares with exact-integer / long double references,
a-priori bounds, sentinels and guards, and the bit-for-bit statements the source
makes.  The program runs once; each group is one test."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "diag_check", "diag_check")
GROUPS = ["qtz_sum", "start", "combine", "finish", "entries", "d0", "adapt_stream", "contract"]


@pytest.fixture(scope="module")
def device_run():
    """(process, parsed JSON line or None, the enumeration's case counts); one
    fresh process, no retry."""
    assert os.path.exists(CHECK), "tests/native/diag_check/diag_check is not built (__graft_entry__.build())"
    c = subprocess.run([CHECK, "--count"], capture_output=True, text=True, timeout=60)
    assert c.returncode == 0, (c.returncode, c.stdout, c.stderr)
    # the enumeration --host runs (tests/test_diag_check_host.py holds --host to it)
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
def test_diag_kernels_match_references(device_run, group):
    """No failed case in the group (every bounded case within its a-priori
    bound, every exact and contract case equal), and as many cases as the
    enumeration has (none skipped on the device).  A HIP error or a signal
    fails every group."""
    r, out, counts = device_run
    assert out is not None, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "hip_error" not in out and r.returncode in (0, 1), (r.returncode, out.get("hip_error"), r.stderr[-2000:])
    assert out["mode"] == "device"
    g = out["groups"][group]
    print(group, "cases", g["cases"], "seconds", g["seconds"], "max_ratio", g["max_ratio"], "wall", out["wall_s"])
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group] and g["cases"] > 0, (g["cases"], counts[group])
    assert g["max_ratio"] <= 1.0

"""The expmv Taylor term kernels one by one on the GPU: tests/native/expmv_check
(built by __graft_entry__.build()) calls launch_expmv_begin, launch_expmv_term,
launch_expmv_check, launch_expmv_slot_check and launch_expmv_step in all 72
template instances of its four forms, the whole stop state machine stage by
stage, and launch_sweep_scales, launch_gram_diag, launch_fill and
launch_pair_start, and compares with exact-integer / long double references,
a-priori bounds, sentinels and guards, and the bit-for-bit statements the source
makes.  The program runs once; each group is one test."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "expmv_check", "expmv_check")
GROUPS = ["begin", "unfused", "step", "stage", "setup"]


@pytest.fixture(scope="module")
def device_run():
    """(process, parsed JSON line or None, the enumeration's case counts); one
    fresh process, no retry."""
    assert os.path.exists(CHECK), "tests/native/expmv_check/expmv_check is not built (__graft_entry__.build())"
    c = subprocess.run([CHECK, "--count"], capture_output=True, text=True, timeout=60)
    assert c.returncode == 0, (c.returncode, c.stdout, c.stderr)
    # the enumeration --host runs (tests/test_expmv_check_host.py holds --host to it)
    counts = {g: v["cases"] for g, v in json.loads(c.stdout.strip().splitlines()[-1])["groups"].items()}
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=180)
    print(r.stdout[-6000:], r.stderr[-2000:])
    try:
        out = json.loads(r.stdout.strip().splitlines()[-1])
    except (IndexError, ValueError):
        out = None
    return r, out, counts


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_expmv_kernels_match_references(device_run, group):
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


@pytest.mark.gpu
def test_deep_shape_reaches_the_third_trip(device_run):
    """The deep shape is sized from the device's own grid of forms 2 and 3
    (expmv_rows_blocks): the heavy, long, medium and short loops of
    k_expmv_rows each make at least three trips, at P = 16 and at P = 1."""
    r, out, _ = device_run
    assert out is not None, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert sorted(t["P"] for t in out["trips"]) == [1, 16], out["trips"]
    for t in out["trips"]:
        print(t)
        assert min(t["heavy"], t["long"], t["medium"], t["short"]) >= 3, t

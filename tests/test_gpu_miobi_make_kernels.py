"""Kernel-level GPU test of kt_miobi_make's kernels (kt_miobi.hip): runs
tests/native/miobi_make_check, which calls the make-edge score and pick
launchers one by one against host loops (t in {2, 3, 16, 17, 31, 32}; candidate
blocks of 2, 63, 64, 65, 129 and 200 ranks with a live m below; empty, full and
random masks, a single free pair in the first position and in the ragged
corner; bit-identical rows in different tiles under grids of 1, 2 and the
maximum; a pick that grows m by one and one that clamps at n).  The case
counts are held to those of the program's --host enumeration; the score
tolerance is 1e-12 relative against a long double sum."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "tests", "native", "miobi_make_check", "miobi_make_check")
GROUPS = ["score", "pick", "apply"]


@pytest.fixture(scope="module")
def kernel_run():
    assert os.path.exists(CHECK), "tests/native/miobi_make_check/miobi_make_check is not built (__graft_entry__.build())"
    h = subprocess.run([CHECK, "--host"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0, (h.returncode, h.stdout, h.stderr)
    counts = {g: v["cases"] for g, v in json.loads(h.stdout.strip().splitlines()[-1])["groups"].items()}
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    try:
        out = json.loads(r.stdout.strip().splitlines()[-1])
    except (IndexError, ValueError):
        out = None
    return r, out, counts


@pytest.mark.parametrize("group", GROUPS)
def test_kernels_match_host_loops(kernel_run, group):
    r, out, counts = kernel_run
    assert out is not None, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "hip_error" not in out and r.returncode in (0, 1), (r.returncode, out.get("hip_error"), r.stderr[-2000:])
    assert out["mode"] == "device"
    g = out["groups"][group]
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group] and g["cases"] > 0, (g["cases"], counts[group])


def test_score_error_is_within_the_bound(kernel_run):
    _, out, _ = kernel_run
    assert out is not None
    print("largest relative score error against the long double sum:", out["max_score_rel_err"])
    assert out["max_score_rel_err"] <= 1e-12

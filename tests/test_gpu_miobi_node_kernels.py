"""Kernel-level GPU test of kt_miobi_break_node's kernels (kt_miobi.hip): runs
tests/native/miobi_node_check, which calls the node score, pick and column-sum
launchers one by one against host loops (t in {2, 3, 16, 17, 31, 32}; n in {1,
63, 64, 65}; rows of 0, 1, the in-flight batch -1 / 0 / +1, the long-row
threshold -1 / 0 / +1, and rows longer than one workgroup trip of a split row;
dead neighbours inside a row, a live row whose neighbours are all dead, every
node dead; grids of 1, 2 and the maximum bit-identical; equal scores in
different workgroups, for short rows and for split rows; the removed-entry
count crossing the threshold with its carry; no-op launches after the stop and
the window-end word).  The case counts are held to those of the program's
--host enumeration; the score bound is computed per row in the program:
(max |x| (len + 3) + t + 8) 2^-53 relative, x the exp argument."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "tests", "native", "miobi_node_check", "miobi_node_check")
GROUPS = ["score", "pick", "apply", "colsum"]


@pytest.fixture(scope="module")
def kernel_run():
    assert os.path.exists(CHECK), "tests/native/miobi_node_check/miobi_node_check is not built (__graft_entry__.build())"
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
    print("largest score error as a fraction of its row's bound:", out["max_score_err_over_bound"])
    assert out["max_score_err_over_bound"] <= 1.0

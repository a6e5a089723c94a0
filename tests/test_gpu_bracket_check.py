"""k_bracket_check (kt_adapt.hip), the device stopping test of the bracket
columns, against the host rule and the stop rule on synthetic
sweep records: tests/native/bracket_check (built by __graft_entry__.build())
runs every shape once and prints the figures; the tolerances are held here.

Tolerance: the device QL differs from the host QL by summation order and FMA
contraction only, so L_j and U_j are allowed ten times the spread between the
host QL and numpy.linalg.eigh on Lanczos tridiagonals ("spread_max" of
tests/golden/adaptive_values.json, 2.35e-13, so 2.35e-12 here), relative to sum
exp(theta_k - mu) over the eigenvalues the sum takes -- the size of the terms
that the weights z_k^2, which the QL gives to an absolute accuracy, multiply --
as tests/test_gpu_node_check.py holds X_j to sum |f(eig(T_j))|.  On the columns
of kind 3 (mu = 640) that scale is ~1 for U_j, the bordered matrix's eigenvalue
at mu, while U_j itself is one weight of ~1e-12: the bound says nothing about
U_j's own digits there (the QL cannot give them), and those columns test the
scaling, the decisions and L_j; kinds 0 and 4 hold U_j.  The device's
stopped flag and depth may differ from the host rule's only where some gap U_k
- L_k the run compared lies within that tolerance of rtol L_k."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "bracket_check", "bracket_check")
with open(os.path.join(ROOT, "tests", "golden", "adaptive_values.json")) as _f:
    TOL = 10.0 * json.load(_f)["spread_max"]


@pytest.fixture(scope="module")
def run():
    assert os.path.exists(CHECK), "tests/native/bracket_check/bracket_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert "hip_error" not in out, out
    return out


def _cols(out):
    for case in out["cases"]:
        for col in case["cols"]:
            yield case, col


@pytest.mark.gpu
def test_every_shape_and_depth_ran(run):
    got = {(c["live"], c["mcap"], c["j"]) for c in run["cases"]}
    for live in (1, 15, 16):
        for j in (1, 2, 3, 5, 8, 12, 16, 167, 168, 169, 170, 255, 256):
            assert (live, 256, j) in got
    assert (16, 128, 127) in got and (16, 128, 128) in got
    assert {c["kind"] for c in run["cases"] if c["live"] >= 15} == {0, 1, 2, 3, 4}
    # the deep depths are reached by running columns, and the cap stops them
    for live in (1, 15, 16):
        assert any(case["live"] == live and case["j"] == 255 and not col["stopped_dev"] for case, col in _cols(run))
        assert any(case["live"] == live and case["j"] == 256 and col["flag_dev"] == 3 for case, col in _cols(run))


@pytest.mark.gpu
def test_sums_match_the_host_rule(run):
    worst = 0.0
    for case, col in _cols(run):
        where = (case["live"], case["mcap"], case["j"], case["kind"], col)
        assert col["lo_host"] > 0.0 and col["lo_dev"] > 0.0, where
        err = abs(col["lo_dev"] - col["lo_host"]) / col["scale_lo"]
        assert col["hi_nan_dev"] == col["hi_nan_host"], where
        if col["scale_hi"] > 0.0:  # the bordered matrix was formed; it has an eigenvalue at mu
            assert not col["hi_nan_host"], where
            err = max(err, abs(col["hi_dev"] - col["hi_host"]) / col["scale_hi"])
        elif not col["hi_nan_host"]:  # a breakdown: hi = lo
            assert col["hi_host"] == col["lo_host"] and col["hi_dev"] == col["lo_dev"], where
        worst = max(worst, err)
        assert err <= TOL, where + (err,)
        assert col["last_dev"] == (col["depth_dev"] if col["stopped_dev"] else case["j"]), where
    print("worst |dev - host| / sum exp(theta - mu) over L_j and U_j", worst, "tolerance", TOL)


@pytest.mark.gpu
def test_stop_decisions_match_the_host_rule(run):
    seen = set()
    for case, col in _cols(run):
        j, kind, r = case["j"], case["kind"], case["run"]
        where = (case["live"], case["mcap"], j, kind, r, col)
        if kind == 1 and j >= 5:  # the breakdown at step 5: exact, hi = lo
            assert (col["stopped_dev"], col["depth_dev"], col["flag_dev"]) == (1, 5, 1), where
            assert col["hi_dev"] == col["lo_dev"], where
        if kind == 2 and j >= 5:  # 3 cos(pi / 6) > 2.5 > 3 cos(pi / 5)
            assert (col["stopped_dev"], col["depth_dev"], col["flag_dev"]) == (1, 5, 2), where
            assert col["hi_nan_dev"] == 1, where
        if kind in (1, 2) and j < 5:
            assert col["stopped_dev"] == 0, where
        if r == 1:  # rtol = -1: only the cap stops these columns
            want = (1, case["mcap"], 3) if j == case["mcap"] else (0, 0, 0)
            assert (col["stopped_dev"], col["depth_dev"], col["flag_dev"]) == want, where
        if col["margin"] > TOL:
            assert col["stopped_dev"] == col["stopped_host"], where
            if col["stopped_dev"]:
                assert (col["depth_dev"], col["flag_dev"]) == (col["depth_host"], col["flag_host"]), where
        if kind == 0 and r == 0 and j >= 16:  # the path graph's bracket closes to 1e-10 well before depth 16
            assert col["stopped_dev"] == 1 and col["flag_dev"] == 0 and 3 <= col["depth_dev"] <= 12, where
        if kind == 3:  # half-width 300: no gap of 1e-10 by depth 256
            assert col["flag_dev"] in (0, 3) and (not col["stopped_dev"] or col["depth_dev"] == case["mcap"]), where
        if col["stopped_dev"]:
            seen.add(col["flag_dev"])
            if col["flag_dev"] == 0:
                assert col["hi_dev"] - col["lo_dev"] <= case["rtol"] * col["lo_dev"], where
    assert seen == {0, 1, 2, 3}


@pytest.mark.gpu
def test_active_count_and_untouched_state(run):
    for case in run["cases"]:
        assert case["active"] == case["running"] == sum(1 for col in case["cols"] if not col["stopped_dev"]), case
        assert case["untouched"] == 1, case
    # both launch forms ran: one 16-lane launch up to depth 168, 8-lane groups from 169
    assert any(c["j"] == 168 and c["live"] == 16 for c in run["cases"])
    assert any(c["j"] == 169 and c["live"] == 16 and c["running"] > 0 for c in run["cases"])

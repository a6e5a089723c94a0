"""k_node_check (kt_adapt.hip), the device stopping test of the node-removal
columns, against the host value function and the lag-2 rule
on synthetic sweep records: tests/native/node_check (built by
__graft_entry__.build()) runs every shape once and prints the figures; the
tolerances are held here.

Tolerance: the device QL differs from the host QL by summation order and FMA
contraction only, so X_j is allowed ten times the spread between the host QL
and numpy.linalg.eigh on Lanczos tridiagonals ("spread_max" of
tests/golden/adaptive_values.json, 2.35e-13, so 2.35e-12 here), relative to
sum |f(eig(T_j))| -- the size of the sums X_j is the difference of, as
tests/test_gpu_quad_check.py holds the quadrature.  The device's stopped flag
and depth may differ from the host rule's only where some |X_k - X_{k-2}| the
run compared lies within that tolerance of tol."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "node_check", "node_check")
with open(os.path.join(ROOT, "tests", "golden", "adaptive_values.json")) as _f:
    TOL = 10.0 * json.load(_f)["spread_max"]


@pytest.fixture(scope="module")
def run():
    assert os.path.exists(CHECK), "tests/native/node_check/node_check is not built (__graft_entry__.build())"
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
    got = {(c["P"], c["mcap"], c["j"]) for c in run["cases"] if not c["sentinel"]}
    for P in (1, 4, 16):
        for mcap in (128, 256):
            for j in (1, 2, 3, 8, 16, 31, 32, mcap):
                assert (P, mcap, j) in got
    assert {col["kind"] for _, col in _cols(run)} == {0, 1, 2, 3, 4, 5}
    assert all(case["seeded"] == (case["j"] > 16) for case in run["cases"])
    # the deepest depth is reached by running columns at every width
    for P in (1, 4, 16):
        assert any(case["P"] == P and case["j"] == 256 and not col["stopped_dev"] for case, col in _cols(run))


@pytest.mark.gpu
def test_value_matches_the_host_function(run):
    worst = 0.0
    for case, col in _cols(run):
        if col["kind"] == 3:
            continue
        err = abs(col["x_dev"] - col["x_host"]) / col["scale"]
        worst = max(worst, err)
        assert err <= TOL, (case["P"], case["mcap"], case["j"], col, err)
        assert abs(col["x_dev"]) < 1e300 and col["scale"] < 1e300, col
        if col["kind"] == 4 and case["j"] >= 8:  # the scaled comparison at theta_max near exp's range
            assert 650.0 < col["theta"] < 709.0 and abs(col["x_dev"]) > 1e250, col
    print("worst |x_dev - x_host| / sum|f(d2)|", worst, "tolerance", TOL)


@pytest.mark.gpu
def test_stop_decisions_match_the_host_rule(run):
    stopped = running = 0
    for case, col in _cols(run):
        j, kind = case["j"], col["kind"]
        where = (case["P"], case["mcap"], j, col)
        if kind == 3:  # stopped before the first check: left as it was
            assert col["stopped_dev"] == 1 and col["depth_dev"] == 2, where
            continue
        if kind == 1:  # beta_1 = 0
            assert (col["stopped_dev"], col["depth_dev"], col["lucky_dev"]) == (1, 1, 1), where
            continue
        if kind == 2 and j >= 5:  # the breakdown at step 5 ends the column there
            assert (col["stopped_dev"], col["depth_dev"], col["lucky_dev"]) == (1, 5, 1), where
            continue
        if col["margin"] > TOL:
            assert col["stopped_dev"] == col["stopped_host"], where
            if col["stopped_dev"]:
                assert col["depth_dev"] == col["depth_host"] and col["lucky_dev"] == col["lucky_host"], where
        if col["stopped_dev"]:
            assert 3 <= col["depth_dev"] <= j, where
            stopped += 1
        else:
            running += 1
        if j <= 2:
            assert col["stopped_dev"] == 0, where  # X_1 and X_2 are only stored
        if kind == 0 and j >= 16:
            # converged by depth 16 (NumPy: depth 9 on every lane), and a seeded run's
            # first comparison, X_{j-2} against X_{j-4}, is between converged values
            assert col["stopped_dev"] == 1 and col["lucky_dev"] == 0, where
            assert col["depth_dev"] == (j - 2 if case["seeded"] else col["depth_host"]), where
        if kind == 4:  # X ~ 1e290 and more: no two of them are 1e-9 apart
            assert col["stopped_dev"] == 0, where
    assert stopped > 0 and running > 0  # the cases exercise both decisions


@pytest.mark.gpu
def test_active_count_and_untouched_state(run):
    for case in run["cases"]:
        assert case["active"] == sum(1 for col in case["cols"] if not col["stopped_dev"]), case
        assert case["untouched"] == 1, case
    five = [c for c in run["cases"] if c["sentinel"]]
    assert len(five) == 8 and all(c["P"] == 16 and c["live"] == 5 and len(c["cols"]) == 5 for c in five)

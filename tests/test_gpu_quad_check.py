"""k_quad_check (kt_adapt.hip), the adaptive Lanczos depth's device stopping
test, against the host rule on synthetic sweep records: tests/native/quad_check
(built by __graft_entry__.build()) runs every case once and prints the figures;
the tolerances are held here.

Tolerance: the device QL differs from the host QL by summation order and FMA
contraction only, so its quadrature is allowed ten times the spread between
the host QL and numpy.linalg.eigh on the same kind of tridiagonal.  Measured
on the CPU (tests/golden/make_adaptive_fixture.py, "spread_max" of
adaptive_values.json: Lanczos tridiagonals of the seven fixture graphs at
depths 3, 8, 31, 32, 128, quadratures scaled by exp(-theta_max)): 2.35e-13
relative, so the device gets 2.35e-12.  The device's stopped flag may differ
from the host's only where one of the host's three ratios lies within that
tolerance of rtol."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "quad_check", "quad_check")
with open(os.path.join(ROOT, "tests", "golden", "adaptive_values.json")) as _f:
    TOL = 10.0 * json.load(_f)["spread_max"]


@pytest.fixture(scope="module")
def run():
    assert os.path.exists(CHECK), "tests/native/quad_check/quad_check is not built (__graft_entry__.build())"
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
    got = {(c["P"], c["mcap"], c["j"]) for c in run["cases"]}
    for P, mcap in ((1, 256), (4, 256), (16, 128), (16, 256)):
        for j in (3, 8, 31, 32, mcap):
            assert (P, mcap, j) in got
    assert {col["kind"] for _, col in _cols(run)} == {0, 1, 2, 3, 4}


@pytest.mark.gpu
def test_quadrature_matches_the_host_rule(run):
    worst = 0.0
    for case, col in _cols(run):
        if col["kind"] == 1:  # zero column: stops at once with q = 0, depth 0
            assert col["stopped_dev"] == 1 and col["depth_dev"] == 0 and col["q_dev"] == 0.0, (case["j"], col)
            continue
        err = abs(col["q_dev"] - col["q_host"]) / abs(col["q_host"])
        worst = max(worst, err)
        assert err <= TOL, (case["P"], case["mcap"], case["j"], col, err)
        assert 0.0 < col["q_dev"] < 1e300, col  # theta_max ~ 900 stays finite
    print("worst relative q difference", worst, "tolerance", TOL)


@pytest.mark.gpu
def test_stopped_flag_matches_the_host_rule(run):
    rtol = run["rtol"]
    stopped = running = 0
    for case, col in _cols(run):
        if col["kind"] == 1:
            continue
        if col["kind"] == 2:  # breakdown at step 2: cut there whatever the depth
            assert col["stopped_dev"] == 1 and col["depth_dev"] == 2 and col["steps_host"] == 2, (case["j"], col)
            continue
        marginal = any(abs(col[r] - rtol) <= TOL for r in ("r1", "r2") + (("r3",) if col["fe1"] else ()))
        if not marginal:
            assert col["stopped_dev"] == col["conv_host"], (case["P"], case["mcap"], case["j"], col)
        if col["stopped_dev"]:
            assert col["depth_dev"] == case["j"], (case["j"], col)
            stopped += 1
        else:
            running += 1
        if case["j"] < 8:
            assert col["stopped_dev"] == 0, col  # nothing but a breakdown stops below depth 8
    assert stopped > 0 and running > 0  # the cases exercise both decisions


@pytest.mark.gpu
def test_active_count_and_untouched_lanes(run):
    for case in run["cases"]:
        assert case["active"] == sum(1 for col in case["cols"] if not col["stopped_dev"]), case
        assert case["untouched"] == 1, case
    five = [c for c in run["cases"] if c["live"] == 5]
    assert len(five) == 1 and five[0]["P"] == 16 and len(five[0]["cols"]) == 5

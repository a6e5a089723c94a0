"""k_quad_check_wide (kt_adapt.hip), the stopping test of the error-controlled
probe sweeps for any sweep width, against the host rule on synthetic sweep
records, and the gated forms of the y-form step launches (kt_kernels.hip):
tests/native/quad_check_wide (built by __graft_entry__.build()) runs every case
once and prints the figures; the tolerances are held here.

Tolerance: the one tests/test_gpu_quad_check.py derives for k_quad_check (the
same per-column arithmetic): ten times the spread between the host QL and
numpy.linalg.eigh, "spread_max" of tests/golden/adaptive_values.json.  The
stopped flag is compared only where none of the host's ratios lies within that
tolerance of rtol.  The gate cases are bitwise."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "quad_check_wide", "quad_check_wide")
with open(os.path.join(ROOT, "tests", "golden", "adaptive_values.json")) as _f:
    TOL = 10.0 * json.load(_f)["spread_max"]
SHAPES = ((1, 1), (16, 16), (64, 48), (128, 128))
DEPTHS = (3, 8, 31, 32, 128, 129, 200, 256)


@pytest.fixture(scope="module")
def run():
    assert os.path.exists(CHECK), "tests/native/quad_check_wide/quad_check_wide is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:], r.stderr[-2000:])
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
    got = {(c["P"], c["live"], c["j"]) for c in run["cases"]}
    assert got == {(P, live, j) for P, live in SHAPES for j in DEPTHS}
    assert {col["kind"] for _, col in _cols(run)} == {0, 1, 2, 3, 4}
    for case in run["cases"]:
        assert len(case["cols"]) == case["live"]


@pytest.mark.gpu
def test_quadrature_matches_the_host_rule(run):
    worst = 0.0
    for case, col in _cols(run):
        if col["kind"] == 1:  # zero column: stops at once with q = 0, depth 0
            assert col["stopped_dev"] == 1 and col["depth_dev"] == 0 and col["q_dev"] == 0.0, (case["j"], col)
            continue
        err = abs(col["q_dev"] - col["q_host"]) / abs(col["q_host"])
        worst = max(worst, err)
        assert err <= TOL, (case["P"], case["j"], col, err)
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
            assert col["stopped_dev"] == col["conv_host"], (case["P"], case["j"], col)
        if col["stopped_dev"]:
            assert col["depth_dev"] == case["j"], (case["j"], col)
            stopped += 1
        else:
            running += 1
        if case["j"] < 8:
            assert col["stopped_dev"] == 0, col  # nothing but a breakdown stops below depth 8
    assert stopped > 0 and running > 0  # the cases exercise both decisions


@pytest.mark.gpu
def test_running_counts_per_workgroup_and_untouched_state(run):
    for case in run["cases"]:
        ng = (case["live"] + 15) // 16
        assert len(case["running"]) == ng
        for b in range(ng):
            want = sum(1 for col in case["cols"][16 * b:16 * b + 16] if not col["stopped_dev"])
            assert case["running"][b] == want, (case["P"], case["j"], b)
        assert case["untouched"] == 1, (case["P"], case["j"])


@pytest.mark.gpu
def test_guard_argument(run):
    assert run["guard_ok"] == 1


@pytest.mark.gpu
def test_gated_step_launches(run):
    got = {(g["kernel"], g["P"]) for g in run["gate"]}
    assert got == {(k, P) for k in ("pass", "pass_i16", "first", "ycoef") for P in (16, 128)}
    for g in run["gate"]:
        assert g["open_equal"] == 1, g
        assert g["closed_untouched"] == 1, g

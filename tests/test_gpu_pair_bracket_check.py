"""k_pair_bracket_check (kt_adapt.hip), the device stopping test of the pair
columns, against the host rule and the stop rule on synthetic
sweep records: tests/native/pair_bracket_check (built by
__graft_entry__.build()) runs every shape once and prints the figures; the
tolerances are held here.

Tolerance: tests/test_gpu_bracket_check.py's.  The device QL differs from the
host QL by summation order and FMA contraction only, so each column's L_j and
U_j are allowed ten times "spread_max" of tests/golden/adaptive_values.json
(2.35e-13, so 2.35e-12 here), relative to sum exp(theta_k - mu) over the
eigenvalues the sum takes.  A pair's decisions (decided, depth, flag, and the
depth at which a column froze) must equal the host rule's wherever the host
rule's own decisions do not change when lo and hi move by that tolerance times
the four sums' unit ("robust"; the program's rtol = 1e-6 and ftol = 1e-9 sit far
above it, and every pair of this set is robust)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "pair_bracket_check", "pair_bracket_check")
with open(os.path.join(ROOT, "tests", "golden", "adaptive_values.json")) as _f:
    TOL = 10.0 * json.load(_f)["spread_max"]


@pytest.fixture(scope="module")
def run():
    assert os.path.exists(CHECK), \
        "tests/native/pair_bracket_check/pair_bracket_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, repr(TOL)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert "hip_error" not in out, out
    return out


def _pairs(out):
    for case in out["cases"]:
        for pair in case["pairs"]:
            yield case, pair


@pytest.mark.gpu
def test_every_shape_and_depth_ran(run):
    got = {(c["live"], c["mcap"], c["j"]) for c in run["cases"]}
    for live in (2, 14, 16):
        for j in (1, 2, 3, 4, 5, 6, 8, 12, 16, 167, 168, 169, 170, 255, 256):
            assert (live, 256, j) in got
    assert (16, 128, 127) in got and (16, 128, 128) in got
    assert {p["kind"] for c, p in _pairs(run) if c["live"] >= 14 and c["run"] == 0} == {0, 1, 2, 3, 4}
    # the deep depths are reached by running pairs, and the cap stops them
    for live in (2, 14, 16):
        assert any(c["live"] == live and c["j"] == 255 and not p["cols"][0]["decided_dev"] for c, p in _pairs(run))
        assert any(c["live"] == live and c["j"] == 256 and p["cols"][0]["flag_dev"] == 3 for c, p in _pairs(run))


@pytest.mark.gpu
def test_sums_match_the_host_rule(run):
    worst = 0.0
    for case, pair in _pairs(run):
        for col in pair["cols"]:
            where = (case["live"], case["mcap"], case["j"], case["run"], pair["p"], pair["kind"], col)
            assert col["lo_host"] > 0.0 and col["lo_dev"] > 0.0, where
            err = abs(col["lo_dev"] - col["lo_host"]) / col["scale_lo"]
            assert col["hi_nan_dev"] == col["hi_nan_host"], where
            if col["scale_hi"] > 0.0:  # the bordered matrix was formed
                assert not col["hi_nan_host"], where
                err = max(err, abs(col["hi_dev"] - col["hi_host"]) / col["scale_hi"])
            elif not col["hi_nan_host"]:  # a breakdown: hi = lo
                assert col["hi_host"] == col["lo_host"] and col["hi_dev"] == col["lo_dev"], where
            worst = max(worst, err)
            assert err <= TOL, where + (err,)
            assert col["last_dev"] == (col["depth_dev"] if col["stopped_dev"] else case["j"]), where
    print("worst |dev - host| / sum exp(theta - mu) over L_j and U_j", worst, "tolerance", TOL)


@pytest.mark.gpu
def test_decisions_match_the_host_rule(run):
    seen, compared = set(), 0
    for case, pair in _pairs(run):
        j, kind, r = case["j"], pair["kind"], case["run"]
        plus, minus = pair["cols"]
        where = (case["live"], case["mcap"], j, r, pair)
        dec = plus["decided_dev"]
        assert minus["decided_dev"] == dec, where
        if dec:
            assert plus["flag_dev"] == minus["flag_dev"] and plus["stopped_dev"] and minus["stopped_dev"], where
            seen.add(plus["flag_dev"])
        depth = max(plus["depth_dev"], minus["depth_dev"]) if dec else 0
        for col in (plus, minus):  # a stopped column of an undecided pair is a frozen one
            if col["stopped_dev"] and not dec:
                assert col["flag_dev"] == 1 and col["hi_dev"] == col["lo_dev"], where
        if pair["robust"]:
            compared += 1
            assert (dec, depth, plus["flag_dev"] if dec else -1) == \
                (pair["decided_host"], pair["depth_host"], pair["flag_host"]), where
            for col in (plus, minus):
                if col["frozen_host"]:
                    assert col["stopped_dev"] and col["depth_dev"] == col["frozen_host"], where
                elif dec:
                    assert col["depth_dev"] == depth, where
                else:
                    assert not col["stopped_dev"], where
        # what each kind is there for
        if kind == 1 and j >= 3:  # the - column froze at step 3 and keeps that depth whatever the pair does
            assert (minus["stopped_dev"], minus["depth_dev"], minus["last_dev"]) == (1, 3, 3), where
            assert minus["hi_dev"] == minus["lo_dev"], where
            if r == 0 and j >= 8:
                assert dec and plus["flag_dev"] in (0, 4) and plus["depth_dev"] > 3, where
        if kind == 2 and j >= 5:
            assert (dec, plus["flag_dev"], plus["depth_dev"], minus["depth_dev"]) == (1, 1, 3, 5), where
        if kind == 2 and j in (3, 4):
            assert (dec, plus["stopped_dev"], plus["depth_dev"], minus["stopped_dev"]) == (0, 1, 3, 0), where
        if kind == 3:  # 3 cos(pi / 6) > 2.5 > 3 cos(pi / 5)
            assert (dec, plus["flag_dev"] if dec else -1) == ((1, 2) if j >= 5 else (0, -1)), where
            if j >= 5:
                assert plus["hi_nan_dev"] == 1 and (plus["depth_dev"], minus["depth_dev"]) == (5, 5), where
        if kind == 0 and r == 0 and j >= 8:
            assert dec and plus["flag_dev"] == 0 and 3 <= depth <= 8, where
        if kind == 4 and r == 0:  # lo = -hi: never flag 0
            assert plus["lo_dev"] == minus["lo_dev"] and plus["hi_dev"] == minus["hi_dev"], where
            if j >= 8:
                assert dec and plus["flag_dev"] == 4, where
        if r == 1:  # rtol = ftol = -1: only the cap decides these pairs
            want = (1, 3) if j == case["mcap"] else (0, 0)
            assert (dec, plus["flag_dev"] if dec else 0) == want, where
            if dec:
                assert plus["depth_dev"] == case["mcap"] and minus["depth_dev"] == (3 if kind == 1 else case["mcap"])
        if dec and plus["flag_dev"] == 0:
            lo = 0.5 * (plus["lo_dev"] - minus["hi_dev"])
            hi = 0.5 * (plus["hi_dev"] - minus["lo_dev"])
            assert lo * hi > 0 and 0 <= hi - lo <= case["rtol"] * min(abs(lo), abs(hi)), where
    assert seen == {0, 1, 2, 3, 4}
    assert compared == sum(1 for _ in _pairs(run)), "every pair of this set is robust"


@pytest.mark.gpu
def test_active_count_and_untouched_state(run):
    for case in run["cases"]:
        assert case["active"] == case["running"], case
        assert case["untouched"] == 1, case
    # both launch forms ran: one 16-lane launch up to depth 168, 8-lane groups from 169
    assert any(c["j"] == 168 and c["live"] == 16 for c in run["cases"])
    assert any(c["j"] == 169 and c["live"] == 16 and c["running"] > 0 for c in run["cases"])

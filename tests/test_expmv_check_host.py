"""tests/native/expmv_check without a GPU: `--host` runs every case with the
launcher replaced by a plain fp64 loop written from kt_launch.h's contract (the
ExpmvState bookkeeping included), so an honest implementation is shown to meet
every bound, every "exact" case to be exact and the stage reference to hold
the stops it must; `--host --mutate=NAME` plants one defect in that stand-in,
which the program must report in the defect's group and in no other.  `--count`
lists the forms of launch_expmv_step the enumeration reaches: a width or flag
set added to the launcher without a case here changes a number below.  Built
by __graft_entry__.build()."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "expmv_check", "expmv_check")
GROUPS = ["begin", "unfused", "step", "stage", "setup"]
# defect -> (the group that must report it, names of which one at least must be
# among the failed cases)
STEP = {"exact", "bounded", "fallback", "task_order"}
MUTATIONS = {
    "short_skip_deg16": ("step", STEP),
    "med_skip_deg17": ("step", STEP),
    "long_drop_last_chain_entry": ("step", STEP),
    "heavy_row_twice": ("step", {"exact", "bounded", "task_order"}),
    "mu_ignored_long": ("step", STEP),
    "weights_ignored": ("step", {"exact", "bounded"}),
    "pad_written_rows": ("step", {"exact", "bounded"}),
    "f_pad_written": ("step", {"exact", "bounded"}),
    "stop_strict_less": ("stage", {"stop2_sharp_hi_equal", "stop3_sharp_hi_equal", "stop4_sharp_hi_equal",
                                   "stop5_sharp_hi_equal"}),
    "c1_wrong_parity": ("stage", None),
    "stale_slot_set": ("stage", None),
    "mv_counts_stopped_term": ("stage", None),
    "stopped_term_writes": ("stage", None),
    "hflag_before_stop": ("stage", None),
    "begin_keeps_set1": ("begin", {"begin"}),
    "scales_nan_as_positive": ("setup", {"exact", "bounded"}),
    "pair_start_same_sign": ("setup", {"exact"}),
}


def run_check(*args):
    assert os.path.exists(CHECK), "tests/native/expmv_check/expmv_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    return r, json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def host_run():
    return run_check("--host")


@pytest.fixture(scope="module")
def count_run():
    r, out = run_check("--count")
    assert r.returncode == 0
    return out


@pytest.fixture(scope="module")
def counts(count_run):
    return {g: count_run["groups"][g]["cases"] for g in GROUPS}


def test_every_group_has_cases(counts):
    for g in GROUPS:
        assert counts[g] > 0, counts


def test_every_step_form_is_enumerated(count_run):
    """The form table of --count: 6 widths x unit / weighted x forms 0 .. 3 x mu
    zero / non-zero, every row with a case, reaching exactly the 72 instances
    of k_expmv_step (6 x 2 x fused / split) and k_expmv_rows (6 x 4 flag sets x
    CHECK on / off), plus the fallback of forms 2 and 3 without task lists."""
    rows = count_run["forms"]["expmv_step"]
    assert len(rows) == 6 * 2 * 4 * 2
    assert len({(f["P"], f["unit"], f["form"], f["mu0"]) for f in rows}) == len(rows)
    for f in rows:
        assert f["cases"] > 0, f
        assert f["reaches"].startswith(("k_expmv_step<%d, " % f["P"], "k_expmv_rows<%d, " % f["P"])), f
    reached = {f["reaches"] for f in rows}
    assert len(reached) == 72, sorted(reached)
    assert len({r for r in reached if r.startswith("k_expmv_step<")}) == 24
    assert len({r for r in reached if r.startswith("k_expmv_rows<")}) == 48
    fb = count_run["forms"]["fallback"]
    assert len(fb) == 1 and fb[0]["cases"] > 0, fb


@pytest.mark.parametrize("group", GROUPS)
def test_host_standin_passes(host_run, counts, group):
    """The fp64 host loops meet every bound and every exact comparison; no
    case of the enumeration is left out.  The stage group's coverage case
    holds the reference to its stops at terms 2, 3 and >= 4, the stage without
    stop, the sharp pairs (one with equality) and the two-stage run."""
    r, out = host_run
    assert out["mode"] == "host"
    g = out["groups"][group]
    print(group, "cases", g["cases"], "max_ratio", g["max_ratio"])
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group]
    assert 0.0 <= g["max_ratio"] <= 1.0
    assert r.returncode == 0, (r.returncode, out["expmv_check"])


def test_host_deep_shape_trips(host_run):
    """The deep shape (sized from the grid of forms 2 and 3) gives every loop
    of k_expmv_rows at least three trips, at P = 16 and at P = 1."""
    _, out = host_run
    assert sorted(t["P"] for t in out["trips"]) == [1, 16]
    for t in out["trips"]:
        assert min(t["heavy"], t["long"], t["medium"], t["short"]) >= 3, t


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_detected(name):
    """One planted defect: non-zero exit, failures in its group and in no
    other, among them the cases aimed at it.  Every group runs, so "no other
    group" is shown, not assumed (--small keeps the widths 1, 4 and 16 and
    leaves the deep shape out)."""
    group, expect = MUTATIONS[name]
    r, out = run_check("--host", "--small", f"--mutate={name}")
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert out["mutate"] == name
    g = out["groups"][group]
    assert g["failed_count"] > 0 and g["failed"], g
    failed = [grp for grp in GROUPS if out["groups"][grp]["failed_count"]]
    assert failed == [group], failed
    for f in g["failed"]:
        assert {"name", "shape", "what", "index", "got", "expected", "bound"} <= set(f), f
    names = {f["name"] for f in g["failed"]}
    if expect is not None:
        assert names & expect, (names, expect)
    assert "coverage" not in names, names


def test_unknown_mutation_is_refused():
    assert os.path.exists(CHECK), "tests/native/expmv_check/expmv_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--host", "--mutate=no_such_defect"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)


def test_mutation_needs_host():
    assert os.path.exists(CHECK), "tests/native/expmv_check/expmv_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--mutate=stop_strict_less"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)

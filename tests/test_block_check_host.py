"""tests/native/block_check without a GPU: `--host` runs every case with the
launcher replaced by a plain fp64 loop, so an honest implementation is shown
to meet every bound and every "exact" case to be exact; `--host --mutate=NAME`
plants one defect in that stand-in, which the program must report in the
defect's group.  Built by __graft_entry__.build()."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "block_check", "block_check")
GROUPS = ["gram", "combine", "chol_rinv", "fro_colmax_scale", "colbatch", "streaming"]
# defect -> (the group that must report it, the cases that must be among the failures)
MUTATIONS = {
    "gram_drop_last_row": ("gram", {"exact", "bounded"}),
    "gram_skip_col32": ("gram", {"exact", "bounded"}),
    "gram_drop_slab": ("gram", {"exact", "bounded"}),
    "combine_ignore_beta": ("combine", {"separate_exact", "separate_bounded"}),
    "combine_inplace_rowwise": ("combine", {"inplace_exact", "inplace_bounded"}),
    "chol_no_shift": ("chol_rinv", {"normal_shift"}),
    "chol_below_diag": ("chol_rinv", {"integer", "normal"}),
    "col_dots_ignore_r_lo": ("colbatch", {"col_dots_exact", "col_dots_bounded"}),
    "absmax_tie_largest": ("streaming", {"absmax_idx_tie_in_wave", "absmax_idx_tie_far_apart"}),
    "normest1_sign0": ("streaming", {"normest1_y_exact", "normest1_y_bounded"}),
}


def run_check(*args):
    assert os.path.exists(CHECK), "tests/native/block_check/block_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    return r, json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def host_run():
    return run_check("--host")


@pytest.fixture(scope="module")
def counts():
    r, out = run_check("--count")
    assert r.returncode == 0
    return {g: out["groups"][g]["cases"] for g in GROUPS}


def test_every_group_has_cases(counts):
    for g in GROUPS:
        assert counts[g] > 0, counts


@pytest.mark.parametrize("group", GROUPS)
def test_host_standin_passes(host_run, counts, group):
    """The fp64 host loops meet every bound and every exact comparison; no
    case of the enumeration is left out."""
    r, out = host_run
    assert out["mode"] == "host"
    g = out["groups"][group]
    print(group, "cases", g["cases"])
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group]
    assert r.returncode == 0, (r.returncode, out["block_check"])


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_detected(name):
    """One planted defect: non-zero exit, failures in its group, among them
    the cases aimed at it.  (--group / --small only shorten the run: a defect
    sits in one group's stand-in, and none needs gram's n >= 8192.)"""
    group, expect = MUTATIONS[name]
    r, out = run_check("--host", "--small", f"--group={group}", f"--mutate={name}")
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert out["mutate"] == name
    g = out["groups"][group]
    assert g["failed_count"] > 0 and g["failed"], g
    failed = [grp for grp in GROUPS if out["groups"][grp]["failed_count"]]
    assert failed == [group], failed
    for f in g["failed"]:
        assert {"name", "shape", "what", "index", "got", "expected", "bound"} <= set(f), f
    names = {f["name"] for f in g["failed"]}
    assert names & expect, (names, expect)


def test_unknown_mutation_is_refused():
    assert os.path.exists(CHECK), "tests/native/block_check/block_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--host", "--mutate=no_such_defect"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)

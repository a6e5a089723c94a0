"""tests/native/diag_check without a GPU: `--host` runs every case with the
launcher replaced by a plain fp64 loop written from kt_launch.h's contract, so
an honest implementation is shown to meet every bound and every "exact" case
to be exact; `--host --mutate=NAME` plants one defect in that stand-in, which
the program must report in the defect's group and in no other.  `--count`
lists the (P, KP) forms the enumeration reaches and the values of the two grid
functions: a width added to kt_diag.hip's by_width / by_defl without a case
here changes a number below.  Built by __graft_entry__.build()."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "diag_check", "diag_check")
GROUPS = ["qtz_sum", "start", "combine", "finish", "entries", "d0", "adapt_stream", "contract"]
# the (P, KP) pairs each launcher's switches in kt_diag.hip admit: P in {1, 2, 4,
# 8, 16}; KP in {1, 4, 16}, and 0 where the launcher has a KP == 0 branch
FORMS = {"diag_qtz": 15, "diag_start": 20, "diag_combine": 20, "diag_combine_y": 5, "diag_finish": 15,
         "entries_accumulate": 20}
# (n, P, diag_grid): n = 0 gives 1, the ceil over 256 / max(P / 2, 1) rows, the cap 1024
DIAG_GRID = [[0, 1, 1], [0, 16, 1], [1, 1, 1], [256, 1, 1], [257, 1, 2], [256, 2, 1], [257, 2, 2], [129, 4, 2],
             [65, 8, 2], [32, 16, 1], [33, 16, 2], [50000, 16, 1024], [262144, 1, 1024], [262145, 1, 1024],
             [32736, 16, 1023], [32768, 16, 1024], [32769, 16, 1024], [2000000000, 16, 1024]]
# (npairs, P, entries_grid): the same rule over pairs, the cap 4096
ENTRIES_GRID = [[0, 1, 1], [0, 16, 1], [1, 16, 1], [32, 16, 1], [33, 16, 2], [257, 2, 2], [129, 4, 2], [65, 8, 2],
                [131040, 16, 4095], [131072, 16, 4096], [131073, 16, 4096], [1048576, 1, 4096], [1048577, 1, 4096],
                [5000000000, 16, 4096]]
# defect -> (the group that must report it, the cases that must be among the
# failures, a word that a failing case's shape must carry or None)
MUTATIONS = {
    "qtz_drop_tail_row": ("qtz_sum", {"exact", "bounded"}, None),
    "qtz_dead_col_live": ("qtz_sum", {"exact", "bounded"}, None),
    "sum_parts_skip_64": ("qtz_sum", {"sum_parts_exact", "sum_parts_bounded"}, "nparts="),
    "start_no_projection": ("start", {"exact", "bounded"}, None),
    "start_norm_from_z": ("start", {"exact", "bounded"}, None),
    "combine_ignore_depth": ("combine", {"exact", "bounded"}, "depth="),
    "combine_pair_depth": ("combine", {"exact", "bounded"}, "depth="),
    "combine_dsum_by_row": ("combine", {"exact", "bounded"}, "KP=0"),
    "combine_overwrite": ("combine", {"exact", "bounded"}, "KP=0"),
    "finish_sign_by_row": ("finish", {"exact", "bounded"}, "perm=1"),
    "entries_swap_signs": ("entries", {"exact", "bounded"}, "accumulate"),
    "entries_dead_lane_adds": ("entries", {"exact", "bounded"}, "accumulate"),
    "e0_half_missing": ("entries", {"exact", "bounded"}, "e0"),
    "d0_row_major_H": ("d0", {"exact", "bounded"}, None),
    "wsum_tab_chunk_off_by_one": ("adapt_stream", {"exact", "bounded"}, "weighted_sum_tab"),
    "unit_start_oob_writes": ("adapt_stream", {"exact"}, "out_of_range"),
}


def run_check(*args):
    assert os.path.exists(CHECK), "tests/native/diag_check/diag_check is not built (__graft_entry__.build())"
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


def test_every_launcher_form_is_enumerated(count_run):
    """The form table of --count: as many (P, KP) pairs per launcher as its
    switches in kt_diag.hip admit, each with the template it reaches."""
    forms = count_run["forms"]
    assert {k: len(v) for k, v in forms.items()} == FORMS
    for rows in forms.values():
        assert len({(f["P"], f["KP"]) for f in rows}) == len(rows)
        for f in rows:
            assert f["reaches"].startswith(("k_diag_", "k_entries_")), f
            assert f"<{f['P']}, {f['KP']}" in f["reaches"], f


def test_grid_functions(count_run):
    """diag_grid and entries_grid (host functions of kt_diag.o): 1 at n = 0,
    the ceil, the caps 1024 and 4096."""
    assert count_run["grids"]["diag_grid"] == DIAG_GRID
    assert count_run["grids"]["entries_grid"] == ENTRIES_GRID


@pytest.mark.parametrize("group", GROUPS)
def test_host_standin_passes(host_run, counts, group):
    """The fp64 host loops meet every bound and every exact comparison; no
    case of the enumeration is left out."""
    r, out = host_run
    assert out["mode"] == "host"
    g = out["groups"][group]
    print(group, "cases", g["cases"], "max_ratio", g["max_ratio"])
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group]
    assert 0.0 <= g["max_ratio"] <= 1.0
    assert r.returncode == 0, (r.returncode, out["diag_check"])


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_detected(name):
    """One planted defect: non-zero exit, failures in its group and in no
    other, among them the cases aimed at it.  Every group runs, so "no other
    group" is shown, not assumed (--small only keeps the widths 1, 4 and 16)."""
    group, expect, word = MUTATIONS[name]
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
    assert names & expect, (names, expect)
    if word is not None:
        assert all(word in f["shape"] for f in g["failed"]), [f["shape"] for f in g["failed"]]


def test_unknown_mutation_is_refused():
    assert os.path.exists(CHECK), "tests/native/diag_check/diag_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--host", "--mutate=no_such_defect"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)


def test_mutation_needs_host():
    assert os.path.exists(CHECK), "tests/native/diag_check/diag_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--mutate=combine_overwrite"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)

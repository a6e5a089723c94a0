"""tests/native/pairs_check without a GPU: `--host` runs every case with the
launcher replaced by a plain fp64 stand-in written from kt_launch.h's contract
(CGS2 + Householder, cyclic Jacobi, the lag-2 stop, a plain CSR edit), so an
honest implementation is shown to meet every bound, every "exact" case to be
exact, and the `whole` cases to meet their keep-conditions (min(R11, R22) >=
1e-3 rho(A) wherever a record enters a projection, every stop decision a factor
4 from tol); `--host --mutate=NAME` plants one defect in that stand-in, which
the program must report in the defect's group and in no other.  `--count` lists
the forms the enumeration reaches: the three launch_pair_eig forms with their
depths and the k_pair_reg<rows, csr> instance and `spec` value of every graph
of the `whole` group (kt::pair_reg_form).  Built by __graft_entry__.build()."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "pairs_check", "pairs_check")
GROUPS = ["select", "orth", "eig", "edit", "whole"]
# launch_pair_eig's three branches and the depths at the edges of xm_waves,
# group_lanes and the 64-eigenvalues-at-a-time loop
EIG_FORMS = {
    "blk": ("k_pair_eig_blk", [1, 2, 3, 8, 16, 17, 28, 29, 32, 33, 64, 65, 129]),
    "wave": ("k_pair_eig_wave<1,4>", [1, 2, 3, 8, 16, 17, 28]),
    "one": ("k_pair_eig", [29, 33]),
}
# graph -> (n, applies, rows, csr, spec, has_long): what pair_reg_plan decides
# for the graphs of the `whole` group.  A change of the LDS layout or of the
# plan shows here first.  Every R and every csr value is reached, not every
# <R, CSR> pair: csr 0 needs the nnz that only fits beside n = 4096 (R = 8).
REG_FORMS = {
    "n2": (2, 1, 2, 2, 1, 0),
    "n3": (3, 1, 2, 1, 1, 0),
    "n511": (511, 1, 2, 2, 1, 1),
    "n512": (512, 1, 2, 1, 1, 0),
    "n513": (513, 1, 2, 1, 1, 1),
    "n1024": (1024, 1, 2, 2, 1, 0),
    "n1025": (1025, 1, 4, 2, 1, 1),
    "n2049": (2049, 1, 6, 1, 1, 1),
    "n3073": (3073, 1, 7, 1, 1, 0),
    "n3585": (3585, 1, 8, 1, 0, 1),
    "n4096a": (4096, 1, 8, 2, 0, 0),
    "n4096b": (4096, 1, 8, 1, 0, 1),
    "n4096c": (4096, 1, 8, 0, 1, 1),
    "n4096d": (4096, 1, 8, 0, 1, 1),
    "n4097": (4097, 0, 0, 0, 0, 1),
}
MID_GRAPHS = ["n511", "n513", "n1024", "n1025", "n2049", "n3073", "n4096a"]
# defect -> (the group that must report it, checks ("what") of which one must
# be among the failures, a word that every failing case's shape must carry or None)
MUTATIONS = {
    "orth_drop_last_row": ("orth", {"R11", "R11 = -5", "Q not written", "Q (rank-deficient)", "W - [p c] h - Q R"}, None),
    "orth_row0_in_s1": ("orth", {"R11", "R11 = -5", "R (rank-deficient)"}, None),
    "orth_row1_in_s2": ("orth", {"R22", "|R22|", "R (rank-deficient)"}, None),
    "orth_no_tau0_branch": ("orth", {"R (rank-deficient)", "Q (rank-deficient)", "R22"}, None),
    "orth_partials_stop_at_64": ("orth", {"R11", "R11 = -5", "h", "h = selected entries of W"}, "n=1100"),
    "orth_store_invalid_lane": ("orth", {"sentinel column"}, None),
    "orth_ignores_skip": ("orth", {"W with skip -> 0", "hr with skip -> 0"}, "skip=2"),
    "eig_no_symmetrise": ("eig", {"Xm (asym)"}, None),
    "eig_cm_on_both": ("eig", {"Xm (lanczos)", "Xm (cluster)", "Xm (midzero)", "Xm (asym)", "Xm (wide)", "Xm (zerolead)"}, None),
    "eig_drop_last_eigenvalue": ("eig", {"Xm (lanczos)", "Xm (cluster)", "Xm (midzero)", "Xm (asym)", "Xm (wide)", "Xm (zerolead)"}, None),
    "eig_lucky_r22_only": ("eig", {"lucky"}, None),
    "eig_stop_lag1": ("eig", {"X0 <- X1", "X0 on stop", "done"}, None),
    "eig_done_not_frozen": ("eig", {"done candidate changed"}, None),
    "active_counts_done": ("eig", {"active[0]"}, None),
    "edit_tie_takes_last": ("edit", {"sel", "Ti", "Tj"}, "ties="),
    "edit_nan_wins": ("edit", {"sel", "selv", "Ti", "Tj"}, None),
    "edit_rp_shift_from_r1": ("edit", {"rp2"}, None),
    "edit_keeps_shortened_long_row": ("edit", {"lr2", "dyn2"}, "long"),
    "edit_ranking_last_entry_lost": ("edit", {"Ti", "Tj"}, None),
    "whole_long_rows_skipped": ("whole", {"Xm", "iter"}, None),
    "whole_cm_without_r12": ("whole", {"Xm", "iter"}, None),
}


def run_check(*args):
    assert os.path.exists(CHECK), "tests/native/pairs_check/pairs_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=180)
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


def test_every_group_has_cases(count_run, counts):
    assert list(count_run["groups"]) == GROUPS
    for g in GROUPS:
        assert counts[g] > 0, counts


def test_pair_eig_forms_are_enumerated(count_run):
    forms = {f["form"]: (f["reaches"], f["depths"]) for f in count_run["forms"]["pair_eig"]}
    assert forms == EIG_FORMS


def test_pair_reg_forms_are_pinned(count_run):
    """The (rows, csr, spec, has_long) each graph of the `whole` group reaches:
    every R in {2, 4, 6, 7, 8}, the fall-back past 8 * 512 rows, csr 0, 1, 2
    and spec 0, 1, n_long 0, a few, and more than kRegLongCap."""
    rows = count_run["forms"]["pair_reg"]
    got = {f["graph"]: (f["n"], f["applies"], f["rows"], f["csr"], f["spec"], f["has_long"]) for f in rows}
    assert got == REG_FORMS
    assert {f["rows"] for f in rows} == {0, 2, 4, 6, 7, 8}
    assert {f["csr"] for f in rows if f["applies"]} == {0, 1, 2}
    assert {f["spec"] for f in rows if f["applies"]} == {0, 1}
    n_long = sorted({f["n_long"] for f in rows})
    assert n_long[0] == 0 and 3 in n_long and n_long[-1] > 256, n_long
    assert {f["unit"] for f in rows} == {0, 1}
    # the graphs with a mid-run stop (a tolerance that stops a candidate at a
    # step 4 <= J < it with every decision a factor 4 away); the others have
    # no `mid` cases
    assert [f["graph"] for f in rows if f["mid"]] == MID_GRAPHS
    assert {f["rows"] for f in rows if f["mid"]} == {2, 4, 6, 7, 8}


@pytest.mark.parametrize("group", GROUPS)
def test_host_standin_passes(host_run, counts, group):
    """The fp64 stand-ins meet every bound and every exact comparison (for
    `whole`: and every keep-condition); no case of the enumeration is left out."""
    r, out = host_run
    assert out["mode"] == "host"
    g = out["groups"][group]
    print(group, "cases", g["cases"], "max_ratio", g["max_ratio"])
    assert g["failed"] == [] and g["failed_count"] == 0, g["failed"]
    assert g["cases"] == counts[group]
    assert 0.0 <= g["max_ratio"] <= 1.0
    assert r.returncode == 0, (r.returncode, out["pairs_check"])


def test_accuracy_constants_follow_their_rule(host_run):
    """K_eig = max(18, 4 r_host) rounded up to a power of two and K_whole =
    max(K_eig, 8 r_whole), with r_host / r_whole the stand-in's own measured
    errors (printed on stderr by --host): the constants in the program are the
    rule's values for what this build measures, not numbers tuned to a kernel."""
    import math
    import re

    r, _ = host_run
    m = re.search(r"r_host = ([0-9.eE+-]+) \(K_eig = ([0-9.eE+-]+)\)", r.stderr)
    w = re.search(r"r_whole = ([0-9.eE+-]+) \(K_whole = ([0-9.eE+-]+)\)", r.stderr)
    assert m and w, r.stderr
    r_host, k_eig = float(m.group(1)), float(m.group(2))
    r_whole, k_whole = float(w.group(1)), float(w.group(2))
    assert r_host > 0.0 and r_whole > 0.0
    assert k_eig == 2.0 ** math.ceil(math.log2(max(18.0, 4.0 * r_host))), (r_host, k_eig)
    assert k_whole == max(k_eig, 8.0 * r_whole), (r_whole, k_whole)


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_detected(name):
    """One planted defect: non-zero exit, failures in its group and in no
    other, among them a check aimed at it.  Every group runs, so "no other
    group" is shown, not assumed (--small only thins the shapes).  One
    limit: the `whole` stand-in reuses the orth stand-in with every defect
    but the whole_* ones switched off (the launchers are separate kernels, so
    a defect of launch_pairs_orth is not one of launch_pair_fused); for the
    seven orth_* defects "not in `whole`" therefore holds by construction."""
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
    whats = {f["what"].replace(" (second run)", "") for f in g["failed"]}
    assert whats & expect, (whats, expect)
    if word is not None:
        assert all(word in f["shape"] for f in g["failed"]), [f["shape"] for f in g["failed"]]


def test_unknown_mutation_is_refused():
    assert os.path.exists(CHECK), "tests/native/pairs_check/pairs_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--host", "--mutate=no_such_defect"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)


def test_mutation_needs_host():
    assert os.path.exists(CHECK), "tests/native/pairs_check/pairs_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--mutate=eig_stop_lag1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)

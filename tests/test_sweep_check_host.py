"""tests/native/sweep_check without a GPU: `--host` runs every case with the
launcher replaced by a plain fp64 loop written from kt_launch.h's contract, so
an honest implementation is shown to meet every bound and every "exact" case
to be exact; `--host --mutate=NAME` plants one defect in that stand-in, which
the program must report in the defect's group and in no other.  `--count`
lists the launcher forms the enumeration reaches: a form added to a launcher
without a case here changes a number below.  Built by __graft_entry__.build()."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "sweep_check", "sweep_check")
GROUPS = ["probes", "spmm_dot", "spmm_block", "lanczos_pass", "lanczos_start", "lanczos_first", "quadform", "coef",
          "update", "contract"]
# the branches of each launcher's form switch in kt_kernels.hip (launch_spmm_lanczos:
# 3 gated + 3 int16 + 4 basis-forming + 6 plain)
FORMS = {"spmm_dot": 10, "spmm_block": 4, "lanczos_pass": 16, "lanczos_start": 7, "lanczos_first": 4, "quadform": 4}
# defect -> (the group that must report it, the cases that must be among the
# failures, a word that a failing case's shape must carry or None)
MUTATIONS = {
    "dot_drop_last_mod4": ("spmm_dot", {"exact", "bounded"}, None),
    "pass_skip_long_plus1": ("lanczos_pass", {"exact", "bounded"}, "A/"),
    "start_val_shift": ("lanczos_start", {"exact"}, None),
    "pass_no_yold": ("lanczos_pass", {"exact", "bounded"}, "yold=1"),
    "quad_no_diag": ("quadform", {"exact", "bounded"}, None),
    "quad_prefix_off_by_one": ("quadform", {"exact", "bounded"}, None),
    "block_drop_last_chunk": ("spmm_block", {"exact", "bounded"}, "A/"),
    "ycoef_guard_overwrite": ("coef", {"ycoef_guard_min", "ycoef_nan_sticks"}, None),
    "reduce_round_down_64": ("coef", {"reduce_norm_exact", "reduce_coef_cgs2_exact", "reduce_ycoef_exact"}, None),
    "start_sign_bit_p1": ("lanczos_start", {"exact", "bounded"}, None),
    "vb_write_bcols": ("lanczos_pass", {"exact", "bounded"}, "form=Vn:"),
    "quad_vb_write_bcols": ("quadform", {"exact", "bounded"}, "form=Vn:"),
    "first_ignore_alpha": ("lanczos_first", {"exact", "bounded"}, None),
    "update_reads_uprev_on_first": ("update", {"exact", "bounded"}, "first=1"),
    "probes_ignore_perm": ("probes", {"rademacher_and_signs"}, "perm=1"),
}


def run_check(*args):
    assert os.path.exists(CHECK), "tests/native/sweep_check/sweep_check is not built (__graft_entry__.build())"
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
    """The form table of --count: as many forms per launcher as its switch in
    kt_kernels.hip has branches, each with the template it reaches."""
    forms = count_run["forms"]
    assert {k: len(v) for k, v in forms.items()} == FORMS
    for rows in forms.values():
        assert len({(f["form"]) for f in rows}) == len(rows)
        for f in rows:
            assert f["reaches"].startswith("k_spmm_"), f


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
    assert r.returncode == 0, (r.returncode, out["sweep_check"])


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_detected(name):
    """One planted defect: non-zero exit, failures in its group and in no
    other, among them the cases aimed at it.  Every group runs, so "no other
    group" is shown, not assumed (--small only keeps the widths 1, 4 and 32)."""
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
    assert os.path.exists(CHECK), "tests/native/sweep_check/sweep_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--host", "--mutate=no_such_defect"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)


def test_mutation_needs_host():
    assert os.path.exists(CHECK), "tests/native/sweep_check/sweep_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK, "--mutate=pass_no_yold"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)

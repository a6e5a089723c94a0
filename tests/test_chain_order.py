"""The chained row order of the relabelled CSR copy (csrc/kt_order.h
chain_order) on the host, without a device:
tests/native/chain_order/chain_order_check (built by __graft_entry__.build())
links the header into a program of its own and checks, on a path, a star, a
cycle with chords, heavy-tailed graphs with and without loops, a graph with
isolated rows, n = 0 and n = 1, that new2old is a bijection, that degree
classes are non-increasing along it, that an equal input in other storage
gives the same order, that long rows sit at their hub_order positions, that
the run property holds, and that the order equals an independent
implementation of the rule."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "chain_order", "chain_order_check")


def test_chain_order_properties_on_the_host():
    assert os.path.exists(CHECK), "tests/native/chain_order/chain_order_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    bad = [g for g in out["graphs"] if g["result"] != "ok"]
    assert not bad, bad
    assert r.returncode == 0 and out["failed"] == 0
    by = {(g["name"], g["long_thresh"]): g for g in out["graphs"]}
    names = {k[0] for k in by}
    assert {"path_301", "star_300", "cycle_chords_211", "heavy_tail_20k", "heavy_tail_loops_6k",
            "isolated_rows_257", "empty_0", "single_1"} <= names
    assert {k[1] for k in by} == {64, 8}
    # the cases are what they claim to be: long rows, more rows than the hub
    # ranks, and rows that were in fact chained
    ht = by[("heavy_tail_20k", 64)]
    assert ht["long_rows"] > 0 and ht["n"] > 4096 and ht["chained"] > 0
    assert by[("heavy_tail_loops_6k", 8)]["long_rows"] > 0
    # a path is one class but for its two ends: nearly every row continues a run
    assert by[("path_301", 64)]["chained"] >= 290
    assert by[("cycle_chords_211", 64)]["chained"] > 0
    assert by[("empty_0", 64)]["n"] == 0 and by[("single_1", 64)]["n"] == 1

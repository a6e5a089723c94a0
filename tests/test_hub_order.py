"""The relabelled CSR copy's row order (csrc/kt_order.h) on the host, without
a device: tests/native/hub_order/hub_order_check (built by
__graft_entry__.build()) links the header into a program of its own and
checks, on heavy-tailed graphs, a star, a path and graphs with empty rows,
that new2old is a bijection, that degree classes are non-increasing along it,
that equal inputs give equal orders, and that the order equals an independent
comparison sort by (class descending, neighbour key ascending, original
index)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "hub_order", "hub_order_check")


def test_hub_order_properties_on_the_host():
    assert os.path.exists(CHECK), "tests/native/hub_order/hub_order_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    bad = [g for g in out["graphs"] if g["result"] != "ok"]
    assert not bad, bad
    assert r.returncode == 0 and out["failed"] == 0
    names = {g["name"] for g in out["graphs"]}
    assert {"heavy_tail_20k", "star_300", "path_301", "isolated_rows_257"} <= names
    assert {g["long_thresh"] for g in out["graphs"]} == {64, 8}

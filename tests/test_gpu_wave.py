"""The wave exchanges of kt_wave.h (DPP / permlane forms) against the
__shfl_xor butterflies they replace: tests/native/wave_check, built by
__graft_entry__.build()."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native", "wave_check", "wave_check")


@pytest.mark.gpu
def test_wave_helpers_match_shfl_xor_butterflies():
    """Every helper agrees with the shuffle form on 4,096 waves of random bits
    (sums and moves by bits, min / max by value, group_min_i for every group
    size); the program's mask names the helper that does not."""
    assert os.path.exists(CHECK), "tests/native/wave_check/wave_check is not built (__graft_entry__.build())"
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mismatch_mask"] == 0, out
    assert out["lanes"] == 64 * 4096

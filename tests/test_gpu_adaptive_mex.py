"""GPU: the MEX shim's trace_exp(A, 'auto') (kt_mex.cpp, KT_ENTRY_TRACE_EXP)
through the stand-in MEX runtime of tests/mexstub, as tests/test_mex_exec.py
runs the other forms: bit for bit the ctypes value, and the depth-cap warning
when the optional third argument forces the cap low."""
import pytest

from conftest import load_graph
from test_mex_exec import Mex, MexRaised

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mex():
    M = Mex()
    yield M
    M.rt.stub_run_atexit()


def test_trace_exp_auto_matches_ctypes_and_warns_at_the_cap(mex):
    import krylov_robustness_amd as kra
    mex.rt.stub_clear()
    A = load_graph("oregon_A0")
    tr, = mex.call("TRACE_EXP", 1, A, "auto")
    assert tr == kra.trace_exp(A, "lanczos-auto", seed=0)
    assert mex.warnings() == []
    assert mex.call("TRACE_EXP", 1, A, "auto", 128.0)[0] == tr
    # the default and 'expmv' forms are what they were
    assert mex.call("TRACE_EXP", 1, A)[0] == kra.trace_exp(A, "lanczos", m=30, seed=0)
    assert mex.call("TRACE_EXP", 1, A, "expmv")[0] == kra.trace_exp(A, "expmv", seed=0)
    assert mex.warnings() == []
    # a cap of 9 is reached: the estimate comes back with the warning
    trc, = mex.call("TRACE_EXP", 1, A, "auto", 9.0)
    assert trc == kra.trace_exp(A, "lanczos-auto", m=9, seed=0)
    assert ("TRACE_EXP:depthcap", "TRACE_EXP:: Lanczos depth cap reached") in mex.warnings()
    with pytest.raises(MexRaised, match="'auto' only"):
        mex.call("TRACE_EXP", 1, A, "lanczos", 9.0)
    with pytest.raises(MexRaised, match="at most 256"):
        mex.call("TRACE_EXP", 1, A, "auto", 300.0)

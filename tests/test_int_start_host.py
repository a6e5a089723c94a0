"""CPU: when a y-form sweep may carry y_0 as int16 row sums
(kt_host_int0_applies, the rule kt_slq_trace applies per call; pure host
code).  On a unit-weight matrix a row's start-pass sum is an integer of
magnitude <= the row's length, so the bound is int16's largest value."""
import ctypes as C

import pytest


def applies(unit, max_row, m):
    from krylov_robustness_amd import _lib
    out = C.c_int(-1)
    assert _lib.load().kt_host_int0_applies(int(unit), int(max_row), int(m), C.byref(out)) == _lib.KT_OK
    return out.value


@pytest.mark.parametrize("max_row", [0, 1, 64, 65, 32766, 32767])
@pytest.mark.parametrize("m", [3, 4, 30, 256])
def test_unit_weight_rows_within_int16(max_row, m):
    assert applies(1, max_row, m) == 1


@pytest.mark.parametrize("max_row", [32768, 65535, 65536, 2 ** 31 - 1, 2 ** 40])
def test_a_row_longer_than_int16_max_keeps_fp64(max_row):
    assert applies(1, max_row, 30) == 0


@pytest.mark.parametrize("max_row", [1, 64, 32767, 32768])
def test_weighted_matrix_keeps_fp64(max_row):
    assert applies(0, max_row, 30) == 0


@pytest.mark.parametrize("m", [1, 2])
def test_sweeps_without_an_ordinary_pass_keep_fp64(m):
    """m = 1 is the start pass alone; at m = 2 the only pass after it is the
    half-gather last pass, which reads y_0 in fp64."""
    assert applies(1, 10, m) == 0


def test_null_result_is_an_argument_error():
    from krylov_robustness_amd import _lib
    assert _lib.load().kt_host_int0_applies(1, 10, 30, None) == _lib.KT_ERR_ARG

"""Host logic of the native logistic-regression solvers (csrc/bhg_logreg_solve.hip): which form a shape takes, and argument errors
that must be refused before anything touches a device.  No GPU."""
import ctypes

import pytest

from betty_amd import _native
from betty_amd.backend import LOGREG_FORM_AUTO, LOGREG_FORM_SINGLE, LOGREG_FORM_STRIPS, logreg_solve_plan


def test_cfg1_plans_single():
    assert logreg_solve_plan(500, 100).startswith("single")
    assert "1 launch per solve" in logreg_solve_plan(500, 100)


@pytest.mark.parametrize("n,d", [(513, 1025), (2048, 4096)])
def test_wide_or_large_problems_plan_strips(n, d):
    line = logreg_solve_plan(n, d)
    assert line.startswith("strips G=")
    G = int(line.split("G=")[1].split(":")[0])
    assert 1 <= G <= 512
    assert "3 launches per cg iteration" in line and "2 per neumann iteration" in line


@pytest.mark.parametrize("n,d", [(1, 1), (255, 1024), (260, 1000), (1 << 18, 1)])
def test_single_admits_every_small_shape(n, d):
    """d <= 1024 and n * d <= 2^18"""
    assert logreg_solve_plan(n, d, LOGREG_FORM_SINGLE).startswith("single")
    assert logreg_solve_plan(n, d, LOGREG_FORM_STRIPS).startswith("strips")


def test_strip_count_is_taken_as_given():
    assert logreg_solve_plan(37, 5, LOGREG_FORM_STRIPS, 7).startswith("strips G=7:")
    assert logreg_solve_plan(3, 2, LOGREG_FORM_STRIPS, 8).startswith("strips G=8:")
    assert logreg_solve_plan(1 << 20, 4096, LOGREG_FORM_AUTO).startswith("strips G=512:")


def test_beyond_4096_columns_plans_none():
    assert logreg_solve_plan(64, 4097) == "none"
    assert int(_native.load().bhg_logreg_solve_ws_bytes(64, 4097)) == 0
    assert int(_native.load().bhg_logreg_solve_ws_bytes(64, 4096)) > 0


def test_a_forced_form_the_shape_does_not_admit_is_an_error():
    with pytest.raises(_native.NativeLibraryError, match="single form"):
        logreg_solve_plan(2048, 4096, LOGREG_FORM_SINGLE)
    with pytest.raises(_native.NativeLibraryError, match="strips form"):
        logreg_solve_plan(64, 4097, LOGREG_FORM_STRIPS)
    with pytest.raises(_native.NativeLibraryError):
        logreg_solve_plan(64, 64, 3)
    with pytest.raises(_native.NativeLibraryError, match="strips"):
        logreg_solve_plan(64, 64, LOGREG_FORM_STRIPS, 513)


@pytest.mark.parametrize("solve", ["bhg_logreg_cg_solve", "bhg_logreg_neumann_solve"])
def test_argument_errors_return_a_code_without_touching_a_device(solve):
    """NULL pointers, n <= 0, K < 0, d beyond every form, a forced form that does not fit: refused by the host checks (no GPU is needed:
    the pointers below are not even device pointers)."""
    lib = _native.load()
    fn = getattr(lib, solve)
    host = (ctypes.c_float * 64)()
    q = ctypes.addressof(host)
    assert fn(None, q, q, q, q, None, q, 4, 4, 1, 1.0, -1.0, 0, 0, None) == -1 and b"NULL" in lib.bhg_last_error()
    assert fn(q, q, q, q, None, None, q, 4, 4, 1, 1.0, -1.0, 0, 0, None) == -1 and b"NULL" in lib.bhg_last_error()
    assert fn(q, q, q, q, q, None, None, 4, 4, 1, 1.0, -1.0, 0, 0, None) == -1 and b"NULL" in lib.bhg_last_error()
    assert fn(q, q, q, q, q, None, q, 0, 4, 1, 1.0, -1.0, 0, 0, None) == -1 and b"empty" in lib.bhg_last_error()
    assert fn(q, q, q, q, q, None, q, -3, 4, 1, 1.0, -1.0, 0, 0, None) == -1
    assert fn(q, q, q, q, q, None, q, 4, 0, 1, 1.0, -1.0, 0, 0, None) == -1
    assert fn(q, q, q, q, q, None, q, 4, 4, -1, 1.0, -1.0, 0, 0, None) == -1 and b"negative" in lib.bhg_last_error()
    assert fn(q, q, q, q, q, None, q, 4, 4097, 1, 1.0, -1.0, 0, 0, None) == -1 and b"no native form" in lib.bhg_last_error()
    assert fn(q, q, q, q, q, None, q, 2048, 4096, 1, 1.0, -1.0, LOGREG_FORM_SINGLE, 0, None) == -1
    assert b"single form" in lib.bhg_last_error()
    buf = ctypes.create_string_buffer(64)
    assert lib.bhg_logreg_solve_plan(0, 4, 0, 0, buf, 64) == -1
    assert lib.bhg_logreg_solve_plan(4, 4, 0, 0, None, 64) == -1

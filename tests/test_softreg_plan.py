"""Host logic of the native softmax-regression solvers (csrc/bhg_softreg_solve.hip): which form a shape takes, the supported family,
and argument errors that must be refused before any device is touched.  No GPU needed."""
import ctypes
import re

import pytest

from betty_amd import _native
from betty_amd.backend import SOFTREG_FORM_AUTO, SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS, softreg_solve_plan

SYMBOLS = ("bhg_softreg_solve_plan", "bhg_softreg_solve_ws_bytes", "bhg_softreg_cg_solve", "bhg_softreg_neumann_solve")


def _ws(n, d, C):
    return int(_native.load().bhg_softreg_solve_ws_bytes(n, d, C))


def test_the_library_exports_and_the_binding_declares_the_four_symbols():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.SYMBOLS and getattr(lib, name) is not None


def test_cfg1_like_shape_plans_single():
    assert softreg_solve_plan(500, 100, 5).startswith("single")
    assert "1 launch per solve" in softreg_solve_plan(500, 100, 5)


@pytest.mark.parametrize("n,d,C", [(513, 1025, 10), (2048, 2048, 16), (100, 784, 10), (65536, 3072, 10), (1 << 20, 4096, 8)])
def test_wider_shapes_plan_strips(n, d, C):
    line = softreg_solve_plan(n, d, C)
    m = re.match(r"strips G=(\d+): (\d+) rows per strip", line)
    assert m, line
    G, rps = int(m.group(1)), int(m.group(2))
    assert 1 <= G <= 512 and G * rps >= n
    assert G * C * d * 4 <= 16 << 20, "auto mode keeps the partial buffer under 16 MiB"
    assert "3 launches per cg iteration" in line and "2 per neumann iteration" in line
    assert _ws(n, d, C) >= 512 * C * d * 4   # (any strip count a caller may force fits)


@pytest.mark.parametrize("n,d,C", [(3, 2, 2), (64, 64, 10), (257, 130, 7), (128, 2048, 2)])
def test_a_shape_both_forms_admit_can_be_forced_either_way(n, d, C):
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_SINGLE).startswith("single")
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_STRIPS).startswith("strips")


def test_a_given_strip_count_is_taken():
    assert softreg_solve_plan(17, 5, 3, SOFTREG_FORM_STRIPS, 7).startswith("strips G=7:")
    assert softreg_solve_plan(3, 2, 2, SOFTREG_FORM_STRIPS, 8).startswith("strips G=8:")
    assert softreg_solve_plan(4096, 257, 12, SOFTREG_FORM_STRIPS, 3).startswith("strips G=3:")
    assert softreg_solve_plan(2048, 2048, 16, SOFTREG_FORM_STRIPS, 512).startswith("strips G=512:")


@pytest.mark.parametrize("n,d,C", [(64, 64, 1), (64, 64, 17), (64, 4097, 4), (64, 2049, 16)])
def test_outside_the_family_nothing_native(n, d, C):
    assert softreg_solve_plan(n, d, C) == "none"
    assert _ws(n, d, C) == 0


def test_the_edges_of_the_family_are_inside():
    for n, d, C in [(64, 4096, 8), (64, 2048, 16), (64, 1, 2), (1, 1, 2)]:
        assert softreg_solve_plan(n, d, C) != "none" and _ws(n, d, C) > 0


def test_a_forced_form_the_shape_does_not_admit_is_an_error():
    with pytest.raises(_native.NativeLibraryError, match="single form"):
        softreg_solve_plan(513, 1025, 10, SOFTREG_FORM_SINGLE)      # C d > 4096
    with pytest.raises(_native.NativeLibraryError, match="single form"):
        softreg_solve_plan(4096, 257, 12, SOFTREG_FORM_SINGLE)      # n d > 2^18
    with pytest.raises(_native.NativeLibraryError, match="single form"):
        softreg_solve_plan(64, 64, 17, SOFTREG_FORM_SINGLE)
    with pytest.raises(_native.NativeLibraryError, match="strips form"):
        softreg_solve_plan(64, 4097, 4, SOFTREG_FORM_STRIPS)
    with pytest.raises(_native.NativeLibraryError, match="strips form"):
        softreg_solve_plan(64, 2049, 16, SOFTREG_FORM_STRIPS)
    with pytest.raises(_native.NativeLibraryError):
        softreg_solve_plan(64, 64, 4, 3)
    with pytest.raises(_native.NativeLibraryError, match="strips"):
        softreg_solve_plan(64, 64, 4, SOFTREG_FORM_STRIPS, 513)


@pytest.mark.parametrize("solve", ["bhg_softreg_cg_solve", "bhg_softreg_neumann_solve"])
def test_argument_errors_return_a_code_without_touching_a_device(solve):
    """NULL pointers, n <= 0, K < 0, a strip count past 512, a shape outside the family, a forced form that does not fit: refused by the
    host checks (no GPU is needed: the pointers below are not even device pointers)."""
    lib = _native.load()
    fn = getattr(lib, solve)
    host = (ctypes.c_float * 64)()
    q = ctypes.addressof(host)

    def call(X=q, out=q, ws=q, n=4, d=4, C=3, K=1, form=SOFTREG_FORM_AUTO, strips=0):
        return fn(X, q, q, q, out, None, ws, n, d, C, K, 1.0, -1.0, form, strips, None)

    for kw, word in [(dict(X=None), b"NULL"), (dict(out=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(n=0), b"empty"), (dict(n=-3), b"empty"),
                     (dict(d=0), b"empty"), (dict(K=-1), b"negative"), (dict(form=SOFTREG_FORM_STRIPS, strips=513), b"strips"),
                     (dict(C=17), b"no native form"), (dict(C=1), b"no native form"), (dict(d=4097), b"no native form"),
                     (dict(C=16, d=2049), b"no native form"), (dict(n=513, d=1025, C=10, form=SOFTREG_FORM_SINGLE), b"single form")]:
        assert call(**kw) == -1, kw
        assert word in lib.bhg_last_error(), (kw, lib.bhg_last_error())
    buf = ctypes.create_string_buffer(64)
    assert lib.bhg_softreg_solve_plan(0, 4, 3, 0, 0, buf, 64) == -1
    assert lib.bhg_softreg_solve_plan(4, 4, 3, 0, 0, None, 64) == -1

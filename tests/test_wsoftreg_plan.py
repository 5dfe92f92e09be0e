"""Host logic of the sample-weighted softmax-regression entry points (csrc/bhg_softreg_solve.hip: bhg_wsoftreg_cg_solve /
bhg_wsoftreg_neumann_solve / bhg_wsoftreg_mixed): the symbols, and the argument errors that must be refused before any device is
touched.  Plan, family and workspace are the softreg ones (tests/test_softreg_plan.py).  No GPU needed."""
import ctypes

import pytest

from betty_amd import _native
from betty_amd.backend import SOFTREG_FORM_AUTO, SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS, HipBackend

SYMBOLS = ("bhg_wsoftreg_cg_solve", "bhg_wsoftreg_neumann_solve", "bhg_wsoftreg_mixed")


def test_the_library_exports_and_the_binding_declares_the_three_symbols():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.SYMBOLS and getattr(lib, name) is not None
        assert hasattr(HipBackend, name[len("bhg_"):])
    assert lib.bhg_version() == 1


@pytest.mark.parametrize("solve", ["bhg_wsoftreg_cg_solve", "bhg_wsoftreg_neumann_solve"])
def test_solve_argument_errors_return_a_code_without_touching_a_device(solve):
    """NULL pointers (the weights among them), n <= 0, K < 0, a strip count past 512, a shape outside the family, a forced form that
    does not fit: refused by the host checks (the pointers below are not even device pointers)."""
    lib = _native.load()
    fn = getattr(lib, solve)
    host = (ctypes.c_float * 64)()
    q = ctypes.addressof(host)

    def call(X=q, a=q, out=q, ws=q, n=4, d=4, C=3, K=1, form=SOFTREG_FORM_AUTO, strips=0):
        return fn(X, q, q, a, q, out, ws, n, d, C, K, 1.0, -1.0, form, strips, None)

    for kw, word in [(dict(X=None), b"NULL"), (dict(a=None), b"NULL"), (dict(out=None), b"NULL"), (dict(ws=None), b"NULL"),
                     (dict(n=0), b"empty"), (dict(n=-3), b"empty"), (dict(d=0), b"empty"), (dict(K=-1), b"negative"),
                     (dict(form=SOFTREG_FORM_STRIPS, strips=513), b"strips"), (dict(C=17), b"no native form"), (dict(C=1), b"no native form"),
                     (dict(d=4097), b"no native form"), (dict(C=16, d=2049), b"no native form"),
                     (dict(n=513, d=1025, C=10, form=SOFTREG_FORM_SINGLE), b"single form")]:
        assert call(**kw) == -1, kw
        assert word in lib.bhg_last_error() and solve.encode() in lib.bhg_last_error(), (kw, lib.bhg_last_error())


def test_mixed_argument_errors_return_a_code_without_touching_a_device():
    lib = _native.load()
    host = (ctypes.c_float * 64)()
    q = ctypes.addressof(host)

    def call(X=q, dir_=q, y=q, c=q, n=4, d=4, C=3):
        return lib.bhg_wsoftreg_mixed(X, q, dir_, y, c, n, d, C, None)

    for kw, word in [(dict(X=None), b"NULL"), (dict(dir_=None), b"NULL"), (dict(y=None), b"NULL"), (dict(c=None), b"NULL"),
                     (dict(n=0), b"empty"), (dict(n=-1), b"empty"), (dict(d=0), b"empty"), (dict(C=17), b"no native form"),
                     (dict(C=1), b"no native form"), (dict(d=4097), b"no native form"), (dict(C=16, d=2049), b"no native form")]:
        assert call(**kw) == -1, kw
        assert word in lib.bhg_last_error() and b"bhg_wsoftreg_mixed" in lib.bhg_last_error(), (kw, lib.bhg_last_error())

"""The workspace of the strips form of the native linear-model solvers (csrc/bhg_linear_solve.hpp: strips_ws), pinned through the
ABI: rr and the den partials up to the byte offset of the vectors, four vectors of N floats padded to a multiple of four, the
partials of the widest strip count a caller may force (512).  No GPU needed."""
import pytest

from betty_amd import _native


def _layout(vec_off, N):
    return vec_off + 16 * ((N + 3) & ~3) + 4 * 512 * N


@pytest.mark.parametrize("n,d", [(1, 1), (500, 100), (7, 3), (33, 1025), (4096, 4094), (1 << 20, 4096)])
def test_logreg_workspace_bytes(n, d):
    assert int(_native.load().bhg_logreg_solve_ws_bytes(n, d)) == _layout(1024, d)


@pytest.mark.parametrize("n,d,C", [(1, 1, 2), (500, 100, 5), (7, 3, 3), (33, 1025, 7), (64, 2047, 16), (1 << 20, 4096, 8), (64, 2048, 16)])
def test_softreg_workspace_bytes(n, d, C):
    assert int(_native.load().bhg_softreg_solve_ws_bytes(n, d, C)) == _layout(8192, C * d)


def test_outside_the_family_there_is_no_workspace():
    lib = _native.load()
    assert int(lib.bhg_logreg_solve_ws_bytes(64, 4097)) == 0
    assert int(lib.bhg_logreg_solve_ws_bytes(0, 64)) == 0
    for n, d, C in [(64, 64, 1), (64, 64, 17), (64, 2049, 16), (0, 64, 4)]:   # C = 1, C = 17, C d > 32768, no rows
        assert int(lib.bhg_softreg_solve_ws_bytes(n, d, C)) == 0

"""Host logic of the fused batch-norm double backward (csrc/bhg_bn.hip): the shape -> launch geometry map of bn_slicing, read through
bhg_bn_plan — the very function the launch path calls.  No GPU needed.

The slicing cuts one channel's N x HW elements into `groups` sample groups of `ng` samples x `chunks` chunks of `chunk` elements of
the H*W run, `tpr` threads per run.  It is right only if the chunks cover the run with none empty, the groups cover the samples with
none empty, and the slice count stays inside what bhg_bn_ws_bytes reserves.  The sweep runs in ONE child process under a time limit:
the slice search is a loop, and a loop that stops terminating must fail this test, not hang the suite (it did not terminate for
N * C <= 3 and HW > 512 * 1024 before `chunks` was bounded by the slice limit)."""
import ctypes
import json
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import bn_plan

MAX_SLICES = 512
NS = (1, 2, 3, 4, 25, 200, 257, 513, 700)
CS = (1, 2, 3, 64, 2049)
HWS = (1, 4, 21, 36, 100, 441, 1024, 1961, 4100, 10244, 524288, 525312, 525313, 1048576)
KEYS = ("vec", "groups", "ng", "chunks", "chunk", "slices", "tpr")

# (N, C, HW) -> (ng, groups, chunks, chunk, tpr): the arithmetic as it stood before the bound on `chunks`, for shapes it terminated on
# (the ResNet-12 layers of BASELINE cfg 3 first).  The bound changes none of them.
TABLE = {
    (25, 64, 7056): (1, 25, 2, 3528, 256),
    (25, 128, 1764): (1, 25, 1, 1764, 256),
    (25, 256, 441): (3, 9, 1, 444, 256),
    (25, 512, 100): (11, 3, 1, 100, 32),
    (3, 5, 21): (3, 1, 1, 24, 32),
    (2, 1, 1): (2, 1, 1, 4, 16),
    (64, 16, 1024): (1, 64, 1, 1024, 256),
    (200, 1, 10244): (5, 40, 11, 932, 256),
    (300, 2, 4100): (3, 100, 4, 1028, 256),
    (1, 3, 1961): (1, 1, 2, 984, 256),
    (257, 1, 8): (128, 3, 1, 8, 16),
    (4, 1, 600000): (4, 1, 512, 1172, 256),
}
# N * C <= 3 and HW > 512 * 1024: the slice search never left its loop on these
FORMERLY_NON_TERMINATING = [(2, 1, 1048576), (1, 3, 1048576), (1, 1, 525312), (3, 1, 600000)]

_CHILD = r"""
import ctypes, json, re, sys
lib = ctypes.CDLL(sys.argv[1])
lib.bhg_bn_plan.restype = ctypes.c_int
lib.bhg_bn_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
buf = ctypes.create_string_buffer(256)
for N, C, HW in json.loads(sys.argv[2]):
    rc = lib.bhg_bn_plan(N, C, HW, buf, 256)
    row = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())} if rc == 0 else {}
    print(json.dumps({"shape": [N, C, HW], "rc": rc, "plan": row}), flush=True)
"""


@pytest.fixture(scope="module")
def plans():
    """(N, C, HW) -> plan dict for the grid, the table and the formerly non-terminating shapes: one child process, 120 s."""
    shapes = [(n, c, hw) for n in NS for c in CS for hw in HWS]
    assert len(shapes) == 630
    shapes += [s for s in list(TABLE) + FORMERLY_NON_TERMINATING if s not in shapes]
    try:
        out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path(), json.dumps(shapes)], capture_output=True, text=True,
                             timeout=120)
    except subprocess.TimeoutExpired as exc:
        seen = exc.stdout.decode() if isinstance(exc.stdout, bytes) else (exc.stdout or "")
        pytest.fail(f"the slice search did not return within 120 s; last shape answered: {seen.splitlines()[-1:] or 'none'}")
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert [tuple(r["shape"]) for r in rows] == shapes
    for r in rows:
        assert r["rc"] == 0 and sorted(r["plan"]) == sorted(KEYS), r
    return {tuple(r["shape"]): r["plan"] for r in rows}


def test_every_shape_of_the_grid_is_sliced_soundly(plans):
    for N in NS:
        for C in CS:
            for HW in HWS:
                p, at = plans[(N, C, HW)], (N, C, HW)
                # slice count: what the workspace formula of bhg_bn_ws_bytes relies on
                assert 1 <= p["slices"] == p["groups"] * p["chunks"] <= MAX_SLICES, (at, p)
                # chunks: 16-byte accesses stay aligned, none is empty, together they cover the run
                assert p["chunk"] % 4 == 0 and p["chunks"] * p["chunk"] >= HW and (p["chunks"] - 1) * p["chunk"] < HW, (at, p)
                # sample groups: none is empty, together they cover the samples
                assert 1 <= p["ng"] <= N and p["groups"] * p["ng"] >= N and (p["groups"] - 1) * p["ng"] < N, (at, p)
                # threads per run: a power of two, 256 / tpr whole rows per workgroup
                assert p["tpr"] in (16, 32, 64, 128, 256), (at, p)
                assert p["vec"] == (4 if HW % 4 == 0 else 1), (at, p)


@pytest.mark.parametrize("shape", list(TABLE), ids=lambda s: "x".join(map(str, s)))
def test_the_slicing_of_shapes_that_always_terminated_is_unchanged(plans, shape):
    p = plans[shape]
    assert (p["ng"], p["groups"], p["chunks"], p["chunk"], p["tpr"]) == TABLE[shape], p
    assert p["slices"] == p["groups"] * p["chunks"]


@pytest.mark.parametrize("shape", FORMERLY_NON_TERMINATING, ids=lambda s: "x".join(map(str, s)))
def test_few_long_runs_plan_one_group_and_at_most_512_chunks(plans, shape):
    N, C, HW = shape
    p = plans[shape]
    assert p["groups"] == 1 and p["ng"] == N and p["chunks"] <= MAX_SLICES, p
    assert p["chunk"] % 4 == 0 and p["chunks"] * p["chunk"] >= HW and (p["chunks"] - 1) * p["chunk"] < HW, p


def test_the_helper_reads_the_same_line():
    p = bn_plan(25, 64, 7056)
    assert p == {"vec": 4, "groups": 25, "ng": 1, "chunks": 2, "chunk": 3528, "slices": 50, "tpr": 256}
    assert bn_plan(3, 5, 21)["vec"] == 1


def test_shapes_the_launch_refuses_are_refused_by_the_plan():
    lib = _native.load()
    for kw, word in [((0, 4, 4), "empty"), ((4, 0, 4), "empty"), ((4, 4, 0), "empty"), ((-1, 4, 4), "empty"), ((4, 65536, 4), "65535 channels")]:
        with pytest.raises(_native.NativeLibraryError, match=word):
            bn_plan(*kw)
    assert bn_plan(4, 65535, 4)["slices"] >= 1
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_bn_plan(4, 4, 4, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_bn_plan(4, 4, 4, buf, 0) == -1
    assert lib.bhg_bn_plan(4, 4, 4, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan

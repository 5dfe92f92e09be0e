"""Host logic of the fused group-norm double backward (csrc/bhg_groupnorm.hip): the shape -> launch geometry map of gn_plan, read through
bhg_groupnorm_plan — the very function the launch path calls — and the refusals of bhg_groupnorm_backward_vjp, which come before any
device access.  No GPU needed.

A row (n, g) is D = (C / G) HW elements.  Resident (D <= 8192): the plan gives a row `tpr` threads (a power of two) and puts `rows` =
256 / tpr rows side by side as one row group = one workgroup; streamed (D > 8192): one workgroup of 256 threads per row, in tiles.  It is
right only if the workgroups cover the N G rows exactly once with none empty, the threads of a row cover its D elements with the vectors
of the kernel instance that runs, and the workspace written fits what bhg_groupnorm_ws_bytes reserves.  The map is closed-form; the sweep
runs in ONE child process under a time limit and times every call."""
import ctypes
import json
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import groupnorm_plan

NS = (1, 2, 3, 255, 257, 4096)
CGS = (1, 2, 3, 4, 7, 32)                    # channels per group
GS = (1, 2, 5, 32)
HWS = (1, 2, 3, 4, 5, 63, 64, 65, 256, 1000, 1024, 1171, 2048, 2049, 3136, 8192, 8193, 32768)
KEYS = ("regime", "D", "vec", "tpr", "rows", "nv", "inst", "tile", "groups", "grid", "ws")
SWEEP_SECONDS, CALL_SECONDS = 5.0, 1.0       # closed-form calls take microseconds; a search that crept back in takes far longer than these

_CHILD = r"""
import ctypes, json, re, sys, time
lib = ctypes.CDLL(sys.argv[1])
lib.bhg_groupnorm_plan.restype = ctypes.c_int
lib.bhg_groupnorm_plan.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
buf = ctypes.create_string_buffer(256)
for N, C, HW, G in json.loads(sys.argv[2]):
    t0 = time.perf_counter()
    rc = lib.bhg_groupnorm_plan(N, C, HW, G, buf, 256)
    dt = time.perf_counter() - t0
    row = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())} if rc == 0 else {}
    print(json.dumps({"shape": [N, C, HW, G], "rc": rc, "plan": row, "seconds": dt}), flush=True)
"""


def shapes():
    return [(n, cg * g, hw, g) for n in NS for cg in CGS for g in GS for hw in HWS if cg * hw <= 2 ** 20]


@pytest.fixture(scope="module")
def sweep():
    """(N, C, HW, G) -> (plan dict, seconds) for the grid: one child process, 60 s."""
    grid = shapes()
    assert len(grid) == len(NS) * len(CGS) * len(GS) * len(HWS)
    try:
        out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path(), json.dumps(grid)], capture_output=True, text=True,
                             timeout=60)
    except subprocess.TimeoutExpired as exc:
        seen = exc.stdout.decode() if isinstance(exc.stdout, bytes) else (exc.stdout or "")
        pytest.fail(f"the plan did not return within 60 s; last shape answered: {seen.splitlines()[-1:] or 'none'}")
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert [tuple(r["shape"]) for r in rows] == grid
    for r in rows:
        assert r["rc"] == 0 and sorted(r["plan"]) == sorted(KEYS), r
    return {tuple(r["shape"]): (r["plan"], r["seconds"]) for r in rows}


def test_every_shape_of_the_grid_is_planned_soundly(sweep):
    lib = _native.load()
    seen = set()
    for at, (p, _) in sweep.items():
        N, C, HW, G = at
        D = (C // G) * HW
        assert p["D"] == D, (at, p)
        assert p["vec"] == (4 if D % 4 == 0 else 1), (at, p)              # 16-byte accesses exactly when D % 4 == 0
        assert p["regime"] == (1 if D > 8192 else 0), (at, p)
        nvec = D // p["vec"]
        seen.add((p["regime"], p["vec"]))
        if p["regime"] == 0:
            # threads of a row: a power of two, whole rows side by side, and the instance's vectors cover the row
            assert p["tpr"] in (1, 2, 4, 8, 16, 32, 64, 128, 256) and p["rows"] * p["tpr"] == 256 and p["tile"] == 0, (at, p)
            assert p["nv"] == -(-nvec // p["tpr"]) and p["nv"] <= p["inst"], (at, p)
            assert p["inst"] in ((2, 4, 8) if p["vec"] == 4 else (2, 8, 32)), (at, p)
            assert p["inst"] == 2 or p["rows"] == 1, (at, p)
            assert p["tpr"] * p["inst"] * p["vec"] >= D, (at, p)           # the row's share of the LDS holds its terms
            # a narrow row leaves no more than half of a row's threads without an element
            assert p["tpr"] == 1 or 2 * nvec > p["tpr"], (at, p)
        else:
            assert (p["tpr"], p["rows"], p["tile"]) == (256, 1, 2048) and p["inst"] * 256 * p["vec"] == p["tile"], (at, p)
            assert p["nv"] == -(-nvec // 256), (at, p)
        # workgroups = row groups: they cover the N G rows exactly once (group i is the rows [i rows, min(N G, (i + 1) rows))), none empty
        assert p["grid"] == p["groups"] == -(-N * G // p["rows"]) >= 1, (at, p)
        assert (p["groups"] - 1) * p["rows"] < N * G <= p["groups"] * p["rows"], (at, p)
        # workspace: written <= reserved
        assert p["ws"] == 8 * N * C <= lib.bhg_groupnorm_ws_bytes(N, C), (at, p)
    assert seen == {(0, 1), (0, 4), (1, 1), (1, 4)}                          # both regimes, both access widths


def test_the_regime_flips_between_8192_and_8193():
    for (C, G, HW), regime in (((2, 2, 8192), "resident"), ((2, 2, 8193), "streamed"), ((16, 2, 1024), "resident"), ((8, 2, 2049), "streamed"),
                               ((8192, 1, 1), "resident"), ((8193, 1, 1), "streamed")):
        assert groupnorm_plan(3, C, HW, G)["regime"] == regime, (C, G, HW)


def test_the_whole_sweep_and_its_slowest_call_return_at_once(sweep):
    times = {at: s for at, (_, s) in sweep.items()}
    slowest = max(times, key=times.get)
    print(f"bhg_groupnorm_plan: {len(times)} shapes in {sum(times.values()) * 1e3:.3f} ms; slowest {slowest}: {times[slowest] * 1e6:.1f} us")
    assert sum(times.values()) <= SWEEP_SECONDS
    assert times[slowest] <= CALL_SECONDS, slowest


def test_the_helper_reads_the_same_line():
    assert groupnorm_plan(64, 64, 1024, 32) == {"regime": "resident", "D": 2048, "vec": 4, "tpr": 256, "rows": 1, "nv": 2, "inst": 2, "tile": 0,
                                                "groups": 2048, "grid": 2048, "ws": 8 * 64 * 64}
    assert groupnorm_plan(32, 256, 3136, 32) == {"regime": "streamed", "D": 25088, "vec": 4, "tpr": 256, "rows": 1, "nv": 25, "inst": 2,
                                                 "tile": 2048, "groups": 1024, "grid": 1024, "ws": 8 * 32 * 256}
    p = groupnorm_plan(7, 14, 1170, 2)
    assert (p["vec"], p["tpr"], p["nv"], p["inst"]) == (1, 256, 32, 32)
    p = groupnorm_plan(100, 8, 4, 4)
    assert (p["D"], p["tpr"], p["rows"], p["groups"]) == (8, 1, 256, 2)


REFUSED = [((0, 4, 4, 2), "empty tensor"), ((-1, 4, 4, 2), "empty tensor"), ((4, 0, 4, 2), "empty tensor"), ((4, -4, 4, 2), "empty tensor"),
           ((4, 4, 0, 2), "empty tensor"), ((4, 4, -3, 2), "empty tensor"), ((4, 4, 4, 0), "empty tensor"), ((4, 4, 4, -2), "empty tensor"),
           ((4, 6, 4, 4), "C is not a multiple of G"), ((4, 2, 2 ** 20 + 1, 2), r"more than 2\^20 elements per row"),
           ((4, 4, 2 ** 19 + 1, 2), r"more than 2\^20 elements per row"), ((4, 2, 2 ** 62, 2), r"more than 2\^20 elements per row"),
           ((2 ** 31, 2, 4, 2), r"more than 2\^31 - 1 rows"), ((2 ** 30, 4, 4, 4), r"more than 2\^31 - 1 rows"),
           ((2 ** 62, 2, 4, 2), r"more than 2\^31 - 1 rows")]


@pytest.mark.parametrize("shape,word", REFUSED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words(shape, word):
    lib = _native.load()
    fake = 0x7000_0000_0000   # never dereferenced: every refusal comes before any device access
    N, C, HW, G = shape
    with pytest.raises(_native.NativeLibraryError, match=word) as exc:
        groupnorm_plan(N, C, HW, G)
    rc = lib.bhg_groupnorm_backward_vjp(fake, fake, fake, fake, fake, fake, fake, fake, N, C, HW, G, fake, fake, fake, fake, 1 << 40, None)
    said = lib.bhg_last_error().decode()
    assert rc == -1 and said.split(": ", 1)[1] in str(exc.value), (shape, said, str(exc.value))


def test_the_workspace_size_and_the_plan_buffer():
    lib = _native.load()
    assert lib.bhg_groupnorm_ws_bytes(0, 4) == 0 and lib.bhg_groupnorm_ws_bytes(4, 0) == 0 and lib.bhg_groupnorm_ws_bytes(-3, 4) == 0
    assert lib.bhg_groupnorm_ws_bytes(2 ** 62, 2 ** 30) == 0                # beyond what size_t holds
    assert lib.bhg_groupnorm_ws_bytes(32, 256) == 8 * 32 * 256 and lib.bhg_groupnorm_ws_bytes(2 ** 31 - 1, 2 ** 20) == 8 * (2 ** 31 - 1) * 2 ** 20
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_groupnorm_plan(4, 4, 4, 2, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_groupnorm_plan(4, 4, 4, 2, buf, 0) == -1
    assert lib.bhg_groupnorm_plan(4, 4, 4, 2, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan


def test_the_launch_refuses_bad_pointers_and_workspaces_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    names = ["x", "gy", "a", "gamma", "mean", "rstd", "b", "c", "dx", "dgy", "dgamma", "ws"]

    def call(N=4, C=8, HW=2, G=2, ws_bytes=None, **over):
        p = {n: fake for n in names}
        p.update(over)
        ws_bytes = lib.bhg_groupnorm_ws_bytes(N, C) if ws_bytes is None else ws_bytes
        rc = lib.bhg_groupnorm_backward_vjp(p["x"], p["gy"], p["a"], p["gamma"], p["mean"], p["rstd"], p["b"], p["c"], N, C, HW, G, p["dx"],
                                            p["dgy"], p["dgamma"], p["ws"], ws_bytes, None)
        return rc, lib.bhg_last_error()

    for required in ("x", "gy", "mean", "rstd", "dx", "dgy"):
        rc, msg = call(**{required: None})
        assert rc == -1 and b"null pointer" in msg, (required, msg)
    rc, msg = call(ws=None)
    assert rc == -1 and b"no workspace" in msg, msg                          # dgamma without ws
    rc, msg = call(ws_bytes=8 * 4 * 8 - 1)
    assert rc == -1 and b"workspace smaller" in msg
    rc, msg = call(ws=fake + 4)
    assert rc == -1 and b"8-byte aligned" in msg
    for row_tensor in ("x", "gy", "a", "dx", "dgy"):                        # D = 8: the vector path
        rc, msg = call(**{row_tensor: fake + 4})
        assert rc == -1 and b"16-byte aligned" in msg, (row_tensor, msg)

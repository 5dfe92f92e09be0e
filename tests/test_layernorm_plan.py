"""Host logic of the fused layer-norm double backward (csrc/bhg_layernorm.hip): the shape -> launch geometry map of ln_plan, read through
bhg_layernorm_plan — the very function the launch path calls — and the refusals of bhg_layernorm_backward_vjp, which come before any
device access.  No GPU needed.

The plan gives a row `tpr` threads (a power of two), puts `rows` = 256 / tpr rows side by side as one row group, and cuts the `groups`
row groups into `slices` slices of `gps` groups: slice s is the rows [s gps rows, min(M, (s + 1) gps rows)).  It is right only if the
slices cover the rows with none empty, there are at most 64 (what bhg_layernorm_ws_bytes reserves), and the threads of a row cover its
D elements with the vectors of the kernel instance that runs.  The map is closed-form; the sweep runs in ONE child process under a time
limit and times every call, so that a search creeping back in fails this test instead of hanging the suite."""
import ctypes
import json
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import layernorm_plan

MAX_SLICES = 64
MS = (1, 2, 3, 63, 64, 65, 800, 4096, 65536, 2 ** 20 + 1)
DS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 768, 1000, 1024, 4096, 8188, 8191, 8192)
KEYS = ("vec", "tpr", "rows", "nv", "inst", "groups", "gps", "slices", "max_slices", "ws")
SWEEP_SECONDS, CALL_SECONDS = 5.0, 1.0   # 210 closed-form calls take under a millisecond together (19 us the slowest); a busy host can stall a
                                         # process for tens of milliseconds, a search that crept back in takes far longer than these

_CHILD = r"""
import ctypes, json, re, sys, time
lib = ctypes.CDLL(sys.argv[1])
lib.bhg_layernorm_plan.restype = ctypes.c_int
lib.bhg_layernorm_plan.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
buf = ctypes.create_string_buffer(256)
for M, D in json.loads(sys.argv[2]):
    t0 = time.perf_counter()
    rc = lib.bhg_layernorm_plan(M, D, buf, 256)
    dt = time.perf_counter() - t0
    row = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())} if rc == 0 else {}
    print(json.dumps({"shape": [M, D], "rc": rc, "plan": row, "seconds": dt}), flush=True)
"""


@pytest.fixture(scope="module")
def sweep():
    """(M, D) -> (plan dict, seconds) for the grid: one child process, 60 s."""
    shapes = [(m, d) for m in MS for d in DS]
    assert len(shapes) == 210
    try:
        out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path(), json.dumps(shapes)], capture_output=True, text=True,
                             timeout=60)
    except subprocess.TimeoutExpired as exc:
        seen = exc.stdout.decode() if isinstance(exc.stdout, bytes) else (exc.stdout or "")
        pytest.fail(f"the plan did not return within 60 s; last shape answered: {seen.splitlines()[-1:] or 'none'}")
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert [tuple(r["shape"]) for r in rows] == shapes
    for r in rows:
        assert r["rc"] == 0 and sorted(r["plan"]) == sorted(KEYS), r
    return {tuple(r["shape"]): (r["plan"], r["seconds"]) for r in rows}


def test_every_shape_of_the_grid_is_planned_soundly(sweep):
    lib = _native.load()
    for M in MS:
        for D in DS:
            p, at = sweep[(M, D)][0], (M, D)
            assert p["vec"] == (4 if D % 4 == 0 else 1), (at, p)
            # threads of a row: a power of two, whole rows side by side, and the instance's vectors cover the row
            assert p["tpr"] in (1, 2, 4, 8, 16, 32, 64, 128, 256) and p["rows"] * p["tpr"] == 256, (at, p)
            nvec = D // p["vec"]
            assert p["nv"] == -(-nvec // p["tpr"]) and p["nv"] <= p["inst"], (at, p)
            assert p["inst"] in ((2, 4, 8) if p["vec"] == 4 else (2, 8, 32)), (at, p)
            assert p["inst"] == 2 or p["rows"] == 1, (at, p)          # rows side by side only with two vectors per thread (the kernel's LDS)
            # a narrow row leaves no more than half of a row's threads without an element
            assert p["tpr"] == 1 or 2 * nvec > p["tpr"], (at, p)
            # row groups cover the rows, none empty
            assert p["groups"] == -(-M // p["rows"]), (at, p)
            # slices: cover the groups, none empty, at most 64
            assert p["max_slices"] == MAX_SLICES and 1 <= p["slices"] <= MAX_SLICES, (at, p)
            assert p["gps"] >= 1 and p["slices"] * p["gps"] >= p["groups"] and (p["slices"] - 1) * p["gps"] < p["groups"], (at, p)
            assert (p["slices"] - 1) * p["gps"] * p["rows"] < M, (at, p)   # the last slice's first row exists
            # the bound takes hold only where there are more groups than slices
            assert p["slices"] == p["groups"] or p["groups"] > MAX_SLICES, (at, p)
            # workspace
            assert p["ws"] == 8 * p["slices"] * D <= lib.bhg_layernorm_ws_bytes(D) == 8 * MAX_SLICES * D, (at, p)


def test_the_whole_sweep_and_its_slowest_call_return_at_once(sweep):
    times = {at: s for at, (_, s) in sweep.items()}
    slowest = max(times, key=times.get)
    print(f"bhg_layernorm_plan: {len(times)} shapes in {sum(times.values()) * 1e3:.3f} ms; slowest {slowest}: {times[slowest] * 1e6:.1f} us")
    assert sum(times.values()) <= SWEEP_SECONDS
    assert times[slowest] <= CALL_SECONDS, slowest


def test_the_helper_reads_the_same_line():
    assert layernorm_plan(800, 768) == {"vec": 4, "tpr": 128, "rows": 2, "nv": 2, "inst": 2, "groups": 400, "gps": 7, "slices": 58,
                                        "max_slices": 64, "ws": 8 * 58 * 768}
    assert layernorm_plan(7, 8192) == {"vec": 4, "tpr": 256, "rows": 1, "nv": 8, "inst": 8, "groups": 7, "gps": 1, "slices": 7,
                                       "max_slices": 64, "ws": 8 * 7 * 8192}
    p = layernorm_plan(7, 8191)
    assert (p["vec"], p["tpr"], p["nv"], p["inst"]) == (1, 256, 32, 32)
    p = layernorm_plan(4097, 64)
    assert (p["tpr"], p["rows"], p["groups"], p["gps"], p["slices"]) == (8, 32, 129, 3, 43)


def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words():
    lib = _native.load()
    fake = 0x7000_0000_0000   # never dereferenced: every refusal comes before any device access
    for (M, D), word in [((4, 0), "empty tensor"), ((0, 4), "empty tensor"), ((-1, 4), "empty tensor"), ((4, -4), "empty tensor"),
                         ((4, 8193), "more than 8192 elements per row")]:
        with pytest.raises(_native.NativeLibraryError, match=word):
            layernorm_plan(M, D)
        rc = lib.bhg_layernorm_backward_vjp(fake, fake, fake, fake, fake, fake, fake, fake, M, D, fake, fake, fake, fake, 1 << 30, None)
        assert rc == -1 and word.encode() in lib.bhg_last_error(), (M, D, lib.bhg_last_error())
    assert lib.bhg_layernorm_ws_bytes(0) == 0 and lib.bhg_layernorm_ws_bytes(8193) == 0 and lib.bhg_layernorm_ws_bytes(-3) == 0
    assert lib.bhg_layernorm_ws_bytes(8192) == 8 * 64 * 8192
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_layernorm_plan(4, 4, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_layernorm_plan(4, 4, buf, 0) == -1
    assert lib.bhg_layernorm_plan(4, 4, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan


def test_the_launch_refuses_bad_pointers_and_workspaces_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    names = ["x", "gy", "a", "gamma", "mean", "rstd", "b", "c", "dx", "dgy", "dgamma", "ws"]

    def call(M=4, D=8, ws_bytes=None, **over):
        p = {n: fake for n in names}
        p.update(over)
        ws_bytes = lib.bhg_layernorm_ws_bytes(D) if ws_bytes is None else ws_bytes
        rc = lib.bhg_layernorm_backward_vjp(p["x"], p["gy"], p["a"], p["gamma"], p["mean"], p["rstd"], p["b"], p["c"], M, D, p["dx"], p["dgy"],
                                            p["dgamma"], p["ws"], ws_bytes, None)
        return rc, lib.bhg_last_error()

    for required in ("x", "gy", "mean", "rstd", "dx", "dgy", "ws"):
        rc, msg = call(**{required: None})
        assert rc == -1 and b"null pointer" in msg, (required, msg)
    rc, msg = call(ws_bytes=8 * 64 * 8 - 1)
    assert rc == -1 and b"workspace smaller" in msg
    rc, msg = call(ws=fake + 4)
    assert rc == -1 and b"8-byte aligned" in msg
    for row_tensor in ("x", "gy", "a", "dx", "dgy"):
        rc, msg = call(**{row_tensor: fake + 4})
        assert rc == -1 and b"16-byte aligned" in msg, (row_tensor, msg)

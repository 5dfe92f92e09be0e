"""Host logic of the declared activations' double backward (csrc/bhg_activation.hip): the size -> launch geometry maps act_plan and
gated_plan, read through bhg_act_plan / bhg_gated_act_plan — the very functions the launches call — and the refusals of
bhg_act_backward_vjp / bhg_gated_act_backward_vjp, which come before any device access.  No GPU needed.

Plain: n elements in `units` of `vec` elements, one unit per thread and trip; grid workgroups of 256 threads make `iters` trips.  Gated:
a row of H elements gets `tpr` threads (a power of two), `rows` = 256 / tpr rows sit side by side, `cb` workgroups lie along a row; the
`work` = rgroups * cb pieces are taken `grid` at a time in `iters` trips.  A plan is right only if grid * block * vec * iters covers the
work, no workgroup is empty, the grid stays under its cap, and the 16-byte path is chosen exactly when its conditions hold.  The maps
are closed-form; the sweeps run in ONE child process under a time limit."""
import ctypes
import json
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import activation_plan, gated_activation_plan

CAP = 2048                                                          # 256 CUs x 8 workgroups
PLAIN_KEYS = ("vec", "block", "grid", "iters", "units", "inst")
GATED_KEYS = ("vec", "block", "grid", "iters", "tpr", "rows", "cb", "rgroups", "work", "inst")

_CHILD = r"""
import ctypes, json, re, sys
lib = ctypes.CDLL(sys.argv[1])
LL = ctypes.c_longlong
lib.bhg_act_plan.restype = ctypes.c_int
lib.bhg_act_plan.argtypes = [LL, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
lib.bhg_gated_act_plan.restype = ctypes.c_int
lib.bhg_gated_act_plan.argtypes = [LL, LL, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
buf = ctypes.create_string_buffer(256)
job = json.loads(sys.stdin.read())
def row(rc):
    return {k: int(v) if re.fullmatch(r"-?\d+", v) else v for k, v in re.findall(r"(\w+)=(\S+)", buf.value.decode())} if rc == 0 else {}
for n, al in job["plain"]:
    rc = lib.bhg_act_plan(n, al, buf, 256)
    print(json.dumps({"at": [n, al], "rc": rc, "plan": row(rc)}))
for r, h, ok in job["gated"]:
    rc = lib.bhg_gated_act_plan(r, h, ok, buf, 256)
    print(json.dumps({"at": [r, h, ok], "rc": rc, "plan": row(rc)}))
"""


def plain_sizes():
    ns = set()
    for e in range(0, 41):
        ns.update(v for v in (2 ** e - 1, 2 ** e, 2 ** e + 1) if v >= 1)
    for vec in (1, 4):                                              # around the grid cap: one unit fewer / more than 2048 workgroups hold, and twice that
        edge = CAP * 256 * vec
        ns.update((edge - vec, edge - 1, edge, edge + 1, edge + vec, 2 * edge - 1, 2 * edge, 2 * edge + 1))
    return [(n, al) for n in sorted(ns) for al in (0, 1)]


def gated_shapes():
    rows = [1, 2, 3, 7, 255, 256, 257, 2047, 2048, 2049, 4097, 2 ** 20 + 1]
    hs = [1, 2, 3, 4, 5, 7, 8, 12, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1028, 2048, 11008, 2 ** 16 + 4, 2 ** 20, 2 ** 20 + 1]
    big = [(2 ** 30, 2 ** 10, 1), (2 ** 40, 1, 1), (1, 2 ** 40, 1), (2 ** 20 + 3, 2 ** 20 + 4, 0)]
    return [(r, h, ok) for r in rows for h in hs for ok in (0, 1)] + big


@pytest.fixture(scope="module")
def sweep():
    job = {"plain": plain_sizes(), "gated": gated_shapes()}
    out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path()], input=json.dumps(job), capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(rows) == len(job["plain"]) + len(job["gated"])
    for r in rows:
        assert r["rc"] == 0, r
    return {tuple(r["at"]): r["plan"] for r in rows[:len(job["plain"])]}, {tuple(r["at"]): r["plan"] for r in rows[len(job["plain"]):]}


def test_every_plain_size_is_planned_soundly(sweep):
    plans, _ = sweep
    assert max(n for n, _ in plans) >= 2 ** 40 and min(n for n, _ in plans) == 1
    deep = 0
    for (n, al), p in plans.items():
        assert sorted(p) == sorted(PLAIN_KEYS), p
        assert p["vec"] == (4 if al else 1) and p["block"] == 256, ((n, al), p)                # the vector path exactly when aligned
        assert p["inst"] == f"k_act_vjp<kind,{p['vec']}>", p
        assert p["units"] == -(-n // p["vec"]), ((n, al), p)
        assert 1 <= p["grid"] <= CAP and p["grid"] == min(-(-p["units"] // 256), CAP), ((n, al), p)
        assert p["grid"] * p["block"] * p["vec"] * p["iters"] >= n, ((n, al), p)                 # the trips cover the work
        assert (p["grid"] - 1) * 256 < p["units"], ((n, al), p)                                    # no workgroup is empty in the first trip
        assert (p["iters"] - 1) * p["grid"] * 256 < p["units"], ((n, al), p)                       # and no trip is
        deep += p["iters"] > 1
    assert deep > 10


def test_every_gated_shape_is_planned_soundly(sweep):
    _, plans = sweep
    seen = set()
    for (rows, H, ok), p in plans.items():
        at = (rows, H, ok)
        assert sorted(p) == sorted(GATED_KEYS), p
        assert p["vec"] == (4 if ok and H % 4 == 0 else 1) and p["block"] == 256, (at, p)
        assert p["inst"] == f"k_gated_act_vjp<kind,{p['vec']}>", p
        hu = H // p["vec"]
        assert p["tpr"] in (1, 2, 4, 8, 16, 32, 64, 128, 256) and p["rows"] * p["tpr"] == 256, (at, p)
        assert p["tpr"] >= min(hu, 256) and (p["tpr"] == 1 or p["tpr"] < 2 * hu), (at, p)         # under half of a row's threads idle
        assert p["cb"] == -(-hu // p["tpr"]) and (p["cb"] == 1 or p["tpr"] == 256), (at, p)
        assert p["cb"] * p["tpr"] * p["vec"] >= H > (p["cb"] - 1) * p["tpr"] * p["vec"], (at, p)   # a row is covered, no column block empty
        assert p["rgroups"] == -(-rows // p["rows"]) and (p["rgroups"] - 1) * p["rows"] < rows, (at, p)
        assert p["work"] == p["rgroups"] * p["cb"], (at, p)
        assert 1 <= p["grid"] == min(p["work"], CAP), (at, p)                                      # every workgroup has a piece in the first trip
        assert p["grid"] * p["iters"] >= p["work"] > p["grid"] * (p["iters"] - 1), (at, p)
        assert p["grid"] * p["block"] * p["vec"] * p["iters"] >= rows * H, (at, p)
        seen.add((p["vec"], p["cb"] > 1, p["iters"] > 1))
    assert seen == {(v, c, i) for v in (1, 4) for c in (False, True) for i in (False, True)}


def test_the_helpers_read_the_same_lines():
    assert activation_plan(800 * 3072) == {"vec": 4, "block": 256, "grid": 2048, "iters": 2, "units": 614400, "inst": "k_act_vjp<kind,4>"}
    assert activation_plan(5, aligned16=False) == {"vec": 1, "block": 256, "grid": 1, "iters": 1, "units": 5, "inst": "k_act_vjp<kind,1>"}
    assert gated_activation_plan(2048, 11008) == {"vec": 4, "block": 256, "grid": 2048, "iters": 11, "tpr": 256, "rows": 1, "cb": 11,
                                                  "rgroups": 2048, "work": 22528, "inst": "k_gated_act_vjp<kind,4>"}
    p = gated_activation_plan(3, 5)
    assert (p["vec"], p["tpr"], p["rows"], p["cb"], p["grid"]) == (1, 8, 32, 1, 1)
    assert gated_activation_plan(7, 12, vec_ok=False)["vec"] == 1


FAKE = 0x7000_0000_0000   # never dereferenced: every refusal comes before any device access


def _plain(kind=0, n=8, **over):
    lib = _native.load()
    p = {k: FAKE for k in ("x", "gy", "a", "dx", "dgy")}
    p.update(over)
    rc = lib.bhg_act_backward_vjp(kind, 1.0, 20.0, p["x"], p["gy"], p["a"], p["dx"], p["dgy"], n, None)
    return rc, lib.bhg_last_error().decode()


def _gated(kind=2, rows=4, H=8, ld=None, **over):
    lib = _native.load()
    names = ("u", "v", "gy", "au", "av", "du", "dv", "dgy")
    p = {k: FAKE for k in names}
    lds = {k: H for k in names}
    lds.update(ld or {})
    p.update(over)
    args = []
    for k in names:
        args += [p[k], lds[k]]
    rc = lib.bhg_gated_act_backward_vjp(kind, rows, H, *args, None)
    return rc, lib.bhg_last_error().decode()


def test_the_plain_launch_refuses_before_any_device_access():
    for kind in (-1, 6, 99):
        rc, msg = _plain(kind=kind)
        assert rc == -1 and "unknown kind" in msg, msg
    for n in (0, -1, -2 ** 40):
        rc, msg = _plain(n=n)
        assert rc == -1 and "empty tensor" in msg, msg
        with pytest.raises(_native.NativeLibraryError, match="empty tensor"):
            activation_plan(n)
    for name in ("x", "gy", "a"):
        rc, msg = _plain(**{name: None})
        assert rc == -1 and "null pointer" in msg, (name, msg)
    rc, msg = _plain(dx=None, dgy=None)
    assert rc == -1 and "no output wanted" in msg, msg
    rc, msg = _plain(n=2 ** 62 + 1)
    assert rc == -1 and "2^62" in msg, msg
    with pytest.raises(_native.NativeLibraryError, match=r"2\^62"):
        activation_plan(2 ** 62 + 1)


def test_the_gated_launch_refuses_before_any_device_access():
    for kind in (-1, 6):
        rc, msg = _gated(kind=kind)
        assert rc == -1 and "unknown kind" in msg, msg
    rc, msg = _gated(kind=5)
    assert rc == -1 and "softplus has no gated form" in msg, msg
    for rows, H in ((0, 8), (-1, 8), (4, 0), (4, -8)):
        rc, msg = _gated(rows=rows, H=H)
        assert rc == -1 and "empty tensor" in msg, msg
        with pytest.raises(_native.NativeLibraryError, match="empty tensor"):
            gated_activation_plan(rows, H)
    for name in ("u", "v", "gy", "au", "av", "du", "dv", "dgy"):
        rc, msg = _gated(ld={name: 7})
        assert rc == -1 and "leading dimension is smaller than H" in msg, (name, msg)
    for name in ("u", "v", "gy"):
        rc, msg = _gated(**{name: None})
        assert rc == -1 and "null pointer" in msg, (name, msg)
    rc, msg = _gated(au=None, av=None)
    assert rc == -1 and "no cotangent" in msg, msg
    rc, msg = _gated(du=None, dv=None, dgy=None)
    assert rc == -1 and "no output wanted" in msg, msg
    rc, msg = _gated(rows=2 ** 40, H=8, ld={"u": 2 ** 23})           # rows * max ld = 2^63
    assert rc == -1 and "2^62" in msg, msg
    rc, msg = _gated(rows=2 ** 60, H=8)
    assert rc == -1 and "2^62" in msg, msg
    with pytest.raises(_native.NativeLibraryError, match=r"2\^62"):
        gated_activation_plan(2 ** 60, 8)
    # an unused array's leading dimension is not read
    rc, msg = _gated(au=None, du=None, dv=None, dgy=None, ld={"au": 0})
    assert rc == -1 and "no output wanted" in msg, msg


def test_the_plan_buffers():
    lib = _native.load()
    buf = ctypes.create_string_buffer(8)
    for fn, args in ((lib.bhg_act_plan, (64, 1)), (lib.bhg_gated_act_plan, (4, 8, 1))):
        assert fn(*args, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
        assert fn(*args, buf, 0) == -1
        assert fn(*args, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan

"""Host logic of the tiled attention double backward (csrc/bhg_attention_tiled.hip): the shape -> tiles, pitches, grids, LDS and
workspace map of tl_plan, read through bhg_attention_tiled_plan — the very function the launch path calls — and the refusals of
bhg_attention_tiled_backward_vjp, which come before any device access.  No GPU needed.

Both launches keep three 64-row operand tiles (Q, gO, aQ), four 32-row ones (K, V, aK, aV) and 64 x 32 score tiles (four in the query
launch, three in the key launch) in the LDS of one CU.  The plan is right only if that fits the 160 KiB a workgroup may take for every
shape of the family, the LDS figure is the sum of those parts, the operand pitch holds d rounded up to 16 and is an odd number of 16-byte
units, the grids are the tile counts times B H, and the workspace is what bhg_attention_tiled_ws_bytes says.  The sweep runs in ONE
child process."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import attention_plan, attention_tiled_plan

MAX_LDS = 163840
NS = (1, 63, 64, 65, 127, 128, 129, 511, 512)
DS = (1, 3, 4, 63, 64)
KEYS = ("vec", "bm", "bn", "dp", "pd", "ps", "grid_q", "grid_k", "lds_q", "lds_k", "max_lds", "ws")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import ctypes, json, re, sys
lib = ctypes.CDLL(sys.argv[1])
lib.bhg_attention_tiled_plan.restype = ctypes.c_int
lib.bhg_attention_tiled_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_size_t]
lib.bhg_attention_tiled_ws_bytes.restype = ctypes.c_size_t
lib.bhg_attention_tiled_ws_bytes.argtypes = [ctypes.c_int] * 3
buf = ctypes.create_string_buffer(256)
for L, S, d, ok in json.loads(sys.argv[2]):
    rc = lib.bhg_attention_tiled_plan(3, 5, L, S, d, ok, buf, 256)
    row = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())} if rc == 0 else {}
    print(json.dumps({"shape": [L, S, d, ok], "rc": rc, "plan": row, "ws": lib.bhg_attention_tiled_ws_bytes(3, 5, L)}), flush=True)
"""


@pytest.fixture(scope="module")
def sweep():
    """(L, S, d, vec_ok) -> (plan dict, ws bytes) for the grid: one child process."""
    shapes = [(L, S, d, ok) for L in NS for S in NS for d in DS for ok in (1, 0)]
    out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path(), json.dumps(shapes)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert [tuple(r["shape"]) for r in rows] == shapes
    for r in rows:
        assert r["rc"] == 0 and sorted(r["plan"]) == sorted(KEYS), r
    return {tuple(r["shape"]): (r["plan"], r["ws"]) for r in rows}


def test_every_shape_of_the_grid_fits_the_lds_and_is_planned_soundly(sweep):
    worst = 0
    for (L, S, d, ok), (p, ws) in sweep.items():
        at = (L, S, d, ok)
        assert p["vec"] == (4 if d % 4 == 0 and ok else 1), (at, p)
        assert (p["bm"], p["bn"], p["ps"], p["max_lds"]) == (64, 32, 36, MAX_LDS), (at, p)
        assert p["dp"] == (d + 15) // 16 * 16 and p["pd"] == p["dp"] + 4 and p["pd"] % 8 == 4, (at, p)   # an odd number of 16-byte units
        assert p["ps"] >= p["bn"] and p["ps"] % 8 == 4, (at, p)
        operands = (3 * p["bm"] + 4 * p["bn"]) * p["pd"]
        assert p["lds_q"] == 4 * (operands + 4 * p["bm"] * p["ps"]), (at, p)          # the sum of its parts, nothing else
        assert p["lds_k"] == 4 * (operands + 3 * p["bm"] * p["ps"]), (at, p)
        assert 0 < p["lds_k"] < p["lds_q"] <= MAX_LDS, (at, p)
        assert p["grid_q"] == 15 * ((L + 63) // 64) and p["grid_k"] == 15 * ((S + 31) // 32), (at, p)
        assert p["ws"] == ws == 15 * L * 5 * 8, (at, p, ws)                          # five doubles per query row
        worst = max(worst, p["lds_q"])
    print(f"bhg_attention_tiled_plan: {len(sweep)} shapes, largest lds = {worst} bytes of {MAX_LDS}")
    assert worst == sweep[(512, 512, 64, 1)][0]["lds_q"] == 123904


def test_the_helper_reads_the_same_line():
    assert attention_tiled_plan(16, 12, 512, 512, 64) == {"vec": 4, "bm": 64, "bn": 32, "dp": 64, "pd": 68, "ps": 36, "grid_q": 192 * 8,
                                                          "grid_k": 192 * 16, "lds_q": 123904, "lds_k": 114688, "max_lds": MAX_LDS,
                                                          "ws": 192 * 512 * 40}
    p = attention_tiled_plan(1, 1, 65, 65, 3)
    assert (p["vec"], p["dp"], p["pd"], p["grid_q"], p["grid_k"], p["ws"]) == (1, 16, 20, 2, 3, 2600)
    assert attention_tiled_plan(1, 1, 65, 65, 8, vec_ok=False)["vec"] == 1
    lib = _native.load()
    assert lib.bhg_attention_tiled_ws_bytes(0, 1, 1) == 0 and lib.bhg_attention_tiled_ws_bytes(1, 1, -3) == 0


def _launch(lib, B=2, H=2, L=70, S=70, d=8, strides=None, mask=None, mask_strides=None, ws=0x7100_0000_0000, ws_bytes=None, **over):
    """bhg_attention_tiled_backward_vjp on host pointers that are never dereferenced."""
    fake = 0x7000_0000_0000
    p = {n: fake for n in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo")}
    p.update(over)
    if strides is None:
        strides = []
        for rows in (L, S, S, L, L, S, S):
            strides += [H * rows * d, rows * d, d, 1]
    st = (ctypes.c_longlong * 28)(*strides) if strides != "null" else None
    mst = (ctypes.c_longlong * 4)(*mask_strides) if mask_strides is not None else None
    if ws_bytes is None:
        ws_bytes = max(B, 0) * max(H, 0) * max(L, 0) * 40
    rc = lib.bhg_attention_tiled_backward_vjp(p["q"], p["k"], p["v"], p["go"], p["aq"], p["ak"], p["av"], st, mask, mst, 0, 0.5, B, H, L, S, d,
                                              p["dq"], p["dk"], p["dv"], p["dgo"], ws, ws_bytes, None)
    return rc, lib.bhg_last_error()


def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words():
    lib = _native.load()
    cases = [(dict(L=0), "empty tensor"), (dict(S=0), "empty tensor"), (dict(d=0), "empty tensor"), (dict(B=0), "empty tensor"),
             (dict(H=-1), "empty tensor"), (dict(L=513), "more than 512 queries"), (dict(S=513), "more than 512 keys"),
             (dict(d=65), "more than 64 elements per head"), (dict(B=1 << 20, H=1 << 10, L=512, S=4), "2\\^31 - 1 workgroups"),
             (dict(B=1 << 20, H=1 << 9, L=4, S=512), "2\\^31 - 1 workgroups")]
    for over, word in cases:
        shape = dict(B=2, H=2, L=70, S=70, d=8)
        shape.update(over)
        with pytest.raises(_native.NativeLibraryError, match=word):
            attention_tiled_plan(**shape)
        rc, msg = _launch(lib, ws_bytes=1 << 62, **shape)
        assert rc == -1 and word.replace("\\", "").encode() in msg, (over, msg)
    attention_tiled_plan(1 << 20, 1 << 10, 64, 32, 8)                          # 2^30 workgroups in both launches: inside
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_attention_tiled_plan(1, 1, 70, 70, 4, 1, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_attention_tiled_plan(1, 1, 70, 70, 4, 1, buf, 0) == -1
    assert lib.bhg_attention_tiled_plan(1, 1, 70, 70, 4, 1, buf, 8) == -1 and b"too small" in lib.bhg_last_error()


def test_the_short_kernel_keeps_its_family_and_its_words():
    with pytest.raises(_native.NativeLibraryError, match="more than 64 queries"):
        attention_plan(2, 2, 65, 4, 8)
    with pytest.raises(_native.NativeLibraryError, match="more than 64 keys"):
        attention_plan(2, 2, 4, 65, 8)
    assert attention_tiled_plan(2, 2, 4, 4, 8)["grid_q"] == 4                  # the tiled kernels take short shapes as well


def test_the_launch_refuses_bad_arguments_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    for required in ("q", "k", "v", "go"):
        rc, msg = _launch(lib, **{required: None})
        assert rc == -1 and b"null pointer" in msg, (required, msg)
    rc, msg = _launch(lib, strides="null")
    assert rc == -1 and b"null pointer" in msg
    rc, msg = _launch(lib, aq=None, ak=None, av=None)
    assert rc == -1 and b"all three cotangents are NULL" in msg
    rc, msg = _launch(lib, dq=None, dk=None, dv=None, dgo=None)
    assert rc == -1 and b"all four outputs are NULL" in msg
    rc, msg = _launch(lib, mask=fake)
    assert rc == -1 and b"mask_strides" in msg
    rc, msg = _launch(lib, ws=None)
    assert rc == -1 and b"null pointer (workspace)" in msg
    rc, msg = _launch(lib, ws_bytes=2 * 2 * 70 * 40 - 1)
    assert rc == -1 and b"workspace too small" in msg
    rc, msg = _launch(lib, ws=0x7100_0000_0004)
    assert rc == -1 and b"8-byte aligned" in msg
    contiguous = []
    for rows in (70,) * 7:
        contiguous += [2 * rows * 8, rows * 8, 8, 1]
    for i in range(7):                                                        # a non-unit last stride, input by input
        bad = list(contiguous)
        bad[4 * i + 3] = 2
        rc, msg = _launch(lib, strides=bad)
        assert rc == -1 and b"last stride" in msg, (i, msg)
    bad = list(contiguous)
    bad[2] = -8
    rc, msg = _launch(lib, strides=bad)
    assert rc == -1 and b"negative stride" in msg
    for name in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo"):   # misalignment on the vector path
        rc, msg = _launch(lib, **{name: fake + 4})
        assert rc == -1 and b"16-byte aligned" in msg, (name, msg)
    # the entries of a NULL input are ignored: its last stride and its alignment refuse nothing (the next refusal is reached instead)
    bad = list(contiguous)
    bad[4 * 4 + 3] = 2
    rc, msg = _launch(lib, strides=bad, aq=None, dq=fake + 4)
    assert rc == -1 and b"16-byte aligned" in msg


def test_header_binding_and_exports_agree_for_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bhg.h")).read(), flags=re.S)
    lib = _native.load()
    for name, nargs, ret in (("bhg_attention_tiled_ws_bytes", 3, ctypes.c_size_t), ("bhg_attention_tiled_plan", 8, ctypes.c_int),
                             ("bhg_attention_tiled_backward_vjp", 24, ctypes.c_int)):
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert proto and len(proto.group(1).split(",")) == nargs == len(_native.SYMBOLS[name][1]), name
        assert _native.SYMBOLS[name][0] is ret and hasattr(lib, name)
        assert getattr(_native.load(), name).argtypes == _native.SYMBOLS[name][1]
    ab = ctypes.CDLL(_native.AB_LIB_PATH)
    assert all(hasattr(ab, n) for n in ("bhg_attention_tiled_ws_bytes", "bhg_attention_tiled_plan", "bhg_attention_tiled_backward_vjp"))

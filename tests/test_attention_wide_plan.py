"""Host logic of the wide attention double backward (csrc/bhg_attention_wide.hip): the shape -> tiles, pitches, grids, LDS and workspace
map of wd_plan, read through bhg_attention_wide_plan — the very function the launch calls — and the refusals of
bhg_attention_wide_backward_vjp, which come before any device access.  No GPU needed.  The sweep runs in ONE child process."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import attention_tiled_plan, attention_wide_plan

MAX_LDS = 163840
NS = (1, 63, 64, 65, 511, 512)
DS = (65, 67, 68, 127, 128)
KEYS = ("vec", "bm", "bn", "ps", "kbm", "kbn", "kps", "dp", "pd", "grid_q", "grid_k", "lds_q", "lds_k", "max_lds", "ws")
NEW = (("bhg_attention_wide_ws_bytes", 3, ctypes.c_size_t), ("bhg_attention_wide_plan", 8, ctypes.c_int),
       ("bhg_attention_wide_backward_vjp", 24, ctypes.c_int))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import ctypes, json, re, sys
lib = ctypes.CDLL(sys.argv[1])
lib.bhg_attention_wide_plan.restype = ctypes.c_int
lib.bhg_attention_wide_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_size_t]
lib.bhg_attention_wide_ws_bytes.restype = ctypes.c_size_t
lib.bhg_attention_wide_ws_bytes.argtypes = [ctypes.c_int] * 3
buf = ctypes.create_string_buffer(256)
for L, S, d, ok in json.loads(sys.argv[2]):
    rc = lib.bhg_attention_wide_plan(3, 5, L, S, d, ok, buf, 256)
    row = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())} if rc == 0 else {}
    print(json.dumps({"shape": [L, S, d, ok], "rc": rc, "plan": row, "ws": lib.bhg_attention_wide_ws_bytes(3, 5, L)}), flush=True)
"""


def test_every_shape_of_the_grid_fits_the_lds_and_is_planned_soundly():
    shapes = [(L, S, d, ok) for L in NS for S in NS for d in DS for ok in (1, 0)]
    out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path(), json.dumps(shapes)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert [tuple(r["shape"]) for r in rows] == shapes
    for r in rows:
        (L, S, d, ok), p, ws = r["shape"], r["plan"], r["ws"]
        assert r["rc"] == 0 and sorted(p) == sorted(KEYS), r
        assert p["vec"] == (4 if d % 4 == 0 and ok else 1), r
        assert (p["bm"], p["bn"], p["ps"], p["kbm"], p["kbn"], p["kps"], p["max_lds"]) == (64, 16, 20, 32, 32, 36, MAX_LDS), r
        assert p["dp"] == (d + 15) // 16 * 16 and p["pd"] == p["dp"] + 4 and p["pd"] % 8 == 4, r       # an odd number of 16-byte units
        assert p["ps"] >= p["bn"] and p["ps"] % 8 == 4 and p["kps"] >= p["kbn"] and p["kps"] % 8 == 4, r
        assert p["lds_q"] == 4 * ((3 * p["bm"] + 4 * p["bn"]) * p["pd"] + 4 * p["bm"] * p["ps"]) <= MAX_LDS, r   # the sum of its parts
        assert p["lds_k"] == 4 * ((3 * p["kbm"] + 4 * p["kbn"]) * p["pd"] + 3 * p["kbm"] * p["kps"]) <= MAX_LDS, r
        assert p["grid_q"] == 15 * ((L + 63) // 64) and p["grid_k"] == 15 * ((S + 31) // 32), r
        assert p["ws"] == ws == 15 * L * 5 * 8, r                                                     # five doubles per query row
    p = attention_wide_plan(16, 8, 512, 512, 128)
    assert (p["lds_q"], p["lds_k"], p["grid_q"], p["grid_k"], p["ws"]) == (155648, 132096, 128 * 8, 128 * 16, 128 * 512 * 40)
    lib = _native.load()
    assert lib.bhg_attention_wide_ws_bytes(0, 1, 1) == 0 and lib.bhg_attention_wide_ws_bytes(1, 1, -3) == 0


def _launch(lib, B=2, H=2, L=70, S=70, d=72, strides=None, mask=None, mask_strides=None, ws=0x7100_0000_0000, ws_bytes=None, **over):
    """bhg_attention_wide_backward_vjp on host pointers that are never dereferenced."""
    fake = 0x7000_0000_0000
    p = {n: fake for n in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo")}
    p.update(over)
    if strides is None:
        strides = [s for rows in (L, S, S, L, L, S, S) for s in (H * rows * d, rows * d, d, 1)]
    st = (ctypes.c_longlong * 28)(*strides) if strides != "null" else None
    mst = (ctypes.c_longlong * 4)(*mask_strides) if mask_strides is not None else None
    if ws_bytes is None:
        ws_bytes = max(B, 0) * max(H, 0) * max(L, 0) * 40
    rc = lib.bhg_attention_wide_backward_vjp(p["q"], p["k"], p["v"], p["go"], p["aq"], p["ak"], p["av"], st, mask, mst, 0, 0.5, B, H, L, S, d,
                                             p["dq"], p["dk"], p["dv"], p["dgo"], ws, ws_bytes, None)
    return rc, lib.bhg_last_error()


def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words():
    lib = _native.load()
    cases = [(dict(L=0), "empty tensor"), (dict(S=0), "empty tensor"), (dict(d=0), "empty tensor"), (dict(B=0), "empty tensor"),
             (dict(H=-1), "empty tensor"), (dict(L=513), "more than 512 queries"), (dict(S=513), "more than 512 keys"),
             (dict(d=64), "fewer than 65 elements per head .*bhg_attention_tiled_backward_vjp"), (dict(d=129), "more than 128 elements per head"),
             (dict(B=1 << 20, H=1 << 10, L=512, S=4), "2\\^31 - 1 workgroups"), (dict(B=1 << 20, H=1 << 9, L=4, S=512), "2\\^31 - 1 workgroups")]
    for over, word in cases:
        shape = dict(B=2, H=2, L=70, S=70, d=72)
        shape.update(over)
        with pytest.raises(_native.NativeLibraryError, match=word):
            attention_wide_plan(**shape)
        rc, msg = _launch(lib, ws_bytes=1 << 62, **shape)
        assert rc == -1 and re.search(word, msg.decode()), (over, msg)
    attention_wide_plan(1 << 20, 1 << 10, 64, 32, 72)                          # 2^30 workgroups in both launches: inside
    with pytest.raises(_native.NativeLibraryError, match="more than 64 elements per head"):
        attention_tiled_plan(2, 2, 70, 70, 65)                                 # the sibling keeps its family and its words
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_attention_wide_plan(1, 1, 70, 70, 72, 1, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_attention_wide_plan(1, 1, 70, 70, 72, 1, buf, 8) == -1 and b"too small" in lib.bhg_last_error()


def test_the_launch_refuses_bad_arguments_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    contiguous = [s for rows in (70,) * 7 for s in (2 * rows * 72, rows * 72, 72, 1)]
    bad_last = [contiguous[:4 * i + 3] + [2] + contiguous[4 * i + 4:] for i in range(7)]       # a non-unit last stride, input by input
    cases = [(dict(**{n: None}), b"null pointer") for n in ("q", "k", "v", "go")] + [
        (dict(strides="null"), b"null pointer"), (dict(aq=None, ak=None, av=None), b"all three cotangents are NULL"),
        (dict(dq=None, dk=None, dv=None, dgo=None), b"all four outputs are NULL"), (dict(mask=fake), b"mask_strides"),
        (dict(ws=None), b"null pointer (workspace)"), (dict(ws_bytes=2 * 2 * 70 * 40 - 1), b"workspace too small"),
        (dict(ws=0x7100_0000_0004), b"8-byte aligned"), (dict(strides=contiguous[:2] + [-72] + contiguous[3:]), b"negative stride"),
    ] + [(dict(strides=s), b"last stride") for s in bad_last] + [
        (dict(**{n: fake + 4}), b"16-byte aligned") for n in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo")   # the vector path
    ] + [(dict(strides=bad_last[4], aq=None, dq=fake + 4), b"16-byte aligned")]                # the entries of a NULL input are ignored
    for over, word in cases:
        rc, msg = _launch(lib, **over)
        assert rc == -1 and word in msg, (over, msg)


def test_header_binding_and_exports_agree_for_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bhg.h")).read(), flags=re.S)
    lib, ab = _native.load(), ctypes.CDLL(_native.AB_LIB_PATH)
    for name, nargs, ret in NEW:
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert proto and len(proto.group(1).split(",")) == nargs == len(_native.SYMBOLS[name][1]), name
        assert _native.SYMBOLS[name][0] is ret and hasattr(lib, name) and hasattr(ab, name)
        assert getattr(lib, name).argtypes == _native.SYMBOLS[name][1]

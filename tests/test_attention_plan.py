"""Host logic of the fused attention double backward (csrc/bhg_attention.hip): the shape -> LDS plan map of at_plan, read through
bhg_attention_plan — the very function the launch path calls — and the refusals of bhg_attention_backward_vjp, which come before any
device access.  No GPU needed.

The plan keeps four L x S score matrices (row pitch ps) and four operand slots of max(L, S) x d (row pitch pd) in the LDS of one CU and
stages the seven operand matrices through the slots in five phases.  It is right only if that fits the 160 KiB a workgroup may take for
every shape of the family, the pitches hold the rows they pad (16-byte aligned on the vector path, where a score row is read 16 bytes at
a time up to S rounded up to 4), and vec = 4 exactly when d % 4 == 0 and the strides allow it.  The sweep runs in ONE child process."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from betty_amd import _native
from betty_amd.backend import attention_plan

MAX_LDS = 163840
NS = (1, 2, 15, 16, 17, 33, 50, 63, 64)
DS = (1, 3, 4, 8, 63, 64)
KEYS = ("vec", "ps", "pd", "rows", "slots", "phases", "grid", "lds", "max_lds")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import ctypes, json, re, sys
lib = ctypes.CDLL(sys.argv[1])
lib.bhg_attention_plan.restype = ctypes.c_int
lib.bhg_attention_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_size_t]
buf = ctypes.create_string_buffer(256)
for L, S, d, ok in json.loads(sys.argv[2]):
    rc = lib.bhg_attention_plan(3, 5, L, S, d, ok, buf, 256)
    row = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())} if rc == 0 else {}
    print(json.dumps({"shape": [L, S, d, ok], "rc": rc, "plan": row}), flush=True)
"""


@pytest.fixture(scope="module")
def sweep():
    """(L, S, d, vec_ok) -> plan dict for the grid: one child process."""
    shapes = [(L, S, d, ok) for L in NS for S in NS for d in DS for ok in (1, 0)]
    out = subprocess.run([sys.executable, "-c", _CHILD, _native.current_lib_path(), json.dumps(shapes)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert [tuple(r["shape"]) for r in rows] == shapes
    for r in rows:
        assert r["rc"] == 0 and sorted(r["plan"]) == sorted(KEYS), r
    return {tuple(r["shape"]): r["plan"] for r in rows}


def test_every_shape_of_the_grid_fits_the_lds_and_is_planned_soundly(sweep):
    worst = 0
    for (L, S, d, ok), p in sweep.items():
        at = (L, S, d, ok)
        assert p["vec"] == (4 if d % 4 == 0 and ok else 1), (at, p)                     # 16-byte accesses exactly when the conditions hold
        assert p["max_lds"] == MAX_LDS and 0 < p["lds"] <= MAX_LDS, (at, p)
        assert (p["slots"], p["phases"], p["grid"], p["rows"]) == (4, 5, 15, max(L, S)), (at, p)
        assert p["lds"] == 4 * (4 * L * p["ps"] + p["slots"] * p["rows"] * p["pd"]), (at, p)   # four score matrices and the slots, nothing else
        assert p["pd"] >= d and p["ps"] >= S, (at, p)
        if p["vec"] == 4:
            assert p["pd"] % 8 == 4, (at, p)            # an odd number of 16-byte units: 16 rows, 16 different bank groups
            assert p["ps"] % 4 == 0 and p["ps"] >= (S + 3) // 4 * 4 and p["ps"] % 32 != 0, (at, p)
            assert p["pd"] <= d + 4 and p["ps"] <= S + 11, (at, p)
        else:
            assert p["pd"] % 2 == 1 and p["ps"] % 2 == 1 and p["pd"] <= d + 1 and p["ps"] <= S + 1, (at, p)
        worst = max(worst, p["lds"])
    print(f"bhg_attention_plan: {len(sweep)} shapes, largest lds = {worst} bytes of {MAX_LDS}")
    assert worst == sweep[(64, 64, 64, 1)]["lds"] == 139264


def test_the_helper_reads_the_same_line():
    assert attention_plan(16, 12, 50, 50, 64) == {"vec": 4, "ps": 56, "pd": 68, "rows": 50, "slots": 4, "phases": 5, "grid": 192,
                                                  "lds": 4 * (4 * 50 * 56 + 4 * 50 * 68), "max_lds": MAX_LDS}
    assert attention_plan(1, 1, 64, 64, 64, vec_ok=False)["lds"] == 4 * 8 * 64 * 65
    p = attention_plan(3, 4, 10, 10, 16)
    assert (p["vec"], p["ps"], p["pd"], p["grid"]) == (4, 16, 20, 12)
    assert attention_plan(1, 1, 5, 60, 8)["ps"] == 68                                  # 64 would put the rows on one bank


def _launch(lib, B=2, H=2, L=4, S=4, d=8, strides=None, mask=None, mask_strides=None, **over):
    """bhg_attention_backward_vjp on host pointers that are never dereferenced."""
    fake = 0x7000_0000_0000
    p = {n: fake for n in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo")}
    p.update(over)
    if strides is None:
        strides = []
        for rows in (L, S, S, L, L, S, S):
            strides += [H * rows * d, rows * d, d, 1]
    st = (ctypes.c_longlong * 28)(*strides) if strides != "null" else None
    mst = (ctypes.c_longlong * 4)(*mask_strides) if mask_strides is not None else None
    rc = lib.bhg_attention_backward_vjp(p["q"], p["k"], p["v"], p["go"], p["aq"], p["ak"], p["av"], st, mask, mst, 0, 0.5, B, H, L, S, d, p["dq"],
                                        p["dk"], p["dv"], p["dgo"], None)
    return rc, lib.bhg_last_error()


def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words():
    lib = _native.load()
    cases = [(dict(L=0), "empty tensor"), (dict(S=0), "empty tensor"), (dict(d=0), "empty tensor"), (dict(B=0), "empty tensor"),
             (dict(H=-1), "empty tensor"), (dict(L=65), "more than 64 queries"), (dict(S=65), "more than 64 keys"),
             (dict(d=65), "more than 64 elements per head")]
    for over, word in cases:
        shape = dict(B=2, H=2, L=4, S=4, d=8)
        shape.update(over)
        with pytest.raises(_native.NativeLibraryError, match=word):
            attention_plan(**shape)
        rc, msg = _launch(lib, **shape)
        assert rc == -1 and word.encode() in msg, (over, msg)
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_attention_plan(1, 1, 4, 4, 4, 1, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_attention_plan(1, 1, 4, 4, 4, 1, buf, 0) == -1
    assert lib.bhg_attention_plan(1, 1, 4, 4, 4, 1, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan


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
    contiguous = []
    for rows in (4, 4, 4, 4, 4, 4, 4):
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
    for name, nargs in (("bhg_attention_plan", 8), ("bhg_attention_backward_vjp", 22)):
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert proto and len(proto.group(1).split(",")) == nargs == len(_native.SYMBOLS[name][1]), name
        assert _native.SYMBOLS[name][0] is ctypes.c_int and hasattr(lib, name)
        assert getattr(_native.load(), name).argtypes == _native.SYMBOLS[name][1]
    ab = ctypes.CDLL(_native.AB_LIB_PATH)
    assert hasattr(ab, "bhg_attention_plan") and hasattr(ab, "bhg_attention_backward_vjp")

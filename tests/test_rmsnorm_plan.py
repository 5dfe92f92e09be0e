"""Host logic of the fused RMS-norm double backward (csrc/bhg_rmsnorm.hip): the shape -> launch geometry map of rms_plan, read through
bhg_rmsnorm_plan — the very function the launch path calls — and the refusals of bhg_rmsnorm_backward_vjp, which come before any device
access.  No GPU needed.

The plan gives a row `tpr` threads (a power of two), puts `rows` = 256 / tpr rows side by side as one row group, and cuts the `groups`
row groups into `slices` slices of `gps` groups: slice s is the rows [s gps rows, min(M, (s + 1) gps rows)).  It is right only if the
slices cover the rows with none empty, there are at most `max_slices` — what fills the chip at the register count of the kernel instance
that runs, NOT layer norm's 64 —, the workspace is exactly what the slices write, and the threads of a row cover its D elements with the
vectors of that instance.  The floor: a slice costs 16 D bytes of partial sums, a row 20 D bytes, so a slice holds at least 8 rows
whenever there is more than one slice (gps * rows >= 8, hence slices <= ceil(M / 8)): the partials stay at about 10 % of the traffic.
The map is closed-form: nothing is searched."""
import ctypes

import pytest

from betty_amd import _native
from betty_amd.backend import rmsnorm_plan

MIN_ROWS = 8
MS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 800, 4096, 65536, 2 ** 20 + 1)
DS = (1, 2, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 255, 256, 257, 768, 1000, 1001, 1024, 2049, 4096, 8188, 8191, 8192)
KEYS = ("vec", "tpr", "rows", "nv", "inst", "groups", "gps", "slices", "max_slices", "ws")
# workgroups of the row pass a CU holds, by (vec, inst): the waves per SIMD the header of csrc/bhg_rmsnorm.hip records
PER_CU = {(4, 2): 4, (4, 4): 3, (4, 8): 1, (1, 2): 8, (1, 8): 4, (1, 32): 1}


def test_every_shape_of_the_grid_is_planned_soundly():
    lib = _native.load()
    capped = set()
    for M in MS:
        for D in DS:
            p, at = rmsnorm_plan(M, D), (M, D)
            assert sorted(p) == sorted(KEYS), (at, p)
            assert p["vec"] == (4 if D % 4 == 0 else 1), (at, p)
            # threads of a row: a power of two, whole rows side by side, and the instance's vectors cover the row
            assert p["tpr"] in (1, 2, 4, 8, 16, 32, 64, 128, 256) and p["rows"] * p["tpr"] == 256, (at, p)
            nvec = D // p["vec"]
            assert p["nv"] == -(-nvec // p["tpr"]) and p["nv"] <= p["inst"], (at, p)
            assert p["inst"] in ((2, 4, 8) if p["vec"] == 4 else (2, 8, 32)), (at, p)
            assert p["inst"] == 2 or p["rows"] == 1, (at, p)          # rows side by side only with two vectors per thread (the kernel's LDS)
            assert p["tpr"] == 1 or 2 * nvec > p["tpr"], (at, p)
            # row groups cover the rows, none empty
            assert p["groups"] == -(-M // p["rows"]), (at, p)
            # slices: cover the groups, none empty, at most what fills the chip
            assert p["max_slices"] == 256 * PER_CU[(p["vec"], p["inst"])] > 64, (at, p)
            assert 1 <= p["slices"] <= p["max_slices"], (at, p)
            assert p["gps"] >= 1 and p["slices"] == -(-p["groups"] // p["gps"]), (at, p)
            assert (p["slices"] - 1) * p["gps"] < p["groups"] and (p["slices"] - 1) * p["gps"] * p["rows"] < M, (at, p)   # the last slice's first row exists
            # the floor on rows per slice
            assert p["slices"] == 1 or p["gps"] * p["rows"] >= MIN_ROWS, (at, p)
            assert p["slices"] <= -(-M // MIN_ROWS), (at, p)
            # the closed form: as many slices as the cap and the floor allow, the groups spread evenly over them
            allowed = min(p["max_slices"], max(1, p["groups"] // -(-MIN_ROWS // p["rows"])))
            assert p["gps"] == -(-p["groups"] // allowed), (at, p)
            # where the cap binds (the floor alone would allow more slices) more than half of it is used: gps = ceil(groups / cap)
            if p["groups"] // -(-MIN_ROWS // p["rows"]) > p["max_slices"]:
                assert 2 * p["slices"] > p["max_slices"], (at, p)
                capped.add((p["vec"], p["inst"]))
            # workspace: exactly what the plan writes
            assert p["ws"] == 8 * p["slices"] * D == lib.bhg_rmsnorm_ws_bytes(M, D), (at, p)
    assert capped == set(PER_CU), capped                             # the cap is reached for large M, by every kernel instance


def test_the_helper_reads_the_same_line():
    assert rmsnorm_plan(800, 768) == {"vec": 4, "tpr": 128, "rows": 2, "nv": 2, "inst": 2, "groups": 400, "gps": 4, "slices": 100,
                                      "max_slices": 1024, "ws": 8 * 100 * 768}
    assert rmsnorm_plan(65536, 4096) == {"vec": 4, "tpr": 256, "rows": 1, "nv": 4, "inst": 4, "groups": 65536, "gps": 86, "slices": 763,
                                         "max_slices": 768, "ws": 8 * 763 * 4096}
    assert rmsnorm_plan(7, 8192) == {"vec": 4, "tpr": 256, "rows": 1, "nv": 8, "inst": 8, "groups": 7, "gps": 7, "slices": 1,
                                     "max_slices": 256, "ws": 8 * 8192}
    assert rmsnorm_plan(4096, 8192)["slices"] == 256 and rmsnorm_plan(4096, 8192)["gps"] == 16
    p = rmsnorm_plan(7, 8191)
    assert (p["vec"], p["tpr"], p["nv"], p["inst"]) == (1, 256, 32, 32)
    p = rmsnorm_plan(2 ** 20 + 1, 8)
    assert (p["tpr"], p["rows"], p["groups"], p["gps"], p["slices"], p["max_slices"]) == (1, 256, 4097, 5, 820, 1024)


def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words():
    lib = _native.load()
    fake = 0x7000_0000_0000   # never dereferenced: every refusal comes before any device access
    for (M, D), word in [((4, 0), "empty tensor"), ((0, 4), "empty tensor"), ((-1, 4), "empty tensor"), ((4, -4), "empty tensor"),
                         ((4, 8193), "more than 8192 elements per row"), ((2 ** 40 + 1, 4), "more than 2^40 rows")]:
        with pytest.raises(_native.NativeLibraryError, match=word.replace("^", r"\^")):
            rmsnorm_plan(M, D)
        rc = lib.bhg_rmsnorm_backward_vjp(fake, fake, fake, fake, fake, fake, M, D, fake, fake, fake, fake, 1 << 30, None)
        assert rc == -1 and word.encode() in lib.bhg_last_error(), (M, D, lib.bhg_last_error())
        assert lib.bhg_rmsnorm_ws_bytes(M, D) == 0
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_rmsnorm_plan(4, 4, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_rmsnorm_plan(4, 4, buf, 0) == -1
    assert lib.bhg_rmsnorm_plan(4, 4, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan


def test_the_launch_refuses_bad_pointers_and_workspaces_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    names = ["x", "gy", "a", "gamma", "rstd", "b", "dx", "dgy", "dgamma", "ws"]

    def call(M=40, D=8, ws_bytes=None, **over):
        p = {n: fake for n in names}
        p.update(over)
        ws_bytes = lib.bhg_rmsnorm_ws_bytes(M, D) if ws_bytes is None else ws_bytes
        rc = lib.bhg_rmsnorm_backward_vjp(p["x"], p["gy"], p["a"], p["gamma"], p["rstd"], p["b"], M, D, p["dx"], p["dgy"], p["dgamma"],
                                          p["ws"], ws_bytes, None)
        return rc, lib.bhg_last_error()

    for required in ("x", "gy", "rstd", "dx", "dgy"):
        rc, msg = call(**{required: None})
        assert rc == -1 and b"null pointer" in msg, (required, msg)
    rc, msg = call(ws=None)
    assert rc == -1 and b"dgamma needs a workspace" in msg, msg
    assert lib.bhg_rmsnorm_ws_bytes(40, 8) == 8 * 8
    rc, msg = call(ws_bytes=8 * 8 - 1)
    assert rc == -1 and b"workspace smaller" in msg, msg
    rc, msg = call(M=4096, D=8192, ws_bytes=8 * 255 * 8192)          # 256 slices: what sufficed for fewer rows does not
    assert rc == -1 and b"workspace smaller" in msg, msg
    rc, msg = call(ws=fake + 4)
    assert rc == -1 and b"8-byte aligned" in msg, msg
    rc, msg = call(gamma=None)                                       # b and dgamma given
    assert rc == -1 and b"b and dgamma need gamma" in msg, msg
    rc, msg = call(gamma=None, b=None)
    assert rc == -1 and b"b and dgamma need gamma" in msg, msg
    rc, msg = call(gamma=None, dgamma=None, ws=None, ws_bytes=0)
    assert rc == -1 and b"b and dgamma need gamma" in msg, msg
    for row_tensor in ("x", "gy", "a", "dx", "dgy"):
        rc, msg = call(**{row_tensor: fake + 4})
        assert rc == -1 and b"16-byte aligned" in msg, (row_tensor, msg)

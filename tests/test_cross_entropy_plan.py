"""bhg_cross_entropy_plan / backend.cross_entropy_plan (host logic only: no GPU): each regime is reached at the shapes it is named for,
every edge one below, at and one above, the workspace is what bhg_cross_entropy_ws_bytes says, every refusal carries its message, and the
plan refuses what the launch refuses in the same words."""
import ctypes

import pytest

from betty_amd import _native
from betty_amd.backend import cross_entropy_plan

PER_CU = {(4, 2): 7, (4, 4): 6, (4, 8): 4, (4, 16): 2, (4, 32): 1, (1, 2): 8, (1, 8): 6, (1, 32): 2}   # csrc/bhg_cross_entropy.hip, header


def test_the_shapes_the_regimes_are_named_for():
    for N, C in [(16, 8), (800, 10), (4096, 1000), (64, 10), (37, 260)]:                      # the classifiers of the examples
        assert cross_entropy_plan(N, C)["regime"] == "short", (N, C)
    for N, C in [(8192, 32000), (4096, 4096), (256, 32768), (8, 16384), (1, 2048)]:
        p = cross_entropy_plan(N, C)
        assert p["regime"] == "row" and p["tpr"] == 256 and p["rows"] == 1 and p["launches"] == 1, (N, C, p)
    for N, C in [(2048, 128256), (8, 128256), (8192, 151936), (8, 32000), (2, 262144)]:        # the vocabulary regime
        p = cross_entropy_plan(N, C)
        assert p["regime"] == "split" and p["launches"] == 2 and p["inst"] == 0, (N, C, p)
    assert cross_entropy_plan(8, 128256)["slices"] == 126 and cross_entropy_plan(8, 128256)["wgs"] == 1008
    assert cross_entropy_plan(2048, 128256)["slices"] == 1    # the rows alone fill the chip: two passes, one workgroup per row each


def test_the_helper_reads_the_same_line():
    assert cross_entropy_plan(4096, 1000) == {"regime": "short", "vec": 4, "tpr": 128, "rows": 2, "nv": 2, "inst": 2, "groups": 2048, "gps": 2,
                                              "slices": 1, "chunk": 1000, "wgs": 1024, "max_wgs": 1792, "launches": 1, "ws": 0}
    assert cross_entropy_plan(4096, 1000, True) == {"regime": "short", "vec": 4, "tpr": 128, "rows": 2, "nv": 2, "inst": 2, "groups": 2048,
                                                    "gps": 2, "slices": 1, "chunk": 1000, "wgs": 1024, "max_wgs": 1792, "launches": 2, "ws": 8 * 1024}
    assert cross_entropy_plan(8192, 32000) == {"regime": "row", "vec": 4, "tpr": 256, "rows": 1, "nv": 32, "inst": 32, "groups": 8192, "gps": 32,
                                               "slices": 1, "chunk": 32000, "wgs": 256, "max_wgs": 256, "launches": 1, "ws": 0}
    assert cross_entropy_plan(3, 32773, True) == {"regime": "split", "vec": 1, "tpr": 256, "rows": 1, "nv": 4, "inst": 0, "groups": 3, "gps": 1,
                                                  "slices": 33, "chunk": 1024, "wgs": 99, "max_wgs": 1280, "launches": 2, "ws": 8 * 99}


def test_edges_one_below_at_and_one_above():
    reg = lambda N, C: cross_entropy_plan(N, C)["regime"]   # noqa: E731
    # short rows end where a row takes the whole workgroup: 256 vectors (two per thread at 128 threads)
    assert [reg(100, C) for C in (1020, 1024, 1028)] == ["short", "short", "row"]
    assert [reg(100, C) for C in (255, 257)] == ["short", "row"] and cross_entropy_plan(100, 255)["vec"] == 1
    # threads per row double at every power of two of vectors; rows side by side halve
    for nvec, tpr in [(2, 1), (3, 2), (4, 2), (5, 4), (64, 32), (65, 64), (128, 64), (129, 128), (256, 128)]:
        p = cross_entropy_plan(100, 4 * nvec)
        assert (p["vec"], p["tpr"], p["rows"]) == (4, tpr, 256 // tpr), (nvec, p)
    for C, tpr in [(2, 1), (3, 2), (5, 4), (63, 32), (65, 64), (127, 64), (129, 128), (255, 128)]:
        p = cross_entropy_plan(100, C)
        assert (p["vec"], p["tpr"], p["rows"]) == (1, tpr, 256 // tpr), (C, p)
    # kernel instances, 16-byte accesses: nv = 2 | 3, 4 | 5, 8 | 9, 16 | 17, 32
    for C, inst in [(2048, 2), (2052, 4), (4096, 4), (4100, 8), (8192, 8), (8196, 16), (16384, 16), (16388, 32), (32768, 32)]:
        p = cross_entropy_plan(300, C)
        assert (p["regime"], p["vec"], p["inst"]) == ("row", 4, inst), (C, p)
    for C, inst in [(511, 2), (513, 8), (2047, 8), (2049, 32), (8191, 32)]:
        p = cross_entropy_plan(100, C)
        assert (p["regime"], p["vec"], p["inst"]) == ("row", 1, inst), (C, p)
    # the register-resident bounds
    assert [reg(300, C) for C in (32764, 32768, 32769, 32772)] == ["row", "row", "split", "split"]
    assert [reg(100, C) for C in (8190, 8191, 8193)] == ["row", "row", "split"]
    # few rows: split below 160 rows, but only rows of more than 16384 elements
    assert [reg(N, 32768) for N in (159, 160, 161)] == ["split", "row", "row"]
    assert [reg(8, C) for C in (16380, 16384, 16388)] == ["row", "row", "split"]
    # the family
    assert reg(1, 262144) == "split"
    with pytest.raises(_native.NativeLibraryError, match="more than 262144 classes"):
        cross_entropy_plan(1, 262145)
    assert reg(2 ** 40, 8) == "short"


def test_workgroup_caps_and_workspace():
    lib = _native.load()
    capped = set()
    for C in (1, 8, 9, 260, 1000, 1001, 2048, 2052, 2049, 4100, 8196, 16400, 32768, 8191, 32773, 128256, 262144):
        for N in (1, 7, 159, 160, 161, 1000, 1793, 2 ** 17, 2 ** 22 + 3):
            for scalar in (False, True):
                p = cross_entropy_plan(N, C, scalar)
                assert p["ws"] == lib.bhg_cross_entropy_ws_bytes(N, C, int(scalar)), (N, C, p)
                assert 1 <= p["wgs"] <= p["max_wgs"], p
                if p["regime"] == "split":
                    assert p["max_wgs"] == 1280 and p["ws"] == 8 * N * p["slices"] and p["chunk"] * p["slices"] >= C > p["chunk"] * (p["slices"] - 1), p
                    assert p["slices"] <= 256 and p["chunk"] % 1024 == 0 and p["wgs"] == min(1280, N * p["slices"]), p
                    continue
                assert p["max_wgs"] == 256 * PER_CU[(p["vec"], p["inst"])], p
                assert p["groups"] == -(-N // p["rows"]) and p["wgs"] == -(-p["groups"] // p["gps"]) and p["gps"] * (p["wgs"] - 1) < p["groups"], p
                assert p["ws"] == (8 * p["wgs"] if scalar else 0), p
                if p["groups"] > p["max_wgs"]:
                    capped.add((p["vec"], p["inst"]))
                    assert 2 * p["wgs"] > p["max_wgs"], p
    assert capped == set(PER_CU), capped   # the cap is reached for large N, by every kernel instance


def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words():
    lib = _native.load()
    fake = 0x7000_0000_0000   # never dereferenced: every refusal comes before any device access
    for (N, C), word in [((4, 0), "empty tensor"), ((0, 4), "empty tensor"), ((-1, 4), "empty tensor"), ((4, -4), "empty tensor"),
                         ((4, 262145), "more than 262144 classes"), ((2 ** 40 + 1, 4), "more than 2^40 rows")]:
        for scalar in (0, 1):
            with pytest.raises(_native.NativeLibraryError, match=word.replace("^", r"\^")):
                cross_entropy_plan(N, C, scalar)
            rc = lib.bhg_cross_entropy_backward_vjp(fake, fake, fake, scalar, None, fake, N, C, -100, fake, fake, fake, 1 << 30, None)
            assert rc == -1 and word.encode() in lib.bhg_last_error(), (N, C, lib.bhg_last_error())
            assert lib.bhg_cross_entropy_ws_bytes(N, C, scalar) == 0
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_cross_entropy_plan(4, 4, 0, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_cross_entropy_plan(4, 4, 0, buf, 0) == -1
    assert lib.bhg_cross_entropy_plan(4, 4, 0, buf, 8) == -1 and b"too small" in lib.bhg_last_error()   # a cut line would parse as another plan


def test_the_launch_refuses_bad_pointers_and_workspaces_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    names = ["lsm", "y", "g", "denom", "a", "dz", "dg", "ws"]

    def call(N=40, C=8, scalar=1, ws_bytes=None, **over):
        p = {n: fake for n in names}
        p.update(over)
        ws_bytes = lib.bhg_cross_entropy_ws_bytes(N, C, scalar) if ws_bytes is None else ws_bytes
        rc = lib.bhg_cross_entropy_backward_vjp(p["lsm"], p["y"], p["g"], scalar, p["denom"], p["a"], N, C, -100, p["dz"], p["dg"], p["ws"], ws_bytes, None)
        return rc, lib.bhg_last_error()

    for required in ("lsm", "y", "g", "a"):
        rc, msg = call(**{required: None})
        assert rc == -1 and b"null pointer" in msg, (required, msg)
    rc, msg = call(dz=None, dg=None)
    assert rc == -1 and b"both outputs are NULL" in msg, msg
    rc, msg = call(scalar=0)                                         # denom given with a per-row g
    assert rc == -1 and b"denom needs a scalar g" in msg, msg
    assert lib.bhg_cross_entropy_ws_bytes(40, 8, 1) == 8 and lib.bhg_cross_entropy_ws_bytes(40, 8, 0) == 0
    rc, msg = call(ws=None)
    assert rc == -1 and b"needs a workspace" in msg, msg
    rc, msg = call(ws_bytes=7)
    assert rc == -1 and b"workspace smaller" in msg, msg
    rc, msg = call(N=3, C=32773, scalar=0, denom=None, ws_bytes=8 * 99 - 1)   # split rows: the partials of s
    assert rc == -1 and b"workspace smaller" in msg, msg
    rc, msg = call(N=3, C=32773, scalar=0, denom=None, ws=None)
    assert rc == -1 and b"needs a workspace" in msg, msg
    rc, msg = call(ws=fake + 4)
    assert rc == -1 and b"8-byte aligned" in msg, msg
    for row_tensor in ("lsm", "a", "dz"):
        rc, msg = call(**{row_tensor: fake + 4})
        assert rc == -1 and b"16-byte aligned" in msg, (row_tensor, msg)

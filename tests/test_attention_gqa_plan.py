"""Host logic of the grouped-query attention double backward (csrc/bhg_attention_gqa.hip): the plan line of bhg_attention_gqa_plan — the
very function the launch calls — for three shapes, and every refusal of the plan and of bhg_attention_gqa_backward_vjp, which come before
any device access.  No GPU needed."""
import ctypes

import pytest

from betty_amd import _native
from betty_amd.backend import attention_gqa_plan

MAX_LDS = 163840


@pytest.mark.parametrize("shape,vec", [((16, 32, 4, 512, 512, 64), 4), ((2, 6, 2, 5, 7, 3), 1), ((3, 8, 1, 20, 100, 20), 4)])
def test_the_plan_packs_the_group_into_the_query_rows(shape, vec):
    B, Hq, Hkv, L, S, d = shape
    p = attention_gqa_plan(*shape)
    g, dp = Hq // Hkv, (d + 15) // 16 * 16
    assert (p["g"], p["rows"], p["vec"], p["bm"], p["bn"], p["ps"], p["dp"], p["pd"]) == (g, g * L, vec, 64, 32, 36, dp, dp + 4), p
    assert p["grid_q"] == B * Hkv * ((g * L + 63) // 64) and p["grid_k"] == B * Hkv * ((S + 31) // 32), p   # 8 x 20 rows: 3 tiles, not 8
    operands = (3 * 64 + 4 * 32) * p["pd"]
    assert p["lds_q"] == 4 * (operands + 4 * 64 * 36) and p["lds_k"] == 4 * (operands + 3 * 64 * 36) and p["lds_q"] <= p["max_lds"] == MAX_LDS, p
    assert p["ws"] == 40 * B * Hq * L == _native.load().bhg_attention_gqa_ws_bytes(B, Hq, L), p
    assert attention_gqa_plan(*shape, vec_ok=False)["vec"] == 1
    assert attention_gqa_plan(1, 8, 1, 512, 512, 64)["lds_q"] == 123904


def _launch(lib, B=2, Hq=4, Hkv=2, L=70, S=70, d=8, strides=None, mask=None, mask_strides=None, ws=0x7100_0000_0000, ws_bytes=1 << 62, **over):
    """bhg_attention_gqa_backward_vjp on host pointers that are never dereferenced."""
    fake = 0x7000_0000_0000
    p = {n: fake for n in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo")}
    p.update(over)
    if strides is None:
        strides = [s for H, rows in ((Hq, L), (Hkv, S), (Hkv, S), (Hq, L), (Hq, L), (Hkv, S), (Hkv, S)) for s in (H * rows * d, rows * d, d, 1)]
    st = (ctypes.c_longlong * 28)(*strides) if strides != "null" else None
    mst = (ctypes.c_longlong * 4)(*mask_strides) if mask_strides is not None else None
    rc = lib.bhg_attention_gqa_backward_vjp(p["q"], p["k"], p["v"], p["go"], p["aq"], p["ak"], p["av"], st, mask, mst, 0, 0.5, B, Hq, Hkv, L, S,
                                            d, p["dq"], p["dk"], p["dv"], p["dgo"], ws, ws_bytes, None)
    return rc, lib.bhg_last_error()


SHAPES_REFUSED = [(dict(L=0), "empty tensor"), (dict(S=0), "empty tensor"), (dict(d=0), "empty tensor"), (dict(B=0), "empty tensor"),
                  (dict(Hq=-2), "empty tensor"), (dict(Hkv=0), "empty tensor"), (dict(L=513), "more than 512 queries"),
                  (dict(S=513), "more than 512 keys"), (dict(d=65), "more than 64 elements per head"),
                  (dict(Hq=5), "not a multiple of the number of key/value heads"), (dict(Hq=2), "bhg_attention_tiled_backward_vjp"),
                  (dict(Hq=18, L=512), "more than 4096 packed query rows"),
                  (dict(B=1 << 20, Hq=1 << 11, Hkv=1 << 10, L=512, S=4), "2\\^31 - 1 workgroups"),
                  (dict(B=1 << 20, Hq=1 << 10, Hkv=1 << 9, L=4, S=512), "2\\^31 - 1 workgroups")]


@pytest.mark.parametrize("over,word", SHAPES_REFUSED, ids=[f"{list(o)[0]}={list(o.values())[0]}" for o, _ in SHAPES_REFUSED])
def test_shapes_the_launch_refuses_are_refused_by_the_plan_with_the_same_words(over, word):
    shape = dict(B=2, Hq=4, Hkv=2, L=70, S=70, d=8)
    shape.update(over)
    with pytest.raises(_native.NativeLibraryError, match=word):
        attention_gqa_plan(*shape.values())
    rc, msg = _launch(_native.load(), **shape)
    assert rc == -1 and word.replace("\\", "").encode() in msg, (over, msg)


def test_the_launch_refuses_bad_arguments_before_any_device_access():
    lib = _native.load()
    fake = 0x7000_0000_0000
    contiguous = [s for H in (4, 2, 2, 4, 4, 2, 2) for s in (H * 70 * 8, 70 * 8, 8, 1)]
    cases = [(dict(q=None), b"null pointer"), (dict(k=None), b"null pointer"), (dict(v=None), b"null pointer"), (dict(go=None), b"null pointer"),
             (dict(strides="null"), b"null pointer"), (dict(aq=None, ak=None, av=None), b"all three cotangents are NULL"),
             (dict(dq=None, dk=None, dv=None, dgo=None), b"all four outputs are NULL"), (dict(mask=fake), b"mask_strides"),
             (dict(ws=None), b"null pointer (workspace)"), (dict(ws_bytes=2 * 4 * 70 * 40 - 1), b"workspace too small"),
             (dict(ws=0x7100_0000_0004), b"8-byte aligned"), (dict(strides=contiguous[:2] + [-8] + contiguous[3:]), b"negative stride"),
             (dict(mask=fake, mask_strides=[0, -1, 0, 1]), b"negative stride")]
    cases += [(dict(strides=contiguous[:4 * i + 3] + [2] + contiguous[4 * i + 4:]), b"last stride") for i in range(7)]
    cases += [({name: fake + 4}, b"16-byte aligned") for name in ("q", "k", "v", "go", "aq", "ak", "av", "dq", "dk", "dv", "dgo")]
    for over, word in cases:
        rc, msg = _launch(lib, **over)
        assert rc == -1 and word in msg, (over, msg)
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_attention_gqa_plan(1, 2, 1, 70, 70, 4, 1, None, 256) == -1 and b"NULL" in lib.bhg_last_error()
    assert lib.bhg_attention_gqa_plan(1, 2, 1, 70, 70, 4, 1, buf, 8) == -1 and b"too small" in lib.bhg_last_error()
    assert lib.bhg_attention_gqa_ws_bytes(0, 2, 1) == 0 and lib.bhg_attention_gqa_ws_bytes(1, 2, -3) == 0


"""Fully masked rows through the five attention entry points — bhg_attention_backward_vjp, bhg_attention_tiled_backward_vjp,
bhg_attention_wide_backward_vjp, bhg_attention_fused_forward and bhg_attention_fused_backward — by the C ABI, against
tests/attention_ref.py evaluated in float64 on the very fp32 inputs.  A row whose keys are all masked has probability zero, as on torch's
math path (tests/test_attention_ref.py holds the reference to that): its rows of the query-side outputs are exact zeros and it adds
nothing to the key-side ones.  Before, such a row was NaN and, the key-side outputs being sums over query rows, turned dk, dv (gk, gv)
of its whole (batch, head) into NaN.

Shapes (B x H x L x S x d), the smallest at which the tiling matters: 2 x 2 x 40 x 64 x 8 (short); 2 x 2 x 130 x 130 x 8 and
2 x 1 x 65 x 65 x 3, scalar reads (tiled and fused); 2 x 2 x 130 x 130 x 80 (wide).  Masks, each on every shape:
    left_pad_causal   a (B, 1, 1, S) zero-stride padding mask with the first p keys -inf for batch element 1 only, plus the causal flag;
                      p = 70 at 130 tokens (a whole 64-row query tile and part of the next are dead, and the key launch streams dead query
                      tiles), p = 5 otherwise.  Rows 0 .. p - 1 of batch element 1 are dead, batch element 0 is untouched.
    one_row           a full random mask with one row -inf in one head: row 64 at 130 tokens (the first row of the second query tile),
                      row 3 otherwise.
    dead_head         a padding mask that removes every key of batch element 1: every output of its heads is exact zeros.
    dead_then_live    the full random mask with one row (the same one) masked on its first keys and live on the last ones: it must be
                      finite, NOT zero, and within the gate — a fix that zeroes a row because a leading key tile was dead fails here.  64 keys
                      are masked where that leaves 8 live ones, otherwise all but 8 (56 of 64, 57 of 65): one live key would make P = 1
                      and dq, gq exact zeros in the reference, and the row could not be told from a zeroed one.

Per output (o, gq, gk, gv of the fused pair; dq, dk, dv, dgo of the three double backwards, with aq, ak, av all given): everything finite;
where the reference is exact zeros by construction — the dead rows of the query-side outputs, every output of a dead head — the kernel's
output is exact zeros too (every term carries the factor P = 0: nothing rounds); per (b, h) slice max|got - want| <= 2e-5 max|want_slice|,
the gate of the sibling files, which for an all-zero slice asks for zeros again.  The fused statistics of a dead row are
(mx, l) = (-inf, 0), the workspace row of the tiled and wide kernels [-inf, 0, 0, 0, 0].  As in the sibling files the outputs, statistics
and workspaces are slices of sentinel-padded, NaN-filled buffers: written inside their bounds only, every element written, the inputs
bit-equal afterwards, a second run the same bits.  Observed: profiles/attention_masked_rows_fp64.txt."""
import ctypes
import functools

import pytest
import torch

import attention_ref
from betty_amd import _native

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
NEG = float("-inf")

# (label, B, H, L, S, d) and the entry points that take the shape
SHORT = ("short", 2, 2, 40, 64, 8)
TILED = ("tiled", 2, 2, 130, 130, 8)
TILED_SCALAR = ("tiled scalar", 2, 1, 65, 65, 3)
WIDE = ("wide", 2, 2, 130, 130, 80)
KERNELS = {SHORT: ("bhg_attention",), TILED: ("bhg_attention_tiled", "fused"), TILED_SCALAR: ("bhg_attention_tiled", "fused"),
           WIDE: ("bhg_attention_wide",)}
MASKS = ["left_pad_causal", "one_row", "dead_head", "dead_then_live"]
RUNS = [(case, kernel) for case, kernels in KERNELS.items() for kernel in kernels]
_id = lambda c: f"{c[0].replace(' ', '_')}-{'x'.join(map(str, c[1:]))}" if isinstance(c, tuple) else c   # noqa: E731


def pad_keys(S):
    return 70 if S == 130 else 5


def the_row(L):
    return 64 if L == 130 else 3


def leading_keys(S):
    """How many leading keys dead_then_live masks in its row: 64 where that leaves at least 8 live ones, otherwise all but 8."""
    return min(64, S - 8)


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(q, k, v, go, aq, ak, av) on the host, fp32; computed once per case, shared, never written."""
    _, B, H, L, S, d = case
    g = torch.Generator().manual_seed(((B * 67 + H) * 67 + L) * 4489 + S * 67 + d + 1)
    q, go, aq = (torch.randn(B, H, L, d, generator=g) for _ in range(3))
    k, v, ak, av = (torch.randn(B, H, S, d, generator=g) for _ in range(4))
    return q, k, v, go, aq, ak, av


@functools.lru_cache(maxsize=None)
def host_mask(case, kind):
    """(mask as the kernel gets it: a (B, H, L, S) view, fp32; causal).  The padding masks keep their zero strides."""
    _, B, H, L, S, d = case
    if kind in ("left_pad_causal", "dead_head"):
        m = torch.zeros(B, 1, 1, S)
        m[1, :, :, :(pad_keys(S) if kind == "left_pad_causal" else S)] = NEG
        m = m.expand(B, H, L, S)
        assert all(s == 0 for s, n in zip(m.stride()[1:3], (H, L)) if n > 1)   # read in place: no (B, H, L, S) copy
        return m, kind == "left_pad_causal"
    m = torch.randn(B, H, L, S, generator=torch.Generator().manual_seed(L * 1000 + S + d))
    m[1, 0, the_row(L), :(S if kind == "one_row" else leading_keys(S))] = NEG
    return m, False


@functools.lru_cache(maxsize=None)
def dead_rows(case, kind):
    """(B, H, L) bool: the rows with no live key, from the scores themselves."""
    q, k = (t.double() for t in host_inputs(case)[:2])
    mask, causal = host_mask(case, kind)
    return (attention_ref.scores(q, k, mask.double(), causal, 1.0) == NEG).all(-1)


@functools.lru_cache(maxsize=None)
def wanted(case, kind):
    """((o, gq, gk, gv), (dq, dk, dv, dgo)) in float64."""
    q, k, v, go, aq, ak, av = (t.double() for t in host_inputs(case))
    mask, causal = host_mask(case, kind)
    mask = mask.double()
    first = (attention_ref.attention(q, k, v, mask, causal),) + tuple(attention_ref.attention_backward(q, k, v, go, mask, causal))
    return first, tuple(attention_ref.attention_backward_vjp(q, k, v, go, aq, ak, av, mask=mask, causal=causal))


def gate(case, kind, names, got, want, query_side, label):
    """Finite, exact zeros where the reference has them by construction, and the gate per (b, h) slice; returns the printed line."""
    dead = dead_rows(case, kind)
    dead_heads = dead.all(-1)                                            # (B, H)
    line = []
    for name, g, w in zip(names, got, want):
        assert bool(torch.isfinite(g).all()), (label, case, kind, name, "not finite")
        if name in query_side:
            assert not w[dead].any() and not g[dead].any(), (label, case, kind, name, "a dead row is not exact zeros")
        assert not w[dead_heads].any() and not g[dead_heads].any(), (label, case, kind, name, "a dead head is not exact zeros")
        err = (g.double() - w).abs().amax(dim=(2, 3))
        top = w.abs().amax(dim=(2, 3))
        assert bool((top > 0).eq(~dead_heads).all()), (label, case, kind, name)      # an all-zero slice is a dead head, nothing else
        assert bool((err <= GATE * top).all()), (label, case, kind, name, float((err / top.clamp_min(1e-300)).max()))
        live = top > 0
        line.append(f"{name} {float((err[live] / top[live]).max()):.3e}")
    if kind == "dead_then_live":                                         # live behind dead key tiles: finite above, and not zeroed
        row = (1, 0, the_row(case[3]))
        assert not dead[row]
        for name, g, w in zip(names, got, want):
            if name in query_side:
                assert bool(w[row].any()) and bool(g[row].any()), (label, case, kind, name, "the row with live keys behind dead ones is zero")
    return f"attention masked rows {label} {_id(case)} {kind}: " + "  ".join(line) + "  (worst (b, h) slice of max|got - want| / max|want_slice|)"


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("case", list(KERNELS), ids=_id)
def test_the_reference_has_the_dead_rows_and_the_gate_can_exclude_no_case(case, kind):
    """CPU: the masks kill the rows they are meant to, the reference is finite with exact zeros there, and rounded to fp32 it passes."""
    _, B, H, L, S, d = case
    dead = dead_rows(case, kind)
    expect = torch.zeros(B, H, L, dtype=torch.bool)
    if kind == "left_pad_causal":
        expect[1, :, :pad_keys(S)] = True
    elif kind == "one_row":
        expect[1, 0, the_row(L)] = True
    elif kind == "dead_head":
        expect[1] = True
    assert torch.equal(dead, expect)
    first, second = wanted(case, kind)
    gate(case, kind, ("o", "gq", "gk", "gv"), [w.float() for w in first], first, ("o", "gq"), "fp64 rounded to fp32")
    gate(case, kind, ("dq", "dk", "dv", "dgo"), [w.float() for w in second], second, ("dq", "dgo"), "fp64 rounded to fp32")


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_inputs(case):
    return tuple(t.to(DEV) for t in host_inputs(case))


@functools.lru_cache(maxsize=None)
def device_mask(case, kind):
    """The mask on the device with the strides it has on the host (a padding mask stays a zero-stride view)."""
    _, B, H, L, S, d = case
    mask, causal = host_mask(case, kind)
    if kind in ("left_pad_causal", "dead_head"):
        mask = mask[:, :1, :1, :].contiguous().to(DEV).expand(B, H, L, S)
        assert all(s == 0 for s, n in zip(mask.stride()[1:3], (H, L)) if n > 1)
        return mask, causal
    return mask.to(DEV), causal


def _padded(shape, dtype=torch.float32):
    numel = 1
    for n in shape:
        numel *= n
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    inner.fill_(float("nan"))
    return buf, inner.view(shape)


def _inside(name, buf, t):
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + t.numel():] == SENTINEL).all()), f"write outside {name}"


def _strides(tensors):
    st = (ctypes.c_longlong * (4 * len(tensors)))()
    for i, t in enumerate(tensors):
        st[4 * i:4 * i + 4] = list(t.stride())
    return st


def _check_statistics(name, rows, dead, dead_row):
    """`rows`: (B, H, L, n) statistics on the host.  Nothing unwritten (NaN), a dead row is `dead_row`, every other row finite."""
    assert not bool(torch.isnan(rows).any()), f"an element of {name} was not written"
    assert bool(torch.isfinite(rows[~dead]).all()), name
    assert bool((rows[dead] == torch.tensor(dead_row, dtype=rows.dtype)).all()), (name, "a dead row", rows[dead][:1])


def run_vjp(case, kind, family):
    """One double-backward call on buffers this function owns: (dq, dk, dv, dgo) and the workspace (None for the short kernel) on the host."""
    lib = _native.load()
    _, B, H, L, S, d = case
    ins = list(device_inputs(case))
    before = [t.clone() for t in ins]
    mask, causal = device_mask(case, kind)
    mask_before = mask.clone()
    bufs = [_padded(shape) for shape in ((B, H, L, d), (B, H, S, d), (B, H, S, d), (B, H, L, d))]
    tail, ws_buf, ws = (), None, None
    if family != "bhg_attention":
        ws_bytes = int(getattr(lib, family + "_ws_bytes")(B, H, L))
        assert ws_bytes == 40 * B * H * L
        ws_buf, ws = _padded((B, H, L, 5), torch.float64)
        tail = (ws.data_ptr(), ws_bytes)
    rc = getattr(lib, family + "_backward_vjp")(*(t.data_ptr() for t in ins), _strides(ins), mask.data_ptr(),
                                                (ctypes.c_longlong * 4)(*mask.stride()), int(causal), attention_ref.default_scale(d), B, H, L, S,
                                                d, *(t.data_ptr() for _, t in bufs), *tail, int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, family + "_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins + [mask], before + [mask_before]):
        assert torch.equal(t, t0), "an input was modified"
    for name, (buf, t) in zip(("dq", "dk", "dv", "dgo"), bufs):
        _inside(name, buf, t)            # (that every element is written and finite is the gate's first assertion)
    if ws is not None:
        _inside("the workspace", ws_buf, ws)
        ws = ws.cpu()
        _check_statistics("the workspace", ws, dead_rows(case, kind), [NEG, 0.0, 0.0, 0.0, 0.0])
    return tuple(t.cpu() for _, t in bufs), ws


def run_fused(case, kind):
    """Forward, then backward on its O and statistics: (o, gq, gk, gv), the statistics and the workspace on the host."""
    lib = _native.load()
    _, B, H, L, S, d = case
    q, k, v, go = device_inputs(case)[:4]
    ins = [q, k, v, go]
    before = [t.clone() for t in ins]
    mask, causal = device_mask(case, kind)
    mask_before = mask.clone()
    mst = (ctypes.c_longlong * 4)(*mask.stride())
    bufs = [_padded(shape) for shape in ((B, H, L, d), (B, H, L, d), (B, H, S, d), (B, H, S, d))]
    stats_buf, stats = _padded((B, H, L, 2))
    ws_bytes = int(lib.bhg_attention_fused_ws_bytes(B, H, L))
    assert ws_bytes == 8 * B * H * L
    ws_buf, ws = _padded((B, H, L), torch.float64)
    s = attention_ref.default_scale(d)
    stream = int(torch.cuda.current_stream().cuda_stream)
    o = bufs[0][1]
    _native.check(lib.bhg_attention_fused_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), _strides([q, k, v]), mask.data_ptr(), mst, int(causal),
                                                  s, B, H, L, S, d, o.data_ptr(), stats.data_ptr(), stream), "bhg_attention_fused_forward")
    _native.check(lib.bhg_attention_fused_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), go.data_ptr(), stats.data_ptr(),
                                                   _strides([q, k, v, o, go]), mask.data_ptr(), mst, int(causal), s, B, H, L, S, d,
                                                   *(t.data_ptr() for _, t in bufs[1:]), ws.data_ptr(), ws_bytes, stream),
                  "bhg_attention_fused_backward")
    torch.cuda.synchronize()
    for t, t0 in zip(ins + [mask], before + [mask_before]):
        assert torch.equal(t, t0), "an input was modified"
    for name, (buf, t) in zip(("o", "gq", "gk", "gv", "stats", "ws"), bufs + [(stats_buf, stats), (ws_buf, ws)]):
        _inside(name, buf, t)
    stats, ws = stats.cpu(), ws.cpu()
    dead = dead_rows(case, kind)
    _check_statistics("the statistics", stats, dead, [NEG, 0.0])
    _check_statistics("the workspace", ws.unsqueeze(-1), dead, [0.0])        # D = rowsum(gO * O) with O = 0
    return tuple(t.cpu() for _, t in bufs), stats, ws


@pytest.mark.gpu
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("case,kernel", RUNS, ids=_id)
def test_kernels_give_zeros_in_fully_masked_rows(case, kernel, kind):
    first, second = wanted(case, kind)
    if kernel == "fused":
        got = run_fused(case, kind)
        print(gate(case, kind, ("o", "gq", "gk", "gv"), got[0], first, ("o", "gq"), "fused"))
        again = run_fused(case, kind)
    else:
        got = run_vjp(case, kind, kernel)
        print(gate(case, kind, ("dq", "dk", "dv", "dgo"), got[0], second, ("dq", "dgo"), kernel[len("bhg_attention_"):] or "short"))
        again = run_vjp(case, kind, kernel)
    # fresh NaN-filled buffers: the same bits, statistics and workspace included (a NaN would also fail here: NaN != NaN)
    for u, w in zip(list(got[0]) + list(got[1:]), list(again[0]) + list(again[1:])):
        assert (u is None and w is None) or torch.equal(u, w)

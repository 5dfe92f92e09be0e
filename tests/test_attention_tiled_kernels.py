"""bhg_attention_tiled_backward_vjp (csrc/bhg_attention_tiled.hip: k_attn_tiled_q, k_attn_tiled_k) through the C ABI against the float64
restatement tests/attention_ref.py evaluated on the very fp32 inputs, array by array, on the smallest shapes at which a tiled kernel can
still go wrong (score tiles are 64 queries x 32 keys): L = S one below / at / one above one and two query tiles (63, 64, 65, 127, 128,
129) at d = 4, and 65, 129 at d = 3 (scalar reads); rectangular 5 x 200, 200 x 5 and 65 x 1 (one key: dq = dk = dv = 0 in the
restatement, gated absolutely at 2e-5 max|dgo want|); d in {1, 3, 4, 63, 64} at 65 x 66; 3 x 5 heads of 130 x 257; ViT's
2 x 12 x 197 x 197 x 64; the family's corner 512 x 512 x 64; and one sharp case, q, k ~ sqrt(8) N(0, 1) at 192 x 192 x 64 (scores with a
standard deviation of about 8).  Each shape with the modes of tests/test_attention_kernels.py — no mask; a (B, 1, 1, S) key-padding mask
with -inf whose broadcast dimensions have stride 0; a full (B, H, L, S) random mask; the causal flag; q, k, v as transposed views of
(B, L, H, d); rows with an odd pitch; an explicit scale; each cotangent absent; each output NULL — and one more: a padding mask that
removes the first 70 keys — fewer where S < 78, so that min(8, S // 2) keys stay live (first_keys_masked) — so that the first key
tiles are masked out entirely from S = 40 upwards while every row has several live keys later (no NaN, and a softmax that is not one-hot).
The explicit scale is 0.37, as in the sibling's test, except on the sharp case, where it is 0.11: the sharp case is defined by scores
with a deviation of 8, and 0.37 would make that 23 (|score| up to 104), where the plain fp32 evaluation of tests/attention_ref.py on the
CPU is itself 3.6e-5 of max|want| from its float64 evaluation — outside the gate for any fp32 arithmetic, whatever the kernel.

Outputs are slices of sentinel-filled buffers, NaN-filled before each call, and the workspace is a slice of exactly
bhg_attention_tiled_ws_bytes bytes of a sentinel-filled buffer: written inside their bounds only; every element of a given output is
written; a NULL output's buffer stays untouched; the inputs are bit-equal afterwards; a second run gives the same bits.

Gate, per (b, h) slice of each output: max|got - want| <= 2e-5 max|want_slice|.  test_the_gate_can_exclude_no_case (CPU)
shows that the restatement rounded to fp32 passes every case.  Observed maxima on one MI355X: profiles/attention_tiled_fp64.txt."""
import ctypes
import functools

import pytest
import torch

import attention_ref
from betty_amd import _native
from betty_amd.backend import attention_tiled_plan

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["plain", "padding", "full_mask", "causal", "transposed", "odd_pitch", "scale", "no_aq", "no_ak", "no_av", "no_dq", "no_dk", "no_dv",
         "no_dgo", "first_keys_masked"]
NAMES = ("dq", "dk", "dv", "dgo")

# (label, B, H, L, S, d)
EDGES = [("edge", 1, 1, n, n, 4) for n in (63, 64, 65, 127, 128, 129)]
EDGES_SCALAR = [("edge scalar", 1, 1, n, n, 3) for n in (65, 129)]
ONE_KEY = ("one key", 1, 1, 65, 1, 8)
RECT = [("rectangular", 1, 1, 5, 200, 8), ("rectangular", 1, 1, 200, 5, 8), ONE_KEY]
WIDTHS = [("width", 1, 1, 65, 66, d) for d in (1, 3, 4, 63, 64)]
HEADS = ("heads", 3, 5, 130, 257, 8)
VIT = ("vit", 2, 12, 197, 197, 64)
FULL = ("full", 1, 2, 512, 512, 64)
SHARP = ("sharp", 1, 1, 192, 192, 64)
CASES = EDGES + EDGES_SCALAR + RECT + WIDTHS + [HEADS, VIT, FULL, SHARP]
_id = lambda c: f"{c[0].replace(' ', '_')}-{'x'.join(map(str, c[1:]))}" if isinstance(c, tuple) else c   # noqa: E731


def first_keys_masked(S):
    """How many keys the extra mode removes from the front: 70 where that leaves at least 8 live ones, otherwise all but min(8, S // 2)
    (at least one) — a row with one live key has P = 1 and three outputs that are exact zeros, which would check little."""
    return min(70, S - min(8, max(1, S // 2)))


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(q, k, v, go, aq, ak, av, full mask, padding mask, first-keys mask) on the host, fp32; computed once per case, shared, never written."""
    label, B, H, L, S, d = case
    g = torch.Generator().manual_seed(((B * 67 + H) * 67 + L) * 4489 + S * 67 + d)
    q, go, aq = (torch.randn(B, H, L, d, generator=g) for _ in range(3))
    k, v, ak, av = (torch.randn(B, H, S, d, generator=g) for _ in range(4))
    if label == "sharp":
        q, k = q * 8 ** 0.5, k * 8 ** 0.5
    full = torch.randn(B, H, L, S, generator=g)
    padding = torch.zeros(B, 1, 1, S)
    if S > 1:
        padding[::2, :, :, S - 1] = float("-inf")    # never every key of a row
    if S > 2:
        padding[1::2, :, :, :2] = float("-inf")
    first = torch.zeros(B, 1, 1, S)
    first[..., :first_keys_masked(S)] = float("-inf")   # whole key tiles at the front, live keys behind them
    return q, k, v, go, aq, ak, av, full, padding, first


def settings(case, mode):
    """(mask kind, causal, scale, present cotangents, wanted outputs) of a mode."""
    present = tuple(mode != f"no_a{ch}" for ch in "qkv")
    outputs = tuple(mode != f"no_{n}" for n in NAMES)
    mask = {"padding": "padding", "full_mask": "full", "first_keys_masked": "first"}.get(mode)
    return mask, mode == "causal", ((0.11 if case[0] == "sharp" else 0.37) if mode == "scale" else None), present, outputs


@functools.lru_cache(maxsize=None)
def wanted(case, key):
    """(dq, dk, dv, dgo) in float64 for (mask kind, causal, scale, present): shared by the modes that only differ in layout or outputs."""
    mask_kind, causal, scale, present = key
    q, k, v, go, aq, ak, av, full, padding, first = (t.double() for t in host_inputs(case))
    a = [t if on else None for t, on in zip((aq, ak, av), present)]
    mask = {"full": full, "padding": padding, "first": first, None: None}[mask_kind]
    return attention_ref.attention_backward_vjp(q, k, v, go, *a, mask=mask, causal=causal, scale=scale)


def gate(case, mode, got, label="case"):
    """Assert the gate per (b, h) slice on the outputs that were asked for, and print the observed maxima; `got` are host tensors or None."""
    mask_kind, causal, scale, present, outputs = settings(case, mode)
    want = wanted(case, (mask_kind, causal, scale, present))
    line = []
    for name, g, w, on in zip(NAMES, got, want, outputs):
        assert (g is not None) == on
        if g is None:
            continue
        err = (g.double() - w).abs().amax(dim=(2, 3))
        top = w.abs().amax(dim=(2, 3))
        if case == ONE_KEY and name != "dgo":          # exact zeros in the restatement: an absolute gate on the scale of dgo
            assert not w.any()
            top = want[3].abs().amax(dim=(2, 3))
        assert bool(torch.isfinite(g).all()), (label, case, mode, name)
        assert bool((err <= GATE * top).all()), (label, case, mode, name, float((err / top.clamp_min(1e-300)).max()))
        live = top > 0
        line.append(f"{name} {float((err[live] / top[live]).max()) if bool(live.any()) else 0.0:.3e}")
    print(f"attention_tiled_vjp {label} {_id(case)} {mode}: " + "  ".join(line) + "  (worst (b, h) slice of max|got - want| / max|want_slice|)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    for mode in MODES:
        mask_kind, causal, scale, present, outputs = settings(case, mode)
        want = wanted(case, (mask_kind, causal, scale, present))
        gate(case, mode, tuple(w.float() if on else None for w, on in zip(want, outputs)), label="fp64 rounded to fp32")


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    return tuple(t.to(DEV) for t in host_inputs(case))


def _padded(shape):
    numel = 1
    for n in shape:
        numel *= n
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    inner.fill_(float("nan"))
    return buf, inner.view(shape)


def _layout(t, mode):
    """The same values in the memory layout of the mode."""
    if mode == "transposed":                       # a transposed view of (B, L, H, d), as nn.MultiheadAttention hands q, k, v in
        return t.transpose(1, 2).contiguous().transpose(1, 2)
    if mode == "odd_pitch":                        # rows one element apart from contiguous: scalar reads even where d % 4 == 0
        wide = torch.zeros(*t.shape[:3], t.shape[3] + 1, device=t.device)
        wide[..., :t.shape[3]] = t
        return wide[..., :t.shape[3]]
    return t


def run_vjp(case, mode):
    """One call on buffers this function owns.  Returns (dq, dk, dv, dgo) on the host (None for a NULL output) after checking the bounds
    of every write (the workspace's included), that a NULL output's buffer is untouched and that the inputs are unchanged."""
    lib = _native.load()
    _, B, H, L, S, d = case
    mask_kind, causal, scale, present, outputs = settings(case, mode)
    q, k, v, go, aq, ak, av, full, padding, first = device_inputs(case)
    ins = [_layout(q, mode), _layout(k, mode), _layout(v, mode), go, aq, ak, av]
    before = [t.clone() for t in ins]
    on = (True, True, True, True) + present
    mask = {"full": full, "padding": padding.expand(B, H, L, S), "first": first.expand(B, H, L, S), None: None}[mask_kind]
    if mask_kind in ("padding", "first"):
        assert all(s == 0 for s, n in zip(mask.stride()[1:3], (H, L)) if n > 1)   # read in place: no (B, H, L, S) copy
    plan = attention_tiled_plan(B, H, L, S, d, vec_ok=all(s % 4 == 0 for t in ins for s, n in zip(t.stride()[:3], t.shape[:3]) if n > 1))
    assert plan["vec"] == (1 if d % 4 or mode == "odd_pitch" else 4), plan
    ws_bytes = int(lib.bhg_attention_tiled_ws_bytes(B, H, L))
    assert ws_bytes == plan["ws"] and ws_bytes % 8 == 0
    ws_buf = torch.full((ws_bytes // 8 + 2 * PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = ws_buf[PAD:PAD + ws_bytes // 8]
    strides = (ctypes.c_longlong * 28)()
    for i, t in enumerate(ins):
        strides[4 * i:4 * i + 4] = list(t.stride())
    mstrides = (ctypes.c_longlong * 4)(*mask.stride()) if mask is not None else None
    bufs = [_padded(shape) for shape in ((B, H, L, d), (B, H, S, d), (B, H, S, d), (B, H, L, d))]
    ptr = lambda t, given=True: t.data_ptr() if given else None   # noqa: E731
    rc = lib.bhg_attention_tiled_backward_vjp(*(ptr(t, g) for t, g in zip(ins, on)), strides, mask.data_ptr() if mask is not None else None,
                                              mstrides, int(causal), attention_ref.default_scale(d) if scale is None else scale, B, H, L, S,
                                              d, *(ptr(t, g) for (_, t), g in zip(bufs, outputs)), ws.data_ptr(), ws_bytes,
                                              int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_attention_tiled_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
    assert bool((ws_buf[:PAD] == SENTINEL).all()) and bool((ws_buf[PAD + ws.numel():] == SENTINEL).all()), "write outside the workspace"
    got = []
    for name, (buf, t), given in zip(NAMES, bufs, outputs):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + t.numel():] == SENTINEL).all()), f"write outside {name}"
        if given:
            assert bool(torch.isfinite(t).all()), f"an element of {name} was not written (or a stale value was read)"
            got.append(t.cpu())
        else:
            assert bool(torch.isnan(t).all()), f"{name} was not given: its buffer must stay untouched"
            got.append(None)
    return tuple(got)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_matches_the_fp64_restatement(case, mode):
    first = run_vjp(case, mode)
    gate(case, mode, first)
    again = run_vjp(case, mode)                                                       # fresh NaN-filled outputs: the same bits
    for name, u, w in zip(NAMES, first, again):
        assert (u is None and w is None) or torch.equal(u, w), name

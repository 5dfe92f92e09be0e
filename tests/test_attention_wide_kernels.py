"""bhg_attention_wide_backward_vjp (csrc/bhg_attention_wide.hip: 64 x 16 score tiles in the query launch, 32 x 32 in the key launch)
through the C ABI against the float64 restatement tests/attention_ref.py evaluated on the very fp32 inputs, with the fifteen modes of
tests/test_attention_tiled_kernels.py.  Gate, per (b, h) slice of each output: max|got - want| <= 2e-5 max|want_slice|;
with one key dq = dk = dv are exact zeros in the restatement and are gated absolutely on dgo's scale.  Outputs and workspace are slices
of sentinel-padded buffers.  The sharp case (scores with a deviation of about 8) runs with the default scale only.
test_the_gate_can_exclude_no_case (CPU) shows that the restatement rounded to fp32 passes every case and mode.
Observed maxima on one MI355X: profiles/attention_wide_fp64.txt."""
import ctypes
import functools

import pytest
import torch

import attention_ref
from betty_amd import _native
from betty_amd.backend import attention_wide_plan

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["plain", "padding", "full_mask", "causal", "transposed", "odd_pitch", "scale", "no_aq", "no_ak", "no_av", "no_dq", "no_dk", "no_dv",
         "no_dgo", "first_keys_masked"]
NAMES = ("dq", "dk", "dv", "dgo")
ONE_KEY = ("one key", 1, 1, 65, 1, 72)
# (label, B, H, L, S, d): one below / at / one above the tiles of 16, 32 and 64; every dp instance and both read widths; the rest
CASES = ([("edge", 1, 1, n, n, 68) for n in (16, 17, 31, 32, 33, 63, 64, 65, 129)] + [("edge scalar", 1, 1, n, n, 65) for n in (33, 65)] +
         [("width", 1, 1, 65, 66, d) for d in (65, 67, 68, 80, 96, 112, 127, 128)] +
         [("rectangular", 1, 1, 5, 200, 72), ("rectangular", 1, 1, 200, 5, 72), ONE_KEY, ("heads", 3, 5, 70, 130, 72),
          ("full", 1, 2, 512, 512, 128), ("sharp", 1, 1, 192, 192, 128)])
PAIRS = [(c, m) for c in CASES for m in MODES if not (c[0] == "sharp" and m == "scale")]
_id = lambda c: f"{c[0].replace(' ', '_')}-{'x'.join(map(str, c[1:]))}" if isinstance(c, tuple) else c   # noqa: E731


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(q, k, v, go, aq, ak, av, full mask, padding mask, first-keys mask) on the host, fp32; computed once per case, never written."""
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
    first[..., :min(70, S - min(8, max(1, S // 2)))] = float("-inf")   # whole key tiles dead at the front, several live keys behind them
    return q, k, v, go, aq, ak, av, full, padding, first


def settings(mode):
    """(mask kind, causal, scale, present cotangents, wanted outputs) of a mode."""
    mask = {"padding": "padding", "full_mask": "full", "first_keys_masked": "first"}.get(mode)
    return mask, mode == "causal", 0.26 if mode == "scale" else None, tuple(mode != f"no_a{c}" for c in "qkv"), tuple(mode != f"no_{n}" for n in NAMES)


@functools.lru_cache(maxsize=None)
def wanted(case, key):
    """(dq, dk, dv, dgo) in float64 for (mask kind, causal, scale, present): shared by the modes that only differ in layout or outputs."""
    mask_kind, causal, scale, present = key
    q, k, v, go, aq, ak, av, full, padding, first = (t.double() for t in host_inputs(case))
    a = [t if on else None for t, on in zip((aq, ak, av), present)]
    mask = {"full": full, "padding": padding, "first": first, None: None}[mask_kind]
    return attention_ref.attention_backward_vjp(q, k, v, go, *a, mask=mask, causal=causal, scale=scale)


def gate(case, mode, got, label="case"):
    """Assert the gate per (b, h) slice on the outputs that were asked for, and print the observed maxima."""
    mask_kind, causal, scale, present, outputs = settings(mode)
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
        line.append(f"{name} {float((err / top.clamp_min(1e-300)).max()):.3e}")
    print(f"attention_wide_vjp {label} {_id(case)} {mode}: " + "  ".join(line) + "  (worst (b, h) slice of max|got - want| / max|want_slice|)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    for mode in (m for c, m in PAIRS if c == case):
        mask_kind, causal, scale, present, outputs = settings(mode)
        want = wanted(case, (mask_kind, causal, scale, present))
        gate(case, mode, tuple(w.float() if on else None for w, on in zip(want, outputs)), label="fp64 rounded to fp32")


def _padded(shape):
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    inner.fill_(float("nan"))
    return buf, inner.view(shape)


def _layout(t, mode):
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
    mask_kind, causal, scale, present, outputs = settings(mode)
    q, k, v, go, aq, ak, av, full, padding, first = (t.to(DEV) for t in host_inputs(case))
    ins = [_layout(q, mode), _layout(k, mode), _layout(v, mode), go, aq, ak, av]
    before = [t.clone() for t in ins]
    on = (True, True, True, True) + present
    mask = {"full": full, "padding": padding.expand(B, H, L, S), "first": first.expand(B, H, L, S), None: None}[mask_kind]
    if mask_kind in ("padding", "first"):
        assert all(s == 0 for s, n in zip(mask.stride()[1:3], (H, L)) if n > 1)   # read in place: no (B, H, L, S) copy
    plan = attention_wide_plan(B, H, L, S, d, vec_ok=all(s % 4 == 0 for t in ins for s, n in zip(t.stride()[:3], t.shape[:3]) if n > 1))
    assert plan["vec"] == (1 if d % 4 or mode == "odd_pitch" else 4), plan
    ws_bytes = int(lib.bhg_attention_wide_ws_bytes(B, H, L))
    assert ws_bytes == plan["ws"] and ws_bytes % 8 == 0
    ws_buf = torch.full((ws_bytes // 8 + 2 * PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = ws_buf[PAD:PAD + ws_bytes // 8]
    strides = (ctypes.c_longlong * 28)()
    for i, t in enumerate(ins):
        strides[4 * i:4 * i + 4] = list(t.stride())
    mstrides = (ctypes.c_longlong * 4)(*mask.stride()) if mask is not None else None
    bufs = [_padded(shape) for shape in ((B, H, L, d), (B, H, S, d), (B, H, S, d), (B, H, L, d))]
    ptr = lambda t, given=True: t.data_ptr() if given else None   # noqa: E731
    rc = lib.bhg_attention_wide_backward_vjp(*(ptr(t, g) for t, g in zip(ins, on)), strides, mask.data_ptr() if mask is not None else None,
                                             mstrides, int(causal), attention_ref.default_scale(d) if scale is None else scale, B, H, L, S,
                                             d, *(ptr(t, g) for (_, t), g in zip(bufs, outputs)), ws.data_ptr(), ws_bytes,
                                             int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_attention_wide_backward_vjp")
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
@pytest.mark.parametrize("case,mode", PAIRS, ids=_id)
def test_kernel_matches_the_fp64_restatement(case, mode):
    first = run_vjp(case, mode)
    gate(case, mode, first)
    again = run_vjp(case, mode)                                                       # fresh NaN-filled outputs: the same bits
    for name, u, w in zip(NAMES, first, again):
        assert (u is None and w is None) or torch.equal(u, w), name

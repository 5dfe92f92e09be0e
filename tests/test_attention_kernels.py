"""bhg_attention_backward_vjp (csrc/bhg_attention.hip: k_attn_vjp) through the C ABI against the float64 restatement
tests/attention_ref.py evaluated on the very fp32 inputs, array by array, on the smallest shapes at which the kernel can still go wrong:
one element; one key (dq = dk = dv = 0 exactly, dgo = av); L = S one below / at / one above 16 and 32 (the 16-row and 16-column steps
of a thread's 4 x 4 outputs) and at 63 / 64; L != S both ways (5 x 64, 64 x 5); d in {1, 3, 4, 63, 64} (scalar and 16-byte accesses,
one element and the full width); B H = 1 and 3 x 5; BASELINE cfg 4's 16 x 12 x 50 x 64; and one sharp case, q, k ~ sqrt(8) N(0, 1) at
64 x 64 x 64 (scores with a standard deviation of about 8).  Each shape with: no mask; a (B, 1, 1, S) key-padding mask with -inf whose
broadcast dimensions have stride 0; a full (B, H, L, S) random mask; the causal flag; q, k, v as transposed views of (B, L, H, d);
rows with an odd pitch (scalar accesses even where d % 4 == 0); an explicit scale; each cotangent absent; each output NULL.

Outputs are slices of sentinel-filled buffers, NaN-filled before each call: they must be written inside their bounds only, and everywhere
inside; a NULL output's buffer stays untouched; the inputs are bit-equal afterwards; a second run gives the same bits.

Gate, per (b, h) slice of each output: max|got - want| <= 2e-5 max|want_slice| — the project's gate for fp32 kernels against fp64
restatements.  The fp32 torch restatement on the CPU sits at <= 9.2e-7 for the unit-score cases and <= 4.6e-6 for the sharp
one; test_the_gate_can_exclude_no_case (CPU) shows that the restatement rounded to fp32 passes every case.  Observed maxima on one
MI355X: profiles/attention_fp64.txt."""
import ctypes
import functools

import pytest
import torch

import attention_ref
from betty_amd import _native
from betty_amd.backend import attention_plan

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["plain", "padding", "full_mask", "causal", "transposed", "odd_pitch", "scale", "no_aq", "no_ak", "no_av", "no_dq", "no_dk", "no_dv",
         "no_dgo"]
NAMES = ("dq", "dk", "dv", "dgo")

# (label, B, H, L, S, d)
ONE = ("one element", 1, 1, 1, 1, 1)
ONE_KEY = [("one key", 1, 2, 7, 1, 8), ("one key", 2, 1, 17, 1, 3)]
EDGES = [("edge", 1, 1, n, n, 4) for n in (15, 16, 17, 31, 32, 33, 63, 64)]
EDGES_SCALAR = [("edge scalar", 1, 1, n, n, 3) for n in (16, 17, 33, 64)]
RECT = [("rectangular", 1, 1, 5, 64, 8), ("rectangular", 1, 1, 64, 5, 8), ("rectangular", 3, 5, 5, 64, 3), ("rectangular", 3, 5, 64, 5, 3)]
WIDTHS = [("width", 1, 1, 17, 18, d) for d in (1, 3, 4, 63, 64)]
HEADS = [("heads", 3, 5, 17, 33, 8), ("heads", 3, 5, 33, 17, 5)]
FULL = ("full", 1, 2, 64, 64, 64)
ROBERTA = ("roberta", 16, 12, 50, 50, 64)
SHARP = ("sharp", 1, 1, 64, 64, 64)
CASES = [ONE] + ONE_KEY + EDGES + EDGES_SCALAR + RECT + WIDTHS + HEADS + [FULL, ROBERTA, SHARP]
_id = lambda c: f"{c[0].replace(' ', '_')}-{'x'.join(map(str, c[1:]))}" if isinstance(c, tuple) else c   # noqa: E731


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(q, k, v, go, aq, ak, av, full mask, padding mask) on the host, fp32; computed once per case, shared, never written."""
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
    return q, k, v, go, aq, ak, av, full, padding


def settings(case, mode):
    """(mask kind, causal, scale, present cotangents, wanted outputs) of a mode."""
    present = tuple(mode != f"no_a{ch}" for ch in "qkv")
    outputs = tuple(mode != f"no_{n}" for n in NAMES)
    mask = {"padding": "padding", "full_mask": "full"}.get(mode)
    return mask, mode == "causal", (0.37 if mode == "scale" else None), present, outputs


@functools.lru_cache(maxsize=None)
def wanted(case, key):
    """(dq, dk, dv, dgo) in float64 for (mask kind, causal, scale, present): shared by the modes that only differ in layout or outputs."""
    mask_kind, causal, scale, present = key
    q, k, v, go, aq, ak, av, full, padding = (t.double() for t in host_inputs(case))
    a = [t if on else None for t, on in zip((aq, ak, av), present)]
    mask = {"full": full, "padding": padding, None: None}[mask_kind]
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
        assert bool((err <= GATE * top).all()), (label, case, mode, name, float((err / top.clamp_min(1e-300)).max()))
        live = top > 0
        line.append(f"{name} {float((err[live] / top[live]).max()) if bool(live.any()) else 0.0:.3e}")
    print(f"attention_vjp {label} {_id(case)} {mode}: " + "  ".join(line) + "  (worst (b, h) slice of max|got - want| / max|want_slice|)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    for mode in MODES:
        mask_kind, causal, scale, present, outputs = settings(case, mode)
        want = wanted(case, (mask_kind, causal, scale, present))
        gate(case, mode, tuple(w.float() if on else None for w, on in zip(want, outputs)), label="fp64 rounded to fp32")


def test_one_key_cases_have_three_zero_outputs():
    for case in ONE_KEY:
        dq, dk, dv, dgo = wanted(case, (None, False, None, (True, True, True)))
        assert not dq.any() and not dk.any() and not dv.any() and bool(dgo.any())


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
    if mode == "odd_pitch":                        # rows one element apart from contiguous: scalar accesses even where d % 4 == 0
        wide = torch.zeros(*t.shape[:3], t.shape[3] + 1, device=t.device)
        wide[..., :t.shape[3]] = t
        return wide[..., :t.shape[3]]
    return t


def run_vjp(case, mode):
    """One call on buffers this function owns.  Returns (dq, dk, dv, dgo) on the host (None for a NULL output) after checking the bounds
    of every write, that every element inside was written, that a NULL output's buffer is untouched and that the inputs are unchanged."""
    lib = _native.load()
    _, B, H, L, S, d = case
    mask_kind, causal, scale, present, outputs = settings(case, mode)
    q, k, v, go, aq, ak, av, full, padding = device_inputs(case)
    ins = [_layout(q, mode), _layout(k, mode), _layout(v, mode), go, aq, ak, av]
    before = [t.clone() for t in ins]
    on = (True, True, True, True) + present
    mask = {"full": full, "padding": padding.expand(B, H, L, S), None: None}[mask_kind]
    if mask_kind == "padding":
        assert all(s == 0 for s, n in zip(mask.stride()[1:3], (H, L)) if n > 1)   # read in place: no (B, H, L, S) copy
    plan = attention_plan(B, H, L, S, d, vec_ok=all(s % 4 == 0 for t in ins for s, n in zip(t.stride()[:3], t.shape[:3]) if n > 1))
    assert plan["vec"] == (1 if d % 4 or mode == "odd_pitch" else 4), plan
    strides = (ctypes.c_longlong * 28)()
    for i, t in enumerate(ins):
        strides[4 * i:4 * i + 4] = list(t.stride())
    mstrides = (ctypes.c_longlong * 4)(*mask.stride()) if mask is not None else None
    bufs = [_padded(shape) for shape in ((B, H, L, d), (B, H, S, d), (B, H, S, d), (B, H, L, d))]
    ptr = lambda t, given=True: t.data_ptr() if given else None   # noqa: E731
    rc = lib.bhg_attention_backward_vjp(*(ptr(t, g) for t, g in zip(ins, on)), strides, mask.data_ptr() if mask is not None else None,
                                        mstrides, int(causal), attention_ref.default_scale(d) if scale is None else scale, B, H, L, S, d,
                                        *(ptr(t, g) for (_, t), g in zip(bufs, outputs)), int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_attention_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
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
    if case[0] == "one key" and mode in ("plain", "transposed", "odd_pitch", "scale", "causal", "full_mask"):
        assert not first[0].any() and not first[1].any() and not first[2].any()      # exact zeros
        assert torch.equal(first[3], device_inputs(case)[6].expand_as(first[3]).cpu())   # dgo = P av with P = 1
    again = run_vjp(case, mode)                                                       # fresh NaN-filled outputs: the same bits
    for name, u, w in zip(NAMES, first, again):
        assert (u is None and w is None) or torch.equal(u, w), name

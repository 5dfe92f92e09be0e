"""bhg_attention_fused_forward and bhg_attention_fused_backward (csrc/bhg_attention_fused.hip) through the C ABI against
attention_ref.attention and attention_ref.attention_backward evaluated in float64 on the very fp32 inputs, on the smallest shapes at
which a 64 x 32 tiling can go wrong: L = S one below / at / one above a query tile and two key tiles (63, 64, 65, 129) at d = 4; 65 at
d = 3 (scalar reads); rectangular 5 x 200, 200 x 5 and 65 x 1 (one key: gq = gk = 0 in the reference, gated absolutely on the scale of
gv); d in {1, 63, 64} at 65 x 66; 3 x 5 heads of 130 x 257; the family's corner 512 x 512 x 64; and one sharp case, q, k ~ sqrt(8) N(0, 1)
at 192 x 192 x 64.  Each shape with: no mask; a (B, 1, 1, S) key-padding mask whose broadcast dimensions have stride 0; a full random
mask; the causal flag; q, k, v as transposed views of (B, L, H, d); rows with an odd pitch; an explicit scale (0.37; 0.11 on the sharp
case, for the reason given in tests/test_attention_tiled_kernels.py); each output NULL; and a padding mask that removes the first 70 keys
(fewer for small S, by that file's rule), so that whole leading key tiles are dead.  No mask removes every key of a row.

O, the statistics, the workspace and the three gradients are slices of sentinel-padded, NaN-filled buffers: written inside their bounds
only, every element written, a NULL output's buffer untouched, the inputs bit-equal afterwards, a second run the same bits.

Gate, per (b, h) slice of each output: max|got - want| <= 2e-5 max|want_slice|.  Observed: profiles/attention_fused_fp64.txt."""
import ctypes
import functools

import pytest
import torch

import attention_ref
from betty_amd import _native
from betty_amd.backend import attention_fused_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["plain", "padding", "full_mask", "causal", "transposed", "odd_pitch", "scale", "no_gq", "no_gk", "no_gv", "first_keys_masked"]
NAMES = ("o", "gq", "gk", "gv")

ONE_KEY = ("one key", 1, 1, 65, 1, 8)
CASES = ([("edge", 1, 1, n, n, 4) for n in (63, 64, 65, 129)] + [("edge scalar", 1, 1, 65, 65, 3)]
         + [("rectangular", 1, 1, 5, 200, 8), ("rectangular", 1, 1, 200, 5, 8), ONE_KEY] + [("width", 1, 1, 65, 66, d) for d in (1, 63, 64)]
         + [("heads", 3, 5, 130, 257, 8), ("full", 1, 2, 512, 512, 64), ("sharp", 1, 1, 192, 192, 64)])
_id = lambda c: f"{c[0].replace(' ', '_')}-{'x'.join(map(str, c[1:]))}" if isinstance(c, tuple) else c   # noqa: E731


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(q, k, v, go, full mask, padding mask, first-keys mask) on the host, fp32; computed once per case, shared, never written."""
    label, B, H, L, S, d = case
    g = torch.Generator().manual_seed(((B * 67 + H) * 67 + L) * 4489 + S * 67 + d)
    q, go = (torch.randn(B, H, L, d, generator=g) for _ in range(2))
    k, v = (torch.randn(B, H, S, d, generator=g) for _ in range(2))
    if label == "sharp":
        q, k = q * 8 ** 0.5, k * 8 ** 0.5
    full = torch.randn(B, H, L, S, generator=g)
    padding = torch.zeros(B, 1, 1, S)
    if S > 1:
        padding[::2, :, :, S - 1] = float("-inf")    # never every key of a row
    if S > 2:
        padding[1::2, :, :, :2] = float("-inf")
    first = torch.zeros(B, 1, 1, S)
    first[..., :min(70, S - min(8, max(1, S // 2)))] = float("-inf")   # whole key tiles at the front, live keys behind them
    return q, k, v, go, full, padding, first


def settings(case, mode):
    """(mask kind, causal, scale) of a mode."""
    mask = {"padding": "padding", "full_mask": "full", "first_keys_masked": "first"}.get(mode)
    return mask, mode == "causal", ((0.11 if case[0] == "sharp" else 0.37) if mode == "scale" else None)


@functools.lru_cache(maxsize=None)
def wanted(case, key):
    """(o, gq, gk, gv) in float64: shared by the modes that only differ in layout or outputs."""
    mask_kind, causal, scale = key
    q, k, v, go, full, padding, first = (t.double() for t in host_inputs(case))
    mask = {"full": full, "padding": padding, "first": first, None: None}[mask_kind]
    want = (attention_ref.attention(q, k, v, mask, causal, scale),) + tuple(attention_ref.attention_backward(q, k, v, go, mask, causal, scale))
    assert all(bool(torch.isfinite(w).all()) for w in want)
    return want


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    return tuple(t.to(DEV) for t in host_inputs(case))


def _padded(shape, dtype=torch.float32):
    numel = 1
    for n in shape:
        numel *= n
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
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


def run(case, mode):
    """Forward, then backward on its O and statistics, on buffers this function owns.  Returns (o, gq, gk, gv) on the host (None for a
    NULL output) after checking the bounds of every write, that a NULL output's buffer is untouched and that the inputs are unchanged."""
    lib = _native.load()
    _, B, H, L, S, d = case
    mask_kind, causal, scale = settings(case, mode)
    q, k, v, go, full, padding, first = device_inputs(case)
    ins = [_layout(q, mode), _layout(k, mode), _layout(v, mode), go]
    before = [t.clone() for t in ins]
    given = (True,) + tuple(mode != f"no_{n}" for n in NAMES[1:])
    mask = {"full": full, "padding": padding.expand(B, H, L, S), "first": first.expand(B, H, L, S), None: None}[mask_kind]
    if mask_kind in ("padding", "first"):
        assert all(s == 0 for s, n in zip(mask.stride()[1:3], (H, L)) if n > 1)   # read in place: no (B, H, L, S) copy
    plan = attention_fused_plan(B, H, L, S, d, vec_ok=all(s % 4 == 0 for t in ins for s, n in zip(t.stride()[:3], t.shape[:3]) if n > 1))
    assert plan["vec"] == (1 if d % 4 or mode == "odd_pitch" else 4), plan
    assert plan["stats"] == 8 and plan["ws"] == int(lib.bhg_attention_fused_ws_bytes(B, H, L)) == 8 * B * H * L
    bufs = [_padded(shape) for shape in ((B, H, L, d), (B, H, L, d), (B, H, S, d), (B, H, S, d))]
    stats_buf, stats = _padded((B, H, L, 2))
    ws_buf, ws = _padded((B, H, L), torch.float64)
    mptr = mask.data_ptr() if mask is not None else None
    mstrides = (ctypes.c_longlong * 4)(*mask.stride()) if mask is not None else None
    s = attention_ref.default_scale(d) if scale is None else scale
    stream = int(torch.cuda.current_stream().cuda_stream)
    o = bufs[0][1]
    fst = (ctypes.c_longlong * 12)(*(x for t in ins[:3] for x in t.stride()))
    _native.check(lib.bhg_attention_fused_forward(*(t.data_ptr() for t in ins[:3]), fst, mptr, mstrides, int(causal), s, B, H, L, S, d,
                                                  o.data_ptr(), stats.data_ptr(), stream), "bhg_attention_fused_forward")
    bst = (ctypes.c_longlong * 20)(*(x for t in ins[:3] + [o, go] for x in t.stride()))
    _native.check(lib.bhg_attention_fused_backward(*(t.data_ptr() for t in ins[:3]), o.data_ptr(), go.data_ptr(), stats.data_ptr(), bst, mptr,
                                                   mstrides, int(causal), s, B, H, L, S, d,
                                                   *(t.data_ptr() if on else None for (_, t), on in zip(bufs[1:], given[1:])), ws.data_ptr(),
                                                   plan["ws"], stream), "bhg_attention_fused_backward")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
    got = []
    for name, (buf, t), on in zip(NAMES + ("stats", "ws"), bufs + [(stats_buf, stats), (ws_buf, ws)], given + (True, True)):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + t.numel():] == SENTINEL).all()), f"write outside {name}"
        if on:
            assert bool(torch.isfinite(t).all()), f"an element of {name} was not written (or a stale value was read)"
            got.append(t.cpu())
        else:
            assert bool(torch.isnan(t).all()), f"{name} was not given: its buffer must stay untouched"
            got.append(None)
    return tuple(got)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernels_match_the_fp64_reference(case, mode):
    first = run(case, mode)
    want = wanted(case, settings(case, mode))
    line = []
    for name, g, w in zip(NAMES, first, want):
        if g is None:
            continue
        err = (g.double() - w).abs().amax(dim=(2, 3))
        top = w.abs().amax(dim=(2, 3))
        if case == ONE_KEY and name in ("gq", "gk"):      # exact zeros in the reference: an absolute gate on the scale of gv
            assert not w.any()
            top = want[3].abs().amax(dim=(2, 3))
        line.append(f"{name} {float((err / top).max()):.3e}")
        assert bool((err <= GATE * top).all()), (case, mode, name, float((err / top).max()))
    print(f"attention_fused {_id(case)} {mode}: " + "  ".join(line) + "  (worst (b, h) slice of max|got - want| / max|want_slice|)")
    again = run(case, mode)                                # fresh NaN-filled buffers: the same bits, statistics and workspace included
    for name, u, w in zip(NAMES + ("stats", "ws"), first, again):
        assert (u is None and w is None) or torch.equal(u, w), name

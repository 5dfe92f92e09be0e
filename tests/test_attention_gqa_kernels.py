"""bhg_attention_gqa_backward_vjp (csrc/bhg_attention_gqa.hip: k_attn_gqa_q, k_attn_gqa_k) through the C ABI against the float64
restatement: tests/attention_ref.attention_backward_vjp on repeat_interleave'd k, v, ak, av, with dk, dv summed over each group.  The
kernel packs the g query heads of a key/value head into g L query rows of 64-row tiles; the cases (B, Hkv, g, L, S, d) are the smallest
at which that can go wrong: the degenerate corner; three heads in one tile, scalar reads; a head boundary inside a tile; heads aligned
to tiles; every tile crossing; causal with L != S both ways; 4096 packed rows, the family's corner.  Gate, per (b, head) slice of each
output: max|got - want| <= 2e-5 max|want_slice|.  At the corner dk and dv sum 4096 packed rows and their gate is
2e-5 sqrt(g L / 512): the random-walk growth of an exact-fp32 sum over the 512 rows at which the tiled sibling's 5.7e-6 was observed.
Outputs and workspace are slices of sentinel-filled buffers: written inside their bounds only, a NULL
output's buffer untouched, a second run the same bits.  Observed maxima on one MI355X: profiles/attention_gqa_fp64.txt."""
import ctypes
import functools

import pytest
import torch

import attention_ref
from betty_amd import _native
from betty_amd.backend import attention_gqa_plan

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
NAMES = ("dq", "dk", "dv", "dgo")
MODES = ["plain", "padding", "full_mask", "causal", "transposed", "odd_pitch", "scale", "no_aq", "no_ak", "no_av", "no_dq", "no_dk", "no_dv",
         "no_dgo", "dead_row"]
CORNER = (1, 1, 8, 512, 512, 64)
CASES = [(1, 1, 2, 1, 1, 1), (2, 2, 3, 5, 7, 3), (2, 1, 2, 50, 70, 64), (1, 2, 4, 64, 33, 16), (1, 1, 8, 65, 65, 20), (1, 2, 2, 70, 50, 32),
         (1, 1, 2, 40, 90, 32), CORNER]
_id = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else c   # noqa: E731


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(q, k, v, go, aq, ak, av) and the masks by kind, on the host in fp32; computed once per case, shared, never written."""
    B, Hkv, g, L, S, d = case
    gen = torch.Generator().manual_seed(sum(n * 67 ** i for i, n in enumerate(case)))
    q, go, aq = (torch.randn(B, Hkv * g, L, d, generator=gen) for _ in range(3))
    k, v, ak, av = (torch.randn(B, Hkv, S, d, generator=gen) for _ in range(4))
    padding = torch.zeros(B, 1, 1, S)
    padding[::2, :, :, S - 1:] = float("-inf") if S > 1 else 0.0        # never every key of a row
    dead = torch.zeros(B, Hkv * g, L, S)
    dead[:, 1, min(3, L - 1)] = float("-inf")                           # one fully masked row in the second head of the first group
    return (q, k, v, go, aq, ak, av), {"full": torch.randn(B, Hkv * g, L, S, generator=gen), "padding": padding, "dead": dead, None: None}


def settings(mode):
    """(mask kind, causal, scale, present cotangents, wanted outputs) of a mode."""
    mask = {"padding": "padding", "full_mask": "full", "dead_row": "dead"}.get(mode)
    return mask, mode == "causal", 0.37 if mode == "scale" else None, tuple(mode != f"no_a{c}" for c in "qkv"), tuple(mode != f"no_{n}" for n in NAMES)


@functools.lru_cache(maxsize=None)
def wanted(case, key):
    """(dq, dk, dv, dgo) in float64 for (mask kind, causal, scale, present): shared by the modes that differ only in layout or outputs."""
    B, Hkv, g, L, S, d = case
    mask_kind, causal, scale, present = key
    ins, masks = host_inputs(case)
    q, k, v, go, aq, ak, av = (t.double() if on else None for t, on in zip(ins, (True,) * 4 + present))
    rep = lambda t: None if t is None else t.repeat_interleave(g, dim=1)   # noqa: E731
    mask = None if mask_kind is None else masks[mask_kind].double()
    dq, dk, dv, dgo = attention_ref.attention_backward_vjp(q, rep(k), rep(v), go, aq, rep(ak), rep(av), mask=mask, causal=causal, scale=scale)
    return dq, dk.view(B, Hkv, g, S, d).sum(2), dv.view(B, Hkv, g, S, d).sum(2), dgo


def _padded(shape, dtype=torch.float32):
    numel = torch.Size(shape).numel()
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    buf[PAD:PAD + numel] = float("nan")
    return buf, buf[PAD:PAD + numel].view(shape)


def _layout(t, mode):
    if mode == "transposed":                       # a transposed view of (B, L, H, d): (H, L) is not contiguous
        return t.transpose(1, 2).contiguous().transpose(1, 2)
    if mode == "odd_pitch":                        # rows one element apart from contiguous: scalar reads even where d % 4 == 0
        return torch.cat([t, torch.zeros_like(t[..., :1])], dim=-1)[..., :t.shape[3]]
    return t


def run_vjp(case, mode):
    """One call on buffers this function owns -> (dq, dk, dv, dgo) on the host (None for a NULL output), after checking the bounds of
    every write, that a NULL output's buffer is untouched and that the inputs are unchanged."""
    lib = _native.load()
    B, Hkv, g, L, S, d = case
    Hq = Hkv * g
    mask_kind, causal, scale, present, outputs = settings(mode)
    host, masks = host_inputs(case)
    ins = [_layout(t.to(DEV), mode) if i < 3 else t.to(DEV) for i, t in enumerate(host)]
    before = [t.clone() for t in ins]
    mask = None if mask_kind is None else masks[mask_kind].to(DEV).expand(B, Hq, L, S)   # broadcast dimensions keep stride 0
    vec_ok = all(s % 4 == 0 for t in ins for s, n in zip(t.stride()[:3], t.shape[:3]) if n > 1)
    plan = attention_gqa_plan(B, Hq, Hkv, L, S, d, vec_ok=vec_ok)
    assert plan["vec"] == (1 if d % 4 or mode == "odd_pitch" else 4) and plan["rows"] == g * L, plan
    ws_bytes = int(lib.bhg_attention_gqa_ws_bytes(B, Hq, L))
    assert ws_bytes == plan["ws"] == 40 * B * Hq * L
    ws_buf, ws = _padded((ws_bytes // 8,), torch.float64)
    strides = (ctypes.c_longlong * 28)(*[s for t in ins for s in t.stride()])
    mstrides = (ctypes.c_longlong * 4)(*mask.stride()) if mask is not None else None
    bufs = [_padded(shape) for shape in ((B, Hq, L, d), (B, Hkv, S, d), (B, Hkv, S, d), (B, Hq, L, d))]
    ptr = lambda t, given=True: t.data_ptr() if given else None   # noqa: E731
    rc = lib.bhg_attention_gqa_backward_vjp(*(ptr(t, on) for t, on in zip(ins, (True,) * 4 + present)), strides,
                                            mask.data_ptr() if mask is not None else None, mstrides, int(causal),
                                            attention_ref.default_scale(d) if scale is None else scale, B, Hq, Hkv, L, S, d,
                                            *(ptr(t, on) for (_, t), on in zip(bufs, outputs)), ws.data_ptr(), ws_bytes,
                                            int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_attention_gqa_backward_vjp")
    torch.cuda.synchronize()
    assert all(torch.equal(t, t0) for t, t0 in zip(ins, before)), "an input was modified"
    got = []
    for name, (buf, t), given in zip(NAMES + ("ws",), bufs + [(ws_buf, ws)], outputs + (True,)):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + t.numel():] == SENTINEL).all()), f"write outside {name}"
        assert bool((~torch.isnan(t)).all() if given else torch.isnan(t).all()), f"{name}: an element not written, or a NULL output touched"
        got.append(t.cpu() if given else None)
    return tuple(got[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_matches_the_fp64_restatement(case, mode):
    B, Hkv, g, L, S, d = case
    mask_kind, causal, scale, present, outputs = settings(mode)
    want = wanted(case, (mask_kind, causal, scale, present))
    first = run_vjp(case, mode)
    line = []
    for name, u, w in zip(NAMES, first, want):
        if u is None:
            continue
        gate = GATE * (g * L / 512) ** 0.5 if case == CORNER and name in ("dk", "dv") else GATE
        err, top = (u.double() - w).abs().amax(dim=(2, 3)), w.abs().amax(dim=(2, 3))
        line.append(f"{name} {float((err / top.clamp_min(1e-300)).max()):.3e}")
        assert bool(torch.isfinite(u).all()), (case, mode, name)
        assert bool((err <= gate * top).all()), (case, mode, name, line[-1])
    print(f"attention_gqa_vjp {_id(case)} {mode}: " + "  ".join(line) + "  (worst (b, head) slice of max|got - want| / max|want_slice|)")
    if mode == "dead_row":                                                            # exact zeros in the dead row of dq and dgo
        assert not first[0][:, 1, min(3, L - 1)].any() and not first[3][:, 1, min(3, L - 1)].any()
    for name, u, w in zip(NAMES, first, run_vjp(case, mode)):                         # fresh NaN-filled outputs: the same bits
        assert (u is None and w is None) or torch.equal(u, w), name

"""bhg_dwconv_backward_vjp (csrc/bhg_dwconv.hip: k_dw_dgy, k_dw_dx, k_dw_dw_part + k_dw_dw_combine) through the C ABI against the float64
restatement tests/dwconv_ref.py, array by array, on the smallest shapes at which the kernels can still go wrong: one element; odd extents;
an unreached last input row and column (stride 2); scalar and 16-byte staging; several units per workgroup; p = 0 with one output
row; the full padding (output larger than the input); flat and tall outputs with the widest halo (units per workgroup halved to fit LDS); one below / at / one above the tile edge and the slice edge bhg_dwconv_plan reports;
the slice bound taking hold; a DARTS shape with several slices per channel.  Each case with (a, b) both present, a NULL and b NULL.

Before every call dx, dw, dgy and the workspace are filled with NaN, and the outputs sit inside larger sentinel-filled buffers: an element
left unwritten, a stale partial sum read, or a write outside the tensor shows.  Inputs are seeded from the case: N(0, 1) everywhere.
Gate: max|got - want| <= 2e-5 max|want| per array — the project's gate for fp32 kernels against fp64 restatements (ATen's own fp32
evaluation of the three formulas sits at <= 2.5e-7 on these shapes; no case needed more than the gate, so the four-times-ATen rule of
DESIGN 3.27 is not used).  Observed maxima on one MI355X: profiles/dwconv_fp64.txt."""
import functools

import pytest
import torch

import dwconv_ref
from betty_amd import _native
from betty_amd.backend import dwconv_plan

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["both", "no_a", "no_b"]

# (N, C, H, W, k, stride, pad, dil)
ONE = (1, 1, 1, 1, 3, 1, 1, 1)
ODD = (2, 3, 7, 5, 3, 2, 1, 1)                 # odd extents, scalar staging (4 x 3 outputs)
K5S2 = (1, 2, 9, 9, 5, 2, 2, 1)
K5D2 = (3, 5, 8, 13, 5, 1, 4, 2)
K7S2 = (2, 17, 16, 16, 7, 2, 3, 1)             # 8 x 8 outputs: four units per workgroup; 16-byte staging of x and of gy
UNREACHED = (2, 3, 8, 8, 3, 2, 0, 1)           # H_out = 3 reaches rows <= 6: the last row and column of dx are zeros the kernel must write
ONE_ROW = (2, 3, 5, 9, 5, 1, 0, 1)             # p = 0, H_out = 1
FULL_PAD = (2, 3, 4, 6, 3, 1, 4, 2)            # p = d (k - 1): 8 x 10 outputs from 4 x 6 inputs
FULL_PAD7 = (1, 2, 3, 4, 7, 2, 12, 2)
BIG = (2, 65, 33, 33, 3, 1, 2, 2)
DARTS = (4, 16, 32, 32, 5, 1, 2, 1)
SLICE_CAP = (70, 1, 8, 32, 3, 1, 1, 1)         # 70 unit groups of one channel: the bound of 64 slices takes hold (35 slices of 2)
TILE_EDGE = [(2, 65, h, w, 3, 1, 2, 2) for h, w in ((7, 31), (8, 32), (9, 33))]          # th x tw = 8 x 32 (asserted below)
SLICE_EDGE = [(n, 65, 8, 32, 3, 1, 2, 2) for n in (31, 32, 33)]                          # 32 slices per channel at C = 65 (asserted below)
FLAT_WIDE = (1, 2, 13, 45, 7, 2, 0, 2)         # 1 x 17 outputs, 13 x 80 floats per unit and term: pb halved to 4 to fit the LDS budget
FLAT_WIDE_PAD = (3, 5, 1, 64, 7, 2, 6, 2)      # H = 1 at half padding: 1 x 32 outputs, 16-byte staging, 15 units over four workgroups of k_dw_dgy
TALL_NARROW = (2, 3, 45, 13, 7, 2, 0, 2)       # the transpose: 17 x 1 outputs (4-wide tiles, 16 rows)
CASES = [ONE, ODD, K5S2, K5D2, K7S2, UNREACHED, ONE_ROW, FULL_PAD, FULL_PAD7, BIG, DARTS, SLICE_CAP, FLAT_WIDE, FLAT_WIDE_PAD,
         TALL_NARROW] + TILE_EDGE + SLICE_EDGE
_id = lambda c: "x".join(map(str, c[:4])) + "-k%ds%dp%dd%d" % c[4:] if isinstance(c, tuple) else c   # noqa: E731


def out_shape(case):
    N, C, H, W, k, s, p, d = case
    return N, C, dwconv_ref.out_extent(H, k, s, p, d), dwconv_ref.out_extent(W, k, s, p, d)


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(x, w, gy, a, b) on the host, fp32; computed once per case, shared, never written."""
    N, C, H, W, k, s, p, d = case
    g = torch.Generator().manual_seed(sum(v * 31 ** i for i, v in enumerate(case)) % (1 << 31))
    x, a = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    w, b = torch.randn(C, 1, k, k, generator=g), torch.randn(C, 1, k, k, generator=g)
    return x, w, torch.randn(out_shape(case), generator=g), a, b


@functools.lru_cache(maxsize=None)
def wanted(case, mode):
    x, w, gy, a, b = (t.double() for t in host_inputs(case))
    return dwconv_ref.dwconv_backward_vjp(x, w, gy, None if mode == "no_a" else a, None if mode == "no_b" else b, *case[5:])


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    return tuple(t.to(DEV) for t in host_inputs(case))


def _padded(numel, dtype=torch.float32):
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    inner.fill_(float("nan"))
    return buf, inner


def _outside_untouched(buf, numel):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + numel:] == SENTINEL).all())


def run_vjp(case, mode, ws=None):
    """One call on buffers this function owns (the workspace may be handed in: reuse across shapes).  Returns (dx, dw, dgy) on the device
    after checking the bounds of every write and that the inputs are unchanged."""
    lib = _native.load()
    N, C, H, W, k, s, p, d = case
    ins = device_inputs(case)
    before = [t.clone() for t in ins]
    x, w, gy, a, b = ins
    a, b = (None if mode == "no_a" else a), (None if mode == "no_b" else b)
    ws_bytes = int(lib.bhg_dwconv_ws_bytes(C, k))
    assert ws_bytes == 8 * 64 * k * k * C
    if ws is None:
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    assert ws.numel() * 8 >= ws_bytes
    ws.fill_(float("nan"))
    dxbuf, dx = _padded(x.numel())
    dwbuf, dw = _padded(w.numel())
    dgybuf, dgy = _padded(gy.numel())
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = lib.bhg_dwconv_backward_vjp(x.data_ptr(), w.data_ptr(), gy.data_ptr(), ptr(a), ptr(b), N, C, H, W, k, s, p, d, dx.data_ptr(),
                                     dw.data_ptr(), dgy.data_ptr(), ws.data_ptr(), ws.numel() * 8, int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_dwconv_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
    for name, buf, t in (("dx", dxbuf, dx), ("dw", dwbuf, dw), ("dgy", dgybuf, dgy)):
        assert _outside_untouched(buf, t.numel()), f"write outside {name}"
        assert bool(torch.isfinite(t).all()), f"an element of {name} was not written (or a stale value was read)"
    return dx.view(x.shape), dw.view(w.shape), dgy.view(gy.shape)


def check_case(label, case, mode, got=None):
    got = run_vjp(case, mode) if got is None else got
    line = []
    for name, g, want in zip(("dx", "dw", "dgy"), got, wanted(case, mode)):
        scale = float(want.abs().max())
        err = float((g.cpu().double() - want).abs().max())
        if scale == 0.0:                                   # an absent cotangent: exact zeros
            assert err == 0.0, (label, case, mode, name, err)
            line.append(f"{name} 0")
        else:
            line.append(f"{name} {err / scale:.3e}")
            assert err <= GATE * scale, (label, case, mode, name, err / scale)
    print(f"dwconv_vjp {label} {_id(case)} {mode}: " + "  ".join(line) + "  (max|got - want| / max|want|)")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernels_match_the_fp64_restatement(case, mode):
    N, C, H, W, k, s, p, d = case
    plan = dwconv_plan(*case)
    if case in TILE_EDGE:
        assert (plan["th"], plan["tw"]) == (8, 32) and (plan["ty"], plan["tx"]) == ((H + 7) // 8, (W + 31) // 32), plan
    if case in SLICE_EDGE:
        assert (plan["pb"], plan["groups"]) == (1, N) and (plan["slices"], plan["gps"]) == {31: (31, 1), 32: (32, 1), 33: (17, 2)}[N], plan
    if case == SLICE_CAP:
        assert (plan["groups"], plan["slices"], plan["gps"]) == (70, 35, 2), plan
    if case == DARTS:
        assert plan["slices"] == 16 and plan["vec"] == 4 and plan["ivec"] == 4, plan
    if case == K7S2:
        assert plan["pb"] == 4 and plan["ipb"] == 1, plan
    if case in (FLAT_WIDE, FLAT_WIDE_PAD):
        assert (plan["th"], plan["tw"], plan["pb"], plan["rows"], plan["ls"]) == (1, 32, 4, 13, 80) and plan["lds_dgy"] == 33280, plan
    if case == UNREACHED:
        want = wanted(case, mode)[0]
        assert not want[:, :, -1, :].any() and not want[:, :, :, -1].any()     # the unreached row and column
    check_case("case", case, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [ODD, K7S2, DARTS, SLICE_CAP], ids=_id)
def test_the_same_call_twice_is_bit_identical(case):
    first, again = run_vjp(case, "both"), run_vjp(case, "both")
    for name, u, v in zip(("dx", "dw", "dgy"), first, again):
        assert torch.equal(u, v), name


@pytest.mark.gpu
def test_two_consecutive_calls_on_one_workspace_the_larger_first():
    """The second call's slices are fewer than the first's: what the first left in the workspace must not reach the second's dw (run_vjp
    refills the workspace with NaN, so the pair is run on a workspace of its own, filled once)."""
    lib = _native.load()
    big, small = DARTS, (2, 16, 7, 5, 5, 2, 2, 1)
    ws = torch.full((lib.bhg_dwconv_ws_bytes(16, 5) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    outs = []
    for case in (big, small):
        N, C, H, W, k, s, p, d = case
        x, w, gy, a, b = device_inputs(case)
        dx, dw, dgy = torch.full_like(x, float("nan")), torch.full_like(w, float("nan")), torch.full_like(gy, float("nan"))
        rc = lib.bhg_dwconv_backward_vjp(x.data_ptr(), w.data_ptr(), gy.data_ptr(), a.data_ptr(), b.data_ptr(), N, C, H, W, k, s, p, d,
                                         dx.data_ptr(), dw.data_ptr(), dgy.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                         int(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "bhg_dwconv_backward_vjp")
        outs.append((dx, dw, dgy))
    torch.cuda.synchronize()
    for case, got in zip((big, small), outs):
        check_case("shared workspace", case, "both", got=got)

"""bhg_act_backward_vjp and bhg_gated_act_backward_vjp (csrc/bhg_activation.hip: k_act_vjp<kind, vec>, k_gated_act_vjp<kind, vec>)
through the C ABI against the float64 restatement tests/activation_ref.py, array by array.

Plain: n = 1, 3, 4, 5, 255, 256, 257, 1023, 4097 and one n that takes two trips of the grid-stride loop with a ragged last trip and an
n % 4 tail; the same sizes with every pointer offset by one float (the scalar instance); dx NULL; dgy NULL.  Gated: (rows, H) = (1, 1),
(3, 5), (2, 4), (7, 12), (257, 64), a row of more than one workgroup, and two shapes of several trips whose column block carries into
the row group (scalar and 16-byte); each with contiguous arrays (ld = H) and as the halves of one glu buffer (ld = 2 H; with H = 5 the
second half is unaligned); au NULL, av NULL, each output NULL.  Special values 0, -0, +-1e-30, +-8, +-20, +-40, +-100, +-1e4 for every
kind: finite, and within the gate.

Every case first reads the plan and asserts `vec` and the instance.  Outputs are slices of sentinel-filled buffers, NaN-filled before
every call: written everywhere inside their bounds and nowhere outside; a NULL output's buffer stays untouched; the inputs are bit-equal
afterwards; a second run gives the same bits.

Gate, per output array: max|got - want| <= 2e-5 max|want| — the project's gate for fp32 kernels against fp64 restatements — and exactly
zero where want is identically zero.  tests/test_activation_ref.py shows the restatement in float32 passing it.  Observed maxima on
one MI355X: profiles/activation_fp64.txt."""
import functools

import pytest
import torch

import activation_ref as ref
from betty_amd import _native
from betty_amd.backend import activation_plan, gated_activation_plan

DEV = "cuda:0"
GATE = 2e-5
PAD, SENTINEL = 64, 1234.5
TWO_TRIPS = 2048 * 256 * 4 + 4 * 300 + 3                           # 16-byte path: 2048 workgroups, a second trip of 301 units, 3 tail elements
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 4097, TWO_TRIPS)
PLAIN = [(k, 1.0, 20.0) for k in ref.KINDS[:5]] + [("softplus", 1.0, 20.0), ("softplus", 2.0, 5.0)]
SHAPES = ((1, 1), (3, 5), (2, 4), (7, 12), (257, 64))
EXTRA_SHAPES = ((3, 1028), (1400, 601), (700, 2404))             # cb = 2; scalar, cb = 3, 3 trips; 16-byte, cb = 3, 2 trips (step_c = 2: carries)
GATED_MODES = ("all", "no_au", "no_av", "no_du", "no_dv", "no_dgy")


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _close(name, got, want, label):
    scale = float(want.abs().max())
    assert bool(torch.isfinite(got).all()), (label, name, "not finite (an element was not written, or the formula overflowed)")
    err = float((got.double() - want).abs().max())
    if scale == 0.0:
        assert err == 0.0, (label, name, err)
        return 0.0
    assert err <= GATE * scale, (label, name, err / scale)
    return err / scale


def _buffer(numel, offset):
    """A sentinel-filled buffer and its NaN-filled inner slice of `numel` floats, 16-byte aligned when offset == 0, else one float off."""
    buf = torch.full((numel + 2 * PAD + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    inner = buf[PAD + offset:PAD + offset + numel]
    inner.fill_(float("nan"))
    return buf, inner


def _outside_untouched(buf, inner):
    lo = (inner.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + inner.numel():] == SENTINEL).all())


def _input(t, offset):
    """The host tensor on the device, 16-byte aligned or one float off."""
    buf = torch.empty(t.numel() + 1 + 4, dtype=torch.float32, device=DEV)
    d = buf[offset:offset + t.numel()].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == (4 * offset)
    return d


# ---- plain --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_inputs(kind, beta, threshold, n, special=False):
    g = torch.Generator().manual_seed(n * 7 + ref.KIND_ID[kind])
    x = 3.0 * torch.randn(n, generator=g)
    if special:
        x[:len(ref.SPECIAL)] = ref.special_values(torch.float32)
    if kind == "softplus":
        x = ref.softplus_safe(x, beta, threshold)
    return x, torch.randn(n, generator=g), torch.randn(n, generator=g)


@functools.lru_cache(maxsize=None)
def plain_wanted(kind, beta, threshold, n, special=False):
    x, gy, a = (t.double() for t in plain_inputs(kind, beta, threshold, n, special))
    return ref.act_backward_vjp(kind, x, gy, a, beta, threshold)


def run_plain(kind, beta, threshold, n, offset, mode, special=False):
    lib = _native.load()
    host = plain_inputs(kind, beta, threshold, n, special)
    ins = [_input(t, offset) for t in host]
    bufs = [_buffer(n, offset) for _ in range(2)]
    on = (mode != "no_dx", mode != "no_dgy")
    ptrs = [inner.data_ptr() if w else None for (_, inner), w in zip(bufs, on)]
    aligned = all(p is None or p % 16 == 0 for p in [t.data_ptr() for t in ins] + ptrs)
    assert aligned == (offset == 0)
    plan = activation_plan(n, aligned)                               # the plan first: vec and the instance
    assert plan["vec"] == (4 if aligned else 1) and plan["inst"] == f"k_act_vjp<kind,{plan['vec']}>", plan
    if n == TWO_TRIPS:
        assert (plan["grid"], plan["iters"]) == ((2048, 2) if aligned else (2048, 5)) and plan["units"] % 256 != 0, plan
    _native.check(lib.bhg_act_backward_vjp(ref.KIND_ID[kind], beta, threshold, *(t.data_ptr() for t in ins), *ptrs, n, _stream()),
                  "bhg_act_backward_vjp")
    torch.cuda.synchronize()
    for t, h in zip(ins, host):
        assert torch.equal(t.cpu(), h), "an input was modified"
    outs = []
    for name, (buf, inner), w in zip(("dx", "dgy"), bufs, on):
        assert _outside_untouched(buf, inner), f"write outside {name}"
        if w:
            assert not bool(torch.isnan(inner).any()), f"an element of {name} was not written"
            outs.append(inner.cpu())
        else:
            assert bool(torch.isnan(inner).all()), f"{name} was not given: its buffer must stay untouched"
            outs.append(None)
    return outs


def check_plain(kind, beta, threshold, n, offset, mode, special=False):
    label = (kind, beta, threshold, n, offset, mode)
    first = run_plain(kind, beta, threshold, n, offset, mode, special)
    worst = 0.0
    for name, got, want in zip(("dx", "dgy"), first, plain_wanted(kind, beta, threshold, n, special)):
        if got is not None:
            worst = max(worst, _close(name, got, want, label))
    again = run_plain(kind, beta, threshold, n, offset, mode, special)
    for u, v in zip(first, again):
        assert (u is None and v is None) or torch.equal(u, v), (label, "a second run gave other bits")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all", "no_dx", "no_dgy"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("kind,beta,threshold", PLAIN, ids=lambda v: str(v))
def test_plain_kernels_match_the_fp64_restatement(kind, beta, threshold, offset, mode):
    worst = max(check_plain(kind, beta, threshold, n, offset, mode) for n in SIZES)
    print(f"act_vjp {kind} beta={beta} threshold={threshold} vec={4 if offset == 0 else 1} {mode}: worst {worst:.3e} of max|want| over n = {SIZES}")


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("kind,beta,threshold", PLAIN, ids=lambda v: str(v))
def test_plain_kernels_on_special_values(kind, beta, threshold, offset):
    worst = check_plain(kind, beta, threshold, 257, offset, "all", special=True)
    print(f"act_vjp {kind} beta={beta} threshold={threshold} vec={4 if offset == 0 else 1} special values: worst {worst:.3e} of max|want|")


# ---- gated --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gated_inputs(kind, rows, H, special=False):
    g = torch.Generator().manual_seed((rows * 131 + H) * 7 + ref.KIND_ID[kind])
    u = 3.0 * torch.randn(rows, H, generator=g)
    if special:
        u.view(-1)[:len(ref.SPECIAL)] = ref.special_values(torch.float32)
    return (u,) + tuple(torch.randn(rows, H, generator=g) for _ in range(4))            # u, v, gy, au, av


@functools.lru_cache(maxsize=None)
def gated_wanted(kind, rows, H, has_au, has_av, special=False):
    u, v, gy, au, av = (t.double() for t in gated_inputs(kind, rows, H, special))
    return ref.gated_backward_vjp(kind, u, v, gy, au if has_au else None, av if has_av else None)


def _halves(first, second, H):
    """One [rows, 2 H] device buffer holding `first` | `second`, and the two strided views."""
    rows = first.shape[0]
    buf = torch.empty(rows * 2 * H + 4, dtype=torch.float32, device=DEV)[:rows * 2 * H].view(rows, 2 * H)
    buf[:, :H].copy_(first)
    buf[:, H:].copy_(second)
    return buf[:, :H], buf[:, H:]


def run_gated(kind, rows, H, layout, mode, special=False):
    lib = _native.load()
    hu, hv, hgy, hau, hav = gated_inputs(kind, rows, H, special)
    has_au, has_av = mode != "no_au", mode != "no_av"
    on = {"du": mode != "no_du", "dv": mode != "no_dv", "dgy": mode != "no_dgy"}
    gy = _input(hgy, 0)
    dgy_buf, dgy = _buffer(rows * H, 0)
    if layout == "glu":                                              # x = [v | u], a = [av | au], dx = [dv | du]: ld = 2 H
        v, u = _halves(hv, hu, H)
        av, au = _halves(hav, hau, H)
        dx_buf, dx = _buffer(rows * 2 * H, 0)
        dx2 = dx.view(rows, 2 * H)
        dv, du = dx2[:, :H], dx2[:, H:]
        ld, out_bufs = 2 * H, [(dx_buf, dx)]
    else:
        u, v, au, av = (_input(t, 0) for t in (hu, hv, hau, hav))
        (du_buf, du), (dv_buf, dv) = _buffer(rows * H, 0), _buffer(rows * H, 0)
        du, dv = du.view(rows, H), dv.view(rows, H)
        ld, out_bufs = H, [(du_buf, du), (dv_buf, dv)]
    out_bufs.append((dgy_buf, dgy))
    arrays = [(u, ld, True), (v, ld, True), (gy, H, True), (au, ld, has_au), (av, ld, has_av), (du, ld, on["du"]), (dv, ld, on["dv"]),
              (dgy, H, on["dgy"])]
    vec_ok = all((not w) or (t.data_ptr() % 16 == 0 and l % 4 == 0) for t, l, w in arrays)
    plan = gated_activation_plan(rows, H, vec_ok)                    # the plan first: vec and the instance
    want_vec = 4 if (H % 4 == 0) else 1                              # with H % 4 == 0 both layouts are aligned; H = 5 and H = 1 are not vectors
    assert plan["vec"] == want_vec and plan["inst"] == f"k_gated_act_vjp<kind,{want_vec}>", plan
    if layout == "glu" and H == 5:
        assert u.data_ptr() % 16 != 0                                # the second half is unaligned
    if (rows, H) == (3, 1028):
        assert plan["cb"] == 2, plan
    if (rows, H) == (1400, 601):
        assert (plan["cb"], plan["iters"], plan["grid"]) == (3, 3, 2048), plan
    if (rows, H) == (700, 2404):
        assert (plan["cb"], plan["iters"], plan["grid"]) == (3, 2, 2048), plan
    args = []
    for t, l, w in arrays:
        args += [t.data_ptr() if w else None, l]
    _native.check(lib.bhg_gated_act_backward_vjp(ref.KIND_ID[kind], rows, H, *args, _stream()), "bhg_gated_act_backward_vjp")
    torch.cuda.synchronize()
    for t, h in zip((u, v, gy, au, av), (hu, hv, hgy, hau, hav)):
        assert torch.equal(t.cpu(), h), "an input was modified"
    for buf, inner in out_bufs:
        assert _outside_untouched(buf, inner), "write outside an output"
    outs = []
    for name, t in (("du", du), ("dv", dv), ("dgy", dgy.view(rows, H))):
        if on[name]:
            assert not bool(torch.isnan(t).any()), f"an element of {name} was not written"
            outs.append(t.cpu())
        else:
            assert bool(torch.isnan(t).all()), f"{name} was not given: its buffer must stay untouched"
            outs.append(None)
    return outs


def check_gated(kind, rows, H, layout, mode, special=False):
    label = (kind, rows, H, layout, mode)
    first = run_gated(kind, rows, H, layout, mode, special)
    worst = 0.0
    for name, got, want in zip(("du", "dv", "dgy"), first, gated_wanted(kind, rows, H, mode != "no_au", mode != "no_av", special)):
        if got is not None:
            worst = max(worst, _close(name, got, want, label))
    again = run_gated(kind, rows, H, layout, mode, special)
    for u, v in zip(first, again):
        assert (u is None and v is None) or torch.equal(u, v), (label, "a second run gave other bits")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("mode", GATED_MODES)
@pytest.mark.parametrize("layout", ["contiguous", "glu"])
@pytest.mark.parametrize("kind", ref.GATED_KINDS)
def test_gated_kernels_match_the_fp64_restatement(kind, layout, mode):
    shapes = SHAPES + (EXTRA_SHAPES if mode == "all" else EXTRA_SHAPES[:1])
    worst = max(check_gated(kind, rows, H, layout, mode) for rows, H in shapes)
    print(f"gated_act_vjp {kind} {layout} {mode}: worst {worst:.3e} of max|want| over (rows, H) = {shapes}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "glu"])
@pytest.mark.parametrize("kind", ref.GATED_KINDS)
def test_gated_kernels_on_special_values(kind, layout):
    worst = max(check_gated(kind, rows, H, layout, "all", special=True) for rows, H in ((7, 12), (3, 5)))
    print(f"gated_act_vjp {kind} {layout} special values: worst {worst:.3e} of max|want|")

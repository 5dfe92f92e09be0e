"""The fused batch-norm double backward (csrc/bhg_bn.hip: k_bn_vjp_stats + k_bn_vjp_apply) through the C ABI, against the fp64
restatement tests/bn_ref.py evaluated on the kernel's own fp32 mean / invstd, in every regime of its slicing: several chunks per run on
the vector and on the scalar path, a ragged last chunk, a ragged last sample group, the group-shrinking loop, the slice bound taking
hold, every `tpr`, thousands of channels.  Each case first reads the plan (bhg_bn_plan, the slicing function the launch calls) and
asserts the regime it is named for, so a later change of the map fails here instead of quietly testing something else.

Inputs per case, seeded from the shape: x = 1.7 N(0, 1) + 0.3, gy, a ~ N(0, 1), gamma in [0.5, 1.5), b, c ~ N(0, 1).
Gate, PER CHANNEL: max|got_c - want_c| <= 2e-6 max|want_c| over the channel's N * H * W elements of dx and of dgy, and
|got_c - want_c| <= 2e-6 |want_c| for dgamma.  The kernels form every output in fp64 and round once at the store: the expected error is
one fp32 rounding, 6e-8 of the element.  test_the_gate_can_exclude_no_case (CPU) shows that the fp64 reference rounded to fp32 passes
and that dgamma is well-conditioned in every channel (bn_ref and autograd's fp64 double backward agree to 1e-9 of it).  Every shape has
M = N * H * W >= 16 per channel (the cancellation regime of two elements per channel stays in tests/test_fused_batchnorm.py).
Observed maxima on one MI355X: profiles/bn_vjp_fp64.txt.

Every case also checks: dx, dgy, dgamma and the workspace — slices of larger sentinel-filled buffers — were written inside their bounds
only and dx, dgy, dgamma everywhere inside; a NULL output's buffer stays untouched; the inputs are bit-equal afterwards; a second run on
a workspace full of NaN gives the same bits (deterministic, and the apply launch reads no partial the stats launch did not write).
Not held here: tensors past 2^31 elements (the 64-bit offsets are right by reading; no test allocates 40 GB to show it)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import bn_ref
from betty_amd import _native
from betty_amd.backend import bn_plan

DEV = "cuda:0"
GATE = 2e-6
EPS = 1e-5
PAD, SENTINEL, SENTINEL_BYTE = 64, 1234.5, 0xA5
NAN_FILL_LIMIT = 256 << 20
NULLS = ["none", "affine_false", "no_a", "no_bc"]

# (N, C, H, W) -> the part of the plan the case is there for
CLAMP_VEC = ((1, 1, 1026, 512), dict(vec=4, groups=1, chunks=512, chunk=1028))      # 513 chunks before the slice bound; last chunk 4 long
CLAMP_SCALAR = ((1, 3, 1, 525313), dict(vec=1, groups=1, chunks=512, chunk=1028))   # last chunk 5 long
TWO_IMAGES = ((2, 1, 1024, 1024), dict(vec=4, groups=1, ng=2, chunks=512, chunk=2048))
RAGGED_VEC = ((2, 3, 2, 1028), dict(vec=4, groups=1, ng=2, chunks=3, chunk=688))    # 688 + 688 + 680
RAGGED_SCALAR = ((1, 3, 37, 53), dict(vec=1, chunks=2, chunk=984))                  # 984 + 977
RAGGED_GROUP = ((257, 1, 2, 4), dict(vec=4, ng=128, groups=3, chunks=1, tpr=16))    # 16 rows side by side; the last group is 1 sample
SHAPES = [
    CLAMP_VEC, CLAMP_SCALAR, TWO_IMAGES, RAGGED_VEC, RAGGED_SCALAR,
    # the group-shrinking loop: ng 1 -> 5
    ((200, 1, 1, 10244), dict(vec=4, ng=5, groups=40, chunks=11, chunk=932)),
    ((200, 1, 1, 10241), dict(vec=1, ng=5, groups=40, chunks=11, chunk=932)),
    ((130, 1, 1, 15364), dict(vec=4, ng=5, groups=26, chunks=16, chunk=964)),
    RAGGED_GROUP,
    # every tpr, vector path
    ((5, 7, 6, 6), dict(vec=4, tpr=16)), ((5, 7, 10, 10), dict(vec=4, tpr=32)), ((5, 7, 10, 20), dict(vec=4, tpr=64)),
    ((5, 7, 20, 20), dict(vec=4, tpr=128, ng=3, groups=2)), ((5, 7, 32, 32), dict(vec=4, tpr=256)),
    # every tpr, scalar path
    ((5, 7, 3, 3), dict(vec=1, tpr=16)), ((5, 7, 3, 7), dict(vec=1, tpr=32)), ((5, 7, 7, 7), dict(vec=1, tpr=64)),
    ((5, 7, 11, 11), dict(vec=1, tpr=128)), ((5, 7, 21, 21), dict(vec=1, tpr=256, ng=3, groups=2)),
    # many channels, one slice each (84 MB of workspace)
    ((4, 4099, 2, 2), dict(vec=4, slices=1, tpr=16)),
]
NULL_SHAPES = [CLAMP_VEC, CLAMP_SCALAR, RAGGED_VEC, RAGGED_SCALAR, RAGGED_GROUP]
LEAK_SHAPES = [((25, 8, 10, 10), dict(vec=4, tpr=32, ng=11, groups=3)), RAGGED_VEC]
FAR_MEAN = ((25, 8, 21, 21), dict(vec=1, ng=3, groups=9, tpr=256))
_ids = lambda case: "x".join(map(str, case[0]))   # noqa: E731


# ---- inputs and the fp64 reference: computed once per case, shared, never written -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_inputs(shape, variant="plain"):
    """(x, gy, a, gamma, b, c, mean32, invstd32) on the host, fp32.  variant "leak": channel 0 has gy, a scaled by 1e-4 and x by 1e3 (a
    channel a whole-tensor norm does not see); "far_mean": x = 100 + 0.01 N(0, 1)."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(((N * 31 + C) * 31 + H) * 31 + W)
    x = torch.randn(shape, generator=g) * 1.7 + 0.3
    gy = torch.randn(shape, generator=g)
    a = torch.randn(shape, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    c = torch.randn(C, generator=g)
    if variant == "leak":
        x[:, 0] *= 1e3
        gy[:, 0] *= 1e-4
        a[:, 0] *= 1e-4
    elif variant == "far_mean":
        x = 100.0 + 0.01 * (x - 0.3) / 1.7
    else:
        assert variant == "plain"
    xd = x.double()
    mean = xd.mean((0, 2, 3))
    invstd = (xd.var((0, 2, 3), unbiased=False) + EPS).rsqrt()
    return x, gy, a, gamma, b, c, mean.float(), invstd.float()


def _select(nulls, a, gamma, b, c):
    """The existing NULL combinations of tests/test_fused_batchnorm.py."""
    return (None if nulls == "no_a" else a, None if nulls == "affine_false" else gamma,
            None if nulls in ("no_bc", "affine_false") else b, None if nulls in ("no_bc", "affine_false") else c)


@functools.lru_cache(maxsize=None)
def wanted(shape, variant="plain", nulls="none"):
    """(dx, dgy, dgamma | None) in fp64 on the host: bn_ref on the fp32 inputs and on the fp32 mean / invstd the kernel is given."""
    x, gy, a, gamma, b, c, mean32, inv32 = host_inputs(shape, variant)
    a, gamma, b, c = _select(nulls, a, gamma, b, c)
    d = lambda t: None if t is None else t.double()   # noqa: E731
    return bn_ref.bn_backward_vjp(x.double(), gy.double(), d(a), d(gamma), mean32.double(), inv32.double(), d(b), d(c))


def per_channel(got, want):
    """(largest max|got_c - want_c| / max|want_c| over the channels, all channels inside the gate).  got, want: [N, C, H, W] or [C]."""
    diff = (got.double() - want).abs()
    err, scale = (diff.amax((0, 2, 3)), want.abs().amax((0, 2, 3))) if want.dim() == 4 else (diff, want.abs())
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()), bool((err <= GATE * scale).all())


# ---- CPU: the gate excludes no case ---------------------------------------------------------------------------------------------------
def _autograd_dgamma(x, gy, a, gamma, b, c):
    """d( <a, gx> + <b, ggamma> + <c, gbeta> ) / d gamma by autograd's own double backward of batch norm, fp64, its own statistics."""
    x, gamma = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    beta = torch.zeros_like(gamma, requires_grad=True)
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS)
    first = torch.autograd.grad(y, (x, gamma, beta), gy, create_graph=True)
    phi = (first[0] * a).sum() + (first[1] * b).sum() + (first[2] * c).sum()
    return torch.autograd.grad(phi, gamma)[0]


ALL_CASES = [(s, "plain") for s, _ in SHAPES] + [(s, "leak") for s, _ in LEAK_SHAPES] + [(FAR_MEAN[0], "far_mean")]


@pytest.mark.parametrize("shape,variant", [sv for sv in ALL_CASES if sv[0][0] * sv[0][1] * sv[0][2] * sv[0][3] < 1 << 20],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_the_gate_can_exclude_no_case(shape, variant):
    N, C, H, W = shape
    assert N * H * W >= 16
    for nulls in NULLS if (shape, variant) in [(s, "plain") for s, _ in NULL_SHAPES] else ["none"]:
        for name, w in zip(("dx", "dgy", "dgamma"), wanted(shape, variant, nulls)):
            if w is None:
                continue
            assert bool(torch.isfinite(w).all())
            ratio, ok = per_channel(w.float(), w)
            assert ok and ratio <= 6.0e-8, (name, nulls, ratio)     # one rounding to fp32: 2^-24
    # dgamma = invstd (M A - Sa Sg - P Q) / M is a difference: two fp64 routes agree to 1e-9 of it in EVERY channel, so the relative gate
    # on a single number does not sit on a cancelled one
    x, gy, a, gamma, b, c, _, _ = (t.double() for t in host_inputs(shape, variant))
    mean = x.mean((0, 2, 3))
    invstd = (x.var((0, 2, 3), unbiased=False) + EPS).rsqrt()
    closed = bn_ref.bn_backward_vjp(x, gy, a, gamma, mean, invstd, b, c)[2]
    auto = _autograd_dgamma(x, gy, a, gamma, b, c)
    worst = float(((closed - auto).abs() / closed.abs()).max())
    print(f"bn_vjp conditioning {shape} {variant}: dgamma, closed form vs autograd fp64: {worst:.3e} of |dgamma_c|, min |dgamma_c| = {float(closed.abs().min()):.3e}")
    assert bool(((closed - auto).abs() <= 1e-9 * closed.abs()).all()), worst


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_inputs(shape, variant="plain"):
    return tuple(t.to(DEV) for t in host_inputs(shape, variant))


def _padded(numel, dtype, fill):
    buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    return buf, inner


def _outside_untouched(buf, numel, fill):
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + numel:] == fill).all())


def run_vjp(shape, variant="plain", nulls="none", nan_ws=False):
    """One bhg_bn_backward_vjp call on buffers this function owns.  Returns (dx, dgy, dgamma | None) on the device after checking the
    bounds of every write, that every output element was written, and that the inputs are unchanged."""
    lib = _native.load()
    N, C, H, W = shape
    ins = device_inputs(shape, variant)
    before = [t.clone() for t in ins]
    x, gy, a, gamma, b, c, mean32, inv32 = ins
    a, gamma, b, c = _select(nulls, a, gamma, b, c)
    numel, ws_bytes = x.numel(), int(lib.bhg_bn_ws_bytes(C))
    assert ws_bytes == 8 * 5 * 512 * C
    dxbuf, dx = _padded(numel, torch.float32, SENTINEL)
    dgybuf, dgy = _padded(numel, torch.float32, SENTINEL)
    dgbuf, dgamma = _padded(C, torch.float32, SENTINEL)
    wsbuf, ws = _padded(ws_bytes, torch.uint8, SENTINEL_BYTE)
    if nan_ws and ws_bytes <= NAN_FILL_LIMIT:
        ws.view(torch.float64).fill_(float("nan"))
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = lib.bhg_bn_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a), ptr(gamma), mean32.data_ptr(), inv32.data_ptr(), ptr(b), ptr(c),
                                 N, C, H * W, dx.data_ptr(), dgy.data_ptr(), ptr(dgamma if gamma is not None else None), ws.data_ptr(),
                                 ws_bytes, int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_bn_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
    assert _outside_untouched(dxbuf, numel, SENTINEL) and _outside_untouched(dgybuf, numel, SENTINEL), "write outside dx / dgy"
    assert _outside_untouched(dgbuf, C, SENTINEL), "write outside dgamma"
    assert _outside_untouched(wsbuf, ws_bytes, SENTINEL_BYTE), "write outside the workspace"
    assert not bool((dx == SENTINEL).any()) and not bool((dgy == SENTINEL).any()), "an element of dx / dgy was not written"
    if gamma is None:
        assert bool((dgbuf == SENTINEL).all()), "dgamma is NULL: its buffer must stay untouched"
    else:
        assert not bool((dgamma == SENTINEL).any()), "a channel of dgamma was not written"
    return dx.view(shape), dgy.view(shape), (dgamma if gamma is not None else None)


def check_case(label, case, variant="plain", nulls="none"):
    shape, regime = case
    N, C, H, W = shape
    assert N * H * W >= 16
    plan = bn_plan(N, C, H * W)
    assert {k: plan[k] for k in regime} == regime, (shape, plan)
    first = run_vjp(shape, variant, nulls)
    again = run_vjp(shape, variant, nulls, nan_ws=True)
    line = []
    for name, got, rerun, want in zip(("dx", "dgy", "dgamma"), first, again, wanted(shape, variant, nulls)):
        if want is None:
            assert got is None and rerun is None
            continue
        assert torch.equal(got, rerun), f"{name}: two runs differ (the second on a workspace full of NaN)"
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), name
        ratio, ok = per_channel(got, want)
        line.append((name, ratio, ok))
    print(f"bn_vjp {label} {shape} {nulls}: " + "  ".join(f"{n} {r:.3e}" for n, r, _ in line) + "  (largest per-channel error / max|want_c|)")
    for name, ratio, ok in line:
        assert ok, (label, shape, nulls, name, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPES, ids=_ids)
def test_every_slicing_regime_matches_the_fp64_reference_per_channel(case):
    check_case("regime", case)


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", NULLS[1:])
@pytest.mark.parametrize("case", NULL_SHAPES, ids=_ids)
def test_null_cotangents_and_affine_false(case, nulls):
    """Where a pointer is NULL the buffer it would have used stays all sentinel (run_vjp)."""
    check_case("nulls", case, nulls=nulls)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEAK_SHAPES, ids=_ids)
def test_channels_do_not_leak_into_each_other(case):
    """Channel 0's gy and a are 1e-4 of the other channels' and its x 1e3 of theirs: its dx and dgy are orders of magnitude away from the
    others', and one norm over the whole tensor would not see an error in the smaller."""
    x, gy = host_inputs(case[0], "leak")[:2]
    assert float(gy[:, 0].abs().max()) < 1e-3 * float(gy[:, 1].abs().max()) and float(x[:, 0].abs().max()) > 1e2 * float(x[:, 1].abs().max())
    check_case("leak", case, variant="leak")


@pytest.mark.gpu
def test_mean_far_from_zero():
    """x = 100 + 0.01 N(0, 1): x - mean must be formed in fp64 from the fp32 mean the kernel is given."""
    check_case("far mean", FAR_MEAN, variant="far_mean")

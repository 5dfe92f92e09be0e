"""tests/activation_ref.py, the float64 restatement of the declared activations' double backward, against autograd's own double backward
of the torch functions in float64: all six kinds, the gated form for the five kinds that have one, F.glu, each cotangent absent in turn.
Inputs: 4000 values of 3 N(0, 1) and 0, -0, +-1e-30, +-8, +-20, +-40, +-100, +-1e4; softplus with (beta, threshold) = (1, 20) and (2, 5),
its inputs kept 1e-3 away from beta x = threshold, where ATen's formula is discontinuous.  Gate: 1e-10 of max|want|.

The same file shows that the restatement evaluated in float32 passes the kernels' gate (2e-5 of max|want| per array, exactly zero where
want is identically zero) on these inputs: the gate of tests/test_activation_kernels.py excludes no input by the formulas alone."""
import pytest
import torch

import activation_ref as ref

GATE = 1e-10
KERNEL_GATE = 2e-5
SOFTPLUS = [(1.0, 20.0), (2.0, 5.0)]
PLAIN = [(k, 1.0, 20.0) for k in ref.KINDS[:5]] + [("softplus", b, t) for b, t in SOFTPLUS]


def _inputs(kind, beta, threshold, seed):
    x = ref.sample_inputs(seed=seed)
    if kind == "softplus":
        x = ref.softplus_safe(x, beta, threshold)
        assert bool(((beta * x - threshold).abs() >= 1e-3).all())
    g = torch.Generator().manual_seed(seed + 100)
    return [x] + [torch.randn(x.shape, generator=g, dtype=torch.float64) for _ in range(4)]


def _close(got, want, gate=GATE):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    assert bool(torch.isfinite(got).all())
    assert err <= gate * scale, (err, scale)
    return err / scale if scale > 0 else 0.0


@pytest.mark.parametrize("kind,beta,threshold", PLAIN, ids=lambda v: str(v))
def test_plain_form_against_autograd(kind, beta, threshold):
    x, gy, a, _, _ = _inputs(kind, beta, threshold, 1)
    x.requires_grad_(True)
    gy.requires_grad_(True)
    y = ref.torch_function(kind, beta, threshold)(x)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    want_dx, want_dgy = torch.autograd.grad(gx, [x, gy], a)
    dx, dgy = ref.act_backward_vjp(kind, x.detach(), gy.detach(), a, beta, threshold)
    print(f"activation_ref {kind} beta={beta} threshold={threshold}: dx {_close(dx, want_dx):.2e} dgy {_close(dgy, want_dgy):.2e} of max|want|")


@pytest.mark.parametrize("absent", ["none", "au", "av"])
@pytest.mark.parametrize("kind", ref.GATED_KINDS)
def test_gated_form_against_autograd(kind, absent):
    u, v, gy, au, av = _inputs(kind, 1.0, 20.0, 2)
    v = 2.0 * v
    for t in (u, v, gy):
        t.requires_grad_(True)
    y = ref.torch_function(kind)(u) * v
    gu, gv = torch.autograd.grad(y, [u, v], gy, create_graph=True)
    outs, cots = {"none": ([gu, gv], [au, av]), "au": ([gv], [av]), "av": ([gu], [au])}[absent]
    want = torch.autograd.grad(outs, [u, v, gy], cots, allow_unused=True)
    got = ref.gated_backward_vjp(kind, u.detach(), v.detach(), gy.detach(), None if absent == "au" else au, None if absent == "av" else av)
    for name, g, w in zip(("du", "dv", "dgy"), got, want):
        if w is None:
            assert not g.any(), name                                # av alone: gv does not depend on v
        else:
            _close(g, w)


def test_glu_against_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([3.0 * torch.randn(50, 40, generator=g, dtype=torch.float64), ref.special_values().repeat(3)[:40].reshape(1, 40)])
    gy = torch.randn(51, 20, generator=g, dtype=torch.float64)
    a = torch.randn(51, 40, generator=g, dtype=torch.float64)
    x.requires_grad_(True)
    gy.requires_grad_(True)
    y = torch.nn.functional.glu(x, -1)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    want_dx, want_dgy = torch.autograd.grad(gx, [x, gy], a, retain_graph=True)
    dx, dgy = ref.glu_backward_vjp(x.detach(), gy.detach(), a)
    _close(dx, want_dx)
    _close(dgy, want_dgy)
    # each half of the cotangent absent in turn (a zero half)
    for half in (slice(0, 20), slice(20, 40)):
        a0 = a.clone()
        a0[:, half] = 0.0
        want_dx, want_dgy = torch.autograd.grad(gx, [x, gy], a0, retain_graph=True)
        H = 20
        au, av = (None if half.start == 20 else a0[:, H:]), (None if half.start == 0 else a0[:, :H])
        du, dv, dgy = ref.gated_backward_vjp("sigmoid", x.detach()[:, H:], x.detach()[:, :H], gy.detach(), au, av)
        _close(torch.cat([dv, du], -1), want_dx)
        _close(dgy, want_dgy)


@pytest.mark.parametrize("kind,beta,threshold", PLAIN, ids=lambda v: str(v))
def test_the_formulas_in_float32_pass_the_kernel_gate(kind, beta, threshold):
    x, gy, a, v, av = _inputs(kind, beta, threshold, 4)
    x32 = x.float()
    if kind == "softplus":
        x32 = ref.softplus_safe(x32, beta, threshold)
    x = x32.double()                                                # the float64 values of the very float32 inputs
    gy, a, v, av = (t.float().double() for t in (gy, a, v, av))
    want = ref.act_backward_vjp(kind, x, gy, a, beta, threshold)
    got = ref.act_backward_vjp(kind, x32, gy.float(), a.float(), beta, threshold)
    worst = max(_close(g, w, KERNEL_GATE) for g, w in zip(got, want))
    if kind in ref.GATED_KINDS:
        want = ref.gated_backward_vjp(kind, x, v, gy, a, av)
        got = ref.gated_backward_vjp(kind, x32, v.float(), gy.float(), a.float(), av.float())
        worst = max([worst] + [_close(g, w, KERNEL_GATE) for g, w in zip(got, want)])
    print(f"activation_ref float32 {kind}: worst {worst:.2e} of max|want| (gate {KERNEL_GATE})")

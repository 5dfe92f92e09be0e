"""tests/cross_entropy_ref.py (the float64 restatement bhg_cross_entropy_backward_vjp is held to) against autograd's own double
backward of F.cross_entropy in float64: reductions none / mean / sum, with and without ignored rows, every row ignored (none and sum:
under mean the loss itself is 0 / 0), one class, targets at class 0 and at class C - 1."""
import pytest
import torch
import torch.nn.functional as F

import cross_entropy_ref as ref

IGNORE = -100
# (N, C, which rows are ignored, which targets)
SHAPES = [(7, 5, (), "random"), (7, 5, (0, 3, 6), "random"), (4, 1, (), "random"), (4, 1, (2,), "random"), (6, 9, (), "first"),
          (6, 9, (1,), "last"), (1, 1, (), "random"), (3, 130, (1,), "random")]
ALL_IGNORED = (5, 4, (0, 1, 2, 3, 4), "random")


def _problem(N, C, ignored, targets, reduction, seed=0):
    gen = torch.Generator().manual_seed(seed + 131 * N + C)
    z = torch.randn(N, C, generator=gen, dtype=torch.float64, requires_grad=True)
    y = {"random": torch.randint(0, C, (N,), generator=gen), "first": torch.zeros(N, dtype=torch.long),
         "last": torch.full((N,), C - 1)}[targets]
    for i in ignored:
        y[i] = IGNORE
    g = torch.randn(N if reduction == "none" else (), generator=gen, dtype=torch.float64).requires_grad_(True)
    a = torch.randn(N, C, generator=gen, dtype=torch.float64)
    return z, y, g, a


def _autograd(z, y, g, a, reduction):
    loss = F.cross_entropy(z, y, reduction=reduction, ignore_index=IGNORE)
    (gz,) = torch.autograd.grad(loss, z, grad_outputs=g, create_graph=True)
    if not gz.requires_grad:   # every row ignored: the gradient is a constant zero
        return gz.detach(), torch.zeros_like(z), torch.zeros_like(g)
    dz, dg = torch.autograd.grad(gz, (z, g), grad_outputs=a, allow_unused=True)
    return gz.detach(), (torch.zeros_like(z) if dz is None else dz), (torch.zeros_like(g) if dg is None else dg)


# every row ignored: none and sum only (under mean the loss itself is 0 / 0)
PROBLEMS = [(s, r) for s in SHAPES for r in ("none", "mean", "sum")] + [(ALL_IGNORED, "none"), (ALL_IGNORED, "sum")]


@pytest.mark.parametrize("shape,reduction", PROBLEMS, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}-ignored{len(v[2])}-{v[3]}")
def test_restatement_matches_autograd_in_float64(shape, reduction):
    N, C, ignored, targets = shape
    z, y, g, a = _problem(N, C, ignored, targets, reduction)
    gz, dz, dg = _autograd(z, y, g, a, reduction)
    lsm = torch.log_softmax(z.detach(), dim=1)
    denom = ref.valid(y, C, IGNORE).sum().double() if reduction == "mean" else None
    scalar = reduction != "none"
    got_gz = ref.cross_entropy_first_backward(lsm, y, g.detach(), IGNORE, denom, scalar_g=scalar)
    got_dz, got_dg = ref.cross_entropy_backward_vjp(lsm, y, g.detach(), a, IGNORE, denom, scalar_g=scalar)
    assert got_dg.shape == g.shape
    for name, u, v in (("gz", got_gz, gz), ("dz", got_dz, dz), ("dg", got_dg, dg)):
        assert float((u - v).abs().max()) <= 1e-13 * max(1.0, float(v.abs().max())), (name, shape, reduction)
    for i in ignored:
        assert not got_dz[i].any() and (reduction != "none" or float(got_dg[i]) == 0.0)


def test_an_out_of_range_target_is_an_ignored_row():
    z, y, g, a = _problem(6, 7, (2,), "random", "none")
    lsm = torch.log_softmax(z.detach(), dim=1)
    want = ref.cross_entropy_backward_vjp(lsm, y, g.detach(), a, IGNORE)
    for bad in (7, -1, 1 << 40):
        y2 = y.clone()
        y2[2] = bad
        got = ref.cross_entropy_backward_vjp(lsm, y2, g.detach(), a, IGNORE)
        assert all(torch.equal(u, v) for u, v in zip(got, want))


def test_ignored_rows_do_not_read_their_inputs():
    z, y, g, a = _problem(6, 7, (0, 5), "random", "sum")
    lsm = torch.log_softmax(z.detach(), dim=1)
    want = ref.cross_entropy_backward_vjp(lsm, y, g.detach(), a, IGNORE)
    lsm[0], a[5] = float("nan"), float("inf")
    got = ref.cross_entropy_backward_vjp(lsm, y, g.detach(), a, IGNORE)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    sdz, sdg = ref.gate_scales(lsm, y, g.detach(), a, IGNORE)
    assert bool(torch.isfinite(sdz).all()) and bool(torch.isfinite(sdg))

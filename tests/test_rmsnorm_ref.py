"""tests/rmsnorm_ref.py — the float64 restatement the RMS-norm kernels (csrc/bhg_rmsnorm.hip) are held to — against autograd's own double
backward of F.rms_norm in float64: (M, D) in {(1, 1), (3, 2), (2, 3), (5, 9), (4, 1000), (2, 8192)} x {plain, the eps-dominated input
x = 1e-4 N(0, 1) with eps = 1e-5, eps=None} x every combination of absent a / gamma / b.
Gate: max|got - want| <= 1e-9 max|want| per array.  At D = 1 the results are differences of nearly equal terms (1 - xh^2 = eps r^2: the
result itself is of the order of eps), so there the gate is relative to the largest sum of absolute terms (rmsnorm_ref.elementwise_abs_terms,
dgamma_abs_terms).  The test prints the worst ratio."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import rmsnorm_ref

SHAPES = [(1, 1), (3, 2), (2, 3), (5, 9), (4, 1000), (2, 8192)]
VARIANTS = {"plain": (1.0, 1e-5), "eps_dominates": (1e-4, 1e-5), "default_eps": (1.0, None)}
GATE = 1e-9


def _autograd(x, gy, gamma, eps, a, b):
    """d( <a, gx> + <b, ggamma> ) / d(x, gy, gamma) by autograd; an output the sum does not depend on is zeros."""
    leaves = [t.clone().requires_grad_(True) for t in (x, gy)]
    x, gy = leaves
    if gamma is not None:
        gamma = gamma.clone().requires_grad_(True)
        leaves.append(gamma)
    y = F.rms_norm(x, (x.shape[1],), gamma, eps)
    firsts = torch.autograd.grad(y, [x] + ([gamma] if gamma is not None else []), gy, create_graph=True)
    gx, ggamma = firsts[0], (firsts[1] if gamma is not None else None)
    phi = sum((u * v).sum() for u, v in ((a, gx), (b, ggamma)) if u is not None)
    if not torch.is_tensor(phi) or not phi.requires_grad:
        return [torch.zeros_like(t) for t in leaves], gx.detach(), (None if ggamma is None else ggamma.detach())
    grads = torch.autograd.grad(phi, leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)], gx.detach(), (None if ggamma is None else ggamma.detach())


def combos():
    """(a present, gamma present, b present); b exists only with gamma."""
    return [c for c in itertools.product([True, False], repeat=3) if c[1] or not c[2]]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("M,D", SHAPES, ids=lambda v: str(v))
def test_restatement_matches_autograds_double_backward_fp64(M, D, variant):
    scale_x, eps = VARIANTS[variant]
    g = torch.Generator().manual_seed(100 * M + D)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a, gamma, b = scale_x * rnd(M, D), rnd(M, D), rnd(M, D), rnd(D), rnd(D)
    rstd = rmsnorm_ref.stats(x, eps)
    worst = 0.0
    for ha, hg, hb in combos():
        aa, gm, bb = (a if ha else None), (gamma if hg else None), (b if hb else None)
        want, gx, ggamma = _autograd(x, gy, gm, eps, aa, bb)
        fx, fg = rmsnorm_ref.rmsnorm_first_backward(x, gy, gm, rstd)
        # (a one-element row: gx = r g (1 - xh^2) is a difference of nearly equal terms too — held to the terms, 2 |r g|)
        first_scale = float(gx.abs().max()) if D > 1 else 2.0 * float((rstd[:, None] * gy * (1.0 if gm is None else gm)).abs().max())
        assert float((fx - gx).abs().max()) <= GATE * first_scale
        assert (fg is None) == (gm is None)
        if gm is not None:
            assert float((fg - ggamma).abs().max()) <= GATE * float(ggamma.abs().max())
        got = rmsnorm_ref.rmsnorm_backward_vjp(x, gy, aa, gm, rstd, bb)
        assert (got[2] is None) == (gm is None)
        sdx, sdgy = rmsnorm_ref.elementwise_abs_terms(x, gy, aa, gm, rstd, bb)
        sdg = rmsnorm_ref.dgamma_abs_terms(x, gy, aa, rstd)
        for name, u, v, terms in zip(("dx", "dgy", "dgamma"), got, want, (sdx, sdgy, sdg)):
            scale = float(v.abs().max()) if D > 1 else float(terms.max())
            err = float((u - v).abs().max())
            assert err <= GATE * scale, (name, M, D, variant, (ha, hg, hb), err, scale)
            if scale > 0:
                worst = max(worst, err / scale)
    print(f"rmsnorm_ref vs autograd's double backward, {M} x {D} {variant}: worst max|diff| / scale = {worst:.2e}")


def test_the_eps_dominated_input_is_far_from_unit_mean_square():
    """mean xh^2 = 1 - eps r^2 must not be taken for 1: about 6e-4 ... 1e-3 here."""
    x = 1e-4 * torch.randn(5, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    r = rmsnorm_ref.stats(x, 1e-5)
    ms = ((x * r[:, None]) ** 2).mean(dim=1)
    assert bool((ms < 5e-3).all()) and bool((ms > 0).all())
    torch.testing.assert_close(ms, 1.0 - 1e-5 * r * r, rtol=1e-9, atol=1e-12)


def test_statistic_is_the_one_the_forward_saves():
    x = torch.randn(3, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    for eps in (1e-5, None):
        _, rstd = torch.ops.aten._fused_rms_norm(x, [6], None, eps)
        torch.testing.assert_close(rmsnorm_ref.stats(x, eps), rstd.reshape(-1), rtol=1e-12, atol=1e-12)
    assert float(rmsnorm_ref.stats(torch.zeros(1, 4, dtype=torch.float64))[0]) == float(torch.finfo(torch.float64).eps) ** -0.5


def test_absent_cotangents_are_zeros_and_the_terms_add_up():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a, gamma, b = rnd(5, 6), rnd(5, 6), rnd(5, 6), rnd(6), rnd(6)
    rstd = rmsnorm_ref.stats(x, 1e-5)
    full = rmsnorm_ref.rmsnorm_backward_vjp(x, gy, a, gamma, rstd, b)
    parts = [rmsnorm_ref.rmsnorm_backward_vjp(x, gy, a, gamma, rstd, None), rmsnorm_ref.rmsnorm_backward_vjp(x, gy, None, gamma, rstd, b)]
    for i in range(3):
        torch.testing.assert_close(parts[0][i] + parts[1][i], full[i], rtol=1e-12, atol=1e-12)
    assert not parts[1][2].any()                                            # dgamma needs a
    assert rmsnorm_ref.rmsnorm_backward_vjp(x, gy, a, None, rstd, None)[2] is None
    sdx, sdgy = rmsnorm_ref.elementwise_abs_terms(x, gy, a, gamma, rstd, b)
    assert bool((sdx >= full[0].abs() - 1e-12).all()) and bool((sdgy >= full[1].abs() - 1e-12).all())
    assert bool((rmsnorm_ref.dgamma_abs_terms(x, gy, a, rstd) >= full[2].abs() - 1e-12).all())

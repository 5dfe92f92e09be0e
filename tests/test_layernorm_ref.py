"""tests/layernorm_ref.py — the float64 restatement the layer-norm kernels (csrc/bhg_layernorm.hip) are held to — against autograd's own
double backward of F.layer_norm in float64: six shapes (one element, one row, one column, two normalised dimensions, an odd width) x
{affine, elementwise_affine=False, bias=False} x {all cotangents, each existing one absent}.
Gate: max|got - want| <= 1e-10 max|want| per array (the depthwise restatement's own gate); the test prints the worst ratio."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import layernorm_ref

# (input shape, normalized_shape)
SHAPES = [((1, 1), (1,)), ((1, 5), (5,)), ((3, 1), (1,)), ((5, 12), (12,)), ((2, 3, 8), (3, 8)), ((7, 33), (33,))]
AFFINE = ["affine", "no_affine", "no_bias"]
GATE = 1e-10
EPS = 1e-5


def _autograd(x, gy, gamma, beta, ns, a, b, c):
    """d( <a, gx> + <b, ggamma> + <c, gbeta> ) / d(x, gy, gamma) by autograd; an output the sum does not depend on is zeros."""
    leaves = [t.clone().requires_grad_(True) for t in (x, gy)]
    x, gy = leaves
    if gamma is not None:
        gamma = gamma.clone().requires_grad_(True)
        leaves.append(gamma)
    if beta is not None:
        beta = beta.clone().requires_grad_(True)
    y = F.layer_norm(x, ns, gamma, beta, EPS)
    firsts = torch.autograd.grad(y, [x] + [t for t in (gamma, beta) if t is not None], gy, create_graph=True)
    gx, ggamma, gbeta = firsts[0], (firsts[1] if gamma is not None else None), (firsts[2] if beta is not None else None)
    phi = sum((u * v).sum() for u, v in ((a, gx), (b, ggamma), (c, gbeta)) if u is not None)
    if not torch.is_tensor(phi) or not phi.requires_grad:   # no cotangent at all, or one that reaches no leaf (D = 1: gx is zero)
        return [torch.zeros_like(t) for t in leaves]
    grads = torch.autograd.grad(phi, leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]


def cotangent_sets(affine):
    """Which of (a, b, c) exist for the layer, and then: all of them, and each one absent."""
    exist = {"affine": "abc", "no_bias": "ab", "no_affine": "a"}[affine]
    return [exist] + [exist.replace(ch, "") for ch in exist]


@pytest.mark.parametrize("affine", AFFINE)
@pytest.mark.parametrize("shape,ns", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_matches_autograds_double_backward_fp64(shape, ns, affine):
    D = 1
    for v in ns:
        D *= v
    M = 1
    for v in shape:
        M *= v
    M //= D
    g = torch.Generator().manual_seed(1000 * M + D)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a = rnd(*shape), rnd(*shape), rnd(*shape)
    gamma, beta, b, c = rnd(*ns), rnd(*ns), rnd(*ns), rnd(*ns)
    if affine == "no_affine":
        gamma = beta = None
    if affine == "no_bias":
        beta = None
    worst = 0.0
    for present in cotangent_sets(affine):
        aa, bb, cc = (a if "a" in present else None), (b if "b" in present else None), (c if "c" in present else None)
        want = _autograd(x, gy, gamma, beta, ns, aa, bb, cc)
        x2 = x.reshape(M, D)
        mean, rstd = layernorm_ref.stats(x2, EPS)
        flat = lambda t: None if t is None else t.reshape(-1)   # noqa: E731
        got = layernorm_ref.layernorm_backward_vjp(x2, gy.reshape(M, D), None if aa is None else aa.reshape(M, D), flat(gamma), mean, rstd,
                                                   flat(bb), flat(cc))
        assert (got[2] is None) == (gamma is None)
        for name, u, v in zip(("dx", "dgy", "dgamma"), got, want):
            scale = float(v.abs().max())
            err = float((u.reshape(v.shape) - v).abs().max())
            assert err <= GATE * scale, (name, shape, affine, present, err, scale)
            if scale > 0:
                worst = max(worst, err / scale)
    print(f"layernorm_ref vs autograd's double backward, {shape} {affine}: worst max|diff| / max|want| = {worst:.2e}")


def test_absent_cotangents_are_zeros_and_the_terms_add_up():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a, gamma, b, c = rnd(5, 12), rnd(5, 12), rnd(5, 12), rnd(12), rnd(12), rnd(12)
    mean, rstd = layernorm_ref.stats(x, EPS)
    full = layernorm_ref.layernorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c)
    parts = [layernorm_ref.layernorm_backward_vjp(x, gy, *args) for args in
             ((a, gamma, mean, rstd, None, None), (None, gamma, mean, rstd, b, None), (None, gamma, mean, rstd, None, c))]
    for i in range(3):
        torch.testing.assert_close(sum(p[i] for p in parts), full[i], rtol=1e-12, atol=1e-12)
    assert not parts[1][2].any() and not parts[2][2].any() and not parts[2][0].any()   # dgamma needs a; c reaches dgy alone
    assert layernorm_ref.layernorm_backward_vjp(x, gy, a, None, mean, rstd, None, None)[2] is None
    terms = layernorm_ref.dgamma_abs_terms(x, gy, a, gamma, mean, rstd)
    assert bool((terms >= full[2].abs() - 1e-12).all())


@pytest.mark.parametrize("combo", list(itertools.product([False, True], repeat=3)), ids=str)
def test_every_combination_of_absent_cotangents_runs(combo):
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a, gamma, b, c = rnd(3, 4), rnd(3, 4), rnd(3, 4), rnd(4), rnd(4), rnd(4)
    mean, rstd = layernorm_ref.stats(x, EPS)
    out = layernorm_ref.layernorm_backward_vjp(x, gy, a if combo[0] else None, gamma, mean, rstd, b if combo[1] else None, c if combo[2] else None)
    assert all(bool(torch.isfinite(t).all()) for t in out)

"""tests/groupnorm_ref.py — the float64 restatement the group-norm kernels (csrc/bhg_groupnorm.hip) are held to — against autograd's own
double backward of F.group_norm in float64: nine shapes ([N, C] inputs, G = 1, G = C, rows of 2, 3, 9, 12 and 16 elements, 1 x 32 x 7 x 7
with G = 8) x {affine, affine=False} x {all cotangents, each existing one absent}.
Gate: max|got - want| <= 1e-10 max|want| per array where a row has at least 4 elements (observed 4e-12); 1e-8 for shorter rows, which are
ill-conditioned — rstd is large — (observed 1.8e-10).  The test prints the worst ratio."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref

# (input shape, G)
SHAPES = [((3, 4), 2), ((2, 6), 2), ((5, 3), 1), ((2, 6, 3), 2), ((2, 4, 6), 2), ((2, 8, 2, 2), 2), ((3, 6, 4, 4), 1), ((3, 5, 7), 5),
          ((1, 32, 7, 7), 8)]
AFFINE = ["affine", "no_affine"]
GATE, GATE_SHORT = 1e-10, 1e-8
EPS = 1e-5


def row_length(shape, G):
    n = 1
    for v in shape[1:]:
        n *= v
    return n // G


def test_the_shapes_are_the_ones_named():
    assert sorted({row_length(s, g) for s, g in SHAPES} & {2, 3, 9, 12, 16}) == [2, 3, 9, 12, 16]
    assert any(len(s) == 2 for s, _ in SHAPES) and any(g == 1 for _, g in SHAPES) and any(g == s[1] and g > 1 for s, g in SHAPES)
    assert ((1, 32, 7, 7), 8) in SHAPES and len(SHAPES) == 9


def _autograd(x, gy, gamma, beta, G, a, b, c):
    """d( <a, gx> + <b, ggamma> + <c, gbeta> ) / d(x, gy, gamma) by autograd; an output the sum does not depend on is zeros."""
    leaves = [t.clone().requires_grad_(True) for t in (x, gy)]
    x, gy = leaves
    if gamma is not None:
        gamma = gamma.clone().requires_grad_(True)
        beta = beta.clone().requires_grad_(True)
        leaves.append(gamma)
    y = F.group_norm(x, G, gamma, beta, EPS)
    firsts = torch.autograd.grad(y, [x] + ([gamma, beta] if gamma is not None else []), gy, create_graph=True)
    gx, ggamma, gbeta = firsts[0], (firsts[1] if gamma is not None else None), (firsts[2] if gamma is not None else None)
    phi = sum((u * v).sum() for u, v in ((a, gx), (b, ggamma), (c, gbeta)) if u is not None)
    if not torch.is_tensor(phi) or not phi.requires_grad:   # no cotangent at all, or one that reaches no leaf
        return [torch.zeros_like(t) for t in leaves]
    grads = torch.autograd.grad(phi, leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]


def cotangent_sets(affine):
    """Which of (a, b, c) exist for the layer, and then: all of them, and each one absent."""
    exist = {"affine": "abc", "no_affine": "a"}[affine]
    return [exist] + [exist.replace(ch, "") for ch in exist]


@pytest.mark.parametrize("affine", AFFINE)
@pytest.mark.parametrize("shape,G", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"G{v}")
def test_restatement_matches_autograds_double_backward_fp64(shape, G, affine):
    C = shape[1]
    g = torch.Generator().manual_seed(1000 * shape[0] + 10 * C + G)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a = rnd(*shape), rnd(*shape), rnd(*shape)
    gamma, beta, b, c = rnd(C), rnd(C), rnd(C), rnd(C)
    if affine == "no_affine":
        gamma = beta = None
    gate = GATE if row_length(shape, G) >= 4 else GATE_SHORT
    mean, rstd = groupnorm_ref.stats(x, G, EPS)
    worst = 0.0
    for present in cotangent_sets(affine):
        aa, bb, cc = (a if "a" in present else None), (b if "b" in present else None), (c if "c" in present else None)
        want = _autograd(x, gy, gamma, beta, G, aa, bb, cc)
        got = groupnorm_ref.groupnorm_backward_vjp(x, gy, aa, gamma, mean, rstd, bb, cc, G)
        assert (got[2] is None) == (gamma is None)
        for name, u, v in zip(("dx", "dgy", "dgamma"), got, want):
            scale = float(v.abs().max())
            err = float((u - v).abs().max())
            assert err <= gate * scale, (name, shape, G, affine, present, err, scale)
            if scale > 0:
                worst = max(worst, err / scale)
    print(f"groupnorm_ref vs autograd's double backward, {shape} G={G} {affine}: worst max|diff| / max|want| = {worst:.2e}")


def test_statistics_are_the_ones_native_group_norm_saves():
    x = torch.randn(3, 6, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    _, mean, rstd = torch.native_group_norm(x, None, None, 3, 6, 5, 2, EPS)
    m, r = groupnorm_ref.stats(x, 2, EPS)
    torch.testing.assert_close(m, mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r, rstd, rtol=1e-12, atol=1e-12)


def test_absent_cotangents_are_zeros_and_the_terms_add_up():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a, gamma, b, c = rnd(5, 6, 4), rnd(5, 6, 4), rnd(5, 6, 4), rnd(6), rnd(6), rnd(6)
    mean, rstd = groupnorm_ref.stats(x, 3, EPS)
    full = groupnorm_ref.groupnorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c, 3)
    parts = [groupnorm_ref.groupnorm_backward_vjp(x, gy, *args, 3) for args in
             ((a, gamma, mean, rstd, None, None), (None, gamma, mean, rstd, b, None), (None, gamma, mean, rstd, None, c))]
    for i in range(3):
        torch.testing.assert_close(sum(p[i] for p in parts), full[i], rtol=1e-12, atol=1e-12)
    assert not parts[1][2].any() and not parts[2][2].any() and not parts[2][0].any()   # dgamma needs a; c reaches dgy alone
    assert groupnorm_ref.groupnorm_backward_vjp(x, gy, a, None, mean, rstd, None, None, 3)[2] is None
    terms = groupnorm_ref.dgamma_abs_terms(x, gy, a, mean, rstd, 3)
    assert bool((terms >= full[2].abs() - 1e-12).all())


@pytest.mark.parametrize("combo", list(itertools.product([False, True], repeat=3)), ids=str)
def test_every_combination_of_absent_cotangents_runs(combo):
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, gy, a, gamma, b, c = rnd(3, 4, 2), rnd(3, 4, 2), rnd(3, 4, 2), rnd(4), rnd(4), rnd(4)
    mean, rstd = groupnorm_ref.stats(x, 2, EPS)
    out = groupnorm_ref.groupnorm_backward_vjp(x, gy, a if combo[0] else None, gamma, mean, rstd, b if combo[1] else None, c if combo[2] else None, 2)
    assert all(bool(torch.isfinite(t).all()) for t in out)

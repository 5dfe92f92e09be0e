"""tests/softreg_ref.py (the fp64 restatement the native softmax-regression solvers are held to) against (a) a float64 autograd double
backward of the loss it restates and (b) the reference's own fp64 results on the seeded instance of tests/softreg_zoo.py (the `fp64`
arrays of tests/golden/softreg.npz, produced by the real reference in float64).

Bound: both sides are float64 (eps = 1.1e-16) and differ in summation order only; a product sums at most n + d < 100 terms and at most
five iterations follow one another on a Hessian whose condition number is below 10 (lam in (0.2, 1.4), the data term is positive
semi-definite with norm <= 0.5 (1 + sqrt(d / n))^2): the two agree to ~1e-13 of the largest entry.  The gate is 1e-10 of the largest
entry, the gate of tests/test_logreg_solve_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import softreg_ref as ref
import softreg_zoo
from conftest import golden_list, load_golden

RTOL = 1e-10
SHAPES = [(5, 3, 2), (17, 5, 3), (33, 9, 16)]


def _instance(n, d, C):
    g = torch.Generator().manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    W = 0.3 * torch.randn(C, d, generator=g, dtype=torch.float64)
    lam = 0.5 + torch.rand(C, d, generator=g, dtype=torch.float64)
    V = torch.randn(C, d, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (n,), generator=g)
    return X, W, lam, V, y


@pytest.mark.parametrize("n,d,C", SHAPES)
def test_hessian_product_and_lam_cotangent_match_autograd(n, d, C):
    X, W, lam, V, y = _instance(n, d, C)
    W, lam = W.requires_grad_(), lam.requires_grad_()
    loss = F.cross_entropy(X @ W.t(), y) + 0.5 * (lam * W * W).sum()
    (g,) = torch.autograd.grad(loss, W, create_graph=True)
    hv, mixed = torch.autograd.grad((g * V).sum(), [W, lam])
    Xn, Wn, lamn, Vn = (t.detach().numpy() for t in (X, W, lam, V))
    P = ref.softmax_rows(Xn @ Wn.T)
    assert np.allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    got_hv = ref.hessian_product(Xn, P, lamn, Vn)
    got_mixed = -ref.lam_cotangent(Wn, Vn)   # lam_cotangent is the cotangent of g . (-solution)
    for name, got, want in (("hessian_product", got_hv, hv.numpy()), ("lam_cotangent", got_mixed, mixed.numpy())):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"({n}, {d}, {C}) {name}: max|restated - autograd| = {err:.3e} = {err / scale:.3e} of max|autograd|")
        assert got.shape == want.shape and err <= RTOL * scale


def test_softmax_rows_survives_saturated_logits():
    P = ref.softmax_rows(np.array([[900.0, -900.0, 0.0], [-1e4, -1e4, -1e4]]))
    assert np.isfinite(P).all() and np.allclose(P[0], [1.0, 0.0, 0.0]) and np.allclose(P[1], 1.0 / 3.0)


def restated(case, inputs):
    X, W, theta, v = (inputs[k] for k in ("batch_x", "inner_0", "upper_0", "vec_0"))
    theta = theta.astype(np.float64)
    lam, dlam = np.logaddexp(0.0, theta), 1.0 / (1.0 + np.exp(-theta))   # softplus and its derivative
    if case.algo == "cg":
        sol = ref.cg(X, W, lam, v, case.cfg["cg_iterations"], case.cfg["cg_alpha"])
    elif case.algo == "neumann":
        sol = ref.neumann(X, W, lam, v, case.cfg["neumann_iterations"], case.cfg["neumann_alpha"])
    else:
        sol = v   # darts / sama with the identity preconditioner: the central difference of 1/2 lam W^2 along v is -(W v) exactly
    return ref.lam_cotangent(W, sol) * dlam


@pytest.mark.parametrize("name", [c.name for c in softreg_zoo.CASES if c.algo in ("cg", "neumann")])
def test_restatement_matches_the_reference_fp64_golden(name):
    case = softreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("softreg")
    (want,) = golden_list(outputs, name, "fp64")
    assert want.dtype == np.float64
    got = restated(case, inputs)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{name}: max|restated - golden| = {err:.3e} = {err / scale:.3e} of max|golden| = {scale:.3e}")
    assert got.shape == want.shape and err <= RTOL * scale


@pytest.mark.parametrize("name", ["softreg_darts", "softreg_sama"])
def test_closed_form_finite_difference_matches_the_reference_fp64_golden(name):
    """The reference's fp64 central difference carries the rounding of w +- eps v divided by 2 eps (eps ~ 0.1 here): ~1e-14."""
    case = softreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("softreg")
    (want,) = golden_list(outputs, name, "fp64")
    got = restated(case, inputs)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{name}: max|closed form - golden| = {err:.3e} = {err / scale:.3e} of max|golden|")
    assert err <= RTOL * scale


def test_the_cg_alpha_quirk_is_in_the_restatement():
    inputs, outputs = load_golden("softreg")
    X, W, theta, v = (inputs[k] for k in ("batch_x", "inner_0", "upper_0", "vec_0"))
    lam = np.logaddexp(0.0, theta.astype(np.float64))
    quirk, textbook = ref.cg(X, W, lam, v, 5, 0.1), 0.1 * ref.cg(X, W, lam, v, 5, 1.0)
    assert np.abs(quirk - textbook).max() > 0.1 * np.abs(quirk).max()


def test_inputs_are_not_modified_and_the_result_has_the_shape_of_rhs():
    inputs, _ = load_golden("softreg")
    arrays = [np.array(inputs[k]) for k in ("batch_x", "inner_0", "upper_0", "vec_0")]
    arrays[2] = np.abs(arrays[2]) + 0.5
    before = [a.copy() for a in arrays]
    assert ref.cg(*arrays, 3, 0.1).shape == arrays[3].shape
    X, W, lam, v = arrays
    assert ref.neumann(X, W, lam, v.reshape(-1), 3, 0.25).shape == (v.size,)
    assert all(np.array_equal(a, b) for a, b in zip(arrays, before))

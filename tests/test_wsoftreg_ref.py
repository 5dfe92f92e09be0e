"""tests/wsoftreg_ref.py (the fp64 restatement the row-weighted native solves and the mixed pass are held to) against (a) a float64
autograd double backward of the loss it restates and (b) the reference's own fp64 results on the seeded instance of
tests/wsoftreg_zoo.py (the `fp64` arrays of tests/golden/wsoftreg.npz, produced by the real reference in float64).

Bound: both sides are float64 (eps = 1.1e-16) and differ in summation order only; a product sums at most n + d < 100 terms and at most
five iterations follow one another on a Hessian whose condition number is below 10 (reg in [0.5, 1.5), the data term is positive
semi-definite with norm <= 0.5 max(a) (1 + sqrt(d / n))^2 and a < 2.5): the two agree to ~1e-13 of the largest entry.  The gate is
1e-10 of the largest entry, the gate of tests/test_softreg_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wsoftreg_ref as ref
import wsoftreg_zoo
from conftest import golden_list, load_golden
from softreg_ref import softmax_rows

RTOL = 1e-10
SHAPES = [(5, 3, 2), (17, 5, 3), (33, 9, 16), (37, 9, 5)]


def _instance(n, d, C):
    g = torch.Generator().manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    W = 0.3 * torch.randn(C, d, generator=g, dtype=torch.float64)
    reg = 0.5 + torch.rand(C, d, generator=g, dtype=torch.float64)
    theta = torch.randn(n, generator=g, dtype=torch.float64)
    V = torch.randn(C, d, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (n,), generator=g)
    return X, W, reg, theta, V, y


@pytest.mark.parametrize("n,d,C", SHAPES)
def test_hessian_product_and_weight_cotangent_match_autograd(n, d, C):
    X, W, reg, theta, V, y = _instance(n, d, C)
    W, theta = W.requires_grad_(), theta.requires_grad_()
    a = torch.sigmoid(theta)
    loss = (a * F.cross_entropy(X @ W.t(), y, reduction="none")).mean() + 0.5 * (reg * W * W).sum()
    (g,) = torch.autograd.grad(loss, W, create_graph=True)
    hv, mixed = torch.autograd.grad((g * V).sum(), [W, theta])
    Xn, Wn, regn, Vn, an = (t.detach().numpy() for t in (X, W, reg, V, a))
    got_hv = ref.hessian_product(Xn, softmax_rows(Xn @ Wn.T), regn, an, Vn)
    got_mixed = ref.weight_cotangent(Xn, Wn, y.numpy(), Vn) * an * (1.0 - an)   # c through a = sigmoid(theta)
    for name, got, want in (("hessian_product", got_hv, hv.numpy()), ("weight_cotangent", got_mixed, mixed.numpy())):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"({n}, {d}, {C}) {name}: max|restated - autograd| = {err:.3e} = {err / scale:.3e} of max|autograd|")
        assert got.shape == want.shape and err <= RTOL * scale


def test_unit_weights_are_the_unweighted_problem():
    import softreg_ref

    X, W, reg, _, V, _ = (t.numpy() for t in _instance(17, 5, 3))
    ones = np.ones(17)
    assert np.array_equal(ref.cg(X, W, reg, ones, V, 4, 0.1), softreg_ref.cg(X, W, reg, V, 4, 0.1))
    assert np.array_equal(ref.neumann(X, W, reg, ones, V, 4, 0.25), softreg_ref.neumann(X, W, reg, V, 4, 0.25))


def restated(case, inputs):
    X, y, W, theta, reg, v = (inputs[k] for k in ("batch_x", "batch_y", "inner_0", "upper_0", "reg", "vec_0"))
    a = 1.0 / (1.0 + np.exp(-theta.astype(np.float64)))
    if case.algo == "cg":
        sol = ref.cg(X, W, reg, a, v, case.cfg["cg_iterations"], case.cfg["cg_alpha"])
    else:
        sol = ref.neumann(X, W, reg, a, v, case.cfg["neumann_iterations"], case.cfg["neumann_alpha"])
    return ref.weight_cotangent(X, W, y, -sol) * a * (1.0 - a)


@pytest.mark.parametrize("name", [c.name for c in wsoftreg_zoo.CASES if c.algo in ("cg", "neumann")])
def test_restatement_matches_the_reference_fp64_golden(name):
    case = wsoftreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("wsoftreg")
    (want,) = golden_list(outputs, name, "fp64")
    assert want.dtype == np.float64
    got = restated(case, inputs)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{name}: max|restated - golden| = {err:.3e} = {err / scale:.3e} of max|golden| = {scale:.3e}")
    assert got.shape == want.shape and err <= RTOL * scale


def test_the_cg_alpha_quirk_is_in_the_restatement():
    inputs, _ = load_golden("wsoftreg")
    X, W, theta, reg, v = (inputs[k] for k in ("batch_x", "inner_0", "upper_0", "reg", "vec_0"))
    a = 1.0 / (1.0 + np.exp(-theta.astype(np.float64)))
    quirk, textbook = ref.cg(X, W, reg, a, v, 5, 0.1), 0.1 * ref.cg(X, W, reg, a, v, 5, 1.0)
    assert np.abs(quirk - textbook).max() > 0.1 * np.abs(quirk).max()


def test_inputs_are_not_modified_and_the_result_has_the_shape_of_rhs():
    inputs, _ = load_golden("wsoftreg")
    arrays = [np.array(inputs[k]) for k in ("batch_x", "inner_0", "reg", "upper_0", "vec_0")]
    arrays[3] = np.abs(arrays[3])
    y = np.array(inputs["batch_y"])
    before = [a.copy() for a in arrays] + [y.copy()]
    assert ref.cg(*arrays, 3, 0.1).shape == arrays[4].shape
    X, W, reg, a, v = arrays
    assert ref.neumann(X, W, reg, a, v.reshape(-1), 3, 0.25).shape == (v.size,)
    assert ref.weight_cotangent(X, W, y, v.reshape(-1)).shape == (X.shape[0],)
    assert all(np.array_equal(p, q) for p, q in zip(arrays + [y], before))

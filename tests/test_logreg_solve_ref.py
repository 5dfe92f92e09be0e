"""tests/logreg_solve_ref.py (the fp64 restatement the native logistic-regression solvers are held to) against the reference's own
fp64 results on the cfg-1 problem: the `fp64` arrays of tests/golden/logreg.npz, produced by the real reference in float64.

Bound: both sides are float64 (eps = 1.1e-16) and differ in summation order only.  A product sums n + d = 600 terms
(<= 600 eps = 7e-14 relative to the sum of magnitudes), at most five iterations follow one another, and H = X^T S X + diag(lam) with
lam = 1 has a condition number below 4 (the data term is positive semi-definite with norm <= 0.25 (1 + sqrt(d / n))^2 < 0.6): the
two results agree to ~1e-12 of the largest entry.  The gate is 1e-10 of the largest entry; K = 0 is exact up to the one product
alpha * v."""
import numpy as np
import pytest

import logreg_solve_ref as ref
import zoo
from conftest import golden_list, load_golden

CASES = ["logreg_cg5", "logreg_cg3_a01", "logreg_cg0", "logreg_neumann5", "logreg_neumann0"]
RTOL = 1e-10


def restated(case, inputs):
    X, w, lam, v = (inputs[k] for k in ("batch_x", "inner_0", "upper_0", "vec_0"))
    if case.algo == "cg":
        sol = ref.cg(X, w, lam, v, case.cfg["cg_iterations"], case.cfg["cg_alpha"])
    else:
        sol = ref.neumann(X, w, lam, v, case.cfg["neumann_iterations"], case.cfg["neumann_alpha"])
    return ref.lam_cotangent(w, sol)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_fp64_golden(name):
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("logreg")
    (want,) = golden_list(outputs, name, "fp64")
    assert want.dtype == np.float64
    got = restated(case, inputs)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{name}: max|restated - golden| = {err:.3e} = {err / scale if scale else 0.0:.3e} of max|golden| = {scale:.3e}")
    assert got.shape == want.shape and err <= RTOL * scale


def test_the_cg_alpha_quirk_is_in_the_restatement():
    """With cg_alpha = 0.1 the reference's answer is NOT 0.1 x the textbook CG answer: the step length is 10 x too long for the
    residual it is applied to.  A restatement without the quirk would match `logreg_cg3_a01` no better than ~1 (relative)."""
    inputs, outputs = load_golden("logreg")
    X, w, lam, v = (inputs[k] for k in ("batch_x", "inner_0", "upper_0", "vec_0"))
    (want,) = golden_list(outputs, "logreg_cg3_a01", "fp64")
    textbook = ref.lam_cotangent(w, 0.1 * ref.cg(X, w, lam, v, 3, 1.0))
    assert np.abs(textbook - want).max() > 0.1 * np.abs(want).max()


def test_inputs_are_not_modified():
    inputs, _ = load_golden("logreg")
    arrays = [np.array(inputs[k]) for k in ("batch_x", "inner_0", "upper_0", "vec_0")]
    before = [a.copy() for a in arrays]
    ref.cg(*arrays, 3, 0.1)
    ref.neumann(*arrays, 3, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(arrays, before))

"""fp64 restatement of the reference's cg / neumann on L2-regularised logistic regression — TEST INFRASTRUCTURE, numpy, no GPU.

Inner loss  L(w, lam) = mean_i BCE(x_i . w, y_i) + 1/2 sum_j lam_j w_j^2  (SURVEY Appendix A.1), so the Hessian in w is

    H = X^T diag(s) X + diag(lam),   s_i = sigma_i (1 - sigma_i) / n,   sigma_i = 1 / (1 + exp(-x_i . w))

(the labels drop out), and the mixed derivative of g . u with respect to lam is w * u.  The two solvers below are what the
reference's hypergradient/cg.py:34-56 and hypergradient/neumann.py:59-66 compute when the double backward is replaced by this H:
same iteration, same quirk (the step length of CG divides by dot(cg_alpha * Hp, p), the residual moves along the UN-scaled Hp), no
convergence test, no breakdown guard.  Everything is float64 whatever comes in; the inputs are never modified.
"""
import numpy as np


def curvature(X, w):
    """s_i = sigma_i (1 - sigma_i) / n, from sigma (1 - sigma) = e / (1 + e)^2 with e = exp(-|z|): no overflow for any z."""
    X, w = np.asarray(X, np.float64), np.asarray(w, np.float64)
    e = np.exp(-np.abs(X @ w))
    return e / ((1.0 + e) * (1.0 + e)) / X.shape[0]


def hessian_product(X, s, lam, p):
    """H p = X^T (s * (X p)) + lam * p."""
    return X.T @ (s * (X @ p)) + lam * p


def cg(X, w, lam, rhs, K, cg_alpha):
    """cg_alpha * x_K of K CG iterations from x = 0, r = p = rhs (cg.py:34-56)."""
    X, lam, rhs = np.asarray(X, np.float64), np.asarray(lam, np.float64), np.asarray(rhs, np.float64)
    s = curvature(X, w)
    x, r, p = np.zeros_like(rhs), rhs.copy(), rhs.copy()
    for _ in range(int(K)):
        hp = hessian_product(X, s, lam, p)
        num = r @ r
        step = num / ((cg_alpha * hp) @ p)     # the quirk: the scaled product in the denominator ...
        x = x + step * p
        r_new = r - step * hp                  # ... the un-scaled one in the residual
        p = r_new + ((r_new @ r_new) / num) * p
        r = r_new
    return cg_alpha * x


def neumann(X, w, lam, rhs, K, alpha):
    """alpha * p_K of K iterations v <- v - alpha H v, p <- p + v from v = p = rhs (neumann.py:59-66)."""
    X, lam, rhs = np.asarray(X, np.float64), np.asarray(lam, np.float64), np.asarray(rhs, np.float64)
    s = curvature(X, w)
    v, p = rhs.copy(), rhs.copy()
    for _ in range(int(K)):
        v = v - alpha * hessian_product(X, s, lam, v)
        p = p + v
    return alpha * p


def lam_cotangent(w, solution):
    """The final hop: d(g . (-solution)) / d lam = w * (-solution), the hypergradient with respect to the lam tensor."""
    return np.asarray(w, np.float64) * (-np.asarray(solution, np.float64))


SOLVERS = {"cg": cg, "neumann": neumann}

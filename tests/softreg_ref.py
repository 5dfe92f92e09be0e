"""fp64 restatement of the reference's cg / neumann on softmax regression with a per-weight L2 penalty — TEST INFRASTRUCTURE, numpy,
no GPU.  The multi-class sibling of tests/logreg_solve_ref.py.

Inner loss  L(W, lam) = mean_i CE(x_i W^T, y_i) + 1/2 sum lam * W^2  with W, lam of shape [C, d], so with P = softmax(X W^T)

    H V = U^T X + lam * V,   Z = X V^T,   U = (P * Z - P * rowsum(P * Z)) / n

(the labels drop out), and the mixed derivative of g . u with respect to lam is W * u.  The two solvers are what the reference's
hypergradient/cg.py:34-56 and hypergradient/neumann.py:59-66 compute when the double backward is replaced by this H: same iteration,
same quirk (the step length of CG divides by dot(cg_alpha * Hp, p), the residual moves along the UN-scaled Hp), no convergence test, no
breakdown guard.  Vectors (rhs, the solution) have W's shape or are flat in W's row-major order; the result has rhs's shape.
Everything is float64 whatever comes in; the inputs are never modified.
"""
import numpy as np


def softmax_rows(logits):
    """Row-wise softmax with the row maximum subtracted: no overflow for any logits."""
    logits = np.asarray(logits, np.float64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def hessian_product(X, P, lam, V):
    """H V = U^T X + lam * V for V of shape [C, d]."""
    Z = X @ V.T
    PZ = P * Z
    U = (PZ - P * PZ.sum(axis=1, keepdims=True)) / X.shape[0]
    return U.T @ X + lam * V


def _setup(X, W, lam, rhs):
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    lam = np.broadcast_to(np.asarray(lam, np.float64), W.shape)
    rhs = np.asarray(rhs, np.float64)
    return X, softmax_rows(X @ W.T), lam, rhs.reshape(W.shape).copy(), rhs.shape


def cg(X, W, lam, rhs, K, cg_alpha):
    """cg_alpha * x_K of K CG iterations from x = 0, r = p = rhs (cg.py:34-56)."""
    X, P, lam, r, shape = _setup(X, W, lam, rhs)
    x, p = np.zeros_like(r), r.copy()
    for _ in range(int(K)):
        hp = hessian_product(X, P, lam, p)
        num = (r * r).sum()
        step = num / ((cg_alpha * hp) * p).sum()     # the quirk: the scaled product in the denominator ...
        x = x + step * p
        r_new = r - step * hp                        # ... the un-scaled one in the residual
        p = r_new + ((r_new * r_new).sum() / num) * p
        r = r_new
    return (cg_alpha * x).reshape(shape)


def neumann(X, W, lam, rhs, K, alpha):
    """alpha * p_K of K iterations v <- v - alpha H v, p <- p + v from v = p = rhs (neumann.py:59-66)."""
    X, P, lam, v, shape = _setup(X, W, lam, rhs)
    p = v.copy()
    for _ in range(int(K)):
        v = v - alpha * hessian_product(X, P, lam, v)
        p = p + v
    return (alpha * p).reshape(shape)


def lam_cotangent(W, solution):
    """The final hop: d(g . (-solution)) / d lam = W * (-solution), the hypergradient with respect to the lam tensor."""
    W = np.asarray(W, np.float64)
    return (W.reshape(-1) * (-np.asarray(solution, np.float64).reshape(-1))).reshape(np.shape(solution))


SOLVERS = {"cg": cg, "neumann": neumann}

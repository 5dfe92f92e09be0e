"""fp64 restatement of the reference's cg / neumann on SAMPLE-WEIGHTED softmax regression — TEST INFRASTRUCTURE, numpy, no GPU.  The
sibling of tests/softreg_ref.py: one weight a_i per row of X (a function of the upper problem's parameters), a constant penalty.

Inner loss  L(W, theta) = (1/n) sum_i a_i CE(x_i W^T, y_i) + 1/2 sum reg * W^2  with W, reg of shape [C, d], so with
P = softmax(X W^T) and Y the one-hot labels

    H V = U^T X + reg * V,   Z = X V^T,   U_i = a_i (P_i * Z_i - P_i (P_i . Z_i)) / n          (the labels drop out)
    cotangent of a along a direction D:   c_i = sum_c (P_ic - Y_ic) (X D^T)_ic / n             (they do not)

The two solvers are what the reference's hypergradient/cg.py:34-56 and hypergradient/neumann.py:59-66 compute when the double backward
is replaced by this H: same iteration, same quirk (the step length of CG divides by dot(cg_alpha * Hp, p), the residual moves along the
UN-scaled Hp), no convergence test, no breakdown guard.  Vectors (rhs, the solution) have W's shape or are flat in W's row-major order;
the result has rhs's shape.  Everything is float64 whatever comes in; the inputs are never modified.
"""
import numpy as np

from softreg_ref import softmax_rows


def hessian_product(X, P, reg, a, V):
    """H V = U^T X + reg * V for V of shape [C, d]."""
    Z = X @ V.T
    PZ = P * Z
    U = (PZ - P * PZ.sum(axis=1, keepdims=True)) * a[:, None] / X.shape[0]
    return U.T @ X + reg * V


def _setup(X, W, reg, a, rhs):
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    reg = np.broadcast_to(np.asarray(reg, np.float64), W.shape)
    a = np.asarray(a, np.float64).reshape(-1)
    rhs = np.asarray(rhs, np.float64)
    return X, softmax_rows(X @ W.T), reg, a, rhs.reshape(W.shape).copy(), rhs.shape


def cg(X, W, reg, a, rhs, K, cg_alpha):
    """cg_alpha * x_K of K CG iterations from x = 0, r = p = rhs (cg.py:34-56)."""
    X, P, reg, a, r, shape = _setup(X, W, reg, a, rhs)
    x, p = np.zeros_like(r), r.copy()
    for _ in range(int(K)):
        hp = hessian_product(X, P, reg, a, p)
        num = (r * r).sum()
        step = num / ((cg_alpha * hp) * p).sum()     # the quirk: the scaled product in the denominator ...
        x = x + step * p
        r_new = r - step * hp                        # ... the un-scaled one in the residual
        p = r_new + ((r_new * r_new).sum() / num) * p
        r = r_new
    return (cg_alpha * x).reshape(shape)


def neumann(X, W, reg, a, rhs, K, alpha):
    """alpha * p_K of K iterations v <- v - alpha H v, p <- p + v from v = p = rhs (neumann.py:59-66)."""
    X, P, reg, a, v, shape = _setup(X, W, reg, a, rhs)
    p = v.copy()
    for _ in range(int(K)):
        v = v - alpha * hessian_product(X, P, reg, a, v)
        p = p + v
    return (alpha * p).reshape(shape)


def weight_cotangent(X, W, y, direction):
    """c [n]: d(g . direction) / d a, the mixed second derivative with respect to the sample weights along ``direction``."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    D = np.asarray(direction, np.float64).reshape(W.shape)
    PmY = softmax_rows(X @ W.T)
    PmY[np.arange(X.shape[0]), np.asarray(y).reshape(-1)] -= 1.0
    return (PmY * (X @ D.T)).sum(axis=1) / X.shape[0]


SOLVERS = {"cg": cg, "neumann": neumann}

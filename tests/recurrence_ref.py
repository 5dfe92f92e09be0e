"""One-step reference of the flat-vector recurrences (csrc/bhg_vector.hip) in numpy — TEST INFRASTRUCTURE, no GPU.

Plain functions on flat ``np.float32`` arrays restating, rounding by rounding, what k_cg_init, k_cg_dot / k_cg_resid / k_cg_dir
(and k_cg_resident, every instance) and k_neumann_step compute:

* every element-wise product and sum is a numpy operation of its own on float32 operands with a float32 scalar, so it is rounded
  to fp32 exactly where the kernels' mul_rn / add_rn / sub_rn round (numpy never contracts two operations into an fma);
* every dot product is taken on ``astype(np.float64)`` operands — an fp32 x fp32 product is exact in fp64 — and summed in index
  order, the order of oracle/recurrence.c, so that the CPU pins in tests/test_recurrence_ref.py are bit for bit.  The kernels sum the
  same exact terms in another order: a test bounds that difference with the sum of absolute terms returned here.

The inputs are never modified.
"""
import numpy as np

F32 = np.float32


def _check(*arrays):
    for a in arrays:
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 1, "flat float32 arrays only"


_BLOCK = 1 << 18   # fp64 terms formed per pass: the temporaries stay in cache at 20 M elements


def dot64(a, b):
    """(sum, sum of absolute terms) of the exact fp64 products a[i] * b[i], both summed in index order: np.add.accumulate is a
    sequential recurrence (np.sum adds pairwise), and a block's first term takes the running sum, so the blocks change nothing."""
    total = total_abs = 0.0
    square = a is b
    for i in range(0, a.size, _BLOCK):
        terms = a[i:i + _BLOCK].astype(np.float64)
        terms *= terms if square else b[i:i + _BLOCK].astype(np.float64)
        if not square:
            mags = np.abs(terms)
            mags[0] = total_abs + mags[0]
            total_abs = float(np.add.accumulate(mags, out=mags)[-1])
        terms[0] = total + terms[0]
        total = float(np.add.accumulate(terms, out=terms)[-1])
    return total, (total if square else total_abs)


def cg_init(vec):
    """cg.py:34-36 and the first numerator: x = 0, r = p = vec, rr = sum vec^2 (fp64)."""
    _check(vec)
    return np.zeros_like(vec), vec.copy(), vec.copy(), dot64(vec, vec)[0]


def shifted(h, p, shift):
    """h' = h + fl(shift * p), only when shift != 0 (the Hessian's diagonal part, kept out of the producer)."""
    if shift == 0:
        return h
    return h + F32(shift) * p


def cg_step(h, x, r, p, rr_old, cg_alpha, shift, out_scale, alpha=None, beta=None):
    """One CG iteration.  Returns (x', r', p'), (rr_old, den, alpha, rr_new, beta), (sum |fl(cg_alpha h') p|, sum r'^2).
    ``alpha=`` / ``beta=`` replace the two step lengths (fp32 values) in the element-wise updates and in the returned tuple; den and
    rr_new are still those of the vectors actually formed."""
    _check(h, x, r, p)
    # (a recurrence that has converged exactly divides 0 by 0, like the kernels: NaN is a value here, not a warning)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hs = shifted(h, p, shift)
        den, den_abs = dot64(F32(cg_alpha) * hs, p)
        a = F32(alpha) if alpha is not None else F32(rr_old) / F32(den)
        r_new = r - a * hs
        rr_new, rr_abs = dot64(r_new, r_new)
        b = F32(beta) if beta is not None else F32(rr_new) / F32(rr_old)
        x_new = x + a * p
        if out_scale != 0:
            x_new = F32(out_scale) * x_new
        p_new = r_new + b * p
    return (x_new, r_new, p_new), (float(rr_old), den, float(a), rr_new, float(b)), (den_abs, rr_abs)


def neumann_step(h, v, p, alpha, shift, out_scale):
    """k_neumann_step: v' = v - fl(alpha * h'), h' = h + fl(shift * v); p' = p + v' [then fl(out_scale * p')].  Returns (v', p')."""
    _check(h, v, p)
    hs = shifted(h, v, shift)
    v_new = v - F32(alpha) * hs
    p_new = v_new + p
    if out_scale != 0:
        p_new = F32(out_scale) * p_new
    return v_new, p_new

"""Neumann-series best-response-Jacobian product on fused gfx950 kernels.

Behavioural twin of /root/reference betty/hypergradient/neumann.py:8-66: ``p = v``; K times
``v <- v - alpha*Hv ; p <- p + v``; result ``alpha*p`` pushed through the mixed second derivative.
Each iteration is ONE streaming kernel (20*N bytes: read Hv, v, p; write v, p) instead of 4*T
ATen launches; the final ``alpha*p`` and the negation are folded into the last iteration.
"""
from __future__ import annotations

from ..backend import get_backend
from ._common import GradientPair, InnerOperator
from .structured import structured_hvp_for


def neumann(vector, curr, prev, sync):
    assert len(curr.paths) == 0, "neumann method is not supported for higher order MLO!"
    vector = list(vector)
    K = int(curr.config.neumann_iterations)
    # neumann.py:39 differentiates w.r.t. trainable_parameters() (cg uses parameters())
    op = InnerOperator(curr, prev, K, vector, structured_hvp_for(curr, prev), curr.trainable_parameters())
    with op.stream():
        try:
            return _neumann(vector, op, K, sync)
        finally:
            op.close()   # (a finite-difference solve that raised must not leave the weights perturbed)


def _neumann(vector, op, K, sync):
    be = get_backend()
    layout = be.layout(vector)
    v, p = layout.state(2)
    v_views = layout.views(v, vector)
    hvp_fn = op.hvp(v_views)
    provider = op.provider

    alpha = float(op.curr.config.neumann_alpha)
    fused = getattr(provider, "fused_neumann", None)
    # a provider whose fused solver derives the mixed derivative from batch-sized factors never touches the accumulator
    skips = getattr(provider, "fused_neumann_skips_solution", None)
    skip_p = bool(fused is not None and alpha != 0.0 and skips is not None and skips(layout, K))
    be.neumann_init(layout, vector, v, None if skip_p else p)  # p = v   (neumann.py:60)

    solve = fused(layout, v, p, K, alpha) if (fused is not None and alpha != 0.0) else False
    if not solve:   # (else the provider's own kernels ran all K iterations: v ping-pongs with a third flat vector of the layout)
        for k in range(K):
            hvp = hvp_fn(v_views)  # neumann.py:62
            last = k == K - 1 and alpha != 0.0
            out_scale = op.out_sign * alpha if last else 0.0   # (-alpha; +alpha for the finite-difference hop, see InnerOperator)
            if isinstance(hvp, GradientPair):   # two first-order gradients: (g+ - g-) / 2 eps is formed inside the step's kernel
                be.neumann_step_fd(layout, hvp.plus, hvp.minus, hvp.two_eps, v, p, alpha, out_scale=out_scale, hvp_shift=op.shift)
            else:
                be.neumann_step(layout, hvp, v, p, alpha, out_scale=out_scale, hvp_shift=op.shift)  # 63-64 (+66)
        if K == 0 or alpha == 0.0:
            be.scale_flat(p, op.out_sign * alpha)  # alpha * p (with p = v when K == 0)   (neumann.py:66)

    return op.mixed(layout.views(p, vector), sync, solve)

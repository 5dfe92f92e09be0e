"""Neumann-series best-response-Jacobian product on fused gfx950 kernels.

Behavioural twin of /root/reference betty/hypergradient/neumann.py:8-66: ``p = v``; K times
``v <- v - alpha*Hv ; p <- p + v``; result ``alpha*p`` pushed through the mixed second derivative.
Each iteration is ONE streaming kernel (20*N bytes: read Hv, v, p; write v, p) instead of 4*T
ATen launches; the final ``alpha*p`` and the negation are folded into the last iteration.
"""
from __future__ import annotations

from ..backend import get_backend
from ._common import InnerOperator
from .structured import structured_hvp_for


def neumann(vector, curr, prev, sync):
    assert len(curr.paths) == 0, "neumann method is not supported for higher order MLO!"
    vector = list(vector)
    K = int(curr.config.neumann_iterations)
    # neumann.py:39 differentiates w.r.t. trainable_parameters() (cg uses parameters())
    op = InnerOperator(curr, prev, K, vector, structured_hvp_for(curr, prev), curr.trainable_parameters())
    with op.stream():
        return _neumann(vector, op, K, sync)


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
            be.neumann_step(layout, hvp, v, p, alpha, out_scale=(-alpha if last else 0.0), hvp_shift=op.shift)  # 63-64 (+66)
        if K == 0 or alpha == 0.0:
            be.scale_flat(p, -alpha)  # alpha * p (with p = v when K == 0)   (neumann.py:66)

    return op.mixed(layout.views(p, vector), sync, solve)

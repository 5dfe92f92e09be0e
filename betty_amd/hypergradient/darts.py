"""Central finite-difference best-response-Jacobian product ("darts") on gfx950 kernels.

Behavioural twin of /root/reference betty/hypergradient/darts.py:8-69.  The vector work —
``||v||``, the three in-place perturbations of the live inner weights — is four multi-tensor
launches (40*N bytes) instead of ``cat`` + ``norm`` + 3*T ``add_`` calls, and ``eps`` stays on
the device (the reference synchronises the host with ``.item()``, darts.py:35).

An inner problem with a structure (``hypergradient_structure``, structured.py) whose provider offers ``finite_difference`` takes
the whole hop from it — for WeightedCEMLP two native forward passes instead of two ``training_step`` calls through autograd, for
ProximalRegularized and LogisticRegressionL2 one streaming launch and no forward pass at all (the difference is exact there) — and
everything else (no structure, FSDP, a collective, upper parameters the structure does not describe) runs the opaque path.  Both
live in ``finite_difference``, which sama shares on its preconditioned direction.
"""
from __future__ import annotations

import torch

from ..backend import get_backend
from ._common import is_fsdp
from .structured import structured_hvp_for
from .utils import grad, replace_none_with_zero


def darts(vector, curr, prev, sync):
    config = curr.config
    fsdp = is_fsdp(curr)
    be = get_backend()
    vector = list(vector)
    layout = be.layout(vector)
    # eps = R / (||v|| + 1e-15)   (darts.py:29-35), 0-dim device tensors
    eps32, eps64, sumsq = be.darts_eps(layout, vector, float(config.darts_alpha))
    if fsdp:
        # darts.py:31-34: every rank holds a shard of v; eps uses the norm of the whole vector.  Same fp32
        # steps as the reference: local norm -> square -> all-reduce(SUM) -> sqrt -> + 1e-15 -> R / .
        import torch.distributed as dist

        sq = sumsq.sqrt().to(torch.float32).pow(2)
        dist.all_reduce(sq, op=dist.ReduceOp.SUM)
        norm = sq.sqrt().add_(1e-15)
        eps64 = float(config.darts_alpha) / norm.to(torch.float64)
        eps32 = eps64.to(torch.float32)
    return finite_difference(curr, prev, layout, vector, eps32, eps64, sync, restore=not config.darts_multitask, is_fsdp=fsdp)


def finite_difference(curr, prev, layout, direction, eps32, eps64, sync, restore, is_fsdp=False, opaque_loss=None):
    """The central finite difference of darts and sama along ``direction`` with radius ``eps``: the structure's own
    ``finite_difference`` when it offers one (never under FSDP), else two ``training_step`` calls through autograd at
    ``w +- eps * direction``.  ``restore``: put the inner weights back afterwards (the multitask variants do not).
    ``opaque_loss``: go straight to the opaque branch and evaluate the inner loss with this callable instead of a bare
    ``training_step_exec`` (the final hop of a finite-difference cg / neumann solve, _common.FiniteDifferenceHVP.mixed)."""
    if not is_fsdp and opaque_loss is None:
        fd = getattr(structured_hvp_for(curr, prev), "finite_difference", None)
        if fd is not None:
            out = fd(layout, direction, eps32, eps64, sync, restore=restore)
            if out is not NotImplemented:
                return out
    be = get_backend()
    weights = [w.data for w in curr.meta_trainable_parameters()]
    upper = prev.trainable_parameters()
    two_eps = (2.0 * eps64).to(torch.float32)  # the reference divides fp32 tensors by the Python float 2*eps

    # w <- w + eps*v   (darts.py:37-38)
    be.axpy_multi(layout, weights, direction, eps32, 1.0)
    loss_p = curr.training_step_exec(curr.cur_batch) if opaque_loss is None else opaque_loss()
    # is_fsdp: the gradient of a flat shard only materialises through backward into .grad (darts.py:40-42, utils.py:9-17)
    grad_p = replace_none_with_zero(grad(loss_p, upper, allow_unused=True, is_fsdp=is_fsdp), upper)
    if sync:
        # darts.py:44-46: -g+/(2 eps) goes straight into .grad
        prev.set_grads(upper, [-(g / two_eps) for g in grad_p])

    # w <- w - 2*eps*v   (darts.py:49-50)
    be.axpy_multi(layout, weights, direction, eps32, -2.0)
    loss_n = curr.training_step_exec(curr.cur_batch) if opaque_loss is None else opaque_loss()
    if sync:
        torch.autograd.backward(loss_n / two_eps, inputs=upper)  # darts.py:52-53 (DDP hooks fire)
        grad_n = None
    else:
        grad_n = replace_none_with_zero(grad(loss_n, upper, allow_unused=True, is_fsdp=is_fsdp), upper)  # darts.py:55-58

    # restore w   (darts.py:61-63)
    if restore:
        be.axpy_multi(layout, weights, direction, eps32, 1.0)

    if sync:
        return None
    return [(gn - gp) / two_eps for gn, gp in zip(grad_n, grad_p)]  # darts.py:65-67

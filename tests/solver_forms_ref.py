"""fp64 reference of every form of the fused MLP solvers (tests/test_solver_forms_fp64.py): numpy / torch on the CPU only, built on
tests/head_j_ref.py (problem, plain_cg, kink_margin, rel, flat are its own).

  plain_neumann   neumann.py:59-66 on N-sized lists with a double-backward HVP, in the problem's own dtype: alpha * sum_{k<=K} v_k
  hypergradient   hypergrad_oracle.cg / .neumann (bit-pinned to the reference elsewhere in the suite)
  solution        the 2L tensors the solvers return, in the scaling include/bhg.h documents: -cg_alpha * x_K (CG), -alpha * p_K
                  (Neumann) — from plain_cg / plain_neumann
  mixed_coeff     coeff[b] = (prob_b - onehot(y_b)) . Rz_b(solution) / B, the R-forward written out layer by layer
  quantities      all of them for one instance, setting, algorithm and dtype, from ONE construction of the problem; it also carries
                  the plain solve to the hypergradient twice — through autograd (the oracle's own last step) and through the
                  coefficient (sum_b coeff_b d w_b / d upper) — which is how the CPU tests tie the three references to the oracle

Nothing of the projected algebra enters: no Gram matrix, no G(.) recurrence, no J.  The fp32 run (dtype=torch.float32) shows what a
correct fp32 computation gives on the same draws."""
import numpy as np
import torch
import torch.nn.functional as F

import head_j_ref as R
from head_j_ref import Config, flat, kink_margin, orc, plain_cg, problem, rel  # noqa: F401  (re-exported: the test file reads them here)


def configured_problem(dims, B, ridge, K, step, seed, algo, dtype=torch.float64, device="cpu"):
    """head_j_ref.problem with the configuration of `algo`: it builds a CG config (cg_alpha = step); Neumann gets its own."""
    curr, prev, vector = R.problem(dims, B, ridge, K, step, seed, dtype=dtype, device=device)
    if algo == "neumann":
        curr.config = Config(type="neumann", neumann_iterations=K, neumann_alpha=step)
    else:
        assert algo == "cg", algo
    return curr, prev, vector


def _inner_gradient(curr):
    params = list(curr.module.parameters())
    return params, torch.autograd.grad(curr.training_step_exec(curr.cur_batch), params, create_graph=True)


def plain_neumann(curr, vector):
    """neumann.py:59-66: acc = v; K times v <- v - alpha H v, acc <- acc + v; returns alpha * acc = alpha * sum_{k<=K} v_k."""
    cfg = curr.config
    params, grad = _inner_gradient(curr)
    v = [t.clone() for t in vector]
    acc = [t.clone() for t in vector]
    for _ in range(cfg.neumann_iterations):
        Hv = torch.autograd.grad(grad, params, grad_outputs=v, retain_graph=True)
        v = [vi - cfg.neumann_alpha * hi for vi, hi in zip(v, Hv)]
        acc = [ai + vi for ai, vi in zip(acc, v)]
    return [cfg.neumann_alpha * a for a in acc]


def _solution(curr, vector, algo):
    """-cg_alpha * x_K (plain_cg returns cg_alpha * x_K) / -alpha * p_K (plain_neumann returns alpha * p_K), detached."""
    series = plain_cg(curr, vector)[1] if algo == "cg" else plain_neumann(curr, vector)
    return [(-t).detach() for t in series]


def _mixed_coeff(curr, sol):
    """coeff[b] = (prob_b - onehot(y_b)) . Rz_b(sol) / B: forward pass, then the R-forward in direction `sol`, layer by layer."""
    x, y = curr.cur_batch
    lins = list(curr.module.layers)
    L, B = len(lins), x.shape[0]
    V, c = sol[0::2], sol[1::2]
    with torch.no_grad():
        h, Rh = x, None
        for l, lin in enumerate(lins):
            W, b = lin.weight.detach(), lin.bias.detach()
            a = h @ W.t() + b
            Ra = h @ V[l].t() + c[l]
            if Rh is not None:
                Ra = Ra + Rh @ W.t()
            if l < L - 1:
                m = (a > 0).to(a.dtype)
                h, Rh = a * m, Ra * m
        prob = F.softmax(a, 1)
        return ((prob - F.one_hot(y, a.shape[1]).to(a.dtype)) * Ra).sum(1) / B


def _hypergradient_through_autograd(curr, prev, sol):
    """cg.py:58-68 / neumann.py:44-54 on the (already negated and scaled) solution: d/d(upper) <grad_inner, sol>."""
    _, grad = _inner_gradient(curr)
    return flat(torch.autograd.grad(grad, prev.trainable_parameters(), grad_outputs=sol))


def _hypergradient_through_coeff(curr, prev, coeff):
    """The inner loss is mean_b w_b ce_b + ridge |theta|^2 with w_b = upper(ce_b): <grad_inner, sol> = sum_b w_b coeff_b, so the
    hypergradient is sum_b coeff_b d w_b / d(upper)."""
    x, y = curr.cur_batch
    with torch.no_grad():
        ce = F.cross_entropy(curr.module(x), y, reduction="none")
    w = prev.fwd(ce.reshape(-1, 1)).reshape(-1)
    return flat(torch.autograd.grad(w, prev.trainable_parameters(), grad_outputs=coeff))


def quantities(dims, B, ridge, K, step, seed, algo, dtype=torch.float64):
    """{"hypergradient": the oracle's, flat; "solution": the 2L tensors; "coeff": B numbers; "hypergradient_plain" /
    "hypergradient_coeff": the plain solve carried to the hypergradient through autograd / through the coefficient} as fp64 numpy."""
    curr, prev, vector = configured_problem(dims, B, ridge, K, step, seed, algo, dtype)
    sol = _solution(curr, vector, algo)
    coeff = _mixed_coeff(curr, sol)
    return {
        "hypergradient": flat(getattr(orc, algo)(vector, curr, prev, False)),
        "solution": [t.numpy().astype(np.float64) for t in sol],
        "coeff": coeff.numpy().astype(np.float64),
        "hypergradient_plain": _hypergradient_through_autograd(curr, prev, sol),
        "hypergradient_coeff": _hypergradient_through_coeff(curr, prev, coeff),
    }


def hypergradient(dims, B, ridge, K, step, seed, algo, dtype=torch.float64):
    curr, prev, vector = configured_problem(dims, B, ridge, K, step, seed, algo, dtype)
    return flat(getattr(orc, algo)(vector, curr, prev, False))


def solution(dims, B, ridge, K, step, seed, algo, dtype=torch.float64):
    curr, _, vector = configured_problem(dims, B, ridge, K, step, seed, algo, dtype)
    return [t.numpy().astype(np.float64) for t in _solution(curr, vector, algo)]


def mixed_coeff(dims, B, ridge, K, step, seed, algo, dtype=torch.float64):
    curr, _, vector = configured_problem(dims, B, ridge, K, step, seed, algo, dtype)
    return _mixed_coeff(curr, _solution(curr, vector, algo)).numpy().astype(np.float64)

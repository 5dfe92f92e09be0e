"""ATen restatement of the finite-difference cg / neumann solve — TEST INFRASTRUCTURE (the checker of tests/test_fd_hvp*.py).

The same algorithm the product runs for ``hypergradient_hvp = "finite_difference"``, written with plain tensor ops in the dtype of
the problem it is given (fp32 or fp64): the same eps rule (eps = R / (||p|| + 1e-15)), gradients by FIRST-order autograd at
w0 +- eps p (perturbed from a snapshot), the reference's recurrences (cg.py:34-56 with its cg_alpha quirk, neumann.py:59-66) on the
materialised difference (g+ - g-) / (2 eps), and the central-difference final hop along u = -alpha x.  No kernel, no flat layout.
"""
import torch


def _dot(a, b):
    return sum((x * y).sum() for x, y in zip(a, b))


def _grads(curr, wrt):
    loss = curr.training_step_exec(curr.cur_batch)
    gs = torch.autograd.grad(loss, wrt, allow_unused=True)
    return [torch.zeros_like(w) if g is None else g.detach() for g, w in zip(gs, wrt)]


def _eps(direction, R):
    return R / (float(torch.sqrt(_dot(direction, direction))) + 1e-15)


def fd_product(curr, w0, direction, R):
    """(grad L(w0 + eps d) - grad L(w0 - eps d)) / (2 eps); the weights are left at w0."""
    params = list(curr.trainable_parameters())
    eps = _eps(direction, R)
    out = []
    for sign in (1.0, -1.0):
        with torch.no_grad():
            for p, w, d in zip(params, w0, direction):
                p.copy_(w + (sign * eps) * d)
        out.append(_grads(curr, params))
    with torch.no_grad():
        for p, w in zip(params, w0):
            p.copy_(w)
    return [(a - b) / (2.0 * eps) for a, b in zip(*out)]


def fd_last_hop(curr, prev, w0, u, R):
    """d/d eps grad_lambda L(w0 + eps u) at 0 by a central difference; the weights are left at w0."""
    params, upper = list(curr.trainable_parameters()), list(prev.trainable_parameters())
    eps = _eps(u, R)
    out = []
    for sign in (1.0, -1.0):
        with torch.no_grad():
            for p, w, d in zip(params, w0, u):
                p.copy_(w + (sign * eps) * d)
        out.append(_grads(curr, upper))
    with torch.no_grad():
        for p, w in zip(params, w0):
            p.copy_(w)
    return [(a - b) / (2.0 * eps) for a, b in zip(*out)]


def fd_solve(algo, vector, curr, prev, R=0.01):
    """The hypergradient list (sync=False) of ``cg`` / ``neumann`` with every Hessian-vector product a central difference."""
    params = list(curr.trainable_parameters())
    w0 = [p.detach().clone() for p in params]
    vector = [v.detach().clone() for v in vector]
    if algo == "cg":
        K, alpha = int(curr.config.cg_iterations), float(curr.config.cg_alpha)
        x = [torch.zeros_like(v) for v in vector]
        r = [v.clone() for v in vector]
        p = [v.clone() for v in vector]
        for _ in range(K):
            hp = fd_product(curr, w0, p, R)
            rr = _dot(r, r)
            a = rr / _dot([alpha * h for h in hp], p)
            x = [xi + a * pi for xi, pi in zip(x, p)]
            r = [ri - a * hi for ri, hi in zip(r, hp)]
            b = _dot(r, r) / rr
            p = [ri + b * pi for ri, pi in zip(r, p)]
        u = [-(alpha * xi) for xi in x]
    else:
        K, alpha = int(curr.config.neumann_iterations), float(curr.config.neumann_alpha)
        v = [t.clone() for t in vector]
        acc = [t.clone() for t in vector]
        for _ in range(K):
            hv = fd_product(curr, w0, v, R)
            v = [vi - alpha * hi for vi, hi in zip(v, hv)]
            acc = [ai + vi for ai, vi in zip(acc, v)]
        u = [-(alpha * ai) for ai in acc]
    return fd_last_hop(curr, prev, w0, u, R)

"""fp64 reference of the head_j form's shape family (tests/test_head_j_fp64.py): numpy / torch on the CPU only.

  problem                  the draws of test_gpu_parity._mlp_problem — CPU generator, fp32 draws, then cast / moved — so the GPU, the
                           CPU fp32 run and the CPU fp64 run see the same numbers
  hypergradient64 / 32     hypergrad_oracle.cg (bit-pinned to the reference elsewhere in the suite) on the fp64 / fp32 problem;
                           spread = rel(hypergradient32, hypergradient64) is the reference's own rounding error on the instance
  last_iteration_arrays64  Rh_2, Rd_2, Rd_3 of the LAST CG iteration: plain N-sized CG with the reference's quirk (the step length uses
                           cg_alpha * Hp, the residual update the un-scaled Hp) and a double-backward HVP gives p_{K-1}; the R-forward and
                           R-backward of that direction are then written out layer by layer.  No projected recurrence, no Gram matrix,
                           no J: independent of the algebra under test.
  kink_margin              how far the instance's ReLUs sit from their kinks, in fp64
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import hypergrad_oracle as orc  # noqa: E402
import zoo  # noqa: E402
from betty_amd import Config  # noqa: E402


def problem(dims, B, ridge, K, alpha, seed, dtype=torch.float64, device="cpu"):
    """(curr, prev, vector).  Order and scale of the draws are test_gpu_parity._mlp_problem's; vector = 0.1 * direction is formed in
    fp32 (what the GPU tests hand the solver) before the cast."""
    g = torch.Generator().manual_seed(seed)
    inner, upper = zoo.MLP(dims), zoo.MWN(16)
    with torch.no_grad():
        for p in list(inner.parameters()) + list(upper.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (1.0 / max(p.shape[-1], 4) ** 0.5))
    x = torch.randn(B, dims[0], generator=g)
    y = torch.randint(0, dims[-1], (B,), generator=g)
    direction = [torch.randn(p.shape, generator=g) for p in inner.parameters()]
    vector = [(0.1 * d).to(device=device, dtype=dtype) for d in direction]
    inner, upper = inner.to(device=device, dtype=dtype), upper.to(device=device, dtype=dtype)
    x, y = x.to(device=device, dtype=dtype), y.to(device)
    prev = zoo.StubProblem("upper", upper, config=Config())
    curr = zoo.StubProblem("inner", inner, config=Config(type="cg", cg_iterations=K, cg_alpha=alpha),
                           loss_fn=zoo.make_reweight_loss(prev, ridge), batch=(x, y))
    return curr, prev, vector


def flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().astype(np.float64).ravel() for t in tensors])


def rel(got, want):
    """Relative L2 error of a list of tensors / arrays against a flat fp64 vector."""
    g = np.concatenate([np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float64).ravel() for t in got])
    w = np.asarray(want, dtype=np.float64).ravel()
    return float(np.linalg.norm(g - w) / np.linalg.norm(w)) if np.all(np.isfinite(g)) else float("inf")


def _hypergradient(dims, B, ridge, K, alpha, seed, dtype):
    curr, prev, vector = problem(dims, B, ridge, K, alpha, seed, dtype=dtype)
    return flat(orc.cg(vector, curr, prev, False))


def hypergradient64(dims, B, ridge, K, alpha, seed):
    return _hypergradient(dims, B, ridge, K, alpha, seed, torch.float64)


def hypergradient32(dims, B, ridge, K, alpha, seed):
    return _hypergradient(dims, B, ridge, K, alpha, seed, torch.float32)


def kink_margin(dims, B, seed):
    """The smallest |pre-activation| over every ReLU of the inner net and of the meta-weight-net in fp64 — the smaller of its absolute
    value and its ratio to the layer's mean |pre-activation| (the measure of tests/golden/make_shapes_golden.py)."""
    curr, prev, _ = problem(dims, B, 0.0, 1, 1.0, seed)
    x, y = curr.cur_batch
    h, m = x, float("inf")
    with torch.no_grad():
        for lin in curr.module.layers[:-1]:
            a = lin(h)
            m = min(m, a.abs().min().item(), (a.abs().min() / a.abs().mean()).item())
            h = F.relu(a)
        ce = F.cross_entropy(curr.module.layers[-1](h), y, reduction="none")
        a = prev.module.l1(ce.reshape(-1, 1))
    return min(m, a.abs().min().item(), (a.abs().min() / a.abs().mean()).item())


def plain_cg(curr, vector):
    """cg.py:34-56 on N-sized lists with a double-backward HVP, in the problem's own dtype: (p_{K-1}, x_final).  The quirk: the step
    length divides by cg_alpha * <Hp, p>, the residual takes the un-scaled Hp; x_final = cg_alpha * sum_k a_k p_k."""
    cfg = curr.config
    params = list(curr.module.parameters())
    grad = torch.autograd.grad(curr.training_step_exec(curr.cur_batch), params, create_graph=True)
    dot = lambda a, b: sum((u * v).sum() for u, v in zip(a, b))
    x = [torch.zeros_like(v) for v in vector]
    r = [v.clone() for v in vector]
    p = [v.clone() for v in vector]
    p_last = None
    for _ in range(cfg.cg_iterations):
        p_last = [t.clone() for t in p]
        Hp = torch.autograd.grad(grad, params, grad_outputs=p, retain_graph=True)
        rr = dot(r, r)
        a = rr / (cfg.cg_alpha * dot(Hp, p))
        x = [xi + a * pi for xi, pi in zip(x, p)]
        r = [ri - a * hi for ri, hi in zip(r, Hp)]
        beta = dot(r, r) / rr
        p = [ri + beta * pi for ri, pi in zip(r, p)]
    return p_last, [cfg.cg_alpha * xi for xi in x]


def hypergradient_of_plain_cg(curr, prev, vector):
    """plain_cg carried to the hypergradient: - d/d(upper) <grad_inner, x_final> (cg.py:58-68)."""
    _, x = plain_cg(curr, vector)
    params = list(curr.module.parameters())
    grad = torch.autograd.grad(curr.training_step_exec(curr.cur_batch), params, create_graph=True)
    out = torch.autograd.grad(grad, prev.trainable_parameters(), grad_outputs=x)
    return flat([-o for o in out])


def last_iteration_arrays(curr, prev, vector):
    """{"Rh2", "Rd2", "Rd3"} of the last CG iteration as numpy fp64 arrays of B rows, computed in the problem's own dtype (the fp32 run
    shows what a correct fp32 computation gives).  Four-layer nets only."""
    p, _ = plain_cg(curr, vector)
    x, y = curr.cur_batch
    lins = list(curr.module.layers)
    assert len(lins) == 4
    Ws, bs = [l.weight.detach() for l in lins], [l.bias.detach() for l in lins]
    V, c = p[0::2], p[1::2]
    B = x.shape[0]
    with torch.no_grad():
        hs, masks, h = [x], [], x
        for l in range(4):
            a = h @ Ws[l].t() + bs[l]
            if l < 3:
                m = (a > 0).to(a.dtype)
                h = a * m
                masks.append(m)
                hs.append(h)
        prob = F.softmax(a, 1)
        ce = -F.log_softmax(a, 1).gather(1, y.reshape(-1, 1)).reshape(-1)
        sd = prev.fwd(ce.reshape(-1, 1)).reshape(-1) / B
        delta3 = sd[:, None] * (prob - F.one_hot(y, a.shape[1]).to(a.dtype))
        Rh0 = masks[0] * (hs[0] @ V[0].t() + c[0])
        Rh1 = masks[1] * (Rh0 @ Ws[1].t() + hs[1] @ V[1].t() + c[1])
        Rh2 = masks[2] * (Rh1 @ Ws[2].t() + hs[2] @ V[2].t() + c[2])
        Rz = Rh2 @ Ws[3].t() + hs[3] @ V[3].t() + c[3]
        Rd3 = sd[:, None] * (prob * Rz - prob * (prob * Rz).sum(1, keepdim=True))
        Rd2 = masks[2] * (delta3 @ V[3] + Rd3 @ Ws[3])
    return {k: v.numpy().astype(np.float64) for k, v in (("Rh2", Rh2), ("Rd2", Rd2), ("Rd3", Rd3))}


def last_iteration_arrays64(dims, B, ridge, K, alpha, seed):
    curr, prev, vector = problem(dims, B, ridge, K, alpha, seed, dtype=torch.float64)
    return last_iteration_arrays(curr, prev, vector)


def last_iteration_arrays32(dims, B, ridge, K, alpha, seed):
    curr, prev, vector = problem(dims, B, ridge, K, alpha, seed, dtype=torch.float32)
    return last_iteration_arrays(curr, prev, vector)

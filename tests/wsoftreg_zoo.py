"""The seeded sample-weighted softmax-regression instance shared by tests/golden/make_wsoftreg_golden.py (the real reference, build
container only), the CPU tests of WeightedSoftmaxRegression and the GPU tests of its native path: n = 64, d = 20, C = 5, the inner
model ``nn.Linear(d, C, bias=False)`` under cross-entropy weighted per sample by a = sigmoid(theta) — a NON-leaf function of the upper
problem's parameter theta in R^n — plus a constant per-weight L2 penalty reg in [0.5, 1.5).  Inputs are stored in
tests/golden/wsoftreg.npz so every consumer sees bit-identical numbers; the problems are zoo.StubProblem pairs like every other case."""
import dataclasses
from typing import Dict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import zoo

N_ROWS, N_FEATURES, N_CLASSES = 64, 20, 5


@dataclasses.dataclass
class Case:
    name: str
    algo: str
    cfg: Dict
    family: str = "wsoftreg"
    rtol: float = 1e-4


CASES = [
    Case("wsoftreg_cg5", "cg", dict(type="cg", cg_iterations=5, cg_alpha=1.0)),
    Case("wsoftreg_cg5_a01", "cg", dict(type="cg", cg_iterations=5, cg_alpha=0.1)),
    Case("wsoftreg_neumann5", "neumann", dict(type="neumann", neumann_iterations=5, neumann_alpha=0.25)),
    Case("wsoftreg_darts", "darts", dict(type="darts", darts_alpha=0.01)),
    Case("wsoftreg_sama", "sama", dict(type="sama", sama_adam_alpha=0.01)),
]
CASE_BY_NAME = {c.name: c for c in CASES}


class SampleWeights(nn.Module):
    """The upper problem: one raw score per training sample; forward returns a = sigmoid(theta) in (0, 1), a non-leaf."""

    def __init__(self, rows):
        super().__init__()
        self.theta = nn.Parameter(torch.zeros(rows))

    def forward(self):
        return torch.sigmoid(self.theta)


def make_wsoftreg_loss(upper, reg, label_smoothing=0.0, reduction="mean", penalty=0.5):
    """What the user writes in ``training_step``; the keyword arguments are the broken promises the structure guard must catch.
    reduction: "mean" (sum / n, the declared form) | "sum" | "normalised" (sum / a.sum())."""
    def loss(self, batch):
        x, y = batch
        a = upper.fwd()
        w = self.module.weight
        ce = a * F.cross_entropy(self.module(x), y, label_smoothing=label_smoothing, reduction="none")
        data = {"mean": lambda: ce.mean(), "sum": lambda: ce.sum(), "normalised": lambda: ce.sum() / a.sum()}[reduction]()
        return data + penalty * (reg.to(w.dtype) * w * w).sum()

    return loss


def seed_inputs(seed=0):
    """Run ONCE by make_wsoftreg_golden.py; everyone else loads the stored arrays."""
    g = torch.Generator().manual_seed(4000 + seed)
    arrays = {
        "batch_x": torch.randn(N_ROWS, N_FEATURES, generator=g),
        "batch_y": torch.randint(0, N_CLASSES, (N_ROWS,), generator=g),
        "inner_0": 0.3 * torch.randn(N_CLASSES, N_FEATURES, generator=g),
        "upper_0": torch.randn(N_ROWS, generator=g),
        "reg": 0.5 + torch.rand(N_CLASSES, N_FEATURES, generator=g),
        "vec_0": 0.01 * torch.randn(N_CLASSES, N_FEATURES, generator=g),
    }
    return {k: v.numpy() for k, v in arrays.items()}


def build_case(case, inputs, config_cls, device="cpu", dtype=torch.float32, inner=None, batch_y=None, **loss_kw):
    """(curr, prev, vector) of a case from stored inputs.  ``inner``: another inner module (a bias) for the refusal tests; ``batch_y``:
    other labels (outside [0, C)) for the guard's."""
    def T(a):
        t = torch.from_numpy(np.asarray(a))
        return (t.to(dtype) if t.is_floating_point() else t).to(device)

    if inner is None:
        inner = nn.Linear(N_FEATURES, N_CLASSES, bias=False)
    upper = SampleWeights(N_ROWS)
    inner, upper = inner.to(device=device, dtype=dtype), upper.to(device=device, dtype=dtype)
    weight = next(m for m in inner.modules() if isinstance(m, nn.Linear)).weight
    weight.data.copy_(T(inputs["inner_0"]))
    upper.theta.data.copy_(T(inputs["upper_0"]))
    prev = zoo.StubProblem("upper", upper, config=config_cls())
    curr = zoo.StubProblem("inner", inner, config=config_cls(**case.cfg), loss_fn=make_wsoftreg_loss(prev, T(inputs["reg"]), **loss_kw),
                           batch=(T(inputs["batch_x"]), T(inputs["batch_y"] if batch_y is None else batch_y)))
    curr.reg = T(inputs["reg"])
    if case.algo == "sama":
        curr.optimizer = torch.optim.SGD(inner.parameters(), lr=0.1)   # SGD: the identity preconditioner
    vector = [T(inputs["vec_0"])] + [torch.zeros_like(p) for p in list(inner.parameters())[1:]]
    return curr, prev, vector


def attach_structure(curr, impl=None, **kw):
    from betty_amd.hypergradient.structured import WeightedSoftmaxRegression

    weight = next(m for m in curr.module.modules() if isinstance(m, nn.Linear)).weight
    curr.hypergradient_structure = lambda prev: WeightedSoftmaxRegression(curr, prev, weight, weight_fn=lambda: prev.fwd(), reg=curr.reg,
                                                                          impl=impl, **kw)
    return curr

#!/usr/bin/env python
"""Softmax-regression hyper-parameter optimisation: the reference's logistic-regression HPO example on multi-class data (the way it
is run on MNIST-style problems: d features, C classes) on the MI355X backend.

Two-level problem: the inner problem fits a linear classifier ``nn.Linear(d, C, bias=False)`` under cross-entropy with one L2
coefficient per weight; the outer problem tunes the coefficients lam = softplus(theta) on validation data through the implicit
hypergradient (cg / neumann / darts / sama).  ``--analytic`` declares the structure: cg / neumann then run their whole K loop in
native launches (csrc/bhg_softreg_solve.hip), darts / sama take the closed-form hop.

    python examples/softmax_regression_hpo.py --algo cg --analytic
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betty_amd import Config  # noqa: E402
from betty_amd.engine import Engine, EngineConfig  # noqa: E402
from betty_amd.problems import ImplicitProblem  # noqa: E402


class Penalty(torch.nn.Module):
    def __init__(self, classes, d):
        super().__init__()
        self.theta = torch.nn.Parameter(torch.zeros(classes, d))

    def forward(self):
        return F.softplus(self.theta)


class Outer(ImplicitProblem):
    def training_step(self, batch):
        x, y = batch
        return F.cross_entropy(self.inner(x), y)


class Inner(ImplicitProblem):
    def training_step(self, batch):
        x, y = batch
        w = self.module.weight
        return F.cross_entropy(self.module(x), y) + 0.5 * (self.outer() * w * w).sum()

    def on_inner_loop_start(self):
        self.module.weight.data.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="cg", choices=["cg", "neumann", "darts", "sama"])
    ap.add_argument("--dim", type=int, default=784)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--analytic", action="store_true", help="declare SoftmaxRegressionL2 (closed-form products, native solve)")
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    d, C = args.dim, args.classes
    w_gt = rng.randn(C, d) / np.sqrt(d)
    x = rng.randn(1000, d)
    x[:, -1] = 1.0   # the model has no bias: a column of ones stands in for it
    y = (x @ w_gt.T + 0.1 * rng.randn(1000, C)).argmax(axis=1)
    tx = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    ty = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))
    cfg = {
        "cg": Config(type="cg", cg_iterations=5, cg_alpha=1.0, unroll_steps=100),
        "neumann": Config(type="neumann", neumann_iterations=5, neumann_alpha=0.25, unroll_steps=100),
        "darts": Config(type="darts", unroll_steps=100),
        "sama": Config(type="sama", unroll_steps=100),
    }[args.algo]
    penalty, linear = Penalty(C, d), torch.nn.Linear(d, C, bias=False)
    outer = Outer(name="outer", module=penalty, optimizer=torch.optim.SGD(penalty.parameters(), lr=1.0, momentum=0.9),
                  train_data_loader=[(tx(x[500:]), ty(y[500:]))], config=Config())
    inner = Inner(name="inner", module=linear, optimizer=torch.optim.SGD(linear.parameters(), lr=0.1),
                  train_data_loader=[(tx(x[:500]), ty(y[:500]))], config=cfg)
    if args.analytic:
        from betty_amd.hypergradient.structured import SoftmaxRegressionL2

        inner.hypergradient_structure = lambda prev: SoftmaxRegressionL2(inner, prev, linear.weight, lam_fn=lambda: prev())
    engine = Engine(config=EngineConfig(train_iters=args.iters), problems=[outer, inner],
                    dependencies={"u2l": {outer: [inner]}, "l2u": {inner: [outer]}})
    engine.run()
    val = outer.training_step(outer.cur_batch).item()
    print(f"algo={args.algo} analytic={args.analytic}  final validation loss {val:.4f}")


if __name__ == "__main__":
    main()

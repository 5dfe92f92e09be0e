#!/usr/bin/env python
"""Data hyper-cleaning on a linear classifier: learn ONE WEIGHT PER TRAINING SAMPLE so that a softmax regression trained on noisy
labels does well on a small clean validation set — the reference's learning_to_reweight / bert_data_reweighting reduced to a linear
model on fixed features, on the MI355X backend.  A toy that needs no dataset and runs in seconds.

Two-level problem: the inner problem fits ``nn.Linear(d, C, bias=False)`` under per-sample-weighted cross-entropy with a constant L2
penalty; the outer problem tunes the sample weights a = sigmoid(theta), theta in R^n, on clean data through the implicit hypergradient.
``--analytic`` declares the structure: cg / neumann then run their whole K loop and the mixed second derivative in native launches
(csrc/bhg_softreg_solve.hip); darts / sama stay on the opaque path.

    python examples/sample_reweighting_linear.py --algo cg --analytic
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

REG = 1e-3


class SampleWeights(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.theta = torch.nn.Parameter(torch.zeros(n))

    def forward(self):
        return torch.sigmoid(self.theta)


class Outer(ImplicitProblem):
    def training_step(self, batch):
        x, y = batch
        return F.cross_entropy(self.inner(x), y)


class Inner(ImplicitProblem):
    def training_step(self, batch):
        x, y = batch   # the whole (noisy) training set, rows in the order of the weights
        w = self.module.weight
        return (self.outer() * F.cross_entropy(self.module(x), y, reduction="none")).mean() + 0.5 * REG * (w * w).sum()

    def on_inner_loop_start(self):
        self.module.weight.data.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="cg", choices=["cg", "neumann", "darts", "sama"])
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.4, help="fraction of training labels replaced by a random class")
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--analytic", action="store_true", help="declare WeightedSoftmaxRegression (closed-form products, native solve)")
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    d, C, n = args.dim, args.classes, 500
    w_gt = rng.randn(C, d)
    x = rng.randn(n + 200, d)
    x[:, -1] = 1.0   # the model has no bias: a column of ones stands in for it
    y = (x @ w_gt.T).argmax(axis=1)
    flipped = rng.rand(n) < args.noise
    y_noisy = np.where(flipped, rng.randint(0, C, n), y[:n])
    flipped &= y_noisy != y[:n]
    tx = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    ty = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))
    cfg = {
        "cg": Config(type="cg", cg_iterations=5, cg_alpha=1.0, unroll_steps=50),
        "neumann": Config(type="neumann", neumann_iterations=5, neumann_alpha=0.25, unroll_steps=50),
        "darts": Config(type="darts", unroll_steps=50),
        "sama": Config(type="sama", unroll_steps=50),
    }[args.algo]
    weights, linear = SampleWeights(n), torch.nn.Linear(d, C, bias=False)
    outer = Outer(name="outer", module=weights, optimizer=torch.optim.Adam(weights.parameters(), lr=0.1),
                  train_data_loader=[(tx(x[n:]), ty(y[n:]))], config=Config())
    inner = Inner(name="inner", module=linear, optimizer=torch.optim.SGD(linear.parameters(), lr=0.5),
                  train_data_loader=[(tx(x[:n]), ty(y_noisy))], config=cfg)
    if args.analytic:
        from betty_amd.hypergradient.structured import WeightedSoftmaxRegression

        inner.hypergradient_structure = lambda prev: WeightedSoftmaxRegression(inner, prev, linear.weight, weight_fn=lambda: prev(), reg=REG)
    engine = Engine(config=EngineConfig(train_iters=args.iters), problems=[outer, inner],
                    dependencies={"u2l": {outer: [inner]}, "l2u": {inner: [outer]}})
    engine.run()
    val = outer.training_step(outer.cur_batch).item()
    a = torch.sigmoid(weights.theta.detach()).cpu().numpy()
    print(f"algo={args.algo} analytic={args.analytic}  final validation loss {val:.4f}")
    print(f"mean weight of the {int(flipped.sum())} mislabelled samples {a[flipped].mean():.3f}, of the {int((~flipped).sum())} clean ones {a[~flipped].mean():.3f}")


if __name__ == "__main__":
    main()

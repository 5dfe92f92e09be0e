#!/usr/bin/env python
"""Differentiable architecture search on one small cell (the structure of BASELINE cfg 5, written for this repository) with every layer of
its separable / dilated operations DECLARED, on synthetic images.

Inner problem: the weights of a supernet — a stem, `--cells` cells whose two edges each mix {skip, sep 3x3, sep 5x5, dil 3x3} with the
architecture's softmax weights, a classifier.  Upper problem: the architecture weights, trained through the implicit hypergradient
(Neumann series, K terms).  The inner training_step stays OPAQUE — the Hessian-vector products are autograd's double backward, as in the
reference (neumann.py:62) — but the operations' layers, ReLU -> depthwise k x k -> 1 x 1 -> BatchNorm2d, are declared with
`betty_amd.nn.declare_layers_(net, depthwise=True)`: the depthwise convolution's share of every product is one bhg_dwconv_backward_vjp call
(csrc/bhg_dwconv.hip, at most four launches) instead of ATen's loop over the groups, the 1 x 1 convolution's three matrix products, and
batch norm's one bhg_bn_backward_vjp call.

    python examples/darts_cell_declared.py --k 3 --iters 20 [--undeclared]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betty_amd import Config  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.engine import Engine, EngineConfig  # noqa: E402
from betty_amd.problems import ImplicitProblem  # noqa: E402

OPS = ("skip", "sep3", "sep5", "dil3")


def stage(C, k, pad, dil=1):
    return [nn.ReLU(), nn.Conv2d(C, C, k, padding=pad, dilation=dil, groups=C, bias=False), nn.Conv2d(C, C, 1, bias=False), nn.BatchNorm2d(C)]


def operation(name, C):
    if name == "skip":
        return nn.Identity()
    if name == "dil3":
        return nn.Sequential(*stage(C, 3, 2, dil=2))
    k = int(name[-1])
    return nn.Sequential(*stage(C, k, k // 2), *stage(C, k, k // 2))   # a separable operation applies its stage twice


class Edge(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.ops = nn.ModuleList([operation(name, C) for name in OPS])

    def forward(self, x, weights):
        return sum(w * op(x) for w, op in zip(weights, self.ops))


class Cell(nn.Module):
    """Two intermediate nodes: node 1 = edge(input), node 2 = edge(input) + edge(node 1); the cell's output is their mean."""

    def __init__(self, C):
        super().__init__()
        self.edges = nn.ModuleList([Edge(C) for _ in range(3)])

    def forward(self, x, alphas):
        n1 = self.edges[0](x, alphas[0])
        n2 = self.edges[1](x, alphas[1]) + self.edges[2](n1, alphas[2])
        return 0.5 * (n1 + n2)


class Supernet(nn.Module):
    def __init__(self, C=16, cells=2, classes=10):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, C, 3, padding=1, bias=False), nn.BatchNorm2d(C))
        self.cells = nn.ModuleList([Cell(C) for _ in range(cells)])
        self.fc = nn.Linear(C, classes)

    def forward(self, x, alphas):
        h = self.stem(x)
        for cell in self.cells:
            h = cell(h, alphas)
        return self.fc(h.mean((2, 3)))


class Architecture(nn.Module):
    def __init__(self, edges=3):
        super().__init__()
        self.alpha = nn.Parameter(1e-3 * torch.randn(edges, len(OPS)))

    def forward(self):
        return F.softmax(self.alpha, dim=-1)


class Arch(ImplicitProblem):   # upper: the architecture, judged on validation batches with the current weights
    def training_step(self, batch):
        x, y = batch
        return F.cross_entropy(self.classifier.module(x, self.module()), y)


class Classifier(ImplicitProblem):   # inner: the supernet's weights on training batches
    def training_step(self, batch):
        x, y = batch
        return F.cross_entropy(self.module(x, self.arch.module()), y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--cells", type=int, default=2)
    ap.add_argument("--undeclared", action="store_true", help="leave every layer undeclared (the A/B arm)")
    args = ap.parse_args()
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    classes = 10
    proto = torch.randn(classes, 3, args.size, args.size, generator=g)

    def batch():
        y = torch.randint(0, classes, (args.batch,), generator=g)
        return proto[y] + 0.7 * torch.randn(args.batch, 3, args.size, args.size, generator=g), y

    train, valid = [batch() for _ in range(8)], [batch() for _ in range(8)]
    net, arch = Supernet(cells=args.cells, classes=classes), Architecture()
    declared = {} if args.undeclared else bnn.declare_layers_(net, depthwise=True)
    cfg = Config(type="neumann", unroll_steps=1, neumann_iterations=args.k, neumann_alpha=0.01)
    upper = Arch(name="arch", module=arch, optimizer=torch.optim.Adam(arch.parameters(), lr=3e-3), train_data_loader=valid,
                 config=Config(retain_graph=True))   # the upper loss depends on alpha directly AND through the weights: two passes over one graph
    inner = Classifier(name="classifier", module=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9), train_data_loader=train, config=cfg)
    engine = Engine(config=EngineConfig(train_iters=args.iters), problems=[upper, inner],
                    dependencies={"u2l": {upper: [inner]}, "l2u": {inner: [upper]}})
    calls0 = bnn.depthwise_conv_calls()
    t0 = time.perf_counter()
    engine.run()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    calls = {k: v - calls0[k] for k, v in bnn.depthwise_conv_calls().items()}
    finite = bool(torch.isfinite(arch.alpha).all())
    print(f"DARTS cell search, {args.cells} cells, declared {declared if declared else 'nothing'}, neumann K={args.k}: {upper.count} upper steps in {dt:.2f} s, "
          f"fused depthwise double-backward calls {calls['backward_vjp']}, alpha finite {finite}")
    print("architecture weights:", [[round(float(v), 3) for v in row] for row in arch().detach().cpu()])


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Measurements of the native path of the declared sample-weighted softmax regression (csrc/bhg_softreg_solve.hip: the row-weighted
solves and k_wsoftreg_mixed) -> profiles/wsoftreg_fused_solve.txt.

    python scripts/wsoftreg_solve_profile.py [--out profiles/wsoftreg_fused_solve.txt]

The comparator is the same commit's generic loop (K x (WeightedSoftmaxRegression.hvp in ATen + a recurrence kernel), then mixed_vjp in
ATen): the only other way this library solves the problem with the structure declared.  The driver (no --step) runs each measurement
as a child process of its own under `timeout`, checks every exit status and stops at the first step that fails: nothing more is started
on the GPU after a fault, an abort or a time limit.

  small  500 x 784 x 10, K = 5, cg    wall time of ONE hypergradient call through the front end with the declared structure,
  large  5000 x 512 x 10, K = 10, cg  stream-synchronised, median of 200 calls per path after 50 warm-up calls, the two paths
                                      ALTERNATING call by call; and the device time of k_wsoftreg_mixed alone (events around one
                                      launch, median of 200 after 20).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"small": (500, 784, 10, 5), "large": (5000, 512, 10, 10)}
STEP_TIMEOUT = 150


def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def step(which):
    _paths()
    import torch

    import zoo
    from betty_amd import Config
    from betty_amd import hypergradient as hg
    from betty_amd.backend import get_backend, softreg_solve_plan
    from betty_amd.hypergradient._common import WSOFTREG_SOLVE_STATS
    from betty_amd.hypergradient.structured import WeightedSoftmaxRegression

    class LoopOnly(WeightedSoftmaxRegression):   # the same provider with its own solver switched off: cg.py runs its loop
        def _fused_solve_ready(self, K, *state):
            return False

    n, d, C, K = SHAPES[which]
    dev = "cuda:0"
    g = torch.Generator().manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g).to(dev)
    y = torch.randint(0, C, (n,), generator=g).to(dev)
    W0 = (0.3 * torch.randn(C, d, generator=g) / d ** 0.5).to(dev)
    rhs = (0.01 * torch.randn(C, d, generator=g)).to(dev)
    theta0 = torch.randn(n, generator=g).to(dev)
    reg = 0.1

    class Sigmoid(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.theta = torch.nn.Parameter(theta0.clone())

        def forward(self):
            return torch.sigmoid(self.theta)

    def problem(cls):
        inner = torch.nn.Linear(d, C, bias=False).to(dev)
        inner.weight.data.copy_(W0)
        prev = zoo.StubProblem("upper", Sigmoid().to(dev), config=Config())

        def loss(self, batch):
            w = self.module.weight
            ce = torch.nn.functional.cross_entropy(self.module(batch[0]), batch[1], reduction="none")
            return (prev.fwd() * ce).mean() + 0.5 * reg * (w * w).sum()

        curr = zoo.StubProblem("inner", inner, config=Config(type="cg", cg_iterations=K, cg_alpha=1.0), loss_fn=loss, batch=(X, y))
        curr.hypergradient_structure = lambda p: cls(curr, p, inner.weight, weight_fn=lambda: p.fwd(), reg=reg)
        return curr, prev

    arms = {"fused": problem(WeightedSoftmaxRegression), "loop": problem(LoopOnly)}
    times = {k: [] for k in arms}
    for _ in range(50):
        for curr, prev in arms.values():
            hg.cg([rhs], curr, prev, False)
    torch.cuda.synchronize()
    before = dict(WSOFTREG_SOLVE_STATS)
    for _ in range(200):
        for name, (curr, prev) in arms.items():
            t0 = time.perf_counter()
            hg.cg([rhs], curr, prev, False)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6)
    took = {k: WSOFTREG_SOLVE_STATS[k] - before[k] for k in before}
    assert took == {"fused": 200, "loop": 200}, took
    out = {"step": which, "n": n, "d": d, "C": C, "K": K, "plan": softreg_solve_plan(n, d, C)}
    for name, ts in times.items():
        out[name] = {"median_us": statistics.median(ts), "min_us": min(ts), "p90_us": sorted(ts)[179]}
    # the mixed pass alone, device time
    be, c, direction = get_backend(), torch.empty(n, device=dev), rhs.reshape(-1).contiguous()
    us = []
    for _ in range(220):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        be.wsoftreg_mixed(X, W0, direction, y, c)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    assert bool(torch.isfinite(c).all())
    out["mixed"] = {"median_us": statistics.median(us[20:]), "min_us": min(us[20:])}
    print("RESULT " + json.dumps(out), flush=True)


def drive(args):
    results = {}
    for which in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", which]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:   # a fault, an abort or a time limit: start nothing more on the GPU
            sys.stderr.write(proc.stdout[-4000:] + proc.stderr[-4000:])
            sys.exit(f"step {which} ended with status {proc.returncode}: stopping")
        results[which] = [json.loads(ln[7:]) for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        print(json.dumps(results[which]), flush=True)
    lines = ["Native cg solve and mixed pass of the declared sample-weighted softmax regression (csrc/bhg_softreg_solve.hip) - one MI355X, one",
             "visit, against the same commit's generic loop (hvp in ATen + recurrence kernel, mixed_vjp in ATen), the two paths alternating",
             "inside one process (scripts/wsoftreg_solve_profile.py).  Wall time of one cg hypergradient call with the declared structure,",
             "stream-synchronised: median (min, 90th percentile) of 200 calls per path after 50 warm-up calls, microseconds.", ""]
    for i, which in enumerate(SHAPES):
        w = results[which]
        lines.append(f"{i + 1}. {w['n']} x {w['d']} x {w['C']}, K = {w['K']} (X = {4 * w['n'] * w['d'] / 2 ** 20:.1f} MiB)   plan: {w['plan']}")
        for name in ("loop", "fused"):
            r = w[name]
            lines.append(f"     {name:6s} {r['median_us']:8.1f} ({r['min_us']:.1f}, {r['p90_us']:.1f})")
        lines.append(f"     native path x {w['loop']['median_us'] / w['fused']['median_us']:.2f} of the loop")
        lines.append(f"     k_wsoftreg_mixed alone, device time (events around one launch, median (min) of 200): "
                     f"{w['mixed']['median_us']:.1f} ({w['mixed']['min_us']:.1f})")
        lines.append("")
    lines += ["Not measured: neumann through the front end, the strips form at n d in the hundreds of MiB (the sibling's figures in",
              "profiles/softreg_fused_solve.txt apply to the pass: the row weight adds one load per row), more than one GPU."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsoftreg_fused_solve.txt"))
    args = ap.parse_args()
    if args.step:
        step(args.step)
    else:
        drive(args)


if __name__ == "__main__":
    main()

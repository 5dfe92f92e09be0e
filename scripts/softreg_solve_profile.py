#!/usr/bin/env python
"""Measurements of the native softmax-regression solvers (csrc/bhg_softreg_solve.hip) -> profiles/softreg_fused_solve.txt.

    python scripts/softreg_solve_profile.py [--out profiles/softreg_fused_solve.txt]

The comparator is the same commit's generic loop (K x (SoftmaxRegressionL2.hvp in ATen + a recurrence kernel)): the only other way
this library solves the problem.  The driver (no --step) runs each measurement as a child process of its own under `timeout`, checks
every exit status and stops at the first step that fails: nothing more is started on the GPU after a fault, an abort or a time limit.

  wall   500 x 784 x 10, K = 5, cg: wall time of ONE hypergradient call through the front end with the declared structure,
         stream-synchronised, median of 200 calls per path after 50 warm-up calls, the two paths ALTERNATING call by call.
  large  65536 x 3072 x 10, K = 5 (X = 768 MiB, larger than the Infinity Cache): device time per ITERATION (events around a K = 5
         solve / 5, median of 9 solves per path after 2, alternating) for cg and neumann, and the fraction of 8 TB/s on the 4 n d
         bytes of X one product must move.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT = {"wall": 150, "large": 240}


def _paths():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def step_wall():
    _paths()
    import torch

    import zoo
    from betty_amd import Config
    from betty_amd import hypergradient as hg
    from betty_amd.backend import softreg_solve_plan
    from betty_amd.hypergradient._common import SOFTREG_SOLVE_STATS
    from betty_amd.hypergradient.structured import SoftmaxRegressionL2

    class LoopOnly(SoftmaxRegressionL2):   # the same provider with its own solver switched off: cg.py runs its loop
        def _fused_solve_ready(self, K, *state):
            return False

    n, d, C, K, dev = 500, 784, 10, 5, "cuda:0"
    g = torch.Generator().manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g).to(dev)
    y = torch.randint(0, C, (n,), generator=g).to(dev)
    W0 = (0.3 * torch.randn(C, d, generator=g) / 28.0).to(dev)
    rhs = (0.01 * torch.randn(C, d, generator=g)).to(dev)

    def problem(cls):
        inner = torch.nn.Linear(d, C, bias=False).to(dev)
        inner.weight.data.copy_(W0)
        upper = zoo.Vec(C * d, 1.0).to(dev)
        prev = zoo.StubProblem("upper", upper, config=Config())

        def loss(self, batch):
            w = self.module.weight
            return torch.nn.functional.cross_entropy(self.module(batch[0]), batch[1]) + 0.5 * (prev.fwd().reshape(w.shape) * w * w).sum()

        curr = zoo.StubProblem("inner", inner, config=Config(type="cg", cg_iterations=K, cg_alpha=1.0), loss_fn=loss, batch=(X, y))
        curr.hypergradient_structure = lambda p: cls(curr, p, inner.weight, lam_fn=lambda: p.fwd().reshape(C, d))
        return curr, prev

    arms = {"fused": problem(SoftmaxRegressionL2), "loop": problem(LoopOnly)}
    times = {k: [] for k in arms}
    for _ in range(50):
        for curr, prev in arms.values():
            hg.cg([rhs], curr, prev, False)
    torch.cuda.synchronize()
    before = dict(SOFTREG_SOLVE_STATS)
    for _ in range(200):
        for name, (curr, prev) in arms.items():
            t0 = time.perf_counter()
            hg.cg([rhs], curr, prev, False)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6)
    took = {k: SOFTREG_SOLVE_STATS[k] - before[k] for k in before}
    assert took == {"fused": 200, "loop": 200}, took
    out = {"step": "wall", "n": n, "d": d, "C": C, "K": K, "plan": softreg_solve_plan(n, d, C)}
    for name, ts in times.items():
        out[name] = {"median_us": statistics.median(ts), "min_us": min(ts), "p90_us": sorted(ts)[179]}
    print("RESULT " + json.dumps(out), flush=True)


def step_large():
    _paths()
    import torch

    from betty_amd.backend import SOFTREG_FORM_STRIPS, get_backend, softreg_solve_plan

    n, d, C, K, dev = 65536, 3072, 10, 5, "cuda:0"
    g = torch.Generator(device=dev).manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g, device=dev)
    W = 0.3 * torch.randn(C, d, generator=g, device=dev) / 55.0   # |logits| ~ 0.3: P is not one-hot
    lam = 0.5 + torch.rand(C, d, generator=g, device=dev)
    rhs = torch.randn(C, d, generator=g, device=dev)
    be = get_backend()
    out = {"step": "large", "n": n, "d": d, "C": C, "K": K, "plan": softreg_solve_plan(n, d, C, SOFTREG_FORM_STRIPS)}
    ws = be.softreg_solve_workspace(n, d, C, dev)
    sol, coeff = torch.empty(C * d, device=dev), torch.empty(C * d, device=dev)
    P = torch.softmax(X @ W.t(), dim=1)
    layout = be.layout([rhs])
    x, r, p = layout.state(3)
    xv, pv = layout.views(x, [rhs]), layout.views(p, [rhs])

    def product(V):   # SoftmaxRegressionL2.hvp
        PZ = P * (X @ V.t())
        U = (PZ - P * PZ.sum(dim=1, keepdim=True)) / n
        return U.t() @ X + lam * V

    def loop_cg():
        be.cg_init(layout, [rhs], x, r, p)
        for k in range(K):
            be.cg_step(layout, [product(pv[0])], x, r, p, 1.0, k, out_scale=-1.0 if k == K - 1 else 0.0)

    def loop_neumann():
        be.neumann_init(layout, [rhs], x, p)
        for k in range(K):
            be.neumann_step(layout, [product(xv[0])], x, p, 0.25, out_scale=-0.25 if k == K - 1 else 0.0)

    runs = {
        "cg": {"fused": lambda: be.softreg_cg_solve(X, W, lam, rhs, sol, coeff, ws, K, 1.0, -1.0, SOFTREG_FORM_STRIPS, 0), "loop": loop_cg},
        "neumann": {"fused": lambda: be.softreg_neumann_solve(X, W, lam, rhs, sol, coeff, ws, K, 0.25, -0.25, SOFTREG_FORM_STRIPS, 0),
                    "loop": loop_neumann},
    }
    for algo, arms in runs.items():
        ms = {k: [] for k in arms}
        for _ in range(11):
            for name, run in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b) * 1e3 / K)
        assert bool(torch.isfinite(sol).all()) and bool(torch.isfinite(x).all())
        out[algo] = {name: {"us_per_iter": statistics.median(v[2:]), "min_us_per_iter": min(v[2:]),
                            "fraction_of_8TBps_on_4nd": 4.0 * n * d / (statistics.median(v[2:]) * 1e-6) / 8e12} for name, v in ms.items()}
    print("RESULT " + json.dumps(out), flush=True)


def drive(args):
    results = {}
    for step in ("wall", "large"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:   # a fault, an abort or a time limit: start nothing more on the GPU
            sys.stderr.write(proc.stdout[-4000:] + proc.stderr[-4000:])
            sys.exit(f"step {step} ended with status {proc.returncode}: stopping")
        results[step] = [json.loads(ln[7:]) for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        print(json.dumps(results[step]), flush=True)
    w, big = results["wall"], results["large"]
    lines = ["Native cg / neumann solve of the declared softmax-regression structure (csrc/bhg_softreg_solve.hip) - one MI355X, one visit,",
             "against the same commit's generic loop, the two paths alternating inside one process (scripts/softreg_solve_profile.py).", "",
             f"1. {w['n']} x {w['d']} x {w['C']}, K = {w['K']}, cg: wall time of one hypergradient call with the declared structure, stream-synchronised,",
             "   median (min, 90th percentile) of 200 calls per path after 50 warm-up calls, microseconds:",
             f"     plan: {w['plan']}"]
    for name in ("loop", "fused"):
        r = w[name]
        lines.append(f"     {name:6s} {r['median_us']:8.1f} ({r['min_us']:.1f}, {r['p90_us']:.1f})")
    lines.append(f"     native solve x {w['loop']['median_us'] / w['fused']['median_us']:.2f} of the loop")
    lines += ["", f"2. {big['n']} x {big['d']} x {big['C']}, K = {big['K']} (X = {4 * big['n'] * big['d'] >> 20} MiB): device time per iteration (events around a whole solve / K;",
              "   median (min) of 9 solves per path), microseconds, and the fraction of 8 TB/s on the 4 n d bytes of X one product must move:",
              f"     plan: {big['plan']}"]
    for algo in ("cg", "neumann"):
        for name in ("loop", "fused"):
            r = big[algo][name]
            lines.append(f"     {algo:8s} {name:6s} {r['us_per_iter']:9.1f} ({r['min_us_per_iter']:.1f}) = {r['fraction_of_8TBps_on_4nd']:.3f} of 8 TB/s")
        lines.append(f"     {algo}: native solve x {big[algo]['loop']['us_per_iter'] / big[algo]['fused']['us_per_iter']:.2f} of the loop")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["wall", "large"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softreg_fused_solve.txt"))
    args = ap.parse_args()
    if args.step == "wall":
        step_wall()
    elif args.step == "large":
        step_large()
    else:
        drive(args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Measurements of the native logistic-regression solvers (csrc/bhg_logreg_solve.hip) -> profiles/logreg_fused_solve.txt.

    python scripts/logreg_solve_profile.py --parent-lib PATH/libbhg.so [--pairs 3] [--out profiles/logreg_fused_solve.txt]

The driver (no --step) runs every measurement as a child process of its own under `timeout`, parent and child arms alternating
(interleaved pairs), checks every exit status and stops at the first step that fails: nothing more is started on the GPU after
a fault, an abort or a time limit.  `--parent-lib`: a build of the PARENT commit's library; the `parent` arm loads it through BHG_LIB
(it lacks the new symbols: that arm drops them from the binding and keeps the declared path of the parent, K x (bhg_logreg_hvp + a
recurrence kernel), which is byte-for-byte the parent's device code).

  cfg1   BASELINE cfg 1 (500 x 100, K = 5), cg and neumann: wall time of ONE hypergradient call through the front end with the declared
         structure, stream-synchronised, median of 200 calls after 50 warm-up calls.
  large  65536 x 4096, K = 5 (X = 1 GiB, larger than the Infinity Cache): device time per ITERATION (events around a K = 5 solve / 5,
         median of 9 solves after 2) — strips form against the parent's bhg_logreg_hvp + bhg_cg_step / bhg_neumann_step launches,
         which read X twice per product (8 n d bytes).  Fraction of 8 TB/s on the 4 n d bytes the strips form must move.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bhg_logreg_solve_plan", "bhg_logreg_solve_ws_bytes", "bhg_logreg_cg_solve", "bhg_logreg_neumann_solve")
STEP_TIMEOUT = {"cfg1": 120, "large": 180}


def _setup(arm):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from betty_amd import _native
    from betty_amd.hypergradient.structured import LogisticRegressionL2

    if arm == "parent":
        import ctypes

        lib = ctypes.CDLL(_native.LIB_PATH)
        for name in NEW_SYMBOLS:   # the parent's library has none of them: bind what it has
            if not hasattr(lib, name):
                _native.SYMBOLS.pop(name, None)
        LogisticRegressionL2.fused_cg = LogisticRegressionL2.fused_neumann = None   # cg.py / neumann.py then run their loop
    return _native


def step_cfg1(arm):
    _native = _setup(arm)
    import torch

    import zoo
    from betty_amd import Config
    from betty_amd import hypergradient as hg
    from betty_amd.hypergradient._common import LOGREG_SOLVE_STATS
    from conftest import load_golden

    out = {"step": "cfg1", "arm": arm, "lib": _native.LIB_PATH}
    for name in ("logreg_cg5", "logreg_neumann5"):
        case = zoo.CASE_BY_NAME[name]
        inputs, _ = load_golden(case.family)
        curr, prev, vector = zoo.build_case(case, inputs, Config, device="cuda:0")
        zoo.attach_logreg_structure(curr)
        fn = hg.jvp_fn_mapping[case.algo]
        for _ in range(50):
            fn(vector, curr, prev, False)
        torch.cuda.synchronize()
        before = dict(LOGREG_SOLVE_STATS)
        times = []
        for _ in range(200):
            t0 = time.perf_counter()
            fn(vector, curr, prev, False)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6)
        took = {k: LOGREG_SOLVE_STATS[k] - before[k] for k in before}
        assert took == ({"fused": 200, "loop": 0} if arm == "child" else {"fused": 0, "loop": 0}), took
        out[name] = {"median_us": statistics.median(times), "min_us": min(times), "p90_us": sorted(times)[179]}
    print("RESULT " + json.dumps(out), flush=True)


def step_large(arm):
    _native = _setup(arm)
    import torch

    from betty_amd.backend import get_backend

    n, d, K = 65536, 4096, 5
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(n + d)
    X = torch.randn(n, d, generator=g, device=dev)
    w = 0.3 * torch.randn(d, generator=g, device=dev) / 64.0   # |x.w| ~ 0.3: s is not vanishingly small
    lam = 0.5 + torch.rand(d, generator=g, device=dev)
    rhs = torch.randn(d, generator=g, device=dev)
    be = get_backend()
    lib = be.lib
    stream = lambda: int(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    out = {"step": "large", "arm": arm, "n": n, "d": d, "K": K, "lib": _native.LIB_PATH}

    def timed(run, reps=11, drop=2):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) * 1e3 / K)
        return statistics.median(ms[drop:]), min(ms[drop:])

    if arm == "child":
        from betty_amd.backend import LOGREG_FORM_STRIPS, logreg_solve_plan

        out["plan"] = logreg_solve_plan(n, d, LOGREG_FORM_STRIPS)
        ws = be.logreg_solve_workspace(n, d, dev)
        sol, coeff = torch.empty(d, device=dev), torch.empty(d, device=dev)
        for algo, fn, step in (("cg", be.logreg_cg_solve, 1.0), ("neumann", be.logreg_neumann_solve, 0.5)):
            med, best = timed(lambda: fn(X, w, lam, rhs, sol, coeff, ws, K, step, -step, LOGREG_FORM_STRIPS, 0))
            assert bool(torch.isfinite(sol).all())
            out[algo] = {"us_per_iter": med, "min_us_per_iter": best, "fraction_of_8TBps_on_4nd": 4.0 * n * d / (med * 1e-6) / 8e12}
    else:
        s, hp = torch.empty(n, device=dev), torch.empty(d, device=dev)
        tmp = torch.empty(int(lib.bhg_logreg_tmp_floats(n, d)), device=dev)
        _native.check(lib.bhg_logreg_prepare(X.data_ptr(), w.data_ptr(), s.data_ptr(), n, d, stream()), "bhg_logreg_prepare")
        layout = be.layout([rhs])
        x, r, p = layout.state(3)

        def product(direction):
            _native.check(lib.bhg_logreg_hvp(X.data_ptr(), s.data_ptr(), lam.data_ptr(), direction.data_ptr(), hp.data_ptr(), tmp.data_ptr(),
                                             n, d, stream()), "bhg_logreg_hvp")

        def cg():
            be.cg_init(layout, [rhs], x, r, p)
            for k in range(K):
                product(p)
                be.cg_step(layout, [hp], x, r, p, 1.0, k, out_scale=-1.0 if k == K - 1 else 0.0)

        def neumann():
            be.neumann_init(layout, [rhs], x, p)
            for k in range(K):
                product(x)
                be.neumann_step(layout, [hp], x, p, 0.5, out_scale=-0.5 if k == K - 1 else 0.0)

        for algo, run in (("cg", cg), ("neumann", neumann)):
            med, best = timed(run)
            out[algo] = {"us_per_iter": med, "min_us_per_iter": best, "fraction_of_8TBps_on_8nd": 8.0 * n * d / (med * 1e-6) / 8e12}
    print("RESULT " + json.dumps(out), flush=True)


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return h.hexdigest()


def drive(args):
    child_lib = os.path.join(ROOT, "betty_amd", "csrc", "libbhg.so")
    lines = ["Native cg / neumann solve of the declared logistic-regression structure (csrc/bhg_logreg_solve.hip) - one MI355X, one visit,",
             "parent and child arms as alternating processes (scripts/logreg_solve_profile.py).",
             f"library: product libbhg.so sha256 {sha256(child_lib)}",
             f"parent commit's library (BHG_LIB): sha256 {sha256(args.parent_lib)}", ""]
    results = {"cfg1": [], "large": []}
    for step in ("cfg1", "large"):
        for pair in range(args.pairs):
            for arm in ("parent", "child"):
                env = dict(os.environ)
                env.pop("BHG_LIB", None)
                if arm == "parent":
                    env["BHG_LIB"] = os.path.abspath(args.parent_lib)
                cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--arm", arm]
                proc = subprocess.run(cmd, env=env, capture_output=True, text=True)
                if proc.returncode != 0:   # a fault, an abort or a time limit: start nothing more on the GPU
                    sys.stderr.write(proc.stdout[-4000:] + proc.stderr[-4000:])
                    sys.exit(f"step {step} arm {arm} pair {pair} ended with status {proc.returncode}: stopping")
                res = [json.loads(ln[7:]) for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
                res["pair"] = pair
                results[step].append(res)
                print(json.dumps(res), flush=True)
    lines.append("1. BASELINE cfg 1 (500 x 100, K = 5): wall time of one hypergradient call with the declared structure, stream-synchronised,")
    lines.append("   median (min, 90th percentile) of 200 calls after 50 warm-up calls, microseconds; one line per pair:")
    for name in ("logreg_cg5", "logreg_neumann5"):
        ratios = []
        for pair in range(args.pairs):
            pa = next(r for r in results["cfg1"] if r["pair"] == pair and r["arm"] == "parent")[name]
            ch = next(r for r in results["cfg1"] if r["pair"] == pair and r["arm"] == "child")[name]
            ratios.append(pa["median_us"] / ch["median_us"])
            lines.append(f"     {name:16s} parent loop {pa['median_us']:8.1f} ({pa['min_us']:.1f}, {pa['p90_us']:.1f})   "
                         f"native solve {ch['median_us']:8.1f} ({ch['min_us']:.1f}, {ch['p90_us']:.1f})   x {ratios[-1]:.2f}")
        lines.append(f"     {name}: native solve faster in {sum(r > 1 for r in ratios)} of {len(ratios)} pairs, x {min(ratios):.2f} - {max(ratios):.2f}")
    lines.append("")
    lines.append("2. 65536 x 4096, K = 5 (X = 1 GiB): device time per iteration (events around a whole K = 5 solve / 5; median (min) of 9 solves),")
    lines.append("   microseconds, and the fraction of 8 TB/s on the bytes of X each arm must move (parent 8 n d, strips form 4 n d); one line per pair:")
    plan = next(r for r in results["large"] if r["arm"] == "child")["plan"]
    lines.append(f"     plan: {plan}")
    for algo in ("cg", "neumann"):
        ratios = []
        for pair in range(args.pairs):
            pa = next(r for r in results["large"] if r["pair"] == pair and r["arm"] == "parent")[algo]
            ch = next(r for r in results["large"] if r["pair"] == pair and r["arm"] == "child")[algo]
            ratios.append(pa["us_per_iter"] / ch["us_per_iter"])
            lines.append(f"     {algo:8s} parent launches {pa['us_per_iter']:8.1f} ({pa['min_us_per_iter']:.1f}) = {pa['fraction_of_8TBps_on_8nd']:.3f}   "
                         f"strips {ch['us_per_iter']:8.1f} ({ch['min_us_per_iter']:.1f}) = {ch['fraction_of_8TBps_on_4nd']:.3f} of 8 TB/s   x {ratios[-1]:.2f}")
        lines.append(f"     {algo}: strips form faster in {sum(r > 1 for r in ratios)} of {len(ratios)} pairs, x {min(ratios):.2f} - {max(ratios):.2f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["cfg1", "large"])
    ap.add_argument("--arm", choices=["parent", "child"], default="child")
    ap.add_argument("--parent-lib")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logreg_fused_solve.txt"))
    args = ap.parse_args()
    if args.step == "cfg1":
        step_cfg1(args.arm)
    elif args.step == "large":
        step_large(args.arm)
    else:
        if not args.parent_lib or not os.path.exists(args.parent_lib):
            ap.error("--parent-lib: a build of the parent commit's libbhg.so is needed for the comparison")
        drive(args)


if __name__ == "__main__":
    main()

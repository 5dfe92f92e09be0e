"""The finite-difference cg solve next to the double-backward solve on the metric workload run OPAQUE (bench.build: the 10 M-parameter
MLP with a meta-weight-net, no declared structure), CG K = 20 on one MI355X.

  python scripts/fd_hvp_profile.py wall     five interleaved pairs (finite-difference solve, double-backward solve): ms per solve
  python scripts/fd_hvp_profile.py trace    two solves of each source after a warm-up, for `rocprofv3 --kernel-trace --stats -- python ...`
  python scripts/fd_hvp_profile.py stats FILE_kernel_stats.csv
                                            us per launch of the pair-form and one-table resident kernels in that trace and their
                                            fraction of 8 TB/s on 32 N and 28 N bytes
"""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def problems():
    import torch

    import bench

    dev = torch.device("cuda:0")
    out = {}
    for name in ("finite_difference", "double_backward"):
        curr, prev, vec = bench.build(dev, 0, K=20, algo="cg")
        if name == "finite_difference":
            curr.hypergradient_hvp = "finite_difference"
        out[name] = (curr, prev, vec)
    return out


def solve(prob):
    import torch

    from betty_amd import hypergradient as hg

    curr, prev, vec = prob
    out = hg.cg(vec, curr, prev, False)
    torch.cuda.synchronize()
    return out


def timed(prob):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solve(prob)
    return (time.perf_counter() - t0) * 1e3


def main():
    mode = sys.argv[1]
    if mode == "stats":
        import bench

        N = sum(a * b + b for a, b in zip(bench.SIZES[:-1], bench.SIZES[1:]))
        print(f"N = {N} elements")
        for row in csv.DictReader(open(sys.argv[2])):
            name = row["Name"]
            if "k_cg_resident" in name or "k_fd_perturb" in name or "k_cg_d" in name or "k_cg_resid" in name:
                us = float(row["AverageNs"]) / 1e3
                per = 32 if "HvpGradPair" in name else 28 if "k_cg_resident" in name else 12 if "k_fd_perturb" in name else 0
                frac = f"  {per} N bytes -> {per * N / (us * 1e-6) / PEAK:.3f} of 8 TB/s" if per else ""
                short = name.replace("bhg::(anonymous namespace)::", "").split("(")[0]
                print(f"{short:<60} calls {row['Calls']:>4}  avg {us:9.2f} us  min {float(row['MinNs']) / 1e3:9.2f}  max {float(row['MaxNs']) / 1e3:9.2f}{frac}")
        return
    import torch

    from betty_amd.backend import get_backend
    from betty_amd.hypergradient import _common

    probs = problems()
    for p in probs.values():   # warm-up: library handles, allocator, the residency census
        solve(p)
        solve(p)
    if mode == "trace":
        for p in probs.values():
            solve(p)
            solve(p)
    else:
        rows = []
        for i in range(5):
            a, b = timed(probs["finite_difference"]), timed(probs["double_backward"])
            rows.append((a, b))
            print(f"pair {i}: finite-difference solve {a:8.2f} ms | double-backward solve {b:8.2f} ms")
        fa, fb = sorted(r[0] for r in rows), sorted(r[1] for r in rows)
        print(f"median: finite-difference {fa[2]:.2f} ms (min {fa[0]:.2f}, max {fa[4]:.2f}) | double backward {fb[2]:.2f} ms (min {fb[0]:.2f}, max {fb[4]:.2f})")
        got, want = solve(probs["finite_difference"]), solve(probs["double_backward"])
        d = torch.cat([(u - w).reshape(-1) for u, w in zip(got, want)]).norm() / torch.cat([w.reshape(-1) for w in want]).norm()
        print(f"distance between the two solves' hypergradients: {float(d):.3e}   (this loss feeds ce.detach() to the upper network: DESIGN.md)")
    print("FD_HVP_STATS", _common.FD_HVP_STATS)
    get_backend().check_health()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What declaring the loss buys (betty_amd.nn.cross_entropy, csrc/bhg_cross_entropy.hip), measured on the GPU.  The comparator is always
THIS commit's undeclared F.cross_entropy, alternating with the declared call inside one process.

  (i)   per call of bhg_cross_entropy_backward_vjp (dz and dg wanted) on 16 x 8, 800 x 10, 4096 x 1000, 8192 x 32000, 2048 x 128256 and
        8 x 128256, for reduction "none" (per-row g) and "mean" (scalar g with denom): the median of --calls stream-synchronised calls,
        kernel launches (torch profiler), and bytes per second on the ALGORITHMIC bytes — lsm and a read once, dz written once, 12 bytes per
        element.  Beside it the same vector-Jacobian product by autograd on the undeclared function (ATen's decomposition), the median of
        --ref-calls, and its launches.
  (ii)  the plan's constants, each as a pair of neighbouring shapes on either side of the edge (the plan itself chooses the regime): the
        register-resident bound (C = 32768 held in registers against C = 32772 split, and 16384 / 8192 for the smaller instances), the
        few-rows threshold (159 rows of 32768 — split — against 160 — rows; 8 / 64 / 128 rows of 16384 — never split — against 16388 —
        split), in nanoseconds per 1000 elements so that neighbours compare.  (The runs that SET the two few-rows constants had them at
        64 rows / 8192 elements and at 256 rows / 16384 elements, and so measured both regimes at 64 / 128 / 256 x 32768 | 32772, at
        8 / 16 / 32 x 8192 | 8196 and at 255 | 256 x 32768: their tables are kept at the end of
        profiles/cross_entropy_double_backward.txt.)
  (iii) one double-backward Hessian-vector product of the inner loss of examples/lm_reweighting_declared.py (two blocks, width 64, 16 x 24
        tokens; its layers declared in both arms), the loss declared against not, at vocabulary 32 and 50304 (split rows): wall time and
        kernel launches.

    python scripts/cross_entropy_profile.py [--out profiles/cross_entropy_double_backward.txt] [--calls 100] [--ref-calls 8] [--reps 5] [--dry]

--dry prints the shape table with its byte counts and plans and stops (no GPU needed); every measurement needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from betty_amd import _native  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.backend import cross_entropy_plan  # noqa: E402

DEV = "cuda:0"
SHAPES = [(16, 8), (800, 10), (4096, 1000), (8192, 32000), (2048, 128256), (8, 128256)]   # (N, C)
EDGES = [("register bound, 8192 rows", [(8192, 8192), (8192, 16384), (8192, 32768), (8192, 32772)]),
         ("fewer rows than CUs, the longest resident row", [(128, 32768), (159, 32768), (160, 32768), (256, 32768)]),
         ("few rows around the shortest row that is split for it", [(n, c) for n in (8, 64, 128) for c in (16384, 16388)])]
PEAK_HBM = 8.0e12   # bytes per second (MI355X)


def _median_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.current_stream().synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def _count_kernels(fn):
    """(kernel launches of one call, the five kernel names launched most often with their counts)."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = sorted(((e.count, e.key) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA), reverse=True)
    return sum(c for c, _ in rows), rows[:5]


def _operands(N, C, reduction):
    g = torch.Generator(device=DEV).manual_seed(N + C)
    z, a = (torch.randn(N, C, generator=g, device=DEV) for _ in range(2))
    y = torch.randint(0, C, (N,), generator=g, device=DEV)
    up = torch.randn(N if reduction == "none" else (), generator=g, device=DEV)
    return z, a, y, up


def per_call(say, calls, ref_calls):
    say(f"(i) bhg_cross_entropy_backward_vjp per call (dz and dg wanted): median of {calls} stream-synchronised calls; the undeclared function's "
        f"double backward of the same cotangent: median of {ref_calls}; launches by the torch profiler")
    say(f"{'N x C':>14s} {'red.':>5s} {'regime':>6s} {'inst':>5s} {'wgs':>5s} {'declared us':>12s} {'launches':>8s} {'GB/s (alg.)':>12s} {'of 8 TB/s':>9s} "
        f"{'undeclared us':>14s} {'launches':>8s} {'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for N, C in SHAPES:
        for reduction in ("none", "mean"):
            z, a, y, up = _operands(N, C, reduction)
            zr, gr = z.clone().requires_grad_(True), up.clone().requires_grad_(True)
            (gz,) = torch.autograd.grad(F.cross_entropy(zr, y, reduction=reduction), zr, gr, create_graph=True)
            undeclared = lambda: torch.autograd.grad(gz, (zr, gr), a, retain_graph=True)   # noqa: E731
            lsm = torch.log_softmax(z, 1)
            denom = torch.tensor(float(N), device=DEV) if reduction == "mean" else None
            declared = lambda: bnn._ce_vjp_hip(lsm, y, up, a, denom, -100, (True, True))   # noqa: E731
            want, got = undeclared(), declared()
            diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, want))
            del want, got
            # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
            t_d1 = _median_ms(declared, calls // 2)
            t_u = _median_ms(undeclared, ref_calls)
            t_d2 = _median_ms(declared, calls - calls // 2)
            t_d = 0.5 * (t_d1 + t_d2)
            n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
            rate = 12 * N * C / (t_d * 1e-3)
            plan = cross_entropy_plan(N, C, reduction == "mean")
            say(f"{N:7d}x{C:6d} {reduction:>5s} {plan['regime']:>6s} {plan['vec']:2d}/{plan['inst']:<2d} {plan['wgs']:5d} {t_d * 1e3:12.1f} {n_d:8d} "
                f"{rate / 1e9:12.1f} {rate / PEAK_HBM:9.3f} {t_u * 1e3:14.1f} {n_u:8d} {t_u / t_d:7.1f} {diff:13.2e}")
            if t_d > t_u:
                slower.append((N, C, reduction))
            del gz, undeclared, declared, zr, z, a, lsm
            torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    return slower


def plan_edges(say, calls):
    say("")
    say(f"(ii) the plan's constants: neighbouring shapes on either side of each edge, per-row g, dz and dg wanted: median of {calls} "
        f"stream-synchronised calls each, three alternating rounds")
    for title, shapes in EDGES:
        say(f"  {title}")
        fns = {}
        for N, C in shapes:
            z, a, y, up = _operands(N, C, "none")
            lsm = torch.log_softmax(z, 1)
            del z
            fns[(N, C)] = lambda lsm=lsm, y=y, up=up, a=a: bnn._ce_vjp_hip(lsm, y, up, a, None, -100, (True, True))   # noqa: E731
        t = {s: [] for s in shapes}
        for _ in range(3):
            for s in shapes:
                t[s].append(_median_ms(fns[s], calls))
        for N, C in shapes:
            ms = statistics.median(t[(N, C)])
            plan = cross_entropy_plan(N, C)
            say(f"    {N:5d} x {C:6d}: {plan['regime']:>5s} inst {plan['inst']:3d} slices {plan['slices']:3d} wgs {plan['wgs']:5d}  {ms * 1e3:9.1f} us  "
                f"{ms * 1e6 / (N * C / 1000):8.2f} ns per 1000 elements  {12 * N * C / (ms * 1e-3) / PEAK_HBM:.3f} of 8 TB/s at 12 B per element")
        del fns
        torch.cuda.empty_cache()


def language_model(say, reps):
    import lm_reweighting_declared as ex

    say("")
    say(f"(iii) one double-backward Hessian-vector product of the inner loss of examples/lm_reweighting_declared.py (two blocks, width 64, 16 x 24 "
        f"tokens; RMS norms, attention and SwiGLU declared in both arms): median wall ms of {reps} (three alternating rounds), kernel launches")
    for vocab in (32, 50304):
        row = {}
        for form in ("undeclared", "declared"):
            torch.manual_seed(0)
            ex.DECLARED[0] = True
            net, mwn = ex.LM(vocab=vocab).to(DEV), ex.MWN().to(DEV)
            bnn.declare_layers_(net, rmsnorm=True)
            g = torch.Generator().manual_seed(0)
            x, y = (t.to(DEV) for t in ex.make_batch(g, vocab, 16, 24, 0.5))
            params = list(net.parameters())
            vec = [torch.randn(t.shape, generator=g).to(DEV) for t in params]
            logits = net(x)
            if form == "declared":
                with bnn.declared_cross_entropy():
                    ce = F.cross_entropy(logits, y.flatten(), reduction="none")
            else:
                ce = F.cross_entropy(logits, y.flatten(), reduction="none")
            loss = torch.mean(mwn(ce.detach().reshape(-1, 1)).reshape(-1) * ce)
            grads = torch.autograd.grad(loss, params, create_graph=True)
            hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
            c0 = bnn.declared_cross_entropy_calls()["backward_vjp"]
            product = torch.cat([t.reshape(-1) for t in hvp()]).double().cpu()
            row[form] = (hvp, bnn.declared_cross_entropy_calls()["backward_vjp"] - c0, product)
        t = {"undeclared": [], "declared": []}
        for _ in range(3):                      # alternate
            for form in t:
                t[form].append(_median_ms(row[form][0], reps))
        n = {form: _count_kernels(row[form][0]) for form in t}
        tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
        plan = cross_entropy_plan(16 * 24, vocab)
        say(f"  vocabulary {vocab:6d} (loss over 384 x {vocab}: {plan['regime']}): undeclared {tu:8.3f} ms, {n['undeclared'][0]:5d} launches | declared "
            f"({row['declared'][1]} fused call per product) {td:8.3f} ms, {n['declared'][0]:5d} launches | x{tu / td:.2f}")
        pu, pd = row["undeclared"][2], row["declared"][2]
        say(f"    declared against undeclared product: {float((pd - pu).norm() / pu.norm()):.2e} of the norm")
        del row
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--ref-calls", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.dry:
        for N, C in SHAPES + [s for _, shapes in EDGES for s in shapes]:
            say(f"{(N, C)}: {12 * N * C} algorithmic bytes; plan {cross_entropy_plan(N, C)}")
        return
    if not torch.cuda.is_available():
        sys.exit("cross_entropy_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/cross_entropy_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    per_call(say, args.calls, args.ref_calls)
    plan_edges(say, args.calls)
    language_model(say, args.reps)
    say("")
    say("not measured: rocprofv3 kernel times, both regimes on the SAME shape (the plan chooses; neighbours stand in), more than one GPU, HIP-graph replay")


if __name__ == "__main__":
    main()

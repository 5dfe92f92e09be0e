#!/usr/bin/env python
"""What declaring the depthwise convolutions buys (betty_amd.nn.DepthwiseConv2d, csrc/bhg_dwconv.hip), measured on the GPU.  The
comparator is always THIS commit's undeclared layer, alternating with the declared one inside one process.

  (i)   per call of bhg_dwconv_backward_vjp at the DARTS supernet's shapes — batch 64; C = 16 / 32 / 64 at 32^2 / 16^2 / 8^2; k = 3, 5;
        d = 1, 2; s = 1, 2 — the median of --calls stream-synchronised calls, and bytes per second on the ALGORITHMIC bytes of the three
        passes: dgy reads a, x and writes dgy; dx reads gy and writes dx; dw reads gy and a: 4 * (4 X + 3 O) bytes, X = N C H W,
        O = N C H_out W_out.  Beside it the same vector-Jacobian product by autograd on the undeclared layer (ATen's convolution double
        backward), the median of --ref-calls calls.
  (ii)  one double-backward Hessian-vector product of a `sep` block and of a `dil` block (ReLU -> depthwise -> 1 x 1 -> BatchNorm2d
        stages), all three declarations against none: kernel launches (torch profiler) and wall time.
  (iii) with --network, where oracle/_ref has the staged NAS models: one product of Network(16, 10, 8) at batch 64, undeclared double
        backward / all three declarations / one forward-over-reverse pass.

    python scripts/dwconv_profile.py [--out profiles/dwconv_double_backward.txt] [--calls 200] [--budget SECONDS] [--network | --only-network] [--fp64-truth] [--dry]

--dry prints the shape table with its byte counts and stops (no GPU needed); every measurement needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from betty_amd import _native  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402

DEV = "cuda:0"
BATCH = 64
LAYERS = [(16, 32), (32, 16), (64, 8)]


def out_extent(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def shapes():
    for C, HW in LAYERS:
        for k in (3, 5):
            for d in (1, 2):
                for s in (1, 2):
                    yield BATCH, C, HW, HW, k, s, d * (k - 1) // 2, d


def algorithmic_bytes(N, C, H, W, k, s, p, d):
    X, O = N * C * H * W, N * C * out_extent(H, k, s, p, d) * out_extent(W, k, s, p, d)
    return 4 * (4 * X + 3 * O)


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


def per_call(say, calls, ref_calls, budget_s):
    t_start = time.perf_counter()
    say(f"(i) bhg_dwconv_backward_vjp per call, batch {BATCH}: median of {calls} stream-synchronised calls; the undeclared layer's double "
        f"backward of the same (a, b): median of {ref_calls}")
    say(f"{'C x H x W':>12s} {'k':>2s} {'s':>2s} {'d':>2s} {'declared us':>12s} {'GB/s (alg.)':>12s} {'undeclared us':>14s} {'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for N, C, H, W, k, s, p, d in shapes():
        if time.perf_counter() - t_start > budget_s:
            say(f"{C:4d}x{H:3d}x{W:3d} {k:2d} {s:2d} {d:2d}  not measured (--budget {budget_s:.0f} s used up)")
            continue
        g = torch.Generator().manual_seed(C * 100 + k * 10 + s * 2 + d)
        x, a = (torch.randn(N, C, H, W, generator=g).to(DEV) for _ in range(2))
        w, b = (torch.randn(C, 1, k, k, generator=g).to(DEV) for _ in range(2))
        gy = torch.randn(N, C, out_extent(H, k, s, p, d), out_extent(W, k, s, p, d), generator=g).to(DEV)
        xr, wr, gyr = (t.clone().requires_grad_(True) for t in (x, w, gy))
        gx, gw = torch.autograd.grad(F.conv2d(xr, wr, None, s, p, d, C), (xr, wr), gyr, create_graph=True)
        undeclared = lambda: torch.autograd.grad((gx, gw), (xr, wr, gyr), (a, b), retain_graph=True)   # noqa: E731
        declared = lambda: bnn._dw_vjp_hip(x, w, gy, a, b, s, p, d)   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, want))
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d2 = _median_ms(declared, calls - calls // 2)
        t_d = 0.5 * (t_d1 + t_d2)
        gbs = algorithmic_bytes(N, C, H, W, k, s, p, d) / (t_d * 1e-3) / 1e9
        say(f"{C:4d}x{H:3d}x{W:3d} {k:2d} {s:2d} {d:2d} {t_d * 1e3:12.1f} {gbs:12.1f} {t_u * 1e3:14.1f} {t_u / t_d:7.1f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((C, H, k, s, d))
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    return slower


def _stage(C, k, stride, pad, dil=1):
    return [nn.ReLU(), nn.Conv2d(C, C, k, stride=stride, padding=pad, dilation=dil, groups=C, bias=False), nn.Conv2d(C, C, 1, bias=False),
            nn.BatchNorm2d(C)]


def _block(kind, C):
    if kind == "sep":     # a separable operation applies its stage twice (both at stride 1 here)
        return nn.Sequential(*_stage(C, 3, 1, 1), *_stage(C, 3, 1, 1))
    return nn.Sequential(*_stage(C, 3, 1, 2, dil=2))


def _count_kernels(fn):
    """(kernel launches of one call, the five kernel names launched most often with their counts)."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = sorted(((e.count, e.key) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA), reverse=True)
    return sum(c for c, _ in rows), rows[:5]


def blocks(say, reps):
    say("")
    say(f"(ii) one double-backward Hessian-vector product of a block at batch {BATCH}, C = 16, 32 x 32: median wall ms of {reps}, kernel launches")
    for kind in ("sep", "dil"):
        row = {}
        for declared in (False, True):
            torch.manual_seed(0)
            net = _block(kind, 16).to(DEV)
            if declared:
                bnn.declare_layers_(net, depthwise=True)
            x = torch.randn(BATCH, 16, 32, 32, device=DEV)
            params = list(net.parameters())
            vec = [torch.randn_like(t) for t in params]
            grads = torch.autograd.grad((net(x) ** 2).mean(), params, create_graph=True)
            hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
            row[declared] = (hvp, [t.clone() for t in hvp()])
        rel = float(torch.cat([(u - v).reshape(-1) for u, v in zip(row[True][1], row[False][1])]).norm() / torch.cat([v.reshape(-1) for v in row[False][1]]).norm())
        t = {True: [], False: []}
        for _ in range(3):                      # alternate
            for declared in (False, True):
                t[declared].append(_median_ms(row[declared][0], reps))
        n = {declared: _count_kernels(row[declared][0]) for declared in (False, True)}
        say(f"  {kind}: undeclared {statistics.median(t[False]):8.3f} ms, {n[False][0]:6d} launches | declared {statistics.median(t[True]):8.3f} ms, "
            f"{n[True][0]:5d} launches | x{statistics.median(t[False]) / statistics.median(t[True]):.2f} | rel diff {rel:.2e}")
        for count, name in n[True][1]:
            say(f"      declared, launched most often: {count:4d} x {name[:110]}")


def network(say, fp64_truth=False):
    import zoo
    from betty_amd import Config

    say("")
    if zoo.nas_dir() is None:
        say("(iii) Network(16, 10, 8): the staged NAS models are not here (oracle/_ref): not measured")
        return
    say(f"(iii) one Hessian-vector product of Network(16, 10, 8) at batch {zoo.CFG5_BATCH}: wall seconds (second of two; the first warms up)")
    products = {}
    forms = (("undeclared double backward", False), ("batch norm + pointwise + depthwise declared", True),
             ("depthwise declared alone", "depthwise"), ("batch norm + pointwise declared alone", "others"))
    if fp64_truth:
        forms += (("the same problem in float64, undeclared", "fp64"),)
    for label, declare in forms:
        curr, prev, vector = zoo.cfg5_as_named_case(Config, DEV, dtype=torch.float64 if declare == "fp64" else torch.float32)
        counts = {}
        if declare is True:
            counts = bnn.declare_layers_(curr.module, depthwise=True)
        elif declare == "depthwise":
            counts = {"depthwise_conv": bnn.declare_depthwise_convs_(curr.module)}
        elif declare == "others":
            counts = bnn.declare_layers_(curr.module)
        params = curr.trainable_parameters()
        grads = torch.autograd.grad(curr.training_step_exec(curr.cur_batch), params, create_graph=True)
        secs = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv = torch.autograd.grad(grads, params, grad_outputs=vector, retain_graph=True)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        products[declare] = torch.cat([t.reshape(-1) for t in hv]).double().cpu()
        say(f"  {label}: {secs[1]:.3f} s (first {secs[0]:.3f} s) {counts if counts else ''}")
        del grads, hv
    for label, declare in forms[1:]:
        say(f"  {label}: {float((products[declare] - products[False]).norm() / products[False].norm()):.2e} of the norm from the undeclared product")
    if fp64_truth:
        for label, declare in forms[:-1]:
            say(f"  {label}: {float((products[declare] - products['fp64']).norm() / products['fp64'].norm()):.2e} of the norm from the float64 product")
    from betty_amd.hypergradient import _common

    curr, prev, vector = zoo.cfg5_as_named_case(Config, DEV)
    curr.hypergradient_hvp, curr.hypergradient_hvp_ack_batchnorm = "forward_over_reverse", True
    hvp = _common.ForwardOverReverseHVP(curr, prev)
    secs = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hvp(vector)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    if hvp.fallback is not None:
        say("  (the forward-over-reverse pass fell back to the double backward)")
    say(f"  one forward-over-reverse pass: {secs[1]:.3f} s (first {secs[0]:.3f} s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--ref-calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=float("inf"),
                    help="seconds part (i) may take before the remaining shapes are reported as not measured (default: every shape is measured)")
    ap.add_argument("--network", action="store_true", help="also part (iii)")
    ap.add_argument("--only-network", action="store_true", help="part (iii) alone")
    ap.add_argument("--fp64-truth", action="store_true", help="part (iii): also the undeclared product of the same problem in float64, and every form's distance from it")
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
        for sh in shapes():
            say(f"{sh}: {algorithmic_bytes(*sh)} algorithmic bytes")
        return
    if not torch.cuda.is_available():
        sys.exit("dwconv_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/dwconv_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}; "
        f"MIOpen {'on' if torch.backends.cudnn.enabled else 'off'}")
    if not args.only_network:
        per_call(say, args.calls, args.ref_calls, args.budget)
        blocks(say, args.reps)
    if args.network or args.only_network:
        network(say, args.fp64_truth)


if __name__ == "__main__":
    main()

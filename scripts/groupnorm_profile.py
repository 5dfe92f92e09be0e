#!/usr/bin/env python
"""What declaring the group norms buys (betty_amd.nn.FusedGroupNorm, csrc/bhg_groupnorm.hip), measured on the GPU.  The comparator is
always THIS commit's undeclared nn.GroupNorm, alternating with the declared one inside one process.

  (i)   per call of bhg_groupnorm_backward_vjp at GN(32) on 64 x 64 x 32 x 32, 64 x 128 x 16 x 16, 64 x 256 x 8 x 8, 32 x 256 x 56 x 56 (the
        streamed regime: rows of 25088 elements; 514 MB of operands, past the Infinity Cache), 256 x 256 x 32 x 32 (resident rows of 8192;
        1.3 GB, past the Infinity Cache) and the instance-norm form G = C on 64 x 64 x 32 x 32: the median of --calls stream-synchronised
        calls, kernel launches (torch profiler), and bytes per second on the ALGORITHMIC bytes — resident: x, gy, a read once, dx, dgy
        written once, 20 bytes per element; streamed: x, gy, a read twice, 32 bytes per element.  Beside it the same vector-Jacobian
        product by autograd on the undeclared layer (ATen's decomposition), the median of --ref-calls.
  (ii)  the first backward under create_graph=True of one layer (64 x 64 x 32 x 32, G = 32), declared (native_group_norm_backward, one
        autograd.Function node) against undeclared (infinitely_differentiable_native_group_norm_backward): that path changes too.
  (iii) one double-backward Hessian-vector product of a small GroupNorm ResNet (a 3 x 3 stem and three stages of two basic blocks, widths
        32 / 64 / 128, GN(8), 32 samples of 3 x 32 x 32), 13 group norms declared against none: wall time, kernel launches, and the
        distance of each from the same problem's float64 product.

    python scripts/groupnorm_profile.py [--out profiles/groupnorm_double_backward.txt] [--calls 100] [--ref-calls 8] [--reps 5] [--dry]

--dry prints the shape table with its byte counts and plans and stops (no GPU needed); every measurement needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from betty_amd import _native  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.backend import groupnorm_plan  # noqa: E402

DEV = "cuda:0"
# (N, C, G, H, W)
SHAPES = [(64, 64, 32, 32, 32), (64, 128, 32, 16, 16), (64, 256, 32, 8, 8), (32, 256, 32, 56, 56), (256, 256, 32, 32, 32), (64, 64, 64, 32, 32)]
PEAK_HBM = 8.0e12   # bytes per second (MI355X)


def algorithmic_bytes(N, C, G, H, W):
    per_element = 32 if groupnorm_plan(N, C, H * W, G)["regime"] == "streamed" else 20
    return per_element * N * C * H * W


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


def per_call(say, calls, ref_calls):
    say(f"(i) bhg_groupnorm_backward_vjp per call (a, b, c all given): median of {calls} stream-synchronised calls; the undeclared layer's "
        f"double backward of the same cotangents: median of {ref_calls}; launches by the torch profiler")
    say(f"{'N x C x H x W, G':>24s} {'regime':>9s} {'D':>6s} {'grid':>6s} {'declared us':>12s} {'launches':>8s} {'GB/s (alg.)':>12s} {'of 8 TB/s':>9s} "
        f"{'undeclared us':>14s} {'launches':>8s} {'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for N, C, G, H, W in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(N + C + H)
        x, gy, a = (torch.randn(N, C, H, W, generator=g, device=DEV) for _ in range(3))
        gamma, beta, b, c = (torch.randn(C, generator=g, device=DEV) for _ in range(4))
        _, mean, rstd = torch.native_group_norm(x, gamma, beta, N, C, H * W, G, 1e-5)
        xr, gyr, gr, br = (t.clone().requires_grad_(True) for t in (x, gy, gamma, beta))
        firsts = torch.autograd.grad(F.group_norm(xr, G, gr, br, 1e-5), (xr, gr, br), gyr, create_graph=True)
        undeclared = lambda: torch.autograd.grad(firsts, (xr, gyr, gr), (a, b, c), retain_graph=True)   # noqa: E731
        declared = lambda: bnn._gn_vjp_hip(x, gy, a, gamma, mean, rstd, b, c, G)   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, want))
        del want, got
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d2 = _median_ms(declared, calls - calls // 2)
        t_d = 0.5 * (t_d1 + t_d2)
        n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
        rate = algorithmic_bytes(N, C, G, H, W) / (t_d * 1e-3)
        plan = groupnorm_plan(N, C, H * W, G)
        say(f"{N:5d}x{C:4d}x{H:3d}x{W:3d}, G={G:3d} {plan['regime']:>9s} {plan['D']:6d} {plan['grid']:6d} {t_d * 1e3:12.1f} {n_d:8d} {rate / 1e9:12.1f} "
            f"{rate / PEAK_HBM:9.3f} {t_u * 1e3:14.1f} {n_u:8d} {t_u / t_d:7.1f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((N, C, G, H, W))
        del firsts, undeclared, declared, xr, gyr, x, gy, a
        torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    return slower


def first_backward(say, calls):
    N, C, G, H, W = SHAPES[0]
    say("")
    say(f"(ii) the first backward under create_graph=True of one layer, {N} x {C} x {H} x {W}, G = {G} (forward outside the timed region): median of "
        f"{calls} stream-synchronised calls (three alternating rounds), kernel launches")
    g = torch.Generator(device=DEV).manual_seed(1)
    x, gy = (torch.randn(N, C, H, W, generator=g, device=DEV) for _ in range(2))
    fns = {}
    for form, cls in (("undeclared", nn.GroupNorm), ("declared", bnn.FusedGroupNorm)):
        layer = cls(G, C).to(DEV)
        xr = x.clone().requires_grad_(True)
        y = layer(xr)
        fns[form] = lambda y=y, xr=xr, layer=layer: torch.autograd.grad(y, (xr, layer.weight, layer.bias), gy, create_graph=True, retain_graph=True)   # noqa: E731
    t = {form: [] for form in fns}
    for _ in range(3):
        for form in t:
            t[form].append(_median_ms(fns[form], calls))
    n = {form: _count_kernels(fns[form])[0] for form in t}
    tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
    say(f"  undeclared {tu * 1e3:9.1f} us, {n['undeclared']:4d} launches | declared {td * 1e3:9.1f} us, {n['declared']:4d} launches | x{tu / td:.2f}")
    return td > tu


class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.c1, self.n1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.GroupNorm(8, cout)
        self.c2, self.n2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.GroupNorm(8, cout)
        self.short = None if stride == 1 and cin == cout else nn.Conv2d(cin, cout, 1, stride, bias=False)

    def forward(self, x):
        h = self.n2(self.c2(F.relu(self.n1(self.c1(x)))))
        return F.relu(h + (x if self.short is None else self.short(x)))


class _ResNet(nn.Module):
    def __init__(self, classes=10):
        super().__init__()
        self.stem, self.norm = nn.Conv2d(3, 32, 3, 1, 1, bias=False), nn.GroupNorm(8, 32)
        self.blocks = nn.Sequential(_Block(32, 32, 1), _Block(32, 32, 1), _Block(32, 64, 2), _Block(64, 64, 1), _Block(64, 128, 2), _Block(128, 128, 1))
        self.head = nn.Linear(128, classes)

    def forward(self, x):
        h = self.blocks(F.relu(self.norm(self.stem(x))))
        return self.head(h.mean(dim=(2, 3)))


def resnet(say, reps):
    say("")
    say(f"(iii) one double-backward Hessian-vector product of a small GroupNorm ResNet (stem + 3 stages of 2 basic blocks, widths 32 / 64 / 128, "
        f"GN(8), 32 x 3 x 32 x 32): median wall ms of {reps} (three alternating rounds), kernel launches")
    row, product = {}, {}
    for form in ("undeclared", "declared", "float64"):
        torch.manual_seed(0)
        net = _ResNet().to(DEV)
        layers = bnn.fuse_groupnorm_(net) if form == "declared" else 0
        dtype = torch.float64 if form == "float64" else torch.float32
        net = net.to(dtype)
        g = torch.Generator().manual_seed(0)
        x, y = torch.randn(32, 3, 32, 32, generator=g).to(DEV, dtype), torch.randint(0, 10, (32,), generator=g).to(DEV)
        params = list(net.parameters())
        vec = [torch.randn(t.shape, generator=g).to(DEV, dtype) for t in params]
        grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=True)
        hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
        c0 = bnn.fused_groupnorm_calls()["backward_vjp"]
        product[form] = torch.cat([t.reshape(-1) for t in hvp()]).double().cpu()
        row[form] = (hvp, layers, bnn.fused_groupnorm_calls()["backward_vjp"] - c0)
    t = {"undeclared": [], "declared": []}
    for _ in range(3):                      # alternate
        for form in t:
            t[form].append(_median_ms(row[form][0], reps))
    n = {form: _count_kernels(row[form][0]) for form in t}
    tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
    say(f"  undeclared {tu:8.3f} ms, {n['undeclared'][0]:6d} launches | declared ({row['declared'][1]} group norms, {row['declared'][2]} fused calls per "
        f"product) {td:8.3f} ms, {n['declared'][0]:5d} launches | x{tu / td:.2f}")
    truth = product["float64"]
    for form in ("undeclared", "declared"):
        say(f"  {form}: {float((product[form] - truth).norm() / truth.norm()):.2e} of the norm, {float((product[form] - truth).abs().max() / truth.abs().max()):.2e} "
            "of max|want| from the float64 product")
    for count, name in n["declared"][1]:
        say(f"      declared, launched most often: {count:4d} x {name[:110]}")


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
        for shape in SHAPES:
            N, C, G, H, W = shape
            say(f"{shape}: {algorithmic_bytes(*shape)} algorithmic bytes; plan {groupnorm_plan(N, C, H * W, G)}")
        return
    if not torch.cuda.is_available():
        sys.exit("groupnorm_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/groupnorm_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}; "
        f"MIOpen {'on' if torch.backends.cudnn.enabled else 'off'}")
    per_call(say, args.calls, args.ref_calls)
    first_backward(say, args.calls)
    resnet(say, args.reps)
    say("")
    say("not measured: rocprofv3 kernel times, whether the streamed regime's second round is served by the L2, more than one GPU, HIP-graph replay")


if __name__ == "__main__":
    main()

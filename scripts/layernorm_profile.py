#!/usr/bin/env python
"""What declaring the layer norms buys (betty_amd.nn.FusedLayerNorm, csrc/bhg_layernorm.hip), measured on the GPU.  The comparator is
always THIS commit's undeclared nn.LayerNorm, alternating with the declared one inside one process.

  (i)  per call of bhg_layernorm_backward_vjp at 800 x 768 (RoBERTa-base, 16 x 50 tokens), 8192 x 1024 and 65536 x 4096 (past the
       Infinity Cache): the median of --calls stream-synchronised calls, kernel launches (torch profiler), and bytes per second on the
       ALGORITHMIC bytes — x, gy, a read once, dx, dgy written once: 20 bytes per element.  Beside it the same vector-Jacobian product by
       autograd on the undeclared layer (ATen's decomposed double backward of native_layer_norm_backward), the median of --ref-calls.
  (ii) one double-backward Hessian-vector product of a two-layer nn.TransformerEncoder (d_model 768, 12 heads, 16 x 50 tokens, the math
       attention path: the fused attention kernels have no double backward), four layer norms declared against none: wall time, kernel
       launches, and the distance of each from the same problem's float64 product.

    python scripts/layernorm_profile.py [--out profiles/layernorm_double_backward.txt] [--calls 200] [--ref-calls 10] [--reps 5] [--dry]

--dry prints the shape table with its byte counts and stops (no GPU needed); every measurement needs a GPU and fails without one."""
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
from betty_amd.backend import layernorm_plan  # noqa: E402

DEV = "cuda:0"
SHAPES = [(800, 768), (8192, 1024), (65536, 4096)]
PEAK_HBM = 8.0e12   # bytes per second (MI355X); bhg_bn_backward_vjp reaches 0.63-0.73 of it past the cache


def algorithmic_bytes(M, D):
    return 20 * M * D


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
    say(f"(i) bhg_layernorm_backward_vjp per call (a, b, c all given): median of {calls} stream-synchronised calls; the undeclared layer's "
        f"double backward of the same cotangents: median of {ref_calls}; launches by the torch profiler")
    say(f"{'M x D':>14s} {'slices':>6s} {'declared us':>12s} {'launches':>8s} {'GB/s (alg.)':>12s} {'of 8 TB/s':>9s} {'undeclared us':>14s} {'launches':>8s} "
        f"{'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for M, D in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(M + D)
        x, gy, a = (torch.randn(M, D, generator=g, device=DEV) for _ in range(3))
        gamma, beta, b, c = (torch.randn(D, generator=g, device=DEV) for _ in range(4))
        _, mean, rstd = torch.native_layer_norm(x, [D], gamma, beta, 1e-5)
        xr, gyr, gr, br = (t.clone().requires_grad_(True) for t in (x, gy, gamma, beta))
        firsts = torch.autograd.grad(F.layer_norm(xr, (D,), gr, br, 1e-5), (xr, gr, br), gyr, create_graph=True)
        undeclared = lambda: torch.autograd.grad(firsts, (xr, gyr, gr), (a, b, c), retain_graph=True)   # noqa: E731
        declared = lambda: bnn._ln_vjp_hip(x, gy, a, gamma, mean, rstd, b, c)   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, want))
        del want, got
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d2 = _median_ms(declared, calls - calls // 2)
        t_d = 0.5 * (t_d1 + t_d2)
        n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
        rate = algorithmic_bytes(M, D) / (t_d * 1e-3)
        say(f"{M:7d}x{D:5d} {layernorm_plan(M, D)['slices']:6d} {t_d * 1e3:12.1f} {n_d:8d} {rate / 1e9:12.1f} {rate / PEAK_HBM:9.3f} {t_u * 1e3:14.1f} {n_u:8d} "
            f"{t_u / t_d:7.1f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((M, D))
        del firsts, undeclared, declared, xr, gyr, x, gy, a
        torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    return slower


def encoder(say, reps):
    from torch.nn.attention import SDPBackend, sdpa_kernel

    say("")
    say(f"(ii) one double-backward Hessian-vector product of a two-layer nn.TransformerEncoder (d_model 768, 12 heads, ffn 3072, no dropout, "
        f"16 x 50 tokens, math attention): median wall ms of {reps} (three alternating rounds), kernel launches")
    row, product = {}, {}
    with sdpa_kernel(SDPBackend.MATH):
        for form in ("undeclared", "declared", "float64"):
            torch.manual_seed(0)
            layer = nn.TransformerEncoderLayer(768, 12, dim_feedforward=3072, dropout=0.0, batch_first=True)
            net = nn.TransformerEncoder(layer, 2, enable_nested_tensor=False).to(DEV)
            layers = bnn.fuse_layernorm_(net) if form == "declared" else 0
            dtype = torch.float64 if form == "float64" else torch.float32
            net = net.to(dtype)
            g = torch.Generator().manual_seed(0)
            x = torch.randn(16, 50, 768, generator=g).to(DEV, dtype)
            params = list(net.parameters())
            vec = [torch.randn(t.shape, generator=g).to(DEV, dtype) for t in params]
            grads = torch.autograd.grad((net(x) ** 2).mean(), params, create_graph=True)
            hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
            c0 = bnn.fused_layernorm_calls()["backward_vjp"]
            product[form] = torch.cat([t.reshape(-1) for t in hvp()]).double().cpu()
            row[form] = (hvp, layers, bnn.fused_layernorm_calls()["backward_vjp"] - c0)
        t = {"undeclared": [], "declared": []}
        for _ in range(3):                      # alternate
            for form in t:
                t[form].append(_median_ms(row[form][0], reps))
        n = {form: _count_kernels(row[form][0]) for form in t}
    tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
    say(f"  undeclared {tu:8.3f} ms, {n['undeclared'][0]:6d} launches | declared ({row['declared'][1]} layer norms, {row['declared'][2]} fused calls per "
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--ref-calls", type=int, default=10)
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
        for M, D in SHAPES:
            say(f"{M} x {D}: {algorithmic_bytes(M, D)} algorithmic bytes; plan {layernorm_plan(M, D)}")
        return
    if not torch.cuda.is_available():
        sys.exit("layernorm_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/layernorm_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}; "
        f"MIOpen {'on' if torch.backends.cudnn.enabled else 'off'}")
    per_call(say, args.calls, args.ref_calls)
    encoder(say, args.reps)


if __name__ == "__main__":
    main()

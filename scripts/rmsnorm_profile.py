#!/usr/bin/env python
"""What declaring the RMS norms buys (betty_amd.nn.FusedRMSNorm, csrc/bhg_rmsnorm.hip), measured on the GPU.  The comparator is always
THIS commit's undeclared nn.RMSNorm, alternating with the declared one inside one process.

  (i)   per call of bhg_rmsnorm_backward_vjp on 800 x 768, 2048 x 4096, 8192 x 4096, 65536 x 4096 (5.4 GB of operands, past the Infinity
        Cache), 4096 x 8192 and 64 x 128: the median of --calls stream-synchronised calls, kernel launches (torch profiler), and bytes per
        second on the ALGORITHMIC bytes — x, gy, a read once, dx, dgy written once, 20 bytes per element.  Beside it the same
        vector-Jacobian product by autograd on the undeclared layer (ATen's decomposition), the median of --ref-calls.
  (ii)  the first backward under create_graph=True of one layer (2048 x 4096), declared (_fused_rms_norm_backward, one autograd.Function
        node) against undeclared (infinitely_differentiable_native_rms_norm_backward): that path changes too.
  (iii) the slice bound: bhg_layernorm_backward_vjp (at most 64 workgroups in its row pass) called on the same buffers at 8192 x 1024 and
        65536 x 4096, alternating with bhg_rmsnorm_backward_vjp (as many workgroups as fill the chip).
  (iv)  one double-backward Hessian-vector product of a two-block LLaMA-style model (width 768, 12 heads, FFN 2048, 16 x 128 tokens, tiled
        causal attention and SwiGLU declared in both arms), its 5 RMS norms declared against none: wall time and kernel launches.

    python scripts/rmsnorm_profile.py [--out profiles/rmsnorm_double_backward.txt] [--calls 100] [--ref-calls 8] [--reps 5] [--dry]

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
from betty_amd.backend import layernorm_plan, rmsnorm_plan  # noqa: E402

DEV = "cuda:0"
SHAPES = [(800, 768), (2048, 4096), (8192, 4096), (65536, 4096), (4096, 8192), (64, 128)]   # (M, D)
BOUND_SHAPES = [(8192, 1024), (65536, 4096)]
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


def per_call(say, calls, ref_calls):
    say(f"(i) bhg_rmsnorm_backward_vjp per call (a and b given): median of {calls} stream-synchronised calls; the undeclared layer's double "
        f"backward of the same cotangents: median of {ref_calls}; launches by the torch profiler")
    say(f"{'M x D':>14s} {'inst':>5s} {'slices':>6s} {'declared us':>12s} {'launches':>8s} {'GB/s (alg.)':>12s} {'of 8 TB/s':>9s} "
        f"{'undeclared us':>14s} {'launches':>8s} {'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for M, D in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(M + D)
        x, gy, a = (torch.randn(M, D, generator=g, device=DEV) for _ in range(3))
        gamma, b = (torch.randn(D, generator=g, device=DEV) for _ in range(2))
        _, rstd = torch.ops.aten._fused_rms_norm(x, [D], gamma, 1e-6)
        xr, gyr, gr = (t.clone().requires_grad_(True) for t in (x, gy, gamma))
        firsts = torch.autograd.grad(F.rms_norm(xr, (D,), gr, 1e-6), (xr, gr), gyr, create_graph=True)
        undeclared = lambda: torch.autograd.grad(firsts, (xr, gyr, gr), (a, b), retain_graph=True)   # noqa: E731
        declared = lambda: bnn._rms_vjp_hip(x, gy, a, gamma, rstd, b)   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, want))
        del want, got
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d2 = _median_ms(declared, calls - calls // 2)
        t_d = 0.5 * (t_d1 + t_d2)
        n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
        rate = 20 * M * D / (t_d * 1e-3)
        plan = rmsnorm_plan(M, D)
        say(f"{M:7d}x{D:5d} {plan['vec']:2d}/{plan['inst']:<2d} {plan['slices']:6d} {t_d * 1e3:12.1f} {n_d:8d} {rate / 1e9:12.1f} {rate / PEAK_HBM:9.3f} "
            f"{t_u * 1e3:14.1f} {n_u:8d} {t_u / t_d:7.1f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((M, D))
        del firsts, undeclared, declared, xr, gyr, x, gy, a
        torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    return slower


def first_backward(say, calls):
    M, D = SHAPES[1]
    say("")
    say(f"(ii) the first backward under create_graph=True of one layer, {M} x {D} (forward outside the timed region): median of {calls} "
        f"stream-synchronised calls (three alternating rounds), kernel launches")
    g = torch.Generator(device=DEV).manual_seed(1)
    x, gy = (torch.randn(M, D, generator=g, device=DEV) for _ in range(2))
    fns = {}
    for form, cls in (("undeclared", nn.RMSNorm), ("declared", bnn.FusedRMSNorm)):
        layer = cls(D).to(DEV)
        xr = x.clone().requires_grad_(True)
        y = layer(xr)
        say(f"  {form}: the output's autograd node is {type(y.grad_fn).__name__}")
        fns[form] = lambda y=y, xr=xr, layer=layer: torch.autograd.grad(y, (xr, layer.weight), gy, create_graph=True, retain_graph=True)   # noqa: E731
    t = {form: [] for form in fns}
    for _ in range(3):
        for form in t:
            t[form].append(_median_ms(fns[form], calls))
    n = {form: _count_kernels(fns[form])[0] for form in t}
    tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
    say(f"  undeclared {tu * 1e3:9.1f} us, {n['undeclared']:4d} launches | declared {td * 1e3:9.1f} us, {n['declared']:4d} launches | x{tu / td:.2f}")


def slice_bound(say, calls):
    say("")
    say(f"(iii) the slice bound: bhg_layernorm_backward_vjp (row pass on at most 64 workgroups) and bhg_rmsnorm_backward_vjp on the same buffers, "
        f"all cotangents given: median of {calls} stream-synchronised calls each, three alternating rounds")
    lib = _native.load()
    for M, D in BOUND_SHAPES:
        g = torch.Generator(device=DEV).manual_seed(M + D)
        x, gy, a = (torch.randn(M, D, generator=g, device=DEV) for _ in range(3))
        gamma, b, c = (torch.randn(D, generator=g, device=DEV) for _ in range(3))
        mean, rstd = x.mean(dim=1), torch.rsqrt(x.var(dim=1, unbiased=False) + 1e-5)
        ln = lambda: bnn._ln_vjp_hip(x, gy, a, gamma, mean, rstd, b, c)   # noqa: E731
        rms = lambda: bnn._rms_vjp_hip(x, gy, a, gamma, rstd, b)   # noqa: E731
        t = {"layernorm": [], "rmsnorm": []}
        for _ in range(3):
            t["layernorm"].append(_median_ms(ln, calls))
            t["rmsnorm"].append(_median_ms(rms, calls))
        tl, tr = statistics.median(t["layernorm"]), statistics.median(t["rmsnorm"])
        say(f"  {M:6d} x {D:4d}: layer norm {tl * 1e3:9.1f} us ({layernorm_plan(M, D)['slices']} slices, {20 * M * D / (tl * 1e-3) / PEAK_HBM:.3f} of 8 TB/s) | "
            f"RMS norm {tr * 1e3:9.1f} us ({rmsnorm_plan(M, D)['slices']} slices, {20 * M * D / (tr * 1e-3) / PEAK_HBM:.3f} of 8 TB/s) | x{tl / tr:.2f}"
            + ("" if tr <= tl else "   <-- the RMS-norm kernel is SLOWER here"))
        del x, gy, a
        torch.cuda.empty_cache()
    del lib


class _LlamaBlock(nn.Module):
    def __init__(self, width, heads, ffn):
        super().__init__()
        self.heads = heads
        self.norm1, self.qkv, self.proj = nn.RMSNorm(width), nn.Linear(width, 3 * width, bias=False), nn.Linear(width, width, bias=False)
        self.norm2, self.gate, self.up = nn.RMSNorm(width), nn.Linear(width, ffn, bias=False), nn.Linear(width, ffn, bias=False)
        self.down = nn.Linear(ffn, width, bias=False)

    def forward(self, x):
        B, T, W = x.shape
        q, k, v = (t.reshape(B, T, self.heads, W // self.heads).transpose(1, 2) for t in self.qkv(self.norm1(x)).chunk(3, dim=-1))
        h = x + self.proj(F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, W))
        n = self.norm2(h)
        return h + self.down(bnn.gated_activation(self.gate(n), self.up(n), "silu"))


class _Llama(nn.Module):
    def __init__(self, width=768, heads=12, ffn=2048, blocks=2, vocab=256):
        super().__init__()
        self.blocks = nn.Sequential(*[_LlamaBlock(width, heads, ffn) for _ in range(blocks)])
        self.norm, self.head = nn.RMSNorm(width), nn.Linear(width, vocab, bias=False)

    def forward(self, x):
        return self.head(self.norm(self.blocks(x)))


def llama(say, reps):
    say("")
    say(f"(iv) one double-backward Hessian-vector product of a two-block LLaMA-style model (width 768, 12 heads, FFN 2048, 16 x 128 tokens; tiled "
        f"causal attention and SwiGLU declared in both arms): median wall ms of {reps} (three alternating rounds), kernel launches")
    row = {}
    for form in ("undeclared", "declared"):
        torch.manual_seed(0)
        net = _Llama().to(DEV)
        layers = bnn.fuse_rmsnorm_(net) if form == "declared" else 0
        g = torch.Generator().manual_seed(0)
        x, y = torch.randn(16, 128, 768, generator=g).to(DEV), torch.randint(0, 256, (16 * 128,), generator=g).to(DEV)
        params = list(net.parameters())
        vec = [torch.randn(t.shape, generator=g).to(DEV) for t in params]
        with bnn.declared_attention(tiled=True):
            loss = F.cross_entropy(net(x).reshape(-1, 256), y)
        grads = torch.autograd.grad(loss, params, create_graph=True)
        hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
        c0 = bnn.fused_rmsnorm_calls()["backward_vjp"]
        product = torch.cat([t.reshape(-1) for t in hvp()]).double().cpu()
        row[form] = (hvp, layers, bnn.fused_rmsnorm_calls()["backward_vjp"] - c0, product)
    t = {"undeclared": [], "declared": []}
    for _ in range(3):                      # alternate
        for form in t:
            t[form].append(_median_ms(row[form][0], reps))
    n = {form: _count_kernels(row[form][0]) for form in t}
    tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
    say(f"  undeclared {tu:8.3f} ms, {n['undeclared'][0]:6d} launches | declared ({row['declared'][1]} RMS norms, {row['declared'][2]} fused calls per "
        f"product) {td:8.3f} ms, {n['declared'][0]:5d} launches | x{tu / td:.2f}")
    pu, pd = row["undeclared"][3], row["declared"][3]
    say(f"  declared against undeclared product: {float((pd - pu).norm() / pu.norm()):.2e} of the norm")
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
        for M, D in SHAPES + BOUND_SHAPES:
            say(f"{(M, D)}: {20 * M * D} algorithmic bytes; plan {rmsnorm_plan(M, D)}")
        return
    if not torch.cuda.is_available():
        sys.exit("rmsnorm_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/rmsnorm_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    per_call(say, args.calls, args.ref_calls)
    first_backward(say, args.calls)
    slice_bound(say, args.calls)
    llama(say, args.reps)
    say("")
    say("not measured: rocprofv3 kernel times, more than one GPU, HIP-graph replay")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What declaring the smooth activations buys (betty_amd.nn.gelu / silu / ... / gated_activation, csrc/bhg_activation.hip), measured on the
GPU.  The comparator is always THIS commit's undeclared torch function, alternating with the declared call inside one process.

  per_call        one call of bhg_act_backward_vjp / bhg_gated_act_backward_vjp: GELU and tanh-GELU at 800 x 3072 (RoBERTa-base's FFN at
                  cfg 4's batch) and 8192 x 4096, tanh and softplus at 100 x 2048 (cfg 2's width), SiLU at 64 x 64 x 32 x 32, sigmoid at
                  8192 x 4096, SwiGLU at 2048 x 11008, glu at 8192 x (2 x 2048): the median of --calls stream-synchronised calls, kernel
                  launches (torch profiler), bytes per second on the ALGORITHMIC bytes (x, gy, a read once, dx, dgy written once: 20 per
                  element; gated: 32) and their fraction of 8 TB/s.  Beside it the same vector-Jacobian product by autograd on the
                  undeclared function (ATen's decomposition), and every kind at one size, 8192 x 4096 — past the Infinity Cache —, to say
                  which kinds the transcendentals bound.
  kernel_time     the launches alone: every plain kind at 8192 x 4096, SwiGLU at 2048 x 11008 and glu at 8192 x (2 x 2048) through the C
                  ABI on preallocated outputs, GPU events around 20 back-to-back calls, the median of 5 rounds: no allocation and no
                  host synchronisation inside the timed region.
  first_backward  the first backward of SiLU under create_graph=True at 64 x 64 x 32 x 32, declared (silu_backward, one node) against
                  undeclared (ATen's decomposition).
  encoder         one double-backward Hessian-vector product of a two-layer nn.TransformerEncoder (d_model 768, 12 heads, ffn 3072, GELU,
                  no dropout, 16 x 50 tokens) with layer norm and attention declared, with and without the activations.

    python scripts/activation_profile.py PART [--out FILE] [--calls 100] [--ref-calls 20] [--reps 5]
    python scripts/activation_profile.py dry          # the shape table with its byte counts and plans: no GPU needed

Each part is one process, to be run under a time limit of its own, the next only if the one before ended well; --out appends."""
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
from betty_amd.backend import activation_plan, gated_activation_plan  # noqa: E402

DEV = "cuda:0"
PEAK_HBM = 8.0e12   # bytes per second (MI355X)
BIG = (8192, 4096)
# (label, form, kind, shape)
SHAPES = [("gelu", "plain", "gelu", (800, 3072)), ("gelu", "plain", "gelu", BIG), ("gelu_tanh", "plain", "gelu_tanh", (800, 3072)),
          ("gelu_tanh", "plain", "gelu_tanh", BIG), ("tanh", "plain", "tanh", (100, 2048)), ("softplus", "plain", "softplus", (100, 2048)),
          ("silu", "plain", "silu", (64, 64, 32, 32)), ("silu", "plain", "silu", BIG), ("tanh", "plain", "tanh", BIG),
          ("sigmoid", "plain", "sigmoid", BIG), ("softplus", "plain", "softplus", BIG), ("swiglu", "gated", "silu", (2048, 11008)),
          ("glu", "glu", "glu", (8192, 2 * 2048))]
TORCH_FN = {"gelu": F.gelu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "silu": F.silu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
            "softplus": F.softplus, "glu": F.glu}


def numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


def algorithmic_bytes(form, shape):
    return 20 * numel(shape) if form == "plain" else 32 * (numel(shape) // 2 if form == "glu" else numel(shape))


def plan_of(form, shape):
    if form == "plain":
        return activation_plan(numel(shape))
    H = shape[-1] // 2 if form == "glu" else shape[-1]
    return gated_activation_plan(numel(shape) // shape[-1], H)


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
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = sorted(((e.count, e.key) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA), reverse=True)
    return sum(c for c, _ in rows), rows[:5]


def per_call(say, calls, ref_calls):
    say(f"per call: median of {calls} stream-synchronised calls of the declared double backward; the undeclared function's double backward of "
        f"the same cotangents by autograd: median of {ref_calls}; launches by the torch profiler")
    say(f"{'kind':>10s} {'shape':>18s} {'grid':>5s} {'iters':>5s} {'declared us':>12s} {'launches':>8s} {'GB/s (alg.)':>12s} {'of 8 TB/s':>9s} "
        f"{'undeclared us':>14s} {'launches':>8s} {'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for label, form, kind, shape in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(numel(shape) % 1000 + len(label))
        if form == "gated":
            u, v, gy, au, av = (torch.randn(shape, generator=g, device=DEV) for _ in range(5))
            ur, vr, gyr = (t.clone().requires_grad_(True) for t in (u, v, gy))
            firsts = torch.autograd.grad(F.silu(ur) * vr, (ur, vr), gyr, create_graph=True)
            undeclared = lambda: torch.autograd.grad(firsts, (ur, vr, gyr), (au, av), retain_graph=True)   # noqa: E731
            declared = lambda: bnn._act_vjp_hip("gated", kind, (u, v, gy, au, av), (True, True, True))   # noqa: E731
        else:
            x, a = (torch.randn(shape, generator=g, device=DEV) for _ in range(2))
            xr = x.clone().requires_grad_(True)
            y = TORCH_FN[kind](xr)
            gy = torch.randn(y.shape, generator=g, device=DEV)
            gyr = gy.clone().requires_grad_(True)
            firsts = torch.autograd.grad(y, xr, gyr, create_graph=True)
            undeclared = lambda: torch.autograd.grad(firsts, (xr, gyr), a, retain_graph=True)   # noqa: E731
            declared = lambda: bnn._act_vjp_hip(form, kind, (x, gy, a), (True, True))   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((p - w).abs().max() / w.abs().max()) for p, w in zip(got, want))
        del want, got
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d2 = _median_ms(declared, calls - calls // 2)
        t_d = 0.5 * (t_d1 + t_d2)
        n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
        rate = algorithmic_bytes(form, shape) / (t_d * 1e-3)
        plan = plan_of(form, shape)
        say(f"{label:>10s} {'x'.join(map(str, shape)):>18s} {plan['grid']:5d} {plan['iters']:5d} {t_d * 1e3:12.1f} {n_d:8d} {rate / 1e9:12.1f} "
            f"{rate / PEAK_HBM:9.3f} {t_u * 1e3:14.1f} {n_u:8d} {t_u / t_d:7.1f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((label, shape))
        del firsts, undeclared, declared
        torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    say("(the declared call's time includes the allocation of its two or three outputs and the ctypes call; launches 1)")


def kernel_time(say):
    say("")
    say("the launches alone: C ABI on preallocated outputs, GPU events around 20 back-to-back calls, median of 5 rounds")
    say(f"{'kind':>10s} {'shape':>18s} {'us per call':>12s} {'GB/s (alg.)':>12s} {'of 8 TB/s':>9s}")
    lib = _native.load()
    st = int(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=DEV).manual_seed(0)
    kinds = {"gelu": 0, "gelu_tanh": 1, "silu": 2, "tanh": 3, "sigmoid": 4, "softplus": 5}
    cases = [(k, "plain", k, BIG) for k in kinds] + [("swiglu", "gated", "silu", (2048, 11008)), ("glu", "glu", "sigmoid", (8192, 2 * 2048))]
    for label, form, kind, shape in cases:
        n = numel(shape)
        if form == "plain":
            x, gy, a, dx, dgy = (torch.randn(n, generator=g, device=DEV) for _ in range(5))
            call = lambda: _native.check(lib.bhg_act_backward_vjp(kinds[kind], 1.0, 20.0, x.data_ptr(), gy.data_ptr(), a.data_ptr(), dx.data_ptr(),   # noqa: E731
                                                                  dgy.data_ptr(), n, st), "bhg_act_backward_vjp")
        else:
            rows, H = n // shape[-1], (shape[-1] // 2 if form == "glu" else shape[-1])
            ld = 2 * H if form == "glu" else H
            off = 4 * H if form == "glu" else 0                      # glu: u, au, du are the second halves of x, a, dx
            bufs = [torch.randn(rows * ld, generator=g, device=DEV) for _ in range(3 if form == "glu" else 6)]
            gy, dgy = (torch.randn(rows * H, generator=g, device=DEV) for _ in range(2))
            if form == "glu":
                xb, ab, db = bufs
                ptrs = [xb.data_ptr() + off, ld, xb.data_ptr(), ld, gy.data_ptr(), H, ab.data_ptr() + off, ld, ab.data_ptr(), ld,
                        db.data_ptr() + off, ld, db.data_ptr(), ld, dgy.data_ptr(), H]
            else:
                u, v, au, av, du, dv = bufs
                ptrs = [u.data_ptr(), ld, v.data_ptr(), ld, gy.data_ptr(), H, au.data_ptr(), ld, av.data_ptr(), ld, du.data_ptr(), ld,
                        dv.data_ptr(), ld, dgy.data_ptr(), H]
            call = lambda: _native.check(lib.bhg_gated_act_backward_vjp(kinds[kind], rows, H, *ptrs, st), "bhg_gated_act_backward_vjp")   # noqa: E731
        rounds = []
        for _ in range(5):
            call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) * 1e3 / 20)
        us = statistics.median(rounds)
        rate = algorithmic_bytes(form, shape) / (us * 1e-6)
        say(f"{label:>10s} {'x'.join(map(str, shape)):>18s} {us:12.1f} {rate / 1e9:12.1f} {rate / PEAK_HBM:9.3f}")
        torch.cuda.empty_cache()


def first_backward(say, calls):
    shape = (64, 64, 32, 32)
    say("")
    say(f"first backward of SiLU under create_graph=True, {'x'.join(map(str, shape))} (forward outside the timed region): median of {calls} "
        "stream-synchronised calls (three alternating rounds), kernel launches")
    g = torch.Generator(device=DEV).manual_seed(1)
    x, gy = (torch.randn(shape, generator=g, device=DEV) for _ in range(2))
    fns = {}
    for form, fn in (("undeclared", F.silu), ("declared", bnn.silu)):
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        fns[form] = lambda y=y, xr=xr: torch.autograd.grad(y, xr, gy, create_graph=True, retain_graph=True)   # noqa: E731
    t = {form: [] for form in fns}
    for _ in range(3):
        for form in t:
            t[form].append(_median_ms(fns[form], calls))
    n = {form: _count_kernels(fns[form])[0] for form in t}
    tu, td = statistics.median(t["undeclared"]), statistics.median(t["declared"])
    say(f"  undeclared {tu * 1e3:9.1f} us, {n['undeclared']:4d} launches | declared {td * 1e3:9.1f} us, {n['declared']:4d} launches | x{tu / td:.2f}")


def encoder(say, reps):
    say("")
    say("one double-backward Hessian-vector product of a two-layer nn.TransformerEncoder (d_model 768, 12 heads, ffn 3072, GELU, no dropout, "
        f"16 x 50 tokens), layer norm and attention declared in both arms: median wall ms of {reps} (three alternating rounds), kernel launches")
    row, product = {}, {}
    for form in ("without", "with", "float64"):
        torch.manual_seed(0)
        layer = nn.TransformerEncoderLayer(768, 12, dim_feedforward=3072, dropout=0.0, activation="gelu", batch_first=True)
        net = nn.TransformerEncoder(layer, 2, enable_nested_tensor=False).to(DEV)
        bnn.fuse_layernorm_(net)
        acts = bnn.declare_activations_(net) if form == "with" else 0
        dtype = torch.float64 if form == "float64" else torch.float32
        net = net.to(dtype)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(16, 50, 768, generator=g).to(DEV, dtype)
        params = list(net.parameters())
        vec = [torch.randn(t.shape, generator=g).to(DEV, dtype) for t in params]
        with bnn.declared_attention():
            grads = torch.autograd.grad((net(x) ** 2).mean(), params, create_graph=True)
        hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
        c0 = bnn.declared_activation_calls()["backward_vjp"]
        product[form] = torch.cat([t.reshape(-1) for t in hvp()]).double().cpu()
        row[form] = (hvp, acts, bnn.declared_activation_calls()["backward_vjp"] - c0)
    t = {"without": [], "with": []}
    for _ in range(3):                      # alternate
        for form in t:
            t[form].append(_median_ms(row[form][0], reps))
    n = {form: _count_kernels(row[form][0]) for form in t}
    tu, td = statistics.median(t["without"]), statistics.median(t["with"])
    say(f"  activations undeclared {tu:8.3f} ms, {n['without'][0]:6d} launches | declared ({row['with'][1]} activations, {row['with'][2]} fused calls "
        f"per product) {td:8.3f} ms, {n['with'][0]:5d} launches | x{tu / td:.2f}")
    truth = product["float64"]
    for form in ("without", "with"):
        say(f"  {form} the activations declared: {float((product[form] - truth).norm() / truth.norm()):.2e} of the norm, "
            f"{float((product[form] - truth).abs().max() / truth.abs().max()):.2e} of max|want| from the float64 product")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["dry", "per_call", "kernel_time", "first_backward", "encoder"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--ref-calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    def say(s):
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    if args.part == "dry":
        for label, form, kind, shape in SHAPES:
            say(f"{label} {shape}: {algorithmic_bytes(form, shape)} algorithmic bytes; plan {plan_of(form, shape)}")
        return
    if not torch.cuda.is_available():
        sys.exit("activation_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/activation_profile.py {args.part} on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    {"per_call": lambda: per_call(say, args.calls, args.ref_calls), "kernel_time": lambda: kernel_time(say), "first_backward": lambda: first_backward(say, args.calls),
     "encoder": lambda: encoder(say, args.reps)}[args.part]()
    if args.part == "encoder":
        say("")
        say("not measured: rocprofv3 kernel times, more than one GPU, HIP-graph replay")


if __name__ == "__main__":
    main()

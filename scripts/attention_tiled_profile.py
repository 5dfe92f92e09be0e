#!/usr/bin/env python
"""Where declaring attention beyond 64 tokens pays (betty_amd.nn.declared_attention(tiled=True), csrc/bhg_attention_tiled.hip), measured
on the GPU: the table that decides betty_amd.nn._ATTN_TILED_MAX.  The comparator is always THIS commit's undeclared math path
(sdpa_kernel(MATH)), alternating with the declared one inside one process.  The script measures the whole kernel family (it raises
_ATTN_TILED_MAX to 512 for its own process), whatever value ships.

  (i)   per call of bhg_attention_tiled_backward_vjp at 16 x 12 heads of n x n x 64, n in {65, 128, 197, 256, 384, 512} without a mask,
        128 and 512 with a (B, 1, 1, S) key-padding mask and 256 causal: the median of --calls stream-synchronised calls and kernel
        launches (torch profiler).  Beside it the same vector-Jacobian product by autograd on the undeclared math attention.
  (ii)  one double-backward Hessian-vector product of the two-layer nn.TransformerEncoder of scripts/attention_profile.py (d_model 768,
        12 heads) at 16 x 128 and 16 x 512 tokens, layer norm declared on both sides, attention undeclared / declared tiled.
  (iii) at 16 x 128 tokens, the distance of each product from the same problem's float64 product.

    python scripts/attention_tiled_profile.py [--out profiles/attention_tiled_double_backward.txt] [--calls 40] [--ref-calls 10] [--reps 5] [--dry]

--dry prints the shape table with its plans and stops (no GPU needed); every measurement needs a GPU and fails without one."""
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
from torch.nn.attention import SDPBackend, sdpa_kernel  # noqa: E402

from betty_amd import _native  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.backend import attention_tiled_plan  # noqa: E402

DEV = "cuda:0"
# B, H, L, S, d, mask ("none", "padding", "causal")
SHAPES = [(16, 12, n, n, 64, "none") for n in (65, 128, 197, 256, 384, 512)] + [(16, 12, 128, 128, 64, "padding"), (16, 12, 512, 512, 64, "padding"),
                                                                                 (16, 12, 256, 256, 64, "causal")]
TOKENS = (128, 512)


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
    say(f"(i) bhg_attention_tiled_backward_vjp per call (aq, ak, av all given, four outputs): median of {calls} stream-synchronised calls; the "
        f"undeclared math path's double backward of the same cotangents: median of {ref_calls}; launches by the torch profiler")
    say(f"{'B x H x L x S x d':>24s} {'mask':>8s} {'lds q / k':>15s} {'declared us':>12s} {'launches':>8s} {'undeclared us':>14s} {'launches':>8s} "
        f"{'ratio':>7s} {'max rel diff':>13s}")
    slower = []
    for B, H, L, S, d, kind in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(L + S + d)
        q, go, aq = (torch.randn(B, H, L, d, generator=g, device=DEV) for _ in range(3))
        k, v, ak, av = (torch.randn(B, H, S, d, generator=g, device=DEV) for _ in range(4))
        mask = None
        if kind == "padding":
            mask = torch.zeros(B, 1, 1, S, device=DEV)
            mask[::2, :, :, S - 5:] = float("-inf")
        causal = kind == "causal"
        scale = d ** -0.5
        qr, kr, vr, gor = (t.clone().requires_grad_(True) for t in (q, k, v, go))
        with sdpa_kernel(SDPBackend.MATH):
            firsts = torch.autograd.grad(F.scaled_dot_product_attention(qr, kr, vr, attn_mask=mask, is_causal=causal), (qr, kr, vr), gor,
                                         create_graph=True)
        undeclared = lambda: torch.autograd.grad(firsts, (qr, kr, vr, gor), (aq, ak, av), retain_graph=True)   # noqa: E731
        expanded = None if mask is None else mask.expand(B, H, L, S)
        declared = lambda: bnn._attn_tiled_vjp_hip(q, k, v, go, aq, ak, av, expanded, causal, scale, (True, True, True, True))   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(got, want))
        del want, got
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d2 = _median_ms(declared, calls - calls // 2)
        t_d = 0.5 * (t_d1 + t_d2)
        n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
        plan = attention_tiled_plan(B, H, L, S, d)
        say(f"{f'{B} x {H} x {L} x {S} x {d}':>24s} {kind:>8s} {str(plan['lds_q']) + ' / ' + str(plan['lds_k']):>15s} {t_d * 1e3:12.1f} {n_d:8d} "
            f"{t_u * 1e3:14.1f} {n_u:8d} {t_u / t_d:7.2f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((B, H, L, S, d, kind))
        del firsts, undeclared, qr, kr, vr, gor
        torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")
    return slower


class _Routed(nn.Module):
    """The encoder with the context its forward records the graph under."""

    def __init__(self, net, declared):
        super().__init__()
        self.net, self.declared = net, declared

    def forward(self, x):
        with (bnn.declared_attention(tiled=True) if self.declared else sdpa_kernel(SDPBackend.MATH)):
            return self.net(x)


def encoder(say, reps, tokens, with_fp64):
    say("")
    say(f"(ii) one double-backward Hessian-vector product of a two-layer nn.TransformerEncoder (d_model 768, 12 heads, ffn 3072, no dropout, "
        f"16 x {tokens} tokens), layer norm declared: median wall ms of {reps} (three alternating rounds), kernel launches")
    row, product = {}, {}
    forms = {"layer norm": (False, torch.float32), "layer norm + tiled attention": (True, torch.float32)}
    if with_fp64:
        forms["float64"] = (False, torch.float64)
    for form, (attn, dtype) in forms.items():
        torch.manual_seed(0)
        layer = nn.TransformerEncoderLayer(768, 12, dim_feedforward=3072, dropout=0.0, batch_first=True)
        net = nn.TransformerEncoder(layer, 2, enable_nested_tensor=False).to(DEV)
        if dtype == torch.float32:
            bnn.fuse_layernorm_(net)
        net = _Routed(net.to(dtype), attn)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(16, tokens, 768, generator=g).to(DEV, dtype)
        params = list(net.parameters())
        vec = [torch.randn(t.shape, generator=g).to(DEV, dtype) for t in params]
        grads = torch.autograd.grad((net(x) ** 2).mean(), params, create_graph=True)
        hvp = lambda grads=grads, params=params, vec=vec: torch.autograd.grad(grads, params, grad_outputs=vec, retain_graph=True)   # noqa: E731
        c0 = bnn.declared_attention_tiled_calls()["backward_vjp"]
        product[form] = torch.cat([t.reshape(-1) for t in hvp()]).double().cpu()
        row[form] = (hvp, bnn.declared_attention_tiled_calls()["backward_vjp"] - c0)
        if dtype == torch.float64:
            del row[form], grads, hvp
            torch.cuda.empty_cache()
    t = {form: [] for form in forms if form != "float64"}
    for _ in range(3):                      # alternate
        for form in t:
            t[form].append(_median_ms(row[form][0], reps))
    n = {form: _count_kernels(row[form][0]) for form in t}
    med = {form: statistics.median(v) for form, v in t.items()}
    for form in t:
        say(f"  {form:30s} {med[form]:8.3f} ms, {n[form][0]:6d} launches, {row[form][1]} tiled attention calls per product | x{med['layer norm'] / med[form]:.2f} "
            f"of attention undeclared")
    if with_fp64:
        say("")
        say(f"(iii) distance from the same problem's float64 product (16 x {tokens} tokens)")
        truth = product["float64"]
        for form in t:
            say(f"  {form:30s} {float((product[form] - truth).norm() / truth.norm()):.2e} of the norm, "
                f"{float((product[form] - truth).abs().max() / truth.abs().max()):.2e} of max|want|")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=40)
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
        for B, H, L, S, d, kind in SHAPES:
            say(f"{B} x {H} x {L} x {S} x {d}, mask {kind}: plan {attention_tiled_plan(B, H, L, S, d)}")
        return
    if not torch.cuda.is_available():
        sys.exit("attention_tiled_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/attention_tiled_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    say(f"betty_amd.nn._ATTN_TILED_MAX as shipped: {bnn._ATTN_TILED_MAX}; raised to 512 for this process")
    bnn._ATTN_TILED_MAX = 512
    per_call(say, args.calls, args.ref_calls)
    for tokens in TOKENS:
        encoder(say, args.reps, tokens, with_fp64=tokens == TOKENS[0])


if __name__ == "__main__":
    main()

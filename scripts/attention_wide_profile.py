#!/usr/bin/env python
"""Where declaring attention with heads of 65 to 128 elements pays (betty_amd.nn.declared_attention(wide=True),
csrc/bhg_attention_wide.hip), measured on the GPU: the table that decides betty_amd.nn._ATTN_WIDE_MAX.  The comparator is always THIS
commit's undeclared math path (sdpa_kernel(MATH)), alternating with the declared one inside one process.

  (i)  per call of bhg_attention_wide_backward_vjp at 16 x 8 heads of n x n x 128, n in {64, 128, 256, 512} without a mask, 256 causal,
       512 with a (B, 1, 1, S) key-padding mask, and 256 x 256 x 80: the median of --calls stream-synchronised calls and kernel
       launches (torch profiler).  Beside it the same vector-Jacobian product by autograd on the undeclared math attention.
  (ii) examples/llama_block_declared.py --width 256 --heads 2 (heads of 128), declared against --undeclared, each in a child process.

    python scripts/attention_wide_profile.py [--out profiles/attention_wide_double_backward.txt] [--calls 40] [--ref-calls 10] [--dry]

--dry prints the shape table with its plans and stops (no GPU needed); every measurement needs a GPU and fails without one."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.nn.attention import SDPBackend, sdpa_kernel  # noqa: E402

from attention_tiled_profile import _count_kernels, _median_ms  # noqa: E402
from betty_amd import _native  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.backend import attention_wide_plan  # noqa: E402

DEV = "cuda:0"
# B, H, L, S, d, mask ("none", "padding", "causal")
SHAPES = [(16, 8, n, n, 128, "none") for n in (64, 128, 256, 512)] + [(16, 8, 256, 256, 128, "causal"), (16, 8, 512, 512, 128, "padding"),
                                                                      (16, 8, 256, 256, 80, "none")]
EXAMPLE = ["--width", "256", "--heads", "2", "--tokens", "128", "--iters", "10", "--k", "5"]


def per_call(say, calls, ref_calls):
    say(f"(i) bhg_attention_wide_backward_vjp per call (aq, ak, av all given, four outputs): median of {calls} stream-synchronised calls; the "
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
        qr, kr, vr, gor = (t.clone().requires_grad_(True) for t in (q, k, v, go))
        with sdpa_kernel(SDPBackend.MATH):
            firsts = torch.autograd.grad(F.scaled_dot_product_attention(qr, kr, vr, attn_mask=mask, is_causal=causal), (qr, kr, vr), gor,
                                         create_graph=True)
        undeclared = lambda: torch.autograd.grad(firsts, (qr, kr, vr, gor), (aq, ak, av), retain_graph=True)   # noqa: E731
        expanded = None if mask is None else mask.expand(B, H, L, S)
        declared = lambda: bnn._attn_wide_vjp_hip(q, k, v, go, aq, ak, av, expanded, causal, d ** -0.5, (True, True, True, True))   # noqa: E731
        want, got = undeclared(), declared()
        diff = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(got, want))
        del want, got
        # alternate: declared, undeclared, declared; the declared figure is the mean of the two halves' medians
        t_d1 = _median_ms(declared, calls // 2)
        t_u = _median_ms(undeclared, ref_calls)
        t_d = 0.5 * (t_d1 + _median_ms(declared, calls - calls // 2))
        n_d, n_u = _count_kernels(declared)[0], _count_kernels(undeclared)[0]
        plan = attention_wide_plan(B, H, L, S, d)
        say(f"{f'{B} x {H} x {L} x {S} x {d}':>24s} {kind:>8s} {str(plan['lds_q']) + ' / ' + str(plan['lds_k']):>15s} {t_d * 1e3:12.1f} {n_d:8d} "
            f"{t_u * 1e3:14.1f} {n_u:8d} {t_u / t_d:7.2f} {diff:13.2e}")
        if t_d > t_u:
            slower.append((B, H, L, S, d, kind))
        del firsts, undeclared, qr, kr, vr, gor
        torch.cuda.empty_cache()
    say(f"shapes where the declared call is slower than the undeclared one: {slower if slower else 'none'}")


def example(say):
    say("")
    say("(ii) examples/llama_block_declared.py " + " ".join(EXAMPLE) + " (heads of 128 elements), one child process per arm, run twice (the second line counts)")
    for arm in ([], ["--undeclared"]):
        for _ in range(2):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "llama_block_declared.py")] + EXAMPLE + arm, capture_output=True,
                                 text=True, timeout=300)
            if out.returncode != 0:
                sys.exit(out.stderr[-2000:])
        for line in out.stdout.strip().splitlines():
            say("  " + line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--ref-calls", type=int, default=10)
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
            say(f"{B} x {H} x {L} x {S} x {d}, mask {kind}: plan {attention_wide_plan(B, H, L, S, d)}")
        return
    if not torch.cuda.is_available():
        sys.exit("attention_wide_profile: no GPU — nothing is measured on a CPU")
    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/attention_wide_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    say(f"betty_amd.nn._ATTN_WIDE_MAX as shipped: {bnn._ATTN_WIDE_MAX}")
    per_call(say, args.calls, args.ref_calls)
    example(say)


if __name__ == "__main__":
    main()

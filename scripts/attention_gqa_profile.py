#!/usr/bin/env python
"""Where declaring grouped-query attention pays (betty_amd.nn.declared_attention(gqa=True), csrc/bhg_attention_gqa.hip), measured on the
GPU: the table that decides betty_amd.nn._ATTN_GQA_MAX.  One process, the arms alternating in every round:

  (a) declared: one bhg_attention_gqa_backward_vjp call on the un-repeated K and V;
  (b) THIS commit's torch function with enable_gqa=True on the math path (sdpa_kernel(MATH)): autograd's double backward of the same
      cotangents — the comparator that decides the routing;
  (c) for information: bhg_attention_tiled_backward_vjp fed K, V, aK, aV repeated g times by hand, its g-fold dk, dv summed by ATen.

  (i)  per call at 16 x (32 on 4) x n x n x 64, n in {64, 128, 256, 512}; 16 x (9 on 3) and 16 x (8 on 1) at 256; (32 on 4) at 256 causal
       and at 512 with a (B, 1, 1, S) key-padding mask: after a warm-up per shape, --rounds rounds of [a, b, c], each the median of
       stream-synchronised calls; the figure is the median of the rounds' medians, the spread their max - min; launches by the torch
       profiler.
  (ii) examples/llama_block_declared.py --heads 8 --kv-heads 2, declared against --undeclared, each in a child process.

    python scripts/attention_gqa_profile.py [--out profiles/attention_gqa_double_backward.txt] [--rounds 5] [--calls 10] [--dry]

--dry prints the shape table with its plans and stops (no GPU needed); every measurement needs a GPU and fails without one."""
import argparse
import hashlib
import os
import statistics
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
from betty_amd.backend import attention_gqa_plan  # noqa: E402

DEV = "cuda:0"
# B, Hq, Hkv, L, S, d, mask ("none", "padding", "causal")
SHAPES = [(16, 32, 4, n, n, 64, "none") for n in (64, 128, 256, 512)] + [(16, 9, 3, 256, 256, 64, "none"), (16, 8, 1, 256, 256, 64, "none"),
                                                                         (16, 32, 4, 256, 256, 64, "causal"), (16, 32, 4, 512, 512, 64, "padding")]
EXAMPLE = ["--width", "512", "--heads", "8", "--kv-heads", "2", "--tokens", "128", "--iters", "10", "--k", "5"]


def per_call(say, rounds, calls):
    say(f"(i) double backward per call (aq, ak, av all given, four outputs), us: median of {rounds} rounds' medians of {calls} stream-synchronised "
        f"calls, arms alternating [a, b, c] in every round; (+-: max - min of the rounds' medians); launches by the torch profiler")
    say(f"{'B x (Hq on Hkv) x L x S x d':>30s} {'mask':>8s} {'grid q / k':>12s} {'(a) declared':>20s} {'n':>3s} {'(b) torch enable_gqa':>22s} {'n':>3s} "
        f"{'b / a':>6s} {'(c) tiled, repeated':>22s} {'n':>3s} {'max rel diff':>13s}")
    slower = []
    for B, Hq, Hkv, L, S, d, kind in SHAPES:
        g = Hq // Hkv
        gen = torch.Generator(device=DEV).manual_seed(L + S + Hq)
        q, go, aq = (torch.randn(B, Hq, L, d, generator=gen, device=DEV) for _ in range(3))
        k, v, ak, av = (torch.randn(B, Hkv, S, d, generator=gen, device=DEV) for _ in range(4))
        mask = None
        if kind == "padding":
            mask = torch.zeros(B, 1, 1, S, device=DEV)
            mask[::2, :, :, S - 5:] = float("-inf")
        causal = kind == "causal"
        qr, kr, vr, gor = (t.clone().requires_grad_(True) for t in (q, k, v, go))
        with sdpa_kernel(SDPBackend.MATH):
            firsts = torch.autograd.grad(F.scaled_dot_product_attention(qr, kr, vr, attn_mask=mask, is_causal=causal, enable_gqa=True),
                                         (qr, kr, vr), gor, create_graph=True)
        torch_fn = lambda: torch.autograd.grad(firsts, (qr, kr, vr, gor), (aq, ak, av), retain_graph=True)   # noqa: E731
        expanded = None if mask is None else mask.expand(B, Hq, L, S)
        need = (True, True, True, True)
        declared = lambda: bnn._attn_gqa_vjp_hip(q, k, v, go, aq, ak, av, expanded, causal, d ** -0.5, need)   # noqa: E731
        kk, vv, akk, avv = (t.repeat_interleave(g, dim=1) for t in (k, v, ak, av))   # repeated once, outside the timed call

        def repeated():
            dq, dk, dv, dgo = bnn._attn_tiled_vjp_hip(q, kk, vv, go, aq, akk, avv, expanded, causal, d ** -0.5, need)
            return dq, dk.view(B, Hkv, g, S, d).sum(2), dv.view(B, Hkv, g, S, d).sum(2), dgo

        want, got = torch_fn(), declared()
        diff = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(got, want))
        del want, got
        arms = (declared, torch_fn, repeated)
        for fn in arms:                                                         # the warm-up of the shape
            _median_ms(fn, 2)
        meds = [[_median_ms(fn, calls, warmup=1) for fn in arms] for _ in range(rounds)]
        t = [statistics.median(m[i] for m in meds) * 1e3 for i in range(3)]
        sp = [(max(m[i] for m in meds) - min(m[i] for m in meds)) * 1e3 for i in range(3)]
        n = [_count_kernels(fn)[0] for fn in arms]
        plan = attention_gqa_plan(B, Hq, Hkv, L, S, d)
        cell = lambda i: f"{t[i]:.1f} +- {sp[i]:.1f}"   # noqa: E731
        say(f"{f'{B} x ({Hq} on {Hkv}) x {L} x {S} x {d}':>30s} {kind:>8s} {str(plan['grid_q']) + ' / ' + str(plan['grid_k']):>12s} {cell(0):>20s} {n[0]:3d} "
            f"{cell(1):>22s} {n[1]:3d} {t[1] / t[0]:6.2f} {cell(2):>22s} {n[2]:3d} {diff:13.2e}")
        if t[0] > t[1] + sp[1]:
            slower.append((B, Hq, Hkv, L, S, d, kind))
        del firsts, torch_fn, qr, kr, vr, gor, kk, vv, akk, avv
        torch.cuda.empty_cache()
    say(f"shapes where (a) is slower than (b) beyond (b)'s spread: {slower if slower else 'none'}")


def example(say):
    say("")
    say("(ii) examples/llama_block_declared.py " + " ".join(EXAMPLE) + " (8 query heads of 64 on 2 key/value heads), one child process per arm, run "
        "twice (the second run's lines count)")
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
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
        for B, Hq, Hkv, L, S, d, kind in SHAPES:
            say(f"{B} x ({Hq} on {Hkv}) x {L} x {S} x {d}, mask {kind}: plan {attention_gqa_plan(B, Hq, Hkv, L, S, d)}")
        return
    if not torch.cuda.is_available():
        sys.exit("attention_gqa_profile: no GPU — nothing is measured on a CPU")
    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/attention_gqa_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    say(f"betty_amd.nn._ATTN_GQA_MAX as shipped: {bnn._ATTN_GQA_MAX}")
    per_call(say, args.rounds, args.calls)
    example(say)
    say("not measured: kernel times by rocprofv3, occupancy, other batch sizes, more than one GPU, HIP-graph replay")


if __name__ == "__main__":
    main()

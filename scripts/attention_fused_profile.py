#!/usr/bin/env python
"""Where the fused forward and first backward of declared attention pay (betty_amd.nn.declared_attention(fused=True),
csrc/bhg_attention_fused.hip), measured on the GPU: the table that decides betty_amd.nn._ATTN_FUSED_MAX.  The comparator is always THIS
commit's tiled-declared path (declared_attention(tiled=True): ATen forward that saves P, first backward written out in torch
operations), alternating with the fused one inside one process.  The script measures the whole family (it raises _ATTN_FUSED_MAX to 512
for its own process), whatever value ships.

  (i)   per call, forward plus first backward (autograd.grad of <O, gO> w.r.t. q, k, v) at 16 x 12 heads of n x n x 64,
        n in {50, 64, 128, 197, 256, 384, 512} without a mask, 256 causal and 512 with a (B, 1, 1, S) key-padding mask: --rounds
        alternating rounds of the median of --calls stream-synchronised calls per arm (the figure is the median of the rounds' medians,
        the spread their min .. max), kernel launches (torch profiler) and torch.cuda.max_memory_allocated over one call.
  (ii)  one double-backward Hessian-vector product of the two-layer encoder of scripts/attention_tiled_profile.py at 16 x 128 and
        16 x 512 tokens, attention undeclared / tiled / fused, and examples/llama_block_declared.py with and without --fused.

    python scripts/attention_fused_profile.py [--out profiles/attention_fused_first_backward.txt] [--calls 20] [--rounds 5] [--reps 5] [--dry]

--dry prints the shape table with its plans and stops (no GPU needed); every measurement needs a GPU and fails without one."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import attention_tiled_profile as tiled_profile  # noqa: E402
from betty_amd import _native  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.backend import attention_fused_plan  # noqa: E402

DEV = "cuda:0"
# B, H, L, S, d, mask ("none", "padding", "causal")
SHAPES = [(16, 12, n, n, 64, "none") for n in (50, 64, 128, 197, 256, 384, 512)] + [(16, 12, 256, 256, 64, "causal"), (16, 12, 512, 512, 64, "padding")]


def per_call(say, calls, rounds):
    say(f"(i) forward + first backward per call: median over {rounds} alternating rounds of the median of {calls} stream-synchronised calls "
        f"[min .. max of the rounds' medians]; launches by the torch profiler; peak MB = torch.cuda.max_memory_allocated over one call")
    say(f"{'B x H x L x S x d':>24s} {'mask':>8s} {'tiled us [spread]':>28s} {'launches':>8s} {'peak MB':>8s} {'fused us [spread]':>28s} {'launches':>8s} "
        f"{'peak MB':>8s} {'ratio':>6s} {'verdict':>8s}")
    verdicts = []
    for B, H, L, S, d, kind in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(L + S + d)
        q, go = (torch.randn(B, H, L, d, generator=g, device=DEV) for _ in range(2))
        k, v = (torch.randn(B, H, S, d, generator=g, device=DEV) for _ in range(2))
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        mask = None
        if kind == "padding":
            mask = torch.zeros(B, 1, 1, S, device=DEV)
            mask[::2, :, :, S - 5:] = float("-inf")

        def arm(fused):
            def call():
                with bnn.declared_attention(tiled=True, fused=fused):
                    out = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=kind == "causal")
                return torch.autograd.grad(out, (q, k, v), go)
            return call

        arms = {"tiled": arm(False), "fused": arm(True)}
        meds, launches, peak = {n: [] for n in arms}, {}, {}
        for _ in range(rounds):                      # alternate
            for name, fn in arms.items():
                meds[name].append(tiled_profile._median_ms(fn, calls) * 1e3)
        for name, fn in arms.items():
            launches[name] = tiled_profile._count_kernels(fn)[0]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        t = {n: statistics.median(m) for n, m in meds.items()}
        # "slower" = the fused median lies above the spread of the comparator's repeated medians
        verdict = "slower" if t["fused"] > max(meds["tiled"]) else "faster" if t["fused"] < min(meds["tiled"]) else "tie"
        verdicts.append(((L, kind), verdict))
        cell = lambda n: f"{t[n]:9.1f} [{min(meds[n]):7.1f} .. {max(meds[n]):7.1f}]"   # noqa: E731
        say(f"{f'{B} x {H} x {L} x {S} x {d}':>24s} {kind:>8s} {cell('tiled'):>28s} {launches['tiled']:8d} {peak['tiled']:8.1f} {cell('fused'):>28s} "
            f"{launches['fused']:8d} {peak['fused']:8.1f} {t['tiled'] / t['fused']:6.2f} {verdict:>8s}")
        torch.cuda.empty_cache()
    say(f"verdicts: {verdicts}")


def llama(say):
    say("")
    say("(ii, continued) examples/llama_block_declared.py --tokens 128 --iters 6 --algo cg (16 x 4 heads of 128 x 128 x 16), a child process per arm, twice alternating")
    for _ in range(2):
        for extra in ([], ["--fused"]):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "llama_block_declared.py"), "--tokens", "128", "--iters", "6",
                                  "--algo", "cg"] + extra, capture_output=True, text=True, timeout=300)
            say(f"  {' '.join(extra) or '(tiled)':8s} rc={out.returncode} " + " | ".join(out.stdout.strip().splitlines()[-2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
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
            say(f"{B} x {H} x {L} x {S} x {d}, mask {kind}: plan {attention_fused_plan(B, H, L, S, d)}")
        return
    if not torch.cuda.is_available():
        sys.exit("attention_fused_profile: no GPU — nothing is measured on a CPU")
    import hashlib

    sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
    say(f"scripts/attention_fused_profile.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; libbhg.so sha256 {sha}")
    say(f"betty_amd.nn._ATTN_FUSED_MAX as shipped: {bnn._ATTN_FUSED_MAX}; raised to 512 for this process")
    bnn._ATTN_FUSED_MAX = bnn._ATTN_TILED_MAX = 512
    per_call(say, args.calls, args.rounds)
    for tokens in tiled_profile.TOKENS:
        tiled_profile.encoder(say, args.reps, tokens, with_fp64=False, fused=True)
    llama(say)


if __name__ == "__main__":
    main()

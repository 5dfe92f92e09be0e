#!/usr/bin/env python
"""Per-token data reweighting of a small LLaMA-style language model whose loss is DECLARED too, on synthetic sequences.

The decoder of examples/llama_block_declared.py (its blocks, declared the same way) with a next-token head over `--vocab` tokens.  Inner
problem: the decoder's weights under the next-token loss over all `[B * T, vocab]` positions, each token's loss weighed by the
meta-weight-net (half of the training sequences continue with noise).  Upper problem: the meta-weight-net, judged on clean sequences,
trained through the implicit hypergradient (cg or neumann, K terms).  The inner training_step stays OPAQUE; beside the three layers its
sibling declares, the loss itself runs under `betty_amd.nn.declared_cross_entropy()`, which F.cross_entropy then reaches: one
bhg_cross_entropy_backward_vjp call per loss and product (csrc/bhg_cross_entropy.hip, at most two launches) instead of ATen's chain of
element-wise and reduction operators over the `[B * T, vocab]` logit matrix — by far the largest activation of the model.

    python examples/lm_reweighting_declared.py --k 5 --iters 10 [--vocab 32] [--undeclared]
"""
import argparse
import contextlib
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betty_amd import Config  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.engine import Engine, EngineConfig  # noqa: E402
from betty_amd.problems import ImplicitProblem  # noqa: E402
from llama_block_declared import DECLARED, MWN, Block  # noqa: E402


class LM(nn.Module):
    def __init__(self, vocab=32, width=64, heads=4, ffn=176, blocks=2):
        super().__init__()
        self.embed = nn.Embedding(vocab, width)
        self.blocks = nn.Sequential(*[Block(width, heads, ffn) for _ in range(blocks)])
        self.norm, self.head = nn.RMSNorm(width), nn.Linear(width, vocab, bias=False)

    def forward(self, tokens):
        """[B, T] tokens -> [B * T, vocab] next-token logits."""
        if not DECLARED[0]:   # the fused SDPA kernels have no double backward: the math path
            with torch.nn.attention.sdpa_kernel(torch.nn.attention.SDPBackend.MATH):
                return self.head(self.norm(self.blocks(self.embed(tokens)))).flatten(0, 1)
        with bnn.declared_attention(tiled=tokens.shape[1] > 64):   # only the forward that records the graph has to run inside
            return self.head(self.norm(self.blocks(self.embed(tokens)))).flatten(0, 1)


def loss_context():
    return bnn.declared_cross_entropy() if DECLARED[0] else contextlib.nullcontext()


RIDGE = 1e-3


class Reweight(ImplicitProblem):   # upper: the meta-weight-net, judged on clean sequences with the current decoder
    def training_step(self, batch):
        x, y = batch
        return F.cross_entropy(self.decoder.module(x), y.flatten())


class Train(ImplicitProblem):      # inner: the decoder on noisy sequences, each TOKEN's loss weighed by the meta-weight-net
    def training_step(self, batch):
        x, y = batch
        with loss_context():
            ce = F.cross_entropy(self.module(x), y.flatten(), reduction="none")
        w = self.reweight(ce.detach().reshape(-1, 1)).reshape(-1)
        return torch.mean(w * ce) + RIDGE * sum((p * p).sum() for p in self.module.parameters())


def make_batch(g, vocab, batch, tokens, noise):
    """Sequences that count upwards from a random start; a noisy sequence continues with random tokens instead."""
    start = torch.randint(0, vocab, (batch, 1), generator=g)
    seq = (start + torch.arange(tokens + 1)) % vocab
    flip = (torch.rand(batch, 1, generator=g) < noise).expand(batch, tokens)
    y = torch.where(flip, torch.randint(0, vocab, (batch, tokens), generator=g), seq[:, 1:])
    return seq[:, :-1].contiguous(), y.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="neumann", choices=["cg", "neumann"])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=32)
    ap.add_argument("--undeclared", action="store_true", help="leave every layer and the loss undeclared (the A/B arm)")
    args = ap.parse_args()
    DECLARED[0] = not args.undeclared
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    train = [make_batch(g, args.vocab, args.batch, args.tokens, 0.5) for _ in range(8)]
    clean = [make_batch(g, args.vocab, args.batch, args.tokens, 0.0) for _ in range(4)]
    net, mwn = LM(vocab=args.vocab, blocks=args.blocks), MWN()
    declared = bnn.declare_layers_(net, rmsnorm=True) if DECLARED[0] else {}
    cfg = Config(type=args.algo, unroll_steps=1, cg_iterations=args.k, cg_alpha=1.0, neumann_iterations=args.k, neumann_alpha=0.05)
    upper = Reweight(name="reweight", module=mwn, optimizer=torch.optim.Adam(mwn.parameters(), lr=1e-3), train_data_loader=clean, config=Config())
    inner = Train(name="decoder", module=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.05), train_data_loader=train, config=cfg)
    engine = Engine(config=EngineConfig(train_iters=args.iters), problems=[upper, inner],
                    dependencies={"u2l": {upper: [inner]}, "l2u": {inner: [upper]}})
    counters = (bnn.fused_rmsnorm_calls, bnn.declared_attention_calls, bnn.declared_activation_calls, bnn.declared_cross_entropy_calls)
    c0 = [f() for f in counters]
    t0 = time.perf_counter()
    engine.run()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rms, attn, act, ce = (f()["backward_vjp"] - was["backward_vjp"] for f, was in zip(counters, c0))
    finite = all(bool(torch.isfinite(p).all()) for p in mwn.parameters())
    print(f"LLaMA-style language model, {args.blocks} blocks, vocabulary {args.vocab}, loss over {args.batch * args.tokens} x {args.vocab} logits, "
          f"declared {declared.get('rmsnorm', 0)} RMS norms{' and the loss' if DECLARED[0] else ' (nothing)'}, {args.algo} K={args.k}: "
          f"{upper.count} upper steps in {dt:.2f} s; fused double-backward calls: RMS norm {rms}, attention {attn}, SwiGLU {act}, "
          f"cross-entropy {ce}; meta-weight-net finite {finite}")


if __name__ == "__main__":
    main()

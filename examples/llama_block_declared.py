#!/usr/bin/env python
"""Data reweighting of a small LLaMA-style decoder with every layer of its blocks DECLARED, on synthetic sequences.

Inner problem: the weights of a pre-norm decoder — `--blocks` blocks of RMSNorm -> causal multi-head attention -> residual -> RMSNorm ->
SwiGLU -> residual, a final RMSNorm and a classifier on the last token.  Upper problem: a meta-weight-net that weighs each sequence's
loss (half of the training labels are noise), trained through the implicit hypergradient (cg or neumann, K terms).  The inner
training_step stays OPAQUE — the Hessian-vector products are autograd's double backward — but its three non-linear layers are declared:

  * the RMS norms with `betty_amd.nn.declare_layers_(net, rmsnorm=True)`: one bhg_rmsnorm_backward_vjp call per layer and product
    (csrc/bhg_rmsnorm.hip, at most two launches) instead of ATen's decomposition;
  * the attention core by running the forward inside `betty_amd.nn.declared_attention()`, which F.scaled_dot_product_attention(...,
    is_causal=True) then reaches (`tiled=True` for sequences of more than 64 tokens);
  * SwiGLU by calling `betty_amd.nn.gated_activation(gate, up, "silu")` where the block would have written F.silu(gate) * up.

    python examples/llama_block_declared.py --k 5 --iters 10 [--undeclared]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betty_amd import Config  # noqa: E402
from betty_amd import nn as bnn  # noqa: E402
from betty_amd.engine import Engine, EngineConfig  # noqa: E402
from betty_amd.problems import ImplicitProblem  # noqa: E402

DECLARED = [True]


class Block(nn.Module):
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
        gate, up = self.gate(n), self.up(n)
        return h + self.down(bnn.gated_activation(gate, up, "silu") if DECLARED[0] else F.silu(gate) * up)


class Decoder(nn.Module):
    def __init__(self, vocab=32, width=64, heads=4, ffn=176, blocks=2, classes=8):
        super().__init__()
        self.embed = nn.Embedding(vocab, width)
        self.blocks = nn.Sequential(*[Block(width, heads, ffn) for _ in range(blocks)])
        self.norm, self.head = nn.RMSNorm(width), nn.Linear(width, classes)

    def forward(self, tokens):
        if not DECLARED[0]:   # the fused SDPA kernels have no double backward: the math path
            with torch.nn.attention.sdpa_kernel(torch.nn.attention.SDPBackend.MATH):
                return self.head(self.norm(self.blocks(self.embed(tokens)))[:, -1])
        with bnn.declared_attention(tiled=tokens.shape[1] > 64):   # only the forward that records the graph has to run inside
            return self.head(self.norm(self.blocks(self.embed(tokens)))[:, -1])


class MWN(nn.Module):
    def __init__(self, hidden=32):
        super().__init__()
        self.l1, self.l2 = nn.Linear(1, hidden), nn.Linear(hidden, 1)

    def forward(self, x):
        return torch.sigmoid(self.l2(F.relu(self.l1(x))))


RIDGE = 1e-3


class Reweight(ImplicitProblem):   # upper: the meta-weight-net, judged on clean batches with the current decoder
    def training_step(self, batch):
        x, y = batch
        return F.cross_entropy(self.decoder.module(x), y)


class Train(ImplicitProblem):      # inner: the decoder on noisy batches, each sequence weighed by the meta-weight-net
    def training_step(self, batch):
        x, y = batch
        ce = F.cross_entropy(self.module(x), y, reduction="none")
        w = self.reweight(ce.detach().reshape(-1, 1)).reshape(-1)
        return torch.mean(w * ce) + RIDGE * sum((p * p).sum() for p in self.module.parameters())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="neumann", choices=["cg", "neumann"])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--undeclared", action="store_true", help="leave every layer undeclared (the A/B arm)")
    args = ap.parse_args()
    DECLARED[0] = not args.undeclared
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    vocab, classes = 32, 8

    def make(noise):
        x = torch.randint(0, vocab, (args.batch, args.tokens), generator=g)
        y = (x[:, 0] + x[:, -1]) % classes                      # the label needs the first token at the last position: attention
        flip = torch.rand(args.batch, generator=g) < noise
        return x, torch.where(flip, torch.randint(0, classes, (args.batch,), generator=g), y)

    train, clean = [make(0.5) for _ in range(8)], [make(0.0) for _ in range(4)]
    net, mwn = Decoder(vocab=vocab, blocks=args.blocks, classes=classes), MWN()
    declared = bnn.declare_layers_(net, rmsnorm=True) if DECLARED[0] else {}
    cfg = Config(type=args.algo, unroll_steps=1, cg_iterations=args.k, cg_alpha=1.0, neumann_iterations=args.k, neumann_alpha=0.05)
    upper = Reweight(name="reweight", module=mwn, optimizer=torch.optim.Adam(mwn.parameters(), lr=1e-3), train_data_loader=clean, config=Config())
    inner = Train(name="decoder", module=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.05), train_data_loader=train, config=cfg)
    engine = Engine(config=EngineConfig(train_iters=args.iters), problems=[upper, inner],
                    dependencies={"u2l": {upper: [inner]}, "l2u": {inner: [upper]}})
    c0 = (bnn.fused_rmsnorm_calls(), bnn.declared_attention_calls(), bnn.declared_activation_calls())
    t0 = time.perf_counter()
    engine.run()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rms, attn, act = (now["backward_vjp"] - was["backward_vjp"] for now, was in
                      zip((bnn.fused_rmsnorm_calls(), bnn.declared_attention_calls(), bnn.declared_activation_calls()), c0))
    finite = all(bool(torch.isfinite(p).all()) for p in mwn.parameters())
    print(f"LLaMA-style decoder, {args.blocks} blocks, declared {declared.get('rmsnorm', 0)} RMS norms{'' if DECLARED[0] else ' (nothing)'}, "
          f"{args.algo} K={args.k}: {upper.count} upper steps in {dt:.2f} s; fused double-backward calls: RMS norm {rms}, attention {attn}, "
          f"SwiGLU {act}; meta-weight-net finite {finite}")


if __name__ == "__main__":
    main()

"""Fully masked rows on the declared-attention routes, shared by the four tests/test_declared_attention*.py files (a plain module, no
test of its own).  A left-padded sequence under a causal mask: the first `pad` keys of the last batch element are padding, so its rows
0 .. pad - 1 see padding only.  Torch's math path (2.10) gives such rows zeros and finite derivatives; so must every route.

dead_rows_mask: the padding and the triangle as ONE additive (B, 1, L, S) float64 mask, for the CPU graph tests.
mha_output_gradient_and_hvp: nn.MultiheadAttention with a bool key_padding_mask and a bool causal attn_mask (one type, so that torch
merges them without its deprecation warning), a mean-pooled linear head and F.cross_entropy — the output, the gradient with respect to
the parameters and one Hessian-vector product, under a declared route in fp32 or under sdpa_kernel(MATH) in any dtype."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

from betty_amd import nn as bnn

PAD = 5    # left padding of sequence 1 in the module test


def dead_rows_mask(B, L, S, pad):
    """((B, 1, L, S) additive float64 mask: -inf for the first `pad` keys of batch element B - 1 and for j > i; the (B, L) dead rows)."""
    mask = torch.zeros(B, 1, L, S, dtype=torch.float64)
    mask[B - 1, :, :, :pad] = float("-inf")
    mask = mask.masked_fill(torch.ones(L, S, dtype=torch.bool).triu(1), float("-inf"))
    dead = (mask == float("-inf")).all(-1)[:, 0]
    assert int(dead.sum()) == min(pad, L) and bool(dead[B - 1, :min(pad, L)].all())
    return mask, dead


def mha_output_gradient_and_hvp(route, dtype, embed, heads, tokens, device):
    """([output], gradients, products) as lists of numpy arrays.  `route`: the keyword arguments of betty_amd.nn.declared_attention, or
    None for the undeclared module under sdpa_kernel(MATH).  The same seeded parameters, input, labels and vector for every call."""
    torch.manual_seed(0)
    mha, head = nn.MultiheadAttention(embed, heads, batch_first=True), nn.Linear(embed, 5)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, tokens, embed, generator=g).to(device, dtype), torch.randint(0, 5, (2,), generator=g).to(device)
    mha, head = mha.to(device, dtype), head.to(device, dtype)
    params = list(mha.parameters()) + list(head.parameters())
    vec = [torch.randn(p.shape, generator=g).to(device, dtype) for p in params]
    pad = torch.zeros(2, tokens, dtype=torch.bool, device=device)
    pad[1, :PAD] = True                                                                  # True: not attended to
    causal = torch.ones(tokens, tokens, dtype=torch.bool, device=device).triu(1)
    with (sdpa_kernel(SDPBackend.MATH) if route is None else bnn.declared_attention(**route)):
        out = mha(x, x, x, key_padding_mask=pad, attn_mask=causal, need_weights=False)[0]
    grads = torch.autograd.grad(F.cross_entropy(head(out.mean(dim=1)), y), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    return [[out.detach().cpu().numpy()]] + [[t.detach().cpu().numpy() for t in ts] for ts in (grads, hv)]


def assert_route_matches_the_math_path(route, embed, heads, tokens, device, gate, label):
    """The module on `route` in fp32 against the same module in float64 under sdpa_kernel(MATH) on the same device: the output, the
    gradient and the product are finite on both sides (so torch's own zeros in dead rows are pinned on the device as well) and within
    `gate` (conftest.rel_err: of the norm and of max|want|)."""
    import numpy as np
    from conftest import rel_err

    want = mha_output_gradient_and_hvp(None, torch.float64, embed, heads, tokens, device)
    got = mha_output_gradient_and_hvp(route, torch.float32, embed, heads, tokens, device)
    for name, g, w in zip(("output", "gradient", "hvp"), got, want):
        assert all(np.isfinite(a).all() for a in w), (label, name, "torch's float64 math path is not finite")
        assert all(np.isfinite(a).all() for a in g), (label, name, "not finite")
        err = max(rel_err(g, w))
        print(f"declared attention, fully masked rows, {label}: {name} vs the float64 math path {err:.2e}")
        assert err <= gate, (label, name, err)

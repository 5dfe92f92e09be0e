"""Float64 restatement of attention's double backward: what csrc/bhg_attention.hip (bhg_attention_backward_vjp) and the declared
attention of betty_amd.nn are held to.  Plain tensor operations in the dtype of the inputs (the tests pass float64);
tests/test_attention_ref.py holds it to autograd's own float64 double backward of the written-out math attention.

Per (batch, head): q, go, aq are L x d, k, v, ak, av are S x d, `mask` is additive, broadcastable to (B, H, L, S) and not differentiated
(-inf allowed), `causal` masks j > i as well, s = scale (default 1 / sqrt(d)).
    forward          P = softmax_rows(s q k^T + m)        O = P v
    first backward   F : (q, k, v, go) -> (gq, gk, gv)
        gP = go v^T      D = rowsum(P * gP)      gS = P * (gP - D)
        gq = s gS k      gk = s gS^T q           gv = P^T go
and for cotangents aq, ak, av of gq, gk, gv — any of them None = absent = zero — attention_backward_vjp returns
    (dq, dk, dv, dgo) = d( <aq, gq> + <ak, gk> + <av, gv> ) / d(q, k, v, go)
        T   = s (aq k^T + q ak^T)            E = rowsum(P * T)
        bgP = P * (T - E)
        bP  = T * (gP - D) - gP * E + go av^T
        bS  = P * (bP - rowsum(P * bP))
        dgo = bgP v + P av                   dv = bgP^T go
        dq  = s (bS k + gS ak)               dk = s (bS^T q + gS^T aq)"""
import math

import torch


def default_scale(d):
    return 1.0 / math.sqrt(d)


def scores(q, k, mask, causal, scale):
    """s q k^T + m with the causal triangle filled with -inf: (B, H, L, S)."""
    sc = scale * (q @ k.transpose(-1, -2))
    if mask is not None:
        sc = sc + mask
    if causal:
        L, S = sc.shape[-2:]
        upper = torch.ones(L, S, dtype=torch.bool, device=sc.device).triu(1)
        sc = sc.masked_fill(upper, float("-inf"))
    return sc


def probabilities(q, k, mask=None, causal=False, scale=None):
    scale = default_scale(q.shape[-1]) if scale is None else scale
    return torch.softmax(scores(q, k, mask, causal, scale), dim=-1)


def attention(q, k, v, mask=None, causal=False, scale=None):
    """The written-out math attention: softmax(s q k^T + m) v."""
    return probabilities(q, k, mask, causal, scale) @ v


def attention_backward(q, k, v, go, mask=None, causal=False, scale=None, P=None):
    """The first backward F: (gq, gk, gv)."""
    scale = default_scale(q.shape[-1]) if scale is None else scale
    P = probabilities(q, k, mask, causal, scale) if P is None else P
    gP = go @ v.transpose(-1, -2)
    gS = P * (gP - (P * gP).sum(-1, keepdim=True))
    return scale * (gS @ k), scale * (gS.transpose(-1, -2) @ q), P.transpose(-1, -2) @ go


def attention_backward_vjp(q, k, v, go, aq, ak, av, mask=None, causal=False, scale=None):
    """q, go, aq: (B, H, L, d); k, v, ak, av: (B, H, S, d); aq, ak, av may be None.  Returns (dq, dk, dv, dgo)."""
    scale = default_scale(q.shape[-1]) if scale is None else scale
    P = probabilities(q, k, mask, causal, scale)
    gP = go @ v.transpose(-1, -2)
    D = (P * gP).sum(-1, keepdim=True)
    gS = P * (gP - D)
    T = torch.zeros_like(P)
    if aq is not None:
        T = T + scale * (aq @ k.transpose(-1, -2))
    if ak is not None:
        T = T + scale * (q @ ak.transpose(-1, -2))
    E = (P * T).sum(-1, keepdim=True)
    bgP = P * (T - E)
    bP = T * (gP - D) - gP * E
    if av is not None:
        bP = bP + go @ av.transpose(-1, -2)
    bS = P * (bP - (P * bP).sum(-1, keepdim=True))
    dgo = bgP @ v
    if av is not None:
        dgo = dgo + P @ av
    dv = bgP.transpose(-1, -2) @ go
    dq = bS @ k
    if ak is not None:
        dq = dq + gS @ ak
    dk = bS.transpose(-1, -2) @ q
    if aq is not None:
        dk = dk + gS.transpose(-1, -2) @ aq
    return scale * dq, scale * dk, dv, dgo

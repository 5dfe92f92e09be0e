"""tests/attention_tiled_ref.py — the float64 restatement of the TILED scheme of csrc/bhg_attention_tiled.hip (one online pass for
the five row statistics with its -inf guard, R by the identity rowsum(P * T * gP) - 2 D E + rowsum(P * (go av^T)), dq / dgo summed over
key tiles and dk / dv over query tiles) — held to tests/attention_ref.py's attention_backward_vjp, which tests/test_attention_ref.py
holds to autograd.  Gate 1e-10 of max|want| per output (the schemes differ by summation order only: about 1e-15 in float64).  Sizes: one
above a query tile, rectangular both ways across several tiles, causal, a padding mask that removes the first 70 keys (two whole key
tiles, and the whole first tile of every row), each cotangent absent.  No GPU needed."""
import pytest
import torch

import attention_ref
import attention_tiled_ref

GATE = 1e-10

# (L, S, d, kind)
CASES = [(65, 65, 4, "plain"), (130, 257, 8, "plain"), (257, 130, 8, "plain"), (200, 200, 8, "causal"), (65, 129, 4, "first70"),
         (130, 257, 8, "additive"), (70, 90, 4, "causal")]


def _inputs(L, S, d, kind, B=2, H=2):
    g = torch.Generator().manual_seed(L * 1000 + S + d)
    q, go, aq = (torch.randn(B, H, L, d, generator=g, dtype=torch.float64) for _ in range(3))
    k, v, ak, av = (torch.randn(B, H, S, d, generator=g, dtype=torch.float64) for _ in range(4))
    mask = None
    if kind == "first70":
        mask = torch.zeros(B, 1, 1, S, dtype=torch.float64)
        mask[..., :70] = float("-inf")
    if kind == "additive":
        mask = torch.randn(B, H, L, S, generator=g, dtype=torch.float64)
    return (q, k, v, go, aq, ak, av), mask, kind == "causal"


def _check(got, want, at):
    for name, u, w in zip(("dq", "dk", "dv", "dgo"), got, want):
        assert bool(torch.isfinite(u).all()), (at, name)
        assert float((u - w).abs().max()) <= GATE * float(w.abs().max()), (at, name, float((u - w).abs().max() / w.abs().max()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{c[3]}")
def test_tiled_scheme_matches_the_restatement(case):
    ins, mask, causal = _inputs(*case)
    want = attention_ref.attention_backward_vjp(*ins, mask=mask, causal=causal)
    _check(attention_tiled_ref.attention_backward_vjp(*ins, mask=mask, causal=causal), want, case)


@pytest.mark.parametrize("absent", [(0,), (1,), (2,), (0, 1), (1, 2)], ids=lambda a: "no_" + "_".join("a" + "qkv"[i] for i in a))
def test_each_cotangent_absent(absent):
    ins, mask, causal = _inputs(65, 129, 4, "first70")
    ins = list(ins)
    for i in absent:
        ins[4 + i] = None
    want = attention_ref.attention_backward_vjp(*ins, mask=mask, causal=causal, scale=0.37)
    _check(attention_tiled_ref.attention_backward_vjp(*ins, mask=mask, causal=causal, scale=0.37), want, absent)


def test_row_statistics_are_the_direct_ones():
    """m, l, D, E, R of the online pass against their definitions, with a first key tile that is masked out entirely."""
    ins, mask, causal = _inputs(65, 129, 4, "first70")
    q, k, v, go, aq, ak, av = ins
    s = attention_ref.default_scale(4)
    sc = attention_ref.scores(q, k, mask, causal, s)
    P = torch.softmax(sc, dim=-1)
    gP = go @ v.transpose(-1, -2)
    T = s * (aq @ k.transpose(-1, -2) + q @ ak.transpose(-1, -2))
    D, E = (P * gP).sum(-1, keepdim=True), (P * T).sum(-1, keepdim=True)
    bP = T * (gP - D) - gP * E + go @ av.transpose(-1, -2)
    m, l, D1, E1, R1 = attention_tiled_ref.row_statistics(*ins, mask=mask, causal=causal)
    for u, w in ((m, sc.amax(-1, keepdim=True)), (l, torch.exp(sc - m).sum(-1, keepdim=True)), (D1, D), (E1, E), (R1, (P * bP).sum(-1, keepdim=True))):
        assert float((u - w).abs().max()) <= GATE * float(w.abs().max())


def test_a_fully_masked_row_is_nan_and_a_wrong_identity_would_show():
    ins, _, _ = _inputs(65, 65, 4, "plain")
    mask = torch.zeros(2, 2, 65, 65, dtype=torch.float64)
    mask[0, 0, 3, :] = float("-inf")
    got = attention_tiled_ref.attention_backward_vjp(*ins, mask=mask)
    assert bool(torch.isnan(got[0][0, 0, 3]).all()) and bool(torch.isfinite(got[0][1]).all())      # as on the math path
    # R without the - 2 D E term is far outside the gate: the check above can fail
    m, l, D, E, R = attention_tiled_ref.row_statistics(*ins)
    assert float((2.0 * D * E).abs().max()) > 1e-3 * float(R.abs().max())

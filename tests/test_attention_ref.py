"""tests/attention_ref.py — the float64 restatement the attention kernel (csrc/bhg_attention.hip) is held to — against autograd's own
double backward of the written-out math attention softmax(s q k^T + m) v in float64: four shapes (one element, square, more queries
than keys, more keys than queries) x {no mask, random additive (B, 1, L, S), key padding with -inf as (B, 1, 1, S), causal where
L = S} x {all cotangents, each one absent}.
Gate: max|got - want| <= 1e-10 max|want| per array (the siblings' gate); the test prints the worst ratio."""
import pytest
import torch

import attention_ref

SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 5, 4), (2, 2, 7, 3, 5), (1, 2, 3, 9, 8)]
MASKS = ["none", "additive", "padding", "causal"]
COTANGENTS = ["qkv", "kv", "qv", "qk"]   # which of aq, ak, av are present
GATE = 1e-10


def make_mask(kind, B, L, S, g, dtype=torch.float64):
    """(mask or None, causal).  The padding mask hides the last key of every second batch entry, never all keys of a row."""
    if kind == "additive":
        return torch.randn(B, 1, L, S, generator=g, dtype=dtype), False
    if kind == "padding":
        m = torch.zeros(B, 1, 1, S, dtype=dtype)
        if S > 1:
            m[::2, :, :, S - 1] = float("-inf")
        return m, False
    return None, kind == "causal"


def _autograd(q, k, v, go, aq, ak, av, mask, causal, scale):
    """d( <aq, gq> + <ak, gk> + <av, gv> ) / d(q, k, v, go) by autograd; an output the sum does not depend on is zeros."""
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, go)]
    q, k, v, go = leaves
    out = attention_ref.attention(q, k, v, mask, causal, scale)
    gq, gk, gv = torch.autograd.grad(out, [q, k, v], go, create_graph=True)
    phi = sum((a * g).sum() for a, g in ((aq, gq), (ak, gk), (av, gv)) if a is not None)
    grads = torch.autograd.grad(phi, leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]


CASES = [(shape, kind) for shape in SHAPES for kind in MASKS if kind != "causal" or shape[2] == shape[3]]   # causal where L = S


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_restatement_matches_autograds_double_backward_fp64(shape, kind):
    B, H, L, S, d = shape
    g = torch.Generator().manual_seed(L * 1000 + S * 10 + d)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    q, go, aq = rnd(B, H, L, d), rnd(B, H, L, d), rnd(B, H, L, d)
    k, v, ak, av = rnd(B, H, S, d), rnd(B, H, S, d), rnd(B, H, S, d), rnd(B, H, S, d)
    mask, causal = make_mask(kind, B, L, S, g)
    worst = 0.0
    for scale in (None, 0.37):
        for present in COTANGENTS:
            a = [(t if ch in present else None) for ch, t in zip("qkv", (aq, ak, av))]
            want = _autograd(q, k, v, go, *a, mask, causal, attention_ref.default_scale(d) if scale is None else scale)
            got = attention_ref.attention_backward_vjp(q, k, v, go, *a, mask=mask, causal=causal, scale=scale)
            for name, u, w in zip(("dq", "dk", "dv", "dgo"), got, want):
                top = float(w.abs().max())
                err = float((u - w).abs().max())
                assert err <= GATE * top, (name, shape, kind, present, err, top)
                if top > 0:
                    worst = max(worst, err / top)
    print(f"attention_ref vs autograd's double backward, {shape} {kind}: worst max|diff| / max|want| = {worst:.2e}")


def test_the_first_backward_is_autograds():
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    q, go, k, v = rnd(2, 3, 5, 4), rnd(2, 3, 5, 4), rnd(2, 3, 6, 4), rnd(2, 3, 6, 4)
    mask = rnd(2, 1, 5, 6)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    want = torch.autograd.grad(attention_ref.attention(*leaves, mask), leaves, go)
    for u, w in zip(attention_ref.attention_backward(q, k, v, go, mask), want):
        torch.testing.assert_close(u, w, rtol=1e-12, atol=1e-12)


def test_one_key_leaves_only_dgo():
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    q, go, aq = rnd(2, 2, 5, 4), rnd(2, 2, 5, 4), rnd(2, 2, 5, 4)
    k, v, ak, av = rnd(2, 2, 1, 4), rnd(2, 2, 1, 4), rnd(2, 2, 1, 4), rnd(2, 2, 1, 4)
    dq, dk, dv, dgo = attention_ref.attention_backward_vjp(q, k, v, go, aq, ak, av)
    assert not dq.any() and not dk.any() and not dv.any()
    torch.testing.assert_close(dgo, av.expand(2, 2, 5, 4), rtol=0, atol=0)   # P = 1: dgo = P av


def test_absent_cotangents_are_zeros_and_the_terms_add_up():
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    q, go, aq = rnd(2, 2, 5, 4), rnd(2, 2, 5, 4), rnd(2, 2, 5, 4)
    k, v, ak, av = rnd(2, 2, 7, 4), rnd(2, 2, 7, 4), rnd(2, 2, 7, 4), rnd(2, 2, 7, 4)
    full = attention_ref.attention_backward_vjp(q, k, v, go, aq, ak, av)
    parts = [attention_ref.attention_backward_vjp(q, k, v, go, *a) for a in ((aq, None, None), (None, ak, None), (None, None, av))]
    for i in range(4):
        torch.testing.assert_close(sum(p[i] for p in parts), full[i], rtol=1e-12, atol=1e-12)
    assert not parts[2][2].any()   # gv = P^T go does not depend on v

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


# ---- fully masked rows: zeros, as on torch's math path --------------------------------------------------------------------------------------
DEAD_SHAPE = (2, 2, 9, 11, 4)
FIRST_GATE = 1e-12    # O and the first derivatives (the gate of test_the_first_backward_is_autograds)


def _dead_row_mask(kind):
    """(mask, dead) at DEAD_SHAPE: the additive mask and a (B, H, L) bool tensor of the rows it removes every key of.
    full: a random (B, H, L, S) mask with one dead row in one head, two dead rows in every head of batch element 1 and one row with a
    single live key.  padding: a (B, 1, 1, S) mask that removes every key of batch element 1."""
    B, H, L, S, _ = DEAD_SHAPE
    dead = torch.zeros(B, H, L, dtype=torch.bool)
    if kind == "full":
        mask = torch.randn(B, H, L, S, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
        mask[0, 1, 3] = float("-inf")
        mask[1, :, 2] = float("-inf")
        mask[1, :, 7] = float("-inf")
        mask[0, 0, 5, :S - 2] = float("-inf")       # mostly masked: two live keys, not a dead row
        dead[0, 1, 3] = dead[1, :, 2] = dead[1, :, 7] = True
    else:
        mask = torch.zeros(B, 1, 1, S, dtype=torch.float64)
        mask[1] = float("-inf")
        dead[1] = True
    return mask, dead


def _torch_math_path(q, k, v, go, aq, ak, av, mask):
    """(O, (gq, gk, gv), (dq, dk, dv, dgo)) by autograd from F.scaled_dot_product_attention under sdpa_kernel(MATH), float64, CPU."""
    from torch.nn.attention import SDPBackend, sdpa_kernel

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, go)]
    with sdpa_kernel(SDPBackend.MATH):
        out = torch.nn.functional.scaled_dot_product_attention(*leaves[:3], attn_mask=mask)
        first = torch.autograd.grad(out, leaves[:3], leaves[3], create_graph=True)
        phi = sum((a * g).sum() for a, g in zip((aq, ak, av), first))
        second = torch.autograd.grad(phi, leaves)
    return out.detach(), [t.detach() for t in first], second


@pytest.mark.parametrize("kind", ["full", "padding"])
def test_fully_masked_rows_are_zeros_as_on_torchs_math_path(kind):
    B, H, L, S, d = DEAD_SHAPE
    g = torch.Generator().manual_seed(23)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    q, go, aq = rnd(B, H, L, d), rnd(B, H, L, d), rnd(B, H, L, d)
    k, v, ak, av = rnd(B, H, S, d), rnd(B, H, S, d), rnd(B, H, S, d), rnd(B, H, S, d)
    mask, dead = _dead_row_mask(kind)
    want_o, want_first, want_second = _torch_math_path(q, k, v, go, aq, ak, av, mask)
    got_o = attention_ref.attention(q, k, v, mask)
    got_first = attention_ref.attention_backward(q, k, v, go, mask)
    got_second = attention_ref.attention_backward_vjp(q, k, v, go, aq, ak, av, mask=mask)
    worst = {}
    for gate, names, got, want in ((FIRST_GATE, ("o", "gq", "gk", "gv"), (got_o,) + tuple(got_first), [want_o] + want_first),
                                   (GATE, ("dq", "dk", "dv", "dgo"), got_second, want_second)):
        for name, u, w in zip(names, got, want):
            assert bool(torch.isfinite(w).all()), ("torch's math path", kind, name)
            assert bool(torch.isfinite(u).all()), (kind, name)
            top, err = float(w.abs().max()), float((u - w).abs().max())
            worst[name] = err / top
            assert err <= gate * top, (kind, name, err, top)
            if name in ("o", "gq", "dq", "dgo"):                      # query-side: the dead rows are exact zeros, in both
                assert not u[dead].any() and not w[dead].any(), (kind, name)
    if kind == "padding":                                            # a dead head: nothing reaches its keys either
        for u in (got_first[1], got_first[2], got_second[1], got_second[2]):
            assert not u[1].any()
    print(f"attention_ref vs torch's math path, dead rows ({kind}): " + "  ".join(f"{n} {e:.1e}" for n, e in worst.items()))

"""betty_amd.nn.wide_scaled_dot_product_attention / declared_attention(wide=True): the two-node graph around
bhg_attention_wide_backward_vjp, for heads of 65 to 128 elements.
CPU: the graph at 2 x 2 x 40 x 50 x 72 with the float64 restatement (tests/attention_tiled_ref.py) in _ATTN_WIDE_VJP_IMPL against
autograd on tests/attention_ref.py (first gradients 1e-12, double backward 1e-10), a None cotangent and an input without gradient
included; the context manager nested with the other two; calls outside the family, which must be the torch function's bits.
GPU: d = 64 counts in the siblings' counters; one attention at 2 x 2 x 70 x 90 x 128 and a one-layer nn.TransformerEncoder (d_model 256,
2 heads, 3 x 40 tokens) under declared_attention(wide=True) against the same under sdpa_kernel(MATH): first gradients to 1e-5 of
max|want|, one Hessian-vector product held to the float64 product by DESIGN 3.27's rule with the factor of the tiled sibling's test
(within 4 x the undeclared fp32 product's own error, or 2e-5), exactly one wide call per attention and product."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

import attention_dead_rows
import attention_ref
import attention_tiled_ref
from betty_amd import nn as bnn

DEV = "cuda:0"
TORCH_SDPA = F.scaled_dot_product_attention
SHAPE = (2, 2, 40, 50, 72)


@pytest.fixture
def restatement():
    seen = []

    def impl(q, k, v, go, aq, ak, av, mask, causal, scale, need):
        seen.append(((aq is not None, ak is not None, av is not None), tuple(need)))
        outs = attention_tiled_ref.attention_backward_vjp(q, k, v, go, aq, ak, av, mask=mask, causal=causal, scale=scale)
        return tuple(t if on else None for t, on in zip(outs, need))

    was = bnn._ATTN_WIDE_VJP_IMPL[0]
    bnn._ATTN_WIDE_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._ATTN_WIDE_VJP_IMPL[0] = was


def _inputs(B, H, L, S, d, seed=0, dtype=torch.float64, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, n, d, generator=g, dtype=torch.float64).to(device, dtype) for n in (L, S, S))


def _grad_and_hvp(apply, qkv, needs=(True, True, True)):
    """Gradient of a non-quadratic loss through attention and one Hessian-vector product, with respect to the inputs that need one."""
    leaves = [t.clone().requires_grad_(on) for t, on in zip(qkv, needs)]
    wrt = [t for t in leaves if t.requires_grad]
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(t.shape, generator=g, dtype=torch.float64).to(t.device, t.dtype) for t in wrt]
    out = apply(*leaves)
    grads = torch.autograd.grad((out ** 3).sum() + (out[..., :1] * out).sum(), wrt, create_graph=True)
    return [t.detach() for t in grads], list(torch.autograd.grad(grads, wrt, grad_outputs=vec))


def _worst(got, want):
    """max|got - want| / max|want| over all tensors together."""
    return max(float((u.double().cpu() - w.double().cpu()).abs().max()) for u, w in zip(got, want)) / max(float(w.abs().max()) for w in want)


@pytest.mark.parametrize("kind,needs", [("none", (True, True, True)), ("causal", (True, True, True)), ("additive", (True, True, True)),
                                        ("none", (True, True, False)), ("none", (False, True, True)),
                                        ("dead_rows", (True, True, True))])   # (new cases go last: the ids count the positions)
def test_two_node_graph_matches_the_written_out_attention_fp64(restatement, kind, needs):
    B, H, L, S, d = SHAPE
    qkv = _inputs(*SHAPE)
    mask = torch.randn(B, 1, L, S, generator=torch.Generator().manual_seed(5), dtype=torch.float64) if kind == "additive" else None
    if kind == "dead_rows":                            # left padding under the triangle: rows 0 .. 4 of the last batch element are dead
        mask = attention_dead_rows.dead_rows_mask(B, L, S, 5)[0]
    expanded, causal = None if mask is None else mask.expand(B, H, L, S), kind == "causal"
    c0 = bnn.declared_attention_wide_calls(), bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()
    want = _grad_and_hvp(lambda q, k, v: attention_ref.attention(q, k, v, mask, causal), qkv, needs)
    got = _grad_and_hvp(lambda q, k, v: bnn._AttnWideForward.apply(q, k, v, expanded, causal, attention_ref.default_scale(d)), qkv, needs)
    wide = {key: n - c0[0][key] for key, n in bnn.declared_attention_wide_calls().items()}
    assert (wide["forward"], wide["backward_vjp"]) == (1, 1) and [need for _, need in restatement] == [needs + (True,)], (wide, restatement)
    assert (bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()) == c0[1:]       # counted apart from the siblings
    assert _worst(got[0], want[0]) <= 1e-12 and _worst(got[1], want[1]) <= 1e-10


def test_an_absent_cotangent_arrives_as_none(restatement):
    qkv = [t.requires_grad_(True) for t in _inputs(*SHAPE, seed=2)]
    firsts = lambda apply: torch.autograd.grad((apply(*qkv) ** 2).sum(), qkv, create_graph=True)   # noqa: E731
    got = torch.autograd.grad(firsts(lambda q, k, v: bnn._AttnWideForward.apply(q, k, v, None, False, 0.5))[1].sum(), qkv)
    want = torch.autograd.grad(firsts(lambda q, k, v: attention_ref.attention(q, k, v, scale=0.5))[1].sum(), qkv)
    assert restatement == [((False, True, False), (True, True, True, True))], restatement
    assert max(float((u - w).abs().max()) for u, w in zip(got, want)) <= 1e-10      # (dq and dv are zeros up to rounding: an absolute gate)


def test_the_context_manager_installs_restores_and_nests():
    short, tiled, wide = bnn.scaled_dot_product_attention, bnn.tiled_scaled_dot_product_attention, bnn.wide_scaled_dot_product_attention
    with bnn.declared_attention(wide=True):
        assert F.scaled_dot_product_attention is wide
        with bnn.declared_attention(tiled=True):
            assert F.scaled_dot_product_attention is tiled
            with bnn.declared_attention():
                assert F.scaled_dot_product_attention is short
                with bnn.declared_attention(tiled=True, wide=True):
                    assert F.scaled_dot_product_attention is wide
                assert F.scaled_dot_product_attention is short
            assert F.scaled_dot_product_attention is tiled
        assert F.scaled_dot_product_attention is wide
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with pytest.raises(ZeroDivisionError):
        with bnn.declared_attention(wide=True):
            1 / 0
    assert F.scaled_dot_product_attention is TORCH_SDPA
    assert all(name in bnn.__all__ for name in ("wide_scaled_dot_product_attention", "declared_attention_wide_calls"))
    assert bnn._ATTN_WIDE_MAX_D == 128 and 64 <= bnn._ATTN_WIDE_MAX <= 512


def _check_outside_cases(device):
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(device)   # noqa: E731
    q, k, v = rnd(2, 2, 40, 72), rnd(2, 2, 50, 72), rnd(2, 2, 50, 72)
    cases = [("float64", q.double(), k.double(), v.double(), {}, True), ("dropout", q, k, v, {"dropout_p": 0.5}, True),
             ("d = 129", rnd(1, 2, 40, 129), rnd(1, 2, 50, 129), rnd(1, 2, 50, 129), {}, True),
             ("L = 513", rnd(1, 2, 513, 72), k[:1], v[:1], {}, True), ("enable_gqa", q, k[:, :1], v[:, :1], {"enable_gqa": True}, True),
             ("no_grad", q, k, v, {}, False), ("a mask that requires grad", q, k, v, {"attn_mask": rnd(2, 1, 40, 50).requires_grad_(True)}, True)]
    c0 = bnn.declared_attention_wide_calls(), bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()
    for label, q, k, v, kw, grad in cases:
        outs = []
        for fn in (bnn.wide_scaled_dot_product_attention, TORCH_SDPA):
            torch.manual_seed(0)
            with torch.set_grad_enabled(grad):
                try:
                    outs.append(fn(q, k, v, **kw))
                except RuntimeError as exc:
                    outs.append(str(exc))
        assert outs[0] == outs[1] if isinstance(outs[1], str) else torch.equal(outs[0], outs[1]), label
    assert (bnn.declared_attention_wide_calls(), bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()) == c0


@pytest.mark.parametrize("device", ["cpu", pytest.param(DEV, marks=pytest.mark.gpu)])
def test_inputs_outside_the_family_return_the_torch_functions_bits(device):
    _check_outside_cases(device)


@pytest.mark.gpu
def test_d_64_through_the_wide_function_counts_in_the_siblings_counters():
    for S, counter in ((64, bnn.declared_attention_calls), (65, bnn.declared_attention_tiled_calls)):
        q, k, v = (t.requires_grad_(True) for t in _inputs(2, 2, 5, S, 64, dtype=torch.float32, device=DEV))
        c0, w0 = counter(), bnn.declared_attention_wide_calls()
        grads = torch.autograd.grad((bnn.wide_scaled_dot_product_attention(q, k, v) ** 2).sum(), (q, k, v), create_graph=True)
        torch.autograd.grad(grads, (q, k, v), grad_outputs=[torch.ones_like(t) for t in (q, k, v)])
        assert counter()["backward_vjp"] - c0["backward_vjp"] == 1 and bnn.declared_attention_wide_calls() == w0, S


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        layer = nn.TransformerEncoderLayer(256, 2, dim_feedforward=64, dropout=0.0, activation="gelu", batch_first=True, norm_first=True)
        self.enc, self.head = nn.TransformerEncoder(layer, 1, enable_nested_tensor=False), nn.Linear(256, 5)

    def forward(self, x):
        return self.head(self.enc(x).mean(dim=1))


def _problem(which, dtype):
    """(function of the leaves, leaves) in `dtype` on the GPU: one attention, or the encoder's loss as a function of its parameters."""
    if which == "attention":
        return (lambda q, k, v: F.scaled_dot_product_attention(q, k, v)), _inputs(2, 2, 70, 90, 128, dtype=dtype, device=DEV)
    torch.manual_seed(1)
    net = _Encoder().to(DEV, dtype)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 40, 256, generator=g).to(DEV, dtype)
    names = [n for n, _ in net.named_parameters()]
    return (lambda *ps: torch.func.functional_call(net, dict(zip(names, ps)), (x,))), tuple(p.detach() for p in net.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["attention", "encoder"])
def test_gradient_and_hvp_against_the_math_path_and_float64(which):
    res = {}
    for route, dtype in (("math", torch.float32), ("declared", torch.float32), ("math", torch.float64)):
        fn, leaves = _problem(which, dtype)
        c0 = bnn.declared_attention_wide_calls()
        with (bnn.declared_attention(wide=True) if route == "declared" else sdpa_kernel(SDPBackend.MATH)):
            res[route, dtype] = _grad_and_hvp(fn, leaves)
        calls = {key: n - c0[key] for key, n in bnn.declared_attention_wide_calls().items()}
        live = 1 if route == "declared" else 0
        assert (calls["forward"], calls["backward_vjp"]) == (live, live), (route, calls)   # exactly one wide call per attention and product
    plain, declared, exact = res["math", torch.float32], res["declared", torch.float32], res["math", torch.float64]
    e_first, e_plain, e_decl = _worst(declared[0], plain[0]), _worst(plain[1], exact[1]), _worst(declared[1], exact[1])
    print(f"declared wide attention, {which}: first gradient vs the math path {e_first:.2e}; product vs the float64 product "
          f"(worst tensor of max|diff| / max|want|): declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_first <= 1e-5, e_first
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


@pytest.mark.gpu
def test_fully_masked_rows_through_multihead_attention_match_the_math_path():
    """A left-padded sequence under a causal mask (tests/attention_dead_rows.py): 2 x 70 tokens, 2 heads of 80.  Gate: the package's
    parity gate, 1e-4, as in the siblings' files."""
    c0 = bnn.declared_attention_wide_calls(), bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()
    attention_dead_rows.assert_route_matches_the_math_path({"wide": True}, 160, 2, 70, DEV, 1e-4, "wide route")
    wide = {key: n - c0[0][key] for key, n in bnn.declared_attention_wide_calls().items()}
    assert wide["forward"] == 1 and wide["backward"] >= 1 and wide["backward_vjp"] >= 1, wide
    assert (bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()) == c0[1:]

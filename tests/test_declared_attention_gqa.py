"""betty_amd.nn.gqa_scaled_dot_product_attention / declared_attention(gqa=True): the two-node graph around
bhg_attention_gqa_backward_vjp for grouped-query heads, at 2 x (2 kv heads x 3) x 70 x 90 x 16 and one causal case.

GPU: output, gradient and one Hessian-vector product against torch's float64 math path with enable_gqa=True, within the tolerances of
tests/test_declared_attention_tiled.py; one forward and one backward_vjp are counted (ONE_EACH below).  CPU: the same plumbing in
float64 with the float64 restatement (tests/attention_ref.py on repeated K and V, dk and dv summed per group) swapped in for the HIP
call.  Calls outside the family are the torch function's bits or its error and move no counter; Hq == Hkv counts in the tiled counters;
the context manager installs, composes with fused / wide and restores after an exception."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

import attention_ref
from conftest import rel_err

from betty_amd import _native
from betty_amd import nn as bnn

DEV = "cuda:0"
TORCH_SDPA = F.scaled_dot_product_attention
SHAPE = (2, 6, 2, 70, 90, 16)   # B, Hq, Hkv, L, S, d


def _inputs(B, Hq, Hkv, L, S, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, n, d, generator=g, dtype=torch.float64) for H, n in ((Hq, L), (Hkv, S), (Hkv, S)))


def _grad_and_hvp(apply, qkv):
    """Output, gradient of a non-quadratic loss through attention and one Hessian-vector product."""
    leaves = [t.clone().requires_grad_(True) for t in qkv]
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(t.shape, generator=g, dtype=torch.float64).to(t) for t in leaves]
    out = apply(*leaves)
    grads = torch.autograd.grad((out ** 3).sum() + (out[..., :1] * out).sum(), leaves, create_graph=True)
    return [out.detach().cpu().numpy()], [t.detach().cpu().numpy() for t in grads], [t.cpu().numpy() for t in torch.autograd.grad(grads, leaves, grad_outputs=vec)]


def _counters():
    return bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls(), bnn.declared_attention_gqa_calls()


def _moved(c0):
    return [{key: n - was[key] for key, n in now.items()} for was, now in zip(c0, _counters())]


# One forward, one fused double backward; the first-backward node runs for the gradient and once more inside the product, where the
# loss's own curvature sends the kernel's dgo back through the forward node (as in the sibling's tests: the loss is not linear in out).
ONE_EACH = {"forward": 1, "backward": 2, "backward_vjp": 1}


@pytest.mark.parametrize("causal", [False, True])
def test_two_node_graph_matches_the_written_out_attention_fp64(causal):
    """The CPU plumbing: the packed forward and first backward, and what reaches the hook."""
    B, Hq, Hkv, L, S, d = SHAPE
    g = Hq // Hkv
    rep = lambda t: None if t is None else t.repeat_interleave(g, dim=1)   # noqa: E731

    def impl(q, k, v, go, aq, ak, av, mask, causal, scale, need):
        assert k.shape[1] == Hkv and all(need)
        dq, dk, dv, dgo = attention_ref.attention_backward_vjp(q, rep(k), rep(v), go, aq, rep(ak), rep(av), mask=mask, causal=causal, scale=scale)
        return dq, dk.view(B, Hkv, g, S, d).sum(2), dv.view(B, Hkv, g, S, d).sum(2), dgo

    qkv = _inputs(*SHAPE)
    mask = None if causal else torch.randn(B, 1, L, S, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want = _grad_and_hvp(lambda q, k, v: attention_ref.attention(q, rep(k), rep(v), mask, causal), qkv)
    was, c0 = bnn._ATTN_GQA_VJP_IMPL[0], _counters()
    bnn._ATTN_GQA_VJP_IMPL[0] = impl
    try:
        expanded = None if mask is None else mask.expand(B, Hq, L, S)
        got = _grad_and_hvp(lambda q, k, v: bnn._AttnGqaForward.apply(q, k, v, expanded, causal, attention_ref.default_scale(d)), qkv)
    finally:
        bnn._ATTN_GQA_VJP_IMPL[0] = was
    assert _moved(c0) == [dict.fromkeys(ONE_EACH, 0)] * 2 + [ONE_EACH]
    for u, w, gate in zip(got, want, (1e-12, 1e-12, 1e-10)):              # the tiled test's FIRST_GATE and FP64_GATE
        assert rel_err(u, w)[1] <= gate, (causal, rel_err(u, w))


def _outside_cases(device):
    """(label, q, k, v, kwargs, grad enabled) of calls outside the grouped-query family."""
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(device)   # noqa: E731
    q, k, v = rnd(2, 6, 70, 8), rnd(2, 2, 90, 8), rnd(2, 2, 90, 8)
    yield "Hq % Hkv != 0", rnd(2, 5, 70, 8), k, v, {"enable_gqa": True}, True
    yield "mismatched heads without enable_gqa", q, k, v, {}, True
    yield "d = 65", rnd(1, 4, 70, 65), rnd(1, 2, 90, 65), rnd(1, 2, 90, 65), {"enable_gqa": True}, True
    yield "L = 513", rnd(1, 4, 513, 8), k[:1], v[:1], {"enable_gqa": True}, True
    yield "g L above 4096", rnd(1, 18, 512, 8), k[:1], v[:1], {"enable_gqa": True}, True
    yield "dropout", q, k, v, {"enable_gqa": True, "dropout_p": 0.5}, True
    yield "float64", q.double(), k.double(), v.double(), {"enable_gqa": True}, True
    yield "no_grad", q, k, v, {"enable_gqa": True}, False


def _check_outside_cases(device):
    c0 = _counters()
    for label, q, k, v, kw, grad in _outside_cases(device):
        outs = []
        for fn in (bnn.gqa_scaled_dot_product_attention, TORCH_SDPA):
            torch.manual_seed(0)
            with torch.set_grad_enabled(grad):
                try:
                    outs.append(fn(q, k, v, **kw))
                except RuntimeError as exc:
                    outs.append(str(exc))
        assert isinstance(outs[0], str) == isinstance(outs[1], str), label
        assert outs[0] == outs[1] if isinstance(outs[1], str) else torch.equal(outs[0], outs[1]), label   # its bits or its own error
    assert _counters() == c0


def test_inputs_outside_the_family_return_the_torch_functions_bits():
    _check_outside_cases("cpu")
    q, k, v = (t.float() for t in _inputs(1, 4, 2, 70, 70, 4))
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._attn_gqa_vjp_hip(q, k, v, q, q, None, None, None, False, 0.5, (True, True, True, True))


def test_the_context_manager_installs_composes_and_restores():
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with bnn.declared_attention(gqa=True):
        assert F.scaled_dot_product_attention is bnn.gqa_scaled_dot_product_attention
        with bnn.declared_attention(tiled=True):
            assert F.scaled_dot_product_attention is bnn.tiled_scaled_dot_product_attention
        assert F.scaled_dot_product_attention is bnn.gqa_scaled_dot_product_attention
    for flags, rest in (({"fused": True}, bnn.fused_scaled_dot_product_attention), ({"wide": True}, bnn.wide_scaled_dot_product_attention),
                        ({"wide": True, "fused": True}, bnn._wide_or_fused_scaled_dot_product_attention)):
        with pytest.raises(ZeroDivisionError):
            with bnn.declared_attention(gqa=True, **flags):
                fn = F.scaled_dot_product_attention
                assert isinstance(fn, functools.partial) and fn.func is bnn._gqa_or and fn.args == (rest,)   # grouped calls first, then `rest`
                1 / 0
        assert F.scaled_dot_product_attention is TORCH_SDPA
    for name in ("gqa_scaled_dot_product_attention", "declared_attention_gqa_calls"):
        assert name in bnn.__all__ and hasattr(bnn, name)
    assert 64 <= bnn._ATTN_GQA_MAX <= 512


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_inputs_outside_the_family_return_the_torch_functions_bits_on_the_gpu():
    _check_outside_cases(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"fused": True}], ids=["gqa", "gqa+fused"])
@pytest.mark.parametrize("causal", [False, True])
def test_output_gradient_and_hvp_against_the_float64_math_path(causal, flags):
    qkv = _inputs(*SHAPE, seed=1)
    with sdpa_kernel(SDPBackend.MATH):
        exact = _grad_and_hvp(lambda q, k, v: TORCH_SDPA(q, k, v, is_causal=causal, enable_gqa=True), [t.to(DEV) for t in qkv])
        plain = _grad_and_hvp(lambda q, k, v: TORCH_SDPA(q, k, v, is_causal=causal, enable_gqa=True), [t.float().to(DEV) for t in qkv])
    c0 = _counters()
    with bnn.declared_attention(gqa=True, **flags):
        got = _grad_and_hvp(lambda q, k, v: F.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=True), [t.float().to(DEV) for t in qkv])
    assert _moved(c0) == [dict.fromkeys(ONE_EACH, 0)] * 2 + [ONE_EACH]
    e_out, e_first, e_decl, e_plain = rel_err(got[0], exact[0])[1], rel_err(got[1], exact[1])[1], rel_err(got[2], exact[2])[1], rel_err(plain[2], exact[2])[1]
    print(f"declared gqa attention causal={causal}: output {e_out:.2e}, gradient {e_first:.2e}, product declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_out <= 1e-5 and e_first <= 1e-5, (e_out, e_first)
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


@pytest.mark.gpu
def test_equal_heads_under_gqa_are_the_tiled_declaration():
    q, k, v = (t.float().to(DEV).requires_grad_(True) for t in _inputs(2, 2, 2, 70, 90, 8))
    for kw in ({}, {"enable_gqa": True}):
        c0 = _counters()
        with bnn.declared_attention(gqa=True):
            out = F.scaled_dot_product_attention(q, k, v, **kw)
        grads = torch.autograd.grad((out ** 2).sum(), (q, k, v), create_graph=True)
        torch.autograd.grad(grads, (q, k, v), grad_outputs=[torch.ones_like(t) for t in (q, k, v)])
        assert _moved(c0) == [dict.fromkeys(ONE_EACH, 0), ONE_EACH, dict.fromkeys(ONE_EACH, 0)], kw

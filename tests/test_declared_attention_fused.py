"""betty_amd.nn.fused_scaled_dot_product_attention / declared_attention(fused=True): the two nodes around bhg_attention_fused_forward and
bhg_attention_fused_backward, whose double backward is the existing fused vector-Jacobian product.

GPU: at 2 x 3 x 70 x 70 x 16 (the tiled double backward) and 2 x 3 x 40 x 64 x 16 (the short one), plain, with a padding mask and causal,
the output, the gradient of a non-quadratic loss and one Hessian-vector product against the written-out math attention in float64 on the
same values (GATE, the siblings' parity gate); the counters; what the graph saves; nn.MultiheadAttention.
CPU: outside the family the function is the torch function; the context manager; the plan (bhg_attention_fused_plan) and its refusals."""
import pytest
import torch
import torch.nn.functional as F

import attention_dead_rows
import attention_ref
from conftest import rel_err

from betty_amd import _native
from betty_amd import nn as bnn
from betty_amd.backend import attention_fused_plan

DEV = "cuda:0"
GATE = 1e-4            # the package's parity gate, as in tests/test_declared_attention_tiled.py
TORCH_SDPA = F.scaled_dot_product_attention


def _inputs(B, H, L, S, d, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, n, d, generator=g).to(device) for n in (L, S, S))


def _out_grad_and_hvp(fn, qkv):
    leaves = [t.clone().requires_grad_(True) for t in qkv]
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(t.shape, generator=g).to(t.device, t.dtype) for t in leaves]
    out = fn(*leaves)
    loss = (out ** 3).sum() + (out[..., :1] * out).sum()
    grads = torch.autograd.grad(loss, leaves, create_graph=True)
    hv = torch.autograd.grad(sum((a * b).sum() for a, b in zip(grads, vec)), leaves)
    return [[out.detach().cpu().numpy()], [t.detach().cpu().numpy() for t in grads], [t.cpu().numpy() for t in hv]]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "padding", "causal"])
@pytest.mark.parametrize("shape", [(2, 3, 70, 70, 16), (2, 3, 40, 64, 16)], ids=["tiled", "short"])
def test_output_gradient_and_hvp_against_the_float64_math_path(shape, kind):
    B, H, L, S, d = shape
    qkv = _inputs(*shape, device=DEV)
    mask = None
    if kind == "padding":
        mask = torch.zeros(B, 1, 1, S, device=DEV)
        mask[::2, :, :, :40] = float("-inf")            # a whole key tile and more
    kw = {"attn_mask": mask, "is_causal": kind == "causal"}
    want = _out_grad_and_hvp(lambda q, k, v: attention_ref.attention(q, k, v, None if mask is None else mask.double(), kind == "causal"),
                             [t.double() for t in qkv])
    c0 = bnn.declared_attention_fused_calls(), bnn.declared_attention_tiled_calls(), bnn.declared_attention_calls()
    with bnn.declared_attention(fused=True):
        got = _out_grad_and_hvp(lambda q, k, v: F.scaled_dot_product_attention(q, k, v, **kw), qkv)
    fused, tiled, short = ({key: n - c[key] for key, n in now.items()} for now, c in
                           zip((bnn.declared_attention_fused_calls(), bnn.declared_attention_tiled_calls(), bnn.declared_attention_calls()), c0))
    # (the product of a non-quadratic loss runs the first backward once more, for the loss's own second derivative)
    assert fused == {"forward": 1, "backward": 2, "backward_vjp": 1} and not any(tiled.values()) and not any(short.values()), (fused, tiled, short)
    for name, g, w in zip(("output", "gradient", "hvp"), got, want):
        err = max(rel_err(g, w))
        print(f"declared fused attention {shape} {kind}: {name} vs float64 {err:.2e}")
        assert err <= GATE, (name, err)


@pytest.mark.gpu
def test_the_graph_saves_no_score_sized_tensor():
    B, H, L, S, d = 2, 3, 70, 70, 16
    q, k, v = (t.requires_grad_(True) for t in _inputs(B, H, L, S, d, device=DEV))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel()) or t, lambda t: t):
        with bnn.declared_attention(fused=True):
            out = F.scaled_dot_product_attention(q, k, v)
        grads = torch.autograd.grad((out ** 2).sum(), (q, k, v), create_graph=True)
    assert saved and max(saved) < B * H * L * S, saved
    assert all(t.shape == p.shape for t, p in zip(grads, (q, k, v)))


@pytest.mark.gpu
def test_multihead_attention_reaches_the_route():
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(64, 4, batch_first=True).to(DEV)
    x = torch.randn(2, 70, 64, device=DEV)
    c0 = bnn.declared_attention_fused_calls()
    with bnn.declared_attention(fused=True):
        got = mha(x, x, x, need_weights=False)[0]
    assert bnn.declared_attention_fused_calls()["forward"] == c0["forward"] + 1
    want = mha.double()(x.double(), x.double(), x.double(), need_weights=False)[0]
    assert max(rel_err([got.detach().cpu().numpy()], [want.detach().cpu().numpy()])) <= GATE


@pytest.mark.gpu
def test_fully_masked_rows_through_multihead_attention_match_the_math_path():
    """A left-padded sequence under a causal mask (tests/attention_dead_rows.py): 2 x 70 tokens, 4 heads of 16."""
    c0 = bnn.declared_attention_fused_calls(), bnn.declared_attention_tiled_calls(), bnn.declared_attention_calls()
    attention_dead_rows.assert_route_matches_the_math_path({"fused": True}, 64, 4, 70, DEV, GATE, "fused route")
    fused = {key: n - c0[0][key] for key, n in bnn.declared_attention_fused_calls().items()}
    assert fused["forward"] == 1 and fused["backward"] >= 1 and fused["backward_vjp"] >= 1, fused
    assert (bnn.declared_attention_tiled_calls(), bnn.declared_attention_calls()) == c0[1:]


def test_outside_the_family_it_is_the_torch_function():
    q, k, v = (t.requires_grad_(True) for t in _inputs(1, 2, 70, 90, 8))
    wide = tuple(t.requires_grad_(True) for t in _inputs(1, 2, 70, 90, 65, seed=1))
    c0 = bnn.declared_attention_fused_calls()
    for label, args, kw, grad in (("cpu", (q, k, v), {}, True), ("d = 65", wide, {}, True), ("dropout", (q, k, v), {"dropout_p": 0.5}, True),
                                  ("no_grad", (q, k, v), {}, False)):
        outs = []
        for fn in (bnn.fused_scaled_dot_product_attention, TORCH_SDPA):
            torch.manual_seed(0)
            with torch.set_grad_enabled(grad):
                outs.append(fn(*args, **kw))
        assert torch.equal(outs[0], outs[1]), label
    assert bnn.declared_attention_fused_calls() == c0
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._AttnFusedForward.apply(q, k, v, None, False, 0.5)


def test_the_context_manager_installs_and_restores():
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with bnn.declared_attention(fused=True):
        assert F.scaled_dot_product_attention is bnn.fused_scaled_dot_product_attention
        with bnn.declared_attention(tiled=True):
            assert F.scaled_dot_product_attention is bnn.tiled_scaled_dot_product_attention
        assert F.scaled_dot_product_attention is bnn.fused_scaled_dot_product_attention
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with pytest.raises(ZeroDivisionError):
        with bnn.declared_attention(wide=True, fused=True):
            assert F.scaled_dot_product_attention not in (TORCH_SDPA, bnn.wide_scaled_dot_product_attention)
            1 / 0
    assert F.scaled_dot_product_attention is TORCH_SDPA
    assert bnn._ATTN_FUSED_MAX <= bnn._ATTN_TILED_MAX


@pytest.mark.parametrize("d", [1, 64])
def test_the_plan(d):
    dp = (d + 15) // 16 * 16
    for n in (64, 65, 512):
        p = attention_fused_plan(3, 5, n, n, d)
        assert (p["vec"], p["bm"], p["bn"], p["ps"], p["dp"], p["pd"], p["stats"]) == (4 if d % 4 == 0 else 1, 64, 32, 36, dp, dp + 4, 8), p
        assert p["grid_f"] == p["grid_q"] == 15 * ((n + 63) // 64) and p["grid_k"] == 15 * ((n + 31) // 32) and p["ws"] == 15 * n * 8, p
        assert p["lds_f"] == 4 * ((64 + 2 * 32) * p["pd"] + 64 * 36), p
        assert p["lds_q"] == 4 * ((2 * 64 + 2 * 32) * p["pd"] + 64 * 36) + 8 * 64, p
        assert p["lds_k"] == 4 * ((2 * 64 + 2 * 32) * p["pd"] + 2 * 64 * 36) <= 163840, p
    assert attention_fused_plan(3, 5, 70, 70, 64, vec_ok=False)["vec"] == 1
    for over, word in ((dict(d=65), "more than 64 elements per head"), (dict(L=513), "more than 512 queries"), (dict(S=513), "more than 512 keys")):
        with pytest.raises(_native.NativeLibraryError, match=word):
            attention_fused_plan(**{**dict(B=3, H=5, L=70, S=70, d=d), **over})

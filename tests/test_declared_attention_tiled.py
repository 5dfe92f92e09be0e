"""betty_amd.nn.tiled_scaled_dot_product_attention / declared_attention(tiled=True): the two-node graph around
bhg_attention_tiled_backward_vjp, for more than 64 tokens.

CPU: the graph at 2 x 2 x 70 x 90 x 4 with the float64 restatement of the tiled scheme (tests/attention_tiled_ref.py) swapped in for the
HIP call, against autograd's own derivatives of the written-out math attention in float64 (first gradients to 1e-12, the double backward
to 1e-10; None cotangents and an input that needs no gradient included); the context manager with and without tiled=True, nested both
ways; inputs outside the declared family, which must be the torch function's bits.
GPU: short shapes through the tiled function count in the OLD counters (a GPU test, not a CPU one: the public function takes a declared
route for CUDA fp32 tensors only, so on the CPU it can reach neither the short nor the tiled nodes — it IS the torch function there,
which the CPU test of the outside cases pins); a one-layer nn.TransformerEncoder (d_model 64, 4 heads,
3 x 100 tokens, norm_first) under declared_attention(tiled=True) against the same net under sdpa_kernel(MATH), plain, with a key-padding
mask and causal; cg / neumann hypergradients (K = 5) of that encoder against the undeclared problem; one tiled call per attention and
product."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

import attention_ref
import attention_tiled_ref
import zoo
from conftest import rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4            # the package's parity gate (hypergradients)
FIRST_GATE = 1e-12     # first gradients of the graph on the CPU in float64
FP64_GATE = 1e-10      # its double backward
TORCH_SDPA = F.scaled_dot_product_attention
SHAPE = (2, 2, 70, 90, 4)
TOKENS = 100


@pytest.fixture
def restatement():
    """The float64 restatement of the tiled scheme in place of the HIP call, and a record of what each call received."""
    seen = []

    def impl(q, k, v, go, aq, ak, av, mask, causal, scale, need):
        seen.append(((aq is not None, ak is not None, av is not None), tuple(need)))
        outs = attention_tiled_ref.attention_backward_vjp(q, k, v, go, aq, ak, av, mask=mask, causal=causal, scale=scale)
        return tuple(t if on else None for t, on in zip(outs, need))

    was = bnn._ATTN_TILED_VJP_IMPL[0]
    bnn._ATTN_TILED_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._ATTN_TILED_VJP_IMPL[0] = was


def _inputs(B, H, L, S, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, n, d, generator=g, dtype=torch.float64) for n in (L, S, S))


def _grad_and_hvp(apply, qkv, needs=(True, True, True)):
    """Gradient of a non-quadratic loss through attention and one Hessian-vector product, with respect to the inputs that need one."""
    leaves = [t.clone().requires_grad_(on) for t, on in zip(qkv, needs)]
    wrt = [t for t in leaves if t.requires_grad]
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(t.shape, generator=g, dtype=t.dtype) for t in wrt]
    out = apply(*leaves)
    loss = (out ** 3).sum() + (out[..., :1] * out).sum()
    grads = torch.autograd.grad(loss, wrt, create_graph=True)
    return [t.detach() for t in grads], torch.autograd.grad(grads, wrt, grad_outputs=vec)


def _mask(kind, B, L, S):
    g = torch.Generator().manual_seed(5)
    if kind == "additive":
        return torch.randn(B, 1, L, S, generator=g, dtype=torch.float64), False
    if kind == "padding":
        m = torch.zeros(B, 1, 1, S, dtype=torch.float64)
        m[::2, :, :, :40] = float("-inf")          # a whole key tile and more
        return m, False
    return None, kind == "causal"


def _delta(c0):
    return ({key: n - c0[0][key] for key, n in bnn.declared_attention_calls().items()},
            {key: n - c0[1][key] for key, n in bnn.declared_attention_tiled_calls().items()})


def _counters():
    return bnn.declared_attention_calls(), bnn.declared_attention_tiled_calls()


@pytest.mark.parametrize("kind", ["none", "additive", "padding", "causal"])
def test_two_node_graph_matches_the_written_out_attention_fp64(restatement, kind):
    B, H, L, S, d = SHAPE
    qkv = _inputs(*SHAPE)
    mask, causal = _mask(kind, B, L, S)
    expanded = None if mask is None else mask.expand(B, H, L, S)
    scale = attention_ref.default_scale(d)
    c0 = _counters()
    want = _grad_and_hvp(lambda q, k, v: attention_ref.attention(q, k, v, mask, causal), qkv)
    assert _counters() == c0
    got = _grad_and_hvp(lambda q, k, v: bnn._AttnTiledForward.apply(q, k, v, expanded, causal, scale), qkv)
    short, tiled = _delta(c0)
    assert not any(short.values()), short                                   # counted apart from the short family
    assert tiled["forward"] == 1 and tiled["backward_vjp"] == 1 and restatement == [((True, True, True), (True, True, True, True))], (tiled, restatement)
    for u, w in zip(got[0], want[0]):
        assert float((u - w).abs().max()) <= FIRST_GATE * float(w.abs().max()), kind
    for u, w in zip(got[1], want[1]):
        assert float((u - w).abs().max()) <= FP64_GATE * float(w.abs().max()), kind


def test_absent_cotangents_arrive_as_none(restatement):
    qkv = [t.requires_grad_(True) for t in _inputs(*SHAPE, seed=2)]

    def firsts(apply):
        return torch.autograd.grad((apply(*qkv) ** 2).sum(), qkv, create_graph=True)

    for pick in range(3):
        del restatement[:]
        got = torch.autograd.grad(firsts(lambda q, k, v: bnn._AttnTiledForward.apply(q, k, v, None, False, 0.5))[pick].sum(), qkv, allow_unused=True)
        want = torch.autograd.grad(firsts(lambda q, k, v: attention_ref.attention(q, k, v, scale=0.5))[pick].sum(), qkv, allow_unused=True)
        assert restatement == [(tuple(i == pick for i in range(3)), (True, True, True, True))], (pick, restatement)
        for u, w in zip(got, want):
            u = torch.zeros(()) if u is None else u
            w = torch.zeros(()) if w is None else w
            assert float((u - w).abs().max()) <= FP64_GATE * max(float(w.abs().max()), 1.0), pick


def test_an_input_that_needs_no_gradient(restatement):
    qkv = _inputs(*SHAPE, seed=3)
    scale = attention_ref.default_scale(SHAPE[4])
    for needs in ((True, True, False), (False, True, True), (True, False, True)):
        del restatement[:]
        want = _grad_and_hvp(lambda q, k, v: attention_ref.attention(q, k, v), qkv, needs)
        got = _grad_and_hvp(lambda q, k, v: bnn._AttnTiledForward.apply(q, k, v, None, False, scale), qkv, needs)
        assert [need for _, need in restatement] == [needs + (True,)], restatement     # the NULL outputs of the HIP call
        for u, w in zip(list(got[0]) + list(got[1]), list(want[0]) + list(want[1])):
            assert float((u - w).abs().max()) <= FP64_GATE * float(w.abs().max()), needs


def test_the_context_manager_installs_restores_and_nests():
    short, tiled = bnn.scaled_dot_product_attention, bnn.tiled_scaled_dot_product_attention
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with bnn.declared_attention():
        assert F.scaled_dot_product_attention is short                      # the default installs what it always installed
    with bnn.declared_attention(tiled=False):
        assert F.scaled_dot_product_attention is short
    with bnn.declared_attention(tiled=True):
        assert F.scaled_dot_product_attention is tiled
        with bnn.declared_attention():                                      # the default nested inside
            assert F.scaled_dot_product_attention is short
        assert F.scaled_dot_product_attention is tiled
        with bnn.declared_attention(tiled=True):
            assert F.scaled_dot_product_attention is tiled
        assert F.scaled_dot_product_attention is tiled
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with bnn.declared_attention():
        with bnn.declared_attention(tiled=True):                            # and inside the default
            assert F.scaled_dot_product_attention is tiled
        assert F.scaled_dot_product_attention is short
    assert F.scaled_dot_product_attention is TORCH_SDPA
    with pytest.raises(ZeroDivisionError):
        with bnn.declared_attention(tiled=True):
            with bnn.declared_attention():
                1 / 0
    assert F.scaled_dot_product_attention is TORCH_SDPA
    for name in ("tiled_scaled_dot_product_attention", "declared_attention_tiled_calls"):
        assert name in bnn.__all__ and hasattr(bnn, name)
    assert 64 <= bnn._ATTN_TILED_MAX <= 512


def _outside_cases(device):
    """(label, q, k, v, kwargs, grad enabled) of calls outside the tiled family on `device`."""
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s, dtype=torch.float32: torch.randn(*s, generator=g, dtype=dtype).to(device)   # noqa: E731
    q, k, v = rnd(2, 2, 70, 8), rnd(2, 2, 90, 8), rnd(2, 2, 90, 8)
    yield "float64", q.double(), k.double(), v.double(), {}, True
    yield "dropout", q, k, v, {"dropout_p": 0.5}, True
    yield "L = 513", rnd(1, 2, 513, 8), k[:1], v[:1], {}, True
    yield "d = 65", rnd(1, 2, 70, 65), rnd(1, 2, 90, 65), rnd(1, 2, 90, 65), {}, True
    yield "no_grad", q, k, v, {}, False
    yield "a mask that requires grad", q, k, v, {"attn_mask": rnd(2, 1, 70, 90).requires_grad_(True)}, True


def _check_outside_cases(device):
    c0 = _counters()
    for label, q, k, v, kw, grad in _outside_cases(device):
        outs = []
        for fn in (bnn.tiled_scaled_dot_product_attention, TORCH_SDPA):
            torch.manual_seed(0)
            with torch.set_grad_enabled(grad):
                try:
                    outs.append(fn(q, k, v, **kw))
                except RuntimeError as exc:
                    outs.append(str(exc))
        if isinstance(outs[1], str):
            assert outs[0] == outs[1], label                                           # the torch function's own error
        else:
            assert torch.equal(outs[0], outs[1]), label
    assert _counters() == c0


def test_inputs_outside_the_family_return_the_torch_functions_bits():
    _check_outside_cases("cpu")
    q, k, v = (t.float().requires_grad_(True) for t in _inputs(*SHAPE))
    c0 = _counters()
    assert torch.equal(bnn.tiled_scaled_dot_product_attention(q, k, v), TORCH_SDPA(q, k, v)) and _counters() == c0   # CPU fp32


def test_the_hip_call_refuses_cpu_tensors():
    from betty_amd import _native

    q, k, v = (t.float() for t in _inputs(1, 1, 70, 70, 4))
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._attn_tiled_vjp_hip(q, k, v, q, q, None, None, None, False, 0.5, (True, True, True, True))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_inputs_outside_the_family_return_the_torch_functions_bits_on_the_gpu():
    _check_outside_cases(DEV)


@pytest.mark.gpu
def test_short_shapes_through_the_tiled_function_are_the_short_declaration():
    q, k, v = (t.float().to(DEV).requires_grad_(True) for t in _inputs(2, 2, 5, 64, 8))
    c0 = _counters()
    out = bnn.tiled_scaled_dot_product_attention(q, k, v)
    grads = torch.autograd.grad((out ** 2).sum(), (q, k, v), create_graph=True)
    torch.autograd.grad(grads, (q, k, v), grad_outputs=[torch.ones_like(t) for t in (q, k, v)])
    short, tiled = _delta(c0)
    assert short["forward"] == 1 and short["backward_vjp"] == 1 and not any(tiled.values()), (short, tiled)
    assert torch.equal(out, bnn.scaled_dot_product_attention(q, k, v))
    assert bnn._ATTN_TILED_MAX >= 65                                        # one more key: the tiled nodes
    q, k, v = (t.float().to(DEV).requires_grad_(True) for t in _inputs(2, 2, 5, 65, 8))
    c0 = _counters()
    bnn.tiled_scaled_dot_product_attention(q, k, v)
    short, tiled = _delta(c0)
    assert tiled["forward"] == 1 and not any(short.values()), (short, tiled)
    c0 = _counters()
    assert torch.equal(bnn.scaled_dot_product_attention(q, k, v), TORCH_SDPA(q, k, v)) and _counters() == c0   # opt-in only


class _Encoder(nn.Module):
    """One nn.TransformerEncoder layer, mean pooling and a linear head.  `route` says under which context the forward records its graph."""

    def __init__(self, kind="plain"):
        super().__init__()
        layer = nn.TransformerEncoderLayer(64, 4, dim_feedforward=64, dropout=0.0, activation="gelu", batch_first=True, norm_first=True)
        self.enc = nn.TransformerEncoder(layer, 1, enable_nested_tensor=False)
        self.head = nn.Linear(64, 5)
        self.kind, self.route = kind, "math"

    def forward(self, x):
        kw = {}
        if self.kind == "padding":
            pad = torch.zeros(x.shape[:2], dtype=torch.bool, device=x.device)
            pad[0, -40:] = True
            pad[2, -1:] = True
            kw["src_key_padding_mask"] = pad
        if self.kind == "causal":
            kw["mask"] = nn.Transformer.generate_square_subsequent_mask(x.shape[1], device=x.device, dtype=x.dtype)
            kw["is_causal"] = True
        with (bnn.declared_attention(tiled=True) if self.route == "declared" else sdpa_kernel(SDPBackend.MATH)):
            return self.head(self.enc(x, **kw).mean(dim=1))


def _encoder_grad_and_hvp(kind, route, dtype=torch.float32):
    torch.manual_seed(1)
    net = _Encoder(kind).to(DEV, dtype)
    net.route = route
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(3, TOKENS, 64, generator=g).to(DEV, dtype), torch.randint(0, 5, (3,), generator=g).to(DEV)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV, dtype) for p in params]
    c0 = _counters()
    grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    short, tiled = _delta(c0)
    live = 1 if route == "declared" and dtype == torch.float32 else 0
    assert tiled["forward"] == live and tiled["backward_vjp"] == live and not any(short.values()), (short, tiled)
    return [t.detach().cpu().numpy() for t in grads], [t.detach().cpu().numpy() for t in hv]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "padding", "causal"])
def test_encoder_gradient_and_hvp_against_the_math_path(kind):
    assert bnn._ATTN_TILED_MAX >= TOKENS
    plain, declared = _encoder_grad_and_hvp(kind, "math"), _encoder_grad_and_hvp(kind, "declared")
    _, e_first = rel_err(declared[0], plain[0])
    exact = _encoder_grad_and_hvp(kind, "math", torch.float64)[1]
    _, e_plain = rel_err(plain[1], exact)
    _, e_decl = rel_err(declared[1], exact)
    print(f"declared tiled attention, encoder {kind}: first gradient vs the math path {e_first:.2e}; product vs the float64 product "
          f"(max|diff| / max|want|): declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert np.isfinite(e_first) and e_first <= 1e-5, e_first       # not to the bit: the first backward is written out
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


def _problem(route, algo, K=5):
    torch.manual_seed(3)
    inner, upper = _Encoder("padding").to(DEV), zoo.MWN(8).to(DEV)
    inner.route = route
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(3, TOKENS, 64, generator=g).to(DEV), torch.randint(0, 5, (3,), generator=g).to(DEV)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_tiled_attention_matches_the_undeclared_problem(algo):
    out = {}
    for route in ("math", "declared"):
        curr, prev, vector = _problem(route, algo)
        c0 = _counters()
        res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[route] = [t.detach().cpu().numpy() for t in res]
        short, tiled = _delta(c0)
        # one tiled call per attention and product: the K = 5 Hessian-vector products of the solve and the mixed second derivative
        assert tiled["backward_vjp"] == (5 + 1 if route == "declared" else 0) and short["backward_vjp"] == 0, (short, tiled)
    rel, _ = rel_err(out["declared"], out["math"])
    print(f"{algo} hypergradient (K = 5), tiled attention declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel

"""betty_amd.nn.FusedLayerNorm: the two-node autograd graph (_LNForward / _LNBackward) and the module around it.

CPU part: the float64 restatement tests/layernorm_ref.py is swapped in through the `_LN_VJP_IMPL` test hook, and the graph is held to
plain nn.LayerNorm in float64: equal first gradients, the double backward to 1e-10 of max|want|, absent cotangents, re-classing.

GPU part: the module against nn.LayerNorm on the same GPU (first gradient to the bit; one Hessian-vector product against the same
problem's float64 product: the declared error at most four times the undeclared fp32 error, DESIGN 3.27's rule, or within 2e-5 of
max|want|); a cg and a neumann hypergradient (K = 5) of a transformer-style block — LayerNorm -> Linear -> GELU -> Linear with a residual
and a final LayerNorm, 48 rows x 64 features, a linear classifier on top so that there is a loss — under a meta-weight-net upper problem,
declared against undeclared at the package's parity gate (rtol 1e-4), one fused call per layer and product; and the inputs that take
nn.LayerNorm's own path."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import layernorm_ref
import zoo
from conftest import rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4          # the package's parity gate (hypergradients)
FP64_GATE = 1e-10    # the graph on the CPU in float64 against nn.LayerNorm's own double backward


def _ref_impl(x, gy, a, gamma, mean, rstd, b, c):
    """tests/layernorm_ref.py behind the signature of nn._ln_vjp_hip."""
    M = mean.numel()
    D = x.numel() // M
    rows = lambda t: None if t is None else t.reshape(M, D)      # noqa: E731
    flat = lambda t: None if t is None else t.reshape(-1)        # noqa: E731
    dx, dgy, dgamma = layernorm_ref.layernorm_backward_vjp(rows(x), rows(gy), rows(a), flat(gamma), flat(mean), flat(rstd), flat(b), flat(c))
    return dx.reshape(x.shape), dgy.reshape(x.shape), None if dgamma is None else dgamma.reshape(gamma.shape)


@pytest.fixture
def restatement():
    """The float64 restatement in place of the HIP call, and a record of the cotangents each call received."""
    seen = []

    def impl(x, gy, a, gamma, mean, rstd, b, c):
        seen.append((a is not None, b is not None, c is not None))
        return _ref_impl(x, gy, a, gamma, mean, rstd, b, c)

    was = bnn._LN_VJP_IMPL[0]
    bnn._LN_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._LN_VJP_IMPL[0] = was


def _layer(kind, ns):
    torch.manual_seed(5)
    ln = nn.LayerNorm(ns, elementwise_affine=kind != "no_affine", bias=kind != "no_bias").double()
    with torch.no_grad():
        for p in ln.parameters():
            p.normal_()
    return ln


def _grad_and_hvp(ln, apply, x):
    """Gradient of a non-quadratic loss through the layer and one Hessian-vector product, with respect to the input and the layer's parameters."""
    x = x.clone().requires_grad_(True)
    leaves = [x] + list(ln.parameters())
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(p.shape, generator=g, dtype=p.dtype) for p in leaves]
    y = apply(x)
    loss = (y ** 3).sum() + (y[..., :1] * y).sum()
    grads = torch.autograd.grad(loss, leaves, create_graph=True)
    return grads, torch.autograd.grad(grads, leaves, grad_outputs=vec)


@pytest.mark.parametrize("kind", ["affine", "no_affine", "no_bias"])
@pytest.mark.parametrize("shape,ns", [((5, 12), (12,)), ((2, 3, 8), (3, 8)), ((4, 1), (1,))], ids=lambda v: "x".join(map(str, v)))
def test_two_node_graph_matches_nn_layernorm_fp64(restatement, shape, ns, kind):
    ln = _layer(kind, ns)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    c0 = bnn.fused_layernorm_calls()
    want = _grad_and_hvp(ln, ln, x)
    assert bnn.fused_layernorm_calls() == c0                                # plain nn.LayerNorm: no node of ours
    got = _grad_and_hvp(ln, lambda t: bnn._LNForward.apply(t, ln.weight, ln.bias, list(ns), ln.eps), x)
    calls = {k: v - c0[k] for k, v in bnn.fused_layernorm_calls().items()}
    assert calls["forward"] == 1 and calls["backward_vjp"] == 1 and len(restatement) == 1, calls
    for u, v in zip(got[0], want[0]):
        assert torch.equal(u, v)                                            # ATen's own first backward on both sides
    for u, v in zip(got[1], want[1]):
        assert float((u - v).abs().max()) <= FP64_GATE * float(v.abs().max()), (shape, kind)


def test_absent_cotangents_arrive_as_none(restatement):
    ln = _layer("affine", (6,))
    x = torch.randn(3, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)

    def firsts(layer):
        y = layer(x)
        return torch.autograd.grad((y ** 2).sum(), [x, ln.weight, ln.bias], create_graph=True)

    for pick, present in ((0, (True, False, False)), (1, (False, True, False)), (2, (False, False, True))):
        del restatement[:]
        got = torch.autograd.grad(firsts(lambda t: bnn._LNForward.apply(t, ln.weight, ln.bias, [6], ln.eps))[pick].sum(), [x, ln.weight], allow_unused=True)
        want = torch.autograd.grad(firsts(ln)[pick].sum(), [x, ln.weight], allow_unused=True)
        assert restatement == [present], (pick, restatement)
        for u, v in zip(got, want):
            u = torch.zeros(()) if u is None else u
            v = torch.zeros(()) if v is None else v
            assert float((u - v).abs().max()) <= FP64_GATE * max(float(v.abs().max()), 1.0), pick


def test_an_input_that_needs_no_gradient(restatement):
    ln = _layer("affine", (6,))
    x = torch.randn(3, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    outs = []
    for apply in (ln, lambda t: bnn._LNForward.apply(t, ln.weight, ln.bias, [6], ln.eps)):
        params = list(ln.parameters())
        grads = torch.autograd.grad((apply(x) ** 3).sum(), params, create_graph=True)
        outs.append(torch.autograd.grad(grads, params, grad_outputs=[torch.ones_like(p) for p in params]))
    for u, v in zip(outs[1], outs[0]):
        assert float((u - v).abs().max()) <= FP64_GATE * float(v.abs().max())
    assert restatement == [(False, True, True)]


class _Block(nn.Module):
    """LayerNorm -> Linear -> GELU -> Linear with a residual, a final LayerNorm, and a linear classifier."""

    def __init__(self, width=64, classes=5):
        super().__init__()
        self.norm1, self.fc1, self.fc2 = nn.LayerNorm(width), nn.Linear(width, 2 * width), nn.Linear(2 * width, width)
        self.norm2, self.head = nn.LayerNorm(width), nn.Linear(width, classes)

    def forward(self, x):
        h = x + self.fc2(F.gelu(self.fc1(self.norm1(x))))
        return self.head(self.norm2(h))


def test_fuse_layernorm_changes_only_the_class():
    torch.manual_seed(0)
    net = nn.Sequential(_Block(), nn.LayerNorm(5, elementwise_affine=False), nn.BatchNorm1d(5))

    class Mine(nn.LayerNorm):
        pass

    net.add_module("mine", Mine(5))
    keys, values = list(net.state_dict()), [v.clone() for v in net.state_dict().values()]
    ids = [id(p) for p in net.parameters()]
    assert bnn.fuse_layernorm_(net) == 3
    assert type(net[0].norm1) is type(net[0].norm2) is type(net[1]) is bnn.FusedLayerNorm and type(net.mine) is Mine
    assert list(net.state_dict()) == keys and [id(p) for p in net.parameters()] == ids
    assert all(torch.equal(u, v) for u, v in zip(net.state_dict().values(), values))
    assert bnn.fuse_layernorm_(net) == 0
    x = torch.randn(4, 64)
    plain = _Block()
    plain.load_state_dict(net[0].state_dict())
    c0 = bnn.fused_layernorm_calls()
    assert torch.equal(net[0](x), plain(x)) and bnn.fused_layernorm_calls() == c0      # a CPU input IS nn.LayerNorm


def test_declare_layers_default_keys_are_unchanged():
    net = nn.Sequential(_Block(), nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=False), nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4))
    assert bnn.declare_layers_(net) == {"batchnorm": 1, "pointwise_conv": 1}
    assert type(net[0].norm1) is nn.LayerNorm and type(net[1]) is nn.Conv2d
    assert bnn.declare_layers_(net, depthwise=True) == {"batchnorm": 0, "pointwise_conv": 0, "depthwise_conv": 1}
    assert type(net[0].norm1) is nn.LayerNorm
    assert bnn.declare_layers_(net, layernorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "layernorm": 2}
    assert type(net[0].norm1) is bnn.FusedLayerNorm
    assert bnn.declare_layers_(net, depthwise=True, layernorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "depthwise_conv": 0, "layernorm": 0}


def test_the_hip_call_refuses_cpu_tensors():
    from betty_amd import _native

    t = torch.zeros(2, 4)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._ln_vjp_hip(t, t, t, None, torch.zeros(2), torch.ones(2), None, None)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
def _block_grad_and_hvp(declared, dtype=torch.float32):
    torch.manual_seed(1)
    net = _Block().to(DEV)
    if declared:
        assert bnn.fuse_layernorm_(net) == 2
    net = net.to(dtype)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(48, 64, generator=g).to(DEV, dtype), torch.randint(0, 5, (48,), generator=g).to(DEV)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV, dtype) for p in params]
    c0 = bnn.fused_layernorm_calls()
    grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    calls = {k: v - c0[k] for k, v in bnn.fused_layernorm_calls().items()}
    live = 2 if declared and dtype == torch.float32 else 0
    assert calls["backward_vjp"] == live and calls["forward"] == live, calls
    return [t.detach() for t in grads], [t.detach() for t in hv]


@pytest.mark.gpu
def test_module_matches_nn_layernorm_gradient_to_the_bit_and_hvp_within_the_fp32_error():
    plain, declared = _block_grad_and_hvp(False), _block_grad_and_hvp(True)
    for u, v in zip(declared[0], plain[0]):
        assert torch.equal(u, v)
    exact = [t.cpu().numpy() for t in _block_grad_and_hvp(False, torch.float64)[1]]
    _, e_plain = rel_err([t.cpu().numpy() for t in plain[1]], exact)
    _, e_decl = rel_err([t.cpu().numpy() for t in declared[1]], exact)
    print(f"FusedLayerNorm vs the float64 product (max|diff| / max|want|): declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


def _problem(declared, algo, K=5):
    torch.manual_seed(3)
    inner, upper = _Block().to(DEV), zoo.MWN(8).to(DEV)
    if declared:
        assert bnn.declare_layers_(inner, layernorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "layernorm": 2}
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(48, 64, generator=g).to(DEV), torch.randint(0, 5, (48,), generator=g).to(DEV)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_declared_layernorm_matches_the_undeclared_problem(algo):
    out = {}
    for declared in (False, True):
        curr, prev, vector = _problem(declared, algo)
        c0 = bnn.fused_layernorm_calls()
        res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[declared] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.fused_layernorm_calls()["backward_vjp"] - c0["backward_vjp"]
        # one fused call per layer and product.  Two layers; the products are the K = 5 Hessian-vector products of the solve and the mixed
        # second derivative that closes it: the meta-weight net enters through the loss, so that hop is one more double backward through
        # the inner network (with a proximal coupling, as in tests/test_depthwise_conv_gpu.py, it does not pass the layers)
        assert calls == (2 * (5 + 1) if declared else 0), calls
    rel, _ = rel_err(out[True], out[False])
    print(f"{algo} hypergradient (K = 5), layer norm declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel


@pytest.mark.gpu
def test_float64_noncontiguous_no_grad_and_wide_inputs_take_nn_layernorms_path():
    torch.manual_seed(0)
    c0 = bnn.fused_layernorm_calls()

    def pair(width, dtype=torch.float32):
        fused, ref = bnn.FusedLayerNorm(width).to(DEV, dtype), nn.LayerNorm(width).to(DEV, dtype)
        with torch.no_grad():
            fused.weight.normal_()
            fused.bias.normal_()
        ref.load_state_dict(fused.state_dict())
        return fused, ref

    def same_bits(fused, ref, inp):
        outs = []
        for layer in (fused, ref):
            t = inp.detach().requires_grad_(True)
            y = layer(t)
            outs.append((y.detach(), torch.autograd.grad((y ** 2).sum(), [t, layer.weight, layer.bias])))
        return torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(u, v) for u, v in zip(outs[0][1], outs[1][1]))

    fused, ref = pair(64, torch.float64)
    assert same_bits(fused, ref, torch.randn(6, 64, device=DEV, dtype=torch.float64))
    fused, ref = pair(64)
    assert same_bits(fused, ref, torch.randn(6, 128, device=DEV)[:, ::2])                         # non-contiguous
    assert same_bits(fused, ref, torch.randn(6, 65, device=DEV)[:, 1:])                           # rows not contiguous, 4-byte aligned
    fused_w, ref_w = pair(8200)
    assert same_bits(fused_w, ref_w, torch.randn(3, 8200, device=DEV))                            # D > 8192
    x = torch.randn(6, 64, device=DEV)
    with torch.no_grad():
        assert torch.equal(fused(x), ref(x))
    assert bnn.fused_layernorm_calls() == c0
    y = fused(x.requires_grad_(True))                                                             # and the declared route is live for the plain input
    assert bnn.fused_layernorm_calls()["forward"] == c0["forward"] + 1 and torch.equal(y, ref(x))

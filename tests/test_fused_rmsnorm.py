"""betty_amd.nn.FusedRMSNorm: the two-node autograd graph (_RMSForward / _RMSBackward), the module and the functional around it.

CPU part: the float64 restatement tests/rmsnorm_ref.py is swapped in through the `_RMS_VJP_IMPL` test hook, and the graph is held to plain
nn.RMSNorm in float64 (first gradients and the double backward to 1e-9 of max|want|: tests/test_rmsnorm_ref.py's gate) on shapes (5, 6),
(2, 6, 3) and (3, 4, 2, 2) — the last with normalized_shape (2, 2) —, affine and not; absent cotangents; an input that needs no gradient;
re-classing; declare_layers_; the functional and the context manager.

GPU part: the module against nn.RMSNorm on the same GPU (output and first gradient, with and without create_graph, equal to the bit to
nn.RMSNorm's ordinary backward where torch routes nn.RMSNorm through aten::_fused_rms_norm — the same two kernels — and to 1e-6 of the norm
otherwise); one Hessian-vector product of a small pre-norm block (RMSNorm -> 2-head causal attention -> RMSNorm -> SwiGLU, width 32, 4 x 10
tokens) against the same problem's float64 product: the declared error at most four times the undeclared fp32 error, DESIGN 3.27's rule,
or within 2e-5 of max|want|; a cg and a neumann hypergradient (K = 5) under the meta-weight-net upper problem of
tests/test_fused_layernorm.py, declared against undeclared at the package's parity gate (rtol 1e-4), one fused call per layer and product;
the forward-over-reverse fall-back; and the inputs that take nn.RMSNorm's own path."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import rmsnorm_ref
import zoo
from conftest import rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4          # the package's parity gate (hypergradients)
FP64_GATE = 1e-9     # the graph on the CPU in float64 against nn.RMSNorm's own double backward


@pytest.fixture
def restatement():
    """The float64 restatement in place of the HIP call, and a record of the cotangents each call received."""
    seen = []

    def impl(x, gy, a, gamma, rstd, b):
        seen.append((a is not None, b is not None))
        return rmsnorm_ref.rmsnorm_backward_vjp(x, gy, a, gamma, rstd, b)

    was = bnn._RMS_VJP_IMPL[0]
    bnn._RMS_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._RMS_VJP_IMPL[0] = was


def _layer(ns, affine=True, eps=1e-5):
    torch.manual_seed(5)
    rms = nn.RMSNorm(ns, eps=eps, elementwise_affine=affine).double()
    with torch.no_grad():
        for p in rms.parameters():
            p.normal_()
    return rms


def _declared(rms):
    return lambda t: bnn._RMSForward.apply(t, rms.weight, list(rms.normalized_shape), rms.eps)


def _grad_and_hvp(rms, apply, x):
    """Gradient of a non-quadratic loss through the layer and one Hessian-vector product, with respect to the input and the layer's parameters."""
    x = x.clone().requires_grad_(True)
    leaves = [x] + list(rms.parameters())
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(p.shape, generator=g, dtype=p.dtype) for p in leaves]
    y = apply(x)
    loss = (y ** 3).sum() + (y[:1] * y).sum()
    grads = torch.autograd.grad(loss, leaves, create_graph=True)
    return grads, torch.autograd.grad(grads, leaves, grad_outputs=vec)


@pytest.mark.parametrize("affine,eps", [(True, 1e-5), (False, 1e-5), (True, None)], ids=["affine", "no_affine", "affine_default_eps"])
@pytest.mark.parametrize("shape,ns", [((5, 6), (6,)), ((2, 6, 3), (6, 3)), ((3, 4, 2, 2), (2, 2))], ids=lambda v: "x".join(map(str, v)))
def test_two_node_graph_matches_nn_rmsnorm_fp64(restatement, shape, ns, affine, eps):
    rms = _layer(ns, affine, eps)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    c0 = bnn.fused_rmsnorm_calls()
    want = _grad_and_hvp(rms, rms, x)
    assert bnn.fused_rmsnorm_calls() == c0                                # plain nn.RMSNorm: no node of ours
    got = _grad_and_hvp(rms, _declared(rms), x)
    calls = {k: v - c0[k] for k, v in bnn.fused_rmsnorm_calls().items()}
    # (the first-backward node runs twice: once for the gradient, once more when the product's cotangent of y passes the forward node)
    assert calls == {"forward": 1, "backward": 2, "backward_vjp": 1} and len(restatement) == 1, calls
    for part in (0, 1):
        for u, v in zip(got[part], want[part]):
            assert u.shape == v.shape
            assert float((u - v).detach().abs().max()) <= FP64_GATE * float(v.detach().abs().max()), (shape, ns, affine, part)


def test_absent_cotangents_arrive_as_none(restatement):
    rms = _layer((6,))
    x = torch.randn(3, 4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)

    def firsts(layer):
        y = layer(x)
        return torch.autograd.grad((y ** 2).sum(), [x, rms.weight], create_graph=True)

    for pick, present in ((0, (True, False)), (1, (False, True))):
        del restatement[:]
        got = torch.autograd.grad(firsts(_declared(rms))[pick].sum(), [x, rms.weight], allow_unused=True)
        want = torch.autograd.grad(firsts(rms)[pick].sum(), [x, rms.weight], allow_unused=True)
        assert restatement == [present], (pick, restatement)
        for u, v in zip(got, want):
            u = torch.zeros(()) if u is None else u
            v = torch.zeros(()) if v is None else v
            assert float((u - v).abs().max()) <= FP64_GATE * max(float(v.abs().max()), 1.0), pick


def test_an_input_that_needs_no_gradient(restatement):
    rms = _layer((6,))
    x = torch.randn(3, 4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    outs = []
    for apply in (rms, _declared(rms)):
        params = list(rms.parameters())
        grads = torch.autograd.grad((apply(x) ** 3).sum(), params, create_graph=True)
        outs.append(torch.autograd.grad(grads, params, grad_outputs=[torch.ones_like(p) for p in params]))
    for u, v in zip(outs[1], outs[0]):
        assert float((u - v).abs().max()) <= FP64_GATE * float(v.abs().max())
    assert restatement == [(False, True)]


class _Block(nn.Module):
    """A LLaMA-style pre-norm block on [B, T, width] tokens: RMSNorm -> 2-head causal attention -> residual -> RMSNorm -> SwiGLU ->
    residual, then the mean over the tokens and a linear classifier.  The attention core is written out (softmax of masked scores): the
    test is about the norms, and the product does not depend on which fused attention kernel torch would pick."""

    def __init__(self, width=32, heads=2, classes=5):
        super().__init__()
        self.heads = heads
        self.norm1, self.qkv, self.proj = nn.RMSNorm(width), nn.Linear(width, 3 * width, bias=False), nn.Linear(width, width, bias=False)
        self.norm2, self.gate, self.up = nn.RMSNorm(width, eps=1e-6), nn.Linear(width, 2 * width, bias=False), nn.Linear(width, 2 * width, bias=False)
        self.down, self.head = nn.Linear(2 * width, width, bias=False), nn.Linear(width, classes)

    def forward(self, x):
        B, T, W = x.shape
        q, k, v = (t.reshape(B, T, self.heads, W // self.heads).transpose(1, 2) for t in self.qkv(self.norm1(x)).chunk(3, dim=-1))
        scores = (q @ k.transpose(-1, -2)) / math.sqrt(W // self.heads)
        scores = scores.masked_fill(torch.ones(T, T, dtype=torch.bool, device=x.device).triu(1), float("-inf"))
        h = x + self.proj((torch.softmax(scores, dim=-1) @ v).transpose(1, 2).reshape(B, T, W))
        n = self.norm2(h)
        h = h + self.down(F.silu(self.gate(n)) * self.up(n))
        return self.head(h.mean(dim=1))


def test_fuse_rmsnorm_changes_only_the_class():
    torch.manual_seed(0)
    net = nn.Sequential(_Block(), nn.RMSNorm(5, elementwise_affine=False), nn.LayerNorm(5))

    class Mine(nn.RMSNorm):
        pass

    net.add_module("mine", Mine(5))
    keys, values = list(net.state_dict()), [v.clone() for v in net.state_dict().values()]
    ids = [id(p) for p in net.parameters()]
    assert bnn.fuse_rmsnorm_(net) == 3
    assert type(net[0].norm1) is type(net[0].norm2) is type(net[1]) is bnn.FusedRMSNorm and type(net.mine) is Mine and type(net[2]) is nn.LayerNorm
    assert list(net.state_dict()) == keys and [id(p) for p in net.parameters()] == ids
    assert all(torch.equal(u, v) for u, v in zip(net.state_dict().values(), values))
    assert net[0].norm1.eps is None and net[0].norm2.eps == 1e-6 and net[1].weight is None
    assert bnn.fuse_rmsnorm_(net) == 0
    x = torch.randn(4, 10, 32)
    plain = _Block()
    plain.load_state_dict(net[0].state_dict())
    c0 = bnn.fused_rmsnorm_calls()
    assert torch.equal(net[0](x), plain(x)) and bnn.fused_rmsnorm_calls() == c0        # a CPU input IS nn.RMSNorm
    said = []
    for layer in (net[0].norm1, plain.norm1):                                           # and nn.RMSNorm's own error for a wrong width
        with pytest.raises(RuntimeError) as exc:
            layer(torch.randn(2, 7))
        said.append(str(exc.value))
    assert said[0] == said[1]


def test_declare_layers_default_keys_are_unchanged():
    net = nn.Sequential(_Block(), nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=False), nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4), nn.LayerNorm(4))
    assert bnn.declare_layers_(net) == {"batchnorm": 1, "pointwise_conv": 1}
    assert type(net[0].norm1) is nn.RMSNorm
    assert bnn.declare_layers_(net, depthwise=True, layernorm=True, groupnorm=True, activations=True) == {
        "batchnorm": 0, "pointwise_conv": 0, "depthwise_conv": 1, "layernorm": 1, "groupnorm": 0, "activations": 0}
    assert type(net[0].norm1) is nn.RMSNorm
    assert bnn.declare_layers_(net, rmsnorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "rmsnorm": 2}
    assert type(net[0].norm1) is type(net[0].norm2) is bnn.FusedRMSNorm
    assert bnn.declare_layers_(net, rmsnorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "rmsnorm": 0}


def test_the_hip_call_refuses_cpu_tensors():
    from betty_amd import _native

    t = torch.zeros(2, 4)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._rms_vjp_hip(t, t, t, None, torch.ones(2), None)


def test_declared_rmsnorm_restores_the_torch_function_on_exit_after_an_exception_too():
    was = F.rms_norm
    assert bnn._TORCH_RMS_NORM is was
    with bnn.declared_rmsnorm():
        assert F.rms_norm is bnn.rms_norm
        with bnn.declared_rmsnorm():                                                    # nesting is safe
            assert F.rms_norm is bnn.rms_norm
        assert F.rms_norm is bnn.rms_norm
        x = torch.randn(3, 6)
        c0 = bnn.fused_rmsnorm_calls()
        assert torch.equal(nn.RMSNorm(6)(x), was(x, (6,), torch.ones(6), None)) and bnn.fused_rmsnorm_calls() == c0   # a CPU input IS the torch function
    assert F.rms_norm is was
    with pytest.raises(KeyError):
        with bnn.declared_rmsnorm():
            raise KeyError("inside")
    assert F.rms_norm is was
    said = []
    for fn in (bnn.rms_norm, was):                                                      # the torch function's own error
        with pytest.raises(RuntimeError) as exc:
            fn(torch.randn(2, 7), (6,))
        said.append(str(exc.value))
    assert said[0] == said[1]


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
def _routed_through_the_fused_kernel():
    """Whether the installed torch runs nn.RMSNorm on this device as aten::_fused_rms_norm (its autograd node says so)."""
    y = nn.RMSNorm(8).to(DEV)(torch.randn(2, 8, device=DEV))
    return "FusedRmsNorm" in type(y.grad_fn).__name__


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ns,affine,eps", [((6, 32), (32,), True, None), ((4, 10, 32), (32,), True, 1e-6), ((3, 5, 4, 6), (4, 6), True, 1e-5),
                                                  ((5, 7, 9), (9,), False, None), ((3, 4100), (4100,), True, 1e-5), ((300, 260), (260,), True, 1e-5)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_module_output_and_first_gradient_equal_nn_rmsnorms_ordinary_backward(shape, ns, affine, eps):
    """nn.RMSNorm's ordinary backward (no create_graph) is _fused_rms_norm_backward; under create_graph ATen replaces it by a decomposition.
    The declared layer runs the single kernel in both cases: the same bits as the ordinary backward, and the same output."""
    torch.manual_seed(2)
    fused, ref = bnn.FusedRMSNorm(ns, eps=eps, elementwise_affine=affine).to(DEV), nn.RMSNorm(ns, eps=eps, elementwise_affine=affine).to(DEV)
    if affine:
        with torch.no_grad():
            fused.weight.normal_()
    ref.load_state_dict(fused.state_dict())
    x = torch.randn(shape, device=DEV)

    def first(layer, create_graph):
        t = x.clone().requires_grad_(True)
        y = layer(t)
        return [y.detach()] + [v.detach() for v in torch.autograd.grad((y ** 3).sum(), [t] + list(layer.parameters()), create_graph=create_graph)]

    routed = _routed_through_the_fused_kernel()
    c0 = bnn.fused_rmsnorm_calls()
    ordinary = first(ref, False)
    assert bnn.fused_rmsnorm_calls() == c0
    for create_graph in (True, False):
        for u, v in zip(first(fused, create_graph), ordinary):
            if routed:
                assert torch.equal(u, v), create_graph
            else:
                assert float((u - v).norm()) <= 1e-6 * float(v.norm()), create_graph
    print(f"FusedRMSNorm {shape}: nn.RMSNorm routed through aten::_fused_rms_norm: {routed} -> held to "
          + ("bit equality" if routed else "1e-6 of the norm"))
    assert bnn.fused_rmsnorm_calls()["forward"] == c0["forward"] + 2


def _tokens(g, dtype=torch.float32):
    return torch.randn(4, 10, 32, generator=g).to(DEV, dtype), torch.randint(0, 5, (4,), generator=g).to(DEV)


def _block_grad_and_hvp(declared, dtype=torch.float32):
    torch.manual_seed(1)
    net = _Block().to(DEV)
    if declared:
        assert bnn.fuse_rmsnorm_(net) == 2
    net = net.to(dtype)
    g = torch.Generator().manual_seed(1)
    x, y = _tokens(g, dtype)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV, dtype) for p in params]
    c0 = bnn.fused_rmsnorm_calls()
    grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    calls = {k: v - c0[k] for k, v in bnn.fused_rmsnorm_calls().items()}
    live = 2 if declared and dtype == torch.float32 else 0
    assert calls["backward_vjp"] == live and calls["forward"] == live, calls   # exactly one fused call per layer and product
    return [t.detach() for t in grads], [t.detach() for t in hv]


@pytest.mark.gpu
def test_block_hvp_within_the_fp32_error_of_the_float64_product():
    plain, declared = _block_grad_and_hvp(False), _block_grad_and_hvp(True)
    rel, _ = rel_err([t.cpu().numpy() for t in declared[0]], [t.cpu().numpy() for t in plain[0]])
    print(f"FusedRMSNorm block, first gradient under create_graph, declared vs undeclared: {rel:.2e} of the norm")
    assert rel <= 1e-6, rel
    exact = [t.cpu().numpy() for t in _block_grad_and_hvp(False, torch.float64)[1]]
    _, e_plain = rel_err([t.cpu().numpy() for t in plain[1]], exact)
    _, e_decl = rel_err([t.cpu().numpy() for t in declared[1]], exact)
    print(f"FusedRMSNorm vs the float64 product (max|diff| / max|want|): declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


def _problem(declared, algo, K=5):
    torch.manual_seed(3)
    inner, upper = _Block().to(DEV), zoo.MWN(8).to(DEV)
    if declared:
        assert bnn.declare_layers_(inner, rmsnorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "rmsnorm": 2}
    g = torch.Generator().manual_seed(3)
    x, y = _tokens(g)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_declared_rmsnorm_matches_the_undeclared_problem(algo):
    out = {}
    for declared in (False, True):
        curr, prev, vector = _problem(declared, algo)
        c0 = bnn.fused_rmsnorm_calls()
        res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[declared] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.fused_rmsnorm_calls()["backward_vjp"] - c0["backward_vjp"]
        # one fused call per layer and product: two layers, the K = 5 Hessian-vector products of the solve and the mixed second derivative
        # that closes it (the meta-weight net enters through the loss: one more double backward through the inner network)
        assert calls == (2 * (5 + 1) if declared else 0), calls
    rel, _ = rel_err(out[True], out[False])
    print(f"{algo} hypergradient (K = 5), RMS norm declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel


@pytest.mark.gpu
def test_forward_over_reverse_on_a_declared_net_falls_back_to_the_double_backward_with_its_warning():
    """Custom Functions have no forward-mode formula: as documented for declared layer norm, the first forward-over-reverse pass fails, the
    solve warns and continues on the double backward — through the fused calls — and gives the default's answer."""
    out = {}
    for mode in (None, "forward_over_reverse"):
        curr, prev, vector = _problem(True, "neumann")
        c0 = bnn.fused_rmsnorm_calls()["backward_vjp"]
        if mode:
            curr.hypergradient_hvp = mode
            with pytest.warns(RuntimeWarning, match="forward-over-reverse HVP not available"):
                res = hg.neumann(vector, curr, prev, False)
        else:
            res = hg.neumann(vector, curr, prev, False)
        out[mode] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.fused_rmsnorm_calls()["backward_vjp"] - c0
        print(f"neumann (K = 5) on the declared net, hypergradient_hvp = {mode}: {calls} fused calls")
        assert calls == 2 * (5 + 1), (mode, calls)
    rel, _ = rel_err(out["forward_over_reverse"], out[None])
    assert rel <= 1e-5, rel


@pytest.mark.gpu
def test_float64_noncontiguous_no_grad_and_wide_inputs_take_nn_rmsnorms_path():
    torch.manual_seed(0)
    c0 = bnn.fused_rmsnorm_calls()

    def pair(D, dtype=torch.float32):
        fused, ref = bnn.FusedRMSNorm(D).to(DEV, dtype), nn.RMSNorm(D).to(DEV, dtype)
        with torch.no_grad():
            fused.weight.normal_()
        ref.load_state_dict(fused.state_dict())
        return fused, ref

    def same_bits(fused, ref, inp, fn=None):
        outs = []
        for layer in (fused, ref):
            t = inp.detach().requires_grad_(True)
            y = layer(t) if fn is None else fn(t, layer)
            outs.append((y.detach(), torch.autograd.grad((y ** 2).sum(), [t, layer.weight])))
        return torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(u, v) for u, v in zip(outs[0][1], outs[1][1]))

    fused, ref = pair(8, torch.float64)
    assert same_bits(fused, ref, torch.randn(6, 5, 8, device=DEV, dtype=torch.float64))
    fused, ref = pair(8)
    assert same_bits(fused, ref, torch.randn(6, 5, 16, device=DEV)[:, :, ::2])                    # non-contiguous
    assert same_bits(fused, ref, torch.randn(6, 9, 8, device=DEV)[:, ::2])                        # rows not contiguous
    fused_w, ref_w = pair(8196)
    assert same_bits(fused_w, ref_w, torch.randn(3, 8196, device=DEV))                            # D = 8196 > 8192
    x = torch.randn(6, 5, 8, device=DEV)
    with torch.no_grad():
        assert torch.equal(fused(x), ref(x))
    # the functional, inside the context manager too: the same conditions
    with bnn.declared_rmsnorm():
        assert same_bits(fused_w, ref_w, torch.randn(3, 8196, device=DEV), fn=lambda t, layer: F.rms_norm(t, (8196,), layer.weight, None))
    assert bnn.fused_rmsnorm_calls() == c0
    y = fused(x.requires_grad_(True))                                                             # and the declared route is live for the plain input
    assert bnn.fused_rmsnorm_calls()["forward"] == c0["forward"] + 1 and torch.equal(y, ref(x))
    with bnn.declared_rmsnorm():
        y = ref(x)                                                                                # nn.RMSNorm itself, through the patched function
    assert bnn.fused_rmsnorm_calls()["forward"] == c0["forward"] + 2 and torch.equal(y, fused(x))

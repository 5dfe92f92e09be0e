"""betty_amd.nn.FusedGroupNorm: the two-node autograd graph (_GNForward / _GNBackward) and the module around it.

CPU part: the float64 restatement tests/groupnorm_ref.py is swapped in through the `_GN_VJP_IMPL` test hook, and the graph is held to
plain nn.GroupNorm in float64: equal first gradients, the double backward to 1e-10 of max|want| (1e-8 where a row has fewer than 4
elements: tests/test_groupnorm_ref.py), absent cotangents, an input that needs no gradient, affine=False, re-classing.

GPU part: the module against nn.GroupNorm on the same GPU (the first gradient equal to the bit to nn.GroupNorm's ordinary backward, the
one without create_graph; one Hessian-vector product against the same problem's float64 product: the declared error at most four times
the undeclared fp32 error, DESIGN 3.27's rule, or within 2e-5 of max|want|); a cg and a neumann hypergradient (K = 5) of a small
Conv -> GroupNorm -> ReLU -> Conv -> GroupNorm -> pool -> Linear net on 48 samples of 3 x 8 x 8 under the meta-weight-net upper problem
of tests/test_fused_layernorm.py, declared against undeclared at the package's parity gate (rtol 1e-4), one fused call per layer and
product; and the inputs that take nn.GroupNorm's own path."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import groupnorm_ref
import zoo
from conftest import rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4          # the package's parity gate (hypergradients)
FP64_GATE, FP64_GATE_SHORT = 1e-10, 1e-8   # the graph on the CPU in float64 against nn.GroupNorm's own double backward (rows of >= 4 / fewer elements)


def _ref_impl(x, gy, a, gamma, mean, rstd, b, c, G):
    """tests/groupnorm_ref.py behind the signature of nn._gn_vjp_hip."""
    return groupnorm_ref.groupnorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c, G)


@pytest.fixture
def restatement():
    """The float64 restatement in place of the HIP call, and a record of the cotangents each call received."""
    seen = []

    def impl(x, gy, a, gamma, mean, rstd, b, c, G):
        seen.append((a is not None, b is not None, c is not None))
        return _ref_impl(x, gy, a, gamma, mean, rstd, b, c, G)

    was = bnn._GN_VJP_IMPL[0]
    bnn._GN_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._GN_VJP_IMPL[0] = was


def _layer(G, C, affine=True):
    torch.manual_seed(5)
    gn = nn.GroupNorm(G, C, affine=affine).double()
    with torch.no_grad():
        for p in gn.parameters():
            p.normal_()
    return gn


def _declared(gn):
    return lambda t: bnn._GNForward.apply(t, gn.weight, gn.bias, gn.num_groups, gn.eps)


def _grad_and_hvp(gn, apply, x):
    """Gradient of a non-quadratic loss through the layer and one Hessian-vector product, with respect to the input and the layer's parameters."""
    x = x.clone().requires_grad_(True)
    leaves = [x] + list(gn.parameters())
    g = torch.Generator().manual_seed(11)
    vec = [torch.randn(p.shape, generator=g, dtype=p.dtype) for p in leaves]
    y = apply(x)
    loss = (y ** 3).sum() + (y[:, :1] * y).sum()
    grads = torch.autograd.grad(loss, leaves, create_graph=True)
    return grads, torch.autograd.grad(grads, leaves, grad_outputs=vec)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "no_affine"])
@pytest.mark.parametrize("shape,G", [((5, 6), 2), ((2, 6, 3), 2), ((3, 4, 2, 2), 1), ((2, 5, 7), 5), ((4, 6), 2)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"G{v}")
def test_two_node_graph_matches_nn_groupnorm_fp64(restatement, shape, G, affine):
    gn = _layer(G, shape[1], affine)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    c0 = bnn.fused_groupnorm_calls()
    want = _grad_and_hvp(gn, gn, x)
    assert bnn.fused_groupnorm_calls() == c0                                # plain nn.GroupNorm: no node of ours
    got = _grad_and_hvp(gn, _declared(gn), x)
    calls = {k: v - c0[k] for k, v in bnn.fused_groupnorm_calls().items()}
    assert calls["forward"] == 1 and calls["backward_vjp"] == 1 and len(restatement) == 1, calls
    D = x.numel() // (shape[0] * G)
    gate = FP64_GATE if D >= 4 else FP64_GATE_SHORT
    for u, v in zip(got[0], want[0]):
        # native_group_norm_backward against the decomposition ATen runs under create_graph: equal to rounding, at the same gate (to the
        # bit against the backward ATen runs without create_graph: the next test)
        assert float((u - v).detach().abs().max()) <= gate * float(v.detach().abs().max()), (shape, G, affine)
    for u, v in zip(got[1], want[1]):
        assert float((u - v).abs().max()) <= gate * float(v.abs().max()), (shape, G, affine)


def test_first_gradient_is_native_group_norm_backward_to_the_bit():
    """Without create_graph nn.GroupNorm runs native_group_norm_backward: the declared node runs the same kernel."""
    gn = _layer(2, 6)
    x = torch.randn(3, 6, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    outs = []
    for apply in (gn, _declared(gn)):
        t = x.clone().requires_grad_(True)
        outs.append(torch.autograd.grad((apply(t) ** 3).sum(), [t, gn.weight, gn.bias]))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_absent_cotangents_arrive_as_none(restatement):
    gn = _layer(2, 6)
    x = torch.randn(3, 6, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)

    def firsts(layer):
        y = layer(x)
        return torch.autograd.grad((y ** 2).sum(), [x, gn.weight, gn.bias], create_graph=True)

    for pick, present in ((0, (True, False, False)), (1, (False, True, False)), (2, (False, False, True))):
        del restatement[:]
        got = torch.autograd.grad(firsts(_declared(gn))[pick].sum(), [x, gn.weight], allow_unused=True)
        want = torch.autograd.grad(firsts(gn)[pick].sum(), [x, gn.weight], allow_unused=True)
        assert restatement == [present], (pick, restatement)
        for u, v in zip(got, want):
            u = torch.zeros(()) if u is None else u
            v = torch.zeros(()) if v is None else v
            assert float((u - v).abs().max()) <= FP64_GATE * max(float(v.abs().max()), 1.0), pick


def test_an_input_that_needs_no_gradient(restatement):
    gn = _layer(2, 6)
    x = torch.randn(3, 6, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    outs = []
    for apply in (gn, _declared(gn)):
        params = list(gn.parameters())
        grads = torch.autograd.grad((apply(x) ** 3).sum(), params, create_graph=True)
        outs.append(torch.autograd.grad(grads, params, grad_outputs=[torch.ones_like(p) for p in params]))
    for u, v in zip(outs[1], outs[0]):
        assert float((u - v).abs().max()) <= FP64_GATE * float(v.abs().max())
    assert restatement == [(False, True, True)]


class _Net(nn.Module):
    """Conv -> GroupNorm -> ReLU -> Conv -> GroupNorm -> pool -> Linear."""

    def __init__(self, classes=5):
        super().__init__()
        self.conv1, self.norm1 = nn.Conv2d(3, 8, 3, padding=1), nn.GroupNorm(2, 8)
        self.conv2, self.norm2 = nn.Conv2d(8, 12, 3, padding=1), nn.GroupNorm(4, 12)
        self.head = nn.Linear(12, classes)

    def forward(self, x):
        h = F.relu(self.norm1(self.conv1(x)))
        h = self.norm2(self.conv2(h))
        return self.head(h.mean(dim=(2, 3)))


def test_fuse_groupnorm_changes_only_the_class():
    torch.manual_seed(0)
    net = nn.Sequential(_Net(), nn.GroupNorm(1, 5, affine=False), nn.LayerNorm(5))

    class Mine(nn.GroupNorm):
        pass

    net.add_module("mine", Mine(1, 5))
    keys, values = list(net.state_dict()), [v.clone() for v in net.state_dict().values()]
    ids = [id(p) for p in net.parameters()]
    assert bnn.fuse_groupnorm_(net) == 3
    assert type(net[0].norm1) is type(net[0].norm2) is type(net[1]) is bnn.FusedGroupNorm and type(net.mine) is Mine and type(net[2]) is nn.LayerNorm
    assert list(net.state_dict()) == keys and [id(p) for p in net.parameters()] == ids
    assert all(torch.equal(u, v) for u, v in zip(net.state_dict().values(), values))
    assert bnn.fuse_groupnorm_(net) == 0
    x = torch.randn(4, 3, 8, 8)
    plain = _Net()
    plain.load_state_dict(net[0].state_dict())
    c0 = bnn.fused_groupnorm_calls()
    assert torch.equal(net[0](x), plain(x)) and bnn.fused_groupnorm_calls() == c0      # a CPU input IS nn.GroupNorm
    said = []
    for layer in (net[0].norm1, plain.norm1):                                           # and nn.GroupNorm's own error for a wrong channel count
        with pytest.raises(RuntimeError) as exc:
            layer(torch.randn(2, 7, 4))
        said.append(str(exc.value))
    assert said[0] == said[1]


def test_declare_layers_default_keys_are_unchanged():
    net = nn.Sequential(_Net(), nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=False), nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4), nn.LayerNorm(4))
    assert bnn.declare_layers_(net) == {"batchnorm": 1, "pointwise_conv": 1}
    assert type(net[0].norm1) is nn.GroupNorm
    assert bnn.declare_layers_(net, depthwise=True, layernorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "depthwise_conv": 1, "layernorm": 1}
    assert type(net[0].norm1) is nn.GroupNorm
    assert bnn.declare_layers_(net, groupnorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "groupnorm": 2}
    assert type(net[0].norm1) is type(net[0].norm2) is bnn.FusedGroupNorm
    assert bnn.declare_layers_(net, depthwise=True, layernorm=True, groupnorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "depthwise_conv": 0,
                                                                                       "layernorm": 0, "groupnorm": 0}


def test_the_hip_call_refuses_cpu_tensors():
    from betty_amd import _native

    t = torch.zeros(2, 4, 3)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._gn_vjp_hip(t, t, t, None, torch.zeros(2, 2), torch.ones(2, 2), None, None, 2)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
def _net_grad_and_hvp(declared, dtype=torch.float32, create_graph=True):
    torch.manual_seed(1)
    net = _Net().to(DEV)
    if declared:
        assert bnn.fuse_groupnorm_(net) == 2
    net = net.to(dtype)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(48, 3, 8, 8, generator=g).to(DEV, dtype), torch.randint(0, 5, (48,), generator=g).to(DEV)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV, dtype) for p in params]
    c0 = bnn.fused_groupnorm_calls()
    grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=create_graph)
    if not create_graph:
        return [t.detach() for t in grads], None
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    calls = {k: v - c0[k] for k, v in bnn.fused_groupnorm_calls().items()}
    live = 2 if declared and dtype == torch.float32 else 0
    assert calls["backward_vjp"] == live and calls["forward"] == live, calls   # one fused call per layer and product
    return [t.detach() for t in grads], [t.detach() for t in hv]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,G,affine", [((6, 8, 5, 5), 2, True), ((4, 12, 7), 4, True), ((5, 6), 3, True), ((3, 8, 4, 4), 8, False),
                                            ((2, 4, 64, 65), 2, True)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_module_first_gradient_equals_nn_groupnorms_ordinary_backward_to_the_bit(shape, G, affine):
    """nn.GroupNorm's ordinary backward (no create_graph) is native_group_norm_backward; under create_graph ATen replaces it by a
    decomposition.  The declared layer runs the single kernel in both cases: the same bits as the ordinary backward, and the same output."""
    torch.manual_seed(2)
    fused, ref = bnn.FusedGroupNorm(G, shape[1], affine=affine).to(DEV), nn.GroupNorm(G, shape[1], affine=affine).to(DEV)
    if affine:
        with torch.no_grad():
            fused.weight.normal_()
            fused.bias.normal_()
    ref.load_state_dict(fused.state_dict())
    x = torch.randn(shape, device=DEV)

    def first(layer, create_graph):
        t = x.clone().requires_grad_(True)
        y = layer(t)
        return [y.detach()] + [v.detach() for v in torch.autograd.grad((y ** 3).sum(), [t] + list(layer.parameters()), create_graph=create_graph)]

    c0 = bnn.fused_groupnorm_calls()
    ordinary = first(ref, False)
    assert bnn.fused_groupnorm_calls() == c0
    for create_graph in (True, False):
        for u, v in zip(first(fused, create_graph), ordinary):
            assert torch.equal(u, v), create_graph
    assert bnn.fused_groupnorm_calls()["forward"] == c0["forward"] + 2


@pytest.mark.gpu
def test_module_hvp_within_the_fp32_error_of_the_float64_product():
    ordinary = _net_grad_and_hvp(False, create_graph=False)[0]            # nn.GroupNorm's ordinary backward: native_group_norm_backward
    plain, declared = _net_grad_and_hvp(False), _net_grad_and_hvp(True)
    # the whole net's first gradient: the other layers' backward kernels are not this layer's to pin, so to rounding here (to the bit for
    # the layer alone: the test above)
    rel, _ = rel_err([t.cpu().numpy() for t in declared[0]], [t.cpu().numpy() for t in ordinary])
    print(f"FusedGroupNorm net, first gradient under create_graph vs nn.GroupNorm's ordinary backward: {rel:.2e} of the norm; "
          f"bit-equal tensors: {[bool(torch.equal(u, v)) for u, v in zip(declared[0], ordinary)]}")
    assert rel <= 1e-6, rel
    exact = [t.cpu().numpy() for t in _net_grad_and_hvp(False, torch.float64)[1]]
    _, e_plain = rel_err([t.cpu().numpy() for t in plain[1]], exact)
    _, e_decl = rel_err([t.cpu().numpy() for t in declared[1]], exact)
    print(f"FusedGroupNorm vs the float64 product (max|diff| / max|want|): declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


def _problem(declared, algo, K=5):
    torch.manual_seed(3)
    inner, upper = _Net().to(DEV), zoo.MWN(8).to(DEV)
    if declared:
        assert bnn.declare_layers_(inner, groupnorm=True) == {"batchnorm": 0, "pointwise_conv": 0, "groupnorm": 2}
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(48, 3, 8, 8, generator=g).to(DEV), torch.randint(0, 5, (48,), generator=g).to(DEV)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_declared_groupnorm_matches_the_undeclared_problem(algo):
    out = {}
    for declared in (False, True):
        curr, prev, vector = _problem(declared, algo)
        c0 = bnn.fused_groupnorm_calls()
        res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[declared] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.fused_groupnorm_calls()["backward_vjp"] - c0["backward_vjp"]
        # one fused call per layer and product: two layers, the K = 5 Hessian-vector products of the solve and the mixed second derivative
        # that closes it (the meta-weight net enters through the loss: one more double backward through the inner network)
        assert calls == (2 * (5 + 1) if declared else 0), calls
    rel, _ = rel_err(out[True], out[False])
    print(f"{algo} hypergradient (K = 5), group norm declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel


@pytest.mark.gpu
def test_forward_over_reverse_on_a_declared_net_falls_back_to_the_double_backward_with_its_warning():
    """Custom Functions have no forward-mode formula: as documented for declared layer norm, the first forward-over-reverse pass fails, the
    solve warns and continues on the double backward — through the fused calls — and gives the default's answer."""
    out = {}
    for mode in (None, "forward_over_reverse"):
        curr, prev, vector = _problem(True, "neumann")
        c0 = bnn.fused_groupnorm_calls()["backward_vjp"]
        if mode:
            curr.hypergradient_hvp = mode
            with pytest.warns(RuntimeWarning, match="forward-over-reverse HVP not available"):
                res = hg.neumann(vector, curr, prev, False)
        else:
            res = hg.neumann(vector, curr, prev, False)
        out[mode] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.fused_groupnorm_calls()["backward_vjp"] - c0
        print(f"neumann (K = 5) on the declared net, hypergradient_hvp = {mode}: {calls} fused calls")
        assert calls == 2 * (5 + 1), (mode, calls)
    rel, _ = rel_err(out["forward_over_reverse"], out[None])
    assert rel <= 1e-5, rel


@pytest.mark.gpu
def test_float64_noncontiguous_no_grad_and_long_row_inputs_take_nn_groupnorms_path():
    torch.manual_seed(0)
    c0 = bnn.fused_groupnorm_calls()

    def pair(G, C, dtype=torch.float32):
        fused, ref = bnn.FusedGroupNorm(G, C).to(DEV, dtype), nn.GroupNorm(G, C).to(DEV, dtype)
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

    fused, ref = pair(2, 8, torch.float64)
    assert same_bits(fused, ref, torch.randn(6, 8, 5, device=DEV, dtype=torch.float64))
    fused, ref = pair(2, 8)
    assert same_bits(fused, ref, torch.randn(6, 8, 10, device=DEV)[:, :, ::2])                    # non-contiguous
    assert same_bits(fused, ref, torch.randn(6, 9, 5, device=DEV)[:, 1:])                         # samples not contiguous, 4-byte aligned
    fused_w, ref_w = pair(1, 2)
    assert same_bits(fused_w, ref_w, torch.randn(2, 2, 2 ** 19 + 1, device=DEV))                  # D = 2^20 + 2 > 2^20
    x = torch.randn(6, 8, 5, device=DEV)
    with torch.no_grad():
        assert torch.equal(fused(x), ref(x))
    assert bnn.fused_groupnorm_calls() == c0
    y = fused(x.requires_grad_(True))                                                             # and the declared route is live for the plain input
    assert bnn.fused_groupnorm_calls()["forward"] == c0["forward"] + 1 and torch.equal(y, ref(x))

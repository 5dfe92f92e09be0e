"""betty_amd.nn's declared activations: the two-node autograd graphs (_ActForward / _ActBackward, _GatedActForward / _GatedActBackward),
the functions, the re-classed modules and the context manager around them.

CPU part: the float64 restatement tests/activation_ref.py is swapped in through the `_ACT_VJP_IMPL` test hook, and the graphs are held to
the plain torch functions in float64: first gradients, the double backward to 1e-10 of max|want|, absent cotangents, an input that needs
no gradient, re-classing, the TransformerEncoderLayer.activation swap, declare_layers_'s default keys, the context manager, and the inputs
that take the torch path.

GPU part: output and first gradient equal to the bit to the torch function's ordinary backward; one Hessian-vector product of
Linear(24, 32) -> act -> Linear(32, 10) on 48 samples per kind, of a SwiGLU block, of nn.GLU and of an nn.TransformerEncoderLayer against
the same problem's float64 product (the declared error at most four times the undeclared fp32 error, DESIGN 3.27's rule, or within 2e-5
of max|want|), one fused call per activation and product; a cg and a neumann hypergradient (K = 5) of a tanh MLP under the
meta-weight-net upper problem, declared against undeclared at the package's parity gate (1e-4), K + 1 fused calls per activation."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

import activation_ref as ref
import zoo
from conftest import rel_err

from betty_amd import Config, _native
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4          # the package's parity gate (hypergradients)
FP64_GATE = 1e-10    # the graph on the CPU in float64 against autograd's own double backward
PLAIN = [(k, 1.0, 20.0) for k in ref.KINDS[:5]] + [("softplus", 1.0, 20.0), ("softplus", 2.0, 5.0)]


@pytest.fixture
def restatement():
    """The restatement in place of the HIP call, and a record of (form, kind, which inputs were given, which outputs were wanted)."""
    seen = []

    def impl(form, kind, ins, need, beta=1.0, threshold=20.0):
        seen.append((form, kind, tuple(t is not None for t in ins), tuple(need)))
        if form == "plain":
            out = ref.act_backward_vjp(kind, *ins, beta, threshold)
        elif form == "glu":
            out = ref.glu_backward_vjp(*ins)
        else:
            out = ref.gated_backward_vjp(kind, *ins)
        return tuple(t if on else None for t, on in zip(out, need))

    was = bnn._ACT_VJP_IMPL[0]
    bnn._ACT_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._ACT_VJP_IMPL[0] = was


def _grad_and_hvp(apply, leaves, seed=11):
    """First gradients of a non-quadratic loss through `apply(*leaves)` under create_graph, and one Hessian-vector product."""
    leaves = [t.clone().requires_grad_(t.requires_grad) for t in leaves]
    live = [t for t in leaves if t.requires_grad]
    g = torch.Generator().manual_seed(seed)
    grads = torch.autograd.grad((apply(*leaves) ** 3).sum(), live, create_graph=True)
    vec = [torch.randn(t.shape, generator=g, dtype=t.dtype) for t in live]
    hv = torch.autograd.grad(grads, live, grad_outputs=vec)
    return [t.detach() for t in grads], [t.detach() for t in hv]


def _assert_close(got, want, gate):
    for u, v in zip(got, want):
        assert float((u - v).abs().max()) <= gate * float(v.abs().max()), float((u - v).abs().max()) / float(v.abs().max())


# ---- on the CPU, in float64, with the restatement swapped in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,beta,threshold", PLAIN, ids=lambda v: str(v))
def test_plain_graph_against_the_torch_function_in_float64(restatement, kind, beta, threshold):
    x = ref.softplus_safe(3.0 * torch.randn(6, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(1)), beta, threshold).requires_grad_(True)
    c0 = bnn.declared_activation_calls()
    want = _grad_and_hvp(ref.torch_function(kind, beta, threshold), [x])
    assert bnn.declared_activation_calls() == c0                    # the torch function: no node of ours
    got = _grad_and_hvp(lambda t: bnn._ActForward.apply(t, kind, beta, threshold), [x])
    calls = {k: v - c0[k] for k, v in bnn.declared_activation_calls().items()}
    # (the first-backward node runs twice: dgy flows on through the loss's dependence on y)
    assert calls["forward"] == 1 and calls["backward_vjp"] == 1, calls
    assert restatement == [("plain", kind, (True, True, True), (True, True))], restatement
    _assert_close(got[0], want[0], 1e-14)
    _assert_close(got[1], want[1], FP64_GATE)


def test_glu_graph_against_the_torch_function_in_float64(restatement):
    x = torch.randn(5, 3, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    want = _grad_and_hvp(lambda t: F.glu(t, -1), [x])
    got = _grad_and_hvp(lambda t: bnn._ActForward.apply(t, "glu", 1.0, 20.0), [x])
    assert restatement == [("glu", "glu", (True, True, True), (True, True))], restatement
    _assert_close(got[0], want[0], 1e-14)
    _assert_close(got[1], want[1], FP64_GATE)


@pytest.mark.parametrize("kind", ref.GATED_KINDS)
def test_gated_graph_against_the_torch_expression_in_float64(restatement, kind):
    g = torch.Generator().manual_seed(3)
    u, v = (torch.randn(7, 6, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(2))
    want = _grad_and_hvp(lambda a, b: ref.torch_function(kind)(a) * b, [u, v])
    got = _grad_and_hvp(lambda a, b: bnn._GatedActForward.apply(a, b, kind), [u, v])
    assert restatement == [("gated", kind, (True,) * 5, (True, True, True))], restatement
    _assert_close(got[0], want[0], 1e-14)
    _assert_close(got[1], want[1], FP64_GATE)


def test_absent_cotangents_and_an_input_that_needs_no_gradient(restatement):
    g = torch.Generator().manual_seed(4)
    u, v = (torch.randn(4, 6, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(2))

    def firsts(apply, a, b):
        return torch.autograd.grad((apply(a, b) ** 3).sum(), [a, b], create_graph=True)

    plain = lambda a, b: F.silu(a) * b                               # noqa: E731
    ours = lambda a, b: bnn._GatedActForward.apply(a, b, "silu")     # noqa: E731
    for pick, given in ((0, (True, False)), (1, (False, True))):    # a loss of gu alone, of gv alone: the other cotangent is None
        del restatement[:]
        got = torch.autograd.grad(firsts(ours, u, v)[pick].sum(), [u, v], allow_unused=True)
        want = torch.autograd.grad(firsts(plain, u, v)[pick].sum(), [u, v], allow_unused=True)
        assert [r[2][3:] for r in restatement] == [given], restatement
        for a, b in zip(got, want):
            if b is None:
                assert a is None or not a.any()
            else:
                _assert_close([a], [b], FP64_GATE)
    # `up` needs no gradient: its outputs are not asked for, and None comes back
    del restatement[:]
    w = v.detach()
    got = _grad_and_hvp(ours, [u, w])
    want = _grad_and_hvp(plain, [u, w])
    assert [r[3] for r in restatement] == [(True, False, True)], restatement
    _assert_close(got[0], want[0], 1e-14)
    _assert_close(got[1], want[1], FP64_GATE)
    # the plain form with an input that needs no gradient records no graph at all
    c0 = bnn.declared_activation_calls()
    y = bnn._ActForward.apply(w, "tanh", 1.0, 20.0)
    assert not y.requires_grad and bnn.declared_activation_calls()["backward"] == c0["backward"]


def test_no_call_at_all_when_every_cotangent_is_none(restatement):
    class Ctx:
        needs_input_grad = (True, True, True, False, False, False)
        saved_tensors = (torch.zeros(3), torch.zeros(3), torch.zeros(3))

    c0 = bnn.declared_activation_calls()
    assert bnn._ActBackward.backward(Ctx(), None) == (None,) * 6
    assert bnn._GatedActBackward.backward(Ctx(), None, None) == (None,) * 5
    assert restatement == [] and bnn.declared_activation_calls() == c0


class _Mine(nn.GELU):
    pass


def _zoo_of_activations():
    return nn.Sequential(nn.Linear(8, 8), nn.GELU(), nn.GELU(approximate="tanh"), nn.SiLU(), nn.Tanh(), nn.Sigmoid(), nn.Softplus(2.0, 5.0),
                         nn.GLU(), nn.Linear(4, 4), nn.SiLU(inplace=True), nn.GLU(dim=0), _Mine(), nn.ReLU())


def test_declare_activations_changes_only_the_class():
    torch.manual_seed(0)
    net = _zoo_of_activations()
    keys, values = list(net.state_dict()), [v.clone() for v in net.state_dict().values()]
    ids = [id(p) for p in net.parameters()]
    assert bnn.declare_activations_(net) == 7
    assert [type(m) for m in net] == [nn.Linear, bnn.DeclaredGELU, bnn.DeclaredGELU, bnn.DeclaredSiLU, bnn.DeclaredTanh, bnn.DeclaredSigmoid,
                                      bnn.DeclaredSoftplus, bnn.DeclaredGLU, nn.Linear, nn.SiLU, nn.GLU, _Mine, nn.ReLU]
    assert (net[2].approximate, net[6].beta, net[6].threshold, net[7].dim) == ("tanh", 2.0, 5.0, -1)
    assert list(net.state_dict()) == keys and [id(p) for p in net.parameters()] == ids
    assert all(torch.equal(u, v) for u, v in zip(net.state_dict().values(), values))
    assert bnn.declare_activations_(net) == 0
    plain = _zoo_of_activations()
    plain.load_state_dict(net.state_dict())
    x = torch.randn(4, 8)
    c0 = bnn.declared_activation_calls()
    assert torch.equal(net(x), plain(x)) and bnn.declared_activation_calls() == c0     # a CPU input IS the torch function


def test_the_transformer_layers_activation_is_swapped():
    enc = nn.TransformerEncoderLayer(16, 2, 16, dropout=0.0, activation="gelu", batch_first=True)
    dec = nn.TransformerDecoderLayer(16, 2, 16, dropout=0.0, activation=F.gelu, batch_first=True)
    relu = nn.TransformerEncoderLayer(16, 2, 16, dropout=0.0, batch_first=True)
    net = nn.ModuleList([enc, dec, relu])
    assert enc.activation is F.gelu and dec.activation is F.gelu
    assert bnn.declare_activations_(net) == 2
    assert enc.activation is bnn.gelu and dec.activation is bnn.gelu and relu.activation is F.relu
    x = torch.randn(2, 5, 16)
    fresh = nn.TransformerEncoderLayer(16, 2, 16, dropout=0.0, activation="gelu", batch_first=True)
    fresh.load_state_dict(enc.state_dict())
    assert torch.equal(enc(x), fresh(x))


def test_declare_layers_default_keys_are_unchanged():
    net = nn.Sequential(nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4), nn.GELU(), nn.Tanh())
    assert bnn.declare_layers_(net) == {"batchnorm": 1, "pointwise_conv": 1}
    assert type(net[2]) is nn.GELU and type(net[3]) is nn.Tanh
    assert bnn.declare_layers_(net, activations=True) == {"batchnorm": 0, "pointwise_conv": 0, "activations": 2}
    assert type(net[2]) is bnn.DeclaredGELU and type(net[3]) is bnn.DeclaredTanh


def test_the_context_manager_restores_the_torch_functions():
    torch_fns = (F.gelu, F.silu, F.softplus, F.glu)
    assert torch_fns == (bnn._TORCH_GELU, bnn._TORCH_SILU, bnn._TORCH_SOFTPLUS, bnn._TORCH_GLU)
    with bnn.declared_activations():
        assert (F.gelu, F.silu, F.softplus, F.glu) == (bnn.gelu, bnn.silu, bnn.softplus, bnn.glu)
        with bnn.declared_activations():
            assert F.gelu is bnn.gelu
        assert (F.gelu, F.silu, F.softplus, F.glu) == (bnn.gelu, bnn.silu, bnn.softplus, bnn.glu)      # the inner exit restores the outer state
        x = torch.randn(3, 4)
        assert torch.equal(nn.GELU()(x), bnn._TORCH_GELU(x)) and torch.equal(nn.GLU()(x), bnn._TORCH_GLU(x))
    assert (F.gelu, F.silu, F.softplus, F.glu) == torch_fns
    with pytest.raises(ZeroDivisionError):
        with bnn.declared_activations():
            1 / 0
    assert (F.gelu, F.silu, F.softplus, F.glu) == torch_fns


def _same_bits(ours, theirs, x, view=lambda t: t):
    outs = []
    for fn in (ours, theirs):
        t = x.detach().clone().requires_grad_(True)
        y = fn(view(t))
        outs.append((y.detach(), torch.autograd.grad((y ** 2).sum(), t)[0]))
    return torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _out_of_family_inputs_take_the_torch_path(device):
    torch.manual_seed(0)
    c0 = bnn.declared_activation_calls()
    pairs = [(bnn.gelu, F.gelu), (lambda t: bnn.gelu(t, approximate="tanh"), lambda t: F.gelu(t, approximate="tanh")), (bnn.silu, F.silu),
             (bnn.tanh, torch.tanh), (bnn.sigmoid, torch.sigmoid), (lambda t: bnn.softplus(t, 2.0, 5.0), lambda t: F.softplus(t, 2.0, 5.0)),
             (bnn.glu, F.glu), (lambda t: bnn.gated_activation(t, t), lambda t: F.silu(t) * t)]
    for ours, theirs in pairs:
        assert _same_bits(ours, theirs, torch.randn(6, 8, device=device, dtype=torch.float64))        # float64
        assert _same_bits(ours, theirs, torch.randn(6, 16, device=device), view=lambda t: t[:, ::2])   # non-contiguous
        x = torch.randn(6, 8, device=device)
        with torch.no_grad():
            assert torch.equal(ours(x), theirs(x))                                                     # grad disabled
    x = torch.randn(6, 8, device=device)
    assert _same_bits(lambda t: bnn.silu(t * 1.0, inplace=True), lambda t: F.silu(t * 1.0, inplace=True), x)
    assert _same_bits(lambda t: bnn.glu(t, 0), lambda t: F.glu(t, 0), x)                               # glu on dimension 0
    assert _same_bits(lambda t: bnn.DeclaredGLU(0)(t), lambda t: F.glu(t, 0), x)
    said = []
    for fn in (bnn.glu, F.glu):                                                                         # an odd last dimension: F.glu's own error
        with pytest.raises(RuntimeError) as exc:
            fn(torch.randn(4, 7, device=device, requires_grad=True))
        said.append(str(exc.value))
    assert said[0] == said[1]
    with pytest.raises(ValueError, match="activation must be one of"):
        bnn.gated_activation(x, x, "softplus")
    assert bnn.declared_activation_calls() == c0


def test_out_of_family_inputs_take_the_torch_path_on_the_cpu():
    _out_of_family_inputs_take_the_torch_path("cpu")


def test_the_hip_call_refuses_cpu_tensors():
    t = torch.zeros(2, 4)
    for form, ins in (("plain", (t, t, t)), ("glu", (t, t[:, :2], t)), ("gated", (t, t, t, t, None))):
        with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
            bnn._act_vjp_hip(form, "silu", ins, (True,) * (3 if form == "gated" else 2))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_out_of_family_inputs_take_the_torch_path_on_the_gpu():
    _out_of_family_inputs_take_the_torch_path(DEV)
    c0 = bnn.declared_activation_calls()
    x = torch.randn(6, 8, device=DEV, requires_grad=True)                                              # and the declared route is live
    assert torch.equal(bnn.gelu(x), F.gelu(x)) and bnn.declared_activation_calls()["forward"] == c0["forward"] + 1


FIRST = [("gelu", bnn.gelu, F.gelu), ("gelu_tanh", lambda t: bnn.gelu(t, approximate="tanh"), lambda t: F.gelu(t, approximate="tanh")),
         ("silu", bnn.silu, F.silu), ("tanh", bnn.tanh, torch.tanh), ("sigmoid", bnn.sigmoid, torch.sigmoid),
         ("softplus", bnn.softplus, F.softplus), ("softplus_2_5", lambda t: bnn.softplus(t, 2.0, 5.0), lambda t: F.softplus(t, 2.0, 5.0)),
         ("glu", bnn.glu, F.glu)] + \
        [(f"gated_{k}", (lambda k: lambda t: bnn.gated_activation(t, t.flip(0) + 0.5, k))(k),
          (lambda k: lambda t: ref.torch_function(k)(t) * (t.flip(0) + 0.5))(k)) for k in ref.GATED_KINDS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ours,theirs", FIRST, ids=[f[0] for f in FIRST])
def test_output_and_first_gradient_equal_the_torch_functions_ordinary_backward_to_the_bit(name, ours, theirs):
    x = 3.0 * torch.randn(33, 10, device=DEV, generator=torch.Generator(DEV).manual_seed(2))

    def first(fn, create_graph):
        t = x.clone().requires_grad_(True)
        y = fn(t)
        return [y.detach(), torch.autograd.grad((y ** 3).sum(), t, create_graph=create_graph)[0].detach()]

    c0 = bnn.declared_activation_calls()
    ordinary = first(theirs, False)
    assert bnn.declared_activation_calls() == c0
    for create_graph in (True, False):
        for u, v in zip(first(ours, create_graph), ordinary):
            assert torch.equal(u, v), (name, create_graph)
    assert bnn.declared_activation_calls()["forward"] == c0["forward"] + 2


class _SwiGLU(nn.Module):
    def __init__(self, declared):
        super().__init__()
        self.gate, self.up, self.down, self.declared = nn.Linear(24, 32), nn.Linear(24, 32), nn.Linear(32, 10), declared

    def forward(self, x):
        g, u = self.gate(x), self.up(x)
        return self.down(bnn.gated_activation(g, u, "silu") if self.declared else F.silu(g) * u)


def _mlp(act):
    return nn.Sequential(nn.Linear(24, 32), act, nn.Linear(32, 10))


NETS = {"gelu": lambda d: _mlp(nn.GELU()), "gelu_tanh": lambda d: _mlp(nn.GELU(approximate="tanh")), "silu": lambda d: _mlp(nn.SiLU()),
        "tanh": lambda d: _mlp(nn.Tanh()), "sigmoid": lambda d: _mlp(nn.Sigmoid()), "softplus": lambda d: _mlp(nn.Softplus()),
        "softplus_2_5": lambda d: _mlp(nn.Softplus(2.0, 5.0)), "glu": lambda d: nn.Sequential(nn.Linear(24, 64), nn.GLU(), nn.Linear(32, 10)),
        "swiglu": _SwiGLU}


def _net_hvp(name, declared, dtype=torch.float32):
    torch.manual_seed(1)
    net = NETS[name](declared).to(DEV)
    if declared and name != "swiglu":
        assert bnn.declare_activations_(net) == 1
    net = net.to(dtype)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(48, 24, generator=g).to(DEV, dtype), torch.randint(0, 10, (48,), generator=g).to(DEV)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV, dtype) for p in params]
    c0 = bnn.declared_activation_calls()
    grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    calls = {k: v - c0[k] for k, v in bnn.declared_activation_calls().items()}
    live = 1 if declared and dtype == torch.float32 else 0
    assert calls["forward"] == live and calls["backward_vjp"] == live, calls              # one fused call per activation and product
    return [t.detach().cpu().numpy() for t in hv]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_hvp_within_the_fp32_error_of_the_float64_product(name):
    exact = _net_hvp(name, False, torch.float64)
    _, e_plain = rel_err(_net_hvp(name, False), exact)
    _, e_decl = rel_err(_net_hvp(name, True), exact)
    print(f"declared {name} vs the float64 product (max|diff| / max|want|): declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


def _encoder_hvp(declared, dtype=torch.float32):
    torch.manual_seed(4)
    layer = nn.TransformerEncoderLayer(64, 4, 64, dropout=0.0, activation="gelu", batch_first=True, norm_first=True).to(DEV)
    if declared:
        assert bnn.declare_activations_(layer) == 1
    layer = layer.to(dtype)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 10, 64, generator=g).to(DEV, dtype)
    params = list(layer.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV, dtype) for p in params]
    c0 = bnn.declared_activation_calls()
    with sdpa_kernel(SDPBackend.MATH):
        grads = torch.autograd.grad((layer(x) ** 2).mean(), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    assert bnn.declared_activation_calls()["backward_vjp"] - c0["backward_vjp"] == (1 if declared and dtype == torch.float32 else 0)
    return [t.detach().cpu().numpy() for t in hv]


@pytest.mark.gpu
def test_transformer_encoder_layer_hvp_runs_one_fused_call():
    exact = _encoder_hvp(False, torch.float64)
    _, e_plain = rel_err(_encoder_hvp(False), exact)
    _, e_decl = rel_err(_encoder_hvp(True), exact)
    print(f"TransformerEncoderLayer, gelu declared vs the float64 product: declared {e_decl:.2e}, undeclared fp32 {e_plain:.2e}")
    assert e_decl <= 4.0 * e_plain or e_decl <= 2e-5, (e_decl, e_plain)


N_ACT = 2


def _problem(declared, algo, K=5):
    torch.manual_seed(3)
    inner = nn.Sequential(nn.Linear(24, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 5)).to(DEV)
    upper = zoo.MWN(8).to(DEV)
    if declared:
        assert bnn.declare_layers_(inner, activations=True) == {"batchnorm": 0, "pointwise_conv": 0, "activations": N_ACT}
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(48, 24, generator=g).to(DEV), torch.randint(0, 5, (48,), generator=g).to(DEV)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_declared_tanh_matches_the_undeclared_problem(algo):
    out = {}
    for declared in (False, True):
        curr, prev, vector = _problem(declared, algo)
        c0 = bnn.declared_activation_calls()
        res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[declared] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.declared_activation_calls()["backward_vjp"] - c0["backward_vjp"]
        # one fused call per activation and product: the K = 5 Hessian-vector products of the solve and the mixed second derivative
        assert calls == (N_ACT * (5 + 1) if declared else 0), calls
    rel, _ = rel_err(out[True], out[False])
    print(f"{algo} hypergradient (K = 5), tanh declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel


@pytest.mark.gpu
def test_forward_over_reverse_on_a_declared_net_falls_back_to_the_double_backward_with_its_warning():
    """Custom Functions have no forward-mode formula: as for the other declared layers, the first forward-over-reverse pass fails, the
    solve warns and continues on the double backward — through the fused calls — and gives the default's answer."""
    out = {}
    for mode in (None, "forward_over_reverse"):
        curr, prev, vector = _problem(True, "neumann")
        c0 = bnn.declared_activation_calls()["backward_vjp"]
        if mode:
            curr.hypergradient_hvp = mode
            with pytest.warns(RuntimeWarning, match="forward-over-reverse HVP not available"):
                res = hg.neumann(vector, curr, prev, False)
        else:
            res = hg.neumann(vector, curr, prev, False)
        out[mode] = [t.detach().cpu().numpy() for t in res]
        assert bnn.declared_activation_calls()["backward_vjp"] - c0 == N_ACT * (5 + 1), mode
    rel, _ = rel_err(out["forward_over_reverse"], out[None])
    assert rel <= 1e-5, rel

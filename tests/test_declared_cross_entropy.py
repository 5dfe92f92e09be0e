"""betty_amd.nn.cross_entropy: the two-node autograd graph (_CEForward / _CEBackward), the function, the module and the context manager.

CPU part: the float64 restatement tests/cross_entropy_ref.py is swapped in through the `_CE_VJP_IMPL` test hook, and the graph is held to
F.cross_entropy in float64 (loss and first gradients equal; the double backward to 1e-12 of max|want|) for the three reductions with an
ignored row, with the loss weighted by a parameter so that the gradient's own cotangent (dg) is exercised; the needs_input_grad subsets;
the context manager's restore and nesting; the module swap; every out-of-family argument reaching the torch function.

GPU part: loss and first gradient equal to the bit to F.cross_entropy's; Hessian-vector products of a linear head and a two-layer MLP at
16 x 8, 64 x 1000 and 4 x 32773 (split rows) against the same problem's float64 product: the declared error at most four times the
undeclared fp32 error (DESIGN 3.27's rule: the margin is 4), so that declared and undeclared sit within five times that error of each
other — the tolerance is measured in the test, not chosen; a cg and a neumann hypergradient (K = 5) of a small reweighting problem,
declared against undeclared at the package's parity gate (rtol 1e-4), one fused call per loss and product."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cross_entropy_ref as ref
import zoo
from conftest import rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4          # the package's parity gate (hypergradients)
FP64_GATE = 1e-12    # the graph on the CPU in float64 against F.cross_entropy's own double backward
IGNORE = -100


@pytest.fixture
def restatement():
    """The float64 restatement in place of the HIP call, and a record of which outputs each call was asked for."""
    seen = []

    def impl(lsm, y, g, a, denom, ignore_index, want):
        seen.append(tuple(want))
        dz, dg = ref.cross_entropy_backward_vjp(lsm, y, g, a, ignore_index, denom, scalar_g=g.dim() == 0)
        return (dz if want[0] else None), (dg if want[1] else None)

    was = bnn._CE_VJP_IMPL[0]
    bnn._CE_VJP_IMPL[0] = impl
    try:
        yield seen
    finally:
        bnn._CE_VJP_IMPL[0] = was


def _declared(reduction, ignore_index=IGNORE):
    return lambda z, y: bnn._CEForward.apply(z, y, reduction, ignore_index)[0]


def _undeclared(reduction, ignore_index=IGNORE):
    return lambda z, y: F.cross_entropy(z, y, reduction=reduction, ignore_index=ignore_index)


def _head_grad_and_hvp(loss_fn, reduction, dtype=torch.float64, device="cpu", N=6, D=5, C=7):
    """A linear head under a loss weighted by a parameter: loss, gradients and one Hessian-vector product with respect to (W, w)."""
    gen = torch.Generator().manual_seed(3)
    W = torch.randn(D, C, generator=gen, dtype=torch.float64).to(device, dtype).requires_grad_(True)
    w = torch.rand(N, generator=gen, dtype=torch.float64).add(0.5).to(device, dtype).requires_grad_(True)
    x = torch.randn(N, D, generator=gen, dtype=torch.float64).to(device, dtype)
    y = torch.randint(0, C, (N,), generator=gen)
    y[2] = IGNORE
    vec = [torch.randn(p.shape, generator=gen, dtype=torch.float64).to(device, dtype) for p in (W, w)]
    ce = loss_fn(x @ W, y.to(device))
    loss = (ce * w).sum() if reduction == "none" else ce * w.sum()
    grads = torch.autograd.grad(loss, (W, w), create_graph=True)
    hv = torch.autograd.grad(grads, (W, w), grad_outputs=vec)
    return loss.detach(), [t.detach() for t in grads], [t.detach() for t in hv]


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_two_node_graph_matches_f_cross_entropy_fp64(restatement, reduction):
    c0 = bnn.declared_cross_entropy_calls()
    want = _head_grad_and_hvp(_undeclared(reduction), reduction)
    assert bnn.declared_cross_entropy_calls() == c0                      # the torch function: no node of ours
    got = _head_grad_and_hvp(_declared(reduction), reduction)
    calls = {k: v - c0[k] for k, v in bnn.declared_cross_entropy_calls().items()}
    # (the first-backward node runs twice: once for the gradient, once more when the product's cotangent of the loss — the vector's
    # component along w — passes the forward node)
    assert calls == {"forward": 1, "backward": 2, "backward_vjp": 1} and restatement == [(True, True)], (calls, restatement)
    assert torch.equal(got[0], want[0]) and all(torch.equal(u, v) for u, v in zip(got[1], want[1]))   # the same ATen kernels
    for u, v in zip(got[2], want[2]):
        assert u.shape == v.shape and float((u - v).abs().max()) <= FP64_GATE * float(v.abs().max()), reduction


def test_needs_input_grad_subsets(restatement):
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(6, 7, generator=gen, dtype=torch.float64)
    y = torch.randint(0, 7, (6,), generator=gen)
    a = torch.randn(6, 7, generator=gen, dtype=torch.float64)
    lsm = torch.log_softmax(z, 1)
    _, tw = torch.ops.aten.nll_loss_forward(lsm, y, None, 1, IGNORE)
    for z_needs, g_needs in ((True, False), (False, True), (True, True)):
        del restatement[:]
        link = lsm.clone().requires_grad_(z_needs)
        g = torch.tensor(0.7, dtype=torch.float64, requires_grad=g_needs)
        gz = bnn._CEBackward.apply(link, g, lsm, y, tw, "mean", IGNORE)
        got = torch.autograd.grad(gz, [t for t, n in ((link, z_needs), (g, g_needs)) if n], grad_outputs=a)
        assert restatement == [(z_needs, g_needs)], restatement
        want = ref.cross_entropy_backward_vjp(lsm, y, g.detach(), a, IGNORE, tw)
        for u, v in zip(got, [t for t, n in zip(want, (z_needs, g_needs)) if n]):
            assert torch.equal(u, v)
    # a loss whose incoming gradient is a constant: dz only
    del restatement[:]
    zz = z.clone().requires_grad_(True)
    (gz,) = torch.autograd.grad(_declared("sum")(zz, y), zz, create_graph=True)
    torch.autograd.grad(gz, zz, grad_outputs=a)
    assert restatement == [(True, False)], restatement


def test_the_logits_are_not_kept_alive_by_the_graph():
    """What the graph saves is log_softmax, the target and total_weight — what torch saves — and not the logits."""
    import weakref

    x = torch.randn(6, 5, dtype=torch.float64)
    W = torch.randn(5, 7, dtype=torch.float64, requires_grad=True)
    z = x @ W
    alive = weakref.ref(z)
    loss = _declared("mean")(z, torch.randint(0, 7, (6,)))
    del z
    assert alive() is None
    loss.backward()
    assert W.grad is not None


def test_declared_cross_entropy_restores_the_torch_function_on_exit_after_an_exception_too():
    was = F.cross_entropy
    assert bnn._TORCH_CROSS_ENTROPY is was
    with bnn.declared_cross_entropy():
        assert F.cross_entropy is bnn.cross_entropy
        with bnn.declared_cross_entropy():                                                  # nesting is safe
            assert F.cross_entropy is bnn.cross_entropy
        assert F.cross_entropy is bnn.cross_entropy
        z, y = torch.randn(3, 6), torch.tensor([1, 0, 5])
        c0 = bnn.declared_cross_entropy_calls()
        assert torch.equal(nn.CrossEntropyLoss()(z, y), was(z, y)) and bnn.declared_cross_entropy_calls() == c0   # a CPU input IS the torch function
    assert F.cross_entropy is was
    with pytest.raises(KeyError):
        with bnn.declared_cross_entropy():
            raise KeyError("inside")
    assert F.cross_entropy is was


def test_declare_cross_entropy_changes_only_the_class_and_declare_layers_default_is_unchanged():
    class Mine(nn.CrossEntropyLoss):
        pass

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Linear(4, 3)
            self.loss, self.smooth, self.mine, self.other = nn.CrossEntropyLoss(ignore_index=1), nn.CrossEntropyLoss(label_smoothing=0.1), Mine(), nn.NLLLoss()

    net = Net()
    assert bnn.declare_layers_(net) == {"batchnorm": 0, "pointwise_conv": 0} and type(net.loss) is nn.CrossEntropyLoss
    assert bnn.declare_layers_(net, cross_entropy=True) == {"batchnorm": 0, "pointwise_conv": 0, "cross_entropy": 2}
    assert type(net.loss) is type(net.smooth) is bnn.DeclaredCrossEntropyLoss and type(net.mine) is Mine and type(net.other) is nn.NLLLoss
    assert bnn.declare_cross_entropy_(net) == 0
    assert net.loss.ignore_index == 1 and net.smooth.label_smoothing == 0.1
    z, y = torch.randn(5, 3), torch.tensor([0, 1, 2, 2, 0])
    c0 = bnn.declared_cross_entropy_calls()
    assert torch.equal(net.loss(z, y), nn.CrossEntropyLoss(ignore_index=1)(z, y))
    assert torch.equal(net.smooth(z, y), nn.CrossEntropyLoss(label_smoothing=0.1)(z, y))
    assert bnn.declared_cross_entropy_calls() == c0                                          # CPU inputs ARE nn.CrossEntropyLoss


def _out_of_family_calls(device):
    """(label, args, kwargs) of calls outside the declared family, and calls that torch itself refuses."""
    gen = torch.Generator().manual_seed(9)
    z = torch.randn(6, 5, generator=gen).to(device)
    y = torch.randint(0, 5, (6,), generator=gen).to(device)
    return [
        ("probability targets", (z, torch.softmax(torch.randn(6, 5, generator=gen), 1).to(device)), {}),
        ("class weights", (z, y), {"weight": (torch.rand(5, generator=gen) + 0.5).to(device)}),
        ("label smoothing", (z, y), {"label_smoothing": 0.1}),
        ("spatial input", (torch.randn(2, 5, 3, generator=gen).to(device), torch.randint(0, 5, (2, 3), generator=gen).to(device)), {}),
        ("unbatched input", (z[0], y[0]), {}),
        ("bfloat16 input", (z.bfloat16(), y), {}),
        ("float64 input", (z.double(), y), {}),
        ("non-contiguous input", (torch.randn(6, 10, generator=gen).to(device)[:, ::2], y), {}),
        ("size_average", (z, y), {"size_average": False}),
        ("reduce", (z, y), {"reduce": False}),
        ("int32 target is torch's own error", (z, y.int()), {}),
        ("wrong target length is torch's own error", (z, y[:4]), {}),
        ("unknown reduction is torch's own error", (z, y), {"reduction": "median"}),
    ]


def _same_result_or_error(args, kwargs):
    outs = []
    for fn in (bnn.cross_entropy, bnn._TORCH_CROSS_ENTROPY):
        leaf = args[0].detach().requires_grad_(True)   # a fresh leaf on the same storage: strides and alignment as given
        try:
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                loss = fn(leaf, *args[1:], **kwargs)
                (grad,) = torch.autograd.grad(loss.sum(), leaf)
            outs.append((loss.detach(), grad))
        except Exception as exc:   # noqa: BLE001 - the torch function's own error, whatever its type
            outs.append((type(exc), str(exc)))
    (a0, a1), (b0, b1) = outs
    if isinstance(a0, type) or isinstance(b0, type):
        return (a0, a1) == (b0, b1)
    return torch.equal(a0, b0) and torch.equal(a1, b1)


@pytest.mark.parametrize("index", range(13))
def test_out_of_family_arguments_reach_the_torch_function_on_cpu(index):
    label, args, kwargs = _out_of_family_calls("cpu")[index]
    c0 = bnn.declared_cross_entropy_calls()
    assert _same_result_or_error(args, kwargs), label
    assert bnn.declared_cross_entropy_calls() == c0, label


def test_cpu_tensors_and_grad_mode_off_are_the_torch_function():
    z, y = torch.randn(6, 5, requires_grad=True), torch.tensor([0, 1, 2, 3, 4, 0])
    c0 = bnn.declared_cross_entropy_calls()
    for reduction in ("none", "mean", "sum"):
        assert torch.equal(bnn.cross_entropy(z, y, reduction=reduction, ignore_index=2), F.cross_entropy(z, y, reduction=reduction, ignore_index=2))
    assert bnn.declared_cross_entropy_calls() == c0


def test_the_hip_call_refuses_cpu_tensors():
    from betty_amd import _native

    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        bnn._ce_vjp_hip(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long), torch.ones(2), torch.zeros(2, 4), None, IGNORE, (True, True))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 8), (64, 1000), (4, 32773)]   # short rows, the classifier of the examples, split rows (the register bound + 5)


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("N,C", SHAPES, ids=lambda v: str(v))
def test_loss_and_first_gradient_equal_f_cross_entropys_to_the_bit(N, C, reduction):
    gen = torch.Generator().manual_seed(N + C)
    z = torch.randn(N, C, generator=gen).to(DEV)
    y = torch.randint(0, C, (N,), generator=gen)
    y[1] = IGNORE
    y = y.to(DEV)
    up = torch.randn(N if reduction == "none" else (), generator=gen).to(DEV)

    def first(fn, create_graph):
        t = z.clone().requires_grad_(True)
        loss = fn(t, y, reduction=reduction)
        return loss.detach(), torch.autograd.grad((loss * up).sum(), t, create_graph=create_graph)[0].detach()

    c0 = bnn.declared_cross_entropy_calls()
    want = first(F.cross_entropy, False)
    assert bnn.declared_cross_entropy_calls() == c0
    for create_graph in (True, False):
        got = first(bnn.cross_entropy, create_graph)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), create_graph
    assert bnn.declared_cross_entropy_calls()["forward"] == c0["forward"] + 2


def _model_grad_and_hvp(model, N, C, reduction, declared, dtype=torch.float32):
    torch.manual_seed(1)
    D = 8
    net = (nn.Linear(D, C) if model == "linear" else nn.Sequential(nn.Linear(D, 16), nn.Tanh(), nn.Linear(16, C))).to(DEV, dtype)
    gen = torch.Generator().manual_seed(N * 31 + C)
    x = torch.randn(N, D, generator=gen).to(DEV, dtype)
    y = torch.randint(0, C, (N,), generator=gen)
    y[N // 2] = IGNORE
    y = y.to(DEV)
    w = (torch.rand(N, generator=gen) + 0.5).to(DEV, dtype)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=gen).to(DEV, dtype) for p in params]
    c0 = bnn.declared_cross_entropy_calls()
    fn = bnn.cross_entropy if declared else F.cross_entropy
    ce = fn(net(x), y, reduction=reduction)
    loss = (ce * w).mean() if reduction == "none" else ce
    grads = torch.autograd.grad(loss, params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    calls = {k: v - c0[k] for k, v in bnn.declared_cross_entropy_calls().items()}
    live = 1 if declared and dtype == torch.float32 else 0
    assert calls == {"forward": live, "backward": live, "backward_vjp": live}, calls   # exactly one fused call per loss and product
    return [t.detach().cpu().numpy() for t in hv]


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("model", ["linear", "mlp"])
@pytest.mark.parametrize("N,C", SHAPES, ids=lambda v: str(v))
def test_hvp_within_the_fp32_error_of_the_float64_product(N, C, model, reduction):
    plain = _model_grad_and_hvp(model, N, C, reduction, False)
    declared = _model_grad_and_hvp(model, N, C, reduction, True)
    exact = _model_grad_and_hvp(model, N, C, reduction, False, torch.float64)
    _, e_plain = rel_err(plain, exact)
    _, e_decl = rel_err(declared, exact)
    _, between = rel_err(declared, plain)
    print(f"declared cross-entropy {model} {N} x {C} {reduction}, max|diff| / max|want| against the float64 product: declared {e_decl:.2e}, "
          f"undeclared fp32 {e_plain:.2e}; declared against undeclared {between:.2e}")
    assert e_plain > 0
    assert e_decl <= 4.0 * e_plain, (e_decl, e_plain)        # the margin: 4
    assert between <= 5.0 * e_plain, (between, e_plain)      # and so, by the triangle inequality


def _problem(algo, K=5):
    torch.manual_seed(3)
    inner, upper = zoo.MLP([12, 20, 10]).to(DEV), zoo.MWN(8).to(DEV)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(24, 12, generator=g).to(DEV), torch.randint(0, 10, (24,), generator=g).to(DEV)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_declared_cross_entropy_matches_the_undeclared_problem(algo):
    import contextlib

    out = {}
    for declared in (False, True):
        curr, prev, vector = _problem(algo)
        c0 = bnn.declared_cross_entropy_calls()
        with (bnn.declared_cross_entropy() if declared else contextlib.nullcontext()):
            res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[declared] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.declared_cross_entropy_calls()["backward_vjp"] - c0["backward_vjp"]
        # one fused call per loss and product: the K = 5 Hessian-vector products of the solve and the mixed second derivative that closes it
        assert calls == (5 + 1 if declared else 0), calls
    rel, _ = rel_err(out[True], out[False])
    print(f"{algo} hypergradient (K = 5), cross-entropy declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(13))
def test_out_of_family_arguments_reach_the_torch_function_on_the_gpu(index):
    label, args, kwargs = _out_of_family_calls(DEV)[index]
    c0 = bnn.declared_cross_entropy_calls()
    assert _same_result_or_error(args, kwargs), label
    assert bnn.declared_cross_entropy_calls() == c0, label


@pytest.mark.gpu
def test_grad_mode_off_misaligned_and_too_many_classes_take_the_torch_path_and_the_plain_call_is_declared():
    gen = torch.Generator().manual_seed(4)
    z, y = torch.randn(6, 5, generator=gen).to(DEV), torch.randint(0, 5, (6,), generator=gen).to(DEV)
    c0 = bnn.declared_cross_entropy_calls()
    with torch.no_grad():
        assert torch.equal(bnn.cross_entropy(z, y), F.cross_entropy(z, y))
    flat = torch.randn(6 * 5 + 1, generator=gen).to(DEV)
    off = flat[1:].reshape(6, 5)                                       # contiguous, 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 != 0 and torch.equal(bnn.cross_entropy(off, y), F.cross_entropy(off, y))
    wide = torch.randn(1, 262145, generator=gen).to(DEV)
    assert torch.equal(bnn.cross_entropy(wide, y[:1]), F.cross_entropy(wide, y[:1]))
    assert bnn.declared_cross_entropy_calls() == c0
    assert torch.equal(bnn.cross_entropy(z.requires_grad_(True), y), F.cross_entropy(z, y))
    with bnn.declared_cross_entropy():
        nn.CrossEntropyLoss()(z, y)                                    # nn.CrossEntropyLoss itself, through the patched function
    assert bnn.declared_cross_entropy_calls()["forward"] == c0["forward"] + 2

"""betty_amd.nn.DepthwiseConv2d on the GPU against plain nn.Conv2d on the same GPU: gradient and Hessian-vector product of a small net, of a
`sep`-style and of a `dil`-style block of a DARTS cell (ReLU -> depthwise -> 1 x 1 -> BatchNorm2d, written from those layer lists), one
bhg_dwconv_backward_vjp call per depthwise layer and product; a cg and a neumann hypergradient through a problem whose inner net has all
three declarations; and the inputs that take nn.Conv2d's own path.  Gate: 1e-4 of the norm, the package's parity bar.

The convolutions of both sides run on ATen's own kernels, not MIOpen's (as in tests/test_fused_batchnorm.py's pointwise test): which
MIOpen solver takes a small grouped shape, and the kernels it compiles for it at first use, differ from machine to machine, and what is
compared here does not depend on which library computes nn.Conv2d."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import zoo
from conftest import rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd import nn as bnn

DEV = "cuda:0"
GATE = 1e-4


@pytest.fixture(autouse=True)
def _aten_convolutions():
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = was


def _dw_pw_bn(C, C_out, k, stride, pad, dil=1):
    return [nn.ReLU(), nn.Conv2d(C, C, k, stride=stride, padding=pad, dilation=dil, groups=C, bias=False), nn.Conv2d(C, C_out, 1, bias=False),
            nn.BatchNorm2d(C_out)]


def small_net(C=8):
    return nn.Sequential(*_dw_pw_bn(C, 6, 3, 1, 1), nn.Flatten(), nn.Linear(6 * 12 * 12, 3))


def sep_block(k, C=8):
    """`sep`-style: two depthwise-separable stages, the first at the cell's stride (2 here), the second at stride 1."""
    return nn.Sequential(*_dw_pw_bn(C, C, k, 2, k // 2), *_dw_pw_bn(C, C, k, 1, k // 2), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(C, 3))


def dil_block(C=8):
    """`dil`-style: one dilated depthwise stage (d = 2) at stride 2."""
    return nn.Sequential(*_dw_pw_bn(C, C, 3, 2, 2, dil=2), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(C, 3))


def _grad_and_hvp(make, declared, layers):
    torch.manual_seed(1)
    net = make().to(DEV)
    if declared:
        assert bnn.declare_depthwise_convs_(net) == layers
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 8, 12, 12, generator=g).to(DEV), torch.randint(0, 3, (4,), generator=g).to(DEV)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g).to(DEV) for p in params]
    c0 = bnn.depthwise_conv_calls()
    grads = torch.autograd.grad(F.cross_entropy(net(x), y), params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    calls = {k: v - c0[k] for k, v in bnn.depthwise_conv_calls().items()}
    assert calls["backward_vjp"] == (layers if declared else 0) and calls["forward"] == (layers if declared else 0), calls
    return [t.detach().cpu().numpy() for t in grads], [t.cpu().numpy() for t in hv]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,layers", [("small net", small_net, 1), ("sep k=3", lambda: sep_block(3), 2), ("sep k=5", lambda: sep_block(5), 2),
                                              ("dil", dil_block, 1)], ids=lambda v: v if isinstance(v, str) else None)
def test_module_matches_nn_conv2d_gradient_and_hvp(name, make, layers):
    want, got = _grad_and_hvp(make, False, layers), _grad_and_hvp(make, True, layers)
    e_g, _ = rel_err(got[0], want[0])
    e_h, _ = rel_err(got[1], want[1])
    print(f"DepthwiseConv2d vs nn.Conv2d on the GPU, {name}: gradient {e_g:.2e}, Hessian-vector product {e_h:.2e}")
    assert e_g <= GATE and e_h <= GATE, (e_g, e_h)


class _Inner(nn.Module):
    """A reduced search cell's worth of declared layers: stem, a `sep` stage, a `dil` stage, classifier."""

    def __init__(self, C=8):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, C, 3, padding=1, bias=False), nn.BatchNorm2d(C))
        self.sep = nn.Sequential(*_dw_pw_bn(C, C, 3, 1, 1), *_dw_pw_bn(C, C, 3, 1, 1))
        self.dil = nn.Sequential(*_dw_pw_bn(C, C, 5, 2, 4, dil=2))
        self.fc = nn.Linear(C, 3)

    def forward(self, x):
        h = self.stem(x)
        h = self.dil(self.sep(h) + h)
        return self.fc(h.mean((2, 3)))


def _problem(declared, algo, K=3):
    torch.manual_seed(3)
    inner, upper = _Inner().to(DEV), _Inner().to(DEV)
    if declared:
        assert bnn.declare_layers_(inner, depthwise=True) == {"batchnorm": 4, "pointwise_conv": 3, "depthwise_conv": 3}
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(6, 3, 10, 10, generator=g).to(DEV), torch.randint(0, 3, (6,), generator=g).to(DEV)
    vector = [0.1 * torch.randn(p.shape, generator=g).to(DEV) for p in inner.parameters()]
    prev = zoo.StubProblem("upper", upper, config=Config())
    cfg = Config(type="cg", cg_iterations=K, cg_alpha=1.0) if algo == "cg" else Config(type="neumann", neumann_iterations=K, neumann_alpha=0.05)
    curr = zoo.StubProblem("inner", inner, config=cfg, loss_fn=zoo.make_imaml_loss(prev, 0.5), batch=(x, y))
    return curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "neumann"])
def test_hypergradient_through_declared_layers_matches_the_undeclared_problem(algo):
    out = {}
    for declared in (False, True):
        curr, prev, vector = _problem(declared, algo)
        c0 = bnn.depthwise_conv_calls()
        res = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        out[declared] = [t.detach().cpu().numpy() for t in res]
        calls = bnn.depthwise_conv_calls()["backward_vjp"] - c0["backward_vjp"]
        assert calls == (3 * 3 if declared else 0), calls            # three depthwise layers, K = 3 products
    rel, _ = rel_err(out[True], out[False])
    print(f"{algo} hypergradient (K = 3), batch norm + pointwise + depthwise declared vs undeclared: {rel:.2e}")
    assert rel <= GATE, rel


@pytest.mark.gpu
def test_channels_last_and_float64_inputs_take_nn_conv2ds_path():
    torch.manual_seed(0)
    conv = bnn.DepthwiseConv2d(8, 8, 3, padding=1, groups=8, bias=False).to(DEV)
    ref = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False).to(DEV)
    ref.load_state_dict(conv.state_dict())
    x = torch.randn(2, 8, 6, 6, device=DEV)
    c0 = bnn.depthwise_conv_calls()
    for which in ("channels_last", "float64"):
        m, r, inp = (conv, ref, x.to(memory_format=torch.channels_last)) if which == "channels_last" else (conv.double(), ref.double(), x.double())
        inp = inp.requires_grad_(True)
        outs = []
        for layer in (m, r):
            y = layer(inp)
            outs.append((y.detach(), torch.autograd.grad((y ** 2).sum(), [inp, layer.weight])))
        assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(u, v) for u, v in zip(outs[0][1], outs[1][1]))
    assert bnn.depthwise_conv_calls() == c0
    y = conv.float()(x.requires_grad_(True))                   # and the declared route is live for the plain input
    assert bnn.depthwise_conv_calls()["forward"] == c0["forward"] + 1 and torch.equal(y, ref.float()(x))

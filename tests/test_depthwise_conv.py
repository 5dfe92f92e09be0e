"""betty_amd.nn.DepthwiseConv2d on the CPU: the two autograd.Function nodes wired as the package wires them, with the float64 restatement
(tests/dwconv_ref.py, the checker) standing in for the HIP call — loss, gradient and Hessian-vector product equal to nn.Conv2d's; where the
module IS nn.Conv2d; the declarations; state_dict; absent cotangents; and the C ABI's host logic (argument validation and the shape ->
geometry map bhg_dwconv_plan), which needs no GPU.  The kernels: tests/test_dwconv_kernels.py; the module on the GPU:
tests/test_depthwise_conv_gpu.py."""
import contextlib
import ctypes
import itertools
import re
import time

import pytest
import torch

import dwconv_ref
from conftest import rel_err

from betty_amd import _native
from betty_amd import nn as bnn
from betty_amd.backend import dwconv_plan


@contextlib.contextmanager
def checker_vjp():
    prev = bnn._DW_VJP_IMPL[0]
    bnn._DW_VJP_IMPL[0] = dwconv_ref.dwconv_backward_vjp
    try:
        yield
    finally:
        bnn._DW_VJP_IMPL[0] = prev


class _AlwaysDeclared(bnn.DepthwiseConv2d):
    """The package's two autograd nodes on CPU float64 tensors (the module itself only takes that route for CUDA fp32 inputs)."""

    def _declared(self, x):
        return True


def _net(dw_cls, C=4, k=3, stride=1, pad=1, dil=1):
    """ReLU -> depthwise -> 1 x 1 -> BN -> Flatten -> Linear, on 8 x 8 inputs."""
    torch.manual_seed(11)
    out = dwconv_ref.out_extent(8, k, stride, pad, dil)
    return torch.nn.Sequential(torch.nn.ReLU(), dw_cls(C, C, k, stride=stride, padding=pad, dilation=dil, groups=C, bias=False),
                               torch.nn.Conv2d(C, 6, 1, bias=False), torch.nn.BatchNorm2d(6), torch.nn.Flatten(),
                               torch.nn.Linear(6 * out * out, 3)).double()


def _loss_grad_hvp(net, x_requires_grad=False):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 4, 8, 8, generator=g, dtype=torch.float64).requires_grad_(x_requires_grad)
    y = torch.randint(0, 3, (5,), generator=g)
    params = list(net.parameters())
    vec = [torch.randn(p.shape, generator=g, dtype=torch.float64) for p in params]
    loss = torch.nn.functional.cross_entropy(net(x), y)
    grads = torch.autograd.grad(loss, params, create_graph=True)
    hv = torch.autograd.grad(grads, params, grad_outputs=vec)
    return float(loss.detach()), [t.detach().numpy() for t in grads], [t.numpy() for t in hv]


@pytest.mark.parametrize("k,stride,pad,dil", [(3, 1, 1, 1), (5, 2, 2, 1), (3, 2, 2, 2), (7, 1, 3, 1), (5, 1, 4, 2)])
def test_declared_layer_gives_the_same_loss_gradient_and_hessian_vector_product(k, stride, pad, dil):
    want = _loss_grad_hvp(_net(torch.nn.Conv2d, k=k, stride=stride, pad=pad, dil=dil))
    c0 = bnn.depthwise_conv_calls()
    with checker_vjp():
        got = _loss_grad_hvp(_net(_AlwaysDeclared, k=k, stride=stride, pad=pad, dil=dil))
    calls = {n: v - c0[n] for n, v in bnn.depthwise_conv_calls().items()}
    # (the backward node runs twice: in the gradient, and when the product's pass comes back through the forward graph)
    assert calls == {"forward": 1, "backward": 2, "backward_vjp": 1}, calls
    assert abs(got[0] - want[0]) <= 1e-10 * abs(want[0])
    e_g, _ = rel_err(got[1], want[1])
    e_h, _ = rel_err(got[2], want[2])
    assert e_g <= 1e-10 and e_h <= 1e-10, (e_g, e_h)


def test_absent_cotangents_gradient_with_respect_to_x_only_and_w_only():
    """d/dx only: the weight takes no gradient, so gw is not computed and its cotangent b is absent; d/dw only (x a plain input): a is absent."""
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(3, 4, 8, 8, generator=g, dtype=torch.float64)
    v_x, v_w = torch.randn(3, 4, 8, 8, generator=g, dtype=torch.float64), torch.randn(4, 1, 3, 3, generator=g, dtype=torch.float64)
    res = {}
    for cls in (torch.nn.Conv2d, _AlwaysDeclared):
        torch.manual_seed(2)
        conv = cls(4, 4, 3, stride=2, padding=1, groups=4, bias=False).double()
        out = []
        with checker_vjp():
            # x only
            conv.weight.requires_grad_(False)
            x = x0.clone().requires_grad_(True)
            gx, = torch.autograd.grad((conv(x) ** 3).sum(), x, create_graph=True)
            out.append(torch.autograd.grad(gx, x, grad_outputs=v_x)[0])
            # w only
            conv.weight.requires_grad_(True)
            gw, = torch.autograd.grad((conv(x0) ** 3).sum(), conv.weight, create_graph=True)
            out.append(torch.autograd.grad(gw, conv.weight, grad_outputs=v_w)[0])
        res[cls] = [t.numpy() for t in out]
    for got, want in zip(res[_AlwaysDeclared], res[torch.nn.Conv2d]):
        assert rel_err([got], [want])[0] <= 1e-10


def test_the_layer_is_nn_conv2d_outside_the_family():
    x4 = torch.randn(2, 4, 9, 9)
    outside = [dict(bias=True), dict(groups=2), dict(out=8), dict(kernel=(3, 5), padding=(1, 2)), dict(kernel=9, padding=4), dict(stride=3),
               dict(padding="same"), dict(padding_mode="reflect"), dict(stride=(1, 2)), dict(dilation=(1, 2)), dict(padding=(1, 0)),
               dict(padding=3), dict(dilation=3)]
    for kw in outside:
        kw = dict(kw)
        m = bnn.DepthwiseConv2d(4, kw.pop("out", 4), kw.pop("kernel", 3), groups=kw.pop("groups", 4), bias=kw.pop("bias", False),
                                padding=kw.pop("padding", 1), **kw)
        assert not m._family(), kw
        ref = torch.nn.Conv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, m.bias is not None, m.padding_mode)
        ref.load_state_dict(m.state_dict())
        c0 = bnn.depthwise_conv_calls()
        torch.testing.assert_close(m(x4), ref(x4), rtol=0, atol=0)
        assert bnn.depthwise_conv_calls() == c0
    inside = bnn.DepthwiseConv2d(4, 4, 3, padding=1, groups=4, bias=False)
    assert inside._family()
    ref = torch.nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=False)
    ref.load_state_dict(inside.state_dict())
    c0 = bnn.depthwise_conv_calls()
    torch.testing.assert_close(inside(x4), ref(x4), rtol=0, atol=0)              # a CPU tensor
    torch.testing.assert_close(inside(x4[0]), ref(x4[0]), rtol=0, atol=0)        # a 3-D input
    forced = _AlwaysDeclared(4, 4, 3, padding=1, groups=4, bias=False).eval()
    forced.load_state_dict(ref.state_dict())
    with torch.no_grad():                                                         # eval under no_grad
        torch.testing.assert_close(forced(x4), ref(x4), rtol=0, atol=0)
    assert bnn.depthwise_conv_calls() == c0
    # the product's double backward has no CPU route
    with pytest.raises(_native.NativeLibraryError):
        bnn._dw_vjp_hip(x4, ref.weight, x4, x4, None, 1, 1, 1)


def test_declarations_count_and_reclass_only_the_family():
    net = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=False), torch.nn.Conv2d(4, 8, 1, bias=False),
                              torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 8, 5, stride=2, padding=4, dilation=2, groups=8, bias=False),
                              torch.nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=True), torch.nn.Conv2d(8, 16, 3, padding=1, groups=8, bias=False),
                              torch.nn.Conv2d(16, 16, 9, padding=4, groups=16, bias=False), torch.nn.Conv2d(16, 16, 3, padding=1, bias=False))
    keys = list(net.state_dict())
    assert bnn.declare_layers_(net) == {"batchnorm": 1, "pointwise_conv": 1}
    assert not any(type(m) is bnn.DepthwiseConv2d for m in net.modules())
    assert bnn.declare_layers_(net, depthwise=True) == {"batchnorm": 0, "pointwise_conv": 0, "depthwise_conv": 2}
    assert [type(m) is bnn.DepthwiseConv2d for m in net] == [False, True, False, False, True, False, False, False, False]
    assert bnn.declare_depthwise_convs_(net) == 0
    assert list(net.state_dict()) == keys
    for name in ("DepthwiseConv2d", "declare_depthwise_convs_", "depthwise_conv_calls", "declare_layers_"):
        assert name in bnn.__all__ and hasattr(bnn, name)


def test_state_dict_round_trips():
    torch.manual_seed(0)
    a = bnn.DepthwiseConv2d(6, 6, 5, stride=2, padding=2, groups=6, bias=False)
    b = torch.nn.Conv2d(6, 6, 5, stride=2, padding=2, groups=6, bias=False)
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight"]
    b.load_state_dict(a.state_dict())
    a2 = bnn.DepthwiseConv2d(6, 6, 5, stride=2, padding=2, groups=6, bias=False)
    a2.load_state_dict(b.state_dict())
    assert torch.equal(a.weight, a2.weight)


# ---- the C ABI's host logic ------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    """Every refusal returns -1 and names its cause before any device access (the pointers are host memory: a call that got past the
    checks would not return -1 with these words).  bhg_dwconv_plan refuses the same shapes with the same words."""
    lib = _native.load()
    host = (ctypes.c_float * 64)()
    q = (ctypes.addressof(host) + 15) & ~15
    assert lib.bhg_dwconv_ws_bytes(3, 5) == 8 * 64 * 25 * 3
    for C, k in [(0, 3), (-1, 3), (3, 0), (3, -3), (0, 0)]:
        assert lib.bhg_dwconv_ws_bytes(C, k) == 0
    base = dict(N=2, C=3, H=8, W=8, k=3, stride=1, pad=1, dil=1)

    def vjp(x=q, w=q, gy=q, a=q, b=q, dx=q, dw=q, dgy=q, ws=q, ws_bytes=None, **kw):
        s = dict(base, **kw)
        return lib.bhg_dwconv_backward_vjp(x, w, gy, a, b, s["N"], s["C"], s["H"], s["W"], s["k"], s["stride"], s["pad"], s["dil"], dx, dw, dgy,
                                           ws, lib.bhg_dwconv_ws_bytes(s["C"], s["k"]) if ws_bytes is None else ws_bytes, None)

    def plan(**kw):
        s = dict(base, **kw)
        buf = ctypes.create_string_buffer(512)
        return lib.bhg_dwconv_plan(s["N"], s["C"], s["H"], s["W"], s["k"], s["stride"], s["pad"], s["dil"], buf, 512)

    shapes = [(dict(k=9, pad=4), b"kernel size"), (dict(k=4), b"kernel size"), (dict(k=1, pad=0), b"kernel size"), (dict(stride=3), b"stride"),
              (dict(stride=0), b"stride"), (dict(dil=3), b"dilation"), (dict(dil=0), b"dilation"), (dict(pad=-1), b"padding"),
              (dict(pad=3), b"padding"), (dict(k=5, dil=2, pad=9), b"padding"), (dict(N=0), b"empty tensor"), (dict(C=0), b"empty tensor"),
              (dict(H=0), b"empty tensor"), (dict(W=-3), b"empty tensor"), (dict(N=-1), b"empty tensor"), (dict(C=65536), b"65535 channels"),
              (dict(H=2, pad=0), b"empty output"), (dict(W=4, k=7, pad=0), b"empty output"), (dict(H=8, W=8, k=5, dil=2, pad=0), b"empty output")]
    for kw, word in shapes:
        assert vjp(**kw) == -1, kw
        said = lib.bhg_last_error()
        assert word in said and b"bhg_dwconv_backward_vjp" in said, (kw, said)
        assert plan(**kw) == -1, kw
        assert said.split(b": ", 1)[1] == lib.bhg_last_error().split(b": ", 1)[1], (kw, said, lib.bhg_last_error())
    assert plan() == 0
    for name in ("x", "w", "gy", "dgy", "ws"):
        assert vjp(**{name: None}) == -1, name
        assert b"null pointer" in lib.bhg_last_error(), (name, lib.bhg_last_error())
    need = lib.bhg_dwconv_ws_bytes(3, 3)
    for n in (need - 1, 0):
        assert vjp(ws_bytes=n) == -1
        assert b"workspace smaller" in lib.bhg_last_error()
    for name in ("x", "a", "gy"):                       # W and the output width are multiples of 4: their planes are staged in 16-byte groups
        for off in (4, 8, 12):
            assert vjp(**{name: q + off}) == -1, (name, off)
            assert b"16-byte aligned" in lib.bhg_last_error(), (name, off, lib.bhg_last_error())
    buf = ctypes.create_string_buffer(8)
    assert lib.bhg_dwconv_plan(2, 3, 8, 8, 3, 1, 1, 1, buf, 8) == -1 and b"buffer too small" in lib.bhg_last_error()
    assert lib.bhg_dwconv_plan(2, 3, 8, 8, 3, 1, 1, 1, None, 0) == -1


LDS_BUDGET = 60 << 10    # kDwMaxLds (csrc/bhg_dwconv.hip): dynamic LDS of one workgroup


def _plan_or_refusal(lib, N, C, H, W, k, s, pad, d):
    """(plan dict, None) or (None, message), and the seconds the call took."""
    buf = ctypes.create_string_buffer(512)
    t0 = time.perf_counter()
    rc = lib.bhg_dwconv_plan(N, C, H, W, k, s, pad, d, buf, 512)
    took = time.perf_counter() - t0
    if rc != 0:
        return None, lib.bhg_last_error(), took
    return {key: int(v) for key, v in re.findall(r"(\w+)=(-?\d+)", buf.value.decode())}, None, took


def _check_plan(p, N, C, H, W, k, s, pad, d, reserved=64):
    Ho, Wo = dwconv_ref.out_extent(H, k, s, pad, d), dwconv_ref.out_extent(W, k, s, pad, d)
    assert (p["Ho"], p["Wo"]) == (Ho, Wo)
    for pre, (eh, ew) in (("", (Ho, Wo)), ("i", (H, W))):
        th, tw, pb, ty, tx = (p[pre + key] for key in ("th", "tw", "pb", "ty", "tx"))
        assert th * tw * pb <= 256 and pb in (1, 2, 4, 8) and th & (th - 1) == 0 and tw & (tw - 1) == 0
        assert (ty - 1) * th < eh <= ty * th and (tx - 1) * tw < ew <= tx * tw
    assert p["vec"] == (4 if W % 4 == 0 else 1) and p["ivec"] == (4 if Wo % 4 == 0 else 1)
    assert p["units"] == N * p["ty"] * p["tx"]                        # every output position of a channel lies in one unit
    assert (p["groups"] - 1) * p["pb"] < p["units"] <= p["groups"] * p["pb"]
    assert 1 <= p["slices"] <= reserved == p["max_slices"]
    assert (p["slices"] - 1) * p["gps"] < p["groups"] <= p["slices"] * p["gps"]   # covered, and the last slice is not empty
    # the staged tiles as the launches size them: both terms of dgy, the gy tile of dx
    assert p["lds_dgy"] == 4 * 2 * p["pb"] * p["rows"] * p["ls"] <= LDS_BUDGET and p["lds_dx"] == 4 * p["ipb"] * p["irows"] * p["ils"] <= LDS_BUDGET
    halo = d * (k - 1)
    assert p["rows"] == (p["th"] - 1) * s + halo + 1 and p["ls"] % 4 == 0 and p["ls"] >= (p["tw"] - 1) * s + halo + 1 + 3
    assert p["irows"] == (p["ith"] - 1 + halo) // s + 1 and p["ils"] % 4 == 0 and p["ils"] >= (p["itw"] - 1 + halo) // s + 1 + 3


def test_plan_covers_every_shape_within_the_reserved_slices_at_once():
    """The sweep of the issue at no, half and full padding: the slices cover N * H_out * W_out with none empty, their count is within
    what bhg_dwconv_ws_bytes reserves, the tiles cover both planes, the staged tiles fit the LDS budget; a shape is refused exactly when
    its output is empty, and says so; no shape makes the host logic search (every single call returns at once)."""
    lib = _native.load()
    extents = (1, 2, 31, 32, 33, 64, 1025)
    n = refused = 0
    slowest = 0.0
    for k, s, d in itertools.product((3, 5, 7), (1, 2), (1, 2)):
        assert lib.bhg_dwconv_ws_bytes(1, k) // (8 * k * k) == 64
        for pad in (0, d * (k - 1) // 2, d * (k - 1)):
            for N, C, H, W in itertools.product(range(1, 6), (1, 3, 64, 65535), extents, extents):
                p, why, took = _plan_or_refusal(lib, N, C, H, W, k, s, pad, d)
                n, slowest = n + 1, max(slowest, took)
                if dwconv_ref.out_extent(H, k, s, pad, d) < 1 or dwconv_ref.out_extent(W, k, s, pad, d) < 1:
                    assert p is None and b"empty output" in why, (N, C, H, W, k, s, pad, d, why)
                    refused += 1
                    continue
                assert p is not None, (N, C, H, W, k, s, pad, d, why)
                _check_plan(p, N, C, H, W, k, s, pad, d)
    assert n == 12 * 3 * 5 * 4 * 49 and 0 < refused < n // 3
    assert slowest < 0.5, slowest     # microseconds of host arithmetic per shape: a search would take minutes


def test_every_tile_of_the_family_fits_the_lds_budget():
    """Every (k, stride, dilation) at EVERY padding 0 .. d (k - 1), over extents that put H_out and W_out on either side of each tile
    size (1, 2, 4, ... 32 and beyond) — flat outputs with the widest halo among them (k = 7, s = 2, d = 2, H_out = 1, W_out >= 17: 13 x 80
    floats per unit and term, which do not fit at eight units per workgroup).  No shape of the family may be refused."""
    lib = _native.load()
    extents = (1, 2, 4, 5, 8, 9, 13, 14, 16, 17, 32, 33, 45, 64, 65, 140)
    worst, seen_halved = (0, None), False
    for k, s, d in itertools.product((3, 5, 7), (1, 2), (1, 2)):
        for pad in range(d * (k - 1) + 1):
            for H, W in itertools.product(extents, extents):
                if dwconv_ref.out_extent(H, k, s, pad, d) < 1 or dwconv_ref.out_extent(W, k, s, pad, d) < 1:
                    continue
                p, why, _ = _plan_or_refusal(lib, 2, 3, H, W, k, s, pad, d)
                assert p is not None, (H, W, k, s, pad, d, why)
                _check_plan(p, 2, 3, H, W, k, s, pad, d)
                worst = max(worst, (max(p["lds_dgy"], p["lds_dx"]), (H, W, k, s, pad, d)))
                seen_halved |= p["th"] * p["tw"] * p["pb"] < 256 and p["pb"] < 8
    p = dwconv_plan(1, 2, 13, 45, 7, 2, 0, 2)      # the reviewer's example: 1 x 17 outputs
    assert (p["Ho"], p["Wo"], p["th"], p["tw"], p["rows"], p["ls"]) == (1, 17, 1, 32, 13, 80) and p["pb"] == 4 and p["lds_dgy"] == 33280, p
    assert seen_halved and worst[0] <= LDS_BUDGET, worst
    print(f"largest staged tile of the family: {worst[0]} bytes at (H, W, k, stride, pad, dil) = {worst[1]}")

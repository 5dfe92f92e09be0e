"""Restatement of the declared activations' double backward (csrc/bhg_activation.hip) in plain tensor operations, in the dtype of its
inputs (float64 in the tests; float32 to show what the formulas themselves cost in that format).

Plain, y = f(x), first backward gx = gy f'(x); for a cotangent a of gx:      dgy = a f'(x)      dx = a gy f''(x).
Gated, y = f(u) v, first backward (gu, gv) = (gy f'(u) v, gy f(u)); for cotangents au, av (either may be None):
    dgy = au f'(u) v + av f(u)      du = au gy f''(u) v + av gy f'(u)      dv = au gy f'(u).
F.glu on the last dimension: the gated form with f = sigmoid, v the FIRST half of x and u the second.

Nothing is written as a subtraction from one: sech^2 and sigmoid(x) sigmoid(-x).  tests/test_activation_ref.py holds this file to
autograd's double backward of the torch functions in float64."""
import math

import torch

KINDS = ("gelu", "gelu_tanh", "silu", "tanh", "sigmoid", "softplus")
KIND_ID = {k: i for i, k in enumerate(KINDS)}
GATED_KINDS = KINDS[:5]
SPECIAL = (0.0, -0.0, 1e-30, -1e-30, 8.0, -8.0, 20.0, -20.0, 40.0, -40.0, 100.0, -100.0, 1e4, -1e4)


def special_values(dtype=torch.float64):
    return torch.tensor(SPECIAL, dtype=dtype)


def sample_inputs(n=4000, seed=0, dtype=torch.float64):
    """The inputs the formulas were checked on: n values of 3 N(0, 1) followed by the special values."""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([3.0 * torch.randn(n, generator=g, dtype=torch.float64), special_values()]).to(dtype)


def softplus_safe(x, beta, threshold, margin=1e-3):
    """x with the values nearer than `margin` to ATen's branch point beta x = threshold moved off it (its formula is discontinuous there)."""
    z = beta * x
    near = (z - threshold).abs() < margin
    return torch.where(near, x + 2.0 * margin / abs(beta), x)


def _sech2(w):
    e = torch.exp(-2.0 * w.abs())
    return 4.0 * e / ((1.0 + e) * (1.0 + e))


def derivs(kind, x, beta=1.0, threshold=20.0):
    """(f, f', f'') of the kind at x, element by element."""
    if kind == "gelu":
        phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        Phi = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
        return x * Phi, Phi + x * phi, phi * (2.0 - x * x)
    if kind == "gelu_tanh":
        k, c = math.sqrt(2.0 / math.pi), 0.044715
        w = k * (x + c * x * x * x)
        wp = k * (1.0 + 3.0 * c * x * x)
        wpp = 6.0 * k * c * x
        t, s = torch.tanh(w), _sech2(w)
        half1pt = torch.sigmoid(2.0 * w)                           # (1 + tanh w) / 2
        return x * half1pt, half1pt + 0.5 * x * s * wp, s * wp + 0.5 * x * (s * wpp - 2.0 * t * s * wp * wp)
    if kind == "silu":
        p, m = torch.sigmoid(x), torch.sigmoid(-x)
        return x * p, p * (1.0 + x * m), p * m * (2.0 + x * (m - p))
    if kind == "tanh":
        t, s = torch.tanh(x), _sech2(x)
        return t, s, -2.0 * t * s
    if kind == "sigmoid":
        p, m = torch.sigmoid(x), torch.sigmoid(-x)
        return p, p * m, p * m * (m - p)
    if kind == "softplus":
        z = beta * x
        lin = z > threshold
        p, m = torch.sigmoid(z), torch.sigmoid(-z)
        f = torch.where(lin, x, torch.nn.functional.softplus(z) / beta)
        return f, torch.where(lin, torch.ones_like(x), p), torch.where(lin, torch.zeros_like(x), beta * p * m)
    raise ValueError(kind)


def act_backward_vjp(kind, x, gy, a, beta=1.0, threshold=20.0):
    """(dx, dgy) of the plain form."""
    _, f1, f2 = derivs(kind, x, beta, threshold)
    return a * gy * f2, a * f1


def gated_backward_vjp(kind, u, v, gy, au, av):
    """(du, dv, dgy) of the gated form; au or av may be None (absent: zero), not both."""
    assert au is not None or av is not None
    f, f1, f2 = derivs(kind, u)
    zero = torch.zeros_like(u)
    au_, av_ = (zero if au is None else au), (zero if av is None else av)
    return au_ * gy * f2 * v + av_ * gy * f1, au_ * gy * f1, au_ * f1 * v + av_ * f


def glu_backward_vjp(x, gy, a):
    """(dx, dgy) of F.glu(x, -1)'s backward for a cotangent a of gx: the gated form on the halves, v first."""
    H = x.shape[-1] // 2
    du, dv, dgy = gated_backward_vjp("sigmoid", x[..., H:], x[..., :H], gy, a[..., H:], a[..., :H])
    return torch.cat([dv, du], dim=-1), dgy


def torch_function(kind, beta=1.0, threshold=20.0):
    """The torch function a kind restates."""
    F = torch.nn.functional
    return {"gelu": F.gelu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "silu": F.silu, "tanh": torch.tanh,
            "sigmoid": torch.sigmoid, "softplus": lambda t: F.softplus(t, beta=beta, threshold=threshold)}[kind]

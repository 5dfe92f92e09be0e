"""The checker's float64 restatement of bhg_dwconv_backward_vjp (csrc/bhg_dwconv.hip): the vector-Jacobian product of a depthwise
convolution's backward F : (x, w, gy) -> (gx, gw), for cotangents a (of gx) and b (of gw), either of which may be None (= zero):

    dgy = conv(a, w) + conv(x, b)      dx = conv_backward_input(gy; filter b)      dw = conv_backward_weight(input a, gy)

written with ATen's own convolution and convolution_backward on the tensors as given (float64 in the tests).  w, b: [C, 1, k, k]."""
import torch
import torch.nn.functional as F


def out_extent(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def dwconv_backward_vjp(x, w, gy, a, b, stride, pad, dil, need_dx=True, need_dw=True):
    """(dx, dw, dgy); every output is a full tensor (zeros where its cotangent is None) unless not needed (None)."""
    C = w.shape[0]
    geo = ([stride, stride], [pad, pad], [dil, dil], False, [0, 0], C)
    dgy = torch.zeros_like(gy)
    if a is not None:
        dgy = dgy + F.conv2d(a, w, None, stride, pad, dil, C)
    if b is not None:
        dgy = dgy + F.conv2d(x, b, None, stride, pad, dil, C)
    dx = dw = None
    if need_dx:
        dx = torch.zeros_like(x) if b is None else torch.ops.aten.convolution_backward(gy, x, b, None, *geo, [True, False, False])[0]
    if need_dw:
        dw = torch.zeros_like(w) if a is None else torch.ops.aten.convolution_backward(gy, a, w, None, *geo, [False, True, False])[1]
    return dx, dw, dgy

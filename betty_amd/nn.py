"""Declared layer structure for OPAQUE inner problems: batch normalisation whose share of a Hessian-vector product is fused.

The reference takes ``H p`` as the double backward ``torch.autograd.grad(in_grad, params, grad_outputs=p)``
(betty/hypergradient/cg.py:39-41, neumann.py:62).  For a convolutional inner network with training-mode batch norm — BASELINE cfg 3,
the ResNet-12 of examples/implicit_maml/models.py:278-483 — ATen differentiates ``native_batch_norm_backward`` by decomposing it into
~340 element-wise and per-channel reduction launches per layer and product: 42 % of the kernel time of a hypergradient step
(profiles/r06_cfg3_step_kernel_breakdown.txt), all of it streaming over three activation-sized tensors.

``FusedBatchNorm2d`` / ``fuse_batchnorm_(module)`` declare the layer instead, the way ``hypergradient_structure`` declares an inner
loss: forward and first backward stay ATen's own kernels (``native_batch_norm`` / ``native_batch_norm_backward`` — MIOpen), but they
are tied into the autograd graph as two ``autograd.Function`` nodes, and the backward OF the backward node — what an HVP's double
backward runs — is ``bhg_bn_backward_vjp`` (csrc/bhg_bn.hip): two launches, 32 bytes per element, deterministic.

Parameters, buffers, ``state_dict`` keys, running-statistics updates and eval-mode behaviour are ``torch.nn.BatchNorm2d``'s own (the
class is a subclass that only overrides ``forward`` for CUDA fp32 training-mode inputs); on anything else — CPU tensors, eval mode,
other dtypes, channels-last — it IS ``nn.BatchNorm2d``.  Third derivatives are not provided (the backward of the backward node is
``once_differentiable``): implicit differentiation needs second order only.

``PointwiseConv2d`` and ``DepthwiseConv2d`` (further down) declare the other two layers of a DARTS / MobileNet-style block,
ReLU -> depthwise k x k -> 1 x 1 -> BatchNorm2d; ``declare_layers_(module, depthwise=True)`` applies all three.  ``FusedLayerNorm``
(at the end) is the same declaration for ``nn.LayerNorm`` — the normalisation of a transformer block;
``declare_layers_(module, layernorm=True)`` applies it; ``FusedGroupNorm`` / ``declare_layers_(module, groupnorm=True)`` do the same for
``nn.GroupNorm``, and ``FusedRMSNorm`` / ``declare_layers_(module, rmsnorm=True)`` / ``rms_norm`` / ``declared_rmsnorm()`` for
``nn.RMSNorm``.  ``scaled_dot_product_attention`` / ``declared_attention()`` (last) declare the
attention core for short sequences: a function and a context manager, because attention is not a module;
``tiled_scaled_dot_product_attention`` / ``declared_attention(tiled=True)`` extend it to 512 tokens (opt-in).  ``gelu``, ``silu``,
``tanh``, ``sigmoid``, ``softplus``, ``glu`` and ``gated_activation`` (at the very end) declare the smooth activations: functions,
``declared_activations()`` as a context manager and ``declare_activations_(module)`` / ``declare_layers_(module, activations=True)``.
``cross_entropy`` / ``declared_cross_entropy()`` / ``DeclaredCrossEntropyLoss`` / ``declare_layers_(module, cross_entropy=True)`` (after
them) declare the loss itself.
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _native

__all__ = ["FusedBatchNorm2d", "fuse_batchnorm_", "fused_batchnorm_calls", "PointwiseConv2d", "declare_pointwise_convs_", "DepthwiseConv2d",
           "declare_depthwise_convs_", "depthwise_conv_calls", "FusedLayerNorm", "fuse_layernorm_", "fused_layernorm_calls", "FusedGroupNorm", "fuse_groupnorm_",
           "fused_groupnorm_calls", "FusedRMSNorm", "fuse_rmsnorm_", "fused_rmsnorm_calls", "rms_norm", "declared_rmsnorm", "declare_layers_",
           "scaled_dot_product_attention", "declared_attention", "declared_attention_calls", "tiled_scaled_dot_product_attention",
           "declared_attention_tiled_calls",
           "gelu", "silu", "tanh", "sigmoid", "softplus", "glu", "gated_activation", "declare_activations_", "declared_activations",
           "declared_activation_calls", "DeclaredGELU", "DeclaredSiLU", "DeclaredTanh", "DeclaredSigmoid", "DeclaredSoftplus", "DeclaredGLU",
           "cross_entropy", "declared_cross_entropy", "declared_cross_entropy_calls", "DeclaredCrossEntropyLoss", "declare_cross_entropy_"]

_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran


def fused_batchnorm_calls() -> dict:
    return dict(_CALLS)


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


_WS = {}   # (device, C) -> scratch for the per-slice sums (stream-ordered reuse: one HVP's layers run back to back on one stream)


def _workspace(device, C, lib):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    n = int(lib.bhg_bn_ws_bytes(int(C)))
    ws = _WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


class _BNTrainBackward(torch.autograd.Function):
    """(x, gy, gamma) -> (gx, ggamma, gbeta): batch norm's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, x, gy, gamma, mean, invstd, eps, impl, reserve):
        _CALLS["backward"] += 1
        gy = gy.contiguous()
        # the backward nn.BatchNorm2d itself would have run (MIOpen's when the forward chose MIOpen: same kernels as an undeclared layer)
        gx, gg, gb = torch.ops.aten._batch_norm_impl_index_backward(impl, x, gy, gamma, None, None, mean, invstd, True, eps,
                                                                    [True, gamma is not None, gamma is not None], reserve)
        ctx.save_for_backward(x, gy, gamma, mean, invstd)
        ctx.set_materialize_grads(False)
        return gx, gg, gb

    @staticmethod
    @once_differentiable
    def backward(ctx, a, b, c):
        x, gy, gamma, mean, invstd = ctx.saved_tensors
        _CALLS["backward_vjp"] += 1
        dx, dgy, dgamma = _VJP_IMPL[0](x, gy, a, gamma, mean, invstd, b, c)
        return dx, dgy, dgamma, None, None, None, None, None


def _vjp_hip(x, gy, a, gamma, mean, invstd, b, c):
    """(dx, dgy, dgamma) through bhg_bn_backward_vjp.  The product's only implementation: it raises when the HIP extension is missing or
    the tensors are not on the GPU."""
    if not x.is_cuda:
        raise _native.NativeLibraryError("FusedBatchNorm2d's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) else t.to(torch.float32).contiguous().clone()

    a, b, c = prep(a), prep(b), prep(c)
    dx, dgy = torch.empty_like(x), torch.empty_like(x)
    dgamma = torch.empty_like(gamma) if gamma is not None else None
    ws = _workspace(x.device, C, lib)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _native.check(
        lib.bhg_bn_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a), ptr(gamma), mean.data_ptr(), invstd.data_ptr(), ptr(b), ptr(c),
                                int(N), int(C), int(HW), dx.data_ptr(), dgy.data_ptr(), ptr(dgamma), ws.data_ptr(), ws.numel(), _stream()),
        "bhg_bn_backward_vjp")
    return dx, dgy, dgamma


_VJP_IMPL = [_vjp_hip]   # TEST HOOK ONLY (tests/test_fused_batchnorm.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _BNTrain(torch.autograd.Function):
    """Training-mode batch norm on ATen's own kernel; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps):
        _CALLS["forward"] += 1
        # F.batch_norm's own dispatch (MIOpen / native): (output, batch mean, batch 1 / sqrt(var + eps), reserve space, implementation)
        y, mean, invstd, reserve, impl = torch._batch_norm_impl_index(x, gamma, beta, running_mean, running_var, True, momentum, eps,
                                                                      torch.backends.cudnn.enabled)
        ctx.save_for_backward(x, gamma, mean, invstd, reserve)
        ctx.eps, ctx.impl = eps, impl
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, mean, invstd, reserve = ctx.saved_tensors
        gx, gg, gb = _BNTrainBackward.apply(x, gy, gamma, mean, invstd, ctx.eps, ctx.impl, reserve)
        return gx, gg, gb, None, None, None, None


class FusedBatchNorm2d(torch.nn.BatchNorm2d):
    """``nn.BatchNorm2d`` whose double backward is fused (module docstring)."""

    def _fusable(self, x) -> bool:
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.data_ptr() % 16 == 0
                and (self.training or (self.running_mean is None and self.running_var is None))
                and (self.weight is None) == (self.bias is None)
                and (self.weight is None or (self.weight.dtype == torch.float32 and self.weight.is_contiguous())))

    def forward(self, x):
        if not self._fusable(x) or not torch.is_grad_enabled():
            return super().forward(x)
        self._check_input_dim(x)
        # nn.BatchNorm2d.forward's bookkeeping of the running statistics, restated (torch/nn/modules/batchnorm.py)
        factor = 0.0 if self.momentum is None else self.momentum
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            factor = 1.0 / float(self.num_batches_tracked) if self.momentum is None else self.momentum
        rm = self.running_mean if (not self.training or self.track_running_stats) else None
        rv = self.running_var if (not self.training or self.track_running_stats) else None
        return _BNTrain.apply(x, self.weight, self.bias, rm, rv, factor, self.eps)


def fuse_batchnorm_(module: torch.nn.Module) -> int:
    """Declare every ``nn.BatchNorm2d`` of ``module`` (exact class; subclasses are left alone) as :class:`FusedBatchNorm2d`, in place:
    same parameters, buffers and hooks, only the class changes.  Returns how many layers were declared."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.BatchNorm2d:
            m.__class__ = FusedBatchNorm2d
            n += 1
    return n


class PointwiseConv2d(torch.nn.Conv2d):
    """``nn.Conv2d`` with a 1 x 1 kernel (stride 1, no padding, one group) evaluated as what it is — a matrix product over the channels,
    ``y[n] = W x[n]`` — so that autograd's double backward of it (cg.py:39-41, neumann.py:62) is three more matrix products on
    rocBLAS / hipBLASLt instead of MIOpen's convolution double backward, which for these shapes can fall to a PER-SAMPLE im2col + GEMM
    loop: on BASELINE cfg 3's ResNet-12 the four 1 x 1 shortcut projections cost 25 launches per sample-loop, 12.6 k ``Im2d2Col`` + 16.6 k
    small GEMM launches and ~220 ms of a 900 ms step (profiles/r06_cfg3_step_kernel_breakdown_declared_batchnorm.txt).  Same parameters,
    ``state_dict`` and results to fp32 rounding; any other configuration of the layer IS ``nn.Conv2d``."""

    def _pointwise(self) -> bool:
        return (self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding in ((0, 0), "valid") and self.dilation == (1, 1)
                and self.groups == 1 and self.padding_mode == "zeros")

    def forward(self, x):
        if not self._pointwise() or x.dim() != 4:
            return super().forward(x)
        n, _, h, w = x.shape
        y = torch.matmul(self.weight.reshape(self.out_channels, self.in_channels), x.reshape(n, self.in_channels, h * w))
        if self.bias is not None:
            y = y + self.bias.reshape(1, -1, 1)
        return y.reshape(n, self.out_channels, h, w)


def declare_pointwise_convs_(module: torch.nn.Module) -> int:
    """Re-class every 1 x 1 / stride 1 / ungrouped ``nn.Conv2d`` of ``module`` (exact class) as :class:`PointwiseConv2d`, in place."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.Conv2d and PointwiseConv2d._pointwise(m):
            m.__class__ = PointwiseConv2d
            n += 1
    return n


# ---- DepthwiseConv2d: the depthwise convolution of a DARTS SepConv / DilConv (or MobileNet) block ------------------------------------------
# ReLU -> depthwise k x k -> 1 x 1 -> BatchNorm2d: with PointwiseConv2d and FusedBatchNorm2d this declares the whole block.  ATen's
# _convolution_double_backward handles a grouped convolution with a loop over its groups — C tiny convolutions per depthwise layer and
# term of a Hessian-vector product, enqueue-bound.  Declared, the layer's forward and first backward stay ATen's own
# kernels, tied into the graph as two autograd.Function nodes as for batch norm, and the backward OF the backward node is one
# bhg_dwconv_backward_vjp call (csrc/bhg_dwconv.hip): at most four launches.
_DW_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_DW_KERNELS, _DW_STRIDES, _DW_DILATIONS = (3, 5, 7), (1, 2), (1, 2)   # the family bhg_dwconv_backward_vjp takes


def depthwise_conv_calls() -> dict:
    return dict(_DW_CALLS)


_DW_WS = {}   # (device, stream) -> scratch for the per-slice sums of dw


def _dw_workspace(device, C, k, lib):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    n = int(lib.bhg_dwconv_ws_bytes(int(C), int(k)))
    ws = _DW_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _DW_WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


def _dw_vjp_hip(x, w, gy, a, b, stride, pad, dil, need_dx=True, need_dw=True):
    """(dx, dw, dgy) through bhg_dwconv_backward_vjp; dx / dw are None where not needed.  The product's only implementation: it raises
    when the HIP extension is missing or the tensors are not on the GPU."""
    if not x.is_cuda:
        raise _native.NativeLibraryError("DepthwiseConv2d's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    N, C, H, W = x.shape
    k = w.shape[-1]

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) else t.to(torch.float32).contiguous().clone()

    x, w, gy, a, b = prep(x), prep(w), prep(gy), prep(a), prep(b)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if need_dw else None
    dgy = torch.empty_like(gy)
    ws = _dw_workspace(x.device, C, k, lib)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _native.check(
        lib.bhg_dwconv_backward_vjp(x.data_ptr(), w.data_ptr(), gy.data_ptr(), ptr(a), ptr(b), int(N), int(C), int(H), int(W), int(k),
                                    int(stride), int(pad), int(dil), ptr(dx), ptr(dw), dgy.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
        "bhg_dwconv_backward_vjp")
    return dx, dw, dgy


_DW_VJP_IMPL = [_dw_vjp_hip]   # TEST HOOK ONLY (tests/test_depthwise_conv.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _DWConvBackward(torch.autograd.Function):
    """(x, w, gy) -> (gx, gw): the depthwise convolution's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, x, w, gy, stride, pad, dil, mask):
        _DW_CALLS["backward"] += 1
        gy = gy.contiguous()
        # the backward nn.Conv2d itself would have run: the same kernels as an undeclared layer
        gx, gw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [stride, stride], [pad, pad], [dil, dil], False, [0, 0], w.shape[0],
                                                        [bool(mask[0]), bool(mask[1]), False])
        ctx.save_for_backward(x, w, gy)
        ctx.geometry = (stride, pad, dil)
        ctx.set_materialize_grads(False)
        return gx, gw

    @staticmethod
    @once_differentiable
    def backward(ctx, a, b):
        x, w, gy = ctx.saved_tensors
        _DW_CALLS["backward_vjp"] += 1
        dx, dw, dgy = _DW_VJP_IMPL[0](x, w, gy, a, b, *ctx.geometry, need_dx=ctx.needs_input_grad[0], need_dw=ctx.needs_input_grad[1])
        return dx, dw, dgy, None, None, None, None


class _DWConv(torch.autograd.Function):
    """The depthwise convolution on ATen's own kernel; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, x, w, stride, pad, dil):
        _DW_CALLS["forward"] += 1
        ctx.save_for_backward(x, w)
        ctx.geometry = (stride, pad, dil)
        return torch.nn.functional.conv2d(x, w, None, stride, pad, dil, w.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx, gw = _DWConvBackward.apply(x, w, gy, *ctx.geometry, (ctx.needs_input_grad[0], ctx.needs_input_grad[1]))
        return gx, gw, None, None, None


class DepthwiseConv2d(torch.nn.Conv2d):
    """``nn.Conv2d`` with ``groups == in_channels == out_channels`` whose double backward is fused (comment above).  Same parameters and
    ``state_dict``; any configuration or input outside the declared family IS ``nn.Conv2d``."""

    def _family(self) -> bool:
        k, s, d, p = self.kernel_size, self.stride, self.dilation, self.padding
        return (self.groups == self.in_channels == self.out_channels and self.in_channels <= 65535 and self.bias is None
                and self.padding_mode == "zeros" and k[0] == k[1] and k[0] in _DW_KERNELS and s[0] == s[1] and s[0] in _DW_STRIDES
                and d[0] == d[1] and d[0] in _DW_DILATIONS and not isinstance(p, str) and p[0] == p[1] and isinstance(p[0], int)
                and 0 <= p[0] <= d[0] * (k[0] - 1))

    def _declared(self, x) -> bool:
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.data_ptr() % 16 == 0):
            return False
        return self.weight.dtype == torch.float32 and self.weight.is_contiguous()

    def forward(self, x):
        if not self._family() or not self._declared(x) or not torch.is_grad_enabled():
            return super().forward(x)
        k, s, d, p = self.kernel_size[0], self.stride[0], self.dilation[0], self.padding[0]
        if min(x.shape[2], x.shape[3]) + 2 * p - d * (k - 1) - 1 < 0 or x.shape[1] != self.in_channels:
            return super().forward(x)     # nn.Conv2d's own error
        return _DWConv.apply(x, self.weight, s, p, d)


def declare_depthwise_convs_(module: torch.nn.Module) -> int:
    """Re-class every depthwise ``nn.Conv2d`` of ``module`` (exact class) in :class:`DepthwiseConv2d`'s family, in place."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.Conv2d and DepthwiseConv2d._family(m):
            m.__class__ = DepthwiseConv2d
            n += 1
    return n


# ---- FusedLayerNorm: the normalisation of a transformer block -------------------------------------------------------------------------------
# ATen differentiates native_layer_norm_backward by decomposition, as it does for batch norm: 216 ATen operator calls per layer and
# product on a 64 x 768 input, most of them activation-sized streaming passes.  Declared, the layer's forward and first backward stay
# ATen's own kernels (native_layer_norm / native_layer_norm_backward), tied into the graph as two autograd.Function nodes as for batch
# norm, and the backward OF the backward node is one bhg_layernorm_backward_vjp call (csrc/bhg_layernorm.hip): at most two launches.
_LN_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_LN_MAX_D = 8192                                               # the family bhg_layernorm_backward_vjp takes: rows of at most 8192 elements


def fused_layernorm_calls() -> dict:
    return dict(_LN_CALLS)


_LN_WS = {}   # (device, stream) -> scratch for the per-slice sums of dgamma


def _ln_workspace(device, D, lib):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    n = int(lib.bhg_layernorm_ws_bytes(int(D)))
    ws = _LN_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _LN_WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


def _ln_vjp_hip(x, gy, a, gamma, mean, rstd, b, c):
    """(dx, dgy, dgamma) through bhg_layernorm_backward_vjp; dgamma is None when gamma is.  The product's only implementation: it raises
    when the HIP extension is missing or the tensors are not on the GPU."""
    if not x.is_cuda:
        raise _native.NativeLibraryError("FusedLayerNorm's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    M = mean.numel()
    D = x.numel() // M

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) else t.to(torch.float32).contiguous().clone()

    x, gy, a, gamma, mean, rstd, b, c = (prep(t) for t in (x, gy, a, gamma, mean, rstd, b, c))
    dx, dgy = torch.empty_like(x), torch.empty_like(x)
    dgamma = torch.empty_like(gamma) if gamma is not None else None
    ws = _ln_workspace(x.device, D, lib)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _native.check(
        lib.bhg_layernorm_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a), ptr(gamma), mean.data_ptr(), rstd.data_ptr(), ptr(b), ptr(c),
                                       int(M), int(D), dx.data_ptr(), dgy.data_ptr(), ptr(dgamma), ws.data_ptr(), ws.numel(), _stream()),
        "bhg_layernorm_backward_vjp")
    return dx, dgy, dgamma


_LN_VJP_IMPL = [_ln_vjp_hip]   # TEST HOOK ONLY (tests/test_fused_layernorm.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _LNBackward(torch.autograd.Function):
    """(x, gy, gamma) -> (gx, ggamma, gbeta): layer norm's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, x, gy, gamma, beta, mean, rstd, normalized_shape, need_dx):
        _LN_CALLS["backward"] += 1
        gy = gy.contiguous()
        # the backward nn.LayerNorm itself would have run: the same kernels as an undeclared layer
        gx, gg, gb = torch.ops.aten.native_layer_norm_backward(gy, x, normalized_shape, mean, rstd, gamma, beta,
                                                               [bool(need_dx), gamma is not None, beta is not None])
        ctx.save_for_backward(x, gy, gamma, mean, rstd)
        ctx.set_materialize_grads(False)
        return (gx if need_dx else None), (gg if gamma is not None else None), (gb if beta is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, a, b, c):
        x, gy, gamma, mean, rstd = ctx.saved_tensors
        _LN_CALLS["backward_vjp"] += 1
        dx, dgy, dgamma = _LN_VJP_IMPL[0](x, gy, a, gamma, mean, rstd, b, c)
        return dx, dgy, dgamma, None, None, None, None, None


class _LNForward(torch.autograd.Function):
    """Layer norm on ATen's own kernel; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, normalized_shape, eps):
        _LN_CALLS["forward"] += 1
        y, mean, rstd = torch.native_layer_norm(x, normalized_shape, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.normalized_shape = normalized_shape
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        gx, gg, gb = _LNBackward.apply(x, gy, gamma, beta, mean, rstd, ctx.normalized_shape, ctx.needs_input_grad[0])
        return gx, gg, gb, None, None


class FusedLayerNorm(torch.nn.LayerNorm):
    """``nn.LayerNorm`` whose double backward is fused (comment above).  Same parameters and ``state_dict``
    (``elementwise_affine=False`` and ``bias=False`` included); an input outside the declared family — not CUDA fp32 contiguous and
    16-byte aligned, more than 8192 normalised elements, grad disabled — IS ``nn.LayerNorm``.  Third derivatives are not provided."""

    def _declared(self, x) -> bool:
        ns = tuple(self.normalized_shape)
        D = 1
        for v in ns:
            D *= v
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0 and x.numel() > 0):
            return False
        if not (1 <= D <= _LN_MAX_D and x.dim() >= len(ns) and tuple(x.shape[x.dim() - len(ns):]) == ns):
            return False                  # a shape mismatch: nn.LayerNorm's own error
        return all(p is None or (p.dtype == torch.float32 and p.is_contiguous() and p.device == x.device) for p in (self.weight, self.bias))

    def forward(self, x):
        if not torch.is_grad_enabled() or not self._declared(x):
            return super().forward(x)
        return _LNForward.apply(x, self.weight, self.bias, list(self.normalized_shape), self.eps)


def fuse_layernorm_(module: torch.nn.Module) -> int:
    """Declare every ``nn.LayerNorm`` of ``module`` (exact class; subclasses are left alone) as :class:`FusedLayerNorm`, in place: same
    parameters and hooks, only the class changes.  Returns how many layers were declared."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.LayerNorm:
            m.__class__ = FusedLayerNorm
            n += 1
    return n


# ---- FusedGroupNorm: the normalisation of a ResNet whose batches are too small for batch norm ------------------------------------------------
# ATen's derivative formula for native_group_norm switches to infinitely_differentiable_native_group_norm_backward as soon as grad mode
# is on: under create_graph=True even the first backward is a chain of element-wise operators, and the double backward a longer one.
# Declared, the layer's forward and first backward are ATen's single kernels (native_group_norm / native_group_norm_backward), tied into
# the graph as two autograd.Function nodes as for layer norm, and the backward OF the backward node is one bhg_groupnorm_backward_vjp
# call (csrc/bhg_groupnorm.hip): at most two launches.
_GN_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_GN_MAX_D = 1 << 20                                            # the family bhg_groupnorm_backward_vjp takes: rows of at most 2^20 elements


def fused_groupnorm_calls() -> dict:
    return dict(_GN_CALLS)


_GN_WS = {}   # (device, stream) -> scratch for the per-sample sums of dgamma


def _gn_workspace(device, N, C, lib):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    n = int(lib.bhg_groupnorm_ws_bytes(int(N), int(C)))
    ws = _GN_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _GN_WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


def _gn_vjp_hip(x, gy, a, gamma, mean, rstd, b, c, G):
    """(dx, dgy, dgamma) through bhg_groupnorm_backward_vjp; dgamma is None when gamma is.  The product's only implementation: it raises
    when the HIP extension is missing or the tensors are not on the GPU."""
    if not x.is_cuda:
        raise _native.NativeLibraryError("FusedGroupNorm's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    N, C = int(x.shape[0]), int(x.shape[1])
    HW = x.numel() // (N * C)

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) else t.to(torch.float32).contiguous().clone()

    x, gy, a, gamma, mean, rstd, b, c = (prep(t) for t in (x, gy, a, gamma, mean, rstd, b, c))
    dx, dgy = torch.empty_like(x), torch.empty_like(x)
    dgamma = torch.empty_like(gamma) if gamma is not None else None
    ws = _gn_workspace(x.device, N, C, lib) if gamma is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _native.check(
        lib.bhg_groupnorm_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a), ptr(gamma), mean.data_ptr(), rstd.data_ptr(), ptr(b), ptr(c),
                                       N, C, int(HW), int(G), dx.data_ptr(), dgy.data_ptr(), ptr(dgamma), ptr(ws),
                                       0 if ws is None else ws.numel(), _stream()),
        "bhg_groupnorm_backward_vjp")
    return dx, dgy, dgamma


_GN_VJP_IMPL = [_gn_vjp_hip]   # TEST HOOK ONLY (tests/test_fused_groupnorm.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _GNBackward(torch.autograd.Function):
    """(x, gy, gamma) -> (gx, ggamma, gbeta): group norm's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, x, gy, gamma, beta, mean, rstd, G, need_dx):
        _GN_CALLS["backward"] += 1
        gy = gy.contiguous()
        N, C = x.shape[0], x.shape[1]
        # the backward nn.GroupNorm itself runs without create_graph: one kernel, not the decomposition
        gx, gg, gb = torch.ops.aten.native_group_norm_backward(gy, x, mean, rstd, gamma, N, C, x.numel() // (N * C), G,
                                                               [bool(need_dx), gamma is not None, beta is not None])
        ctx.save_for_backward(x, gy, gamma, mean, rstd)
        ctx.G = G
        ctx.set_materialize_grads(False)
        return (gx if need_dx else None), (gg if gamma is not None else None), (gb if beta is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, a, b, c):
        x, gy, gamma, mean, rstd = ctx.saved_tensors
        _GN_CALLS["backward_vjp"] += 1
        dx, dgy, dgamma = _GN_VJP_IMPL[0](x, gy, a, gamma, mean, rstd, b, c, ctx.G)
        return dx, dgy, dgamma, None, None, None, None, None


class _GNForward(torch.autograd.Function):
    """Group norm on ATen's own kernel; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps):
        _GN_CALLS["forward"] += 1
        N, C = x.shape[0], x.shape[1]
        y, mean, rstd = torch.native_group_norm(x, gamma, beta, N, C, x.numel() // (N * C), G, eps)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.G = G
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        gx, gg, gb = _GNBackward.apply(x, gy, gamma, beta, mean, rstd, ctx.G, ctx.needs_input_grad[0])
        return gx, gg, gb, None, None


class FusedGroupNorm(torch.nn.GroupNorm):
    """``nn.GroupNorm`` whose double backward is fused (comment above).  Same parameters and ``state_dict`` (``affine=False``
    included); an input outside the declared family — not CUDA fp32 contiguous and 16-byte aligned, fewer than 2 dimensions, more than
    2^20 elements per (sample, group) row, a shape ``nn.GroupNorm`` itself refuses, grad disabled — IS ``nn.GroupNorm``, with its bits and
    its errors.  Third derivatives are not provided."""

    def _declared(self, x) -> bool:
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.is_contiguous() and x.data_ptr() % 16 == 0 and x.numel() > 0):
            return False
        N, C, G = x.shape[0], x.shape[1], self.num_groups
        if C != self.num_channels or G <= 0 or C % G != 0:
            return False                  # nn.GroupNorm's own error
        D = x.numel() // (N * G)
        if not (D <= _GN_MAX_D and N * D > 1 and N * G < 2 ** 31):   # N * D == 1: F.group_norm refuses a single value per group
            return False
        return all(p is None or (p.dtype == torch.float32 and p.is_contiguous() and p.device == x.device) for p in (self.weight, self.bias))

    def forward(self, x):
        if not torch.is_grad_enabled() or not self._declared(x):
            return super().forward(x)
        return _GNForward.apply(x, self.weight, self.bias, self.num_groups, self.eps)


def fuse_groupnorm_(module: torch.nn.Module) -> int:
    """Declare every ``nn.GroupNorm`` of ``module`` (exact class; subclasses are left alone) as :class:`FusedGroupNorm`, in place: same
    parameters and hooks, only the class changes.  Returns how many layers were declared."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.GroupNorm:
            m.__class__ = FusedGroupNorm
            n += 1
    return n


# ---- FusedRMSNorm: the normalisation of a LLaMA-style pre-norm decoder block ---------------------------------------------------------------
# On the GPU nn.RMSNorm runs aten::_fused_rms_norm, whose derivative formula switches to infinitely_differentiable_native_rms_norm_backward
# as soon as grad mode is on: under create_graph=True even the first backward is a chain of element-wise operators, and the double
# backward a longer one.  Declared, the layer's forward and first backward are ATen's single kernels (_fused_rms_norm /
# _fused_rms_norm_backward), tied into the graph as two autograd.Function nodes as for layer norm, and the backward OF the backward node
# is one bhg_rmsnorm_backward_vjp call (csrc/bhg_rmsnorm.hip): at most two launches.
_RMS_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_RMS_MAX_D = 8192                                               # the family bhg_rmsnorm_backward_vjp takes: rows of at most 8192 elements
_TORCH_RMS_NORM = torch.nn.functional.rms_norm                  # what anything outside the family IS


def fused_rmsnorm_calls() -> dict:
    return dict(_RMS_CALLS)


_RMS_WS = {}   # (device, stream) -> scratch for the per-slice sums of dgamma


def _rms_workspace(device, M, D, lib):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    n = int(lib.bhg_rmsnorm_ws_bytes(int(M), int(D)))
    ws = _RMS_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _RMS_WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


def _rms_vjp_hip(x, gy, a, gamma, rstd, b):
    """(dx, dgy, dgamma) through bhg_rmsnorm_backward_vjp; dgamma is None when gamma is.  The product's only implementation: it raises
    when the HIP extension is missing or the tensors are not on the GPU."""
    if not x.is_cuda:
        raise _native.NativeLibraryError("FusedRMSNorm's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    M = rstd.numel()
    D = x.numel() // M

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) else t.to(torch.float32).contiguous().clone()

    x, gy, a, gamma, rstd, b = (prep(t) for t in (x, gy, a, gamma, rstd, b))
    if gamma is None:
        b = None
    dx, dgy = torch.empty_like(x), torch.empty_like(x)
    dgamma = torch.empty_like(gamma) if gamma is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    with torch.cuda.device(x.device):
        ws = _rms_workspace(x.device, M, D, lib) if gamma is not None else None
        _native.check(
            lib.bhg_rmsnorm_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a), ptr(gamma), rstd.data_ptr(), ptr(b), int(M), int(D),
                                         dx.data_ptr(), dgy.data_ptr(), ptr(dgamma), ptr(ws), 0 if ws is None else ws.numel(), _stream()),
            "bhg_rmsnorm_backward_vjp")
    return dx, dgy, dgamma


_RMS_VJP_IMPL = [_rms_vjp_hip]   # TEST HOOK ONLY (tests/test_fused_rmsnorm.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _RMSBackward(torch.autograd.Function):
    """(x, gy, gamma) -> (gx, ggamma): RMS norm's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, x, gy, gamma, rstd, normalized_shape, need_dx):
        _RMS_CALLS["backward"] += 1
        gy = gy.contiguous()
        if x.is_cuda:
            # the backward nn.RMSNorm itself runs without create_graph: one kernel, not the decomposition
            gx, gg = torch.ops.aten._fused_rms_norm_backward(gy, x, normalized_shape, rstd, gamma, [bool(need_dx), gamma is not None])
        else:
            # _fused_rms_norm_backward has no CPU kernel: the closed form (csrc/bhg_rmsnorm.hip), for the CPU plumbing tests only — the
            # module never declares a CPU input
            xh = x * rstd
            g = gy if gamma is None else gy * gamma
            dims = tuple(range(x.dim() - len(normalized_shape), x.dim()))
            gx = rstd * (g - xh * (g * xh).mean(dim=dims, keepdim=True)) if need_dx else None
            gg = (gy * xh).reshape(-1, *normalized_shape).sum(0) if gamma is not None else None
        ctx.save_for_backward(x, gy, gamma, rstd)
        ctx.set_materialize_grads(False)
        return (gx if need_dx else None), (gg if gamma is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, a, b):
        need = ctx.needs_input_grad
        if (a is None and b is None) or not any(need[:3]):
            return (None,) * 6
        x, gy, gamma, rstd = ctx.saved_tensors
        _RMS_CALLS["backward_vjp"] += 1
        dx, dgy, dgamma = _RMS_VJP_IMPL[0](x, gy, a, gamma, rstd, b)
        return (dx if need[0] else None), (dgy if need[1] else None), (dgamma if need[2] else None), None, None, None


class _RMSForward(torch.autograd.Function):
    """RMS norm on ATen's own kernel; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, x, gamma, normalized_shape, eps):
        _RMS_CALLS["forward"] += 1
        y, rstd = torch.ops.aten._fused_rms_norm(x, normalized_shape, gamma, eps)
        ctx.save_for_backward(x, gamma, rstd)
        ctx.normalized_shape = normalized_shape
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, rstd = ctx.saved_tensors
        gx, gg = _RMSBackward.apply(x, gy, gamma, rstd, ctx.normalized_shape, ctx.needs_input_grad[0])
        return gx, gg, None, None


def _rms_declared(x, normalized_shape, weight) -> bool:
    """Whether an RMS norm of ``x`` over ``normalized_shape`` with ``weight`` lies in the declared family (FusedRMSNorm's docstring)."""
    if not (torch.is_grad_enabled() and torch.is_tensor(x) and isinstance(normalized_shape, (list, tuple))):
        return False
    ns = tuple(normalized_shape)
    if not all(isinstance(v, int) for v in ns) or len(ns) == 0:
        return False
    D = 1
    for v in ns:
        D *= v
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0 and x.numel() > 0 and not x.is_nested):
        return False
    if not (1 <= D <= _RMS_MAX_D and x.dim() >= len(ns) and tuple(x.shape[x.dim() - len(ns):]) == ns):
        return False                  # a shape mismatch: the torch function's own error
    if weight is None:
        return True
    return (torch.is_tensor(weight) and weight.dtype == torch.float32 and weight.is_contiguous() and weight.device == x.device
            and tuple(weight.shape) == ns)


def rms_norm(input, normalized_shape, weight=None, eps=None):
    """``torch.nn.functional.rms_norm`` whose double backward is fused (comment above): the hook for hand-written norm modules.  Declared
    inside :class:`FusedRMSNorm`'s family; anything else IS the torch function with the caller's arguments, errors included."""
    if not ((eps is None or isinstance(eps, (int, float))) and _rms_declared(input, normalized_shape, weight)):
        return _TORCH_RMS_NORM(input, normalized_shape, weight, eps)
    return _RMSForward.apply(input, weight, list(normalized_shape), None if eps is None else float(eps))


class FusedRMSNorm(torch.nn.RMSNorm):
    """``nn.RMSNorm`` whose double backward is fused (comment above).  Same parameters and ``state_dict`` (``elementwise_affine=False``
    and ``eps=None`` included; a multi-dimensional ``normalized_shape`` is one row of its product); an input outside the declared family —
    not CUDA fp32 contiguous and 16-byte aligned, more than 8192 normalised elements, zero elements, grad disabled, a weight on another
    device or of another dtype — IS ``nn.RMSNorm``, errors included.  Third derivatives are not provided."""

    def forward(self, x):
        if not _rms_declared(x, tuple(self.normalized_shape), self.weight):
            return super().forward(x)
        return _RMSForward.apply(x, self.weight, list(self.normalized_shape), self.eps)


def fuse_rmsnorm_(module: torch.nn.Module) -> int:
    """Declare every ``nn.RMSNorm`` of ``module`` (exact class; subclasses are left alone) as :class:`FusedRMSNorm`, in place: same
    parameters and hooks, only the class changes.  Returns how many layers were declared."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.RMSNorm:
            m.__class__ = FusedRMSNorm
            n += 1
    return n


@contextlib.contextmanager
def declared_rmsnorm():
    """Inside the context ``torch.nn.functional.rms_norm`` is :func:`rms_norm`: ``nn.RMSNorm`` and model code that calls the torch
    function reach the declaration without being rewritten.  Only the forward that records the graph has to run inside.  Restored on
    exit, exceptions included; nesting is safe."""
    F = torch.nn.functional
    previous = F.rms_norm
    F.rms_norm = rms_norm
    try:
        yield
    finally:
        F.rms_norm = previous


def declare_layers_(module: torch.nn.Module, depthwise: bool = False, layernorm: bool = False, groupnorm: bool = False,
                    activations: bool = False, rmsnorm: bool = False, cross_entropy: bool = False) -> dict:
    """Every layer declaration this module offers, in place: ``{"batchnorm": n, "pointwise_conv": m}``, with ``depthwise=True`` also
    ``"depthwise_conv": k``, with ``layernorm=True`` also ``"layernorm": l``, with ``groupnorm=True`` also ``"groupnorm": g``, with
    ``activations=True`` also ``"activations": a`` (``declare_activations_``, further down), and with ``rmsnorm=True`` also
    ``"rmsnorm": r``, and with ``cross_entropy=True`` also ``"cross_entropy": c`` (``declare_cross_entropy_``, at the very end)."""
    out = {"batchnorm": fuse_batchnorm_(module), "pointwise_conv": declare_pointwise_convs_(module)}
    if depthwise:
        out["depthwise_conv"] = declare_depthwise_convs_(module)
    if layernorm:
        out["layernorm"] = fuse_layernorm_(module)
    if groupnorm:
        out["groupnorm"] = fuse_groupnorm_(module)
    if activations:
        out["activations"] = declare_activations_(module)
    if rmsnorm:
        out["rmsnorm"] = fuse_rmsnorm_(module)
    if cross_entropy:
        out["cross_entropy"] = declare_cross_entropy_(module)
    return out


# ---- declared attention: the core of a transformer block, short sequences -------------------------------------------------------------------
# The fused SDPA kernels have no double backward, and on the math path ATen differentiates bmm -> softmax -> bmm by decomposition, per
# head batch and per product.  Declared, the forward is the math path on ATen's kernels, the first backward is written out in torch
# operations, both tied into the graph as two autograd.Function nodes as for layer norm, and the backward OF the backward node is one
# bhg_attention_backward_vjp call (csrc/bhg_attention.hip): ONE launch, one workgroup per (batch, head), no workspace.
_ATTN_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_ATTN_MAX = 64                                                   # the family bhg_attention_backward_vjp takes: L, S, d <= 64
_TORCH_SDPA = torch.nn.functional.scaled_dot_product_attention   # what anything outside the family IS


def declared_attention_calls() -> dict:
    return dict(_ATTN_CALLS)


_ATTN_TILED_WS = {}   # (device, stream) -> the tiled kernels' row statistics


def _attn_tiled_workspace(device, n):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    ws = _ATTN_TILED_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _ATTN_TILED_WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


def _attn_vjp_hip(q, k, v, go, aq, ak, av, mask, causal, scale, need):
    """(dq, dk, dv, dgo) through bhg_attention_backward_vjp; ``need`` says which of the four are wanted (the others are None).  Strided
    views are handed in as they are.  The product's only implementation: it raises when the HIP extension is missing or the tensors are
    not on the GPU."""
    return _attn_vjp_launch(q, k, v, go, aq, ak, av, mask, causal, scale, need, False)


def _attn_tiled_vjp_hip(q, k, v, go, aq, ak, av, mask, causal, scale, need):
    """The same through bhg_attention_tiled_backward_vjp (L, S <= 512): two launches and a workspace cached per (device, stream)."""
    return _attn_vjp_launch(q, k, v, go, aq, ak, av, mask, causal, scale, need, True)


def _attn_vjp_launch(q, k, v, go, aq, ak, av, mask, causal, scale, need, tiled):
    if not q.is_cuda:
        raise _native.NativeLibraryError("declared attention's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    B, H, L, d = q.shape
    S = k.shape[2]

    def prep(t, shape):
        if t is None:
            return None
        t = t.detach()
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        if tuple(t.shape) != shape:
            t = t.expand(shape)
        if (d > 1 and t.stride(3) != 1) or t.data_ptr() % 16 != 0:
            t = t.contiguous() if not t.is_contiguous() else t.clone()
        return t

    lshape, sshape = (B, H, L, d), (B, H, S, d)
    ins = [prep(t, sh) for t, sh in zip((q, k, v, go, aq, ak, av), (lshape, sshape, sshape, lshape, lshape, sshape, sshape))]
    strides = (ctypes.c_longlong * 28)()
    for i, t in enumerate(ins):
        if t is not None:
            strides[4 * i:4 * i + 4] = list(t.stride())
    mstrides = None
    if mask is not None:
        mask = mask.detach()
        mstrides = (ctypes.c_longlong * 4)(*mask.stride())
    outs = [torch.empty(sh, dtype=torch.float32, device=q.device) if on else None for on, sh in zip(need, (lshape, sshape, sshape, lshape))]
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    with torch.cuda.device(q.device):
        if tiled:
            ws = _attn_tiled_workspace(q.device, int(lib.bhg_attention_tiled_ws_bytes(B, H, L)))
            _native.check(
                lib.bhg_attention_tiled_backward_vjp(*(ptr(t) for t in ins), strides, ptr(mask), mstrides, 1 if causal else 0, float(scale),
                                                     B, H, L, S, d, *(ptr(t) for t in outs), ws.data_ptr(), ws.numel(), _stream()),
                "bhg_attention_tiled_backward_vjp")
        else:
            _native.check(
                lib.bhg_attention_backward_vjp(*(ptr(t) for t in ins), strides, ptr(mask), mstrides, 1 if causal else 0, float(scale), B, H, L,
                                               S, d, *(ptr(t) for t in outs), _stream()),
                "bhg_attention_backward_vjp")
    return tuple(outs)


_ATTN_VJP_IMPL = [_attn_vjp_hip]   # TEST HOOK ONLY (tests/test_declared_attention.py swaps in the float64 restatement to check the graph plumbing on CPU)


def _attn_first_backward(ctx, calls, q, k, v, go, P, mask, causal, scale):
    calls["backward"] += 1
    gP = go @ v.transpose(-1, -2)
    gS = P * (gP - (P * gP).sum(-1, keepdim=True))
    gq, gk, gv = (gS @ k) * scale, (gS.transpose(-1, -2) @ q) * scale, P.transpose(-1, -2) @ go
    ctx.save_for_backward(q, k, v, go, mask)
    ctx.causal, ctx.scale = causal, scale
    ctx.set_materialize_grads(False)
    return gq, gk, gv


def _attn_double_backward(ctx, calls, impl, aq, ak, av):
    q, k, v, go, mask = ctx.saved_tensors
    if aq is None and ak is None and av is None:
        return (None,) * 8
    calls["backward_vjp"] += 1
    dq, dk, dv, dgo = impl[0](q, k, v, go, aq, ak, av, mask, ctx.causal, ctx.scale, tuple(ctx.needs_input_grad[:4]))
    return dq, dk, dv, dgo, None, None, None, None


def _attn_forward(ctx, calls, q, k, v, mask, causal, scale):
    calls["forward"] += 1
    sc = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        sc = sc + mask
    if causal:
        sc = sc.masked_fill(torch.ones(sc.shape[-2:], dtype=torch.bool, device=sc.device).triu(1), float("-inf"))
    P = torch.softmax(sc, dim=-1)
    ctx.save_for_backward(q, k, v, P, mask)
    ctx.causal, ctx.scale = causal, scale
    return P @ v


class _AttnBackward(torch.autograd.Function):
    """(q, k, v, go) -> (gq, gk, gv): attention's first backward as a graph node whose own backward is ONE fused call.  P is what the
    forward computed; its dependence on q and k is part of the fused call."""

    @staticmethod
    def forward(ctx, q, k, v, go, P, mask, causal, scale):
        return _attn_first_backward(ctx, _ATTN_CALLS, q, k, v, go, P, mask, causal, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, aq, ak, av):
        return _attn_double_backward(ctx, _ATTN_CALLS, _ATTN_VJP_IMPL, aq, ak, av)


class _AttnForward(torch.autograd.Function):
    """The math-path attention on ATen's own kernels; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, causal, scale):
        return _attn_forward(ctx, _ATTN_CALLS, q, k, v, mask, causal, scale)

    @staticmethod
    def backward(ctx, go):
        q, k, v, P, mask = ctx.saved_tensors
        gq, gk, gv = _AttnBackward.apply(q, k, v, go, P, mask, ctx.causal, ctx.scale)
        return gq, gk, gv, None, None, None


# Beyond 64 tokens (opt-in): the same two nodes, counted apart, whose double backward is ONE bhg_attention_tiled_backward_vjp call
# (csrc/bhg_attention_tiled.hip: two launches over 64 x 32 score tiles and a workspace for the row statistics).  The forward still
# materialises and saves P.
_ATTN_TILED_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}
_ATTN_TILED_MAX = 512   # the largest measured length up to which no measured shape is slower declared (profiles/attention_tiled_double_backward.txt)
_ATTN_TILED_VJP_IMPL = [_attn_tiled_vjp_hip]   # TEST HOOK ONLY (tests/test_declared_attention_tiled.py swaps in the float64 restatement)


def declared_attention_tiled_calls() -> dict:
    return dict(_ATTN_TILED_CALLS)


class _AttnTiledBackward(_AttnBackward):
    @staticmethod
    def forward(ctx, q, k, v, go, P, mask, causal, scale):
        return _attn_first_backward(ctx, _ATTN_TILED_CALLS, q, k, v, go, P, mask, causal, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, aq, ak, av):
        return _attn_double_backward(ctx, _ATTN_TILED_CALLS, _ATTN_TILED_VJP_IMPL, aq, ak, av)


class _AttnTiledForward(_AttnForward):
    @staticmethod
    def forward(ctx, q, k, v, mask, causal, scale):
        return _attn_forward(ctx, _ATTN_TILED_CALLS, q, k, v, mask, causal, scale)

    @staticmethod
    def backward(ctx, go):
        q, k, v, P, mask = ctx.saved_tensors
        gq, gk, gv = _AttnTiledBackward.apply(q, k, v, go, P, mask, ctx.causal, ctx.scale)
        return gq, gk, gv, None, None, None


def _declared_mask(q, k, v, attn_mask, dropout_p, is_causal, kw, max_len=_ATTN_MAX):
    """False when the call is outside the declared family (at most ``max_len`` queries and keys); otherwise the additive fp32 mask as a
    (B, H, L, S) view, or None."""
    if kw.pop("enable_gqa", False) or kw:
        return False
    if not (torch.is_grad_enabled() and dropout_p == 0.0 and all(torch.is_tensor(t) for t in (q, k, v))):
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.device == q.device and not t.is_nested for t in (q, k, v)):
        return False
    B, H, L, d = q.shape
    S = k.shape[2]
    if not (tuple(k.shape) == (B, H, S, d) and tuple(v.shape) == (B, H, S, d) and B >= 1 and H >= 1 and B * H < 2 ** 31):
        return False
    if not (1 <= L <= max_len and 1 <= S <= max_len and 1 <= d <= _ATTN_MAX):
        return False
    if d > 1 and not all(t.stride(3) == 1 for t in (q, k, v)):
        return False
    if attn_mask is None:
        return None
    if is_causal or not torch.is_tensor(attn_mask) or attn_mask.requires_grad or attn_mask.device != q.device or attn_mask.dim() > 4:
        return False   # (a mask AND is_causal: the torch function's own error)
    if attn_mask.dtype == torch.bool:
        attn_mask = torch.zeros(attn_mask.shape, dtype=torch.float32, device=q.device).masked_fill_(~attn_mask, float("-inf"))   # once
    elif attn_mask.dtype != torch.float32:
        return False
    try:
        return attn_mask.expand(B, H, L, S)
    except RuntimeError:
        return False


def scaled_dot_product_attention(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, **kw):
    """``torch.nn.functional.scaled_dot_product_attention`` whose double backward is fused (comment above), for CUDA fp32 4-D inputs with
    a unit last stride, at most 64 queries, 64 keys and 64 elements per head, grad enabled, no dropout, no ``enable_gqa``, and a mask
    that is absent, bool or fp32 and does not require grad.  Anything else IS the torch function with the caller's arguments, errors
    included.  Third derivatives are not provided."""
    mask = _declared_mask(query, key, value, attn_mask, dropout_p, is_causal, dict(kw))
    if mask is False:
        return _TORCH_SDPA(query, key, value, attn_mask=attn_mask, dropout_p=dropout_p, is_causal=is_causal, scale=scale, **kw)
    s = 1.0 / math.sqrt(query.shape[-1]) if scale is None else float(scale)
    return _AttnForward.apply(query, key, value, mask, bool(is_causal), s)


def tiled_scaled_dot_product_attention(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, **kw):
    """``scaled_dot_product_attention`` above, whose declared family also takes more than 64 and at most ``_ATTN_TILED_MAX`` queries and
    keys (d <= 64 and every other condition as above).  With at most 64 of both it IS the function above: the same nodes, the same
    counters.  Longer, the double backward is one bhg_attention_tiled_backward_vjp call, counted by ``declared_attention_tiled_calls()``.
    Anything else IS the torch function with the caller's arguments, errors included."""
    mask = _declared_mask(query, key, value, attn_mask, dropout_p, is_causal, dict(kw), max(_ATTN_MAX, _ATTN_TILED_MAX))
    if mask is False:
        return _TORCH_SDPA(query, key, value, attn_mask=attn_mask, dropout_p=dropout_p, is_causal=is_causal, scale=scale, **kw)
    s = 1.0 / math.sqrt(query.shape[-1]) if scale is None else float(scale)
    node = _AttnForward if max(query.shape[2], key.shape[2]) <= _ATTN_MAX else _AttnTiledForward
    return node.apply(query, key, value, mask, bool(is_causal), s)


@contextlib.contextmanager
def declared_attention(tiled: bool = False):
    """Inside the context ``torch.nn.functional.scaled_dot_product_attention`` is the function above: ``nn.MultiheadAttention``,
    ``nn.TransformerEncoder`` and model code that calls the torch function reach the declaration without being rewritten, and
    ``sdpa_kernel(MATH)`` is not needed for shapes in the family.  ``tiled=True`` installs ``tiled_scaled_dot_product_attention``
    instead (sequences of up to ``_ATTN_TILED_MAX`` tokens).  Only the forward that records the graph has to run inside; the
    solve's double backward runs wherever it runs.  Restored on exit, exceptions included; nesting is safe."""
    F = torch.nn.functional
    previous = F.scaled_dot_product_attention
    F.scaled_dot_product_attention = tiled_scaled_dot_product_attention if tiled else scaled_dot_product_attention
    try:
        yield
    finally:
        F.scaled_dot_product_attention = previous


# ---- declared activations: GELU, SiLU, tanh, sigmoid, softplus, GLU and the gated forms of a transformer's feed-forward block --------------
# ATen differentiates an activation's backward by decomposition: 5 (tanh) to 37 (tanh-approximated GELU) element-wise launches per
# activation and product, and F.silu's FIRST backward is already 8 operators once grad mode is on.  Declared, the forward is the torch
# function's own kernel and the first backward ATen's single backward kernel (gelu_backward, silu_backward, tanh_backward,
# sigmoid_backward, softplus_backward, glu_backward; a few torch operations for the gated form), tied into the graph as two
# autograd.Function nodes as for layer norm, and the backward OF the backward node is one bhg_act_backward_vjp or
# bhg_gated_act_backward_vjp call (csrc/bhg_activation.hip): ONE launch, no workspace.  Activations are functions as well as modules:
# functions, a context manager (like declared_attention) and a re-classing of the nn modules (like fuse_layernorm_).
_ACT_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_ACT_KINDS = {"gelu": 0, "gelu_tanh": 1, "silu": 2, "tanh": 3, "sigmoid": 4, "softplus": 5}   # include/bhg.h: BHG_ACT_*
_ACT_GATED = ("gelu", "gelu_tanh", "silu", "tanh", "sigmoid")
_ACT_MIN_NUMEL = 1   # no measured shape is slower declared (profiles/activation_double_backward.txt): the family starts at one element
_TORCH_GELU, _TORCH_SILU = torch.nn.functional.gelu, torch.nn.functional.silu   # what anything outside the family IS
_TORCH_SOFTPLUS, _TORCH_GLU = torch.nn.functional.softplus, torch.nn.functional.glu
_TORCH_TANH, _TORCH_SIGMOID = torch.tanh, torch.sigmoid


def declared_activation_calls() -> dict:
    return dict(_ACT_CALLS)


def _act_forward_fn(kind, x, beta, threshold):
    if kind == "gelu":
        return _TORCH_GELU(x)
    if kind == "gelu_tanh":
        return _TORCH_GELU(x, approximate="tanh")
    if kind == "silu":
        return _TORCH_SILU(x)
    if kind == "tanh":
        return _TORCH_TANH(x)
    if kind == "sigmoid":
        return _TORCH_SIGMOID(x)
    return _TORCH_SOFTPLUS(x, beta=beta, threshold=threshold)


def _act_backward_fn(kind, gy, x, y, beta, threshold):
    """ATen's single backward kernel of the kind: what the torch function's ordinary backward runs (y: the output, for tanh / sigmoid)."""
    aten = torch.ops.aten
    if kind == "gelu":
        return aten.gelu_backward(gy, x, approximate="none")
    if kind == "gelu_tanh":
        return aten.gelu_backward(gy, x, approximate="tanh")
    if kind == "silu":
        return aten.silu_backward(gy, x)
    if kind == "tanh":
        return aten.tanh_backward(gy, y)
    if kind == "sigmoid":
        return aten.sigmoid_backward(gy, y)
    return aten.softplus_backward(gy, x, beta, threshold)


def _act_vjp_hip(form, kind, ins, need, beta=1.0, threshold=20.0):
    """The double backward's one call.  form "plain": ins = (x, gy, a) -> (dx, dgy) through bhg_act_backward_vjp; "glu": the same
    tensors of F.glu(x, -1), taken as the halves of the gated form (v first, u second) and written into the halves of one dx; "gated":
    ins = (u, v, gy, au, av) -> (du, dv, dgy) through bhg_gated_act_backward_vjp.  ``need`` says which outputs are wanted (the others are
    None).  The product's only implementation: it raises when the HIP extension is missing or the tensors are not on the GPU."""
    if not ins[0].is_cuda:
        raise _native.NativeLibraryError("a declared activation's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()

    ins = [prep(t) for t in ins]
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    k = _ACT_KINDS["sigmoid" if form == "glu" else kind]
    with torch.cuda.device(ins[0].device):
        if form == "plain":
            x, gy, a = ins
            dx, dgy = (torch.empty_like(x) if on else None for on in need)
            _native.check(lib.bhg_act_backward_vjp(k, float(beta), float(threshold), x.data_ptr(), gy.data_ptr(), a.data_ptr(), ptr(dx), ptr(dgy),
                                                   x.numel(), _stream()), "bhg_act_backward_vjp")
            return dx, dgy
        if form == "glu":
            x, gy, a = ins
            H = x.shape[-1] // 2
            rows = x.numel() // (2 * H)
            dx, dgy = (torch.empty_like(t) if on else None for on, t in zip(need, (x, gy)))
            off = lambda t: None if t is None else t.data_ptr() + 4 * H   # noqa: E731  (the second half of a row: u, au, du)
            _native.check(lib.bhg_gated_act_backward_vjp(k, rows, H, off(x), 2 * H, x.data_ptr(), 2 * H, gy.data_ptr(), H, off(a), 2 * H,
                                                         a.data_ptr(), 2 * H, off(dx), 2 * H, ptr(dx), 2 * H, ptr(dgy), H, _stream()),
                          "bhg_gated_act_backward_vjp")
            return dx, dgy
        u, v, gy, au, av = ins
        H = u.shape[-1] if u.dim() else 1
        rows = u.numel() // H
        du, dv, dgy = (torch.empty_like(u) if on else None for on in need)
        _native.check(lib.bhg_gated_act_backward_vjp(k, rows, H, u.data_ptr(), H, v.data_ptr(), H, gy.data_ptr(), H, ptr(au), H, ptr(av), H,
                                                     ptr(du), H, ptr(dv), H, ptr(dgy), H, _stream()), "bhg_gated_act_backward_vjp")
        return du, dv, dgy


_ACT_VJP_IMPL = [_act_vjp_hip]   # TEST HOOK ONLY (tests/test_declared_activations.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _ActBackward(torch.autograd.Function):
    """(x, gy) -> gx = gy f'(x): an activation's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, x, gy, y, kind, beta, threshold):
        _ACT_CALLS["backward"] += 1
        gy = gy.contiguous()
        if kind == "glu":
            gx = torch.ops.aten.glu_backward(gy, x, x.dim() - 1)
        else:
            gx = _act_backward_fn(kind, gy, x, y, beta, threshold)   # the backward the torch function itself runs: the same kernel
        ctx.save_for_backward(x, gy)
        ctx.kind, ctx.beta, ctx.threshold = kind, beta, threshold
        ctx.set_materialize_grads(False)
        return gx

    @staticmethod
    @once_differentiable
    def backward(ctx, a):
        need = tuple(ctx.needs_input_grad[:2])
        if a is None or not any(need):
            return (None,) * 6
        x, gy = ctx.saved_tensors
        _ACT_CALLS["backward_vjp"] += 1
        dx, dgy = _ACT_VJP_IMPL[0]("glu" if ctx.kind == "glu" else "plain", ctx.kind, (x, gy, a), need, ctx.beta, ctx.threshold)
        return dx, dgy, None, None, None, None


class _ActForward(torch.autograd.Function):
    """An activation on the torch function's own kernel; its backward is the node above (so create_graph=True records THAT node)."""

    @staticmethod
    def forward(ctx, x, kind, beta, threshold):
        _ACT_CALLS["forward"] += 1
        y = _TORCH_GLU(x, -1) if kind == "glu" else _act_forward_fn(kind, x, beta, threshold)
        ctx.save_for_backward(x, y if kind in ("tanh", "sigmoid") else None)
        ctx.kind, ctx.beta, ctx.threshold = kind, beta, threshold
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        return _ActBackward.apply(x, gy, None if y is None else y.detach(), ctx.kind, ctx.beta, ctx.threshold), None, None, None


class _GatedActBackward(torch.autograd.Function):
    """(u, v, gy) -> (gu, gv) = (gy f'(u) v, gy f(u)): the gated form's backward as a graph node whose own backward is ONE fused call."""

    @staticmethod
    def forward(ctx, u, v, gy, fu, kind):
        _ACT_CALLS["backward"] += 1
        gy = gy.contiguous()
        gu = _act_backward_fn(kind, gy * v, u, fu, 1.0, 20.0)   # what autograd runs for act(u) * v: mul's backward, then the kind's
        gv = gy * fu
        ctx.save_for_backward(u, v, gy)
        ctx.kind = kind
        ctx.set_materialize_grads(False)
        return gu, gv

    @staticmethod
    @once_differentiable
    def backward(ctx, au, av):
        need = tuple(ctx.needs_input_grad[:3])
        if (au is None and av is None) or not any(need):
            return (None,) * 5
        u, v, gy = ctx.saved_tensors
        _ACT_CALLS["backward_vjp"] += 1
        du, dv, dgy = _ACT_VJP_IMPL[0]("gated", ctx.kind, (u, v, gy, au, av), need)
        return du, dv, dgy, None, None


class _GatedActForward(torch.autograd.Function):
    """act(gate) * up on the torch functions' own kernels; its backward is the node above."""

    @staticmethod
    def forward(ctx, u, v, kind):
        _ACT_CALLS["forward"] += 1
        fu = _act_forward_fn(kind, u, 1.0, 20.0)
        ctx.save_for_backward(u, v, fu)
        ctx.kind = kind
        return fu * v

    @staticmethod
    def backward(ctx, gy):
        u, v, fu = ctx.saved_tensors
        gu, gv = _GatedActBackward.apply(u, v, gy, fu, ctx.kind)
        return (gu if ctx.needs_input_grad[0] else None), (gv if ctx.needs_input_grad[1] else None), None


def _act_declared(x) -> bool:
    return (torch.is_grad_enabled() and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and x.numel() >= _ACT_MIN_NUMEL and not x.is_nested)


def gelu(input, approximate="none"):
    """``torch.nn.functional.gelu`` whose double backward is one fused launch (comment above), for CUDA fp32 contiguous inputs of at
    least one element with grad enabled.  Anything else IS the torch function with the caller's arguments, errors included.  Third
    derivatives are not provided."""
    if approximate not in ("none", "tanh") or not _act_declared(input):
        return _TORCH_GELU(input, approximate=approximate)
    return _ActForward.apply(input, "gelu" if approximate == "none" else "gelu_tanh", 1.0, 20.0)


def silu(input, inplace=False):
    """``torch.nn.functional.silu``, declared as :func:`gelu` is (``inplace=True`` keeps the torch path)."""
    if inplace or not _act_declared(input):
        return _TORCH_SILU(input, inplace=inplace)
    return _ActForward.apply(input, "silu", 1.0, 20.0)


def tanh(input):
    """``torch.tanh``, declared as :func:`gelu` is."""
    if not _act_declared(input):
        return _TORCH_TANH(input)
    return _ActForward.apply(input, "tanh", 1.0, 20.0)


def sigmoid(input):
    """``torch.sigmoid``, declared as :func:`gelu` is."""
    if not _act_declared(input):
        return _TORCH_SIGMOID(input)
    return _ActForward.apply(input, "sigmoid", 1.0, 20.0)


def softplus(input, beta=1.0, threshold=20.0):
    """``torch.nn.functional.softplus``, declared as :func:`gelu` is, with ATen's linear branch where ``beta * x > threshold``."""
    if not (_act_declared(input) and isinstance(beta, (int, float)) and isinstance(threshold, (int, float)) and beta != 0):
        return _TORCH_SOFTPLUS(input, beta=beta, threshold=threshold)
    return _ActForward.apply(input, "softplus", float(beta), float(threshold))


def glu(input, dim=-1):
    """``torch.nn.functional.glu`` on the last dimension, of even size, declared as :func:`gelu` is: the gated form with the logistic
    function, the first half of a row the linear factor.  Any other ``dim`` keeps the torch path."""
    if not (_act_declared(input) and isinstance(dim, int) and input.dim() >= 1 and dim in (-1, input.dim() - 1) and input.shape[-1] % 2 == 0):
        return _TORCH_GLU(input, dim)
    return _ActForward.apply(input, "glu", 1.0, 20.0)


def gated_activation(gate, up, activation="silu"):
    """``act(gate) * up`` — SwiGLU with ``"silu"``, GeGLU with ``"gelu"`` / ``"gelu_tanh"``, also ``"tanh"`` and ``"sigmoid"`` — whose
    double backward is one fused launch, for two CUDA fp32 contiguous tensors of equal shape on one device with grad enabled.  Anything
    else is the same expression in torch operations."""
    if activation not in _ACT_GATED:
        raise ValueError(f"gated_activation: activation must be one of {_ACT_GATED}, got {activation!r}")
    if not (_act_declared(gate) and _act_declared(up) and gate.shape == up.shape and gate.device == up.device):
        return _act_forward_fn(activation, gate, 1.0, 20.0) * up
    return _GatedActForward.apply(gate, up, activation)


class DeclaredGELU(torch.nn.GELU):
    def forward(self, input):
        return gelu(input, approximate=self.approximate)


class DeclaredSiLU(torch.nn.SiLU):
    def forward(self, input):
        return silu(input, inplace=self.inplace)


class DeclaredTanh(torch.nn.Tanh):
    def forward(self, input):
        return tanh(input)


class DeclaredSigmoid(torch.nn.Sigmoid):
    def forward(self, input):
        return sigmoid(input)


class DeclaredSoftplus(torch.nn.Softplus):
    def forward(self, input):
        return softplus(input, self.beta, self.threshold)


class DeclaredGLU(torch.nn.GLU):
    def forward(self, input):
        return glu(input, self.dim)


_ACT_MODULES = {torch.nn.GELU: DeclaredGELU, torch.nn.SiLU: DeclaredSiLU, torch.nn.Tanh: DeclaredTanh, torch.nn.Sigmoid: DeclaredSigmoid,
                torch.nn.Softplus: DeclaredSoftplus, torch.nn.GLU: DeclaredGLU}


def declare_activations_(module: torch.nn.Module) -> int:
    """Declare every ``nn.GELU``, ``nn.SiLU``, ``nn.Tanh``, ``nn.Sigmoid``, ``nn.Softplus`` and ``nn.GLU`` of ``module`` (exact classes;
    subclasses are left alone) in place: only the class changes.  ``nn.SiLU(inplace=True)`` and an ``nn.GLU`` on a dimension other than
    -1 are left as they are.  ``nn.TransformerEncoderLayer`` / ``nn.TransformerDecoderLayer`` capture their activation function at
    construction: where that attribute IS torch's ``F.gelu`` it is replaced by :func:`gelu`.  Returns how many were declared."""
    n = 0
    for m in module.modules():
        cls = _ACT_MODULES.get(type(m))
        if cls is not None:
            if (cls is DeclaredSiLU and m.inplace) or (cls is DeclaredGLU and m.dim != -1):
                continue
            m.__class__ = cls
            n += 1
        elif type(m) in (torch.nn.TransformerEncoderLayer, torch.nn.TransformerDecoderLayer) and m.activation is _TORCH_GELU:
            m.activation = gelu
            n += 1
    return n


@contextlib.contextmanager
def declared_activations():
    """Inside the context ``torch.nn.functional.gelu`` / ``silu`` / ``softplus`` / ``glu`` are the functions above: ``nn.GELU``,
    ``nn.SiLU``, ``nn.Softplus``, ``nn.GLU`` and model code that calls the torch functions reach the declaration without being rewritten
    (``torch.tanh`` / ``torch.sigmoid`` and the Tensor methods are not patched: ``nn.Tanh`` / ``nn.Sigmoid`` are reached by
    ``declare_activations_``, other code by calling :func:`tanh` / :func:`sigmoid`).  Only the forward that records the graph has to run
    inside.  Restored on exit, exceptions included; nesting is safe."""
    F = torch.nn.functional
    previous = (F.gelu, F.silu, F.softplus, F.glu)
    F.gelu, F.silu, F.softplus, F.glu = gelu, silu, softplus, glu
    try:
        yield
    finally:
        F.gelu, F.silu, F.softplus, F.glu = previous


# ---- declared cross-entropy: the loss every opaque inner problem ends in -------------------------------------------------------------------
# Under create_graph=True the first backward of F.cross_entropy is nll_loss_backward followed by _log_softmax_backward_data, and ATen
# differentiates those two by a chain of element-wise and reduction operators over the whole [N, C] logit matrix.  Declared, the forward
# (log_softmax, nll_loss_forward) and the first backward are ATen's own kernels, tied into the graph as two autograd.Function nodes as for
# the norms, and the backward OF the backward node is one bhg_cross_entropy_backward_vjp call (csrc/bhg_cross_entropy.hip): at most two
# launches.  What is saved is what torch saves — ATen's log_softmax output, the target and total_weight — and not the logits: the forward
# node hands its log_softmax out as a second output that nothing but the backward node sees, and that output stands in for the logits
# in the graph (its cotangent IS the logits': _CEForward.backward passes it through unchanged).
_CE_CALLS = {"forward": 0, "backward": 0, "backward_vjp": 0}   # test / measurement hook: which nodes ran
_CE_MAX_C = 262144                                              # the family bhg_cross_entropy_backward_vjp takes
_TORCH_CROSS_ENTROPY = torch.nn.functional.cross_entropy        # what anything outside the family IS
_CE_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}               # at::Reduction


def declared_cross_entropy_calls() -> dict:
    return dict(_CE_CALLS)


_CE_WS = {}   # (device, stream) -> scratch for the per-slice sums of split rows and the per-workgroup sums of a scalar dg


def _ce_workspace(device, n):
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    ws = _CE_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _CE_WS[key] = torch.empty(max(n, 1 << 16), dtype=torch.uint8, device=device)
    return ws


def _ce_vjp_hip(lsm, y, g, a, denom, ignore_index, want):
    """(dz, dg) through bhg_cross_entropy_backward_vjp, each None where ``want`` says so; g is [N] or 0-dim (then dg is 0-dim and denom,
    one device float or None, divides g going in and dg going out).  The product's only implementation: it raises when the HIP extension
    is missing or the tensors are not on the GPU."""
    if not lsm.is_cuda:
        raise _native.NativeLibraryError("the declared cross-entropy's double backward needs CUDA/HIP tensors; there is no CPU fallback")
    lib = _native.load()
    N, C = lsm.shape
    scalar = g.dim() == 0

    def prep(t):
        t = t.detach()
        return t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) else t.to(torch.float32).contiguous().clone()

    lsm, g, a = (prep(t) for t in (lsm, g, a))
    y = y.detach().contiguous()
    denom = None if denom is None else prep(denom)
    dz = torch.empty_like(lsm) if want[0] else None
    dg = torch.empty_like(g) if want[1] else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    with torch.cuda.device(lsm.device):
        n = int(lib.bhg_cross_entropy_ws_bytes(int(N), int(C), int(scalar)))
        ws = _ce_workspace(lsm.device, n) if n else None
        _native.check(
            lib.bhg_cross_entropy_backward_vjp(lsm.data_ptr(), y.data_ptr(), g.data_ptr(), int(scalar), ptr(denom), a.data_ptr(), int(N), int(C),
                                               int(ignore_index), ptr(dz), ptr(dg), ptr(ws), 0 if ws is None else ws.numel(), _stream()),
            "bhg_cross_entropy_backward_vjp")
    return dz, dg


_CE_VJP_IMPL = [_ce_vjp_hip]   # TEST HOOK ONLY (tests/test_declared_cross_entropy.py swaps in the float64 restatement to check the graph plumbing on CPU)


class _CEBackward(torch.autograd.Function):
    """(z, g) -> gz: cross-entropy's backward as a graph node whose own backward is ONE fused call.  ``z`` only links the graph (it is
    whatever stands for the logits there; it is neither read nor saved)."""

    @staticmethod
    def forward(ctx, z, g, lsm, y, total_weight, reduction, ignore_index):
        _CE_CALLS["backward"] += 1
        g = g.contiguous()
        lsm = lsm.detach()
        gl = torch.ops.aten.nll_loss_backward(g, lsm, y, None, _CE_REDUCTIONS[reduction], ignore_index, total_weight)
        gz = torch.ops.aten._log_softmax_backward_data(gl, lsm, 1, lsm.dtype)
        ctx.save_for_backward(lsm, y, g, total_weight)
        ctx.reduction, ctx.ignore_index = reduction, ignore_index
        ctx.set_materialize_grads(False)
        return gz

    @staticmethod
    @once_differentiable
    def backward(ctx, a):
        need = ctx.needs_input_grad
        if a is None or not (need[0] or need[1]):
            return (None,) * 7
        lsm, y, g, total_weight = ctx.saved_tensors
        _CE_CALLS["backward_vjp"] += 1
        denom = total_weight if ctx.reduction == "mean" else None
        dz, dg = _CE_VJP_IMPL[0](lsm, y, g, a, denom, ctx.ignore_index, (bool(need[0]), bool(need[1])))
        return (dz if need[0] else None), (dg if need[1] else None), None, None, None, None, None


class _CEForward(torch.autograd.Function):
    """Cross-entropy on ATen's own kernels; its backward is the node above (so create_graph=True records THAT node).  Returns
    (loss, link): link is the saved log_softmax, handed out only so that the backward can reach the logits' place in the graph without
    the logits being kept alive.  INTERNAL ONLY: link is a differentiable output whose derivative with respect to the logits is
    treated as the identity, not log_softmax's Jacobian — it must reach nothing but _CEBackward, and :func:`cross_entropy` discards it."""

    @staticmethod
    def forward(ctx, z, y, reduction, ignore_index):
        _CE_CALLS["forward"] += 1
        lsm = torch.log_softmax(z, 1)
        loss, total_weight = torch.ops.aten.nll_loss_forward(lsm, y, None, _CE_REDUCTIONS[reduction], ignore_index)
        ctx.save_for_backward(lsm, y, total_weight)
        ctx.reduction, ctx.ignore_index = reduction, ignore_index
        ctx.set_materialize_grads(False)
        return loss, lsm

    @staticmethod
    def backward(ctx, g, glink):
        lsm, y, total_weight = ctx.saved_tensors
        gz = None
        if g is not None:
            gz = _CEBackward.apply(lsm, g, lsm, y, total_weight, ctx.reduction, ctx.ignore_index)
        if glink is not None:   # the cotangent of the logits' stand-in: the double backward's dz
            gz = glink if gz is None else gz + glink
        return gz, None, None, None


def _ce_declared(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing) -> bool:
    """Whether a cross-entropy call lies in the declared family (:func:`cross_entropy`'s docstring)."""
    if not (torch.is_grad_enabled() and torch.is_tensor(input) and torch.is_tensor(target)):
        return False
    if not (weight is None and size_average is None and reduce is None and reduction in _CE_REDUCTIONS):
        return False
    if not (isinstance(label_smoothing, (int, float)) and label_smoothing == 0.0 and isinstance(ignore_index, int) and not isinstance(ignore_index, bool)):
        return False
    if not (input.is_cuda and input.dtype == torch.float32 and input.dim() == 2 and input.is_contiguous() and input.data_ptr() % 16 == 0
            and not input.is_nested):
        return False
    N, C = input.shape
    if not (N >= 1 and 1 <= C <= _CE_MAX_C):
        return False
    return target.dtype == torch.int64 and target.dim() == 1 and target.shape[0] == N and target.device == input.device


def cross_entropy(input, target, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
    """``torch.nn.functional.cross_entropy`` whose double backward is fused (comment above).  Loss and first gradient are ATen's own
    kernels' (bit-equal to the torch function's).  Declared only when grad mode is on, ``input`` is CUDA fp32, 2-D ``[N, C]``, contiguous
    and 16-byte aligned with ``N >= 1`` and ``1 <= C <= 262144``, ``target`` is int64 ``[N]`` on the same device (class indices),
    ``weight is None``, ``label_smoothing == 0.0``, ``size_average`` and ``reduce`` are ``None`` and ``reduction`` is ``"none"``,
    ``"mean"`` or ``"sum"``.  Anything else IS the torch function with the caller's arguments, errors included: probability targets,
    class weights, label smoothing, ``[N, C, d1, ...]`` and unbatched ``[C]`` inputs, half and bfloat16 inputs, CPU tensors, the
    deprecated ``size_average`` / ``reduce``, an unknown ``reduction``, grad mode off.  Third derivatives are not provided."""
    if not _ce_declared(input, target, weight, size_average, ignore_index, reduce, reduction, label_smoothing):
        return _TORCH_CROSS_ENTROPY(input, target, weight=weight, size_average=size_average, ignore_index=ignore_index, reduce=reduce,
                                    reduction=reduction, label_smoothing=label_smoothing)
    loss, _ = _CEForward.apply(input, target, reduction, ignore_index)
    return loss


class DeclaredCrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """``nn.CrossEntropyLoss`` whose double backward is fused: same arguments and buffers; a call outside :func:`cross_entropy`'s family
    (class weights, label smoothing, ...) IS ``nn.CrossEntropyLoss``."""

    def forward(self, input, target):
        return cross_entropy(input, target, weight=self.weight, ignore_index=self.ignore_index, reduction=self.reduction,
                             label_smoothing=self.label_smoothing)


def declare_cross_entropy_(module: torch.nn.Module) -> int:
    """Declare every ``nn.CrossEntropyLoss`` of ``module`` (exact class; subclasses are left alone) as :class:`DeclaredCrossEntropyLoss`,
    in place: only the class changes.  Returns how many were declared."""
    n = 0
    for m in module.modules():
        if type(m) is torch.nn.CrossEntropyLoss:
            m.__class__ = DeclaredCrossEntropyLoss
            n += 1
    return n


@contextlib.contextmanager
def declared_cross_entropy():
    """Inside the context ``torch.nn.functional.cross_entropy`` is :func:`cross_entropy`: ``nn.CrossEntropyLoss`` and model code that
    calls the torch function reach the declaration without being rewritten.  Only the forward that records the graph has to run inside.
    Restored on exit, exceptions included; nesting is safe."""
    F = torch.nn.functional
    previous = F.cross_entropy
    F.cross_entropy = cross_entropy
    try:
        yield
    finally:
        F.cross_entropy = previous

"""Shared pieces of cg / neumann / cg_global: inner-gradient graph, HVP sources, final mixed VJP, and InnerOperator, which picks
one source for a solve."""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import List, Sequence

import torch


def inner_gradient(curr):
    """``g = d L_in / d w`` with a graph (cg.py:27-32, neumann.py:31-36): re-evaluates the inner
    loss on the inner problem's last batch at the current inner weights."""
    in_loss = curr.training_step_exec(curr.cur_batch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        in_grad = torch.autograd.grad(in_loss, curr.trainable_parameters(), create_graph=True)
    return in_grad


class AutogradHVP:
    """Default Hessian-vector product: PyTorch-ROCm double backward through the user's opaque
    ``training_step`` (cg.py:39-41, neumann.py:62)."""

    def __init__(self, in_grad, params):
        self.in_grad = in_grad
        self.params = list(params)

    def __call__(self, direction_views: Sequence[torch.Tensor]):
        return torch.autograd.grad(self.in_grad, self.params, grad_outputs=direction_views, retain_graph=True)


# ---- forward-over-reverse Hessian-vector product (opt-in, round 5) ------------------------------------------------------------
# H v = d/d eps [ grad_w L(w + eps v) ]: forward-mode tangents (torch.autograd.forward_ad) carried through ONE evaluation of the
# loss and its ordinary backward — the same quantity as the double backward of cg.py:39-41 / neumann.py:62, to rounding.  Why it
# exists: ATen's `_convolution_double_backward` handles a GROUPED convolution by a Python-visible loop over the groups — 16 to 64
# tiny convolutions per depthwise layer and term — so the double backward of a DARTS supernet (BASELINE cfg 5: the reference's
# `Network(16, 10, 8)`, eight cells x 14 edges x 4 separable / dilated ops) is ~300 k launches enqueued by the host:
# 18.4 s per product on the MI355X box against 1.9 s for the whole forward-over-reverse pass, whose derivative formulas are
# whole-tensor convolutions (profiles/r05_cfg5_hvp_conv_modes.txt).  K + 1 passes per solve: K products and the mixed second
# derivative d/d eps grad_lambda L(w + eps (-alpha x)); no `in_grad` graph is built at all.
# OPT-IN: `inner_problem.hypergradient_hvp = "forward_over_reverse"`.  The problem promises that
#   * its trainable parameters are exactly parameters of `problem.module` (they are swapped for dual tensors by name);
#   * training_step is a deterministic function of (parameters, batch) given the RNG state: the state at the start of the solve is
#     restored before every pass, so dropout draws the same masks K + 1 times (the reference's ONE graph has one set of masks);
#   * module buffers (batch-norm running statistics) may be updated in place: the first pass updates the real ones — once, as the
#     reference's single training_step call does — the others work on clones.
# Operators without a forward-mode formula raise NotImplementedError on the first pass: the caller falls back to the double backward.
def forward_over_reverse_wanted(curr) -> bool:
    return getattr(curr, "hypergradient_hvp", None) == "forward_over_reverse"


class ForwardOverReverseHVP:
    def __init__(self, curr, prev):
        import torch.autograd.forward_ad as fwAD  # noqa: PLC0415
        from torch.nn.utils import stateless  # noqa: PLC0415

        self.fwAD, self._swap = fwAD, stateless._reparametrize_module
        self.curr, self.prev = curr, prev
        self.module = curr.module
        self.params = list(curr.trainable_parameters())
        by_id = {id(p): n for n, p in self.module.named_parameters()}
        missing = [i for i, p in enumerate(self.params) if id(p) not in by_id]
        if missing:
            raise ValueError("hypergradient_hvp = 'forward_over_reverse': trainable parameters must be parameters of problem.module")
        self.names = [by_id[id(p)] for p in self.params]
        dev = self.params[0].device
        self._cuda = dev.type == "cuda"
        self._rng_cpu = torch.get_rng_state()
        self._rng_dev = torch.cuda.get_rng_state(dev) if self._cuda else None
        self._dev = dev
        self.passes = 0
        self.fallback = self.in_grad = None
        # the first pass updates module buffers in place (batch-norm statistics): kept so that a FAILED first pass can be undone before
        # the double backward runs training_step again — buffers advance once per solve either way
        self._buffers0 = {n: b.detach().clone() for n, b in self.module.named_buffers()}
        self._warn_train_mode_batchnorm()

    def _warn_train_mode_batchnorm(self):
        """on the dense-convolution ResNet-12 of BASELINE cfg 3 (train-mode batch norm) this method measured 0.57x the double
        backward's speed and a solve 4.4e-3 away from it (profiles/r05_opaque_product_vs_reference_on_gpu.txt) — it pays only where the
        double backward is host-bound (grouped convolutions: cfg 5, x 9.9, 8.7e-5).  Said loudly, once per problem, where the module
        normalises with batch statistics; `problem.hypergradient_hvp_ack_batchnorm = True` acknowledges it."""
        bn = [n for n, m in self.module.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training]
        if not bn or getattr(self.curr, "hypergradient_hvp_ack_batchnorm", False) or getattr(self.curr, "_bhg_for_bn_warned", False):
            return
        grouped = any(isinstance(m, torch.nn.modules.conv._ConvNd) and m.groups > 1 for m in self.module.modules())
        warnings.warn(
            f"betty_amd: hypergradient_hvp = 'forward_over_reverse' on a module with {len(bn)} train-mode batch-norm layer(s) "
            f"(first: {bn[0]!r}){'' if grouped else ' and NO grouped convolution'}: forward-mode tangents through batch statistics measured "
            "4.4e-3 from the double backward's solve on a dense-convolution ResNet-12 at 0.57x its speed; the method pays where the "
            "double backward is host-bound (grouped / depthwise convolutions).  Compare both on your problem; set "
            "problem.hypergradient_hvp_ack_batchnorm = True to silence this.", RuntimeWarning, stacklevel=3)
        try:
            self.curr._bhg_for_bn_warned = True
        except AttributeError:
            pass

    @staticmethod
    def _is_missing_forward_formula(exc) -> bool:
        """Only a missing forward-mode derivative may trigger the fall-back — not an out-of-memory error or a shape bug in the user's
        training_step, which must surface as they are."""
        if isinstance(exc, NotImplementedError):
            return True
        if isinstance(exc, torch.cuda.OutOfMemoryError):
            return False
        msg = str(exc).lower()
        return any(k in msg for k in ("forward ad", "forward-mode", "forward mode", "jvp", "dual level", "dual tensor", "fwad"))

    def _pass(self, tangents, wrt_upper: bool):
        fwAD = self.fwAD
        if self.passes > 0:   # the same random draws as the first pass
            torch.set_rng_state(self._rng_cpu)
            if self._cuda:
                torch.cuda.set_rng_state(self._rng_dev, self._dev)
        swap = {}
        if self.passes > 0:   # running statistics were updated by the first pass: later passes must not move them again
            swap.update({n: b.detach().clone() for n, b in self.module.named_buffers()})
        self.passes += 1
        with fwAD.dual_level():
            duals = [fwAD.make_dual(p.detach().requires_grad_(True), t.detach().reshape(p.shape)) for p, t in zip(self.params, tangents)]
            swap.update(dict(zip(self.names, duals)))
            with self._swap(self.module, swap):
                loss = self.curr.training_step_exec(self.curr.cur_batch)
            wrt = list(self.prev.trainable_parameters()) if wrt_upper else duals
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                grads = torch.autograd.grad(loss, wrt, allow_unused=wrt_upper)
            out = []
            for g, w in zip(grads, wrt):
                t = None if g is None else fwAD.unpack_dual(g).tangent
                out.append(torch.zeros_like(w) if t is None else t.detach())
        return out

    def __call__(self, direction_views: Sequence[torch.Tensor]):
        if self.fallback is not None:
            return self.fallback(direction_views)
        try:
            return self._pass(direction_views, wrt_upper=False)
        except (NotImplementedError, RuntimeError) as exc:
            if self.passes > 1 or not self._is_missing_forward_formula(exc):
                raise
            # undo what the failed pass did to the module's buffers: inner_gradient() below runs training_step once more, and the
            # statistics must have advanced exactly once when the solve returns
            with torch.no_grad():
                for n, b in self.module.named_buffers():
                    if n in self._buffers0 and b.shape == self._buffers0[n].shape:
                        b.copy_(self._buffers0[n])
            # an operator of this training_step has no forward-mode formula: the reference's double backward takes over for the solve
            warnings.warn(f"betty_amd: forward-over-reverse HVP not available for this training_step ({type(exc).__name__}: {exc}); "
                          "using the double backward", RuntimeWarning)
            torch.set_rng_state(self._rng_cpu)
            if self._cuda:
                torch.cuda.set_rng_state(self._rng_dev, self._dev)
            self.in_grad = inner_gradient(self.curr)
            self.fallback = AutogradHVP(self.in_grad, self.params)
            return self.fallback(direction_views)

    def mixed(self, neg_x_views, sync: bool):
        """cg.py:58-68 / neumann.py:44-54: d(g . neg_x)/d lambda = tangent of grad_lambda L in direction neg_x on the inner weights."""
        if self.fallback is not None:
            return mixed_vjp(self.in_grad, self.prev, neg_x_views, sync)
        grads = self._pass(neg_x_views, wrt_upper=True)
        upper = list(self.prev.trainable_parameters())
        if sync:
            # accumulate THROUGH autograd (AccumulateGrad nodes), like the reference's backward(..., inputs=upper): hooks fire
            torch.autograd.backward(upper, grad_tensors=grads)
            return None
        return grads


# ---- finite-difference Hessian-vector product (opt-in): cg / neumann without any second-order autograd call -----------------
#     H p ~= ( grad_w L(w + eps p) - grad_w L(w - eps p) ) / (2 eps),        eps = R / (||p|| + 1e-15)
# Both other sources need every operator of training_step to be twice differentiable (or to have a forward-mode formula): a
# `once_differentiable` custom Function, a fused attention kernel, a checkpointed block or a vendor op without a double backward
# raises in the first product.  This source asks for what training itself asks for — one backward — and costs 2 K + 3 ordinary
# passes per solve: ONE forward at the unperturbed weights w0, which is the pass that moves the module's buffers (batch-norm running
# statistics are those of w0, as after the reference's single training_step) and advances the RNG stream; two forward / backward
# passes per iteration; two for the final hop.  No `in_grad` graph is built at all.
#   * the live weights are perturbed from a flat SNAPSHOT taken once per solve (bhg_fd_perturb: w <- w0 + (+-eps) p), never by
#     in-place +eps / -2 eps / +eps steps, and the solve ends with a scatter of the snapshot: the weights come back bit for bit;
#   * the recurrence kernels consume the two gradient lists directly (bhg_cg_step_fd / bhg_neumann_step_fd form (g+ - g-) / 2 eps in
#     registers): no N-sized H p is written;
#   * the final hop d/d eps grad_lambda L(w + eps u)|0 at u = -alpha x is the opaque branch of darts.finite_difference (sync
#     semantics unchanged: DDP hooks fire through `backward`).  darts returns the NEGATIVE of that derivative along its direction,
#     so the solvers leave +alpha x in the flat solution for this source (InnerOperator.out_sign).
# OPT-IN: `inner_problem.hypergradient_hvp = "finite_difference"`, radius R = `inner_problem.hypergradient_fd_radius` (default: the
# reference's darts_alpha default, 0.01).  What a user gives up is the truncation error of an fp32 central difference
# (profiles/fd_hvp_accuracy.txt).  The same promises as forward-over-reverse: trainable parameters are parameters of
# `problem.module`; the RNG state at the start of the solve is restored before every pass (dropout draws one set of masks); the first
# pass updates module buffers, the others run on clones.  Where it cannot apply (fd_hvp_blocker) the double backward runs, after one
# warning per problem, and nothing is touched.
FD_HVP_STATS = {"solves": 0, "pairs": 0, "fallbacks": 0}
FD_HVP_DEFAULT_RADIUS = 0.01
# cg / neumann calls on a declared LogisticRegressionL2 that offered the provider's own solver: `fused` ran the whole K loop in native
# launches (csrc/bhg_logreg_solve.hip), `loop` took K x (product + recurrence kernel) — K = 0, impl = "torch", d > 4096, ...
LOGREG_SOLVE_STATS = {"fused": 0, "loop": 0}
# the same for a declared SoftmaxRegressionL2 (csrc/bhg_softreg_solve.hip): `loop` — K = 0, impl = "torch", a shape outside the family
# (C > 16, d > 4096, C d > 32768), unaligned / non-contiguous / non-fp32 tensors, hypergradient_hvp = "finite_difference"
SOFTREG_SOLVE_STATS = {"fused": 0, "loop": 0}
# ... and for a declared WeightedSoftmaxRegression (the row-weighted kernels of the same file): `loop` under the same conditions
WSOFTREG_SOLVE_STATS = {"fused": 0, "loop": 0}


def finite_difference_wanted(curr) -> bool:
    return getattr(curr, "hypergradient_hvp", None) == "finite_difference"


def fd_hvp_blocker(curr):
    """None when FiniteDifferenceHVP can run on ``curr``, else the reason (a string) the double backward takes the solve."""
    if is_fsdp(curr):
        return "the problem is FSDP-sharded (a flat shard's gradient only materialises through backward into .grad)"
    if len(getattr(curr, "paths", None) or []) > 0:
        return "the problem has lower-level paths"
    if getattr(curr, "hypergradient_graph", False) == "persistent":
        return "hypergradient_graph = 'persistent' is set (the persistent graphs capture the double backward)"
    if torch.is_autocast_enabled() or precision_of(curr) in ("fp16", "bf16"):
        return "autocast is on (a half-precision difference of gradients has no digits left at this radius)"
    for p in curr.trainable_parameters():
        if p.dtype != torch.float32 or not p.is_contiguous() or (p.numel() > 0 and p.data_ptr() % 16 != 0):
            return "a trainable parameter is not a contiguous, 16-byte aligned fp32 tensor"
    return None


def finite_difference_usable(curr) -> bool:
    """finite_difference_wanted and not blocked; a blocked request warns once per problem and counts as a fallback."""
    if not finite_difference_wanted(curr):
        return False
    why = fd_hvp_blocker(curr)
    if why is None:
        return True
    FD_HVP_STATS["fallbacks"] += 1
    if not getattr(curr, "_bhg_fd_hvp_warned", False):
        warnings.warn(f"betty_amd: hypergradient_hvp = 'finite_difference' does not apply here: {why}; using the double backward",
                      RuntimeWarning, stacklevel=4)
        try:
            curr._bhg_fd_hvp_warned = True
        except AttributeError:
            pass
    return False


class GradientPair:
    """What FiniteDifferenceHVP hands the solvers instead of a product: grad L(w + eps p), grad L(w - eps p) and the 0-dim fp32
    device tensor 2 eps.  cg / neumann pass it to be.cg_step_fd / be.neumann_step_fd."""

    __slots__ = ("plus", "minus", "two_eps")

    def __init__(self, plus, minus, two_eps):
        self.plus, self.minus, self.two_eps = plus, minus, two_eps


class FiniteDifferenceHVP:
    def __init__(self, curr, prev, loss_fn=None):
        from torch.nn.utils import stateless  # noqa: PLC0415

        from ..backend import get_backend  # noqa: PLC0415

        self._swap = stateless._reparametrize_module
        self.curr, self.prev, self.module = curr, prev, curr.module
        # what is differentiated: the problem's training_step, or (ProximalRegularized) its data loss alone
        self.loss_fn = loss_fn if loss_fn is not None else (lambda: curr.training_step_exec(curr.cur_batch))
        self.params = list(curr.trainable_parameters())
        owned = {id(p) for p in self.module.parameters()}
        if any(id(p) not in owned for p in self.params):
            raise ValueError("hypergradient_hvp = 'finite_difference': trainable parameters must be parameters of problem.module")
        self.radius = float(getattr(curr, "hypergradient_fd_radius", FD_HVP_DEFAULT_RADIUS))
        self.be = get_backend()
        self.weights = [p.data for p in self.params]
        self.layout = self.be.layout(self.weights)
        w0 = getattr(self.layout, "_fd_hvp_snapshot", None)
        if w0 is None:
            w0 = self.layout._fd_hvp_snapshot = self.layout.new_flat()
        self.w0 = w0
        self.be.flatten(self.layout, self.weights, self.w0)   # once per solve
        dev = self.params[0].device
        self._dev, self._cuda = dev, dev.type == "cuda"
        self._rng_cpu = torch.get_rng_state()
        self._rng_dev = torch.cuda.get_rng_state(dev) if self._cuda else None
        self.passes, self.pairs, self.dirty = 0, 0, False
        FD_HVP_STATS["solves"] += 1
        # the ONE pass that moves the real buffers and the RNG stream, at w0: what the reference's single training_step does.  Its
        # value is not used; every later pass runs on buffer clones with the RNG state of the solve's start.
        self.loss()

    def loss(self):
        """One evaluation of the inner loss at the weights of the moment: the RNG stream of the solve's start, and — after the first
        pass (at w0, in __init__), which moves the real ones as the reference's single training_step does — clones of the module's
        buffers AS THEY WERE at the start of the solve, so every perturbed pass normalises with the statistics the first one saw."""
        swap = {}
        if self.passes > 0:
            torch.set_rng_state(self._rng_cpu)
            if self._cuda:
                torch.cuda.set_rng_state(self._rng_dev, self._dev)
            swap = {n: b.clone() for n, b in self._buffers0.items()}
        else:
            self._buffers0 = {n: b.detach().clone() for n, b in self.module.named_buffers()}
        self.passes += 1
        if not swap:
            return self.loss_fn()
        with self._swap(self.module, swap):
            return self.loss_fn()

    def _grad_at(self, direction_views, eps32, sign: float):
        self.be.fd_perturb(self.layout, self.weights, self.w0, direction_views, eps32, sign)
        self.dirty = True
        loss = self.loss()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            grads = torch.autograd.grad(loss, self.params, allow_unused=True)   # first order: no create_graph anywhere
        return [torch.zeros_like(p) if g is None else g for g, p in zip(grads, self.params)]

    def __call__(self, direction_views: Sequence[torch.Tensor]) -> GradientPair:
        eps32, eps64, _ = self.be.darts_eps(self.layout, direction_views, self.radius)
        two_eps = (2.0 * eps64).to(torch.float32)
        plus = self._grad_at(direction_views, eps32, 1.0)
        minus = self._grad_at(direction_views, eps32, -1.0)
        self.pairs += 1
        FD_HVP_STATS["pairs"] += 1
        return GradientPair(plus, minus, two_eps)

    def restore(self):
        """The inner weights back to the snapshot, bit for bit."""
        if self.dirty:
            self.be.scatter(self.layout, self.w0, self.weights)
            self.dirty = False

    def mixed(self, pos_views, sync: bool):
        """cg.py:58-68 / neumann.py:44-54 without the double backward: d/d eps grad_lambda L(w + eps u)|0 at u = -alpha x.  ``pos_views``
        holds +alpha x = -u: darts' central difference along d is (grad(w - eps d) - grad(w + eps d)) / 2 eps, which at d = -u is the
        derivative along u."""
        from .darts import finite_difference  # noqa: PLC0415

        self.restore()
        eps32, eps64, _ = self.be.darts_eps(self.layout, pos_views, self.radius)
        self.dirty = True   # the hop's in-place steps leave w0 + eps d - 2 eps d: put the snapshot back instead of a third rounding
        try:
            return finite_difference(self.curr, self.prev, self.layout, pos_views, eps32, eps64, sync, restore=False, opaque_loss=self.loss)
        finally:
            self.restore()


# ---- hipGraph replay of an opaque Hessian-vector product ----------------------------------------------------------------
# The double backward of a user's training_step is hundreds to thousands of small ATen launches (cfg 2's MLP: ~1.1 ms per
# HVP, launch-bound): the K HVPs of one solve run the SAME launch sequence on the SAME addresses — the autograd graph of
# `in_grad` is fixed for the step and the direction lives in one persistent flat vector — so the sequence is captured once
# (HIP graph) and replayed K - 2 times.
#   call 1: eager (settles library handles, workspaces, autotuning on the capture stream)
#   call 2: captured (hipStreamBeginCapture .. EndCapture around torch.autograd.grad), then replayed
#   call 3..K: replayed
# Autograd runs a backward node on the stream its forward ran on, so the graph of `in_grad` must be BUILT on the stream
# that later captures: `solve_stream` moves the whole solve to a library-owned side stream when the caller sits on the
# default (legacy) stream, which HIP cannot capture.  A capture that raises (a host sync inside the double backward, ...)
# leaves the wrapper eager for the rest of the solve.
# OPT-IN (measured on the MI355X, round 3): cfg 2 with the opaque HVP goes from 43.9 to 72.4 steps/s and seven solves of
# seven captures each replay cleanly, a ResNet-12 (GPU-bound double backward) gains nothing — and hipStreamEndCapture
# SEGFAULTS inside ROCm 7.2 on the tiny logistic-regression graph of the reference's regression scenario, which no
# try / except can contain.  So nothing is captured unless the user says so: `curr.hypergradient_graph = True` on the inner
# problem, or BHG_HVP_GRAPH=1 in the environment (=0 forces it off).
_SOLVE_STREAMS = {}
GRAPH_STATS = {"captures": 0, "replays": 0, "fallbacks": 0}


def hvp_graph_wanted(K: int, tensors, curr=None) -> bool:
    mode = os.environ.get("BHG_HVP_GRAPH", "")
    if mode == "0" or K < 3 or not tensors or not tensors[0].is_cuda:
        return False
    return mode == "1" or bool(getattr(curr, "hypergradient_graph", False))


@contextlib.contextmanager
def solve_stream(device, enabled: bool):
    """Run the body on a capturable stream (see above); joins the caller's stream on both sides."""
    if not enabled:
        yield None
        return
    cur = torch.cuda.current_stream(device)
    if cur != torch.cuda.default_stream(device):
        yield cur       # the caller already works on a stream of its own
        return
    side = _SOLVE_STREAMS.get(device.index)
    if side is None:
        side = _SOLVE_STREAMS[device.index] = torch.cuda.Stream(device)
    side.wait_stream(cur)
    try:
        with torch.cuda.stream(side):
            yield side
    finally:
        cur.wait_stream(side)


class GraphedHVP:
    """Wraps an eager HVP callable ``fn(direction_views) -> tuple of tensors`` (pure device work on fixed addresses)."""

    def __init__(self, fn):
        self.fn, self.calls, self.graph, self.out, self.key, self.dead = fn, 0, None, None, None, False

    @staticmethod
    def _key(views):
        return tuple((v.data_ptr(), tuple(v.shape), v.dtype) for v in views)

    def __call__(self, views):
        self.calls += 1
        if self.dead:
            return self.fn(views)
        key = self._key(views)
        if self.graph is not None:
            if key == self.key:
                self.graph.replay()
                GRAPH_STATS["replays"] += 1
                return self.out
            self.dead = True            # the caller moved the direction: the captured addresses are stale
            return self.fn(views)
        dev = views[0].device
        if self.calls == 1 or torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev):
            self.key = key
            return self.fn(views)
        if key != self.key:
            self.dead = True
            return self.fn(views)
        graph = torch.cuda.CUDAGraph()
        try:
            # a private memory pool per graph (released with the graph at the end of the solve): a pool handle shared
            # across solves is dropped by the caching allocator when the previous graph dies (round-3 measurement: the second
            # capture then trips an internal assert of HIPCachingAllocator)
            graph.capture_begin(capture_error_mode="thread_local")
            try:
                out = self.fn(views)
            finally:
                graph.capture_end()
            graph.replay()
        except Exception as exc:   # not capturable on this stack: eager for the rest of the solve
            self.dead = True
            GRAPH_STATS["fallbacks"] += 1
            warnings.warn(f"betty_amd: hipGraph capture of the Hessian-vector product failed ({type(exc).__name__}: {exc}); "
                          "continuing with eager launches", RuntimeWarning)
            torch.cuda.synchronize(dev)
            return self.fn(views)
        GRAPH_STATS["captures"] += 1
        GRAPH_STATS["replays"] += 1
        self.graph, self.out = graph, tuple(out)
        return self.out


class PersistentOpaqueGraphs:
    """Opt-in `inner_problem.hypergradient_graph = "persistent"`: the inner problem promises that its ``training_step`` is a
    STATIC function of (parameters, upper parameters, batch) — same shapes, no data-dependent Python control flow, no host
    side effects that matter.  Then not only the K HVPs of one solve but the steps of a whole run share two HIP graphs:

        G1   loss = training_step(batch*) ; in_grad = autograd.grad(loss, params, create_graph=True)   (batch* = static copies)
        G2   hvp  = autograd.grad(in_grad, params, grad_outputs=direction views, retain_graph=True)

    A step is then: copy the batch into batch*, replay G1 (the autograd graph OBJECT of `in_grad` is the one built at capture
    time; its saved tensors live at fixed addresses inside G1's pool and are refreshed by the replay), K x replay G2, and the
    usual EAGER mixed second derivative through that autograd graph (with retain_graph=True, so the graph survives the step;
    DistributedDataParallel hooks fire as always).  First step of a signature: eager (warm-up); second: capture; from the
    third on: replay.  Anything that changes the signature (parameter storage, batch shapes, direction buffer) recaptures.
    Not taken under DistributedDataParallel-wrapped upper modules reached inside the capture (their forward does host
    bookkeeping).  Measured (MI355X, cfg 2, opaque HVP, CG K = 20): see DESIGN.md section 5.

    STATIC-CLOSURE REQUIREMENT: the eager backward through the captured autograd graph is made to pass autograd's in-place check
    by setting the version counters of the TRACKED tensors (parameters, buffers, the static batch copies) back to their
    capture-time values (`saved_versions`, through the private `torch._C._autograd._unsafe_set_version_counter`).  Any other
    tensor `training_step` closes over and that is saved for backward is either caught by that check (an error) or, if it is
    rewritten in place between steps without autograd noticing, silently stale: a `training_step` that uses such tensors must
    not opt in.  `persistent_graphs_for` refuses (returns None) when the private API is absent."""

    def __init__(self):
        self.sig = None
        self.state = 0          # 0: nothing seen | 1: warmed up eagerly | 2: captured | -1: gave up
        self.g1 = self.g2 = None
        self.g3 = self.g3_key = self.g3_out = None   # the captured final hop (mixed); g3_dead: its capture failed once, eager for good
        self.g3_dead = False
        self.static_leaves = self.spec = None
        self.in_grad = self.out = None
        self.tracked, self.versions = [], []

    @contextlib.contextmanager
    def saved_versions(self):
        """The eager backward through the CAPTURED autograd graph checks that the tensors it saved (weights, upper weights,
        the static batch) still carry the version numbers of capture time — but optimizers and the batch refresh have written
        to them in place since (that is the point: same storage, new values, refreshed by the replay of G1).  Around that one
        backward the version counters are set to their capture-time values and restored afterwards, so every OTHER autograd
        graph that holds these tensors (the upper loss of the step, say) sees the numbers it expects."""
        if self.state != 2 or not self.tracked:
            yield
            return
        now = [t._version for t in self.tracked]
        torch._C._autograd._unsafe_set_version_counter(self.tracked, self.versions)
        try:
            yield
        finally:
            torch._C._autograd._unsafe_set_version_counter(self.tracked, now)

    @staticmethod
    def _signature(curr, params, batch_leaves, views):
        leaves = tuple((tuple(t.shape), t.dtype, str(t.device)) if torch.is_tensor(t) else ("leaf", repr(t)) for t in batch_leaves)
        return (tuple((id(p), p.data_ptr(), tuple(p.shape)) for p in params), leaves, GraphedHVP._key(views))

    def begin_step(self, curr, params, views, prev=None):
        """-> (in_grad, hvp_fn, persistent): `persistent` tells mixed_vjp to keep the autograd graph alive."""
        from torch.utils import _pytree as pytree

        leaves, spec = pytree.tree_flatten(curr.cur_batch)
        sig = self._signature(curr, params, leaves, views)
        dev = views[0].device
        on_default = torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)
        if self.state == -1 or on_default:
            in_grad = inner_gradient(curr)
            return in_grad, AutogradHVP(in_grad, params), False
        if sig != self.sig or self.state == 0:      # new signature: an eager step first (warm-up on the capture stream)
            self.sig, self.state = sig, 1
            self.g1 = self.g2 = self.in_grad = self.out = None
            self.g3 = self.g3_key = self.g3_out = None
            in_grad = inner_gradient(curr)
            return in_grad, AutogradHVP(in_grad, params), False
        if self.state == 1:                         # second step of this signature: capture G1 and G2
            try:
                self.static_leaves = [t.clone() if torch.is_tensor(t) else t for t in leaves]
                self.spec = spec
                static_batch = pytree.tree_unflatten(self.static_leaves, spec)
                g1 = torch.cuda.CUDAGraph()
                g1.capture_begin(capture_error_mode="thread_local")
                try:
                    loss = curr.training_step_exec(static_batch)
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        in_grad = torch.autograd.grad(loss, curr.trainable_parameters(), create_graph=True)
                finally:
                    g1.capture_end()
                g1.replay()
                g2 = torch.cuda.CUDAGraph()
                g2.capture_begin(capture_error_mode="thread_local")
                try:
                    out = torch.autograd.grad(in_grad, list(params), grad_outputs=views, retain_graph=True)
                finally:
                    g2.capture_end()
                self.g1, self.g2, self.in_grad, self.out, self.state = g1, g2, in_grad, tuple(out), 2
                tracked = list(params) + [t for t in self.static_leaves if torch.is_tensor(t)]
                if prev is not None:
                    mod = getattr(prev, "module", None)
                    tracked += list(prev.trainable_parameters()) + (list(mod.buffers()) if mod is not None else [])
                cmod = getattr(curr, "module", None)
                tracked += list(cmod.buffers()) if cmod is not None else []
                seen, uniq = set(), []
                for t in tracked:
                    if id(t) not in seen:
                        seen.add(id(t))
                        uniq.append(t)
                self.tracked, self.versions = uniq, [t._version for t in uniq]
                GRAPH_STATS["captures"] += 2
            except Exception as exc:
                self.state = -1
                GRAPH_STATS["fallbacks"] += 1
                warnings.warn(f"betty_amd: persistent hipGraph capture of the inner gradient / HVP failed ({type(exc).__name__}: {exc}); "
                              "continuing with eager launches", RuntimeWarning)
                torch.cuda.synchronize(dev)
                in_grad = inner_gradient(curr)
                return in_grad, AutogradHVP(in_grad, params), False
        else:                                       # replay: refresh the static batch, recompute loss / in_grad in place
            for st, t in zip(self.static_leaves, leaves):
                if torch.is_tensor(st):
                    st.copy_(t)
            self.g1.replay()
            GRAPH_STATS["replays"] += 1

        def hvp(direction_views):
            if GraphedHVP._key(direction_views) != self.sig[2]:
                raise RuntimeError("persistent HVP graph: the direction moved inside a solve")
            self.g2.replay()
            GRAPH_STATS["replays"] += 1
            return self.out

        return self.in_grad, hvp, True

    def mixed(self, prev, neg_x_views, sync: bool):
        """Final hop of a step whose `in_grad` lives in the persistent graph G1: the mixed second derivative (cg.py:58-68) as a THIRD
        captured graph, G3 = autograd.grad(in_grad, upper, grad_outputs=views) — captured on the first replayed step, replayed
        afterwards.  `sync=True` accumulates the replayed result into `.grad` (the upper modules are not DDP-wrapped here —
        persistent graphs are not taken under DDP — so there is no reducer hook a `backward` would have to fire)."""
        upper = list(prev.trainable_parameters())
        key = (tuple((id(p), p.data_ptr()) for p in upper), GraphedHVP._key(neg_x_views))
        if self.g3_dead:   # a capture of this hop failed once: stay eager for good (no retry, no warning per step)
            return mixed_vjp(self.in_grad, prev, neg_x_views, sync, retain_graph=True)
        if self.g3 is None or self.g3_key != key:
            with self.saved_versions():
                try:
                    g3 = torch.cuda.CUDAGraph()
                    g3.capture_begin(capture_error_mode="thread_local")
                    try:
                        outs = torch.autograd.grad(self.in_grad, upper, grad_outputs=neg_x_views, retain_graph=True)
                    finally:
                        g3.capture_end()
                    self.g3, self.g3_key, self.g3_out = g3, key, tuple(outs)
                    GRAPH_STATS["captures"] += 1
                except Exception as exc:   # stay eager for this hop
                    self.g3 = None
                    self.g3_dead = True
                    warnings.warn(f"betty_amd: hipGraph capture of the mixed second derivative failed ({type(exc).__name__}: {exc}); "
                                  "this hop stays eager for the rest of the run", RuntimeWarning)
                    torch.cuda.synchronize(neg_x_views[0].device)
                    return mixed_vjp(self.in_grad, prev, neg_x_views, sync, retain_graph=True)
        self.g3.replay()
        GRAPH_STATS["replays"] += 1
        grads = [g.clone() for g in self.g3_out]
        if sync:
            for p, g in zip(upper, grads):
                p.grad = g if p.grad is None else p.grad + g
            return None
        return grads


def _uses_ddp(problem) -> bool:
    from torch.nn.parallel import DistributedDataParallel as DDP

    return any(isinstance(getattr(problem, name, None), DDP) for name in ("fwd", "module"))


def precision_of(problem) -> str:
    """``problem.config.precision`` ("fp32" when the problem has no config or the config no precision)."""
    return str(getattr(getattr(problem, "config", None), "precision", "fp32"))


def is_fsdp(problem) -> bool:
    return getattr(problem, "_strategy", "default") == "fsdp"


def persistent_graphs_for(curr, K: int, tensors, prev=None):
    """The inner problem's PersistentOpaqueGraphs when it opted in with hypergradient_graph = "persistent", else None."""
    if os.environ.get("BHG_HVP_GRAPH", "") == "0" or K < 1 or not tensors or not tensors[0].is_cuda:
        return None
    if _uses_ddp(curr) or (prev is not None and _uses_ddp(prev)):   # a DDP forward does host bookkeeping: not capturable
        return None
    if getattr(curr, "hypergradient_graph", False) != "persistent":
        return None
    if not hasattr(getattr(torch._C, "_autograd", None), "_unsafe_set_version_counter"):   # the private API saved_versions() needs
        warnings.warn("betty_amd: this PyTorch has no torch._C._autograd._unsafe_set_version_counter — persistent HVP graphs are off",
                      RuntimeWarning)
        return None
    cache = getattr(curr, "_bhg_persistent_graphs", None)
    if cache is None:
        cache = curr._bhg_persistent_graphs = PersistentOpaqueGraphs()
    return cache


def mixed_vjp(in_grad, prev, neg_x_views: List[torch.Tensor], sync: bool, retain_graph: bool = False):
    """Final hop to the upper parameters (cg.py:58-68, neumann.py:44-54).

    ``neg_x_views`` already holds ``-(alpha * x)``; by linearity of the VJP
    ``-(d(g.x)/d lambda) == d(g.(-x))/d lambda`` bit for bit, so no extra negation pass is needed.
    ``sync=True`` accumulates into ``.grad`` through ``backward`` (DDP reducer hooks fire) and
    returns None; ``sync=False`` returns the list for ``Problem.set_grads``."""
    upper = prev.trainable_parameters()
    if sync:
        torch.autograd.backward(in_grad, inputs=upper, grad_tensors=neg_x_views, retain_graph=retain_graph)
        return None
    return list(torch.autograd.grad(in_grad, upper, grad_outputs=neg_x_views, retain_graph=retain_graph))


class InnerOperator:
    """The inner problem's Hessian for ONE solve of cg / neumann / cg_global: ``hvp(direction_views)`` builds the Hessian-vector
    product, ``mixed(neg_views, sync, solve)`` is the final hop to the upper parameters through the same source.  The source is, in
    this order: a structured provider; the persistent graphs (hypergradient_graph = "persistent"); forward-over-reverse passes
    (hypergradient_hvp = "forward_over_reverse"); central differences of first-order gradients (hypergradient_hvp =
    "finite_difference": ``hvp`` then returns GradientPair objects and the solvers leave ``out_sign * alpha * x`` = +alpha x for
    ``mixed``); a double backward through ``inner_gradient``.  A provider that offers ``first_order_loss`` (ProximalRegularized) keeps
    its shift and its closed-form hop and takes the finite-difference source for its data-loss product only.  An autograd-based product of one
    solve may be replayed as a HIP graph (GraphedHVP); ``graphs=False`` (cg_global) turns off every option but the provider and the
    plain double backward.  ``params``: what the autograd and persistent products differentiate.  Enter ``stream()`` around the whole
    solve: a captured product needs its autograd graph built on the capturing stream."""

    def __init__(self, curr, prev, K: int, vector, provider, params, graphs: bool = True):
        self.curr, self.prev, self.provider, self.params = curr, prev, provider, params
        self.graphed = graphs and (provider is None or getattr(provider, "hvp_is_autograd", False)) and hvp_graph_wanted(K, vector, curr)
        self.persist = persistent_graphs_for(curr, K, vector, prev) if graphs and provider is None else None
        self.for_hvp = graphs and provider is None and self.persist is None and forward_over_reverse_wanted(curr)
        self.fd_loss = getattr(provider, "first_order_loss", None)
        self.fd_hvp = bool(graphs and (provider is None or self.fd_loss is not None) and finite_difference_usable(curr))
        if self.fd_hvp:
            self.persist = None
            self.graphed = False   # nothing to capture: the product is two training_step calls
        # sign of the flat solution the solvers hand to mixed(): -alpha x, or +alpha x for the finite-difference hop (see above)
        self.out_sign = 1.0 if (self.fd_hvp and provider is None) else -1.0
        self.device = vector[0].device if vector else None
        # a structured provider may leave a diagonal part of the Hessian (ridge) to the recurrence kernel
        self.shift = float(getattr(provider, "hvp_shift", 0.0))
        self.in_grad, self.keep_graph, self.fwd, self.fd = None, False, None, None

    def stream(self):
        return solve_stream(self.device, self.graphed or self.persist is not None)

    def close(self):
        """End of the solve, reached on every path out of it: a finite-difference solve that raised half-way (training_step at
        w0 +- eps p ran out of memory, ...) must not leave the user's weights perturbed."""
        if self.fd is not None:
            self.fd.restore()

    def hvp(self, direction_views):
        if self.fd_hvp:   # no second-order call at all: H p from two first-order gradients
            self.fd = FiniteDifferenceHVP(self.curr, self.prev, None if self.provider is None else self.fd_loss())
            return self.fd
        if self.provider is not None:
            fn = self.provider.prepare()
        elif self.persist is not None:
            self.in_grad, fn, self.keep_graph = self.persist.begin_step(self.curr, list(self.params), direction_views, self.prev)
        elif self.for_hvp:   # no double-backward graph: H p by forward-over-reverse passes
            fn = self.fwd = ForwardOverReverseHVP(self.curr, self.prev)
        else:
            self.in_grad = inner_gradient(self.curr)
            fn = AutogradHVP(self.in_grad, self.params)
        if self.graphed and self.persist is None and not self.for_hvp:
            fn = GraphedHVP(fn)
        return fn

    def mixed(self, neg_views, sync: bool, solve=False):
        """``solve``: what a fused solver returned; a token (not True) tells the provider WHICH solve the views name (structured.py)."""
        if self.fd is not None:
            if self.provider is None:
                return self.fd.mixed(neg_views, sync)   # (holds +alpha x here: out_sign)
            self.fd.restore()
        if self.provider is not None:
            if solve and solve is not True:
                return self.provider.mixed_vjp(neg_views, sync, solve=solve)
            return self.provider.mixed_vjp(neg_views, sync)
        if self.for_hvp:   # the mixed second derivative is one more forward-over-reverse pass (or the fallback's double backward)
            return self.fwd.mixed(neg_views, sync)
        if self.keep_graph:   # the captured autograd graph of `in_grad` outlives the step (see PersistentOpaqueGraphs.saved_versions)
            return self.persist.mixed(self.prev, neg_views, sync)
        return mixed_vjp(self.in_grad, self.prev, neg_views, sync)

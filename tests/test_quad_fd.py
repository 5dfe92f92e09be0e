"""The closed-form finite-difference hop (darts, sama) of the two structures whose upper parameters enter the inner loss through a term
quadratic in the inner weights: ``ProximalRegularized.finite_difference`` (implicit MAML, 2 reg v) and
``LogisticRegressionL2.finite_difference`` (-(w v) into lam's graph), betty_amd/hypergradient/structured.py — on the ATen twin with the
checker backend (CPU) and on ``bhg_quad_fd`` (csrc/bhg_fd_quad.hip, GPU).

Same cases and goldens as the opaque path (tests/golden/<family>.npz from the reference's own darts.py / sama.py) at each case's rtol.
The weights after a call are compared bit for bit with the opaque path's / the backend's own three ``axpy_multi`` calls.  The kernel's
result is a single rounded product per element (plus one fp32 add when accumulating), so the direct sweep asserts equality with its
restatement.  The end-to-end accuracy bound needs no constant: against the reference's algorithm in fp64, the closed form may not be
further away than the opaque fp32 hop on the same inputs."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import zoo
from _cpu_checker_backend import CpuCheckerBackend
from conftest import golden_list, load_golden, rel_err

from betty_amd import Config, _native
from betty_amd import hypergradient as hg
from betty_amd.backend import use_backend
from betty_amd.flat import FlatLayout

QUAD_CASES = ["imaml_darts", "logreg_darts", "logreg_sama_sgd", "logreg_sama_multitask"]
R = 0.01   # Config.darts_alpha's default: eps = R / ||v||


@pytest.fixture()
def checker():
    with use_backend(CpuCheckerBackend()) as b:
        yield b


class _UnsyncedDDP(torch.nn.parallel.DistributedDataParallel):
    """Stands in for a DistributedDataParallel wrapper of the upper module (what the dispatch looks at: the type) without a process
    group: its forward is the module's."""

    def __init__(self, module):
        torch.nn.Module.__init__(self)
        self.module = module

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)


def _forbid_training_step(curr):
    """The closed form never calls the user's training_step: make any call to it fail loudly."""
    def boom(batch):
        raise AssertionError("the opaque path ran: training_step_exec was called")

    curr.training_step_exec = boom


def _count_training_steps(curr):
    ran, real = [], curr.training_step_exec

    def counted(batch):
        ran.append(1)
        return real(batch)

    curr.training_step_exec = counted
    return ran


def _declare(curr, family, impl, **kw):
    from betty_amd.hypergradient.structured import LogisticRegressionL2, ProximalRegularized

    if family == "imaml":
        def structure(prev):
            return ProximalRegularized(curr, prev, data_loss=lambda batch: F.cross_entropy(curr.module(batch[0]), batch[1]), reg=0.5,
                                       impl=impl, **kw)
    else:
        def structure(prev):
            return LogisticRegressionL2(curr, prev, curr.module.w, lam_fn=lambda: prev.fwd(), impl=impl, **kw)

    curr.hypergradient_structure = structure
    return curr


def _case(name, impl, device="cpu", **kw):
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config, device=device)
    if impl is not None:
        _declare(curr, case.family, impl, **kw)
    return case, outputs, curr, prev, vector


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _check_against_golden(case, curr, prev, vector, sync, outputs, fill=None):
    """sync=True: from ``.grad`` = None (the golden's own start) or, with ``fill``, from a pre-filled ``.grad`` whose rounding the
    difference then carries (the bound of tests/test_structured_fd.py, scaled by |fill|)."""
    if sync and fill is not None:
        for p in prev.trainable_parameters():
            p.grad = torch.full_like(p, fill)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, sync)
    if sync:
        assert out is None
        got = [g - (fill or 0.0) for g in _np([p.grad for p in prev.trainable_parameters()])]
        want = golden_list(outputs, case.name, "sync32")
        rel, _ = rel_err(got, want)
        scale = 1.0 if fill is None else max(1.0, fill / max(np.abs(np.concatenate([w.ravel() for w in want])).max(), 1e-30))
        print(f"{case.name} sync fill={fill}: rel err vs the reference's fp32 golden = {rel:.3e} (rtol {case.rtol:g} x {scale:.3g})")
        assert rel <= case.rtol * scale + (1e-6 * scale if fill is not None else 0.0), rel
    else:
        want = golden_list(outputs, case.name, "fp32")
        assert len(out) == len(want)
        rel, mx = rel_err(_np(out), want)
        rel64, _ = rel_err(_np(out), golden_list(outputs, case.name, "fp64"))
        ref64, _ = rel_err(want, golden_list(outputs, case.name, "fp64"))
        print(f"{case.name}: rel err vs the reference's fp32 golden = {rel:.3e} (max {mx:.3e}); vs its fp64 golden: closed form {rel64:.3e}, "
              f"the fp32 golden itself {ref64:.3e}")
        assert rel <= case.rtol and mx <= 10 * case.rtol, (rel, mx)
    # the weights the reference leaves behind: restored up to its own drift, or w- under *_multitask
    for p, w in zip(curr.trainable_parameters(), golden_list(outputs, case.name, "w32")):
        np.testing.assert_allclose(p.data.cpu().numpy(), w, rtol=0, atol=2e-7)


def _opaque_weights(name, device):
    """The inner weights the opaque path leaves behind on the same inputs (no structure declared)."""
    case, _, curr, prev, vector = _case(name, None, device=device)
    ran = _count_training_steps(curr)
    hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    assert len(ran) == 2
    return [p.data.clone() for p in curr.parameters()]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the ATen twin (impl="torch") with the checker backend
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("name", QUAD_CASES)
def test_aten_twin_matches_reference(name, sync, checker):
    case, outputs, curr, prev, vector = _case(name, "torch")
    _forbid_training_step(curr)
    _check_against_golden(case, curr, prev, vector, sync, outputs)


@pytest.mark.parametrize("name", QUAD_CASES)
def test_aten_twin_accumulates_into_a_prefilled_grad(name, checker):
    case, outputs, curr, prev, vector = _case(name, "torch")
    _forbid_training_step(curr)
    _check_against_golden(case, curr, prev, vector, True, outputs, fill=0.25)


@pytest.mark.parametrize("name", QUAD_CASES)
def test_aten_twin_takes_the_closed_form_not_the_training_step(name, checker):
    """Fails on a tree whose providers have no ``finite_difference``: the opaque path calls training_step_exec."""
    case, outputs, curr, prev, vector = _case(name, "torch")
    _forbid_training_step(curr)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    rel, _ = rel_err(_np(out), golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol, rel


@pytest.mark.parametrize("name", ["imaml_darts", "logreg_darts", "logreg_sama_multitask"])
def test_aten_twin_leaves_the_opaque_paths_weights(name, checker):
    """restore True (darts) and False (sama_multitask): bit for bit the weights of the three axpys."""
    want = _opaque_weights(name, "cpu")
    case, _, curr, prev, vector = _case(name, "torch")
    _forbid_training_step(curr)
    hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    for a, b in zip(curr.parameters(), want):
        assert torch.equal(a.data, b)


def test_proximal_sync_goes_through_autograd_under_ddp(checker):
    """A DistributedDataParallel wrapper on the upper module: the gradient reaches ``.grad`` by ``autograd.backward`` on the parameters,
    so their hooks (the reducer's) fire; without a wrapper and with ``.grad`` allocated the hop adds in place and no hook runs."""
    for wrapped in (True, False):
        case, outputs, curr, prev, vector = _case("imaml_darts", "torch")
        _forbid_training_step(curr)
        if wrapped:
            prev.fwd = _UnsyncedDDP(prev.module)
        fired = []
        for p in prev.trainable_parameters():
            p.grad = torch.full_like(p, 0.25)
            p.register_hook(lambda g, fired=fired: fired.append(1))
        held = [p.grad for p in prev.trainable_parameters()]
        assert hg.darts(vector, curr, prev, True) is None
        assert len(fired) == (len(held) if wrapped else 0)
        got = [g - 0.25 for g in _np([p.grad for p in prev.trainable_parameters()])]
        want = golden_list(outputs, case.name, "sync32")
        rel, _ = rel_err(got, want)
        scale = max(1.0, 0.25 / np.abs(np.concatenate([w.ravel() for w in want])).max())
        assert rel <= case.rtol * scale + 1e-6 * scale, rel


def _fallback_variants():
    def fsdp(curr, prev, vector):
        prev._strategy = "fsdp"

    def precision(curr, prev, vector):
        curr.config.precision = "bf16"

    def strided_direction(curr, prev, vector):
        vector[0] = torch.stack([vector[0], vector[0]], dim=-1)[..., 0]
        assert not vector[0].is_contiguous()

    def double_direction(curr, prev, vector):
        vector[0] = vector[0].double()

    def declined(curr, prev, vector):
        real = curr.hypergradient_structure
        curr.hypergradient_structure = lambda p: (lambda s: (setattr(s, "closed_form_fd", False), s)[-1])(real(p))

    return [fsdp, precision, strided_direction, double_direction, declined]


@pytest.mark.parametrize("name", ["imaml_darts", "logreg_darts"])
def test_fallback_conditions_reach_the_opaque_path(name, checker):
    """FSDP, a non-fp32 problem, a non-contiguous or non-fp32 direction and a declaration that declines keep the opaque path, unchanged:
    training_step runs twice and the result is the opaque one."""
    want = None
    for mutate in [lambda c, p, v: c.__dict__.pop("hypergradient_structure")] + _fallback_variants():
        case, outputs, curr, prev, vector = _case(name, "torch")
        mutate(curr, prev, vector)
        ran = _count_training_steps(curr)
        out = hg.darts(vector, curr, prev, False)
        assert len(ran) == 2, mutate.__name__
        if want is None:
            want = _np(out)   # the opaque path without any structure
        elif mutate.__name__ != "double_direction":
            for a, b in zip(_np(out), want):
                np.testing.assert_array_equal(a, b)


def test_autocast_keeps_the_opaque_path(checker):
    case, _, curr, prev, vector = _case("logreg_darts", "torch")
    ran = _count_training_steps(curr)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        hg.darts(vector, curr, prev, False)
    assert len(ran) == 2


def test_unaligned_upper_parameters_keep_the_opaque_path(checker):
    """Proximal: upper parameters that do not align one-to-one with the inner ones.  Logistic: an upper parameter lam does not depend on."""
    case, _, curr, prev, vector = _case("imaml_darts", "torch")
    prov = curr.hypergradient_structure(prev)   # declared while the parameters still align
    curr.hypergradient_structure = lambda p: prov
    params = list(prev.module.parameters())
    prev.trainable_parameters = lambda: params[:-1]
    ran = _count_training_steps(curr)
    out = hg.darts(vector, curr, prev, False)
    assert len(ran) == 2 and len(out) == len(params) - 1

    case, outputs, curr, prev, vector = _case("logreg_darts", "torch")
    extra = torch.nn.Parameter(torch.zeros(3))
    params = list(prev.module.parameters()) + [extra]
    prev.trainable_parameters = lambda: params
    ran = _count_training_steps(curr)
    out = hg.darts(vector, curr, prev, False)
    assert len(ran) == 2 and float(out[1].abs().max()) == 0.0
    rel, _ = rel_err(_np(out[:1]), golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol


class _BNNet(torch.nn.Module):
    def __init__(self, track, dropout=False):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(4, track_running_stats=track)
        self.drop = torch.nn.Dropout(0.5) if dropout else torch.nn.Identity()
        self.fc = torch.nn.Linear(4, 5)

    def forward(self, x):
        return self.fc(self.drop(torch.relu(self.bn(self.conv(x)))).mean((2, 3)))


def _bn_problem(track, dropout=False, device="cpu", impl="torch", **kw):
    from betty_amd.hypergradient.structured import ProximalRegularized

    g = torch.Generator().manual_seed(11)
    torch.manual_seed(5)
    inner = _BNNet(track, dropout).to(device)
    upper = copy.deepcopy(inner).to(device)
    for q in upper.parameters():
        q.data.add_(0.05 * torch.randn(q.shape, generator=g).to(device))
    batch = (torch.randn(10, 3, 8, 8, generator=g).to(device), torch.randint(0, 5, (10,), generator=g).to(device))
    prev = zoo.StubProblem("upper", upper, config=Config())
    curr = zoo.StubProblem("inner", inner, config=Config(type="darts", darts_alpha=0.05), loss_fn=zoo.make_imaml_loss(prev, 0.5), batch=batch)
    curr.hypergradient_structure = lambda p: ProximalRegularized(
        curr, p, data_loss=lambda b: F.cross_entropy(curr.module(b[0]), b[1]), reg=0.5, impl=impl, **kw)
    vector = [0.01 * torch.randn(p.shape, generator=g).to(device) for p in inner.parameters()]
    return curr, prev, vector


def test_forward_side_effects_decide_between_closed_form_and_opaque(checker):
    """The opaque hop runs the network twice: a training-mode BatchNorm2d that tracks running statistics moves them twice, a training-mode
    dropout layer consumes RNG.  Such a module keeps the opaque path unless the declaration says closed_form_fd=True, and then the
    buffers are not touched; eval mode, or statistics that are not tracked, take the closed form on their own."""
    def run(curr, prev, vector):
        ran = _count_training_steps(curr)
        out = hg.darts(vector, curr, prev, False)
        return len(ran), out

    curr, prev, vector = _bn_problem(track=True)
    mean0 = curr.module.bn.running_mean.clone()
    n, want = run(curr, prev, vector)
    assert n == 2 and int(curr.module.bn.num_batches_tracked) == 2 and not torch.equal(curr.module.bn.running_mean, mean0)

    curr, prev, vector = _bn_problem(track=True, closed_form_fd=True)
    n, got = run(curr, prev, vector)
    assert n == 0 and int(curr.module.bn.num_batches_tracked) == 0 and torch.equal(curr.module.bn.running_mean, mean0)
    rel, _ = rel_err(_np(got), _np(want))
    # the opaque fp32 hop divides a difference of two roundings of w +- eps v (each within u |w|, u = 2^-24) by 2 eps |v|: with |w| ~ 0.3
    # and eps |v| ~ 4e-3 here that is ~ 2e-6 per element; 1e-3 separates it from a wrong formula (a factor, a sign: >= 1)
    assert rel <= 1e-3, rel
    for v, o in zip(vector, got):
        assert torch.equal(o, v)   # 2 reg v with reg = 0.5

    curr, prev, vector = _bn_problem(track=True)
    curr.module.eval()
    assert run(curr, prev, vector)[0] == 0
    curr, prev, vector = _bn_problem(track=False)
    assert run(curr, prev, vector)[0] == 0
    curr, prev, vector = _bn_problem(track=False, dropout=True)
    assert run(curr, prev, vector)[0] == 2
    curr, prev, vector = _bn_problem(track=False, dropout=True)
    curr.module.drop.eval()
    assert run(curr, prev, vector)[0] == 0


def test_side_effect_rule_is_looked_up_once_per_provider(checker):
    from betty_amd.hypergradient import structured

    curr, prev, vector = _bn_problem(track=False)
    prov = curr.hypergradient_structure(prev)
    curr.hypergradient_structure = lambda p: prov
    looked, real = [], structured._forward_has_side_effects

    def spy(module):
        looked.append(1)
        return real(module)

    structured._forward_has_side_effects = spy
    try:
        _forbid_training_step(curr)
        hg.darts(vector, curr, prev, False)
        hg.darts(vector, curr, prev, False)
    finally:
        structured._forward_has_side_effects = real
    assert len(looked) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: argument validation of bhg_quad_fd (no launch, no device)
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib():
    try:
        return _native.load()
    except _native.NativeLibraryError as exc:
        pytest.skip(f"libbhg not built: {exc}")


def test_quad_fd_argument_validation_without_gpu():
    """Bad arguments are refused before any HIP call with a non-zero code and a message.  Every pointer below is a valid host address,
    so only the checks stand between these calls and a launch; the one good call has no chunks and launches nothing."""
    lib = _lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.addressof(host)
    tab_arr = (ctypes.c_void_p * 4)(p, p, p, p)
    tab = ctypes.cast(tab_arr, _native._PP)
    holed_arr = (ctypes.c_void_p * 4)(p, None, p, p)
    holed = ctypes.cast(holed_arr, _native._PP)
    odd_arr = (ctypes.c_void_p * 4)(p, p + 2, p, p)
    odd = ctypes.cast(odd_arr, _native._PP)

    def call(w=tab, d=tab, o=tab, T=4, chunks=p, n=1, eps=p, scale=1.0, mode=0, restore=1, acc=0):
        return lib.bhg_quad_fd(w, d, o, T, chunks, n, eps, scale, mode, restore, acc, None)

    assert call(n=0) == 0
    for kw, word in [(dict(w=None), b"NULL"), (dict(d=None), b"NULL"), (dict(o=None), b"NULL"), (dict(T=0), b"T must"), (dict(T=-3), b"T must"),
                     (dict(n=-1), b"negative"), (dict(chunks=None), b"chunk table"), (dict(eps=None), b"eps"), (dict(mode=2), b"mode"),
                     (dict(mode=-1), b"mode"), (dict(scale=float("nan")), b"finite"), (dict(scale=float("inf")), b"finite"),
                     (dict(scale=float("-inf")), b"finite"), (dict(w=holed), b"NULL"), (dict(d=holed), b"NULL"), (dict(o=holed), b"NULL"),
                     (dict(d=odd), b"aligned")]:
        assert call(**kw) != 0, kw
        assert word in lib.bhg_last_error(), (kw, lib.bhg_last_error())
    assert call(n=0, mode=1, scale=0.0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the providers over bhg_quad_fd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("name", QUAD_CASES)
def test_hip_matches_reference(name, sync):
    case, outputs, curr, prev, vector = _case(name, "hip", device="cuda")
    _forbid_training_step(curr)
    _check_against_golden(case, curr, prev, vector, sync, outputs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUAD_CASES)
def test_hip_accumulates_into_a_prefilled_grad(name):
    case, outputs, curr, prev, vector = _case(name, "hip", device="cuda")
    _forbid_training_step(curr)
    _check_against_golden(case, curr, prev, vector, True, outputs, fill=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUAD_CASES)
def test_hip_takes_the_closed_form_not_the_training_step(name):
    """The default declaration (no impl named) through darts / sama while training_step raises."""
    case, outputs, curr, prev, vector = _case(name, None, device="cuda")
    (zoo.attach_prox_structure if case.family == "imaml" else zoo.attach_logreg_structure)(curr)
    _forbid_training_step(curr)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    rel, _ = rel_err(_np(out), golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol, rel


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["imaml_darts", "logreg_darts", "logreg_sama_multitask"])
def test_hip_leaves_the_opaque_paths_weights(name):
    want = _opaque_weights(name, "cuda")
    case, _, curr, prev, vector = _case(name, "hip", device="cuda")
    _forbid_training_step(curr)
    hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    for a, b in zip(curr.parameters(), want):
        assert torch.equal(a.data, b)


@pytest.mark.gpu
def test_hip_twin_and_kernel_agree_exactly():
    """Same formulas, same roundings: the ATen twin on the HIP backend's axpys and the kernel give the same bits."""
    for name in QUAD_CASES:
        res = []
        for impl in ("torch", "hip"):
            case, _, curr, prev, vector = _case(name, impl, device="cuda")
            _forbid_training_step(curr)
            out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
            res.append(([o.clone() for o in out], [p.data.clone() for p in curr.parameters()]))
        for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
            assert torch.equal(a, b), name


@pytest.mark.gpu
def test_hip_fallbacks_reach_the_opaque_path():
    for name in ("imaml_darts", "logreg_darts"):
        for mutate in _fallback_variants():
            case, _, curr, prev, vector = _case(name, "hip", device="cuda")
            mutate(curr, prev, vector)
            ran = _count_training_steps(curr)
            hg.darts(vector, curr, prev, False)
            assert len(ran) == 2, (name, mutate.__name__)
    curr, prev, vector = _bn_problem(track=True, device="cuda", impl="hip")
    ran = _count_training_steps(curr)
    hg.darts(vector, curr, prev, False)
    assert len(ran) == 2 and int(curr.module.bn.num_batches_tracked) == 2
    curr, prev, vector = _bn_problem(track=True, device="cuda", impl="hip", closed_form_fd=True)
    _forbid_training_step(curr)
    out = hg.darts(vector, curr, prev, False)
    assert int(curr.module.bn.num_batches_tracked) == 0
    for v, o in zip(vector, out):
        assert torch.equal(o, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: bhg_quad_fd through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 8           # sentinel elements on either side of every tensor of the sweep
SENTINEL = -7.5


def _guarded(values, shift):
    """``values`` stored ``shift`` elements (4 * shift bytes) past a 16-byte boundary, sentinels all round.  Returns (buffer, view)."""
    n = values.numel()
    buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + shift
    buf[lo:lo + n] = values
    view = buf[lo:lo + n]
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return buf, view


def _guards_intact(buf, shift, n):
    lo = GUARD + shift
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all())


def _sweep_shapes():
    rng = np.random.RandomState(3)
    many = [int(x) for x in rng.choice([1, 2, 3, 5, 7, 63, 64, 65, 1023, 4095, 4096, 4097, 8191, 12289, 20001], size=48)]
    return {
        "one": [[1], [3], [5], [4095], [4097], [3 * 4096 + 2]],
        "two": [[4097, 3], [6, 8193]],
        "48 tensors": [many],
        "130 tensors (two launches)": [[int(x) for x in rng.choice([1, 7, 64, 4097, 5001], size=130)]],
    }


def _run_quad_fd(sizes, mode, restore, accumulate, shifts, seed=0):
    """One bhg_quad_fd call on tensors of ``sizes`` stored ``shifts`` = (w, v, out) elements past a 16-byte boundary; asserts the weights
    bit for bit against three bhg_axpy_multi calls on an aligned copy, the result against its restatement and the guards."""
    from betty_amd.backend import get_backend

    be, lib = get_backend(), _native.load()
    g = torch.Generator().manual_seed(100 + seed)
    dev = torch.device("cuda")
    lay = FlatLayout(sizes, dev)
    w0 = [torch.randn(n, generator=g).to(dev) for n in sizes]
    v = [(0.01 * torch.randn(n, generator=g)).to(dev) for n in sizes]
    o0 = [torch.randn(n, generator=g).to(dev) for n in sizes]
    scale = 0.6   # 2 reg with reg = 0.3: a product that rounds
    eps32, _, _ = be.darts_eps(lay, v, R)
    eps32 = eps32.reshape(1).clone()
    # what the opaque path does to the weights: the backend's own three axpys on an aligned copy
    want_w = [t.clone() for t in w0]
    be.axpy_multi(lay, want_w, v, eps32, 1.0)
    be.axpy_multi(lay, want_w, v, eps32, -2.0)
    if restore:
        be.axpy_multi(lay, want_w, v, eps32, 1.0)
    # fp64 restatement of the result: the product of two fp32 numbers is exact in fp64, so its rounding to fp32 is THE fp32 product
    s32 = float(np.float32(scale))
    if mode == 0:
        want_o = [(t.double() * s32).float() for t in v]
    else:
        want_o = [(-(a.double() * b.double())).float() for a, b in zip(w0, v)]
    if accumulate:
        want_o = [a + b for a, b in zip(o0, want_o)]   # one more fp32 add
    bw, bv, bo = ([_guarded(t, s) for t in ts] for ts, s in zip((w0, v, o0), shifts))
    tabs = [_native.ptr_array([view.data_ptr() for _, view in b]) for b in (bw, bv, bo)]
    _native.check(lib.bhg_quad_fd(tabs[0][0], tabs[1][0], tabs[2][0], len(sizes), lay.chunks_dev.data_ptr(), lay.n_chunks, eps32.data_ptr(),
                                  scale, mode, restore, accumulate, int(torch.cuda.current_stream().cuda_stream)), "bhg_quad_fd")
    torch.cuda.synchronize()
    tag = (sizes if len(sizes) <= 4 else f"{len(sizes)} tensors", mode, restore, accumulate, shifts)
    for i, n in enumerate(sizes):
        assert torch.equal(bw[i][1], want_w[i]), ("weights", i, tag)
        assert torch.equal(bo[i][1], want_o[i]), ("out", i, tag)
        assert torch.equal(bv[i][1], v[i]), ("direction written", i, tag)
        for b, s in zip((bw[i], bv[i], bo[i]), shifts):
            assert _guards_intact(b[0], s, n), ("out of bounds", i, tag)


SHIFTS = [(0, 0, 0), (1, 1, 1), (3, 3, 3), (1, 2, 0), (0, 0, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("restore", [0, 1])
@pytest.mark.parametrize("mode", [0, 1], ids=["proximal", "logistic"])
def test_kernel_sweep(mode, restore, accumulate):
    """Tensor counts 1, 2, 48 and 130, sizes that are not multiples of 4, chunks that start 4, 8 or 12 bytes past a 16-byte boundary
    (shared by the three tensors: vector body after a scalar head; different: scalar chunk)."""
    for group in _sweep_shapes().values():
        for sizes in group:
            for shifts in SHIFTS:
                _run_quad_fd(sizes, mode, restore, accumulate, shifts)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,restore,accumulate,shifts", [(0, 1, 0, (0, 0, 0)), (1, 1, 1, (0, 0, 0)), (1, 0, 0, (1, 1, 1)), (0, 0, 1, (2, 1, 0))])
def test_kernel_at_cfg3_size(mode, restore, accumulate, shifts):
    """N = 10,430,533 (BASELINE cfg 3's ResNet-12) in one tensor and split over three: more chunks than workgroups."""
    _run_quad_fd([10_430_533], mode, restore, accumulate, shifts)
    _run_quad_fd([7_000_001, 3_430_529, 3], mode, restore, accumulate, shifts, seed=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: accuracy of the end-to-end proximal hop at a few million inner parameters
# ---------------------------------------------------------------------------------------------------------------------------------
PROX_DIMS, PROX_BATCH, PROX_REG = [1024, 1536, 1024, 10], 64, 0.3


def build_prox_problem(device, dtype=torch.float32, declare=True, seed=0):
    """An implicit-MAML shaped problem built from a seed: inner MLP 1024-1536-1024-10 (3,157,002 parameters), the upper problem a
    perturbed copy, loss = CE + reg ||w - theta||^2 (zoo.make_imaml_loss), direction 0.01 N(0, 1).  Returns (curr, prev, vector)."""
    from betty_amd.hypergradient.structured import ProximalRegularized

    g = torch.Generator().manual_seed(4000 + seed)
    torch.manual_seed(4100 + seed)
    inner = zoo.MLP(PROX_DIMS)
    upper = copy.deepcopy(inner)
    for q in upper.parameters():
        q.data.add_(0.05 * torch.randn(q.shape, generator=g))
    vector = [(0.01 * torch.randn(p.shape, generator=g)).to(device=device, dtype=dtype) for p in inner.parameters()]
    batch = (torch.randn(PROX_BATCH, PROX_DIMS[0], generator=g).to(device=device, dtype=dtype),
             torch.randint(0, PROX_DIMS[-1], (PROX_BATCH,), generator=g).to(device))
    inner, upper = inner.to(device=device, dtype=dtype), upper.to(device=device, dtype=dtype)
    prev = zoo.StubProblem("upper", upper, config=Config())
    curr = zoo.StubProblem("inner", inner, config=Config(type="darts", darts_alpha=0.05), loss_fn=zoo.make_imaml_loss(prev, PROX_REG),
                           batch=batch)
    if declare:
        curr.hypergradient_structure = lambda p: ProximalRegularized(
            curr, p, data_loss=lambda b: F.cross_entropy(curr.module(b[0]), b[1]), reg=PROX_REG)
    return curr, prev, vector


@pytest.mark.gpu
def test_hip_proximal_scale_is_no_further_from_fp64_truth_than_the_opaque_path():
    """3.2 M inner parameters.  Truth: the reference's darts in fp64 (oracle/hypergrad_oracle.py).  The opaque fp32 hop on the same inputs
    is the yardstick: native error <= opaque error, no constant.  Weights bit-identical to the opaque path's."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import hypergrad_oracle as horc

    dev = torch.device("cuda")
    curr, prev, vector = build_prox_problem(dev, declare=False)
    ran = _count_training_steps(curr)
    want = [t.clone() for t in hg.darts(vector, curr, prev, False)]
    assert len(ran) == 2
    w_opaque = [p.data.clone() for p in curr.parameters()]
    curr, prev, vector = build_prox_problem(dev)
    _forbid_training_step(curr)
    got = [t.clone() for t in hg.darts(vector, curr, prev, False)]
    for a, b in zip(curr.parameters(), w_opaque):
        assert torch.equal(a.data, b)
    curr64, prev64, vector64 = build_prox_problem(dev, dtype=torch.float64, declare=False)
    truth = [t.detach().clone() for t in horc.darts(vector64, curr64, prev64, False)]
    np_ = lambda ts: [t.detach().double().cpu().numpy() for t in ts]
    e_opaque, _ = rel_err(np_(want), np_(truth))
    e_native, _ = rel_err(np_(got), np_(truth))
    print(f"proximal darts, N = {sum(v.numel() for v in vector)}: distance to the fp64 truth: opaque {e_opaque:.3e}, native {e_native:.3e}")
    assert e_native <= e_opaque, (e_native, e_opaque)

"""The native logistic-regression solvers (csrc/bhg_logreg_solve.hip: bhg_logreg_cg_solve / bhg_logreg_neumann_solve) through the C ABI,
against the fp64 restatement of the reference's iteration (tests/logreg_solve_ref.py), and through the front ends
(LogisticRegressionL2.fused_cg / fused_neumann) against the reference's goldens.

Inputs follow test_gpu_parity.py::test_logreg_hvp_kernels_vs_autograd: X ~ N(0, 1), w = 0.3 N(0, 1), lam in [0.5, 1.5), rhs ~ N(0, 1),
seed n + d.  Gate of the kernel tests: max|out - want| <= 2e-5 max|want| — the bound that test already holds these products to; the
reference's own fp32 arithmetic sits at <= 2.2e-7 from fp64 on every shape below, so the gate excludes no case.  `coeff` (= w * out)
has the same gate.  Every case also checks that the inputs are bit-equal afterwards and that `out`, `coeff` and the workspace —
slices of larger sentinel-filled buffers — were written inside their bounds only.
"""
import functools

import numpy as np
import pytest
import torch

import logreg_solve_ref as ref
import zoo
from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd.backend import LOGREG_FORM_AUTO, LOGREG_FORM_SINGLE, LOGREG_FORM_STRIPS, get_backend, logreg_solve_plan
from betty_amd.hypergradient._common import LOGREG_SOLVE_STATS
from betty_amd.hypergradient.structured import LogisticRegressionL2
from conftest import golden_list, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2e-5
# algorithm, step (cg_alpha | alpha): textbook CG, the cg_alpha quirk, Neumann
ALGOS = [("cg", 1.0), ("cg", 0.1), ("neumann", 0.5)]
ALGO_IDS = ["cg_a1", "cg_a01", "neumann_a05"]
SINGLE_SHAPES = [(1, 1, 1), (3, 2, 2), (37, 5, 3), (64, 64, 4), (500, 100, 5), (257, 129, 5), (260, 1000, 5), (255, 1024, 4)]
STRIPS_SHAPES = SINGLE_SHAPES + [(513, 1025, 6), (4096, 257, 8), (2048, 4096, 10)]
GIVEN_STRIPS = [(37, 5, 3, 1), (37, 5, 3, 7), (3, 2, 2, 8), (4096, 257, 8, 3)]
AUTO_SHAPES = [(500, 100, 5), (513, 1025, 6)]
PAD, SENTINEL, SENTINEL_BYTE = 64, 1234.5, 0xA5


@functools.lru_cache(maxsize=None)
def host_inputs(n, d):
    g = torch.Generator().manual_seed(n + d)
    X = torch.randn(n, d, generator=g)
    w = 0.3 * torch.randn(d, generator=g)
    torch.rand(n, generator=g)   # (the labels of the kernel test this follows: they do not enter the Hessian)
    lam = 0.5 + torch.rand(d, generator=g)
    rhs = torch.randn(d, generator=g)
    return X, w, lam, rhs


@functools.lru_cache(maxsize=None)
def device_inputs(n, d):
    return tuple(t.to(DEV) for t in host_inputs(n, d))


@functools.lru_cache(maxsize=None)
def wanted(n, d, K, algo, step):
    """(step * solution, its lam cotangent w * (-step * solution)) in fp64 — computed once per case, shared, read-only."""
    X, w, lam, rhs = (t.numpy() for t in host_inputs(n, d))
    sol = ref.SOLVERS[algo](X, w, lam, rhs, K, step)
    out, coeff = -sol, ref.lam_cotangent(w, sol)
    out.setflags(write=False)
    coeff.setflags(write=False)
    return out, coeff


def run_solve(n, d, K, algo, step, form, strips=0, dirty_ws=None, with_coeff=True):
    """One solve with out_scale = -step (what the front ends ask for).  Returns (out, coeff) as float32 host arrays after checking
    that the inputs are unchanged and nothing outside out / coeff / the workspace was written."""
    be = get_backend()
    ins = device_inputs(n, d)
    before = [t.clone() for t in ins]
    X, w, lam, rhs = ins
    ws_bytes = int(be.lib.bhg_logreg_solve_ws_bytes(n, d))
    assert ws_bytes > 0
    outbuf = torch.full((d + 2 * PAD,), SENTINEL, device=DEV)
    cobuf = torch.full((d + 2 * PAD,), SENTINEL, device=DEV)
    wsbuf = torch.full((ws_bytes + 2 * PAD,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    out, coeff, ws = outbuf[PAD:PAD + d], cobuf[PAD:PAD + d], wsbuf[PAD:PAD + ws_bytes]
    assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if dirty_ws is not None:
        ws.view(torch.float32)[: ws_bytes // 4].fill_(dirty_ws)
    fn = be.logreg_cg_solve if algo == "cg" else be.logreg_neumann_solve
    fn(X, w, lam, rhs, out, coeff if with_coeff else None, ws, K, step, -step, form, strips)
    torch.cuda.synchronize()
    for a, b in zip(ins, before):
        assert torch.equal(a, b), "an input was modified"
    for buf, val in ((outbuf, SENTINEL), (cobuf, SENTINEL)):
        assert bool((buf[:PAD] == val).all()) and bool((buf[PAD + d:] == val).all()), "write outside out / coeff"
    if not with_coeff:
        assert bool((cobuf == SENTINEL).all())
    assert bool((wsbuf[:PAD] == SENTINEL_BYTE).all()) and bool((wsbuf[PAD + ws_bytes:] == SENTINEL_BYTE).all()), "write outside the workspace"
    return out.cpu().numpy(), coeff.cpu().numpy()


def check(label, n, d, K, algo, step, got_out, got_coeff):
    want_out, want_coeff = wanted(n, d, K, algo, step)
    for name, got, want in (("out", got_out, want_out), ("coeff", got_coeff, want_coeff)):
        assert np.isfinite(got).all(), (label, name)
        err, scale = np.abs(got.astype(np.float64) - want).max(), np.abs(want).max()
        print(f"{label} n={n} d={d} K={K} {algo} step={step} {name}: max|got - want| = {err:.3e} = {err / scale if scale else 0.0:.3e} of max|want|")
        assert err <= GATE * scale, (label, name, err, scale)


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,K", SINGLE_SHAPES)
def test_single_form(n, d, K, algo, step):
    assert logreg_solve_plan(n, d, LOGREG_FORM_SINGLE).startswith("single")
    check("single", n, d, K, algo, step, *run_solve(n, d, K, algo, step, LOGREG_FORM_SINGLE))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,K", STRIPS_SHAPES)
def test_strips_form(n, d, K, algo, step):
    assert logreg_solve_plan(n, d, LOGREG_FORM_STRIPS).startswith("strips")
    check("strips", n, d, K, algo, step, *run_solve(n, d, K, algo, step, LOGREG_FORM_STRIPS))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,K,strips", GIVEN_STRIPS)
def test_strips_form_with_a_given_strip_count(n, d, K, strips, algo, step):
    """1 strip, strips that do not divide n, more strips than rows (empty strips write zeros)."""
    assert logreg_solve_plan(n, d, LOGREG_FORM_STRIPS, strips).startswith(f"strips G={strips}:")
    check(f"strips G={strips}", n, d, K, algo, step, *run_solve(n, d, K, algo, step, LOGREG_FORM_STRIPS, strips))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,K", AUTO_SHAPES)
def test_auto_form(n, d, K, algo, step):
    check("auto: " + logreg_solve_plan(n, d).split(":")[0], n, d, K, algo, step, *run_solve(n, d, K, algo, step, LOGREG_FORM_AUTO))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,K,form", [(257, 129, 5, LOGREG_FORM_SINGLE), (513, 1025, 6, LOGREG_FORM_STRIPS)])
def test_deterministic_and_independent_of_the_workspace(n, d, K, form, algo, step):
    """Two runs are bit-equal, the second on a workspace full of NaN: nothing is read from it that the solve has not written."""
    a_out, a_coeff = run_solve(n, d, K, algo, step, form)
    b_out, b_coeff = run_solve(n, d, K, algo, step, form, dirty_ws=float("nan"))
    assert np.array_equal(a_out, b_out) and np.array_equal(a_coeff, b_coeff)
    check("dirty workspace", n, d, K, algo, step, b_out, b_coeff)


@pytest.mark.parametrize("form,n,d,K", [(LOGREG_FORM_SINGLE, 37, 5, 3), (LOGREG_FORM_STRIPS, 37, 5, 3), (LOGREG_FORM_STRIPS, 4096, 257, 2)])
def test_inputs_unchanged_writes_in_bounds_and_coeff_is_optional(form, n, d, K):
    """run_solve holds every case to this; here also without `coeff` (NULL): the buffer it would go to stays untouched."""
    for algo, step in ALGOS:
        out, _ = run_solve(n, d, K, algo, step, form, with_coeff=False)
        with_coeff, coeff = run_solve(n, d, K, algo, step, form)
        assert np.array_equal(out, with_coeff)
        w = host_inputs(n, d)[1].numpy()
        assert np.array_equal(coeff, w * with_coeff)   # one fp32 product, exactly


def test_zero_iterations_through_the_abi():
    """K = 0: x_0 = 0 (CG), p_0 = rhs (Neumann), scaled."""
    n, d = 37, 5
    for form in (LOGREG_FORM_SINGLE, LOGREG_FORM_STRIPS):
        for algo, step in ALGOS:
            check("K=0", n, d, 0, algo, step, *run_solve(n, d, 0, algo, step, form))


# ---- through the front ends --------------------------------------------------------------------------------------------------------
def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _front_end(name, sync):
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config, device=DEV)
    zoo.attach_logreg_structure(curr)
    before = dict(LOGREG_SOLVE_STATS)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, sync)
    if sync:
        assert out is None
        out = [p.grad for p in prev.trainable_parameters()]
    rel, mx = rel_err(_np(out), golden_list(outputs, case.name, "fp32"))
    print(f"{name} sync={sync}: rel = {rel:.3e}, max = {mx:.3e} against the reference's fp32 golden")
    assert rel <= 1e-4 and mx <= 1e-3, (rel, mx)
    return {k: LOGREG_SOLVE_STATS[k] - before[k] for k in before}


@pytest.mark.parametrize("name", ["logreg_cg5", "logreg_cg3_a01", "logreg_neumann5"])
@pytest.mark.parametrize("sync", [False, True])
def test_front_end_takes_the_native_solve(name, sync):
    assert _front_end(name, sync) == {"fused": 1, "loop": 0}


@pytest.mark.parametrize("name", ["logreg_cg0", "logreg_neumann0"])
@pytest.mark.parametrize("sync", [False, True])
def test_front_end_zero_iterations_keep_the_loop(name, sync):
    assert _front_end(name, sync)["fused"] == 0


def _declared_problem(n, d, algo, K, step, impl=None):
    X, w, lam, rhs = device_inputs(n, d)
    inner, upper = zoo.Vec(d, 0.0).to(DEV), zoo.Vec(d, 1.0).to(DEV)
    inner.w.data.copy_(w)
    upper.w.data.copy_(lam)
    y = (torch.rand(n, generator=torch.Generator().manual_seed(1)) < 0.5).float().to(DEV)
    cfg = dict(type="cg", cg_iterations=K, cg_alpha=step) if algo == "cg" else dict(type="neumann", neumann_iterations=K, neumann_alpha=step)
    prev = zoo.StubProblem("upper", upper, config=Config())
    curr = zoo.StubProblem("inner", inner, config=Config(**cfg), loss_fn=zoo.make_logreg_loss(prev), batch=(X, y))
    curr.hypergradient_structure = lambda prev_: LogisticRegressionL2(curr, prev_, curr.module.w, lam_fn=lambda: prev_.fwd(), impl=impl)
    return curr, prev, [rhs.clone()]


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,impl", [(64, 4097, None), (500, 100, "torch")], ids=["d4097", "impl_torch"])
def test_front_end_fallbacks_take_the_loop(n, d, impl, algo, step):
    """No native form (d > 4096) and impl = "torch": today's K x (product + recurrence kernel), counted under `loop`."""
    K = 3
    curr, prev, vector = _declared_problem(n, d, algo, K, step, impl)
    before = dict(LOGREG_SOLVE_STATS)
    (got,) = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
    assert {k: LOGREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": 0, "loop": 1}
    want = wanted(n, d, K, algo, step)[1]
    err, scale = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max(), np.abs(want).max()
    print(f"fallback n={n} d={d} impl={impl} {algo} step={step}: max|got - want| = {err:.3e} = {err / scale:.3e} of max|want|")
    assert err <= GATE * scale


def test_front_end_native_solve_on_a_declared_strips_problem():
    """A declared problem too wide for one workgroup: the front end takes the strips form and matches the fp64 restatement."""
    n, d, K = 513, 1025, 6
    for algo, step in ALGOS:
        curr, prev, vector = _declared_problem(n, d, algo, K, step)
        before = dict(LOGREG_SOLVE_STATS)
        (got,) = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        assert {k: LOGREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": 1, "loop": 0}
        want = wanted(n, d, K, algo, step)[1]
        err, scale = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max(), np.abs(want).max()
        print(f"front end strips n={n} d={d} {algo} step={step}: max|got - want| = {err:.3e} = {err / scale:.3e} of max|want|")
        assert err <= GATE * scale

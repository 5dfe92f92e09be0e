"""The native softmax-regression solvers (csrc/bhg_softreg_solve.hip: bhg_softreg_cg_solve / bhg_softreg_neumann_solve) through the C
ABI, against the fp64 restatement of the reference's iteration (tests/softreg_ref.py), and through the front ends
(SoftmaxRegressionL2.fused_cg / fused_neumann) against the reference's goldens.

Inputs per case, seeded n + d + C: X ~ N(0, 1), W = 0.3 N(0, 1), lam in [0.5, 1.5), rhs ~ N(0, 1); the saturated variant takes
W = 6.0 N(0, 1), logits into the hundreds (a softmax without its row maximum, or padded classes left in it, returns NaN there).
Gate of the kernel tests, the one tests/test_logreg_solve.py uses: max|got - want| <= 2e-5 max|want| for `out` and for `coeff`
(= W * out).  An fp32 ATen evaluation of the same iteration sits at <= 2.1e-7 of max|want| on every shape below and <= 3.2e-7 on the
saturated variant, so the gate excludes no case.  Every case also checks that the inputs are bit-equal afterwards and that `out`,
`coeff` and the workspace — slices of larger sentinel-filled buffers — were written inside their bounds only.
"""
import functools

import numpy as np
import pytest
import torch

import softreg_ref as ref
import softreg_zoo
import zoo
from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd.backend import SOFTREG_FORM_AUTO, SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS, get_backend, softreg_solve_plan
from betty_amd.hypergradient._common import SOFTREG_SOLVE_STATS
from betty_amd.hypergradient.structured import SoftmaxRegressionL2
from conftest import golden_list, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2e-5
# algorithm, step (cg_alpha | alpha): textbook CG, the cg_alpha quirk, Neumann
ALGOS = [("cg", 1.0), ("cg", 0.1), ("neumann", 0.25)]
ALGO_IDS = ["cg_a1", "cg_a01", "neumann_a025"]
# (n, d, C, K): smallest possible | d % 4 != 0, rows < 16 | row-tile tail, 13 padded classes | aligned | full class tile, unaligned row
# starts | tails | the MNIST shape
SINGLE_SHAPES = [(1, 1, 2, 1), (3, 2, 2, 2), (17, 5, 3, 3), (64, 64, 10, 4), (33, 129, 16, 4), (257, 130, 7, 5)]
# ... | strips only | strips only | strips only, the family's C d limit
STRIPS_SHAPES = SINGLE_SHAPES + [(100, 784, 10, 5), (513, 1025, 10, 4), (4096, 257, 12, 6), (2048, 2048, 16, 3)]
GIVEN_STRIPS = [(17, 5, 3, 3, 1), (17, 5, 3, 3, 7), (3, 2, 2, 2, 8), (4096, 257, 12, 6, 3)]
SATURATED = [(64, 64, 10, 4), (257, 130, 7, 5)]
PAD, SENTINEL, SENTINEL_BYTE = 64, 1234.5, 0xA5


@functools.lru_cache(maxsize=None)
def host_inputs(n, d, C, w_scale=0.3):
    g = torch.Generator().manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g)
    W = w_scale * torch.randn(C, d, generator=g)
    lam = 0.5 + torch.rand(C, d, generator=g)
    rhs = torch.randn(C * d, generator=g)
    return X, W, lam, rhs


@functools.lru_cache(maxsize=None)
def device_inputs(n, d, C, w_scale=0.3):
    return tuple(t.to(DEV) for t in host_inputs(n, d, C, w_scale))


@functools.lru_cache(maxsize=None)
def wanted(n, d, C, K, algo, step, w_scale=0.3):
    """(-step-scaled solution, its lam cotangent W * (-solution)) in fp64 — computed once per case, shared, read-only."""
    X, W, lam, rhs = (t.numpy() for t in host_inputs(n, d, C, w_scale))
    sol = ref.SOLVERS[algo](X, W, lam, rhs, K, step)
    out, coeff = -sol, ref.lam_cotangent(W, sol)
    out.setflags(write=False)
    coeff.setflags(write=False)
    return out, coeff


def run_solve(n, d, C, K, algo, step, form, strips=0, dirty_ws=None, with_coeff=True, w_scale=0.3):
    """One solve with out_scale = -step (what the front ends ask for).  Returns (out, coeff) as float32 host arrays after checking
    that the inputs are unchanged and nothing outside out / coeff / the workspace was written."""
    be = get_backend()
    ins = device_inputs(n, d, C, w_scale)
    before = [t.clone() for t in ins]
    X, W, lam, rhs = ins
    N = C * d
    ws_bytes = int(be.lib.bhg_softreg_solve_ws_bytes(n, d, C))
    assert ws_bytes > 0
    outbuf = torch.full((N + 2 * PAD,), SENTINEL, device=DEV)
    cobuf = torch.full((N + 2 * PAD,), SENTINEL, device=DEV)
    wsbuf = torch.full((ws_bytes + 2 * PAD,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    out, coeff, ws = outbuf[PAD:PAD + N], cobuf[PAD:PAD + N], wsbuf[PAD:PAD + ws_bytes]
    assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if dirty_ws is not None:
        ws.view(torch.float32)[: ws_bytes // 4].fill_(dirty_ws)
    fn = be.softreg_cg_solve if algo == "cg" else be.softreg_neumann_solve
    fn(X, W, lam, rhs, out, coeff if with_coeff else None, ws, K, step, -step, form, strips)
    torch.cuda.synchronize()
    for a, b in zip(ins, before):
        assert torch.equal(a, b), "an input was modified"
    for buf, val in ((outbuf, SENTINEL), (cobuf, SENTINEL)):
        assert bool((buf[:PAD] == val).all()) and bool((buf[PAD + N:] == val).all()), "write outside out / coeff"
    if not with_coeff:
        assert bool((cobuf == SENTINEL).all())
    assert bool((wsbuf[:PAD] == SENTINEL_BYTE).all()) and bool((wsbuf[PAD + ws_bytes:] == SENTINEL_BYTE).all()), "write outside the workspace"
    return out.cpu().numpy(), coeff.cpu().numpy()


def check(label, n, d, C, K, algo, step, got_out, got_coeff, w_scale=0.3):
    want_out, want_coeff = wanted(n, d, C, K, algo, step, w_scale)
    for name, got, want in (("out", got_out, want_out), ("coeff", got_coeff, want_coeff)):
        err, scale = np.abs(got.astype(np.float64) - want).max(), np.abs(want).max()
        print(f"{label} n={n} d={d} C={C} K={K} {algo} step={step} {name}: max|got - want| = {err:.3e} = {err / scale if scale else 0.0:.3e} of max|want|")
        assert np.isfinite(got).all(), (label, name)
        assert err <= GATE * scale, (label, name, err, scale)


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K", SINGLE_SHAPES)
def test_single_form(n, d, C, K, algo, step):
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_SINGLE).startswith("single")
    check("single", n, d, C, K, algo, step, *run_solve(n, d, C, K, algo, step, SOFTREG_FORM_SINGLE))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K", STRIPS_SHAPES)
def test_strips_form(n, d, C, K, algo, step):
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_STRIPS).startswith("strips")
    check("strips", n, d, C, K, algo, step, *run_solve(n, d, C, K, algo, step, SOFTREG_FORM_STRIPS))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K,strips", GIVEN_STRIPS)
def test_strips_form_with_a_given_strip_count(n, d, C, K, strips, algo, step):
    """1 strip, strips that do not divide n, more strips than rows (empty strips write zeros), strips of several super-tiles."""
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_STRIPS, strips).startswith(f"strips G={strips}:")
    check(f"strips G={strips}", n, d, C, K, algo, step, *run_solve(n, d, C, K, algo, step, SOFTREG_FORM_STRIPS, strips))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("form", [SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS], ids=["single", "strips"])
@pytest.mark.parametrize("n,d,C,K", SATURATED)
def test_saturated_logits(n, d, C, K, form, algo, step):
    X, W, _, _ = host_inputs(n, d, C, 6.0)
    assert float((X @ W.t()).abs().max()) > 100.0
    got = run_solve(n, d, C, K, algo, step, form, w_scale=6.0)
    check("saturated", n, d, C, K, algo, step, *got, w_scale=6.0)


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K", [(64, 64, 10, 4), (513, 1025, 10, 4)])
def test_auto_form(n, d, C, K, algo, step):
    check("auto: " + softreg_solve_plan(n, d, C).split(":")[0], n, d, C, K, algo, step, *run_solve(n, d, C, K, algo, step, SOFTREG_FORM_AUTO))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K,form", [(257, 130, 7, 5, SOFTREG_FORM_SINGLE), (513, 1025, 10, 4, SOFTREG_FORM_STRIPS)])
def test_deterministic_and_independent_of_the_workspace(n, d, C, K, form, algo, step):
    """Two runs are bit-equal, the second on a workspace full of NaN: nothing is read from it that the solve has not written."""
    a_out, a_coeff = run_solve(n, d, C, K, algo, step, form)
    b_out, b_coeff = run_solve(n, d, C, K, algo, step, form, dirty_ws=float("nan"))
    assert np.array_equal(a_out, b_out) and np.array_equal(a_coeff, b_coeff)
    check("dirty workspace", n, d, C, K, algo, step, b_out, b_coeff)


@pytest.mark.parametrize("form,n,d,C,K", [(SOFTREG_FORM_SINGLE, 17, 5, 3, 3), (SOFTREG_FORM_STRIPS, 17, 5, 3, 3), (SOFTREG_FORM_STRIPS, 4096, 257, 12, 2)])
def test_coeff_is_optional_and_is_one_rounded_product(form, n, d, C, K):
    """run_solve holds every case to the bounds; here also without `coeff` (NULL): the buffer it would go to stays untouched."""
    for algo, step in ALGOS:
        out, _ = run_solve(n, d, C, K, algo, step, form, with_coeff=False)
        with_coeff, coeff = run_solve(n, d, C, K, algo, step, form)
        assert np.array_equal(out, with_coeff)
        W = host_inputs(n, d, C)[1].numpy().reshape(-1)
        assert np.array_equal(coeff, W * with_coeff)   # one fp32 product, exactly


def test_zero_iterations_through_the_abi():
    """K = 0: x_0 = 0 (CG), p_0 = rhs (Neumann), scaled."""
    n, d, C = 17, 5, 3
    for form in (SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS):
        for algo, step in ALGOS:
            check("K=0", n, d, C, 0, algo, step, *run_solve(n, d, C, 0, algo, step, form))


# ---- through the front ends --------------------------------------------------------------------------------------------------------
def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


@pytest.mark.parametrize("name", ["softreg_cg5", "softreg_cg5_a01", "softreg_neumann5"])
@pytest.mark.parametrize("sync", [False, True])
def test_front_end_takes_the_native_solve(name, sync):
    """The golden instance, default impl: the first-use guard passes on the honest problem and the native solve runs."""
    case = softreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("softreg")
    curr, prev, vector = softreg_zoo.build_case(case, inputs, Config, device=DEV)
    softreg_zoo.attach_structure(curr)
    before = dict(SOFTREG_SOLVE_STATS)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, sync)
    if sync:
        assert out is None
        out = [p.grad for p in prev.trainable_parameters()]
    assert {k: SOFTREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": 1, "loop": 0}
    assert any(k[-1] == "SoftmaxRegressionL2" for k in curr._bhg_structure_verified), "the guard ran and passed"
    rel, mx = rel_err(_np(out), golden_list(outputs, name, "fp32"))
    print(f"{name} sync={sync}: rel = {rel:.3e}, max = {mx:.3e} against the reference's fp32 golden")
    assert rel <= 1e-4 and mx <= 1e-3, (rel, mx)


@pytest.mark.parametrize("name", ["softreg_darts", "softreg_sama"])
def test_front_end_finite_difference_hop(name):
    case = softreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("softreg")
    curr, prev, vector = softreg_zoo.build_case(case, inputs, Config, device=DEV)
    softreg_zoo.attach_structure(curr)
    curr.training_step_exec = None   # the closed form never calls it
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    rel, _ = rel_err(_np(out), golden_list(outputs, name, "fp32"))
    assert rel <= 1e-4, rel


def _declared_problem(n, d, C, algo, K, step, strided_x=False):
    X, W, lam, rhs = device_inputs(n, d, C)
    if strided_x:
        X = torch.stack([X, X], dim=-1)[..., 0]
        assert not X.is_contiguous()
    inner = torch.nn.Linear(d, C, bias=False).to(DEV)
    inner.weight.data.copy_(W)
    upper = zoo.Vec(C * d, 1.0).to(DEV)
    upper.w.data.copy_(lam.reshape(-1))
    y = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(1)).to(DEV)
    cfg = dict(type="cg", cg_iterations=K, cg_alpha=step) if algo == "cg" else dict(type="neumann", neumann_iterations=K, neumann_alpha=step)
    prev = zoo.StubProblem("upper", upper, config=Config())

    def loss(self, batch):
        x, yy = batch
        w = self.module.weight
        return torch.nn.functional.cross_entropy(self.module(x), yy) + 0.5 * (prev.fwd().reshape(w.shape) * w * w).sum()

    curr = zoo.StubProblem("inner", inner, config=Config(**cfg), loss_fn=loss, batch=(X, y))
    curr.hypergradient_structure = lambda p: SoftmaxRegressionL2(curr, p, inner.weight, lam_fn=lambda: p.fwd().reshape(C, d))
    return curr, prev, [rhs.reshape(C, d).clone()]


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,strided,fused", [(64, 64, 17, False, 0), (64, 64, 10, True, 0), (64, 64, 10, False, 1), (513, 1025, 10, False, 1)],
                         ids=["C17_loop", "strided_X_loop", "single", "strips"])
def test_front_end_on_declared_problems(n, d, C, strided, fused, algo, step):
    """Outside the family (C = 17) and a non-contiguous X: today's K x (product + recurrence kernel), counted under `loop`; inside:
    the native solve.  Either way the hypergradient w.r.t. lam matches the fp64 restatement."""
    K = 3
    curr, prev, vector = _declared_problem(n, d, C, algo, K, step, strided)
    before = dict(SOFTREG_SOLVE_STATS)
    (got,) = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
    assert {k: SOFTREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": fused, "loop": 1 - fused}
    want = wanted(n, d, C, K, algo, step)[1]
    err, scale = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max(), np.abs(want).max()
    print(f"front end n={n} d={d} C={C} strided={strided} {algo} step={step}: max|got - want| = {err:.3e} = {err / scale:.3e} of max|want|")
    assert err <= GATE * scale

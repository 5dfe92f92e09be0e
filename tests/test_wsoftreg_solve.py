"""The row-weighted native solves and the mixed pass of sample-weighted softmax regression (csrc/bhg_softreg_solve.hip:
bhg_wsoftreg_cg_solve / bhg_wsoftreg_neumann_solve / bhg_wsoftreg_mixed) through the C ABI, against the fp64 restatement
(tests/wsoftreg_ref.py), and through the front ends (WeightedSoftmaxRegression.fused_cg / fused_neumann / mixed_vjp) against the
reference's goldens.

Inputs per case, seeded n + d + C, the first four exactly those of tests/test_softreg_solve.py: X ~ N(0, 1), W = 0.3 N(0, 1), reg in
[0.5, 1.5), rhs ~ N(0, 1); then a = 2.5 U(0, 1) with every fifth weight exactly 0 and y uniform in [0, C).  The saturated variant takes
W = 6.0 N(0, 1), logits into the hundreds.

Gate of the solves, the project's: max|got - want| <= 2e-5 max|want|.  An fp32 ATen evaluation of the same iteration on exactly these
inputs sits at <= 4.1e-7 of max|want|, the saturated variant included, so the gate excludes no case.  Every case also checks that the
inputs are bit-equal afterwards and that `out` and the workspace — slices of larger sentinel-filled buffers — were written inside their
bounds only.

The mixed pass is fed the fp64 solution rounded to fp32, so its gate sees the kernel alone: 2e-5 of max|c| on the unsaturated shapes
(fp32 ATen sits at <= 2e-6).  On the saturated variant fp32 itself loses digits in the logits (fp32 ATen: 1.3e-5 of max|c| at
4096 x 257 x 12), so the gate there is max(2e-5, 4 x the error of an fp32 ATen evaluation of c on the same inputs) — the factor
tests/test_head_j_fp64.py gives its fp32 spread; the test computes that evaluation on the CPU and prints it.
profiles/wsoftreg_fp64.txt has the observed maxima.
"""
import functools

import numpy as np
import pytest
import torch

import wsoftreg_ref as ref
import wsoftreg_zoo
import zoo
from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd.backend import SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS, get_backend, softreg_solve_plan
from betty_amd.hypergradient._common import WSOFTREG_SOLVE_STATS
from betty_amd.hypergradient.structured import WeightedSoftmaxRegression
from conftest import golden_list, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2e-5
FP32_SPREAD = 4.0
# algorithm, step (cg_alpha | alpha): textbook CG, the cg_alpha quirk, Neumann
ALGOS = [("cg", 1.0), ("cg", 0.1), ("neumann", 0.25)]
ALGO_IDS = ["cg_a1", "cg_a01", "neumann_a025"]
# (n, d, C, K): smallest possible | d % 4 != 0, rows < 16 | row-tile tail, 13 padded classes | aligned | full class tile, unaligned row
# starts | tails | the MNIST shape | strips only | strips only, several super-tiles per strip
SINGLE_SHAPES = [(1, 1, 2, 1), (3, 2, 2, 2), (17, 5, 3, 3), (64, 64, 10, 4), (33, 129, 16, 4), (257, 130, 7, 5)]
STRIPS_SHAPES = SINGLE_SHAPES + [(100, 784, 10, 5), (513, 1025, 10, 4), (4096, 257, 12, 6)]
GIVEN_STRIPS = [(17, 5, 3, 3, 1), (17, 5, 3, 3, 7), (4096, 257, 12, 6, 3)]
SATURATED = [(64, 64, 10, 4), (257, 130, 7, 5)]
# the mixed pass: n = 1 | one tile and a row | one super-tile and a row (two workgroups) | 17 workgroups, the last with three rows;
# then the other widths of the solves (16-byte path: d = 64, 784; 16 classes; d > 1024)
MIXED_SHAPES = [(1, 1, 2, 1), (17, 5, 3, 3), (257, 130, 7, 5), (4099, 257, 12, 6), (64, 64, 10, 4), (33, 129, 16, 4), (100, 784, 10, 5),
                (513, 1025, 10, 4)]
MIXED_SATURATED = SATURATED + [(4096, 257, 12, 6)]
PAD, SENTINEL, SENTINEL_BYTE = 64, 1234.5, 0xA5


@functools.lru_cache(maxsize=None)
def host_inputs(n, d, C, w_scale=0.3):
    g = torch.Generator().manual_seed(n + d + C)
    X = torch.randn(n, d, generator=g)
    W = w_scale * torch.randn(C, d, generator=g)
    reg = 0.5 + torch.rand(C, d, generator=g)
    rhs = torch.randn(C * d, generator=g)
    a = 2.5 * torch.rand(n, generator=g)
    a[::5] = 0.0
    y = torch.randint(0, C, (n,), generator=g)
    return X, W, reg, rhs, a, y


@functools.lru_cache(maxsize=None)
def device_inputs(n, d, C, w_scale=0.3):
    return tuple(t.to(DEV) for t in host_inputs(n, d, C, w_scale))


@functools.lru_cache(maxsize=None)
def solution(n, d, C, K, algo, step, w_scale=0.3):
    """The step-scaled solution in fp64 — computed once per case, shared, read-only."""
    X, W, reg, rhs, a, _ = (t.numpy() for t in host_inputs(n, d, C, w_scale))
    sol = ref.SOLVERS[algo](X, W, reg, a, rhs, K, step)
    sol.setflags(write=False)
    return sol


def run_solve(n, d, C, K, algo, step, form, strips=0, dirty_ws=None, w_scale=0.3, ones=False, unweighted=False):
    """One solve with out_scale = -step (what the front ends ask for).  Returns `out` as a device tensor after checking that the inputs
    are unchanged and nothing outside out / the workspace was written.  ones: a == 1; unweighted: bhg_softreg_*_solve instead."""
    be = get_backend()
    ins = device_inputs(n, d, C, w_scale)
    before = [t.clone() for t in ins]
    X, W, reg, rhs, a, _ = ins
    if ones:
        a = torch.ones_like(a)
    N = C * d
    ws_bytes = int(be.lib.bhg_softreg_solve_ws_bytes(n, d, C))
    assert ws_bytes > 0
    outbuf = torch.full((N + 2 * PAD,), SENTINEL, device=DEV)
    wsbuf = torch.full((ws_bytes + 2 * PAD,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    out, ws = outbuf[PAD:PAD + N], wsbuf[PAD:PAD + ws_bytes]
    assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if dirty_ws is not None:
        ws.view(torch.float32)[: ws_bytes // 4].fill_(dirty_ws)
    if unweighted:
        (be.softreg_cg_solve if algo == "cg" else be.softreg_neumann_solve)(X, W, reg, rhs, out, None, ws, K, step, -step, form, strips)
    else:
        (be.wsoftreg_cg_solve if algo == "cg" else be.wsoftreg_neumann_solve)(X, W, reg, a, rhs, out, ws, K, step, -step, form, strips)
    torch.cuda.synchronize()
    for p, q in zip(ins, before):
        assert torch.equal(p, q), "an input was modified"
    assert bool((outbuf[:PAD] == SENTINEL).all()) and bool((outbuf[PAD + N:] == SENTINEL).all()), "write outside out"
    assert bool((wsbuf[:PAD] == SENTINEL_BYTE).all()) and bool((wsbuf[PAD + ws_bytes:] == SENTINEL_BYTE).all()), "write outside the workspace"
    return out.clone()


def check(label, n, d, C, K, algo, step, got, w_scale=0.3):
    got, want = got.cpu().numpy(), -solution(n, d, C, K, algo, step, w_scale).reshape(-1)
    err, scale = np.abs(got.astype(np.float64) - want).max(), np.abs(want).max()
    print(f"{label} n={n} d={d} C={C} K={K} {algo} step={step} out: max|got - want| = {err:.3e} = {err / scale if scale else 0.0:.3e} of max|want|")
    assert np.isfinite(got).all(), label
    assert err <= GATE * scale, (label, err, scale)


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K", SINGLE_SHAPES)
def test_single_form(n, d, C, K, algo, step):
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_SINGLE).startswith("single")
    check("single", n, d, C, K, algo, step, run_solve(n, d, C, K, algo, step, SOFTREG_FORM_SINGLE))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K", STRIPS_SHAPES)
def test_strips_form(n, d, C, K, algo, step):
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_STRIPS).startswith("strips")
    check("strips", n, d, C, K, algo, step, run_solve(n, d, C, K, algo, step, SOFTREG_FORM_STRIPS))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K,strips", GIVEN_STRIPS)
def test_strips_form_with_a_given_strip_count(n, d, C, K, strips, algo, step):
    """1 strip, strips that do not divide n, strips of several super-tiles."""
    assert softreg_solve_plan(n, d, C, SOFTREG_FORM_STRIPS, strips).startswith(f"strips G={strips}:")
    check(f"strips G={strips}", n, d, C, K, algo, step, run_solve(n, d, C, K, algo, step, SOFTREG_FORM_STRIPS, strips))


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("form", [SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS], ids=["single", "strips"])
@pytest.mark.parametrize("n,d,C,K", SATURATED)
def test_saturated_logits(n, d, C, K, form, algo, step):
    X, W = host_inputs(n, d, C, 6.0)[:2]
    assert float((X @ W.t()).abs().max()) > 100.0
    check("saturated", n, d, C, K, algo, step, run_solve(n, d, C, K, algo, step, form, w_scale=6.0), w_scale=6.0)


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K,form", [(257, 130, 7, 5, SOFTREG_FORM_SINGLE), (513, 1025, 10, 4, SOFTREG_FORM_STRIPS)])
def test_deterministic_and_independent_of_the_workspace(n, d, C, K, form, algo, step):
    """Two runs are bit-equal, the second on a workspace full of NaN: nothing is read from it that the solve has not written."""
    first = run_solve(n, d, C, K, algo, step, form)
    second = run_solve(n, d, C, K, algo, step, form, dirty_ws=float("nan"))
    assert torch.equal(first, second)
    check("dirty workspace", n, d, C, K, algo, step, second)


@pytest.mark.parametrize("form,shapes", [(SOFTREG_FORM_SINGLE, SINGLE_SHAPES), (SOFTREG_FORM_STRIPS, STRIPS_SHAPES)], ids=["single", "strips"])
def test_unit_weights_reproduce_the_unweighted_solve_bit_for_bit(form, shapes):
    for n, d, C, K in shapes:
        for algo, step in ALGOS:
            weighted = run_solve(n, d, C, K, algo, step, form, ones=True)
            plain = run_solve(n, d, C, K, algo, step, form, unweighted=True)
            assert torch.equal(weighted, plain), (n, d, C, K, algo, step)


def test_zero_iterations_through_the_abi():
    """K = 0: x_0 = 0 (CG), p_0 = rhs (Neumann), scaled."""
    n, d, C = 17, 5, 3
    for form in (SOFTREG_FORM_SINGLE, SOFTREG_FORM_STRIPS):
        for algo, step in ALGOS:
            check("K=0", n, d, C, 0, algo, step, run_solve(n, d, C, 0, algo, step, form))


# ---- the mixed pass ------------------------------------------------------------------------------------------------------------------
def run_mixed(n, d, C, K, w_scale=0.3):
    """c of the kernel (float32 host array), the fp64 c and an fp32 ATen evaluation on the CPU, all along the fp64 CG solution rounded
    to fp32.  Checks the inputs and the sentinels around c."""
    be = get_backend()
    X, W, _, _, _, y = device_inputs(n, d, C, w_scale)
    hX, hW, _, _, _, hy = host_inputs(n, d, C, w_scale)
    direction = torch.from_numpy(solution(n, d, C, K, "cg", 1.0, w_scale).astype(np.float32)).reshape(-1)
    dev_dir = direction.to(DEV)
    before = [t.clone() for t in (X, W, dev_dir, y)]
    cbuf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
    c = cbuf[PAD:PAD + n]
    assert y.dtype == torch.int64
    be.wsoftreg_mixed(X, W, dev_dir, y, c)
    torch.cuda.synchronize()
    for p, q in zip((X, W, dev_dir, y), before):
        assert torch.equal(p, q), "an input was modified"
    assert bool((cbuf[:PAD] == SENTINEL).all()) and bool((cbuf[PAD + n:] == SENTINEL).all()), "write outside c"
    assert bool((c != SENTINEL).all()), "a row was not written"
    want = ref.weight_cotangent(hX.numpy(), hW.numpy(), hy.numpy(), direction.numpy())
    PmY = torch.softmax(hX @ hW.t(), dim=1)
    PmY[torch.arange(n), hy] -= 1.0
    aten = ((PmY * (hX @ direction.reshape(C, d).t())).sum(dim=1) / n).numpy()
    return c.cpu().numpy(), want, aten


@pytest.mark.parametrize("n,d,C,K", MIXED_SHAPES)
def test_mixed_pass(n, d, C, K):
    got, want, aten = run_mixed(n, d, C, K)
    scale = np.abs(want).max()
    err, err_aten = np.abs(got.astype(np.float64) - want).max(), np.abs(aten.astype(np.float64) - want).max()
    print(f"mixed n={n} d={d} C={C}: max|got - want| = {err:.3e} = {err / scale:.3e} of max|c|; fp32 ATen: {err_aten / scale:.3e}")
    assert np.isfinite(got).all() and scale > 0
    assert err <= GATE * scale, (err, scale)


@pytest.mark.parametrize("n,d,C,K", MIXED_SATURATED)
def test_mixed_pass_on_saturated_logits(n, d, C, K):
    got, want, aten = run_mixed(n, d, C, K, w_scale=6.0)
    scale = np.abs(want).max()
    err, err_aten = np.abs(got.astype(np.float64) - want).max(), np.abs(aten.astype(np.float64) - want).max()
    gate = max(GATE, FP32_SPREAD * err_aten / scale)
    print(f"mixed saturated n={n} d={d} C={C}: max|got - want| = {err:.3e} = {err / scale:.3e} of max|c|; fp32 ATen: {err_aten / scale:.3e}; "
          f"gate {gate:.3e}")
    assert np.isfinite(got).all() and scale > 0
    assert err <= gate * scale, (err, scale, gate)


def test_mixed_pass_is_deterministic():
    a, _, _ = run_mixed(4099, 257, 12, 6)
    b, _, _ = run_mixed(4099, 257, 12, 6)
    assert np.array_equal(a, b)


# ---- through the front ends --------------------------------------------------------------------------------------------------------
def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


@pytest.mark.parametrize("name", ["wsoftreg_cg5", "wsoftreg_cg5_a01", "wsoftreg_neumann5"])
@pytest.mark.parametrize("sync", [False, True])
def test_front_end_takes_the_native_path(name, sync):
    """The golden instance, default impl: the first-use guard passes on the honest problem, the native solve and the mixed pass run."""
    case = wsoftreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("wsoftreg")
    curr, prev, vector = wsoftreg_zoo.build_case(case, inputs, Config, device=DEV)
    wsoftreg_zoo.attach_structure(curr)
    before = dict(WSOFTREG_SOLVE_STATS)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, sync)
    if sync:
        assert out is None
        out = [p.grad for p in prev.trainable_parameters()]
    assert {k: WSOFTREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": 1, "loop": 0}
    assert any(k[-1] == "WeightedSoftmaxRegression" for k in curr._bhg_structure_verified), "the guard ran and passed"
    rel, mx = rel_err(_np(out), golden_list(outputs, name, "fp32"))
    print(f"{name} sync={sync}: rel = {rel:.3e}, max = {mx:.3e} against the reference's fp32 golden")
    assert rel <= 1e-4 and mx <= 1e-3, (rel, mx)


def _declared_problem(n, d, C, algo, K, step, transposed_x=False):
    X, W, reg, rhs, a, y = device_inputs(n, d, C)
    if transposed_x:
        X = X.t().contiguous().t()
        assert not X.is_contiguous()
    inner = torch.nn.Linear(d, C, bias=False).to(DEV)
    inner.weight.data.copy_(W)
    upper = zoo.Vec(n, 1.0).to(DEV)
    upper.w.data.copy_(a)
    cfg = dict(type="cg", cg_iterations=K, cg_alpha=step) if algo == "cg" else dict(type="neumann", neumann_iterations=K, neumann_alpha=step)
    prev = zoo.StubProblem("upper", upper, config=Config())

    def loss(self, batch):
        x, yy = batch
        w = self.module.weight
        return (prev.fwd() * torch.nn.functional.cross_entropy(self.module(x), yy, reduction="none")).mean() + 0.5 * (reg * w * w).sum()

    curr = zoo.StubProblem("inner", inner, config=Config(**cfg), loss_fn=loss, batch=(X, y))
    curr.hypergradient_structure = lambda p: WeightedSoftmaxRegression(curr, p, inner.weight, weight_fn=lambda: p.fwd(), reg=reg)
    return curr, prev, [rhs.reshape(C, d).clone()]


@pytest.mark.parametrize("algo,step", ALGOS, ids=ALGO_IDS)
@pytest.mark.parametrize("n,d,C,K,how,fused", [(64, 64, 10, 0, None, 0), (64, 64, 17, 3, None, 0), (64, 64, 10, 3, "transposed", 0),
                                               (64, 64, 10, 3, "fd", 0), (64, 64, 10, 3, None, 1), (513, 1025, 10, 3, None, 1)],
                         ids=["K0_loop", "C17_loop", "transposed_X_loop", "finite_difference_loop", "single", "strips"])
def test_front_end_on_declared_problems(n, d, C, K, how, fused, algo, step):
    """K = 0, outside the family (C = 17), a non-contiguous X, hypergradient_hvp = "finite_difference": K x (product + recurrence
    kernel) and c in ATen, counted under `loop`; inside: the native path.  Either way the hypergradient with respect to the sample
    weights (the upper parameter IS a here) matches the fp64 restatement."""
    curr, prev, vector = _declared_problem(n, d, C, algo, K, step, how == "transposed")
    if how == "fd":
        curr.hypergradient_hvp = "finite_difference"
    before = dict(WSOFTREG_SOLVE_STATS)
    (got,) = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
    assert {k: WSOFTREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": fused, "loop": 1 - fused}
    X, W, _, _, _, y = (t.numpy() for t in host_inputs(n, d, C))
    want = ref.weight_cotangent(X, W, y, -solution(n, d, C, K, algo, step))
    err, scale = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max(), np.abs(want).max()
    print(f"front end n={n} d={d} C={C} K={K} {how} {algo} step={step}: max|got - want| = {err:.3e} = {err / scale if scale else 0.0:.3e} of max|want|")
    assert got.shape == (n,) and err <= GATE * scale

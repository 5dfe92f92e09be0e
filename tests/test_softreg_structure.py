"""``SoftmaxRegressionL2`` (betty_amd/hypergradient/structured.py) on the CPU: the ATen closed form (``impl="torch"``) with the checker
backend, through the four front ends, against the reference's own fp32 results on the seeded instance of tests/softreg_zoo.py
(tests/golden/softreg.npz), and the first-use guard against training steps the declaration does not describe."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import softreg_zoo
from _cpu_checker_backend import CpuCheckerBackend
from conftest import golden_list, load_golden, rel_err

from betty_amd import Config, _native
from betty_amd import hypergradient as hg
from betty_amd.backend import use_backend
from betty_amd.hypergradient import structured
from betty_amd.hypergradient._common import SOFTREG_SOLVE_STATS
from betty_amd.hypergradient.structured import SoftmaxRegressionL2, StructureMismatchError

NAMES = [c.name for c in softreg_zoo.CASES]


@pytest.fixture()
def checker():
    with use_backend(CpuCheckerBackend()) as b:
        yield b


def _case(name, impl="torch", inner=None, loss_kw=None, **kw):
    case = softreg_zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden("softreg")
    curr, prev, vector = softreg_zoo.build_case(case, inputs, Config, inner=inner, **(loss_kw or {}))
    if impl is not None:
        softreg_zoo.attach_structure(curr, impl=impl, **kw)
    return case, outputs, curr, prev, vector


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _count_training_steps(curr):
    ran, real = [], curr.training_step_exec

    def counted(batch):
        ran.append(1)
        return real(batch)

    curr.training_step_exec = counted
    return ran


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_front_ends_reproduce_the_reference(name, sync, checker):
    case, outputs, curr, prev, vector = _case(name)
    ran = _count_training_steps(curr)
    before = dict(SOFTREG_SOLVE_STATS)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, sync)
    if sync:
        assert out is None
        out = [p.grad for p in prev.trainable_parameters()]
    rel, mx = rel_err(_np(out), golden_list(outputs, name, "fp32"))
    print(f"{name} sync={sync}: rel = {rel:.3e}, max = {mx:.3e} against the reference's fp32 golden")
    assert rel <= 1e-4 and mx <= 1e-3, (rel, mx)
    if case.algo in ("cg", "neumann"):
        assert len(ran) == 1, "one training_step: the first-use guard; the products are closed form"
        assert {k: SOFTREG_SOLVE_STATS[k] - before[k] for k in before} == {"fused": 0, "loop": 1}   # impl = "torch" keeps the loop
    else:
        assert len(ran) == 0, "the closed-form hop never calls training_step"


def test_guard_verdict_is_cached_on_the_problem(checker):
    case, _, curr, prev, vector = _case("softreg_cg5")
    ran = _count_training_steps(curr)
    hg.cg(vector, curr, prev, False)
    hg.cg(vector, curr, prev, False)
    assert len(ran) == 1
    case, _, curr, prev, vector = _case("softreg_cg5", verify=False)
    ran = _count_training_steps(curr)
    hg.cg(vector, curr, prev, False)
    assert len(ran) == 0


def test_guard_leaves_the_rng_stream_alone(checker):
    case, _, curr, prev, vector = _case("softreg_neumann5")
    torch.manual_seed(7)
    want = torch.rand(3)
    torch.manual_seed(7)
    hg.neumann(vector, curr, prev, False)
    assert torch.equal(torch.rand(3), want)


def test_darts_leaves_the_opaque_paths_weights(checker):
    case, outputs, curr, prev, vector = _case("softreg_darts", impl=None)
    ran = _count_training_steps(curr)
    hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    want = [p.data.clone() for p in curr.parameters()]
    case, _, curr, prev, vector = _case("softreg_darts")
    hg.darts(vector, curr, prev, False)
    for a, b in zip(curr.parameters(), want):
        assert torch.equal(a.data, b)
    for a, w in zip(curr.parameters(), golden_list(outputs, "softreg_darts", "w32")):
        np.testing.assert_allclose(a.data.numpy(), w, rtol=0, atol=2e-7)   # (the reference's own perturb / restore drift)


@pytest.mark.parametrize("loss_kw", [dict(label_smoothing=0.1), dict(reduction="sum"), dict(penalty=1.0)],
                         ids=["label_smoothing", "reduction_sum", "penalty_without_half"])
@pytest.mark.parametrize("algo", ["softreg_cg5", "softreg_neumann5"])
def test_guard_raises_on_a_training_step_the_closed_form_does_not_describe(algo, loss_kw, checker):
    case, _, curr, prev, vector = _case(algo, loss_kw=loss_kw)
    with pytest.raises(StructureMismatchError, match="SoftmaxRegressionL2"):
        hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    # ... and a refused problem is not remembered as verified
    with pytest.raises(StructureMismatchError):
        hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)


def test_guard_passes_at_the_inner_optimum(checker):
    """Where the unrolled inner loop leaves the weights the gradient's two terms cancel: the check measures its error against their
    size, not against the vanishing sum (a relative error of the sum would refuse every converged honest problem)."""
    case, _, curr, prev, vector = _case("softreg_cg5")
    w = curr.module.weight
    for _ in range(400):
        (g,) = torch.autograd.grad(curr.training_step_exec(curr.cur_batch), [w])
        w.data.sub_(0.5 * g)
    (g,) = torch.autograd.grad(curr.training_step_exec(curr.cur_batch), [w])
    assert float(g.norm()) < 1e-5 * float(w.norm())
    hg.cg(vector, curr, prev, False)
    case, _, curr2, prev2, vector = _case("softreg_cg5", loss_kw=dict(label_smoothing=0.1))
    curr2.module.weight.data.copy_(w.data)
    with pytest.raises(StructureMismatchError):
        hg.cg(vector, curr2, prev2, False)


def test_guard_can_be_switched_off(checker):
    case, _, curr, prev, vector = _case("softreg_cg5", loss_kw=dict(reduction="sum"), verify=False)
    hg.cg(vector, curr, prev, False)
    case, _, curr, prev, vector = _case("softreg_cg5", loss_kw=dict(reduction="sum"))
    structured.VERIFY_STRUCTURE = False
    try:
        hg.cg(vector, curr, prev, False)
    finally:
        structured.VERIFY_STRUCTURE = True


def test_a_model_with_a_bias_is_refused():
    inputs, _ = load_golden("softreg")
    inner = nn.Linear(softreg_zoo.N_FEATURES, softreg_zoo.N_CLASSES, bias=True)
    curr, prev, _ = softreg_zoo.build_case(softreg_zoo.CASE_BY_NAME["softreg_cg5"], inputs, Config, inner=inner)
    with pytest.raises(ValueError, match="bias"):
        SoftmaxRegressionL2(curr, prev, inner.weight, lam_fn=lambda: prev.fwd())
    vec = nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="2-D"):
        SoftmaxRegressionL2(curr, prev, vec, lam_fn=lambda: prev.fwd())


def test_default_impl_has_no_cpu_fallback():
    case, _, curr, prev, vector = _case("softreg_cg5", impl=None)
    softreg_zoo.attach_structure(curr)
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        curr.hypergradient_structure(prev).prepare()


def test_lam_may_broadcast(checker):
    """One coefficient per feature, shared by the classes: lam of shape [d] broadcasts to [C, d]."""
    case, _, curr, prev, vector = _case("softreg_cg5", impl=None)
    theta = nn.Parameter(torch.full((softreg_zoo.N_FEATURES,), 0.3))
    prev.module = nn.ParameterList([theta])
    prev.fwd = lambda: torch.nn.functional.softplus(theta)
    (want,) = hg.cg(vector, curr, prev, False)            # opaque double backward
    curr.hypergradient_structure = lambda p: SoftmaxRegressionL2(curr, p, curr.module.weight, lam_fn=lambda: p.fwd(), impl="torch")
    (got,) = hg.cg(vector, curr, prev, False)
    rel, _ = rel_err(_np([got]), _np([want]))
    assert got.shape == theta.shape and rel <= 1e-4, rel


class _DropoutLinear(nn.Module):
    def __init__(self):
        super().__init__()
        self.drop = nn.Dropout(0.5)
        self.lin = nn.Linear(softreg_zoo.N_FEATURES, softreg_zoo.N_CLASSES, bias=False)

    @property
    def weight(self):
        return self.lin.weight

    def forward(self, x):
        return self.lin(self.drop(x))


def test_declined_and_side_effect_modules_take_the_opaque_hop(checker):
    case, _, curr, prev, vector = _case("softreg_darts", closed_form_fd=False)
    ran = _count_training_steps(curr)
    hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    case, _, curr, prev, vector = _case("softreg_darts", inner=_DropoutLinear())
    assert curr.module.training
    ran = _count_training_steps(curr)
    hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    case, _, curr, prev, vector = _case("softreg_darts", inner=_DropoutLinear())
    curr.module.eval()
    ran = _count_training_steps(curr)
    hg.darts(vector, curr, prev, False)
    assert len(ran) == 0

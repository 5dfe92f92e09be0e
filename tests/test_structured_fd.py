"""The finite-difference hop (darts, sama) of a declared WeightedCEMLP inner problem: ``provider.finite_difference``
(betty_amd/hypergradient/structured.py), on the ATen twin with the checker backend (CPU) and on the HIP kernels of csrc/bhg_fd.hip (GPU).

Same cases and goldens as the opaque path (tests/golden/<family>.npz from the reference's own darts.py / sama.py): the result at the
case's rtol, the inner weights after the call at the opaque path's perturb / restore drift."""
import os
import sys

import numpy as np
import pytest
import torch

import zoo
from _cpu_checker_backend import CpuCheckerBackend
from conftest import golden_list, load_golden, rel_err

from betty_amd import Config
from betty_amd import hypergradient as hg
from betty_amd.backend import use_backend

FD_CASES = ["reweight_darts", "reweight_darts_multitask", "deep_darts", "reweight_sama_adam"]


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
    """The native hop never calls the user's training_step: make any call to it fail loudly."""
    def boom(batch):
        raise AssertionError("the opaque path ran: training_step_exec was called")

    curr.training_step_exec = boom


def _declare(curr, family, impl, weight_net, verify=True):
    from betty_amd.hypergradient.structured import SigmoidMLPWeightNet, WeightedCEMLP

    def structure(prev):
        return WeightedCEMLP(curr, prev, layers=list(curr.module.layers), weight_fn=lambda ce: prev.fwd(ce.reshape(-1, 1)),
                             ridge=zoo.RIDGE[family], impl=impl, verify=verify,
                             weight_net=SigmoidMLPWeightNet(prev.module.l1, prev.module.l2) if weight_net else None)

    curr.hypergradient_structure = structure
    return curr


def _check_against_golden(case, curr, prev, vector, sync, outputs):
    if sync:
        for p in prev.trainable_parameters():
            p.grad = torch.full_like(p, 0.25)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, sync)
    if sync:
        assert out is None
        got = [p.grad.detach().cpu().numpy() - 0.25 for p in prev.trainable_parameters()]
        want = golden_list(outputs, case.name, "sync32")
        rel, _ = rel_err(got, want)
        scale = max(1.0, 0.25 / max(np.abs(np.concatenate([w.ravel() for w in want])).max(), 1e-30))
        assert rel <= case.rtol * scale + 1e-6 * scale, rel
    else:
        want = golden_list(outputs, case.name, "fp32")
        assert len(out) == len(want)
        rel, mx = rel_err([o.detach().cpu().numpy() for o in out], want)
        assert rel <= case.rtol and mx <= 10 * case.rtol, (rel, mx)
    # the weights the reference leaves behind: restored up to its own drift, or w- under *_multitask
    for p, w in zip(curr.trainable_parameters(), golden_list(outputs, case.name, "w32")):
        np.testing.assert_allclose(p.data.cpu().numpy(), w, rtol=0, atol=2e-7)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the ATen twin (impl="torch") with the checker backend
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("name", FD_CASES)
def test_aten_twin_matches_reference(name, sync, checker):
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config)
    _declare(curr, case.family, "torch", weight_net=False)
    _check_against_golden(case, curr, prev, vector, sync, outputs)


@pytest.mark.parametrize("name", ["reweight_darts", "reweight_sama_adam"])
def test_aten_twin_takes_the_structure_not_the_training_step(name, checker):
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config)
    _declare(curr, case.family, "torch", weight_net=False, verify=False)
    _forbid_training_step(curr)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    rel, _ = rel_err([o.detach().numpy() for o in out], golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol, rel


def test_structure_guard_runs_before_the_first_hop_and_is_shared(checker):
    from betty_amd.hypergradient import structured

    case = zoo.CASE_BY_NAME["reweight_darts"]
    inputs, _ = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config)
    _declare(curr, case.family, "torch", weight_net=False)
    calls = []
    real = structured.WeightedCEMLP._autograd_second_order   # the double backward of the check

    def spy(self, params, upper):
        calls.append(1)
        return real(self, params, upper)

    structured.WeightedCEMLP._autograd_second_order = spy
    try:
        hg.darts(vector, curr, prev, False)
        hg.darts(vector, curr, prev, False)
        assert len(calls) == 1   # verdict cached on the problem
        curr.hypergradient_structure(prev).prepare()   # ... and shared with prepare() (cg / neumann)
        assert len(calls) == 1
    finally:
        structured.WeightedCEMLP._autograd_second_order = real


def test_structure_guard_rejects_a_wrong_declaration(checker):
    from betty_amd.hypergradient.structured import StructureMismatchError

    case = zoo.CASE_BY_NAME["reweight_darts"]
    inputs, _ = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config)
    _declare(curr, case.family, "torch", weight_net=False)
    real = curr.hypergradient_structure
    curr.hypergradient_structure = lambda p: (lambda s: (setattr(s, "ridge", 0.0), setattr(s, "hvp_shift", 0.0), s)[-1])(real(p))
    with pytest.raises(StructureMismatchError):
        hg.darts(vector, curr, prev, False)


def test_fallback_conditions_reach_the_opaque_path(checker):
    """A foreign upper parameter (declared weight net), FSDP and a non-fp32 problem keep the opaque path, unchanged."""
    case = zoo.CASE_BY_NAME["reweight_darts"]
    inputs, outputs = load_golden(case.family)
    want = golden_list(outputs, case.name, "fp32")
    ran = []

    def variant(mutate):
        curr, prev, vector = zoo.build_case(case, inputs, Config)
        _declare(curr, case.family, "torch", weight_net=True, verify=False)
        mutate(curr, prev)
        real = curr.training_step_exec

        def counted(batch):
            ran.append(1)
            return real(batch)

        curr.training_step_exec = counted
        return curr, prev, vector

    # an extra upper parameter the declared weight net does not own
    extra = torch.nn.Parameter(torch.zeros(3))

    def foreign(curr, prev):
        params = list(prev.module.parameters()) + [extra]
        prev.trainable_parameters = lambda: params

    curr, prev, vector = variant(foreign)
    out = hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    rel, _ = rel_err([o.detach().numpy() for o in out[:4]], want)
    assert rel <= case.rtol and float(out[4].abs().max()) == 0.0

    ran.clear()
    curr, prev, vector = variant(lambda c, p: None)
    wn = curr.hypergradient_structure(prev).weight_net
    curr.hypergradient_structure = (lambda real: (lambda p: (lambda s: (setattr(s.weight_net, "average_over", True), s)[-1])(real(p))))(
        curr.hypergradient_structure)
    hg.darts(vector, curr, prev, False)
    assert wn is not None and len(ran) == 2   # a collective is declared: opaque path

    ran.clear()   # the upper forward is a DistributedDataParallel wrapper (its reducer would take the mean)
    curr, prev, vector = variant(lambda c, p: setattr(p, "fwd", _UnsyncedDDP(p.module)))
    out = hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    rel, _ = rel_err([o.detach().numpy() for o in out], want)
    assert rel <= case.rtol


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the HIP kernels (csrc/bhg_fd.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def _gpu_case(name, weight_net, verify=True, impl="hip"):
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden(case.family)
    curr, prev, vector = zoo.build_case(case, inputs, Config, device="cuda")
    if impl is not None:
        _declare(curr, case.family, impl, weight_net=weight_net, verify=verify)
    return case, outputs, curr, prev, vector


@pytest.mark.gpu
@pytest.mark.parametrize("weight_net", [True, False], ids=["mwn", "weight_fn"])
@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("name", FD_CASES)
def test_hip_matches_reference(name, sync, weight_net):
    case, outputs, curr, prev, vector = _gpu_case(name, weight_net)
    _check_against_golden(case, curr, prev, vector, sync, outputs)


@pytest.mark.gpu
@pytest.mark.parametrize("weight_net", [True, False], ids=["mwn", "weight_fn"])
@pytest.mark.parametrize("name", FD_CASES)
def test_hip_takes_the_native_hop(name, weight_net):
    """verify=False and a training_step that raises: only the native hop can succeed."""
    case, outputs, curr, prev, vector = _gpu_case(name, weight_net, verify=False)
    _forbid_training_step(curr)
    out = hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    rel, _ = rel_err([o.detach().cpu().numpy() for o in out], golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol, rel


@pytest.mark.gpu
@pytest.mark.parametrize("weight_net", [True, False], ids=["mwn", "weight_fn"])
@pytest.mark.parametrize("name", FD_CASES)
def test_hip_weights_bit_identical_to_the_opaque_path(name, weight_net):
    """Same structure-free problem, same eps: the native hop leaves exactly the weights the three axpys leave."""
    case, _, curr, prev, vector = _gpu_case(name, weight_net)
    _, _, curr_o, prev_o, vector_o = _gpu_case(name, weight_net, impl=None)
    hg.jvp_fn_mapping[case.algo](vector, curr, prev, False)
    hg.jvp_fn_mapping[case.algo](vector_o, curr_o, prev_o, False)
    for a, b in zip(curr.trainable_parameters(), curr_o.trainable_parameters()):
        assert torch.equal(a.data, b.data)


@pytest.mark.gpu
@pytest.mark.parametrize("weight_net", [True, False], ids=["mwn", "weight_fn"])
def test_hip_sync_accumulates_on_a_prefilled_grad(weight_net):
    case, _, curr, prev, vector = _gpu_case("reweight_darts", weight_net)
    out = [o.clone() for o in hg.darts(vector, curr, prev, False)]
    case, _, curr, prev, vector = _gpu_case("reweight_darts", weight_net)
    fill = [torch.randn_like(p) for p in prev.trainable_parameters()]
    for p, f in zip(prev.trainable_parameters(), fill):
        p.grad = f.clone()
    assert hg.darts(vector, curr, prev, True) is None
    got = [p.grad - f for p, f in zip(prev.trainable_parameters(), fill)]
    want = [o.cpu().numpy() for o in out]
    rel, _ = rel_err([g.cpu().numpy() for g in got], want)
    # (the pre-fill's own rounding is what the difference carries: the bound of test_host_logic's sync test, scaled by |fill|)
    scale = max(1.0, max(float(f.abs().max()) for f in fill) / max(np.abs(np.concatenate([w.ravel() for w in want])).max(), 1e-30))
    assert rel <= case.rtol * scale + 1e-6 * scale, (rel, scale)


@pytest.mark.gpu
def test_hip_cfg2_scale_agrees_with_the_opaque_path():
    """bench.build's shapes (10 M inner parameters), seed 0: within 2x of the opaque fp32 result's own distance to an fp64 truth (2e-3
    floor), the rule of test_gpu_parity.py::test_cfg4_roberta_scale_darts."""
    import bench

    dev = torch.device("cuda")
    curr, prev, vector = bench.build(dev, seed=0, algo="darts")
    w0 = [p.data.clone() for p in curr.parameters()]
    u0 = [p.data.clone() for p in prev.module.parameters()]
    want = [t.clone() for t in hg.darts(vector, curr, prev, False)]   # opaque (no structure declared)
    w_opaque = [p.data.clone() for p in curr.parameters()]
    for p, w in zip(curr.parameters(), w0):
        p.data.copy_(w)
    bench.declare_structure(curr, "hip")
    got = [t.clone() for t in hg.darts(vector, curr, prev, False)]
    for a, b in zip(curr.parameters(), w_opaque):
        assert torch.equal(a.data, b)
    # truth: the reference's algorithm in fp64 (oracle/hypergrad_oracle.py restates darts.py on plain torch)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import hypergrad_oracle as horc

    curr64, prev64, _ = bench.build(dev, seed=0, algo="darts", dtype=torch.float64)
    for p, w in zip(curr64.parameters(), w0):
        p.data.copy_(w.double())
    for p, u in zip(prev64.module.parameters(), u0):
        p.data.copy_(u.double())
    truth = [t.detach().clone() for t in horc.darts([v.double() for v in vector], curr64, prev64, False)]
    del curr64, prev64
    np_ = lambda ts: [t.detach().double().cpu().numpy() for t in ts]
    e_ref, _ = rel_err(np_(want), np_(truth))
    e_got, _ = rel_err(np_(got), np_(truth))
    rel, _ = rel_err(np_(got), np_(want))
    print(f"cfg2 darts vs fp64 truth: opaque {e_ref:.2e}, native {e_got:.2e}; native vs opaque {rel:.2e}")
    assert rel <= max(2e-3, e_ref), (rel, e_ref)
    assert e_got <= max(2e-3, 2.0 * e_ref), (e_got, e_ref)


@pytest.mark.gpu
def test_hip_fallbacks_reach_the_opaque_path():
    """A DDP-wrapped upper forward and a foreign upper parameter keep the opaque path (training_step runs twice)."""
    import os

    import torch.distributed as dist

    ran = []

    def counting(curr):
        real = curr.training_step_exec

        def counted(batch):
            ran.append(1)
            return real(batch)

        curr.training_step_exec = counted

    case, outputs, curr, prev, vector = _gpu_case("reweight_darts", weight_net=True, verify=False)
    extra = torch.nn.Parameter(torch.zeros(3, device="cuda"))
    params = list(prev.module.parameters()) + [extra]
    prev.trainable_parameters = lambda: params
    counting(curr)
    out = hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    rel, _ = rel_err([o.detach().cpu().numpy() for o in out[:4]], golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol, rel

    ran.clear()
    case, outputs, curr, prev, vector = _gpu_case("reweight_darts", weight_net=False, verify=False)
    prev.fwd = _UnsyncedDDP(prev.module)
    counting(curr)
    out = hg.darts(vector, curr, prev, False)
    assert len(ran) == 2
    rel, _ = rel_err([o.detach().cpu().numpy() for o in out], golden_list(outputs, case.name, "fp32"))
    assert rel <= case.rtol, rel

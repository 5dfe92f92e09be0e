"""bhg_layernorm_backward_vjp (csrc/bhg_layernorm.hip: k_ln_vjp_rows + k_ln_vjp_combine) through the C ABI against the float64 restatement
tests/layernorm_ref.py, array by array, on the smallest shapes at which the kernels can still go wrong: one element; every width at
which the row pass takes another path (scalar / 16-byte accesses, one row per workgroup or several side by side, 2 / 4 / 8 resp.
2 / 8 / 32 vectors per thread) at M = 7; one row; a ragged last row group; one below / at / one above the rows-per-workgroup edge and
the 64-slice bound the plan reports; the bound taking hold (4097 x 64); RoBERTa's 800 x 768; a far mean (x = 100 + 0.01 N(0, 1)); one
row whose x is 1e3 and whose gy, a are 1e-4 times its neighbours' (a leak between rows would show).  Each case with all pointers given,
a NULL, gamma NULL (affine off: b, c and dgamma NULL as well), b and c NULL, and c alone NULL.  Each case first reads the plan and
asserts the regime it is named for.

The restatement is evaluated on the very fp32 mean / rstd the kernel reads.  Outputs and workspace are slices of sentinel-filled
buffers: they must be written inside their bounds only, and everywhere inside; a NULL output's buffer stays untouched; the inputs are
bit-equal afterwards; a second run on a NaN-filled workspace gives the same bits.

Gate, per row of dx and dgy: max|got - want| <= 2e-5 max|want_row| — the project's gate for fp32 kernels against fp64 restatements
(DESIGN 3.28).  Per column of dgamma: |got - want| <= 2e-5 sum_i |gy_ij r_i at_ij|, the sum of the absolute terms, so that cancellation
in a column cannot fail a correct kernel.  test_the_gate_can_exclude_no_case (CPU) shows that the restatement rounded to fp32 passes every
case.  Observed maxima on one MI355X: profiles/layernorm_fp64.txt."""
import functools

import pytest
import torch

import layernorm_ref
from betty_amd import _native
from betty_amd.backend import layernorm_plan

DEV = "cuda:0"
GATE = 2e-5
EPS = 1e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["all", "no_a", "no_gamma", "no_bc", "no_c"]

# (label, M, D, variant)
ONE = ("one element", 1, 1, "plain")
WIDTHS = [("width", 7, d, "plain") for d in (3, 4, 5, 63, 64, 65, 768, 1000, 8188, 8192)]
ONE_ROW = [("one row", 1, 5, "plain"), ("one row", 1, 768, "plain")]
RAGGED = ("ragged last group", 70, 64, "plain")                                   # 32 rows side by side: groups of 32, 32, 6
ROWS_EDGE = [("rows edge", m, 64, "plain") for m in (31, 32, 33)]                # rows per workgroup = 32 at D = 64 (asserted below)
SLICE_EDGE = [("slice edge", m, 64, "plain") for m in (2047, 2048, 2049)]        # 64 row groups of 32 rows: the bound of 64 slices
SLICE_EDGE_WIDE = [("slice edge, one row per group", m, 4096, "plain") for m in (63, 64, 65)]
SLICE_CAP = ("slice bound", 4097, 64, "plain")                                    # 129 row groups: 43 slices of 3
ROBERTA = ("roberta", 800, 768, "plain")
FAR_MEAN = [("far mean", 7, 768, "far_mean"), ("far mean", 70, 64, "far_mean"), ("far mean", 7, 1000, "far_mean")]
LEAK = [("leak", 7, 768, "leak"), ("leak", 70, 64, "leak"), ("leak", 7, 1000, "leak")]
CASES = [ONE] + WIDTHS + ONE_ROW + [RAGGED] + ROWS_EDGE + SLICE_EDGE + SLICE_EDGE_WIDE + [SLICE_CAP, ROBERTA] + FAR_MEAN + LEAK
_id = lambda c: f"{c[0].replace(' ', '_').replace(',', '')}-{c[1]}x{c[2]}" if isinstance(c, tuple) else c   # noqa: E731


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(x, gy, a, gamma, mean, rstd, b, c) on the host, fp32; computed once per case, shared, never written.  mean and rstd are the
    float64 statistics of the fp32 x, rounded to fp32: what the kernel reads and what the restatement is evaluated on."""
    _, M, D, variant = case
    g = torch.Generator().manual_seed((M * 8209 + D) * 3 + len(variant))
    x, gy, a = (torch.randn(M, D, generator=g) for _ in range(3))
    gamma, b, c = (torch.randn(D, generator=g) for _ in range(3))
    if variant == "far_mean":
        x = 100.0 + 0.01 * x
    if variant == "leak":
        row = M // 2
        x[row] *= 1e3
        gy[row] *= 1e-4
        a[row] *= 1e-4
    mean, rstd = layernorm_ref.stats(x.double(), EPS)
    return x, gy, a, gamma, mean.float(), rstd.float(), b, c


def present(mode):
    """Which of (a, gamma, b, c) the call is given."""
    return {"all": (True, True, True, True), "no_a": (False, True, True, True), "no_gamma": (True, False, False, False),
            "no_bc": (True, True, False, False), "no_c": (True, True, True, False)}[mode]


@functools.lru_cache(maxsize=None)
def wanted(case, mode):
    """(dx, dgy, dgamma or None, the absolute terms of dgamma or None) in float64."""
    x, gy, a, gamma, mean, rstd, b, c = (t.double() for t in host_inputs(case))
    ha, hg, hb, hc = present(mode)
    a, gamma, b, c = (a if ha else None), (gamma if hg else None), (b if hb else None), (c if hc else None)
    dx, dgy, dgamma = layernorm_ref.layernorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c)
    return dx, dgy, dgamma, (layernorm_ref.dgamma_abs_terms(x, gy, a, gamma, mean, rstd) if hg else None)


def gate(case, mode, got, label="case"):
    """Assert the gate on (dx, dgy, dgamma) and print the observed maxima; `got` are host tensors (dgamma None when gamma is)."""
    dx, dgy, dgamma, terms = wanted(case, mode)
    line = []
    for name, g, want in (("dx", got[0], dx), ("dgy", got[1], dgy)):
        err = (g.double() - want).abs().amax(dim=1)
        scale = want.abs().amax(dim=1)
        assert bool((err <= GATE * scale).all()), (label, case, mode, name, float((err / scale.clamp_min(1e-300)).max()))
        live = scale > 0
        line.append(f"{name} {float((err[live] / scale[live]).max()) if bool(live.any()) else 0.0:.3e}")
    assert (got[2] is None) == (dgamma is None)
    if dgamma is not None:
        err = (got[2].double() - dgamma).abs()
        assert bool((err <= GATE * terms).all()), (label, case, mode, "dgamma", float((err / terms.clamp_min(1e-300)).max()))
        live = terms > 0
        line.append(f"dgamma {float((err[live] / terms[live]).max()) if bool(live.any()) else 0.0:.3e}")
    print(f"layernorm_vjp {label} {_id(case)} {mode}: " + "  ".join(line) + "  (worst row of max|got - want| / max|want_row|; dgamma: / sum|terms|)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    for mode in MODES:
        dx, dgy, dgamma, _ = wanted(case, mode)
        gate(case, mode, (dx.float(), dgy.float(), None if dgamma is None else dgamma.float()), label="fp64 rounded to fp32")


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    return tuple(t.to(DEV) for t in host_inputs(case))


def _padded(numel, dtype=torch.float32):
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    inner.fill_(float("nan"))
    return buf, inner


def _outside_untouched(buf, numel):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + numel:] == SENTINEL).all())


def run_vjp(case, mode):
    """One call on buffers this function owns.  Returns (dx, dgy, dgamma or None) on the host after checking the bounds of every write,
    that every element inside was written, that a NULL output's buffer and the unused part of the workspace are untouched, and that
    the inputs are unchanged."""
    lib = _native.load()
    _, M, D, _ = case
    ins = device_inputs(case)
    before = [t.clone() for t in ins]
    x, gy, a, gamma, mean, rstd, b, c = ins
    ha, hg, hb, hc = present(mode)
    ws_bytes = int(lib.bhg_layernorm_ws_bytes(D))
    assert ws_bytes == 8 * 64 * D
    used = layernorm_plan(M, D)["ws"] // 8 if hg else 0
    wsbuf, ws = _padded(ws_bytes // 8, torch.float64)
    dxbuf, dx = _padded(M * D)
    dgybuf, dgy = _padded(M * D)
    dgbuf, dgamma = _padded(D)
    ptr = lambda t, on=True: t.data_ptr() if on else None   # noqa: E731
    rc = lib.bhg_layernorm_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a, ha), ptr(gamma, hg), mean.data_ptr(), rstd.data_ptr(), ptr(b, hb),
                                        ptr(c, hc), M, D, dx.data_ptr(), dgy.data_ptr(), ptr(dgamma, hg), ws.data_ptr(), ws_bytes,
                                        int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_layernorm_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
    for name, buf, t in (("dx", dxbuf, dx), ("dgy", dgybuf, dgy), ("dgamma", dgbuf, dgamma), ("ws", wsbuf, ws)):
        assert _outside_untouched(buf, t.numel()), f"write outside {name}"
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dgy).all()), "an element of dx / dgy was not written (or a stale value was read)"
    assert bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all()), "the workspace: written where the plan says, nowhere else"
    if hg:
        assert bool(torch.isfinite(dgamma).all()), "an element of dgamma was not written (or a stale partial sum was read)"
    else:
        assert bool(torch.isnan(dgamma).all()), "dgamma was not given: its buffer must stay untouched"
    return dx.view(M, D).cpu(), dgy.view(M, D).cpu(), (dgamma.cpu() if hg else None)


def assert_regime(case):
    label, M, D, _ = case
    plan = layernorm_plan(M, D)
    assert plan["vec"] == (4 if D % 4 == 0 else 1), plan
    if case == ONE:
        assert (plan["tpr"], plan["rows"], plan["nv"], plan["slices"]) == (1, 256, 1, 1), plan
    if label == "width":
        want = {3: (1, 2, 2, 2), 4: (4, 1, 1, 2), 5: (1, 4, 2, 2), 63: (1, 32, 2, 2), 64: (4, 8, 2, 2), 65: (1, 64, 2, 2), 768: (4, 128, 2, 2),
                1000: (4, 128, 2, 2), 8188: (4, 256, 8, 8), 8192: (4, 256, 8, 8)}[D]
        assert (plan["vec"], plan["tpr"], plan["nv"], plan["inst"]) == want and plan["groups"] == -(-7 // plan["rows"]), plan
    if label == "one row":
        assert plan["groups"] == plan["slices"] == 1 and plan["rows"] > 1, plan
    if case == RAGGED:
        assert (plan["rows"], plan["groups"], plan["slices"]) == (32, 3, 3), plan
    if label == "rows edge":
        assert plan["rows"] == 32 and plan["groups"] == {31: 1, 32: 1, 33: 2}[M], plan
    if label == "slice edge":
        assert plan["rows"] == 32 and (plan["groups"], plan["gps"], plan["slices"]) == {2047: (64, 1, 64), 2048: (64, 1, 64), 2049: (65, 2, 33)}[M], plan
    if label.startswith("slice edge, one row"):
        assert plan["rows"] == 1 and plan["inst"] == 4 and (plan["groups"], plan["gps"], plan["slices"]) == {63: (63, 1, 63), 64: (64, 1, 64), 65: (65, 2, 33)}[M], plan
    if case == SLICE_CAP:
        assert (plan["groups"], plan["gps"], plan["slices"], plan["max_slices"]) == (129, 3, 43, 64), plan
    if case == ROBERTA:
        assert (plan["tpr"], plan["rows"], plan["groups"], plan["gps"], plan["slices"]) == (128, 2, 400, 7, 58), plan


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_case_sits_in_the_regime_it_is_named_for(case):
    assert_regime(case)


def test_the_scalar_instances_with_8_and_32_vectors_are_covered_too():
    """The widths the issue lists reach the scalar path with two vectors per thread only; 1001 and 8191 take its other two instances
    (they run in test_kernels_match_the_fp64_restatement through EXTRA)."""
    assert [layernorm_plan(7, d)["inst"] for d in (1001, 8191)] == [8, 32] and layernorm_plan(7, 8191)["vec"] == 1


EXTRA = [("scalar instances", 7, 1001, "plain"), ("scalar instances", 7, 8191, "plain"), ("four vectors", 7, 2052, "plain")]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES + EXTRA, ids=_id)
def test_kernels_match_the_fp64_restatement(case, mode):
    assert_regime(case)
    first = run_vjp(case, mode)
    gate(case, mode, first)
    if case == ONE:
        assert not first[0].any()                                  # xh = 0: dx = 0
    again = run_vjp(case, mode)                                     # fresh NaN-filled workspace and outputs: the same bits
    for name, u, v in zip(("dx", "dgy", "dgamma"), first, again):
        assert (u is None and v is None) or torch.equal(u, v), name


@pytest.mark.gpu
@pytest.mark.parametrize("big,small", [(SLICE_CAP, RAGGED), (ROBERTA, WIDTHS[6]), (SLICE_EDGE_WIDE[2], WIDTHS[7])], ids=lambda c: _id(c))
def test_two_consecutive_calls_on_one_workspace_the_larger_first(big, small):
    """The second call's slices are fewer than the first's: what the first left in the workspace must not reach the second's dgamma.
    The pair runs back to back on one workspace, filled with NaN once."""
    lib = _native.load()
    ws = torch.full((lib.bhg_layernorm_ws_bytes(max(big[2], small[2])) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    assert layernorm_plan(*big[1:3])["ws"] > layernorm_plan(*small[1:3])["ws"]
    outs = []
    for case in (big, small):
        _, M, D, _ = case
        x, gy, a, gamma, mean, rstd, b, c = device_inputs(case)
        dx, dgy, dgamma = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.full_like(gamma, float("nan"))
        rc = lib.bhg_layernorm_backward_vjp(x.data_ptr(), gy.data_ptr(), a.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            b.data_ptr(), c.data_ptr(), M, D, dx.data_ptr(), dgy.data_ptr(), dgamma.data_ptr(), ws.data_ptr(),
                                            ws.numel() * 8, int(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "bhg_layernorm_backward_vjp")
        outs.append((dx, dgy, dgamma))
    torch.cuda.synchronize()
    for case, got in zip((big, small), outs):
        gate(case, "all", tuple(t.cpu() for t in got), label="shared workspace")

"""bhg_rmsnorm_backward_vjp (csrc/bhg_rmsnorm.hip: k_rms_vjp_rows + k_rms_vjp_combine) through the C ABI against the float64 restatement
tests/rmsnorm_ref.py, array by array, on the smallest shapes at which the kernels can still go wrong.  Cases are (M, D): one element;
rows of 2, 3, 9 (scalar accesses), 12 and 16 (16-byte accesses) elements; D = 63, 64, 65 with two rows; D = 1000; one shape per kernel
instance (2, 4, 8 vectors per thread; 2, 8, 32 scalars), read off the plan; the bound D = 8188 and 8192; one below / at / one above the
rows-per-workgroup edge the plan reports at D = 8, with a ragged last row group; enough rows at D = 8 that the slice cap is hit, with
several row groups per slice and a ragged last slice; 600 x 260.  Variants: plain; eps_dominates (x = 1e-4 N(0, 1) with eps = 1e-5: mean
xh^2 is about 1e-3, not 1); leak (one row whose x is 1e3 and whose gy, a are 1e-4 times its neighbours': a leak between rows would
show); torch's default eps (finfo(float32).eps).  Each case with all pointers given, a NULL, gamma NULL (b, dgamma and the workspace NULL
as well), b NULL, and dgamma NULL (the workspace given: it must stay untouched).  Each case first reads the plan and asserts the regime
it is named for.

The restatement is evaluated on the very fp32 rstd the kernel reads.  Outputs and workspace are slices of sentinel-filled buffers: they
must be written inside their bounds only, and everywhere inside; a NULL output's buffer stays untouched; the inputs are bit-equal
afterwards; a second run on NaN-filled outputs and workspace gives the same bits.

Gate, per row of dx and dgy for D >= 2: max|got - want| <= 2e-5 max|want_row| — the project's gate for fp32 kernels against fp64
restatements.  A one-element row needs another scale, and so does dgamma for every D: at D = 1, dx and dgamma are
differences of nearly equal terms (1 - xh^2 = eps r^2), so the scale there is the sum of the absolute terms — r (|q| + |xh mqx| + |xh t|)
for dx, |gamma r| (|a| + |xh A1|) + |b xh| for dgy, sum_i |gy r| (|a| + |xh A1|) per column for dgamma — and against those the same 2e-5
holds.  test_the_gate_can_exclude_no_case (CPU) shows that the restatement rounded to fp32 passes every case and mode and that every
denominator is positive.  Observed maxima on one MI355X: profiles/rmsnorm_fp64.txt."""
import functools

import pytest
import torch

import rmsnorm_ref
from betty_amd import _native
from betty_amd.backend import rmsnorm_plan

DEV = "cuda:0"
GATE = 2e-5
EPS = 1e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["all", "no_a", "no_gamma", "no_b", "no_dgamma"]

# (label, M, D, variant)
ONE = ("one element", 1, 1, "plain")
SHORT = [("D=2 scalar", 3, 2, "plain"), ("D=3 scalar", 2, 3, "plain"), ("D=9 scalar", 5, 9, "plain"), ("D=12 vector", 3, 12, "plain"),
         ("D=16 vector", 2, 16, "plain")]
WAVE = [("around one wave of columns", 2, d, "plain") for d in (63, 64, 65)]
D1000 = ("D=1000", 4, 1000, "plain")
INSTANCES = [("vector instance 2", 3, 2048, "plain"), ("vector instance 4", 3, 2052, "plain"), ("vector instance 8", 3, 4100, "plain"),
             ("scalar instance 2", 3, 510, "plain"), ("scalar instance 8", 3, 1001, "plain"), ("scalar instance 32", 3, 2049, "plain")]
BOUND = [("bound D=8188", 2, 8188, "plain"), ("bound D=8192", 2, 8192, "plain")]
ROWS_EDGE = [("rows edge 255", 255, 8, "plain"), ("rows edge 256", 256, 8, "plain"), ("rows edge 257 ragged", 257, 8, "plain")]
CAPPED = ("cap hit ragged last slice", 256 * 2052 + 5, 8, "plain")   # 2053 row groups of 256 rows, the last of 5: above the cap of 1024 slices
GRID = ("600 x 260", 600, 260, "plain")
EPS_DOMINATES = [("eps dominates", 1, 1, "eps_dominates"), ("eps dominates", 5, 9, "eps_dominates"), ("eps dominates", 4, 1000, "eps_dominates"),
                 ("eps dominates", 2, 8192, "eps_dominates")]
LEAK = [("leak", 5, 9, "leak"), ("leak", 4, 1000, "leak"), ("leak", 3, 4100, "leak"), ("leak", 257, 8, "leak")]
DEFAULT_EPS = [("default eps", 1, 1, "default_eps"), ("default eps", 5, 9, "default_eps"), ("default eps", 4, 1000, "default_eps")]
CASES = [ONE] + SHORT + WAVE + [D1000] + INSTANCES + BOUND + ROWS_EDGE + [CAPPED, GRID] + EPS_DOMINATES + LEAK + DEFAULT_EPS


def _id(c):
    return f"{c[0].replace(' ', '_')}-{c[1]}x{c[2]}" if isinstance(c, tuple) else c


def dims(case):
    return case[1], case[2]


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(x, gy, a, gamma, rstd, b) on the host, fp32; computed once per case, shared, never written.  rstd is the float64 statistic of the
    fp32 x, rounded to fp32: what the kernel reads and what the restatement is evaluated on."""
    M, D = dims(case)
    g = torch.Generator().manual_seed((M * 8209 + D) * 7 + len(case[3]))
    x, gy, a = (torch.randn(M, D, generator=g) for _ in range(3))
    gamma, b = (torch.randn(D, generator=g) for _ in range(2))
    eps = EPS
    if case[3] == "eps_dominates":
        x = 1e-4 * x
    if case[3] == "default_eps":
        eps = None
    if case[3] == "leak":
        for t, f in ((x, 1e3), (gy, 1e-4), (a, 1e-4)):
            t[M // 2] *= f
    rstd = rmsnorm_ref.stats(x.double(), torch.finfo(torch.float32).eps if eps is None else eps)
    return x, gy, a, gamma, rstd.float(), b


def present(mode):
    """Which of (a, gamma, b, dgamma, ws) the call is given."""
    return {"all": (True, True, True, True, True), "no_a": (False, True, True, True, True), "no_gamma": (True, False, False, False, False),
            "no_b": (True, True, False, True, True), "no_dgamma": (True, True, True, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def wanted(case, mode):
    """(dx, dgy, dgamma or None) and the scales (per row of dx, per row of dgy, per column of dgamma or None), all in float64."""
    M, D = dims(case)
    x, gy, a, gamma, rstd, b = (t.double() for t in host_inputs(case))
    ha, hg, hb, hd, _ = present(mode)
    a, gamma, b = (a if ha else None), (gamma if hg else None), (b if hb else None)
    dx, dgy, dgamma = rmsnorm_ref.rmsnorm_backward_vjp(x, gy, a, gamma, rstd, b)
    if D >= 2:
        sdx, sdgy = dx.abs().amax(dim=1), dgy.abs().amax(dim=1)
    else:
        tx, tgy = rmsnorm_ref.elementwise_abs_terms(x, gy, a, gamma, rstd, b)
        sdx, sdgy = tx.amax(dim=1), tgy.amax(dim=1)
    terms = rmsnorm_ref.dgamma_abs_terms(x, gy, a, rstd) if hd else None
    return dx, dgy, (dgamma if hd else None), sdx, sdgy, terms


def gate(case, mode, got, label="case"):
    """Assert the gate on (dx, dgy, dgamma) and print the observed maxima; `got` are host tensors (dgamma None when not wanted)."""
    M, D = dims(case)
    dx, dgy, dgamma, sdx, sdgy, terms = wanted(case, mode)
    line = []
    for name, g, want, scale in (("dx", got[0], dx, sdx), ("dgy", got[1], dgy, sdgy)):
        err = (g.double().reshape(M, D) - want).abs().amax(dim=1)
        assert bool((err <= GATE * scale).all()), (label, case, mode, name, float((err / scale.clamp_min(1e-300)).max()))
        live = scale > 0
        line.append(f"{name} {float((err[live] / scale[live]).max()) if bool(live.any()) else 0.0:.3e}")
    assert (got[2] is None) == (dgamma is None)
    if dgamma is not None:
        err = (got[2].double() - dgamma).abs()
        assert bool((err <= GATE * terms).all()), (label, case, mode, "dgamma", float((err / terms.clamp_min(1e-300)).max()))
        live = terms > 0
        line.append(f"dgamma {float((err[live] / terms[live]).max()) if bool(live.any()) else 0.0:.3e}")
    print(f"rmsnorm_vjp {label} {_id(case)} {case[3]} {mode}: " + "  ".join(line)
          + "  (worst row of max|got - want| / " + ("max|want_row|" if D >= 2 else "sum|terms|") + "; dgamma: / sum|terms|)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    """The restatement rounded to fp32 passes every case and mode; and the gate's denominators are positive, so that it asks something of
    every row and column — except where the result is zero by the mathematics, where the gate asks for exactly zero: dgamma without a
    (at = 0)."""
    for mode in MODES:
        dx, dgy, dgamma, sdx, sdgy, terms = wanted(case, mode)
        gate(case, mode, (dx.float(), dgy.float(), None if dgamma is None else dgamma.float()), label="fp64 rounded to fp32")
        assert bool((sdx > 0).all()) and bool((sdgy > 0).all()), (case, mode)
        if terms is not None and mode != "no_a":
            assert bool((terms > 0).all()), (case, mode)


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
    that every element inside was written, that a NULL output's buffer and an unwanted workspace are untouched, and that the inputs are
    unchanged."""
    lib = _native.load()
    M, D = dims(case)
    ins = device_inputs(case)
    before = [t.clone() for t in ins]
    x, gy, a, gamma, rstd, b = ins
    ha, hg, hb, hd, hw = present(mode)
    plan = rmsnorm_plan(M, D)
    ws_bytes = int(lib.bhg_rmsnorm_ws_bytes(M, D))
    assert ws_bytes == 8 * plan["slices"] * D == plan["ws"]
    wsbuf, ws = _padded(ws_bytes // 8, torch.float64)
    dxbuf, dx = _padded(x.numel())
    dgybuf, dgy = _padded(x.numel())
    dgbuf, dgamma = _padded(D)
    ptr = lambda t, on=True: t.data_ptr() if on else None   # noqa: E731
    rc = lib.bhg_rmsnorm_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a, ha), ptr(gamma, hg), rstd.data_ptr(), ptr(b, hb), M, D,
                                      dx.data_ptr(), dgy.data_ptr(), ptr(dgamma, hd), ptr(ws, hw), ws_bytes if hw else 0,
                                      int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_rmsnorm_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t, t0), "an input was modified"
    for name, buf, t in (("dx", dxbuf, dx), ("dgy", dgybuf, dgy), ("dgamma", dgbuf, dgamma), ("ws", wsbuf, ws)):
        assert _outside_untouched(buf, t.numel()), f"write outside {name}"
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dgy).all()), "an element of dx / dgy was not written (or a stale value was read)"
    if hd:
        assert bool(torch.isfinite(ws).all()), "the workspace: every partial the plan names is written"
        assert bool(torch.isfinite(dgamma).all()), "an element of dgamma was not written (or a stale partial sum was read)"
    else:
        assert bool(torch.isnan(ws).all()), "dgamma was not given: the workspace must stay untouched"
        assert bool(torch.isnan(dgamma).all()), "dgamma was not given: its buffer must stay untouched"
    return dx.cpu(), dgy.cpu(), (dgamma.cpu() if hd else None)


def assert_regime(case):
    label = case[0]
    M, D = dims(case)
    plan = rmsnorm_plan(M, D)
    want = {  # D: (vec, tpr, rows, inst)
        1: (1, 1, 256, 2), 2: (1, 1, 256, 2), 3: (1, 2, 128, 2), 9: (1, 8, 32, 2), 12: (4, 2, 128, 2), 16: (4, 2, 128, 2),
        63: (1, 32, 8, 2), 64: (4, 8, 32, 2), 65: (1, 64, 4, 2), 1000: (4, 128, 2, 2), 2048: (4, 256, 1, 2), 2052: (4, 256, 1, 4),
        4100: (4, 256, 1, 8), 510: (1, 256, 1, 2), 1001: (1, 256, 1, 8), 2049: (1, 256, 1, 32), 8188: (4, 256, 1, 8), 8192: (4, 256, 1, 8),
        8: (4, 1, 256, 2), 260: (4, 64, 4, 2)}[D]
    assert (plan["vec"], plan["tpr"], plan["rows"], plan["inst"]) == want, (case, plan)
    assert plan["groups"] == -(-M // plan["rows"]) and plan["slices"] == -(-plan["groups"] // plan["gps"]) <= plan["max_slices"], plan
    if label.startswith(("vector instance", "scalar instance")):
        assert plan["inst"] == int(label.split()[-1]) and plan["vec"] == (4 if label.startswith("vector") else 1), plan
        below = {2: 0, 4: 2, 8: 4} if plan["vec"] == 4 else {2: 0, 8: 2, 32: 8}
        assert plan["nv"] > below[plan["inst"]], plan                                 # the smallest instance that holds the row
    if label.startswith("bound"):
        assert plan["nv"] == 8 and (D == 8192 or -(-(D // 4) // 256) == 8 and (D // 4) % 256 != 0), plan   # 8188: a ragged last vector round
    if label.startswith("rows edge"):
        assert plan["rows"] == 256 and plan["groups"] == {255: 1, 256: 1, 257: 2}[M] and plan["slices"] == plan["groups"], plan
    if case == CAPPED:
        # more row groups than the cap: several per slice, the last slice short, the last row group ragged
        assert plan["groups"] > plan["max_slices"] and plan["gps"] > 1 and 2 * plan["slices"] > plan["max_slices"], plan
        assert plan["groups"] % plan["gps"] != 0 and M % plan["rows"] != 0, plan
    if case == GRID:
        assert plan["groups"] == 150 and plan["gps"] == 2 and plan["slices"] == 75, plan    # the floor of 8 rows per slice, not the cap


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_case_sits_in_the_regime_it_is_named_for(case):
    assert_regime(case)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernels_match_the_fp64_restatement(case, mode):
    assert_regime(case)
    first = run_vjp(case, mode)
    gate(case, mode, first)
    if mode == "no_a":
        assert not first[2].any()                                   # at = 0: dgamma is zeros
    again = run_vjp(case, mode)                                     # fresh NaN-filled workspace and outputs: the same bits
    for name, u, v in zip(("dx", "dgy", "dgamma"), first, again):
        assert (u is None and v is None) or torch.equal(u, v), name


@pytest.mark.gpu
@pytest.mark.parametrize("big,small", [(GRID, D1000), (BOUND[1], SHORT[2]), (ROWS_EDGE[2], SHORT[3])], ids=lambda c: _id(c))
def test_two_consecutive_calls_on_one_workspace_the_larger_first(big, small):
    """What the first call left in the workspace must not reach the second's dgamma.  The pair runs back to back on one workspace, filled
    with NaN once."""
    lib = _native.load()
    need = [lib.bhg_rmsnorm_ws_bytes(c[1], c[2]) for c in (big, small)]
    assert need[0] > need[1]
    ws = torch.full((need[0] // 8,), float("nan"), dtype=torch.float64, device=DEV)
    outs = []
    for case in (big, small):
        M, D = dims(case)
        x, gy, a, gamma, rstd, b = device_inputs(case)
        dx, dgy, dgamma = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.full_like(gamma, float("nan"))
        rc = lib.bhg_rmsnorm_backward_vjp(x.data_ptr(), gy.data_ptr(), a.data_ptr(), gamma.data_ptr(), rstd.data_ptr(), b.data_ptr(), M, D,
                                          dx.data_ptr(), dgy.data_ptr(), dgamma.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                          int(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "bhg_rmsnorm_backward_vjp")
        outs.append((dx, dgy, dgamma))
    torch.cuda.synchronize()
    for case, got in zip((big, small), outs):
        gate(case, "all", tuple(t.cpu() for t in got), label="shared workspace")

"""bhg_cross_entropy_backward_vjp (csrc/bhg_cross_entropy.hip: k_ce_vjp_rows, k_ce_dg_combine, k_ce_split_sums, k_ce_split_out) through
the C ABI against the float64 restatement tests/cross_entropy_ref.py, array by array, on the smallest shapes at which the kernels can
still go wrong.  Cases are (N, C): one element; C = 2, 3, 9 (scalar accesses), 12 and 16 (16-byte accesses); C = 63, 64, 65 with two rows;
4 x 1000; one shape per kernel instance (2, 4, 8, 16, 32 vectors per thread; 2, 8, 32 scalars), read off the plan; the rows-per-workgroup
edge at C = 8 (256 rows side by side) one below, at and one above, with a ragged last row group; the register-resident bounds (32768
with 16-byte accesses, 8191 with scalar ones) and one above each; split rows: 3 x (32768 + 5) with a ragged last slice, 2 x 262144, and
the few-rows edges (8 x 16384 stays a row, 8 x 16388 and 159 x 16388 are split, 160 x 16388 is not); enough rows of 8 that the workgroup cap is
hit, with a ragged last workgroup and row group; 600 x 260.  Variants: plain; confident (logits x 30: P nearly one-hot); leak (one row
whose a is 1e3 and whose g is 1e-4 times its neighbours'); ignored rows first, last and middle; every row ignored; a target outside
[0, C) standing in for an ignored one.  Modes: per-row g; a scalar g without and with denom; dz NULL; dg NULL.

The restatement is evaluated on the very fp32 log_softmax the kernel reads.  Outputs and workspace are slices of sentinel-filled
buffers: they must be written inside their bounds only, and everywhere inside; the inputs are bit-equal afterwards; a second run on
NaN-filled outputs and workspace gives the same bits.  An ignored row's lsm and a are NaN in the device inputs: zeros must come out.

Gate: the project's 2e-5 for fp32 kernels against fp64 restatements, against a sum-of-absolute-terms scale (a confident row makes
a_k - s a difference of nearly equal terms, as D = 1 does for RMS norm) — dz, per row: |g_i| max_c P_ic (|a_ic| + sum_c' P_ic' |a_ic'|);
dg, per row: sum_c P_ic |a_ic| + |a_iy|; a scalar dg: the sum of the per-row scales, divided by denom where one is given.  An ignored
row's scale is zero: exact zeros are asked.  test_the_gate_can_exclude_no_case (CPU) shows that the restatement rounded to fp32 passes
every case and mode and that every scale of a non-ignored row is positive.  Observed maxima on one MI355X: profiles/cross_entropy_fp64.txt."""
import functools

import pytest
import torch

import cross_entropy_ref as ref
from betty_amd import _native
from betty_amd.backend import cross_entropy_plan

DEV = "cuda:0"
GATE = 2e-5
IGNORE = -100
PAD, SENTINEL = 64, 1234.5
MODES = ["rows", "scalar", "scalar_denom", "no_dz", "no_dg"]
BOUND_VEC, BOUND_SCALAR = 32768, 8191

# (label, N, C, variant, regime, plan fields)
ONE = ("one element", 1, 1, "plain", "short", dict(vec=1, tpr=1, rows=256))
SMALL = [("C=2 scalar", 3, 2, "plain", "short", dict(vec=1, tpr=1, rows=256)), ("C=3 scalar", 2, 3, "plain", "short", dict(vec=1, tpr=2, rows=128)),
         ("C=9 scalar", 5, 9, "plain", "short", dict(vec=1, tpr=8, rows=32)), ("C=12 vector", 3, 12, "plain", "short", dict(vec=4, tpr=2, rows=128)),
         ("C=16 vector", 2, 16, "plain", "short", dict(vec=4, tpr=2, rows=128))]
WAVE = [("around one wave of columns", 2, 63, "plain", "short", dict(vec=1, tpr=32, rows=8)),
        ("around one wave of columns", 2, 64, "plain", "short", dict(vec=4, tpr=8, rows=32)),
        ("around one wave of columns", 2, 65, "plain", "short", dict(vec=1, tpr=64, rows=4))]
C1000 = ("C=1000", 4, 1000, "plain", "short", dict(vec=4, tpr=128, rows=2, inst=2))
INSTANCES = [("vector instance 2", 3, 2048, "plain", "row", dict(vec=4, inst=2)), ("vector instance 4", 3, 2052, "plain", "row", dict(vec=4, inst=4)),
             ("vector instance 8", 3, 4100, "plain", "row", dict(vec=4, inst=8)), ("vector instance 16", 64, 8196, "plain", "row", dict(vec=4, inst=16)),
             ("vector instance 32", 160, 16400, "plain", "row", dict(vec=4, inst=32)), ("scalar instance 2", 3, 510, "plain", "row", dict(vec=1, inst=2)),
             ("scalar instance 8", 3, 1001, "plain", "row", dict(vec=1, inst=8)), ("scalar instance 32", 3, 2049, "plain", "row", dict(vec=1, inst=32))]
ROWS_EDGE = [("rows edge 255", 255, 8, "plain", "short", dict(rows=256, groups=1)), ("rows edge 256", 256, 8, "plain", "short", dict(rows=256, groups=1)),
             ("rows edge 257 ragged", 257, 8, "plain", "short", dict(rows=256, groups=2, wgs=2))]
SHORT_EDGE = [("short edge 1020", 3, 1020, "plain", "short", dict(tpr=128, rows=2)), ("short edge 1024", 3, 1024, "plain", "short", dict(tpr=128, rows=2)),
              ("short edge 1028", 3, 1028, "plain", "row", dict(tpr=256, rows=1, inst=2))]
BOUND = [("vector bound", 160, BOUND_VEC, "plain", "row", dict(vec=4, inst=32, nv=32)), ("vector bound + 1", 4, BOUND_VEC + 1, "plain", "split", dict(vec=1)),
         ("scalar bound", 3, BOUND_SCALAR, "plain", "row", dict(vec=1, inst=32, nv=32)), ("scalar bound + 2", 3, BOUND_SCALAR + 2, "plain", "split", dict(vec=1))]
SPLIT = [("split ragged last slice", 3, BOUND_VEC + 5, "plain", "split", dict(vec=1, slices=33, chunk=1024)),
         ("split longest row", 2, 262144, "plain", "split", dict(vec=4, slices=256, chunk=1024)),
         ("few rows stay rows", 8, 16384, "plain", "row", dict(vec=4, inst=16)), ("few rows split", 8, 16388, "plain", "split", dict(vec=4, slices=17, chunk=1024)),
         ("159 rows split", 159, 16388, "plain", "split", dict(vec=4, slices=9, chunk=2048)), ("160 rows are rows", 160, 16388, "plain", "row", dict(vec=4, inst=32))]
CAPPED = ("cap hit ragged last workgroup", 256 * 1792 + 5, 8, "plain", "short", dict(rows=256, groups=1793, gps=2, wgs=897, max_wgs=1792))
GRID = ("600 x 260", 600, 260, "plain", "short", dict(vec=4, tpr=64, rows=4, groups=150, wgs=150))
_BASES = {"tiny": (5, 9, "short"), "classifier": (4, 1000, "short"), "row": (5, 4100, "row"), "sidebyside": (257, 8, "short"), "split": (5, BOUND_VEC + 5, "split")}


def _variants(name, bases):
    return [(f"{name} {b}", _BASES[b][0], _BASES[b][1], name, _BASES[b][2], {}) for b in bases]


VARIANTS = (_variants("confident", ("tiny", "classifier", "row", "split")) + [("confident one element", 1, 1, "confident", "short", {})]
            + _variants("leak", ("tiny", "classifier", "row", "sidebyside", "split")) + _variants("ignored", ("tiny", "classifier", "row", "sidebyside", "split"))
            + _variants("all_ignored", ("tiny", "row", "split")) + _variants("out_of_range", ("tiny", "row", "split")))
CASES = [ONE] + SMALL + WAVE + [C1000] + INSTANCES + ROWS_EDGE + SHORT_EDGE + BOUND + SPLIT + [CAPPED, GRID] + VARIANTS
CASES = [c[:5] + (tuple(sorted(c[5].items())),) for c in CASES]   # hashable


def _id(c):
    return f"{c[0].replace(' ', '_')}-{c[1]}x{c[2]}" if isinstance(c, tuple) else c


def g_kind(mode):
    return {"rows": "rows", "no_dz": "rows", "no_dg": "rows", "scalar": "scalar", "scalar_denom": "scalar_denom"}[mode]


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(lsm, y, g_rows, g_scalar, denom, a) on the host, fp32 (y int64); computed once per case, shared, never written.  lsm is the
    float64 log_softmax of the fp32 logits, rounded to fp32: what the kernel reads and what the restatement is evaluated on."""
    _, N, C, variant = case[:4]
    gen = torch.Generator().manual_seed((N * 8209 + C) * 7 + len(variant))
    z, a = (torch.randn(N, C, generator=gen) for _ in range(2))
    y = torch.randint(0, C, (N,), generator=gen)
    g_rows, g_scalar = torch.randn(N, generator=gen), torch.randn((), generator=gen)
    if variant == "confident":
        z = 30.0 * z
    if variant == "leak":
        a[N // 2] *= 1e3
        g_rows[N // 2] *= 1e-4
    if variant == "ignored":
        y[0] = y[N - 1] = y[N // 2] = IGNORE
    if variant == "all_ignored":
        y[:] = IGNORE
    if variant == "out_of_range":
        y[0], y[N - 1], y[N // 2] = C, -1, 1 << 40
    lsm = torch.log_softmax(z.double(), dim=1).float()
    denom = ref.valid(y, C, IGNORE).sum().float().reshape(1)
    return lsm, y, g_rows, g_scalar, denom, a


@functools.lru_cache(maxsize=None)
def wanted(case, kind):
    """(dz, dg, sdz, sdg) in float64 for a per-row g ("rows") or a scalar one without / with denom."""
    _, N, C = case[:3]
    lsm, y, g_rows, g_scalar, denom, a = host_inputs(case)
    g = g_rows.double() if kind == "rows" else g_scalar.double()
    dn = denom.double() if kind == "scalar_denom" else None
    dz, dg = ref.cross_entropy_backward_vjp(lsm.double(), y, g, a.double(), IGNORE, dn, scalar_g=kind != "rows")
    sdz, sdg = ref.gate_scales(lsm.double(), y, g, a.double(), IGNORE, dn, scalar_g=kind != "rows")
    return dz, dg, sdz, sdg


def gate(case, mode, got, label="case"):
    """Assert the gate on (dz or None, dg or None) and print the observed maxima; `got` are host tensors."""
    _, N, C = case[:3]
    dz, dg, sdz, sdg = wanted(case, g_kind(mode))
    line = []
    if got[0] is not None:
        err = (got[0].double().reshape(N, C) - dz).abs().amax(dim=1)
        assert bool((err <= GATE * sdz).all()), (label, case, mode, "dz", float((err / sdz.clamp_min(1e-300)).max()))
        live = sdz > 0
        line.append(f"dz {float((err[live] / sdz[live]).max()) if bool(live.any()) else 0.0:.3e}")
    if got[1] is not None:
        if case[3] == "all_ignored" and mode == "scalar_denom":
            assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(dg).all())   # 0 / 0, as the mean of no rows is
            line.append("dg nan (0 / 0)")
        else:
            err, scale = (got[1].double().reshape(dg.shape) - dg).abs().reshape(-1), sdg.reshape(-1)
            assert bool((err <= GATE * scale).all()), (label, case, mode, "dg", float((err / scale.clamp_min(1e-300)).max()))
            live = scale > 0
            line.append(f"dg {float((err[live] / scale[live]).max()) if bool(live.any()) else 0.0:.3e}")
    print(f"cross_entropy_vjp {label} {_id(case)} {case[3]} {mode}: " + "  ".join(line) + "  (worst row of max|got - want| / sum|terms|)")


def assert_regime(case):
    _, N, C, _, regime, fields = case
    for scalar in (False, True):
        plan = cross_entropy_plan(N, C, scalar)
        assert plan["regime"] == regime, (case, plan)
        for k, v in fields:
            assert plan[k] == v, (case, k, plan)
        assert plan["vec"] == (4 if C % 4 == 0 else 1) and plan["wgs"] <= plan["max_wgs"], plan
        if regime == "split":
            assert plan["launches"] == 2 and plan["chunk"] % 1024 == 0 and plan["slices"] == -(-C // plan["chunk"]) <= 256, plan
            assert plan["ws"] == 8 * N * plan["slices"], plan
        else:
            assert plan["launches"] == (2 if scalar else 1) and plan["rows"] == 256 // plan["tpr"], plan
            assert plan["groups"] == -(-N // plan["rows"]) and plan["wgs"] == -(-plan["groups"] // plan["gps"]), plan
            assert plan["nv"] <= plan["inst"] and plan["ws"] == (8 * plan["wgs"] if scalar else 0), plan
            if case[0].startswith(("vector instance", "scalar instance")):
                below = {2: 0, 4: 2, 8: 4, 16: 8, 32: 16} if plan["vec"] == 4 else {2: 0, 8: 2, 32: 8}
                assert plan["nv"] > below[plan["inst"]], plan   # the smallest instance that holds the row
    if case[0] == "split ragged last slice":
        assert C % 1024 == 5
    if case[:3] == CAPPED[:3]:
        assert plan["groups"] > plan["max_wgs"] and plan["groups"] % plan["gps"] != 0 and N % plan["rows"] != 0, plan


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_case_sits_in_the_regime_it_is_named_for(case):
    assert_regime(case)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    """The restatement rounded to fp32 passes every case and mode; and every scale of a non-ignored row is positive, so that the gate asks
    something of every such row (of an ignored row it asks exact zeros)."""
    _, N, C = case[:3]
    m = ref.valid(host_inputs(case)[1], C, IGNORE)
    for mode in MODES:
        dz, dg, sdz, sdg = wanted(case, g_kind(mode))
        gate(case, mode, (None if mode == "no_dz" else dz.float(), None if mode == "no_dg" else dg.float()), label="fp64 rounded to fp32")
        assert bool((sdz[m] > 0).all()) and not sdz[~m].any() and not dz[~m].any(), (case, mode)
        if g_kind(mode) == "rows":
            assert bool((sdg[m] > 0).all()) and not sdg[~m].any() and not dg[~m].any(), (case, mode)
        elif bool(m.any()):
            assert float(sdg) > 0, (case, mode)


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    """The host inputs on the device — with NaN in lsm and a wherever the row is ignored: the kernel must not read them."""
    lsm, y, g_rows, g_scalar, denom, a = (t.clone() for t in host_inputs(case))
    m = ref.valid(y, case[2], IGNORE)
    lsm[~m] = float("nan")
    a[~m] = float("nan")
    return tuple(t.to(DEV) for t in (lsm, y, g_rows, g_scalar.reshape(1), denom, a))


def _padded(numel, dtype=torch.float32):
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    inner = buf[PAD:PAD + numel]
    assert inner.data_ptr() % 16 == 0
    inner.fill_(float("nan"))
    return buf, inner


def _outside_untouched(buf, numel):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + numel:] == SENTINEL).all())


def run_vjp(case, mode):
    """One call on buffers this function owns.  Returns (dz or None, dg or None) on the host after checking the bounds of every write,
    that every element inside was written, and that the inputs are unchanged."""
    lib = _native.load()
    _, N, C = case[:3]
    ins = device_inputs(case)
    before = [t.clone() for t in ins]
    lsm, y, g_rows, g_scalar, denom, a = ins
    kind = g_kind(mode)
    scalar = kind != "rows"
    plan = cross_entropy_plan(N, C, scalar)
    ws_bytes = int(lib.bhg_cross_entropy_ws_bytes(N, C, int(scalar)))
    assert ws_bytes == plan["ws"]
    wsbuf, ws = _padded(ws_bytes // 8, torch.float64)
    dzbuf, dz = _padded(N * C)
    dgbuf, dg = _padded(1 if scalar else N)
    g = g_scalar if scalar else g_rows
    rc = lib.bhg_cross_entropy_backward_vjp(lsm.data_ptr(), y.data_ptr(), g.data_ptr(), int(scalar), denom.data_ptr() if kind == "scalar_denom" else None,
                                            a.data_ptr(), N, C, IGNORE, None if mode == "no_dz" else dz.data_ptr(),
                                            None if mode == "no_dg" else dg.data_ptr(), ws.data_ptr(), ws_bytes,
                                            int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_cross_entropy_backward_vjp")
    torch.cuda.synchronize()
    for t, t0 in zip(ins, before):
        assert torch.equal(t.view(torch.int32 if t.dtype == torch.float32 else t.dtype), t0.view(torch.int32 if t.dtype == torch.float32 else t.dtype)), "an input was modified"
    for name, buf, t in (("dz", dzbuf, dz), ("dg", dgbuf, dg), ("ws", wsbuf, ws)):
        assert _outside_untouched(buf, t.numel()), f"write outside {name}"
    nan_dg = case[3] == "all_ignored" and mode == "scalar_denom"
    if mode == "no_dz":
        assert bool(torch.isnan(dz).all()), "dz was not given: its buffer must stay untouched"
    else:
        assert bool(torch.isfinite(dz).all()), "an element of dz was not written (or an ignored row was read)"
    if mode == "no_dg":
        assert bool(torch.isnan(dg).all()), "dg was not given: its buffer must stay untouched"
    else:
        assert nan_dg or bool(torch.isfinite(dg).all()), "an element of dg was not written (or a stale partial sum was read)"
    assert bool(torch.isfinite(ws).all()), "the workspace: every partial the plan names is written"
    return (None if mode == "no_dz" else dz.cpu()), (None if mode == "no_dg" else dg.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernels_match_the_fp64_restatement(case, mode):
    assert_regime(case)
    first = run_vjp(case, mode)
    gate(case, mode, first)
    again = run_vjp(case, mode)   # fresh NaN-filled workspace and outputs: the same bits
    for name, u, v in zip(("dz", "dg"), first, again):
        assert (u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32)), name


@pytest.mark.gpu
def test_scalar_g_with_dz_only_needs_no_combine_and_leaves_dg_alone():
    """A scalar g with dg NULL: one launch in the short / row regimes, and the partials of dg are not written."""
    lib = _native.load()
    case = GRID[:5] + (tuple(sorted(GRID[5].items())),)
    _, N, C = case[:3]
    lsm, y, _, g_scalar, denom, a = device_inputs(case)
    ws = torch.full((int(lib.bhg_cross_entropy_ws_bytes(N, C, 1)) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    dz = torch.full((N, C), float("nan"), device=DEV)
    rc = lib.bhg_cross_entropy_backward_vjp(lsm.data_ptr(), y.data_ptr(), g_scalar.data_ptr(), 1, denom.data_ptr(), a.data_ptr(), N, C, IGNORE,
                                            dz.data_ptr(), None, None, 0, int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_cross_entropy_backward_vjp")
    torch.cuda.synchronize()
    gate(case, "scalar_denom", (dz.cpu(), None), label="dz only")
    assert bool(torch.isnan(ws).all())

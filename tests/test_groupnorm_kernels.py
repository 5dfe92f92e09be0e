"""bhg_groupnorm_backward_vjp (csrc/bhg_groupnorm.hip: k_gn_vjp_rows / k_gn_vjp_rows_streamed + k_gn_vjp_combine) through the C ABI against
the float64 restatement tests/groupnorm_ref.py, array by array, on the smallest shapes at which the kernels can still go wrong.  Cases are
(N, C, G, HW): one element; rows of 2, 3, 9 (scalar accesses, an odd channel edge), 12 (a 16-byte vector straddling a channel edge) and
16 elements; the instance-norm form G = C at HW = 63, 64, 65; the layer-norm form G = 1; D = 1000; the resident edge (8188, 8192) and the
first streamed rows (8196 with 16-byte, 8193 with scalar accesses); ResNet's D = 25088; the family's bound D = 2^20; one below / at / one
above the rows-per-workgroup edge the plan reports at D = 8, with a ragged last row group; many workgroups; a far mean
(x = 100 + 0.01 N(0, 1)); one row whose x is 1e3 and whose gy, a are 1e-4 times its neighbours' (a leak between rows would show).  Each
case with all pointers given, a NULL, gamma NULL (affine off: b, c, dgamma and the workspace NULL as well), b and c NULL, c alone NULL,
and dgamma NULL (the workspace given: it must stay untouched).  Each case first reads the plan and asserts the regime it is named for.

The restatement is evaluated on the very fp32 mean / rstd the kernel reads.  Outputs and workspace are slices of sentinel-filled
buffers: they must be written inside their bounds only, and everywhere inside; a NULL output's buffer stays untouched; the inputs are
bit-equal afterwards; a second run on NaN-filled outputs and workspace gives the same bits.

Gate, per row (n, g) of dx and dgy: max|got - want| <= 2e-5 max|want_row| — the project's gate for fp32 kernels against fp64
restatements.  Per channel of dgamma: |got - want| <= 2e-5 sum_{n,hw} |gy r at|, the sum of the absolute terms, so
that cancellation in a channel cannot fail a correct kernel.  test_the_gate_can_exclude_no_case (CPU) shows that the restatement
rounded to fp32 passes every case and that the gate's denominators are positive wherever the mathematics leaves them so.  Observed
maxima on one MI355X: profiles/groupnorm_fp64.txt."""
import functools

import pytest
import torch

import groupnorm_ref
from betty_amd import _native
from betty_amd.backend import groupnorm_plan

DEV = "cuda:0"
GATE = 2e-5
EPS = 1e-5
PAD, SENTINEL = 64, 1234.5
MODES = ["all", "no_a", "no_gamma", "no_bc", "no_c", "no_dgamma"]

# (label, N, C, G, HW, variant)
ONE = ("one element", 1, 1, 1, 1, "plain")
SHORT = [("D=2", 3, 4, 2, 1, "plain"), ("D=3", 2, 2, 2, 3, "plain"), ("D=9 scalar odd channel edge", 2, 6, 2, 3, "plain"),
         ("D=12 vector across a channel edge", 2, 4, 2, 6, "plain"), ("D=16", 2, 8, 2, 4, "plain")]
INSTANCE = [("instance-norm form", 2, 3, 3, hw, "plain") for hw in (63, 64, 65)]
LAYER = ("layer-norm form", 3, 6, 1, 16, "plain")
D1000 = ("D=1000", 2, 16, 2, 125, "plain")
RESIDENT_EDGE = [("resident edge D=8188", 2, 8, 2, 2047, "plain"), ("resident edge D=8192", 2, 16, 2, 1024, "plain")]
STREAMED = [("first streamed vector row D=8196", 2, 8, 2, 2049, "plain"), ("first streamed scalar row D=8193", 2, 2, 2, 8193, "plain"),
            ("resnet D=25088", 2, 16, 2, 3136, "plain"), ("bound D=2^20", 1, 4, 1, 262144, "plain")]
ROWS_EDGE = [("rows edge 255", 51, 10, 5, 4, "plain"), ("rows edge 256", 32, 16, 8, 4, "plain"), ("rows edge 257 ragged", 257, 2, 1, 4, "plain")]
GRID = ("many rows", 64, 64, 32, 16, "plain")
FAR_MEAN = [("far mean", 2, 6, 2, 3, "far_mean"), ("far mean", 2, 16, 2, 125, "far_mean"), ("far mean", 2, 8, 2, 2049, "far_mean")]
LEAK = [("leak", 3, 6, 1, 16, "leak"), ("leak", 2, 16, 2, 125, "leak"), ("leak", 2, 8, 2, 2049, "leak")]
CASES = [ONE] + SHORT + INSTANCE + [LAYER, D1000] + RESIDENT_EDGE + STREAMED + ROWS_EDGE + [GRID] + FAR_MEAN + LEAK
# beyond the list: the other kernel instances (4 vectors per thread; the scalar ones with 8 and 32), a grid above the CU count (600
# workgroups), channels shorter than a 16-byte vector (HW = 1, 2) on the vector path, a streamed row whose channels are shorter than a
# tile and not aligned with it, and a streamed row of many one-element channels
EXTRA = [("four vectors", 2, 4, 2, 1026, "plain"), ("scalar instances", 2, 2, 2, 1001, "plain"), ("scalar instances", 2, 14, 2, 1170, "plain"),
         ("600 workgroups", 600, 4, 2, 260, "plain"), ("HW=1 vector path", 5, 64, 4, 1, "plain"), ("HW=2 vector path", 3, 12, 2, 2, "plain"),
         ("streamed short channels", 2, 26, 1, 333, "plain"), ("streamed HW=1", 2, 9000, 1, 1, "plain"), ("streamed HW=5", 1, 4004, 2, 5, "plain")]


def _id(c):
    return f"{c[0].replace(' ', '_')}-{c[1]}x{c[2]}g{c[3]}hw{c[4]}{'' if c[5] == 'plain' else '-' + c[5]}" if isinstance(c, tuple) else c


def dims(case):
    _, N, C, G, HW, _ = case
    return N, C, G, HW, (C // G) * HW


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    """(x, gy, a, gamma, mean, rstd, b, c) on the host, fp32; computed once per case, shared, never written.  x is [N, C, HW]; mean and
    rstd are the float64 statistics of the fp32 x, rounded to fp32: what the kernel reads and what the restatement is evaluated on."""
    N, C, G, HW, D = dims(case)
    g = torch.Generator().manual_seed(((N * 8209 + C) * 31 + G) * 3 + HW + len(case[5]))
    x, gy, a = (torch.randn(N, C, HW, generator=g) for _ in range(3))
    gamma, b, c = (torch.randn(C, generator=g) for _ in range(3))
    if case[5] == "far_mean":
        x = 100.0 + 0.01 * x
    if case[5] == "leak":
        row = (N * G) // 2
        for t, f in ((x, 1e3), (gy, 1e-4), (a, 1e-4)):
            t.view(N * G, D)[row] *= f
    mean, rstd = groupnorm_ref.stats(x.double(), G, EPS)
    return x, gy, a, gamma, mean.float(), rstd.float(), b, c


def present(mode):
    """Which of (a, gamma, b, c, dgamma, ws) the call is given."""
    return {"all": (True, True, True, True, True, True), "no_a": (False, True, True, True, True, True),
            "no_gamma": (True, False, False, False, False, False), "no_bc": (True, True, False, False, True, True),
            "no_c": (True, True, True, False, True, True), "no_dgamma": (True, True, True, True, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def wanted(case, mode):
    """(dx, dgy, dgamma or None, the absolute terms of dgamma or None) in float64; dx and dgy as [N * G, D] rows."""
    N, C, G, HW, D = dims(case)
    x, gy, a, gamma, mean, rstd, b, c = (t.double() for t in host_inputs(case))
    ha, hg, hb, hc, hd, _ = present(mode)
    a, gamma, b, c = (a if ha else None), (gamma if hg else None), (b if hb else None), (c if hc else None)
    dx, dgy, dgamma = groupnorm_ref.groupnorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c, G)
    terms = groupnorm_ref.dgamma_abs_terms(x, gy, a, mean, rstd, G) if hd else None
    return dx.reshape(N * G, D), dgy.reshape(N * G, D), (dgamma if hd else None), terms


def gate(case, mode, got, label="case"):
    """Assert the gate on (dx, dgy, dgamma) and print the observed maxima; `got` are host tensors (dgamma None when not wanted)."""
    N, C, G, HW, D = dims(case)
    dx, dgy, dgamma, terms = wanted(case, mode)
    line = []
    for name, g, want in (("dx", got[0], dx), ("dgy", got[1], dgy)):
        err = (g.double().reshape(N * G, D) - want).abs().amax(dim=1)
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
    print(f"groupnorm_vjp {label} {_id(case)} {mode}: " + "  ".join(line) + "  (worst row of max|got - want| / max|want_row|; dgamma: / sum|terms|)")


@pytest.mark.parametrize("case", CASES + EXTRA, ids=_id)
def test_the_gate_can_exclude_no_case(case):
    """The restatement rounded to fp32 passes; and the gate's denominators are positive, so that it asks something of every row and
    channel — except where the result is zero by the mathematics, where the gate asks for exactly zero: a one-element row (xh = 0: dx = 0,
    at = 0: dgamma's terms are 0, dgy = c), and dgamma without a (at = 0)."""
    N, C, G, HW, D = dims(case)
    for mode in MODES:
        dx, dgy, dgamma, terms = wanted(case, mode)
        gate(case, mode, (dx.float(), dgy.float(), None if dgamma is None else dgamma.float()), label="fp64 rounded to fp32")
        if D > 1:
            assert bool((dx.abs().amax(dim=1) > 0).all()) and bool((dgy.abs().amax(dim=1) > 0).all()), (case, mode)
            if terms is not None and mode != "no_a":
                assert bool((terms > 0).all()), (case, mode)
        elif mode in ("all", "no_a", "no_dgamma"):
            assert bool((dgy.abs().amax(dim=1) > 0).all()), (case, mode)


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
    N, C, G, HW, D = dims(case)
    ins = device_inputs(case)
    before = [t.clone() for t in ins]
    x, gy, a, gamma, mean, rstd, b, c = ins
    ha, hg, hb, hc, hd, hw = present(mode)
    ws_bytes = int(lib.bhg_groupnorm_ws_bytes(N, C))
    assert ws_bytes == 8 * N * C == groupnorm_plan(N, C, HW, G)["ws"]
    wsbuf, ws = _padded(ws_bytes // 8, torch.float64)
    dxbuf, dx = _padded(x.numel())
    dgybuf, dgy = _padded(x.numel())
    dgbuf, dgamma = _padded(C)
    ptr = lambda t, on=True: t.data_ptr() if on else None   # noqa: E731
    rc = lib.bhg_groupnorm_backward_vjp(x.data_ptr(), gy.data_ptr(), ptr(a, ha), ptr(gamma, hg), mean.data_ptr(), rstd.data_ptr(), ptr(b, hb),
                                        ptr(c, hc), N, C, HW, G, dx.data_ptr(), dgy.data_ptr(), ptr(dgamma, hd), ptr(ws, hw),
                                        ws_bytes if hw else 0, int(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "bhg_groupnorm_backward_vjp")
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
    N, C, G, HW, D = dims(case)
    plan = groupnorm_plan(N, C, HW, G)
    assert plan["D"] == D and plan["vec"] == (4 if D % 4 == 0 else 1), plan
    assert plan["regime"] == ("streamed" if D > 8192 else "resident"), plan
    assert plan["grid"] == plan["groups"] == -(-N * G // plan["rows"]) and plan["ws"] == 8 * N * C, plan
    want = {  # D: (regime, vec, tpr, rows, inst)
        1: ("resident", 1, 1, 256, 2), 2: ("resident", 1, 1, 256, 2), 3: ("resident", 1, 2, 128, 2), 9: ("resident", 1, 8, 32, 2),
        12: ("resident", 4, 2, 128, 2), 16: ("resident", 4, 2, 128, 2), 63: ("resident", 1, 32, 8, 2), 64: ("resident", 4, 8, 32, 2),
        65: ("resident", 1, 64, 4, 2), 96: ("resident", 4, 16, 16, 2), 1000: ("resident", 4, 128, 2, 2), 8188: ("resident", 4, 256, 1, 8),
        8192: ("resident", 4, 256, 1, 8), 8196: ("streamed", 4, 256, 1, 2), 8193: ("streamed", 1, 256, 1, 8), 25088: ("streamed", 4, 256, 1, 2),
        2 ** 20: ("streamed", 4, 256, 1, 2), 8: ("resident", 4, 1, 256, 2), 32: ("resident", 4, 4, 64, 2),
        2052: ("resident", 4, 256, 1, 4), 1001: ("resident", 1, 256, 1, 8), 8190: ("resident", 1, 256, 1, 32), 520: ("resident", 4, 128, 2, 2),
        6: ("resident", 1, 4, 64, 2), 8658: ("streamed", 1, 256, 1, 8), 9000: ("streamed", 4, 256, 1, 2), 10010: ("streamed", 1, 256, 1, 8)}[D]
    assert (plan["regime"], plan["vec"], plan["tpr"], plan["rows"], plan["inst"]) == want, (case, plan)
    if label.startswith("rows edge"):
        assert plan["rows"] == 256 and plan["groups"] == {255: 1, 256: 1, 257: 2}[N * G], plan
    if case == GRID:
        assert plan["groups"] == 32, plan
    if label == "600 workgroups":
        assert plan["grid"] == 600, plan


@pytest.mark.parametrize("case", CASES + EXTRA, ids=_id)
def test_every_case_sits_in_the_regime_it_is_named_for(case):
    assert_regime(case)


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
@pytest.mark.parametrize("big,small", [(GRID, D1000), (STREAMED[2], STREAMED[0]), (ROWS_EDGE[2], SHORT[2])], ids=lambda c: _id(c))
def test_two_consecutive_calls_on_one_workspace_the_larger_first(big, small):
    """What the first call left in the workspace must not reach the second's dgamma.  The pair runs back to back on one workspace, filled
    with NaN once."""
    lib = _native.load()
    need = [lib.bhg_groupnorm_ws_bytes(c[1], c[2]) for c in (big, small)]
    assert need[0] > need[1]
    ws = torch.full((need[0] // 8,), float("nan"), dtype=torch.float64, device=DEV)
    outs = []
    for case in (big, small):
        N, C, G, HW, D = dims(case)
        x, gy, a, gamma, mean, rstd, b, c = device_inputs(case)
        dx, dgy, dgamma = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.full_like(gamma, float("nan"))
        rc = lib.bhg_groupnorm_backward_vjp(x.data_ptr(), gy.data_ptr(), a.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            b.data_ptr(), c.data_ptr(), N, C, HW, G, dx.data_ptr(), dgy.data_ptr(), dgamma.data_ptr(),
                                            ws.data_ptr(), ws.numel() * 8, int(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "bhg_groupnorm_backward_vjp")
        outs.append((dx, dgy, dgamma))
    torch.cuda.synchronize()
    for case, got in zip((big, small), outs):
        gate(case, "all", tuple(t.cpu() for t in got), label="shared workspace")

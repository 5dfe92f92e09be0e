"""Every form plan_solve (csrc/mlp/solve_plan.inc) gives the fused MLP solvers, held to an fp64 reference that shares none of their
algebra (tests/solver_forms_ref.py: the oracle's cg / neumann, a plain N-sized CG / Neumann series with a double-backward HVP, an
R-forward written out layer by layer) — on the PRODUCT library, the forms reached by shape alone.  No debug key is set anywhere here.

Three quantities per (case, setting, algorithm):
  hypergradient      with and without keep_solution:  rel <= 1e-4  and  rel <= max(1e-5, 4 spread)
  solution           keep_solution=True: x (CG) / p (Neumann) read from the layout's state, EACH of the 2L tensors on its own:
                     |got - want| / |want| <= max(1e-5, 4 e32) and <= 1e-4   (W_0 holds most of the norm and would hide a wrong b_2)
  mixed coefficient  keep_solution=False: buf.coeff[:B], sample by sample: max|got - want| <= max(2e-5, 4 e32) max|want|, all finite
spread / e32 = the error of the SAME reference computed in fp32 on the CPU on the instance (the gates are therefore ones a correct
fp32 computation meets by construction: four times its own error, or the floor).  Beside them: the launch counters of every solve are
what the plan promises, and a second run of the same solve on the same cached buffers is bit-equal.

Which case is here for which form: the table CASES, asserted literally by test_every_case_reaches_the_form_it_is_here_for.

Settings (ridge, step, K): K = 1 has no recurrence step; K = 2 is the first projected iteration (ChainMode.second); at K = 3 every
parity slot (pb0 / pb1, gp1 / gp2, the two Rh_0 slots of vnew, the v0 / v1 ping-pong) has been both written and read; step 0.5 for CG
is the reference's cg_alpha quirk; ridge 0 is shift = 0.

Seeds: sum(dims) + B, the next one where an instance misses a condition (kink margin >= 1.5e-6; the reference's own fp32-vs-fp64 error
<= 2e-5 at every setting on the hypergradient, on each tensor of the solution and on the coefficient):
  [256,256,128,64,10]  B = 256: seed 970 has a kink margin of 1.48e-7 -> 971 (margin 9.8e-6)
  [192,192,96,10]      B = 1:   the Hessian of one sample has a handful of distinct eigenvalues, CG is close to converged after three
                                to five iterations and, having no breakdown guard (cg.py:38-56), amplifies rounding from there: the
                                fp32 spread of CG at (0.3, 1.0, 5), (0.3, 0.5, 4) or (0.0, 1.0, 3) exceeds 2e-5 for four seeds in five
                                (3.2e-5, 4.2e-5, 4.5e-5, 1.6e-4, 3.3e-5, 5.0e-5, 2.7e-3 at 491 .. 497) and depends on the host's
                                CPU (498 has 4.9e-6 on one host, 3.0e-5 on another).  491 .. 560 each miss the bound on at least
                                one of the two hosts measured -> 561 (3.6e-6 / 1.2e-5)
  [256,256,128,64,24]  B = 100: seed 828 has a hypergradient spread of 2.8e-5 for CG at (0.0, 1.0, 3) -> 829 (worst spread 8.9e-6)
  [256,256,192,640,10] B = 100: seed 1454 has a hypergradient spread of 2.7e-5 for CG at (0.0, 1.0, 3) -> 1455 (worst spread 5.1e-6)
  [70,130,36,10]       B = 100: at seed 346 CG at (0.0, 1.0, 3) is badly conditioned: the CPU fp32 spread is 1.8e-5 on one host and 5.5e-6
                                on another, while both GPU forms sit at 1.7e-5 — inside the bound, but the tight gate would hang on the
                                host's rounding -> 347 (worst spread 1.9e-6)
(all measured with one CPU thread, as conftest.py runs the suite).  No other seed was replaced.

Measured errors: profiles/solver_forms_fp64.txt."""
import functools

import numpy as np
import pytest
import torch

import solver_forms_ref as R
from betty_amd import _native
from betty_amd.hypergradient import _mlp_hip

# ---- the plans, as literals: (form, proj_level, lin, lin_head, head_j, upd_first, closing) ---------------------------------------------
G, GK, NONE = "k_graw", "k_grawk", "k_outer_all"
CLASSIC = ("classic", 0, 0, 0, 0, 0, NONE)
HOISTED = ("hoisted", 0, 0, 0, 0, 0, NONE)


def PSTEP(closing):
    return ("fully-projected (k_pstep launch)", 2, 0, 0, 0, 0, closing)


def SIX(closing, head_j):
    return ("six-launch (k_wskpl .. k_headu .. k_graw)", 2, 1, 1, head_j, 0, closing)


def SIXC(closing, upd_first):
    return ("six-launch-class (k_wskpl first, recurrences beside the chain)", 2, 1, 0, 0, upd_first, closing)


def KEEP(closing):
    return ("projected-keep-state", 1, 0, 0, 0, 0, closing)


def NEU(closing):
    return ("projected-neumann (update inside k_graw)", 1, 0, 0, 0, 0, closing)


# (dims, B, seed, CG without x, CG with x, Neumann without accumulator, Neumann with accumulator)
CASES = [
    ([36, 7], 5, 48, CLASSIC, CLASSIC, CLASSIC, CLASSIC),                                   # L = 1: head only
    ([256, 192, 10], 128, 586, CLASSIC, CLASSIC, CLASSIC, CLASSIC),                         # L = 2
    ([64, 64, 32, 10], 17, 187, HOISTED, HOISTED, HOISTED, CLASSIC),                        # the cost model declines projection
    ([128, 128, 64, 10], 300, 630, HOISTED, HOISTED, HOISTED, CLASSIC),                     # three 128-row batch tiles
    ([128, 128, 64, 10], 64, 394, PSTEP(G), KEEP(G), NEU(G), CLASSIC),
    ([192, 192, 96, 10], 1, 561, PSTEP(G), KEEP(G), NEU(G), CLASSIC),                       # one sample (491 .. 560: see above)
    ([256, 384, 128, 10], 200, 978, PSTEP(GK), KEEP(GK), NEU(GK), CLASSIC),
    ([256, 256, 128, 64, 10], 256, 971, SIX(GK, 0), KEEP(GK), NEU(GK), CLASSIC),            # Bp = 256, no padded row (970: kink 1.48e-7)
    ([256, 256, 128, 64, 24], 100, 829, SIXC(G, 0), KEEP(G), NEU(G), CLASSIC),              # 24 classes (828: spread 2.8e-5)
    ([256, 256, 192, 640, 10], 100, 1455, SIXC(G, 0), KEEP(G), NEU(G), CLASSIC),            # last hidden layer > 512 (1454: spread 2.7e-5)
    ([256, 256, 128, 64, 100], 100, 904, SIXC(G, 0), KEEP(G), NEU(G), CLASSIC),             # 100-class head
    ([256, 256, 128, 128, 64, 10], 100, 942, SIXC(G, 1), KEEP(G), NEU(G), CLASSIC),         # deeper than four layers: upd_first
    ([256, 256, 128, 128, 64, 10], 200, 1042, SIXC(GK, 1), KEEP(GK), NEU(GK), CLASSIC),
    ([256, 128, 128, 64, 10], 100, 686, SIX(G, 1), KEEP(G), NEU(G), CLASSIC),               # head_j on the product build
    ([70, 130, 36, 10], 100, 347, PSTEP(G), KEEP(G), NEU(G), CLASSIC),                      # the zero-padded twin: kernels see 96-160-64-10 (346: see above)
]
TWIN = 14

# (ridge, step, K)
SETTINGS = {
    "cg": [(0.3, 1.0, 1), (0.3, 1.0, 2), (0.3, 1.0, 5), (0.3, 0.5, 4), (0.0, 1.0, 3)],
    "neumann": [(0.3, 0.25, 1), (0.3, 0.25, 2), (0.3, 0.25, 6), (0.0, 0.25, 3)],
}
RUNS = [(c, a, s) for c in range(len(CASES)) for a in ("cg", "neumann") for s in range(len(SETTINGS[a]))]

SPREAD_MAX, KINK_MIN = 2e-5, 1.5e-6                  # tests/test_shapes_goldens.py's bounds on an instance
HARD, TIGHT_FLOOR, TIGHT_FACTOR = 1e-4, 1e-5, 4.0    # tests/test_head_j_fp64.py's
ARRAY_GATE = 2e-5                                    # tests/test_head_j_fp64.py's

_id = lambda v: str(v).replace(" ", "")
_case_id = lambda c: f"{_id(CASES[c][0])}-B{CASES[c][1]}"
_run_id = lambda r: "%s-%s-ridge%s-step%s-K%s" % ((_case_id(r[0]), r[1]) + SETTINGS[r[1]][r[2]])


def _kdims(case):
    """The widths the kernels see (the twin's for nets of >= 3 layers: _mlp_hip.make_state)."""
    dims = CASES[case][0]
    return list(_mlp_hip.padded_dims(dims)) if len(dims) - 1 >= 3 else list(dims)


def _plan(case, algo, keep):
    d = _native.plan_describe(_kdims(case), CASES[case][1], algo, keep)
    return d, (d["form"], d["proj_level"], d["lin"], d["lin_head"], d["head_j"], d["upd_first"], d["closing"])


def _table(case, algo, keep):
    return CASES[case][3 + 2 * (algo == "neumann") + int(keep)]


# ---- the reference, computed once per (instance, setting, algorithm) and left unchanged ------------------------------------------------
def _frozen(q):
    for a in [q["hypergradient"], q["coeff"], q["hypergradient_plain"], q["hypergradient_coeff"]] + q["solution"]:
        a.setflags(write=False)
    return q


def _quantities(case, algo, s, dtype):
    dims, B, seed = CASES[case][:3]
    ridge, step, K = SETTINGS[algo][s]
    return R.quantities(dims, B, ridge, K, step, seed, algo, dtype)


@functools.lru_cache(maxsize=None)
def _ref(case, algo, s):
    return _frozen(_quantities(case, algo, s, torch.float64))


@functools.lru_cache(maxsize=None)
def _kink(case):
    dims, B, seed = CASES[case][:3]
    return R.kink_margin(dims, B, seed)


def _l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want)) if np.all(np.isfinite(got)) else float("inf")


def _max_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max()) if np.all(np.isfinite(got)) else float("inf")


@functools.lru_cache(maxsize=None)
def _e32(case, algo, s):
    """(spread of the hypergradient, [e32 of each solution tensor], e32 of the coefficient): CPU fp32 against CPU fp64."""
    q32, q64 = _quantities(case, algo, s, torch.float32), _ref(case, algo, s)
    return (R.rel([q32["hypergradient"]], q64["hypergradient"]), [_l2(a, b) for a, b in zip(q32["solution"], q64["solution"])],
            _max_err(q32["coeff"], q64["coeff"]))


def _names(case):
    return [f"{n}_{l}" for l in range(len(CASES[case][0]) - 1) for n in ("W", "b")]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_form_it_is_here_for():
    """The table, literally: form, proj_level, lin, lin_head, head_j, upd_first and closing of all four (algorithm, keep_solution)
    plans of every case.  A change to the cost model that moves a case to another form fails here."""
    assert not _native.is_ab()
    for case, (dims, B) in enumerate(c[:2] for c in CASES):
        for algo in ("cg", "neumann"):
            for keep in (False, True):
                d, got = _plan(case, algo, keep)
                assert d["fused"] == 1, (dims, B)
                assert got == _table(case, algo, keep), (dims, B, algo, keep, got)
    assert _kdims(TWIN) == [96, 160, 64, 10] != CASES[TWIN][0]
    assert all(_kdims(c) == CASES[c][0] for c in range(len(CASES)) if c != TWIN)
    # every form of the issue's list is there
    free = {CASES[c][3] for c in range(len(CASES))}
    assert {CLASSIC, HOISTED, PSTEP(G), PSTEP(GK), SIX(G, 1), SIX(GK, 0), SIXC(G, 0), SIXC(G, 1), SIXC(GK, 1)} <= free
    assert {KEEP(G), KEEP(GK), HOISTED, CLASSIC} == {CASES[c][4] for c in range(len(CASES))}
    assert {NEU(G), NEU(GK), HOISTED, CLASSIC} == {CASES[c][5] for c in range(len(CASES))}


@pytest.mark.parametrize("case", range(len(CASES)), ids=_case_id)
def test_plain_solves_of_the_reference_reproduce_the_oracle(case):
    """plain_cg / plain_neumann carried to the hypergradient — through autograd, and through mixed_coeff's layer-by-layer R-forward
    (sum_b coeff_b d w_b / d upper) — give the oracle's fp64 output to 1e-9 at every setting: the solution and the coefficient the
    GPU is held to are those of the solve the oracle ran."""
    for c, algo, s in (r for r in RUNS if r[0] == case):
        q = _ref(c, algo, s)
        for how in ("hypergradient_plain", "hypergradient_coeff"):
            err = R.rel([q[how]], q["hypergradient"])
            assert err <= 1e-9, (algo, SETTINGS[algo][s], how, err)


@pytest.mark.parametrize("case", range(len(CASES)), ids=_case_id)
def test_every_instance_meets_its_conditions(case):
    dims, B, seed = CASES[case][:3]
    assert dims[-1] >= 2, "one class: the softmax error is identically zero and the case proves nothing"
    assert _kink(case) >= KINK_MIN, _kink(case)
    for c, algo, s in (r for r in RUNS if r[0] == case):
        q, (spread, e_sol, e_coeff) = _ref(c, algo, s), _e32(c, algo, s)
        what = (algo, SETTINGS[algo][s])
        assert np.linalg.norm(q["hypergradient"]) > 0.0 and np.abs(q["coeff"]).max() > 0.0, what
        assert len(q["solution"]) == 2 * (len(dims) - 1) and all(np.linalg.norm(t) > 0.0 for t in q["solution"]), what
        assert q["coeff"].shape == (B,)
        print(f"SF64 instance dims={_id(dims)} B={B} seed={seed} algo={algo} setting={SETTINGS[algo][s]} kink_margin={_kink(case):.2e} "
              f"spread={spread:.2e} e32_solution_max={max(e_sol):.2e} e32_coeff={e_coeff:.2e}")
        assert spread <= SPREAD_MAX, what + (spread,)
        assert max(e_sol) <= SPREAD_MAX, what + (dict(zip(_names(case), e_sol)),)
        assert e_coeff <= SPREAD_MAX, what + (e_coeff,)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _buffers(curr):
    """The device buffers of the net — of its zero-padded twin where it runs on one."""
    first = curr.module.layers[0]
    if first in _mlp_hip._TWINS:
        (twin,) = _mlp_hip._TWINS[first].values()
        first = twin.layers[0]
    (buf,) = _mlp_hip._BUFFERS[first].values()
    return buf


def _padding_nonzeros(curr, vector, algo):
    """How many PADDED elements of the twin's own solution vector are not zero (None: the net runs on no twin)."""
    from betty_amd.backend import get_backend

    first = curr.module.layers[0]
    if first not in _mlp_hip._TWINS:
        return None
    (twin,) = _mlp_hip._TWINS[first].values()
    play = get_backend().layout(twin.dirs)
    pflat = play.state(3)[0 if algo == "cg" else 2]   # PaddedHipMLPState.cg_solve: px; .neumann_solve: pp
    count = 0
    for view, real in zip(play.views(pflat, twin.dirs), vector):
        pad = view.clone()
        pad[tuple(slice(0, n) for n in real.shape)] = 0.0
        count += int(pad.count_nonzero())
    return count


def _solve_twice(case, algo, s, keep, fused=True):
    """Two runs of one solve on one problem (the buffers are cached per network): per run the hypergradient, the solution tensors
    (keep), the mixed coefficient and the launch counters' deltas."""
    from betty_amd import hypergradient as hg
    from betty_amd.backend import get_backend
    from betty_amd.hypergradient.structured import WeightedCEMLP

    assert not _native.is_ab()
    dims, B, seed = CASES[case][:3]
    ridge, step, K = SETTINGS[algo][s]
    curr, prev, vector = R.configured_problem(dims, B, ridge, K, step, seed, algo, dtype=torch.float32, device="cuda:0")
    curr.hypergradient_structure = lambda prev_: WeightedCEMLP(
        curr, prev_, layers=list(curr.module.layers), weight_fn=lambda ce: prev_.fwd(ce.reshape(-1, 1)), ridge=ridge,
        impl="hip", fused=fused, keep_solution=keep, verify=False)
    lib = _native.load()
    count = lambda: (lib.bhg_mlp_hoist_launches(), lib.bhg_mlp_proj_iterations(), lib.bhg_mlp_lin_launches())
    runs = []
    for _ in range(2):
        c0 = count()
        out = hg.jvp_fn_mapping[algo](vector, curr, prev, False)
        run = {"hypergradient": [t.detach().cpu().numpy() for t in out], "counters": tuple(a - b for a, b in zip(count(), c0))}
        run["coeff"] = _buffers(curr).coeff[:B].cpu().numpy()
        if keep:
            lay = get_backend().layout(vector)
            state = lay.state(3)[0] if algo == "cg" else lay.state(2)[1]   # x / p, as test_gpu_parity._run_solver reads them
            run["solution"] = [v.cpu().numpy() for v in lay.views(state, vector)]
            run["padding_nonzeros"] = _padding_nonzeros(curr, vector, algo)
        runs.append(run)
    return runs


@functools.lru_cache(maxsize=None)
def _gpu(case, algo, s, keep):
    """(the first run, {array: is the second run's bit-equal}, the second run's counters)."""
    first, second = _solve_twice(case, algo, s, keep)
    same = {k: all(np.array_equal(a, b) for a, b in zip(first[k], second[k])) for k in ("hypergradient", "solution") if k in first}
    same["coeff"] = np.array_equal(first["coeff"], second["coeff"])
    return first, same, second["counters"]


def _line(kind, case, algo, s, keep, rest):
    dims, B, seed = CASES[case][:3]
    ridge, step, K = SETTINGS[algo][s]
    return (f"SF64 {kind} dims={_id(dims)} B={B} seed={seed} ridge={ridge} step={step} K={K} algo={algo} keep={int(keep)} "
            f"form={_table(case, algo, keep)[0].split(' ')[0]}/{_table(case, algo, keep)[6]} {rest}")


def _unfused(case, algo, s):
    """The neighbouring form every shape has on the product library: K x (bhg_mlp_hvp + recurrence kernel), N-sized throughout."""
    return _solve_twice(case, algo, s, True, fused=False)[0]


def _verdict(err, other):
    return "the instance is at fault: take the next seed" if other * 2 >= err else "the fused form is at fault"


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True], ids=["free", "keep"])
@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_hypergradient_against_fp64(run, keep):
    """Hard gate rel <= 1e-4; tight gate rel <= max(1e-5, 4 spread).  A miss of the tight gate reports what the un-fused loop and the
    other keep_solution form give on the instance: within 2x the instance is at fault (next seed), otherwise the form is."""
    case, algo, s = run
    want, spread = _ref(case, algo, s)["hypergradient"], _e32(case, algo, s)[0]
    err = R.rel(_gpu(case, algo, s, keep)[0]["hypergradient"], want)
    tight = max(TIGHT_FLOOR, TIGHT_FACTOR * spread)
    print(_line("hg", case, algo, s, keep, f"spread={spread:.2e} kink_margin={_kink(case):.2e} rel={err:.2e} tight_gate={tight:.2e} "
                                           f"hard_gate={HARD:.0e}"))
    assert err <= HARD, err
    if err > tight:
        others = {"un-fused": R.rel(_unfused(case, algo, s)["hypergradient"], want),
                  "keep_solution=%s" % (not keep): R.rel(_gpu(case, algo, s, not keep)[0]["hypergradient"], want)}
        pytest.fail(f"rel {err:.2e} > tight gate {tight:.2e} (spread {spread:.2e}); " + ", ".join(f"{k} {v:.2e}" for k, v in others.items())
                    + ": " + _verdict(err, min(others.values())))


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_solution_tensor_by_tensor_against_fp64(run):
    """keep_solution=True: -cg_alpha x_K (CG) / -alpha p_K (Neumann) as the solver leaves it in the layout's state, each of the 2L
    tensors against plain CG / the plain Neumann series in fp64.  On the twin the caller's (un-padded) vector is compared and the
    padded elements of the twin's own vector are exactly zero."""
    case, algo, s = run
    want, e32 = _ref(case, algo, s)["solution"], _e32(case, algo, s)[1]
    got = _gpu(case, algo, s, True)[0]
    assert len(got["solution"]) == len(want) and all(g.shape == w.shape for g, w in zip(got["solution"], want))
    assert (got["padding_nonzeros"] == 0) if case == TWIN else (got["padding_nonzeros"] is None), got["padding_nonzeros"]
    errs = [_l2(g, w) for g, w in zip(got["solution"], want)]
    gates = [max(TIGHT_FLOOR, TIGHT_FACTOR * e) for e in e32]
    print(_line("sol", case, algo, s, True, " ".join(f"{n}:e32={e:.1e},rel={r:.1e},gate={g:.1e}" for n, e, r, g in zip(_names(case), e32, errs, gates))
                + f" hard_gate={HARD:.0e}"))
    bad = [(n, r, g) for n, r, g in zip(_names(case), errs, gates) if not (r <= g and r <= HARD)]
    if bad:
        other = dict(zip(_names(case), (_l2(g, w) for g, w in zip(_unfused(case, algo, s)["solution"], want))))
        pytest.fail("; ".join(f"{n}: rel {r:.2e} > gate {min(g, HARD):.2e}, un-fused {other[n]:.2e} ({_verdict(r, other[n])})" for n, r, g in bad))


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_mixed_coefficient_sample_by_sample_against_fp64(run):
    """keep_solution=False: buf.coeff[:B] after the solve (bhg_mlp_cg_mixed_coeff / bhg_mlp_neumann_mixed_coeff: from the Rz sums the
    solver accumulated) against (prob_b - onehot(y_b)) . Rz_b(solution) / B of the plain fp64 solve."""
    case, algo, s = run
    want, e32 = _ref(case, algo, s)["coeff"], _e32(case, algo, s)[2]
    got = _gpu(case, algo, s, False)[0]["coeff"]
    assert got.shape == want.shape == (CASES[case][1],)
    assert np.isfinite(got).all()
    err, gate = _max_err(got, want), max(ARRAY_GATE, TIGHT_FACTOR * e32)
    print(_line("coeff", case, algo, s, False, f"e32={e32:.2e} max_err={err:.2e} gate={gate:.2e} worst_sample="
                                               f"{int(np.abs(got.astype(np.float64) - want).argmax())}"))
    if not err <= gate:
        other = _max_err(_unfused(case, algo, s)["coeff"], want)
        pytest.fail(f"max|got - want| / max|want| = {err:.2e} > gate {gate:.2e} (e32 {e32:.2e}); un-fused {other:.2e}: {_verdict(err, other)}")


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True], ids=["free", "keep"])
@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_the_form_that_ran_is_the_one_in_the_table(run, keep):
    """The launch counters around each solve (bhg_mlp_hoist_launches, bhg_mlp_proj_iterations, bhg_mlp_lin_launches) are what the plan
    promises — test_the_description_is_what_the_library_then_does's arithmetic, extended to Neumann and keep_solution: one hoisted
    N-sized pass for a projected solve, K for a hoisted one, none for the classic chain; K - 1 (CG) / K (Neumann) projected iterations;
    k_wskpl once per iteration of the six-launch forms."""
    case, algo, s = run
    K = SETTINGS[algo][s][2]
    d, got = _plan(case, algo, keep)
    assert got == _table(case, algo, keep)
    want = (0 if not d["hoist"] else (1 if d["proj_level"] >= 1 else K),
            0 if d["proj_level"] == 0 else (K - 1 if algo == "cg" else K),
            K if d["lin"] else 0)
    assert d["hoist"] == (0 if got[0] == "classic" else 1) and (algo == "cg" or d["lin"] == 0)
    first, _, again = _gpu(case, algo, s, keep)
    assert first["counters"] == want and again == want, (got, first["counters"], again, want)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True], ids=["free", "keep"])
@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_a_second_run_on_the_same_buffers_is_bit_equal(run, keep):
    case, algo, s = run
    same = _gpu(case, algo, s, keep)[1]
    assert sorted(same) == (["coeff", "hypergradient", "solution"] if keep else ["coeff", "hypergradient"])
    assert all(same.values()), same

"""The head_j form of the projected CG iteration (csrc/bhg_mlp_headj.hip, mlp/head_body.inc under BHG_HEAD_J, hoist_head) held to an
fp64 reference of its own (tests/head_j_ref.py: the oracle's cg and a plain N-sized CG, nothing of the projected algebra) across the
shape family the plan gives it: batch <= 128, <= 12 classes, last hidden width <= 512.

Which case takes which branch (every line is asserted from plan / shape arithmetic in test_every_case_reaches_the_branch_it_is_here_for):

  branch                                                             case (dims, B)
  ------------------------------------------------------------------ ------------------------------------------------------------
  head_body.inc, `k0 > 0` reload of the J.Rh_1 loop (d_2 > 768)      [64,64,800,64,10], 37
  headj_tile, nct = d_2 / 32 split unevenly over four waves          [64,64,800,64,10], 37    (25 -> 6/6/6/7)
  headj_tile, idle waves (nch_w == 0): three / two                   [64,64,32,96,3], 24 and [64,64,32,32,2], 1 / [96,64,64,128,5], 32
  headj_tile, XCD remap (ntn & 7) == 0 with one / three / four groups [96,64,64,128,5], 32 / [64,96,160,384,12], 31 / [128,96,160,512,12], 128
  hoist_head, nt < B, clearing loop `z = t + nt; z < t2n`: one trip  [64,64,96,64,2], 32  (nt = 16; three trips on the 32 x 32 arm, nt = 8)
  hoist_head, nt < B, several trips on the default arm               [70,50,36,100,10], 97  (twin: d_3 = 128, nt = 32, t2n = 97)
  hoist_head, nt == B                                                [64,64,32,96,3], 24; [96,64,64,128,5], 32; [128,96,160,512,12], 128
  hoist_head, nt > B (partials behind the layers' own in partT2)     [64,96,160,384,12], 31 (nt = 96); [64,64,32,32,2], 1 (nt = 8)
  classes: min(wave + 4 j, C - 1) clamps, sD stride kHjC != C        C = 2, 3, 5, 10; C = kHjC = 12 (no clamp) twice
  B = 1 / 31 / 32 / 128 (one row, one short of a row tile, one tile, no padded row)   last / fifth / first and fourth / sixth case
  widths that are not multiples of 32 (zero-padded twin)             [70,50,36,100,10], 97

Seeds: sum(dims) + B, the next one where an instance misses a condition (head_j_ref.kink_margin >= 1.5e-6, reference fp32-vs-fp64
spread <= 2e-5 at all five settings, fp32 arrays within a quarter of the array gate):
  [128,96,160,512,12] B = 128: seed 1036 has a kink margin of 5.4e-7 -> 1037 (margin 1.54e-6).  No other seed was replaced.

Nothing after the last head launch writes Rh_2, Rd_2 or Rd_3: the backward chain (hoist_backward) writes Rd_1 and Rd_0, the last
iteration of a solve without a solution vector ends with its step length (chain_close: skip_outputs), and bhg_mlp_cg_mixed_coeff reads
the accumulated Rz(x) and writes the coefficient only.  All three arrays are therefore compared.

Measured errors: profiles/head_j_fp64.txt."""
import functools

import numpy as np
import pytest
import torch

import head_j_ref as R
from betty_amd import _native
from betty_amd.hypergradient import _mlp_hip

# (dims, B, seed)
CASES = [
    ([64, 64, 96, 64, 2], 32, 322),
    ([64, 64, 800, 64, 10], 37, 1039),
    ([64, 64, 32, 96, 3], 24, 283),
    ([96, 64, 64, 128, 5], 32, 389),
    ([64, 96, 160, 384, 12], 31, 747),
    ([128, 96, 160, 512, 12], 128, 1037),   # (1036: kink margin 5.4e-7)
    ([70, 50, 36, 100, 10], 97, 363),
    ([64, 64, 32, 32, 2], 1, 195),
]
# (ridge, cg_alpha, K): K = 1 builds no J; K = 2 is one head_j iteration; cg_alpha != 1 is the reference's quirk; ridge 0 is shift = 0
SETTINGS = [(0.3, 1.0, 1), (0.3, 1.0, 2), (0.3, 1.0, 5), (0.3, 0.5, 4), (0.0, 1.0, 3)]
ARRAY_SETTINGS = [(0.3, 1.0, 2), (0.3, 0.5, 4), (0.0, 1.0, 3)]
ARMS = {"default": {}, "tile32": {"HEAD_J_TILE": "0"}}

SPREAD_MAX, KINK_MIN = 2e-5, 1.5e-6      # tests/test_shapes_goldens.py's bounds on an instance
HARD, TIGHT_FLOOR, TIGHT_FACTOR = 1e-4, 1e-5, 4.0   # north_star's rtol; fused vs un-fused at cfg 2; another summation tree, one sample
ARRAY_GATE = 2e-5                        # test_mlp_hvp_kernels_vs_aten_and_autograd's

_id = lambda v: str(v).replace(" ", "")
_case_id = lambda c: f"{_id(c[0])}-B{c[1]}"
_set_id = lambda s: f"ridge{s[0]}-alpha{s[1]}-K{s[2]}"


# ---- the reference, computed once per instance and left unchanged ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hg64(case, s):
    dims, B, seed = CASES[case]
    out = R.hypergradient64(dims, B, *_rka(SETTINGS[s]), seed)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _spread(case, s):
    dims, B, seed = CASES[case]
    return R.rel([R.hypergradient32(dims, B, *_rka(SETTINGS[s]), seed)], _hg64(case, s))


@functools.lru_cache(maxsize=None)
def _kink(case):
    dims, B, seed = CASES[case]
    return R.kink_margin(dims, B, seed)


@functools.lru_cache(maxsize=None)
def _arrays64(case, s):
    dims, B, seed = CASES[case]
    out = R.last_iteration_arrays64(dims, B, *_rka(SETTINGS[s]), seed)
    for a in out.values():
        a.setflags(write=False)
    return out


def _rka(setting):
    ridge, alpha, K = setting
    return ridge, K, alpha   # head_j_ref's argument order


def _tiles(d3, shape):
    """headj_tiles at the padded batch of 128 rows: 32 x 16 tiles (shape 1, the default) or 32 x 32 (shape 0)."""
    return (128 // 32) * (d3 // (16 if shape else 32))


def _max_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: _case_id(CASES[i]))
def test_plain_cg_of_the_array_reference_reproduces_the_oracle(case):
    """last_iteration_arrays64 takes its direction from head_j_ref.plain_cg; carried to the hypergradient that CG gives the oracle's
    (hypergradient64) to 1e-9 at every setting — quirk, ridge 0 and K = 1 included."""
    dims, B, seed = CASES[case]
    for s, setting in enumerate(SETTINGS):
        curr, prev, vector = R.problem(dims, B, *_rka(setting), seed)
        err = R.rel([R.hypergradient_of_plain_cg(curr, prev, vector)], _hg64(case, s))
        assert err <= 1e-9, (setting, err)


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: _case_id(CASES[i]))
def test_every_instance_meets_its_conditions(case):
    dims, B, seed = CASES[case]
    assert dims[-1] >= 2, "one class: the softmax error is identically zero and the case proves nothing"
    assert _kink(case) >= KINK_MIN, _kink(case)
    for s, setting in enumerate(SETTINGS):
        assert np.linalg.norm(_hg64(case, s)) > 0.0
        assert _spread(case, s) <= SPREAD_MAX, (setting, _spread(case, s))
    assert all(s in SETTINGS for s in ARRAY_SETTINGS)


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: _case_id(CASES[i]))
def test_the_array_gate_is_one_a_correct_fp32_computation_meets(case):
    """The same arrays computed on the CPU in fp32 (plain CG, layer by layer) stay within a QUARTER of the gate the GPU is held to."""
    dims, B, seed = CASES[case]
    for setting in ARRAY_SETTINGS:
        want = _arrays64(case, SETTINGS.index(setting))
        got = R.last_iteration_arrays32(dims, B, *_rka(setting), seed)
        for name in ("Rh2", "Rd2", "Rd3"):
            assert np.abs(want[name]).max() > 0.0
            assert _max_err(got[name], want[name]) <= ARRAY_GATE / 4, (setting, name, _max_err(got[name], want[name]))


def test_every_case_reaches_the_branch_it_is_here_for(bhg_debug):
    """The docstring's table, from the plan and the kernels' own index arithmetic (bhg_mlp_headj.hip: headj_tile; bhg_mlp.hip: hoist_head)."""
    bhg_debug.setenv("BHG_PROJ_MAX_RATIO", "100000000")
    kdims = [list(_mlp_hip.padded_dims(dims)) for dims, _, _ in CASES]
    for (dims, B, _), kd in zip(CASES, kdims):
        assert _native.plan_describe(kd, B)["head_j"] == 1, (dims, B)
        assert B <= 128 and 2 <= kd[4] <= 12 and kd[3] <= 512 and kd[3] % 32 == 0 and kd[2] % 32 == 0
    waves = lambda d2: [(w + 1) * (d2 // 32) // 4 - w * (d2 // 32) // 4 for w in range(4)]   # nch_w of the four waves
    remap_groups = lambda d3: (d3 // 16) // 8 if (d3 // 16) & 7 == 0 else 0                       # 32 x 16 tiles: ntn = d_3 / 16
    B_of = [c[1] for c in CASES]
    # 0: C = 2, one row tile, nt < B with the clearing loop (one trip; three on the 32 x 32 arm)
    assert kdims[0][4] == 2 and B_of[0] == 32 and _tiles(kdims[0][3], 1) == 16 < B_of[0] and _tiles(kdims[0][3], 0) == 8
    assert len(range(0 + 16, B_of[0], 16)) == 1 and len(range(0 + 8, B_of[0], 8)) == 3
    # 1: the second trip of the J.Rh_1 loop (three batches of 256 k per trip), 25 k-chunks over four waves
    assert kdims[1][2] > 768 and waves(kdims[1][2]) == [6, 6, 6, 7]
    # 2: three idle waves, nt == B, odd C
    assert waves(kdims[2][2]) == [0, 0, 0, 1] and _tiles(kdims[2][3], 1) == B_of[2] == 24 and kdims[2][4] % 2 == 1
    # 3: two idle waves, the remap with one group, nt == B
    assert waves(kdims[3][2]).count(0) == 2 and remap_groups(kdims[3][3]) == 1 and _tiles(kdims[3][3], 1) == B_of[3] == 32
    # 4: the remap with three groups, nt > B, C = kHjC, B one short of a row tile
    assert remap_groups(kdims[4][3]) == 3 and _tiles(kdims[4][3], 1) == 96 > B_of[4] == 31 and kdims[4][4] == 12
    # 5: the widest head, four groups, nt == B, no padded row
    assert kdims[5][3] == 512 and remap_groups(512) == 4 and _tiles(512, 1) == B_of[5] == 128 and kdims[5][4] == 12
    # 6: the zero-padded twin; nt < B with several trips of the clearing loop on the default arm
    assert kdims[6] != CASES[6][0] and kdims[6] == [96, 64, 64, 128, 10] and _tiles(kdims[6][3], 1) == 32
    assert len(range(0 + 32, B_of[6], 32)) == 3 and len(range(31 + 32, B_of[6], 32)) == 2
    # 7: one sample, the smallest d_3 (no remap: ntn = 2), three idle waves, nt > B
    assert B_of[7] == 1 and kdims[7][3] == 32 and remap_groups(32) == 0 and waves(kdims[7][2]) == [0, 0, 0, 1] and _tiles(32, 1) == 8 > 1
    assert sorted({kd[4] for kd in kdims}) == [2, 3, 5, 10, 12]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _gpu_problem(case, setting):
    from betty_amd.hypergradient.structured import WeightedCEMLP

    dims, B, seed = CASES[case]
    ridge, alpha, K = setting
    curr, prev, vector = R.problem(dims, B, ridge, K, alpha, seed, dtype=torch.float32, device="cuda:0")
    curr.hypergradient_structure = lambda prev_: WeightedCEMLP(
        curr, prev_, layers=list(curr.module.layers), weight_fn=lambda ce: prev_.fwd(ce.reshape(-1, 1)), ridge=ridge,
        impl="hip", fused=True, keep_solution=False, verify=False)
    return curr, prev, vector


def _solve(curr, prev, vector, K):
    """One solution-free fused CG solve; the launch counters prove which form ran: K k_wskpl launches, K - 1 projected iterations."""
    from betty_amd import hypergradient as hg

    lib = _native.load()
    l0, p0 = lib.bhg_mlp_lin_launches(), lib.bhg_mlp_proj_iterations()
    out = [t.detach().cpu().numpy() for t in hg.jvp_fn_mapping["cg"](vector, curr, prev, False)]
    return out, (lib.bhg_mlp_lin_launches() - l0, lib.bhg_mlp_proj_iterations() - p0)


def _arm(bhg_debug, env, head_j=1, case=None):
    bhg_debug.reset()
    bhg_debug.setenv("BHG_PROJ_MAX_RATIO", "100000000")   # (the form is under test, not the cost model that gates projection)
    for k, v in env.items():
        bhg_debug.setenv(k, v)
    dims, B, _ = CASES[case]
    assert _native.plan_describe(_mlp_hip.padded_dims(dims), B)["head_j"] == head_j, (dims, B, env)


def _buffers(curr):
    """The device buffers of the net — of its zero-padded twin where it runs on one."""
    first = curr.module.layers[0]
    if first in _mlp_hip._TWINS:
        (twin,) = _mlp_hip._TWINS[first].values()
        first = twin.layers[0]
    (buf,) = _mlp_hip._BUFFERS[first].values()
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("setting", SETTINGS, ids=_set_id)
@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: _case_id(CASES[i]))
def test_hypergradient_against_fp64(case, setting, arm, bhg_debug):
    """Hard gate rel <= 1e-4 (north_star's rtol); tight gate rel <= max(1e-5, 4 * spread), spread = the reference's own fp32-vs-fp64
    error on this instance.  A miss of the tight gate reports what the six-launch form and the classic chain give on the instance:
    within 2x the instance is at fault (next seed), otherwise k_headj is."""
    dims, B, seed = CASES[case]
    ridge, alpha, K = setting
    s = SETTINGS.index(setting)
    want, spread = _hg64(case, s), _spread(case, s)
    _arm(bhg_debug, ARMS[arm], case=case)
    got, counters = _solve(*_gpu_problem(case, setting), K)
    assert counters == (K, K - 1), counters
    err = R.rel(got, want)
    tight = max(TIGHT_FLOOR, TIGHT_FACTOR * spread)
    print(f"HJ64 hg dims={_id(dims)} B={B} seed={seed} ridge={ridge} alpha={alpha} K={K} arm={arm} spread={spread:.2e} "
          f"kink_margin={_kink(case):.2e} rel={err:.2e} tight_gate={tight:.2e} hard_gate={HARD:.0e}")
    assert err <= HARD, err
    if err > tight:
        others = {}
        for name, env in (("six", {"HEAD_J": "0"}), ("classic", {"BHG_MLP_HOIST": "0"})):
            _arm(bhg_debug, env, head_j=0, case=case)
            others[name] = R.rel(_solve(*_gpu_problem(case, setting), K)[0], want)
        pytest.fail(f"rel {err:.2e} > tight gate {tight:.2e} (spread {spread:.2e}); six launches {others['six']:.2e}, classic chain "
                    f"{others['classic']:.2e}: {'the instance' if min(others.values()) * 2 >= err else 'k_headj'} is at fault")


@pytest.mark.gpu
@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("setting", ARRAY_SETTINGS, ids=_set_id)
@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: _case_id(CASES[i]))
def test_arrays_of_the_last_iteration_against_fp64(case, setting, arm, bhg_debug):
    """Rh_2 (the tiles), Rd_3 and Rd_2 (the head rows through J) as the LAST head_j launch of a solve leaves them, against the fp64
    R-forward / R-backward of plain CG's direction p_{K-1}: NaN before the solve, finite after it, rows >= B exactly zero, rows < B
    within max|got - want| <= 2e-5 max|want|.  Nothing after that launch writes the three arrays (module docstring).  On the ragged
    net the twin's real columns are compared; its padded columns are exactly zero."""
    dims, B, seed = CASES[case]
    ridge, alpha, K = setting
    want = _arrays64(case, SETTINGS.index(setting))
    _arm(bhg_debug, ARMS[arm], case=case)
    curr, prev, vector = _gpu_problem(case, setting)
    _solve(curr, prev, vector, K)                      # allocates the buffers
    buf = _buffers(curr)
    assert buf.BP == 128 and tuple(buf.dims) == _mlp_hip.padded_dims(dims)
    arrays = {"Rh2": buf.Rh[2], "Rd2": buf.Rd[2], "Rd3": buf.Rd[3]}
    for a in arrays.values():
        a.fill_(float("nan"))
    out, counters = _solve(curr, prev, vector, K)
    assert counters == (K, K - 1), counters
    assert all(np.isfinite(o).all() for o in out)
    errs = {}
    for name, dev in arrays.items():
        got = dev.cpu().numpy().astype(np.float64)
        cols = want[name].shape[1]
        assert got.shape == (128, {"Rh2": buf.dims[3], "Rd2": buf.dims[3], "Rd3": dims[4]}[name]) and want[name].shape[0] == B
        assert np.isfinite(got).all(), f"{name}: every element must be written by the last iteration"
        assert not got[B:].any(), f"{name}: rows >= B must be exactly zero"
        assert not got[:, cols:].any(), f"{name}: padded columns must be exactly zero"
        errs[name] = _max_err(got[:B, :cols], want[name])
    print(f"HJ64 arr dims={_id(dims)} B={B} seed={seed} ridge={ridge} alpha={alpha} K={K} arm={arm} "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f" array_gate={ARRAY_GATE:.0e}")
    assert max(errs.values()) <= ARRAY_GATE, errs

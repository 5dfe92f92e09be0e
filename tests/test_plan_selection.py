"""The map "shape -> solver form" (the plan logic had no unit test of its own beyond launch counters).

``bhg_mlp_plan_describe`` (include/bhg.h) evaluates the host logic that picks the form — hoist_plan's shape rules and cost model,
plan_solve (csrc/mlp/solve_plan.inc: projection level, the chain's first product by linearity, the head launch with the recurrences, the closing
launch) — WITHOUT launching anything, so this file runs on the CPU box.  The GPU half ties the description to what the library then
does: the launch counters of a real solve on the same shapes."""
import pytest

from betty_amd import _native
from betty_amd.hypergradient import _mlp_hip

SIX = "six-launch (k_wskpl .. k_headu .. k_graw)"
SIX_CLASS = "six-launch-class (k_wskpl first, recurrences beside the chain)"
PSTEP = "fully-projected (k_pstep launch)"
NEU = "projected-neumann (update inside k_graw)"

# (dims the kernels see, batch) -> cg solution-free, cg with x, neumann solution-free, neumann with accumulator; closing launch of the projected forms
CASES = [
    # the metric workload and its family: four layers, narrow head (<= 12 classes, last hidden width <= 512): the six-launch form
    ([3072, 2048, 1536, 384, 10], 100, SIX, "projected-keep-state", NEU, "classic", "k_graw"),
    ([800, 512, 256, 128, 10], 100, SIX, "projected-keep-state", NEU, "classic", "k_graw"),         # the padded twin of 784-512-256-128-10
    ([512, 256, 256, 64, 10], 128, SIX, "projected-keep-state", NEU, "classic", "k_graw"),
    # batches beyond 128 rows: the K-looped closing launch
    ([512, 256, 256, 64, 10], 200, SIX, "projected-keep-state", NEU, "classic", "k_grawk"),
    ([256, 256, 128, 64, 10], 256, SIX, "projected-keep-state", NEU, "classic", "k_grawk"),
    # four layers whose head the head-with-recurrences launch does not take (last hidden layer > 512 wide; more than 12 classes)
    ([256, 256, 192, 640, 10], 100, SIX_CLASS, "projected-keep-state", NEU, "classic", "k_graw"),
    ([256, 256, 128, 64, 24], 100, SIX_CLASS, "projected-keep-state", NEU, "classic", "k_graw"),
    # deeper than four layers: k_wskpl with its update blocks behind the publisher
    ([256, 256, 256, 256, 128, 10], 100, SIX_CLASS, "projected-keep-state", NEU, "classic", "k_graw"),
    ([512, 512, 256, 256, 128, 10], 300, SIX_CLASS, "projected-keep-state", NEU, "classic", "k_grawk"),
    ([256, 192, 128, 64, 32, 10], 300, "hoisted", "hoisted", "hoisted", "classic", None),   # (the same depth, narrow: the cost model declines — B^2 Gram work)
    # three layers: no product between the first and the pre-head one -> the k_pstep launch stays
    ([256, 384, 128, 10], 100, PSTEP, "projected-keep-state", NEU, "classic", "k_graw"),
    # the cost model: a batch wider than the narrowest hidden layer, or eight narrow layers -> hoisted chain, no projection
    ([256, 384, 128, 10], 1024, "hoisted", "hoisted", "hoisted", "classic", None),
    ([64, 96, 64, 32, 64, 96, 32, 64, 10], 50, "hoisted", "hoisted", "hoisted", "classic", None),
    # two layers, or widths that are not multiples of 32 (as the kernels would see them WITHOUT the twin): the classic chain
    ([256, 192, 10], 128, "classic", "classic", "classic", "classic", None),
    ([784, 512, 256, 128, 10], 100, "classic", "classic", "classic", "classic", None),
    ([70, 130, 36, 10], 100, "classic", "classic", "classic", "classic", None),
]


@pytest.mark.parametrize("dims,B,cg_free,cg_x,neu_free,neu_acc,closing", CASES, ids=lambda v: str(v) if isinstance(v, (list, int)) else None)
def test_shape_to_form(dims, B, cg_free, cg_x, neu_free, neu_acc, closing):
    got = {(a, k): _native.plan_describe(dims, B, a, k) for a in ("cg", "neumann") for k in (False, True)}
    assert all(v["fused"] == 1 and v["narrow_head"] == 1 for v in got.values())
    assert got[("cg", False)]["form"] == cg_free and got[("cg", True)]["form"] == cg_x
    assert got[("neumann", False)]["form"] == neu_free and got[("neumann", True)]["form"] == neu_acc
    d = got[("cg", False)]
    assert d["lin"] == (1 if cg_free in (SIX, SIX_CLASS) else 0) and d["lin_head"] == (1 if cg_free == SIX else 0)
    assert d["upd_first"] == (1 if (cg_free == SIX_CLASS and len(dims) - 1 > 4) else 0)
    assert d["proj_level"] == (2 if cg_free in (SIX, SIX_CLASS, PSTEP) else 0)
    assert got[("cg", True)]["proj_level"] == (1 if cg_x == "projected-keep-state" else 0)
    if closing is not None:
        assert d["closing"] == closing == got[("neumann", False)]["closing"]
        assert d["gram_floats"] > 0
    else:
        assert d["gram_floats"] == 0, "no Gram region is carved when the plan does not project"
    # the packed once-per-step passes go with the hoisted plan
    assert d["packed_prepare"] == d["plan_ok"]
    # round 6: the global-batch solve (Config(type="cg_global")) exchanges batch-sized factors exactly where the plan projects and the
    # caller does not ask for x; the slab the ranks gather per iteration holds Rd_0 .. Rd_{L-1}, Rh_0 .. Rh_{L-2} of the padded batch
    assert d["global_form"] == ("factor-exchange" if d["proj_level"] == 2 else "one-pass")
    assert got[("cg", True)]["global_form"] == "one-pass"
    if d["proj_level"] == 2:
        Bp = (B + 127) // 128 * 128
        assert d["fx_slab_bytes"] >= 4 * Bp * (sum(dims[1:]) + sum(dims[1:-1])) and d["fx_ws_bytes_world8"] > 0
    else:
        assert d["fx_slab_bytes"] == 0 and d["fx_ws_bytes_world8"] == 0


# ---- every debug key the plan reads: arm -> form, as literals (taken from the library before plan_solve existed) ------------------------
# (form, proj_level, lin, lin_head, head_j, closing) of the solution-free CG plan and of the solution-free Neumann plan
G, GK, HP = "k_graw", "k_grawk", "k_hoist+k_proj_update"


def _six(closing, head_j=0):
    return (SIX, 2, 1, 1, head_j, closing)


def _six_class(closing):
    return (SIX_CLASS, 2, 1, 0, 0, closing)


def _pstep(closing):
    return (PSTEP, 2, 0, 0, 0, closing)


def _keep(closing):
    return ("projected-keep-state", 1, 0, 0, 0, closing)


def _neu(closing):
    return (NEU, 1, 0, 0, 0, closing)


def _off(form):
    return (form, 0, 0, 0, 0, "k_outer_all")


ARM_SHAPES = [([3072, 2048, 1536, 384, 10], 100), ([256, 384, 128, 10], 100), ([256, 256, 256, 256, 128, 10], 100), ([512, 256, 256, 64, 10], 200)]
ARM_DEFAULT = [(_six(G, 1), _neu(G)), (_pstep(G), _neu(G)), (_six_class(G), _neu(G)), (_six(GK), _neu(GK))]   # (head_j: a padded batch of 128 only)
_ALL_PSTEP = [(_pstep(G), _neu(G)), None, (_pstep(G), _neu(G)), (_pstep(GK), _neu(GK))]           # both six-launch forms fall back to the k_pstep launch
_HEAD_OUT = [(_six_class(G), _neu(G)), None, None, (_six_class(GK), _neu(GK))]                     # the update blocks leave the head launch
# one row per arm: the four shapes in order, None = as the default arm
ARM_FORMS = {
    None: [None] * 4,
    ("mlp_proj", 0): [(_off("hoisted"), _off("classic"))] * 4,
    ("mlp_proj", 9): [(_keep(G), _neu(G))] * 3 + [(_keep(GK), _neu(GK))],
    ("mlp_hoist", 0): [(_off("classic"), _off("classic"))] * 4,
    ("mlp_hoist", 2): [None] * 4,
    ("cg_eager_p", 1): [(_off("classic-eager"), _neu(G))] * 3 + [(_off("classic-eager"), _neu(GK))],   # Neumann stays projected
    ("lin_first", 0): _ALL_PSTEP,
    ("lin_update_next", 0): _HEAD_OUT,
    ("lin_update_in_head", 0): _HEAD_OUT,
    ("lin_nub", 1): _HEAD_OUT,
    ("head_no_prefetch", 1): _HEAD_OUT,
    ("head_j", 0): [(_six(G, 0), _neu(G)), None, None, None],
    ("packed_chain", 0): _ALL_PSTEP,
    ("packed_gram", 0): _ALL_PSTEP,
    ("graw_v2", 0): _ALL_PSTEP,
    ("graw_kloop", 0): [None, None, None, (_pstep(HP), _neu(HP))],
    ("rnew_in_graw", 0): _ALL_PSTEP,
    ("alpha_in_hoist", 0): _ALL_PSTEP,
    ("proj_small_alone", 1): _ALL_PSTEP,
    ("proj_step_alone", 1): _ALL_PSTEP,
    ("pstep_v2", 0): _ALL_PSTEP,
    ("lin_deep", 0): [None, None, (_pstep(G), _neu(G)), None],
    ("neumann_vnew", 0): [None] * 4,
    ("cg_rhs_direct", 0): [None] * 4,
    ("mlp_no_head", 1): [(_off("unfused"), _off("unfused"))] * 4,
    ("mlp_no_fused_solve", 1): [(_off("unfused"), _off("unfused"))] * 4,
    ("proj_max_ratio", 50): [None] + [(_off("hoisted"), _off("hoisted"))] * 3,
}


def _plan_tuple(d):
    return (d["form"], d["proj_level"], d["lin"], d["lin_head"], d["head_j"], d["closing"])


@pytest.mark.parametrize("arm", list(ARM_FORMS), ids=lambda a: "default" if a is None else f"{a[0]}={a[1]}")
def test_arm_to_form(arm, bhg_debug):
    if arm is not None:
        bhg_debug.setenv(*arm)
    for (dims, B), want, dflt in zip(ARM_SHAPES, ARM_FORMS[arm], ARM_DEFAULT):
        got = (_plan_tuple(_native.plan_describe(dims, B, "cg")), _plan_tuple(_native.plan_describe(dims, B, "neumann")))
        assert got == (want or dflt), (arm, dims, B)


def _state_mask(dims, B, has_x):
    d = _native.Mlp()
    d.L, d.B, d.Bp = len(dims) - 1, int(B), (int(B) + 127) // 128 * 128
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    import ctypes

    return int(_native.load().bhg_mlp_cg_state_mask(ctypes.byref(d), has_x))


@pytest.mark.parametrize("dims,B", [(c[0], c[1]) for c in CASES], ids=lambda v: str(v))
def test_state_mask_follows_the_plan(dims, B):
    """The tensors bhg_mlp_cg_solve_rhs reads from the flat state: all of them unless the solution-free CG plan is fully projected —
    then exactly the biases and the head weight (bit 2 (L - 1))."""
    L = len(dims) - 1
    ones = (1 << 64) - 1
    want = ones
    if _native.plan_describe(dims, B, "cg")["proj_level"] == 2:
        want = sum(1 << (2 * l + 1) for l in range(L)) | 1 << (2 * (L - 1))
    assert _state_mask(dims, B, 0) == want
    assert _state_mask(dims, B, 1) == ones


def test_wide_head_has_no_fused_solver_and_the_twin_rounds_widths_up():
    d = _native.plan_describe([192, 256, 128, 1000], 72)               # beyond the head kernels' 256 classes
    assert (d["fused"], d["narrow_head"], d["form"]) == (0, 0, "unfused")
    d = _native.plan_describe([256, 384, 128, 100], 100)               # round 6: a 100-class head takes the fused forms
    assert (d["fused"], d["narrow_head"], d["form"]) == (1, 1, PSTEP)
    assert _native.plan_describe([512, 256, 256, 64, 100], 100)["form"] == SIX_CLASS
    assert _native.plan_describe([192, 256, 132, 10], 72)["form"] == "classic"      # feature width % 32 != 0 as the kernels see it ...
    assert _native.plan_describe([192, 256, 130, 10], 72)["form"] == "unfused"      # (% 4 != 0: not even the narrow-head kernels)
    assert _mlp_hip.padded_dims([192, 256, 130, 10]) == (192, 256, 160, 10)          # ... so the host side hands them the twin
    assert _native.plan_describe(_mlp_hip.padded_dims([192, 256, 130, 10]), 72)["form"] == PSTEP
    assert _mlp_hip.padded_dims([784, 512, 250, 100, 10]) == (800, 512, 256, 128, 10)
    assert _mlp_hip.padded_dims([3072, 2048, 1536, 384, 10]) == (3072, 2048, 1536, 384, 10)
    with pytest.raises(_native.NativeLibraryError):
        _native.plan_describe([10], 5)   # no layer


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B", [([512, 256, 256, 64, 10], 128), ([256, 384, 128, 10], 100), ([784, 512, 256, 128, 10], 100),
                                    ([256, 256, 256, 256, 128, 10], 100), ([256, 192, 10], 128), ([256, 384, 128, 10], 1024)], ids=lambda v: str(v))
def test_the_description_is_what_the_library_then_does(dims, B):
    """A real solve on the same shapes: the launch counters agree with the description (cg without a solution vector)."""
    import sys
    import os

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_gpu_parity as tgp

    lib = _native.load()
    K = 4
    d = _native.plan_describe(_mlp_hip.padded_dims(dims) if len(dims) - 1 >= 3 else dims, B)
    h0, p0, l0 = lib.bhg_mlp_hoist_launches(), lib.bhg_mlp_proj_iterations(), lib.bhg_mlp_lin_launches()
    tgp._run_solver("cg", dims, B, 0.5, K, 7, True, keep=False)
    dh, dp, dl = lib.bhg_mlp_hoist_launches() - h0, lib.bhg_mlp_proj_iterations() - p0, lib.bhg_mlp_lin_launches() - l0
    want_h = 0 if not d["hoist"] else (1 if d["proj_level"] >= 1 else K)
    assert (dh, dp, dl) == (want_h, (K - 1) if d["proj_level"] == 2 else 0, K if d["lin"] else 0), (d, dh, dp, dl)

"""The last iteration of a fused CG solve without a solution vector (csrc/bhg_mlp.hip: hoist_backward; csrc/bhg_mlp_tail.hip: k_t2_dots)
and the one set-up launch of the head_j form (csrc/bhg_mlp_headj.hip: k_headj_pack's two chores).

Nothing reads the R-backward products of that iteration, so the solve launches k_t2_dots in their place: the same second-order shares
T2_l = 2 <Gb_l(p), Rh_{l-1}(p)> of p.Hp, from the same operands, into the same slots of partT2.  The measurement build keeps the
products behind the key cg_last_backward = 1 — the PARENT ARM every solve here is compared against — and the runtime's memset + copy
behind head_j_setup = 0.

Against the parent arm the only difference is the order of an fp64 sum (the tiles' partials against the flat partition's): at most one
fp32 ulp in alpha_{K-1}, which scales the last direction's share of the result — gate 1.2e-6 relative L2 (10 x fp32 epsilon) on the
hypergradient and on the mixed coefficient.  Against fp64 the gates are tests/test_solver_forms_fp64.py's own (imported), on that
file's settings.  Measured: profiles/cg_last_iteration_fp64.txt.

Nets: [64,64,96,384,12] at B = 96 (head_j, 16 x 16 tiles) and B = 31 (head_j, 32 x 16 tiles, their T2h partials BEHIND the layers' in
partT2: the slot contract); [64,64,96,64,12] at B = 33 and 97 (a strip of one row behind a full row tile); [256,256,128,64,24] at
B = 100 (six-launch, no head_j); [256,256,128,128,64,10] at B = 100 (five layers: three dot products in one launch);
[64,64,32,10] at B = 17 with packed_chain = 0 (two hidden layers, the hoisted chain on row-major operands: launch_gemm_wsk's slots).
The last three are cases of tests/test_solver_forms_fp64.py, with its seeds; the small head_j nets need the cost model's gate lifted
(proj_max_ratio), like every test of that form.  Seeds: sum(dims) + B, the next one where the instance misses a condition
(test_every_instance_meets_its_conditions)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import solver_forms_ref as R
import test_solver_forms_fp64 as G   # the gates (HARD, TIGHT_*, ARRAY_GATE), the instance conditions, _buffers
from betty_amd import Config, _native
from betty_amd.hypergradient import _mlp_hip

LIFT = {"BHG_PROJ_MAX_RATIO": "100000000"}
# (dims, B, seed, keys the FORM needs, head_j, head_j_tile)
NETS = [
    ([64, 64, 96, 384, 12], 96, 716, LIFT, 1, 2),
    ([64, 64, 96, 384, 12], 31, 651, LIFT, 1, 1),
    ([64, 64, 96, 64, 12], 33, 333, LIFT, 1, 2),
    ([64, 64, 96, 64, 12], 97, 397, LIFT, 1, 2),
    ([256, 256, 128, 64, 24], 100, 829, {}, 0, -1),
    ([256, 256, 128, 128, 64, 10], 100, 942, {}, 0, -1),
    ([64, 64, 32, 10], 17, 187, {"BHG_PACKED_CHAIN": "0"}, 0, -1),
]
KS, RIDGES, ALPHAS = (1, 2, 3, 5), (0.3, 0.0), (1.0, 0.5)
ARM_GATE = 1.2e-6                       # 10 x fp32 epsilon: one ulp of alpha_{K-1}, with room
FP64_SETTINGS = G.SETTINGS["cg"]        # (ridge, cg_alpha, K)

_id = lambda v: str(v).replace(" ", "")
_net_id = lambda n: f"{_id(NETS[n][0])}-B{NETS[n][1]}"


# ---- the reference, computed once per (net, setting) and left unchanged ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(net, s, fp64=True):
    dims, B, seed = NETS[net][:3]
    ridge, alpha, K = FP64_SETTINGS[s]
    q = R.quantities(dims, B, ridge, K, alpha, seed, "cg", torch.float64 if fp64 else torch.float32)
    out = {"hypergradient": q["hypergradient"], "coeff": q["coeff"]}
    for a in out.values():
        a.setflags(write=False)
    return out


def _e32(net, s):
    q32, q64 = _ref(net, s, False), _ref(net, s)
    return R.rel([q32["hypergradient"]], q64["hypergradient"]), G._max_err(q32["coeff"], q64["coeff"])


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_the_sweep_is_the_one_the_kernel_can_go_wrong_on(bhg_debug):
    """The forms, from the plan: head_j with either tile shape, six-launch without head_j, five layers, and the hoisted chain on
    row-major operands; K = 1 (iteration 0 is also the last one) is in the sweep; B covers a full padded batch row tile, one row
    short of a tile, one row beyond a tile."""
    assert 1 in KS and 2 in KS and 0.0 in RIDGES and 0.5 in ALPHAS
    for dims, B, _, env, head_j, tile in NETS:
        bhg_debug.reset()
        for k, v in env.items():
            bhg_debug.setenv(k, v)
        d = _native.plan_describe(list(_mlp_hip.padded_dims(dims)), B)
        assert (d["head_j"], d["head_j_tile"], d["hoist"]) == (head_j, tile, 1), (dims, B, d)
        assert list(_mlp_hip.padded_dims(dims)) == dims
    assert {len(n[0]) - 1 for n in NETS} == {3, 4, 5}
    bhg_debug.reset()
    bhg_debug.setenv("BHG_PACKED_CHAIN", "0")
    assert _native.plan_describe(NETS[6][0], NETS[6][1])["form"] == "hoisted"
    # 32 x 16 tiles at B = 31: 96 partials of the head launch, more than B — they sit behind the layers' own slots
    assert (128 // 32) * (384 // 16) > 31
    assert {n[1] % 32 for n in NETS} >= {0, 31, 1}


@pytest.mark.parametrize("net", range(len(NETS)), ids=_net_id)
def test_every_instance_meets_its_conditions(net):
    dims, B, seed = NETS[net][:3]
    assert R.kink_margin(dims, B, seed) >= G.KINK_MIN
    for s, setting in enumerate(FP64_SETTINGS):
        spread, e_coeff = _e32(net, s)
        print(f"CGL instance dims={_id(dims)} B={B} seed={seed} setting={setting} spread={spread:.2e} e32_coeff={e_coeff:.2e}")
        assert np.linalg.norm(_ref(net, s)["hypergradient"]) > 0.0 and np.abs(_ref(net, s)["coeff"]).max() > 0.0
        assert spread <= G.SPREAD_MAX and e_coeff <= G.SPREAD_MAX, (setting, spread, e_coeff)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _arm(bhg_debug, net, **keys):
    bhg_debug.reset()
    for k, v in NETS[net][3].items():
        bhg_debug.setenv(k, v)
    for k, v in keys.items():
        bhg_debug.setenv(k, str(v))


def _declare(curr, ridge):
    from betty_amd.hypergradient.structured import WeightedCEMLP

    curr.hypergradient_structure = lambda prev_: WeightedCEMLP(
        curr, prev_, layers=list(curr.module.layers), weight_fn=lambda ce: prev_.fwd(ce.reshape(-1, 1)), ridge=ridge,
        impl="hip", fused=True, keep_solution=False, verify=False)


def _gpu_problem(net, ridge, K, alpha):
    dims, B, seed = NETS[net][:3]
    curr, prev, vector = R.problem(dims, B, ridge, K, alpha, seed, dtype=torch.float32, device="cuda:0")
    _declare(curr, ridge)
    return curr, prev, vector


def _solve(curr, prev, vector):
    """One solution-free fused CG solve: hypergradient and mixed coefficient as fp64 numpy, the launch counters' deltas."""
    from betty_amd import hypergradient as hg

    lib = _native.load()
    count = lambda: (lib.bhg_mlp_hoist_launches(), lib.bhg_mlp_proj_iterations(), lib.bhg_mlp_lin_launches())
    c0 = count()
    out = R.flat(hg.jvp_fn_mapping["cg"](vector, curr, prev, False))
    counters = tuple(a - b for a, b in zip(count(), c0))
    B = curr.cur_batch[0].shape[0]
    return out, G._buffers(curr).coeff[:B].cpu().numpy().astype(np.float64), counters


def _live_and_dead(buf):
    """What the last iteration must leave as the parent does (every Rh_l; Rd_{L-1}, Rd_{L-2}: the head launch) / what it no longer writes."""
    L = len(buf.Rd)
    live = {f"Rh{l}": buf.Rh[l] for l in range(L - 1)}
    live.update({f"Rd{l}": buf.Rd[l] for l in (L - 2, L - 1)})
    return live, [buf.Rd[l] for l in range(L - 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("net", range(len(NETS)), ids=_net_id)
def test_against_the_parent_arm(net, bhg_debug):
    """K x ridge x cg_alpha: hypergradient and mixed coefficient within 1.2e-6 of the arm that still runs the backward products; every
    Rh_l and the head launch's Rd bit-equal to it; Rd_{l < L-2} NaN before the solve — they stay NaN at K = 1, the result is finite; the same
    launch counters."""
    dims, B = NETS[net][:2]
    worst = (0.0, 0.0)
    for ridge in RIDGES:
        for alpha in ALPHAS:
            for K in KS:
                curr, prev, vector = _gpu_problem(net, ridge, K, alpha)
                _arm(bhg_debug, net, CG_LAST_BACKWARD=1)
                hg_p, coeff_p, count_p = _solve(curr, prev, vector)
                live, dead = _live_and_dead(G._buffers(curr))
                assert all(torch.isfinite(a).all() for a in dead), "the parent arm writes every Rd_l"
                kept = {k: a.clone() for k, a in live.items()}
                for a in dead:
                    a.fill_(float("nan"))
                _arm(bhg_debug, net)
                hg_n, coeff_n, count_n = _solve(curr, prev, vector)
                assert np.isfinite(hg_n).all() and np.isfinite(coeff_n).all(), (ridge, alpha, K)
                assert count_n == count_p, (ridge, alpha, K, count_n, count_p)
                for k, a in live.items():
                    assert torch.equal(a, kept[k]), f"{k} of the last iteration differs from the parent arm's (ridge={ridge} alpha={alpha} K={K})"
                if K == 1:   # (no earlier iteration wrote them either: the backward launches are gone)
                    assert all(torch.isnan(a).all() for a in dead), "the last iteration no longer writes Rd_l, l < L - 2"
                e_hg, e_c = R.rel([hg_n], hg_p), G._l2(coeff_n, coeff_p)
                print(f"CGL arms dims={_id(dims)} B={B} ridge={ridge} alpha={alpha} K={K} rel_hg={e_hg:.2e} rel_coeff={e_c:.2e} gate={ARM_GATE:.1e}")
                worst = (max(worst[0], e_hg), max(worst[1], e_c))
                assert e_hg <= ARM_GATE and e_c <= ARM_GATE, (ridge, alpha, K, e_hg, e_c)
    print(f"CGL arms-max dims={_id(dims)} B={B} rel_hg={worst[0]:.2e} rel_coeff={worst[1]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("net", range(len(NETS)), ids=_net_id)
def test_against_fp64(net, bhg_debug):
    """tests/test_solver_forms_fp64.py's gates on its own settings: hypergradient rel <= 1e-4 and <= max(1e-5, 4 spread); mixed
    coefficient max error <= max(2e-5, 4 e32) of the largest coefficient."""
    dims, B, seed = NETS[net][:3]
    for s, (ridge, alpha, K) in enumerate(FP64_SETTINGS):
        _arm(bhg_debug, net)
        hg_n, coeff_n, _ = _solve(*_gpu_problem(net, ridge, K, alpha))
        spread, e32 = _e32(net, s)
        err, tight = R.rel([hg_n], _ref(net, s)["hypergradient"]), max(G.TIGHT_FLOOR, G.TIGHT_FACTOR * spread)
        err_c, gate_c = G._max_err(coeff_n, _ref(net, s)["coeff"]), max(G.ARRAY_GATE, G.TIGHT_FACTOR * e32)
        print(f"CGL fp64 dims={_id(dims)} B={B} seed={seed} ridge={ridge} alpha={alpha} K={K} spread={spread:.2e} rel={err:.2e} "
              f"tight_gate={tight:.2e} hard_gate={G.HARD:.0e} e32_coeff={e32:.2e} coeff_err={err_c:.2e} coeff_gate={gate_c:.2e}")
        assert err <= G.HARD and err <= tight, (ridge, alpha, K, err, tight)
        assert err_c <= gate_c, (ridge, alpha, K, err_c, gate_c)


@pytest.mark.gpu
@pytest.mark.parametrize("net,B2", [(0, 45), (3, 9), (5, 33)], ids=lambda v: str(v))
def test_reused_buffers_with_a_smaller_second_batch(net, B2, bhg_debug):
    """The same network twice on the same buffers, the second time with fewer samples (the rows B2 .. B of Gb_l and Rh_{l-1} hold the
    first solve's numbers: the dot products must not read them): bit for bit what fresh buffers give, and the parent arm's result."""
    import zoo

    ridge, K = 0.3, 3
    _arm(bhg_debug, net)
    curr, prev, vector = _gpu_problem(net, ridge, K, 1.0)
    first, _, _ = _solve(curr, prev, vector)
    assert np.isfinite(first).all()
    x, y = curr.cur_batch
    curr.cur_batch = (x[:B2].contiguous(), y[:B2].contiguous())
    reused, coeff, counters = _solve(curr, prev, vector)
    fresh_p = zoo.StubProblem("inner", copy.deepcopy(curr.module), config=Config(type="cg", cg_iterations=K, cg_alpha=1.0),
                              loss_fn=zoo.make_reweight_loss(prev, ridge), batch=curr.cur_batch)
    _declare(fresh_p, ridge)
    fresh, fresh_coeff, fresh_counters = _solve(fresh_p, prev, vector)
    assert G._buffers(fresh_p) is not G._buffers(curr) and counters == fresh_counters
    assert np.array_equal(reused, fresh) and np.array_equal(coeff, fresh_coeff), R.rel([reused], fresh)
    _arm(bhg_debug, net, CG_LAST_BACKWARD=1)
    parent, parent_coeff, parent_counters = _solve(curr, prev, vector)
    assert parent_counters == counters
    assert R.rel([reused], parent) <= ARM_GATE and G._l2(coeff, parent_coeff) <= ARM_GATE


def _fws_view(buf, entry, ctype, torch_dtype):
    n = ctypes.c_int(0)
    ptr = getattr(_native.load(), entry)(ctypes.byref(buf.desc), buf.fws.data_ptr(), ctypes.byref(n))
    size = ctypes.sizeof(ctype)
    assert ptr and n.value > 0
    off = int(ptr) - buf.fws.data_ptr()
    assert 0 <= off and off % size == 0 and off + size * n.value <= buf.fws.numel()
    return buf.fws[off: off + size * n.value].view(torch_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("net", [0, 1, 2], ids=_net_id)
def test_the_set_up_launch_clears_and_copies(net, bhg_debug):
    """head_j: the pair buffers of T2h and the copy of r|b0 are NaN before every solve; K = 2, 3, 4 give bit for bit what the arm with the
    runtime's memset and copy (head_j_setup = 0) gives.  (32 x 16 tiles, net 1, use no pair buffer: only the copy is at stake there.)"""
    ridge = 0.3
    curr, prev, vector = _gpu_problem(net, ridge, 2, 1.0)
    _arm(bhg_debug, net)
    _solve(curr, prev, vector)                      # allocates the buffers
    buf = G._buffers(curr)
    t2h = _fws_view(buf, "bhg_mlp_head_j_t2h_dev", ctypes.c_double, torch.float64)
    rb0c = _fws_view(buf, "bhg_mlp_rb0_copy_dev", ctypes.c_float, torch.float32)
    assert t2h.numel() == 2 * buf.BP and rb0c.numel() == buf.dims[1]
    for K in (2, 3, 4):
        curr.config = Config(type="cg", cg_iterations=K, cg_alpha=1.0)
        got = {}
        for setup in (0, 1):
            _arm(bhg_debug, net, HEAD_J_SETUP=setup)
            t2h.fill_(float("nan"))
            rb0c.fill_(float("nan"))
            hg_k, coeff_k, counters = _solve(curr, prev, vector)
            assert counters == (1, K - 1, K), (K, setup, counters)
            assert np.isfinite(hg_k).all() and torch.isfinite(rb0c).all(), (K, setup)
            got[setup] = (hg_k, coeff_k, rb0c.clone())
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (K, R.rel([got[1][0]], got[0][0]))
        assert torch.equal(got[0][2], got[1][2])

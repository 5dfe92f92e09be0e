"""The head launch of a projected CG iteration in its head_j form (csrc/bhg_mlp_headj.hpp / .hip): the head rows read the pre-head
product through J_b = W_3 diag(mask_2[b]) W_2, built once per solve, and the pre-head tiles ride in the head launch.

CPU: the identity in fp64 (addend term and masks included), and the plan key.  GPU: J against fp64 with the dot-product bound, the new
form against today's six launches (debug key head_j = 0, measurement library) and against the classic chain, bit-reproducibility, launch
counters, and reused buffers with a smaller second batch (stale rows of J and Rh_2)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from betty_amd import Config, _native

SIX = "six-launch (k_wskpl .. k_headu .. k_graw)"


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_the_identity_in_fp64():
    """sum_k W_3[c][k] Rh_2[b][k]  ==  J_b[c] . Rh_1[b]  +  sum_k W_3[c][k] mask_2[b][k] (addend[b][k] + c_2[k])  with
    Rh_2 = mask_2 * (Rh_1 W_2^T + addend + c_2) and J_b = W_3 diag(mask_2[b]) W_2."""
    rng = np.random.default_rng(11)
    B, C, d2, d3 = 7, 10, 96, 64
    W2, W3 = rng.standard_normal((d3, d2)), rng.standard_normal((C, d3))
    Rh1, addend, c2 = rng.standard_normal((B, d2)), rng.standard_normal((B, d3)), rng.standard_normal(d3)
    mask = (rng.random((B, d3)) < 0.5).astype(np.float64)
    mask[0] = 0.0   # a sample with every unit off
    mask[1] = 1.0   # ... and one with every unit on
    Rh2 = mask * (Rh1 @ W2.T + addend + c2)
    want = Rh2 @ W3.T
    J = np.einsum("ck,bk,kn->bcn", W3, mask, W2)
    got = np.einsum("bcn,bn->bc", J, Rh1) + (mask * (addend + c2)) @ W3.T
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(J[0], np.zeros((C, d2)))
    assert np.abs(J[1] - W3 @ W2).max() <= 1e-12 * np.abs(W3 @ W2).max()


def test_plan_key_head_j_follows_the_six_launch_form_at_one_batch_tile():
    import test_plan_selection as T

    seen = 0
    for dims, B, cg_free, *_ in T.CASES:
        d = _native.plan_describe(dims, B)
        want = 1 if (cg_free == SIX and B <= 128) else 0
        assert d["head_j"] == want, (dims, B, d)
        seen += want
        # only the solution-free CG solve has the form
        assert _native.plan_describe(dims, B, "cg", True)["head_j"] == 0
        assert _native.plan_describe(dims, B, "neumann", False)["head_j"] == 0
    assert seen == 3
    assert _native.plan_describe([128, 96, 160, 512, 12], 128)["head_j"] == 1   # the widest head the form takes
    assert _native.plan_describe([256, 256, 192, 640, 10], 100)["head_j"] == 0
    assert _native.plan_describe([256, 256, 128, 64, 24], 100)["head_j"] == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _solve(curr, prev, direction, K, ridge):
    """One solution-free fused CG solve on `curr` (P._run_solver's call, on a problem the caller keeps)."""
    import test_gpu_parity as P
    from betty_amd.hypergradient.structured import WeightedCEMLP

    curr.config = Config(type="cg", cg_iterations=K, cg_alpha=1.0)
    curr.hypergradient_structure = lambda prev_: WeightedCEMLP(
        curr, prev_, layers=list(curr.module.layers), weight_fn=lambda ce: prev_.fwd(ce.reshape(-1, 1)), ridge=ridge,
        impl="hip", fused=True, keep_solution=False, verify=False)
    return P._np(P.hg.jvp_fn_mapping["cg"]([0.1 * d for d in direction], curr, prev, False))


def _buffers(curr):
    from betty_amd.hypergradient import _mlp_hip

    (buf,) = _mlp_hip._BUFFERS[curr.module.layers[0]].values()
    return buf


def _j_view(buf):
    lib = _native.load()
    rows, cols = ctypes.c_int(0), ctypes.c_int(0)
    ptr = lib.bhg_mlp_head_j_dev(ctypes.byref(buf.desc), buf.fws.data_ptr(), ctypes.byref(rows), ctypes.byref(cols))
    assert ptr, "the plan takes the head_j form: J lives in the fused workspace"
    off = int(ptr) - buf.fws.data_ptr()
    assert 0 <= off and off + 4 * rows.value * cols.value <= buf.fws.numel()
    return buf.fws[off: off + 4 * rows.value * cols.value].view(torch.float32).view(rows.value, cols.value)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B", [([64, 64, 96, 64, 10], 37), ([128, 96, 160, 512, 12], 128)], ids=lambda v: str(v))
def test_j_against_fp64(dims, B, bhg_debug):
    """J as the library builds it (k_headj_pack + the chain's backward product through W_2) against numpy fp64, element by element
    within d_3 * 2^-24 * (|W_3| diag(mask) |W_2|) — the standard bound of a d_3-long fp32 dot product whose factors are exact (the mask
    is 0 / 1).  The J region of the workspace is NaN before the solve: every row below round32(B C) must be written, rows >= B C zero."""
    import test_gpu_parity as P

    bhg_debug.setenv("BHG_PROJ_MAX_RATIO", "100000000")   # (the form is under test, not the cost model that gates projection)
    assert _native.plan_describe(dims, B)["head_j"] == 1
    curr, prev, direction, _ = P._mlp_problem(dims, B, 0.05, 7 + B)
    _solve(curr, prev, direction, 2, 0.05)            # allocates the buffers
    buf = _buffers(curr)
    J = _j_view(buf)
    C, d3, d2 = dims[4], dims[3], dims[2]
    assert J.shape == ((B * C + 31) // 32 * 32, d2)
    J.fill_(float("nan"))
    out = _solve(curr, prev, direction, 2, 0.05)
    assert all(np.isfinite(o).all() for o in out)
    got = J.cpu().numpy().astype(np.float64)
    W3 = curr.module.layers[3].weight.detach().cpu().numpy().astype(np.float64)
    W2 = curr.module.layers[2].weight.detach().cpu().numpy().astype(np.float64)
    mask = buf.mask[2][:B].cpu().numpy().astype(np.float64)
    assert set(np.unique(mask)) <= {0.0, 1.0} and 0.0 < mask.mean() < 1.0
    A = (mask[:, None, :] * W3[None, :, :]).reshape(B * C, d3)
    want, bound = A @ W2, d3 * 2.0 ** -24 * (np.abs(A) @ np.abs(W2))
    err = np.abs(got[: B * C] - want)
    print(f"J {dims} B={B}: max err {err.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.isfinite(got).all(), "J must be written in full before it is used"
    assert (err <= bound).all(), float((err - bound).max())
    assert np.array_equal(got[B * C:], np.zeros_like(got[B * C:]))


FORM_CASES = [([512, 256, 256, 64, 10], 128), ([800, 512, 256, 128, 10], 100), ([256, 128, 160, 512, 12], 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 20])
@pytest.mark.parametrize("dims,B", FORM_CASES, ids=lambda v: str(v))
def test_head_j_form_matches_the_six_launches_and_the_classic_chain(dims, B, K, bhg_debug):
    """head_j = 1 (the default) against head_j = 0 (today's six launches) and the classic chain, tolerances of
    test_hoisted_and_projected_chain_match_classic_chain's arms.  Ridge as there: 0.05, and 2.0 for K = 20 (with 0.05 the Hessian of
    these random instances is indefinite and twenty iterations turn any difference in summation order into an O(1) one)."""
    import test_gpu_parity as P

    lib = _native.load()
    ridge = 2.0 if K >= 20 else 0.05
    seed = sum(dims) + B
    # (tile32: the 32 x 32 tiles, the arm of the default's 32 x 16.  The T2h partials of the tiles land in the head rows' old slots at the
    #  first two shapes — no more tiles than samples — and behind the layers' own at the third, B = 33.)
    arms = {"head_j": {}, "tile32": {"HEAD_J_TILE": "0"}, "six": {"HEAD_J": "0"}, "classic": {"BHG_MLP_HOIST": "0"}}
    out = {}
    for name, env in arms.items():
        bhg_debug.reset()
        bhg_debug.setenv("BHG_PROJ_MAX_RATIO", "100000000")
        for k, v in env.items():
            bhg_debug.setenv(k, v)
        assert _native.plan_describe(dims, B)["head_j"] == (1 if name in ("head_j", "tile32") else 0)
        l0, p0 = lib.bhg_mlp_lin_launches(), lib.bhg_mlp_proj_iterations()
        out[name] = P._run_solver("cg", dims, B, ridge, K, seed, True, keep=False)[0]
        dl, dp = lib.bhg_mlp_lin_launches() - l0, lib.bhg_mlp_proj_iterations() - p0
        assert (dl, dp) == ((0, 0) if name == "classic" else (K, K - 1)), (name, dl, dp)
        if name == "head_j":
            again = P._run_solver("cg", dims, B, ridge, K, seed, True, keep=False)[0]
            assert all(np.array_equal(u, v) for u, v in zip(again, out[name])), "bit-reproducible"
    tol = 1e-4 if K >= 20 else 5e-5
    for name in ("head_j", "tile32"):
        rel_six, _ = P.rel_err(out[name], out["six"])
        rel_cls, _ = P.rel_err(out[name], out["classic"])
        print(f"{name} {dims} B={B} K={K}: vs six launches {rel_six:.2e}, vs classic chain {rel_cls:.2e}")
        assert rel_six <= tol and rel_cls <= tol, (name, rel_six, rel_cls)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B,B2", [([512, 256, 256, 64, 10], 128, 45), ([256, 128, 160, 512, 12], 33, 9)], ids=lambda v: str(v))
def test_reused_buffers_with_a_smaller_second_batch(dims, B, B2, bhg_debug):
    """The same network twice on the same device buffers, the second time with fewer samples: rows of J, Rh_2 and the packed operands
    that the first solve wrote and the second does not own must not reach its result.  Reference: the same second solve on a copy of
    the network — fresh buffers — which must give the same bits."""
    import test_gpu_parity as P

    bhg_debug.setenv("BHG_PROJ_MAX_RATIO", "100000000")
    curr, prev, direction, _ = P._mlp_problem(dims, B, 0.05, 3 + B)
    first = _solve(curr, prev, direction, 4, 0.05)
    assert all(np.isfinite(o).all() for o in first)
    x, y = curr.cur_batch
    curr.cur_batch = (x[:B2].contiguous(), y[:B2].contiguous())
    reused = _solve(curr, prev, direction, 4, 0.05)
    twin = copy.deepcopy(curr.module)
    import zoo

    fresh_p = zoo.StubProblem("inner", twin, config=Config(type="cg"), loss_fn=zoo.make_reweight_loss(prev, 0.05), batch=curr.cur_batch)
    fresh = _solve(fresh_p, prev, direction, 4, 0.05)
    assert _buffers(fresh_p) is not _buffers(curr)
    assert all(np.array_equal(u, v) for u, v in zip(reused, fresh)), P.rel_err(reused, fresh)
    J = _j_view(_buffers(curr)).cpu().numpy()
    assert J.shape[0] == (B2 * dims[4] + 31) // 32 * 32 and np.array_equal(J[B2 * dims[4]:], np.zeros_like(J[B2 * dims[4]:]))

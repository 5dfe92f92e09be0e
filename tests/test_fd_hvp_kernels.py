"""The pair-form kernels of the finite-difference Hessian-vector product, bit for bit (include/bhg.h: bhg_fd_perturb, bhg_cg_step_fd,
bhg_neumann_step_fd): `cg_step_fd` / `neumann_step_fd` on (g+, g-, two_eps) must leave x, r, p (v, p) BIT-IDENTICAL to the existing
one-table step fed with ATen's `(g+ - g-) / two_eps`; `fd_perturb` bit-identical to ATen's `w0 + (sign * eps) * p`.  The sweep covers
1 / 8 / 122 / 1,399 tensors, numels that are not multiples of 4, vectors on both sides of every resident instance's capacity
(register-only, LDS-assisted, hybrid, streaming), k = 0 / middle / last with out_scale != 0, and four arms of (cg_alpha, hvp_shift, two_eps) — the shift-free form every opaque problem
runs among them.
Argument validation runs without a GPU."""
import ctypes

import pytest
import torch

from betty_amd import _native

DEV = "cuda:0"


def _layouts():
    g = torch.Generator().manual_seed(5)
    out = {
        "T1_odd": [3 * 4096 + 1],
        "T8": [1, 3, 4095, 4097, 10, 70001, 6, 12345],
        "T122": [int(n) for n in torch.randint(1, 5000, (122,), generator=g)],
        "T1399": [int(n) for n in torch.randint(1, 3000, (1399,), generator=g)],
    }
    return out


def _big_layouts(be):
    """Chunk counts around the capacities of the resident instances on THIS device (11 / 15 / 2 x 14 chunks per CU)."""
    cap = int(be.lib.bhg_cg_resident_capacity_chunks())
    cus = cap // 28
    if cus <= 0:
        return {}
    return {
        "register_only_full": [4096 * (11 * cus - 1) + 5, 4093],
        "lds_assisted": [4096 * (13 * cus) + 2, 777],
        "hybrid": [4096 * (20 * cus) + 3],
        "beyond_capacity_streams": [4096 * (28 * cus + 3) + 1],
    }


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))   # (bit patterns: a NaN equals itself here)


def _rand(numels, gen, scale=1.0):
    return [(scale * torch.randn(n, generator=gen)).to(DEV) for n in numels]


def _cg_sequence(be, layout, vector, pairs, two_eps, fd, variant, cg_alpha, shift):
    x, r, p = (layout.new_flat() for _ in range(3))
    be.cg_init(layout, vector, x, r, p)
    states = []
    K = len(pairs)
    for k, (gp, gm) in enumerate(pairs):
        out_scale = -0.7 if k == K - 1 else 0.0
        if fd:
            be.cg_step_fd(layout, gp, gm, two_eps, x, r, p, cg_alpha, k, out_scale=out_scale, variant=variant, hvp_shift=shift)
        else:
            hvp = [(a - b) / two_eps for a, b in zip(gp, gm)]   # ATen: subtraction rounded, then a true division by the 0-dim tensor
            be.cg_step(layout, hvp, x, r, p, cg_alpha, k, out_scale=out_scale, variant=variant, hvp_shift=shift)
        states.append((x.clone(), r.clone(), p.clone(), be.cg_scalars(layout)))
    be.after_cg(layout)
    return states


# (cg_alpha, hvp_shift, two_eps): the shift-free form is what every opaque problem runs; the shifted one is the proximal structure's
CG_ARMS = [(1.0, 0.0, 0.0123), (0.7, 0.3, 0.0123), (1.3, 0.0, 3.7e-5), (0.25, 2.0, 1.9)]


def _check_layout(numels, variant=None):
    from betty_amd.backend import get_backend
    from betty_amd.flat import FlatLayout

    be = get_backend()
    gen = torch.Generator().manual_seed(len(numels) + numels[0])
    layout = FlatLayout(numels, torch.device(DEV))
    vector = _rand(numels, gen)
    pairs = [(_rand(numels, gen), _rand(numels, gen)) for _ in range(3)]
    for cg_alpha, shift, te in CG_ARMS:
        two_eps = torch.tensor(te, device=DEV)
        want = _cg_sequence(be, layout, vector, pairs, two_eps, False, variant, cg_alpha, shift)
        got = _cg_sequence(be, layout, vector, pairs, two_eps, True, variant, cg_alpha, shift)
        for k, (w, g) in enumerate(zip(want, got)):
            for name, a, b in zip("xrp", w[:3], g[:3]):
                assert _same_bits(a, b), f"cg_step_fd: {name} differs at k={k} (T={len(numels)}, N={sum(numels)}, arm {(cg_alpha, shift, te)})"
            assert torch.equal(w[3], g[3]), "the iteration's scalars differ"
        assert torch.isfinite(want[0][0]).all()   # (later iterations of a random, indefinite 'Hessian' may overflow: same bits either way)

    def neumann_sequence(fd, alpha, shift, two_eps):
        v, p = layout.new_flat(), layout.new_flat()
        be.neumann_init(layout, vector, v, p)
        for k, (gp, gm) in enumerate(pairs):
            out_scale = -alpha if k == len(pairs) - 1 else 0.0
            if fd:
                be.neumann_step_fd(layout, gp, gm, two_eps, v, p, alpha, out_scale=out_scale, hvp_shift=shift)
            else:
                be.neumann_step(layout, [(a - b) / two_eps for a, b in zip(gp, gm)], v, p, alpha, out_scale=out_scale, hvp_shift=shift)
        return v, p

    for alpha, shift, te in CG_ARMS:
        two_eps = torch.tensor(te, device=DEV)
        want_vp, got_vp = neumann_sequence(False, alpha, shift, two_eps), neumann_sequence(True, alpha, shift, two_eps)
        assert _same_bits(want_vp[0], got_vp[0]) and _same_bits(want_vp[1], got_vp[1]), \
            f"neumann_step_fd differs (T={len(numels)}, N={sum(numels)}, arm {(alpha, shift, te)})"
    # perturb from a snapshot, both signs
    w0 = layout.new_flat()
    be.flatten(layout, vector, w0, 1.0)
    eps = torch.tensor([3.21e-3], device=DEV)[0]
    weights = [torch.full_like(t, float("nan")) for t in vector]
    for sign in (1.0, -1.0):
        be.fd_perturb(layout, weights, w0, pairs[0][0], eps, sign)
        a = eps * sign
        for w, base, d in zip(weights, vector, pairs[0][0]):
            assert torch.equal(w, base + a * d), f"fd_perturb differs (sign={sign}, T={len(numels)})"
    be.scatter(layout, w0, weights, 1.0)
    assert all(torch.equal(w, base) for w, base in zip(weights, vector)), "the snapshot must bring the weights back bit for bit"
    torch.cuda.synchronize()
    be.check_health()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["T1_odd", "T8", "T122", "T1399"])
@pytest.mark.parametrize("variant", [None, _native.BHG_CG_STREAM, _native.BHG_CG_RESIDENT])
def test_pair_steps_and_perturb_are_bitwise_the_one_table_steps_on_the_aten_difference(name, variant):
    _check_layout(_layouts()[name], variant)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["register_only_full", "lds_assisted", "hybrid", "beyond_capacity_streams"])
def test_pair_steps_on_both_sides_of_the_resident_capacities(name):
    from betty_amd.backend import get_backend

    big = _big_layouts(get_backend())
    assert big, "no resident capacity reported on this device"
    _check_layout(big[name])
    torch.cuda.empty_cache()


def test_argument_validation_without_gpu():
    """Bad arguments are rejected before any HIP call: negative return code + message, no crash (none of these paths touches the device)."""
    lib = _native.load()
    one = (ctypes.c_void_p * 1)(0)
    tab = ctypes.cast(one, _native._PP)
    null_tab = ctypes.cast(None, _native._PP)
    # NULL / mismatched tables (one of the pair missing) with T > 0
    for gp, gm in ((null_tab, null_tab), (tab, null_tab), (null_tab, tab)):
        assert lib.bhg_cg_step_fd(gp, gm, 1, 1, 1, 1, None, None, None, 1.0, 0, 0.0, 0.0, 0, 1, None) == -1
        assert b"NULL" in lib.bhg_last_error()
        assert lib.bhg_neumann_step_fd(gp, gm, 1, 1, 1, 1, None, None, 0.1, 0.0, 0.0, 1, None) == -1
        assert b"NULL" in lib.bhg_last_error()
        assert lib.bhg_fd_perturb(gp, 1, gm, 1, 1, 1, 1, 1.0, None, None) == -1
        assert b"NULL" in lib.bhg_last_error()
    # negative sizes, missing chunk table
    assert lib.bhg_cg_step_fd(tab, tab, 1, -1, None, 0, None, None, None, 1.0, 0, 0.0, 0.0, 0, 1, None) == -1
    assert b"negative" in lib.bhg_last_error()
    assert lib.bhg_neumann_step_fd(tab, tab, 1, 1, None, 3, None, None, 0.1, 0.0, 0.0, 1, None) == -1
    assert b"chunk table" in lib.bhg_last_error()
    assert lib.bhg_fd_perturb(tab, 1, tab, 1, None, 2, 1, 1.0, None, None) == -1
    assert b"chunk table" in lib.bhg_last_error()
    # workspace missing, negative iteration index, missing two_eps / eps / snapshot / state
    assert lib.bhg_cg_step_fd(tab, tab, 1, 1, 1, 1, None, None, None, 1.0, 0, 0.0, 0.0, 0, None, None) == -1
    assert b"workspace" in lib.bhg_last_error()
    assert lib.bhg_cg_step_fd(tab, tab, 1, 1, 1, 1, None, None, None, 1.0, -1, 0.0, 0.0, 0, 1, None) == -1
    assert lib.bhg_cg_step_fd(tab, tab, None, 1, 1, 1, 1, 1, 1, 1.0, 0, 0.0, 0.0, 0, 1, None) == -1
    assert b"two_eps" in lib.bhg_last_error()
    assert lib.bhg_neumann_step_fd(tab, tab, None, 1, 1, 1, 1, 1, 0.1, 0.0, 0.0, 1, None) == -1
    assert b"two_eps" in lib.bhg_last_error()
    assert lib.bhg_neumann_step_fd(tab, tab, 1, 1, 1, 1, None, None, 0.1, 0.0, 0.0, 1, None) == -1
    assert b"state vector" in lib.bhg_last_error()
    assert lib.bhg_fd_perturb(tab, None, tab, 1, 1, 1, 1, 1.0, None, None) == -1
    assert b"snapshot" in lib.bhg_last_error()
    assert lib.bhg_fd_perturb(tab, 1, tab, 1, 1, 1, None, 1.0, None, None) == -1
    assert b"eps" in lib.bhg_last_error()
    # empty problems are a no-op, not an error
    assert lib.bhg_cg_step_fd(null_tab, null_tab, None, 0, None, 0, None, None, None, 1.0, 0, 0.0, 0.0, 0, 1, None) == 0
    assert lib.bhg_neumann_step_fd(null_tab, null_tab, None, 0, None, 0, None, None, 0.1, 0.0, 0.0, None, None) == 0
    assert lib.bhg_fd_perturb(null_tab, None, null_tab, 0, None, 0, None, 1.0, None, None) == 0

"""The CG and Neumann recurrence kernels of csrc/bhg_vector.hip, ONE STEP AT A TIME against tests/recurrence_ref.py (numpy, fp64 dots;
pinned bit for bit to oracle/recurrence.c and the CPU checker by tests/test_recurrence_ref.py).

Every iteration is checked on its own: the GPU's state BEFORE the launch is copied to the host, the reference takes one step from
exactly those bits and the same H p bits (formed by ATen on the device, downloaded), and the GPU's state AFTER the launch must be

* in the dots rr_old, pHp, rr_new: within 2 * N * 2^-53 * S of the reference, S the reference's sum of absolute terms of that dot —
  the worst case of two fp64 summations of the same exact terms (fp32 x fp32 products are exact in fp64) in different orders:
  each is within (N - 1) * 2^-53 * S of the true sum.  Derived, not measured; one missing 4096-element chunk out of 7,000 is ~1e-4 * S;
* in alpha, beta as published: the reference's fp32 value or one of its two neighbours (the fp64 dots may round to adjacent fp32
  values), AND exactly the fp32 quotient of the kernel's own published dots (the kernels state `(float)rr / (float)den`);
* in x', r', p': BIT-IDENTICAL to the reference step evaluated with the published alpha and beta — the kernels state their
  rounding sequence (mul_rn, then add_rn / sub_rn), so given the scalars there is nothing left to tolerate;
* zero in every padding element.

The sweep takes every instance of the resident kernel to the edges of its capacity (register-only full to its last slot, first and last
size of the LDS-assisted instance, first size of the hybrid instance and one with a long streamed remainder; each case asserts the
chunk count that selects its instance), the three streaming
kernels as one step and phase by phase (bhg_cg_phase), stream / resident alternating inside a solve, with and without the diagonal
shift — the shifted arms are what the proximal and ridge solves run — and bhg_cg_init_masked on its own.
"""
import numpy as np
import pytest
import torch

import recurrence_ref as ref
from betty_amd import _native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U53 = 2.0 ** -53

SMALL = {
    "one": [1],
    "tiny3": [3, 5, 7],
    "chunk_edges": [4095, 4096, 4097],
    "T50_table": [17] * 50,   # T > 32: the pointer table lives in the workspace
    "T8_ragged": [1, 3, 4095, 4097, 10, 70001, 6, 12345],
}
# name -> (numels, chunks) as functions of cus = workgroups of the resident kernel.  A chunk never spans tensors, so a list counts
# sum(ceil(numel / 4096)); cg_step_launch takes the register-only instance up to 11 * cus chunks, the LDS-assisted one up to 15 * cus,
# the hybrid one beyond (capacity 28 * cus).  The two "two_tensors" lists sit one chunk PAST an edge with two ragged tail chunks
# (their first tensor alone would stop one chunk short of it): the next instance's first size, reached with a second tensor.
BIG = {
    "register_only_full": (lambda c: [4096 * (11 * c - 2) + 5, 4093], lambda c: 11 * c),         # every slot of every workgroup holds data
    "lds_first": (lambda c: [4096 * (11 * c) + 1], lambda c: 11 * c + 1),                        # first size of the LDS-assisted instance
    "lds_first_two_tensors": (lambda c: [4096 * (11 * c - 1) + 5, 4093], lambda c: 11 * c + 1),
    "lds_last": (lambda c: [4096 * (15 * c - 2) + 2, 777], lambda c: 15 * c),                    # its last: all 15 slots, 9 of them in LDS
    "hybrid_first": (lambda c: [4096 * (15 * c) + 3], lambda c: 15 * c + 1),                     # first size of the hybrid instance
    "hybrid_first_two_tensors": (lambda c: [4096 * (15 * c - 1) + 2, 777], lambda c: 15 * c + 1),
    "hybrid_20": (lambda c: [4096 * (20 * c) + 3], lambda c: 20 * c + 1),                        # 14 resident slots + a streamed remainder
}
VARIANTS = ["stream", "resident", "phased", "alternating"]
CG_ARMS = [(1.0, 0.0), (0.7, 0.3), (0.25, 2.0)]           # (cg_alpha, hvp_shift)
NEUMANN_ARMS = [(0.3, 0.0), (0.3, 0.3), (0.05, 2.0)]      # (alpha, hvp_shift)


@pytest.fixture(scope="module")
def be():
    from betty_amd.backend import get_backend

    b = get_backend()
    assert b.name == "hip"
    return b


def _sizes(be, name):
    if name in SMALL:
        return SMALL[name]
    cus = int(be.lib.bhg_cg_resident_capacity_chunks()) // 28
    assert cus > 0, "no resident capacity reported on this device"
    return BIG[name][0](cus)


def _assert_instance(be, name, lay):
    """The chunk count decides the resident instance: hold every capacity-edge case to the count it is named for."""
    if name in SMALL:
        return
    cus = int(be.lib.bhg_cg_resident_capacity_chunks()) // 28
    assert lay.n_chunks == BIG[name][1](cus), f"{name}: {lay.n_chunks} chunks, meant {BIG[name][1](cus)} (cus = {cus})"
    instance = "register" if lay.n_chunks <= 11 * cus else "lds" if lay.n_chunks <= 15 * cus else "hybrid"
    assert lay.n_chunks <= 28 * cus and name.startswith(instance), f"{name} runs the {instance} instance ({lay.n_chunks} chunks, cus = {cus})"


class _Problem:
    """One layout with its seeded data: the right-hand side, the diagonal d = 1 + 0.5 sin(index) and a fixed noise list on the device."""

    def __init__(self, numels, seed):
        from betty_amd.flat import FlatLayout

        self.lay = FlatLayout(numels, torch.device(DEV))
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.vec = [torch.randn(n, generator=gen, device=DEV) for n in numels]
        self.noise = [torch.randn(n, generator=gen, device=DEV) for n in numels]
        self.d = [1.0 + 0.5 * torch.sin(torch.arange(n, device=DEV, dtype=torch.float32)) for n in numels]
        self.N = int(sum(numels))
        pad = np.ones(self.lay.flat_size, dtype=bool)
        for s, n in zip(self.lay.starts, self.lay.numels):
            pad[s:s + n] = False
        self.pad = pad

    def hvp(self, flat):
        """hv = d * q + 0.05 * noise on the views of `flat`: keeps the recurrence well scaled and is NOT a multiple of q, so a shift
        applied to the wrong slice changes bits.  ATen on the device; the kernel and the reference read the same bits."""
        return [d * t + 0.05 * nz for d, t, nz in zip(self.d, self.lay.views(flat, self.vec), self.noise)]

    def payload(self, flat_np):
        return np.concatenate([flat_np[s:s + n] for s, n in zip(self.lay.starts, self.lay.numels)])


def _host(t):
    return t.detach().cpu().numpy()


def _differing(a, b):
    """Indices at which two float32 arrays differ as bit patterns.  IEEE 754 leaves the sign and payload of a GENERATED NaN to the
    implementation (a recurrence that has converged exactly, N = 1 after its first step, divides 0 by 0 on both sides), so a NaN
    matches a NaN; every other element must have the same bits."""
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    return np.flatnonzero((a.view(np.int32) != b.view(np.int32)) & ~(np.isnan(a) & np.isnan(b)))


def _bits_equal(a, b):
    return _differing(a, b).size == 0


def _same_value(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _is_neighbour(got, want):
    """got is the fp32 value `want` or adjacent to it (np.nextafter either way); NaN only for NaN."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return got in (want, np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf)))


def _launch_cg(be, lay, variant, k, hv, x, r, p, cg_alpha, out_scale, shift):
    if variant == "phased":
        for phase in (0, 1, 2):
            be.cg_phase(phase, lay, hv, x, r, p, cg_alpha, k, out_scale=out_scale, hvp_shift=shift)
        return
    v = {"stream": _native.BHG_CG_STREAM, "resident": _native.BHG_CG_RESIDENT,
         "alternating": (_native.BHG_CG_STREAM, _native.BHG_CG_RESIDENT, _native.BHG_CG_STREAM)[k % 3]}[variant]
    be.cg_step(lay, hv, x, r, p, cg_alpha, k, out_scale=out_scale, variant=v, hvp_shift=shift)
    lay._cg_variant = None   # the Python wrapper pins the variant per solve; these tests name it per step


def _cg_iterations(be, prob, x, r, p, variant, cg_alpha, shift, K, check=True, keep=False):
    """K iterations from the state in x, r, p (after a cg_init).  check: every iteration against the reference stepped from the GPU's
    own pre-state of that iteration.  keep: device clones of (x, r, p, scalars) after every iteration."""
    lay, N = prob.lay, prob.N
    kept = []
    for k in range(K):
        out_scale = -cg_alpha if k == K - 1 else 0.0
        hv = prob.hvp(p)
        if check:
            pre_flat = [_host(t) for t in (x, r, p)]
            assert not any(np.any(a[prob.pad] != 0.0) for a in pre_flat), f"padding is not zero before iteration {k}"
            pre = [prob.payload(a) for a in pre_flat]
            h = np.concatenate([_host(t) for t in hv])
        _launch_cg(be, lay, variant, k, hv, x, r, p, cg_alpha, out_scale, shift)
        if keep:
            kept.append((x.clone(), r.clone(), p.clone(), be.cg_scalars(lay)))
        if not check:
            continue
        post = [_host(t) for t in (x, r, p)]
        rr_old, den, alpha, rr_new, beta = (float(s) for s in _host(be.cg_scalars(lay)))
        where = f"iteration {k}, {variant}, N={N}, T={lay.T}, arm {(cg_alpha, shift)}"
        where += f": published rr_old={rr_old!r} pHp={den!r} alpha={alpha!r} rr_new={rr_new!r} beta={beta!r}"
        rr_ref = ref.dot64(pre[1], pre[1])[0]
        vecs, scal, sums = ref.cg_step(h, pre[0], pre[1], pre[2], rr_ref, cg_alpha, shift, out_scale)
        if not (alpha == scal[2] and beta == scal[4]):
            # a neighbouring step length: the vectors (and rr_new, the dot of THAT r') are held to the step with the published values.
            # (With equal values this second evaluation would be the first one again.)
            vecs, scal_pub, sums_pub = ref.cg_step(h, pre[0], pre[1], pre[2], rr_ref, cg_alpha, shift, out_scale, alpha=alpha, beta=beta)
            scal, sums = scal[:3] + (scal_pub[3], scal[4]), (sums[0], sums_pub[1])
        for name, got, want, S in (("rr_old", rr_old, scal[0], scal[0]), ("pHp", den, scal[1], sums[0]), ("rr_new", rr_new, scal[3], sums[1])):
            bound = 2.0 * N * U53 * S
            assert abs(got - want) <= bound or (np.isnan(got) and np.isnan(want)), f"{name} = {got!r}, reference {want!r}, bound {bound:.3e} ({where})"
        assert _is_neighbour(alpha, scal[2]), f"alpha = {alpha!r}, reference {scal[2]!r} ({where})"
        assert _is_neighbour(beta, scal[4]), f"beta = {beta!r}, reference {scal[4]!r} ({where})"
        with np.errstate(divide="ignore", invalid="ignore"):
            assert _same_value(alpha, float(np.float32(rr_old) / np.float32(den))), f"alpha is not the fp32 quotient of the published dots ({where})"
            assert _same_value(beta, float(np.float32(rr_new) / np.float32(rr_old))), f"beta is not the fp32 quotient of the published dots ({where})"
        for name, got, want in zip("xrp", post, vecs):
            g = prob.payload(got)
            bad = _differing(g, want)
            if bad.size:
                raise AssertionError(f"{name}' differs from the reference step in {bad.size} of {N} elements, first at payload index "
                                     f"{bad[0]}: got {g[bad[0]]!r}, want {want[bad[0]]!r} ({where})")
            assert not np.any(got[prob.pad] != 0.0), f"padding of {name} was written ({where})"
    assert not be.cg_barrier_timed_out(lay)
    return kept


def _cg_cases():
    out = []
    for name in SMALL:
        out += [(name, v, a) for v in VARIANTS for a in range(3)]
    for name in BIG:
        out += [(name, v, a) for v in VARIANTS for a in (0, 2)]
    return out


@pytest.mark.parametrize("name,variant,arm", _cg_cases(), ids=lambda v: str(v))
def test_cg_step_every_instance_one_iteration_at_a_time(name, variant, arm, be):
    if variant in ("resident", "alternating") and not be.lib.bhg_cg_resident_ok():
        pytest.skip("the resident kernel is not eligible on this device (residency census failed)")
    numels = _sizes(be, name)
    cg_alpha, shift = CG_ARMS[arm]
    K = 3 if name in SMALL else 2
    prob = _Problem(numels, seed=101 + len(numels) + numels[0] % 1000)
    lay = prob.lay
    _assert_instance(be, name, lay)
    x, r, p = (lay.new_flat() for _ in range(3))
    want = None
    if variant == "phased":   # the three kernels, one call per phase, are the streaming step: same bits, scalars included
        be.cg_init(lay, prob.vec, x, r, p)
        want = _cg_iterations(be, prob, x, r, p, "stream", cg_alpha, shift, K, check=False, keep=True)
    be.cg_init(lay, prob.vec, x, r, p)
    got = _cg_iterations(be, prob, x, r, p, variant, cg_alpha, shift, K, keep=want is not None)
    if want is not None:
        for k, (w, g) in enumerate(zip(want, got)):
            for nm, a, b in zip("xrp", w[:3], g[:3]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"phased {nm} is not the streaming step's at k={k}"
            assert torch.equal(w[3].view(torch.int64), g[3].view(torch.int64)), f"phased scalars are not the streaming step's at k={k}"
    torch.cuda.synchronize()
    be.check_health()
    del prob, lay, x, r, p, want, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("arm", range(3))
@pytest.mark.parametrize("name", list(SMALL) + ["lds_first"])
def test_neumann_step_one_iteration_at_a_time(name, arm, be):
    numels = _sizes(be, name)
    alpha, shift = NEUMANN_ARMS[arm]
    K = 3
    prob = _Problem(numels, seed=211 + len(numels) + numels[0] % 1000)
    lay = prob.lay
    _assert_instance(be, name, lay)
    v, p = lay.new_flat(), lay.new_flat()
    be.neumann_init(lay, prob.vec, v, p)
    for k in range(K):
        out_scale = -alpha if k == K - 1 else 0.0
        hv = prob.hvp(v)
        pre_flat = [_host(t) for t in (v, p)]
        assert not any(np.any(a[prob.pad] != 0.0) for a in pre_flat), f"padding is not zero before iteration {k}"
        pre = [prob.payload(a) for a in pre_flat]
        h = np.concatenate([_host(t) for t in hv])
        if k == 0:
            vec = np.concatenate([_host(t) for t in prob.vec])
            assert _bits_equal(pre[0], vec) and _bits_equal(pre[1], vec), "neumann_init: v = p = vector"
        be.neumann_step(lay, hv, v, p, alpha, out_scale=out_scale, hvp_shift=shift)
        post = [_host(t) for t in (v, p)]
        want = ref.neumann_step(h, pre[0], pre[1], alpha, shift, out_scale)
        for nm, got, w in zip("vp", post, want):
            g = prob.payload(got)
            bad = _differing(g, w)
            if bad.size:
                raise AssertionError(f"{nm}' differs from the reference step in {bad.size} of {prob.N} elements, first at payload index "
                                     f"{bad[0]}: got {g[bad[0]]!r}, want {w[bad[0]]!r} (iteration {k}, arm {(alpha, shift)})")
            assert not np.any(got[prob.pad] != 0.0), f"padding of {nm} was written (iteration {k})"
        assert np.isfinite(post[0]).all() and np.isfinite(post[1]).all()
    del prob, lay, v, p
    torch.cuda.empty_cache()


# ---- bhg_cg_init_masked on its own ------------------------------------------------------------------------------------------
SENTINEL = 12345.0
# the suite's pool of small tensor sizes (tests/test_gpu_parity.py: _fuzz_sizes): float4 tails, chunk edges, up to three chunks
POOL = [1, 2, 3, 4, 5, 63, 64, 65, 4093, 4094, 4095, 4096, 4097, 4099, 8191, 8192, 8193, 12288]
# ... drawn with a fixed seed, and PLACED where the mask's rules bite, so that none of it is left to the draw: multi-chunk tensors
# on a set bit (0), on cleared bits (1, 6), on the mask's last bit (63) and past it (64, 69), a one-element tensor past it (65)
PLACED = {0: 4097, 1: 8193, 6: 12288, 63: 4097, 64: 8193, 65: 1, 69: 12288}
MASKS = {"none": 0, "some": 0b10100101, "all": (1 << 64) - 1, "bit63": 1 << 63}


@pytest.mark.parametrize("case", ["none", "some", "all", "bit63", "some_without_x"])
@pytest.mark.parametrize("T", [8, 70])
def test_cg_init_masked_writes_only_kept_tensors_and_counts_all(T, case, be):
    rs = np.random.RandomState(T)
    numels = [int(rs.choice(POOL)) for _ in range(T)]
    for t, n in PLACED.items():
        if t < T:
            numels[t] = n
    prob = _Problem(numels, seed=307 + T)
    lay = prob.lay
    mask = MASKS[case.split("_")[0]]
    with_x = not case.endswith("without_x")
    x, r, p = (torch.full((lay.flat_size,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(3))
    be.cg_init(lay, prob.vec, x if with_x else None, r, p, keep_mask=mask)
    xh, rh, ph = (_host(t) for t in (x, r, p))
    for t, (s, n, vt) in enumerate(zip(lay.starts, lay.numels, prob.vec)):
        kept = t >= 64 or ((mask >> t) & 1) == 1   # tensors past the 64-bit mask are always written
        want = _host(vt) if kept else np.full(n, SENTINEL, np.float32)
        assert _bits_equal(rh[s:s + n], want) and _bits_equal(ph[s:s + n], want), f"tensor {t} (kept={kept}, mask={mask:#x})"
        assert _bits_equal(xh[s:s + n], np.zeros(n, np.float32) if with_x else np.full(n, SENTINEL, np.float32)), f"x of tensor {t}"
    for name, a in zip("xrp", (xh, rh, ph)):
        assert np.all(a[prob.pad] == np.float32(SENTINEL)), f"padding of {name} was written"
    # the cleared tensors' share of r.r was still counted: complete r and p by hand, restore the layout's zero padding, and the
    # first step's published rr_old must be the dot over ALL tensors (held to sum r^2 of the pre-state by the dot bound)
    flat_vec = lay.new_flat()
    for s, n, vt in zip(lay.starts, lay.numels, prob.vec):
        flat_vec[s:s + n] = vt
    r.copy_(flat_vec)
    p.copy_(flat_vec)
    x.zero_()
    _cg_iterations(be, prob, x, r, p, "stream", 0.7, 0.3, 1)
    rr_old = float(_host(be.cg_scalars(lay))[0])
    vec = np.concatenate([_host(t) for t in prob.vec])
    rr_all = ref.dot64(vec, vec)[0]
    assert abs(rr_old - rr_all) <= 2.0 * prob.N * U53 * rr_all, (rr_old, rr_all)

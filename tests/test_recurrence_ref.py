"""tests/recurrence_ref.py pinned on the CPU: bit for bit against oracle/recurrence.c where the oracle can follow (hvp_shift = 0) and
against the CPU checker backend's shifted steps (hvp_shift = 0.3 / 2.0), three chained iterations each, scalars included.  What the GPU
tests of tests/test_recurrence_kernels.py hold the kernels to is therefore the arithmetic the rest of the suite already trusts."""
import ctypes

import numpy as np
import pytest
import torch

import recurrence_ref as ref
from _cpu_checker_backend import CpuCheckerBackend, load_oracle_lib

SIZES = [1, 5, 4097, 70001]
K = 3


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(_bits(a), _bits(b))


def _data(n):
    rs = np.random.RandomState(1000 + n)
    vec = rs.standard_normal(n).astype(np.float32)
    d = (1.0 + 0.5 * np.sin(np.arange(n, dtype=np.float64))).astype(np.float32)
    noise = [(0.05 * rs.standard_normal(n)).astype(np.float32) for _ in range(K)]
    return vec, d, noise


def _hvp(d, q, noise):
    return d * q + noise   # not a multiple of q: a shift applied to the wrong vector changes bits


@pytest.fixture(scope="module")
def orc():
    return load_oracle_lib()


@pytest.mark.parametrize("n", SIZES)
def test_cg_step_without_shift_is_the_oracle_bit_for_bit(n, orc):
    vec, d, noise = _data(n)
    cg_alpha = 0.7
    x, r, p, rr = ref.cg_init(vec)
    xo, ro, po = (np.full(n, 9.0, np.float32) for _ in range(3))
    orc.orc_cg_init(_ptr(vec), _ptr(xo), _ptr(ro), _ptr(po), n)
    rro = orc.orc_sqnorm(_ptr(vec), n)
    assert _same_bits(x, xo) and _same_bits(r, ro) and _same_bits(p, po) and rr == rro
    for k in range(K):
        h = _hvp(d, p, noise[k])
        out_scale = -cg_alpha if k == K - 1 else 0.0
        (x, r, p), scal, sums = ref.cg_step(h, x, r, p, rr, cg_alpha, 0.0, out_scale)
        den = orc.orc_dot_scaled(_ptr(h), _ptr(po), n, cg_alpha)
        a = np.float32(rro) / np.float32(den)
        rr_new = orc.orc_cg_resid(_ptr(h), _ptr(ro), n, float(a))
        b = np.float32(rr_new) / np.float32(rro)
        orc.orc_cg_dir(_ptr(xo), _ptr(ro), _ptr(po), n, float(a), float(b), out_scale)
        assert scal == (rro, den, float(a), rr_new, float(b)), (k, scal)
        assert _same_bits(x, xo) and _same_bits(r, ro) and _same_bits(p, po), k
        assert sums[0] >= abs(den) and sums[1] == rr_new   # the sums of absolute terms bound their dots
        rr, rro = scal[3], rr_new
    assert np.isfinite(x).all() and np.abs(x).max() > 0


@pytest.mark.parametrize("n", SIZES)
def test_neumann_step_without_shift_is_the_oracle_bit_for_bit(n, orc):
    vec, d, noise = _data(n)
    v, p = vec.copy(), vec.copy()
    vo, po = vec.copy(), vec.copy()
    for k in range(K):
        h = _hvp(d, v, noise[k])
        out_scale = -0.3 if k == K - 1 else 0.0
        v, p = ref.neumann_step(h, v, p, 0.3, 0.0, out_scale)
        orc.orc_neumann_step(_ptr(h), _ptr(vo), _ptr(po), n, 0.3, out_scale)
        assert _same_bits(v, vo) and _same_bits(p, po), k


@pytest.mark.parametrize("cg_alpha,shift", [(0.7, 0.3), (0.25, 2.0)])
@pytest.mark.parametrize("n", SIZES)
def test_shifted_cg_step_is_the_cpu_checker_bit_for_bit(n, cg_alpha, shift):
    vec, d, noise = _data(n)
    chk = CpuCheckerBackend()
    tv = [torch.from_numpy(vec.copy())]
    lay = chk.layout(tv)
    xc, rc, pc = (torch.zeros(lay.flat_size, dtype=torch.float32) for _ in range(3))
    chk.cg_init(lay, tv, xc, rc, pc)
    x, r, p, rr = ref.cg_init(vec)
    s0 = lay.starts[0]
    for k in range(K):
        h = _hvp(d, p, noise[k])
        out_scale = -cg_alpha if k == K - 1 else 0.0
        (x, r, p), scal, _ = ref.cg_step(h, x, r, p, rr, cg_alpha, shift, out_scale)
        chk.cg_step(lay, [torch.from_numpy(h)], xc, rc, pc, cg_alpha, k, out_scale=out_scale, hvp_shift=shift)
        assert scal == tuple(float(s) for s in chk.last_scalars), (k, scal, chk.last_scalars)
        for got, want in ((x, xc), (r, rc), (p, pc)):
            assert _same_bits(got, want.numpy()[s0:s0 + n]), k
        rr = scal[3]


@pytest.mark.parametrize("alpha,shift", [(0.3, 0.3), (0.05, 2.0)])
@pytest.mark.parametrize("n", SIZES)
def test_shifted_neumann_step_is_the_cpu_checker_bit_for_bit(n, alpha, shift):
    vec, d, noise = _data(n)
    chk = CpuCheckerBackend()
    tv = [torch.from_numpy(vec.copy())]
    lay = chk.layout(tv)
    vc, pc = (torch.zeros(lay.flat_size, dtype=torch.float32) for _ in range(2))
    chk.neumann_init(lay, tv, vc, pc)
    v, p = vec.copy(), vec.copy()
    s0 = lay.starts[0]
    for k in range(K):
        h = _hvp(d, v, noise[k])
        out_scale = -alpha if k == K - 1 else 0.0
        v, p = ref.neumann_step(h, v, p, alpha, shift, out_scale)
        chk.neumann_step(lay, [torch.from_numpy(h)], vc, pc, alpha, out_scale=out_scale, hvp_shift=shift)
        assert _same_bits(v, vc.numpy()[s0:s0 + n]) and _same_bits(p, pc.numpy()[s0:s0 + n]), k


def test_step_length_overrides_and_untouched_inputs():
    """alpha= / beta= replace the step lengths in the element-wise updates only; the dots stay those of the vectors formed; the inputs
    are never written."""
    vec, d, noise = _data(4097)
    x, r, p, rr = ref.cg_init(vec)
    x = (0.5 * vec).astype(np.float32)
    h = _hvp(d, p, noise[0])
    keep = [a.copy() for a in (h, x, r, p)]
    (x1, r1, p1), s1, _ = ref.cg_step(h, x, r, p, rr, 0.7, 0.3, -0.7)
    (x2, r2, p2), s2, _ = ref.cg_step(h, x, r, p, rr, 0.7, 0.3, -0.7, alpha=s1[2], beta=s1[4])
    assert s1 == s2 and _same_bits(x1, x2) and _same_bits(r1, r2) and _same_bits(p1, p2)
    a_up = float(np.nextafter(np.float32(s1[2]), np.float32(np.inf)))
    (x3, r3, p3), s3, _ = ref.cg_step(h, x, r, p, rr, 0.7, 0.3, -0.7, alpha=a_up, beta=0.5)
    assert s3[1] == s1[1] and s3[2] == a_up and s3[4] == 0.5
    assert _same_bits(r3, r - np.float32(a_up) * ref.shifted(h, p, 0.3))
    assert _same_bits(p3, r3 + np.float32(0.5) * p)
    assert _same_bits(x3, np.float32(-0.7) * (x + np.float32(a_up) * p))
    assert not _same_bits(r3, r1)
    assert all(_same_bits(a, b) for a, b in zip(keep, (h, x, r, p)))
    # the shift is rounded on its own: h + fl(shift * p), not an fma and not (1 + shift d) p
    hs = ref.shifted(h, p, 2.0)
    assert _same_bits(hs, h + (np.float32(2.0) * p)) and ref.shifted(h, p, 0.0) is h

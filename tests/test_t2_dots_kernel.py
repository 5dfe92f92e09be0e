"""k_t2_dots (csrc/bhg_mlp_tail.hip) through its own entry bhg_mlp_t2_dots: the launch that replaces the R-backward products of the
last iteration of a fused CG solve without a solution vector.  Per layer, the slots of partT2 it owns must sum to
2 * sum_{m < B, n} Gb[m][n] * Rh[m][n] (numpy fp64), every one of them written, nothing around them touched, rows >= B never read,
and a second run must give the same bits.

The gate.  A product of two floats is exact in fp64 (24 + 24 significant bits), so kernel and reference add the SAME numbers and differ
by the order of an fp64 sum only: 1e-12 relative.  The inputs carry a positive mean (products average 0.25 + ...), so the sum does not
cancel and "relative" means what it says at every size, B = 1 with 32 columns included.

Shapes: RB in {32, 96, 1536} (one float4 row of a wave / less than one workgroup's round / many workgroups with an uneven last one),
RA = 32 * ceil(B / 32) for B in {1, 31, 32, 33, 100}, one layer and three layers (all three widths, in both orders of size) per launch."""
import ctypes

import numpy as np
import pytest
import torch

from betty_amd import _native

RBS, BS = (32, 96, 1536), (1, 31, 32, 33, 100)
GATE = 1e-12
SENTINEL = -12345.678
_I = ctypes.POINTER(ctypes.c_int)


def _layers(widths, B, seed):
    """[(Gb, Rh)] on the device: fp32 [RA][RB], rows < B drawn with mean 0.5, rows >= B NaN."""
    g = torch.Generator().manual_seed(seed)
    RA = 32 * ((B + 31) // 32)
    out = []
    for RB in widths:
        pair = []
        for _ in range(2):
            a = torch.full((RA, RB), float("nan"), dtype=torch.float32)
            a[:B] = 0.5 + torch.randn((B, RB), generator=g, dtype=torch.float32)
            pair.append(a.to("cuda:0"))
        out.append(tuple(pair))
    return RA, out


def _launch(layers, RA, B, part, offs):
    lib = _native.load()
    n = len(layers)
    gb = (ctypes.c_void_p * n)(*[a.data_ptr() for a, _ in layers])
    rh = (ctypes.c_void_p * n)(*[b.data_ptr() for _, b in layers])
    ra = (ctypes.c_int * n)(*([RA] * n))
    rb = (ctypes.c_int * n)(*[a.shape[1] for a, _ in layers])
    off = (ctypes.c_int * n)(*offs)
    rc = lib.bhg_mlp_t2_dots(n, ctypes.cast(gb, _native._PP), ctypes.cast(rh, _native._PP), ctypes.cast(ra, _I), ctypes.cast(rb, _I), B,
                             part.data_ptr(), ctypes.cast(off, _I), None)
    assert rc == 0, lib.bhg_last_error()
    torch.cuda.synchronize()


def _check(widths, B, seed):
    RA, layers = _layers(widths, B, seed)
    slots = [(RA // 32) * (RB // 32) for RB in widths]
    lead, tail = 3, 5
    offs = [lead + sum(slots[:i]) for i in range(len(widths))]
    total = lead + sum(slots) + tail
    part = torch.full((total,), SENTINEL, dtype=torch.float64, device="cuda:0")
    _launch(layers, RA, B, part, offs)
    first = part.cpu().numpy().copy()
    assert (first[:lead] == SENTINEL).all() and (first[total - tail:] == SENTINEL).all(), "slots outside the layers' ranges were written"
    for (a, b), off, ns, RB in zip(layers, offs, slots, widths):
        mine = first[off: off + ns]
        assert np.isfinite(mine).all() and not (mine == SENTINEL).any(), "every slot of a layer is written: a partial or 0.0"
        want = 2.0 * float((a[:B].cpu().numpy().astype(np.float64) * b[:B].cpu().numpy().astype(np.float64)).sum())
        got = float(mine.sum())
        err = abs(got - want) / abs(want)
        print(f"T2D RB={RB} RA={RA} B={B} layers={len(widths)} slots={ns} nonzero={int((mine != 0).sum())} rel={err:.2e} gate={GATE:.0e}")
        assert err <= GATE, (RB, B, err)
    part.fill_(SENTINEL)
    _launch(layers, RA, B, part, offs)
    assert np.array_equal(part.cpu().numpy(), first), "a second run is bit-equal to the first"


@pytest.mark.gpu
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("RB", RBS)
def test_one_layer(RB, B):
    _check([RB], B, 1000 * RB + B)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("widths", [(1536, 96, 32), (32, 1536, 96)], ids=lambda w: "x".join(map(str, w)))
def test_three_layers_in_one_launch(widths, B):
    _check(list(widths), B, 7 * sum(widths) + B)


def test_bad_arguments_are_refused_before_any_launch():
    """Host checks only (no device is touched): layer count, NULL tables, widths and rows that are no multiples of 32, B beyond RA."""
    lib = _native.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    one = lambda v: ctypes.cast((ctypes.c_int * 1)(v), _I)
    ptr = lambda v: ctypes.cast((ctypes.c_void_p * 1)(v), _native._PP)
    call = lambda n=1, gb=p, rh=p, RA=32, RB=32, B=1, part=p, off=0: lib.bhg_mlp_t2_dots(n, ptr(gb), ptr(rh), one(RA), one(RB), B, part, one(off), None)
    for kw in (dict(n=0), dict(n=33), dict(gb=0), dict(rh=None), dict(gb=p + 4), dict(RA=48), dict(RB=40), dict(RB=0), dict(B=0), dict(B=33),
               dict(part=None), dict(off=-1)):
        assert call(**kw) == -1, kw
    null = ctypes.cast(None, _native._PP)
    assert lib.bhg_mlp_t2_dots(1, null, ptr(p), one(32), one(32), 1, p, one(0), None) == -1

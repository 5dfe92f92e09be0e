"""The finite-difference kernels of csrc/bhg_fd.hip, called directly: ``bhg_mlp_fd_forward`` (CE at w+ and w-, the inner weights left
where the reference's three axpys leave them) and ``bhg_mwn_fd_vjp`` (the meta-weight-net VJP at both points), at the batches, widths,
depths and class counts where tiled kernels go wrong, against fp64 restatements of the same operations.

Tolerances follow the fp64-truth rule of the repository: the kernel's distance to an fp64 truth may be at most twice the distance of the
same computation in fp32 ATen (or autograd), or a small stated floor, whichever is larger; a plain cap independent of ATen applies too.
The weights after a call are compared bit for bit with the backend's own ``axpy_multi`` (what the header promises)."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import zoo
from conftest import rel_err

from betty_amd import Config, _native
from betty_amd import hypergradient as hg

DEV = "cuda"
R = 0.01          # Config.darts_alpha's default: eps = R / ||v||
U32 = 2.0 ** -24  # unit roundoff of fp32

# the tile shapes of csrc/bhg_fd.hip, restated (what the sweep has to straddle)
TM, TN, TK, WG_TARGET, MAX_SPLITS, MAX_B = 128, 32, 32, 512, 32, 512


def fd_splits(N, K):
    """The split-K count of csrc/bhg_fd.hip, restated: about WG_TARGET workgroups, at most MAX_SPLITS and one per K step, and as many
    as leave the last split a non-empty range of K steps."""
    tiles, ksteps = -(-N // TN), -(-K // TK)
    s = max(1, min(WG_TARGET // tiles, MAX_SPLITS, ksteps))
    while s > 1 and (s - 1) * -(-ksteps // s) >= ksteps:
        s -= 1
    return s


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _fd_lib():
    try:
        return _native.load()
    except _native.NativeLibraryError as exc:
        pytest.skip(f"libbhg not built: {exc}")


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: argument validation and the workspace's split count (no launch, no device)
# ---------------------------------------------------------------------------------------------------------------------------------
def _dims(d):
    return (ctypes.c_int * len(d))(*d)


def test_fd_argument_validation_without_gpu():
    """Bad shapes are refused before any HIP call: bhg_mlp_fd_ws_bytes returns 0, bhg_mlp_fd_forward and bhg_mwn_fd_vjp return a non-zero
    code with a message.  Every pointer below is a valid host address, so only the checks stand between these calls and a launch."""
    lib = _fd_lib()
    good, B = [8, 16, 4], 4
    assert lib.bhg_mlp_fd_ws_bytes(_dims(good), 2, B) > 0
    bad = [(good, 2, 0), (good, 2, MAX_B + 1), ([8, 0, 4], 2, B), ([0, 16, 4], 2, B), ([8, 16, 0], 2, B), (good, 0, B),
           ([4] * 34, 33, B)]
    for d, L, b in bad:
        assert lib.bhg_mlp_fd_ws_bytes(_dims(d), L, b) == 0, (d, L, b)
    assert lib.bhg_mlp_fd_ws_bytes(None, 2, B) == 0

    host = (ctypes.c_float * 64)()
    p = ctypes.addressof(host)
    tab = (ctypes.c_void_p * 64)(*([p] * 64))
    ptab = ctypes.cast(tab, _native._PP)

    def fwd(d, L, b, ws_bytes):
        return lib.bhg_mlp_fd_forward(p, p, b, _dims(d), L, ptab, ptab, p, 1, p, p, p, ws_bytes, None)

    for d, L, b in bad:
        assert fwd(d, L, b, 1 << 30) != 0, (d, L, b)
        assert lib.bhg_last_error(), (d, L, b)
    assert fwd(good, 2, MAX_B + 1, 1 << 30) != 0 and b"batch" in lib.bhg_last_error()
    assert fwd([8, 0, 4], 2, B, 1 << 30) != 0 and b"width" in lib.bhg_last_error()
    assert fwd(good, 33, B, 1 << 30) != 0 and b"layer" in lib.bhg_last_error()
    need = lib.bhg_mlp_fd_ws_bytes(_dims(good), 2, B)
    assert fwd(good, 2, B, need - 1) != 0 and b"workspace" in lib.bhg_last_error()
    assert lib.bhg_mlp_fd_forward(None, p, B, _dims(good), 2, ptab, ptab, p, 1, p, p, p, need, None) != 0
    assert b"NULL" in lib.bhg_last_error()

    def vjp(b, H):
        return lib.bhg_mwn_fd_vjp(p, p, b, p, p, p, p, H, p, 0, p, p, p, p, None)

    for b, H in ((4, 0), (4, 2049), (4, -1), (0, 4)):
        assert vjp(b, H) != 0, (b, H)
        assert b"hidden width" in lib.bhg_last_error(), (b, H)
    assert lib.bhg_mwn_fd_vjp(None, p, 4, p, p, p, p, 4, p, 0, p, p, p, p, None) != 0 and b"NULL" in lib.bhg_last_error()


# (K, N) pairs whose split count is 1, uneven (the last split shorter), or the cap of 32
SPLIT_SHAPES = [(1, 10), (3, 1), (31, 2048), (32, 33), (33, 33), (33, 2048), (100, 10), (100, 2048), (970, 1024), (1000, 31),
                (1000, 2048), (2048, 64), (3000, 2048), (3072, 10), (3072, 65), (3072, 2048), (5000, 1)]


@pytest.mark.parametrize("K,N", SPLIT_SHAPES)
def test_fd_split_count_partitions_k(K, N):
    """The split count the library sizes its partials for, read back from bhg_mlp_fd_ws_bytes of a one-layer net at B = 32 (where every
    region of the workspace is a multiple of its 256-byte alignment): every split owns a non-empty range of K steps, there are at most
    32 of them, and the count is the restated rule's."""
    lib = _fd_lib()
    B = 32
    slab = 2 * B * N * 4   # one split's [2][B][N] partials; also the [2][B][C] logits (C = N here)
    total = lib.bhg_mlp_fd_ws_bytes(_dims([K, N]), 1, B)
    bpm = -(-(2 * N * 4) // 256) * 256
    rest = total - slab - bpm
    assert rest > 0 and rest % slab == 0, (total, slab, bpm)
    s = rest // slab
    ksteps = -(-K // TK)
    per = -(-ksteps // s)
    assert 1 <= s <= min(MAX_SPLITS, ksteps), s
    assert (s - 1) * per < ksteps, (s, per, ksteps)   # the last split is not empty
    assert s * per >= ksteps                          # ... and the splits cover K
    assert s == fd_splits(N, K), (s, fd_splits(N, K))


def test_split_shapes_cover_the_partition_cases():
    got = {fd_splits(N, K) for K, N in SPLIT_SHAPES}
    assert 1 in got and MAX_SPLITS in got
    uneven = [(K, N) for K, N in SPLIT_SHAPES if fd_splits(N, K) > 1 and -(-K // TK) % fd_splits(N, K)]
    assert uneven


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: bhg_mlp_fd_forward
# ---------------------------------------------------------------------------------------------------------------------------------
class _Net:
    """Random fp32 weights, direction, input and labels of a ReLU MLP with widths ``dims`` at batch ``B`` (fixed seed)."""

    def __init__(self, dims, B, seed):
        g = torch.Generator().manual_seed(seed)
        self.dims, self.B, self.L = list(dims), B, len(dims) - 1
        self.params, self.dirs = [], []
        for K, N in zip(dims[:-1], dims[1:]):
            bound = 1.0 / math.sqrt(K)   # nn.Linear's initialisation
            self.params += [(torch.rand(N, K, generator=g) * 2 - 1) * bound, (torch.rand(N, generator=g) * 2 - 1) * bound]
            self.dirs += [0.01 * torch.randn(N, K, generator=g), 0.01 * torch.randn(N, generator=g)]
        self.x = torch.randn(B, dims[0], generator=g)
        self.y = torch.randint(0, dims[-1], (B,), generator=g)
        self.to(DEV)

    def to(self, dev):
        self.params = [t.to(dev).contiguous() for t in self.params]
        self.dirs = [t.to(dev).contiguous() for t in self.dirs]
        self.x, self.y = self.x.to(dev).contiguous(), self.y.to(dev).contiguous()
        return self


def _forward(h, params, dtype):
    L = len(params) // 2
    h = h.to(dtype)
    for l in range(L):
        h = F.linear(h, params[2 * l].to(dtype), params[2 * l + 1].to(dtype))
        if l + 1 < L:
            h = torch.relu(h)
    return h


def _ce(z, y):
    return torch.logsumexp(z, dim=1) - z.gather(1, y.reshape(-1, 1)).reshape(-1)


def _run_fd_forward(net, restore):
    """One bhg_mlp_fd_forward through the C ABI.  Returns (ce [2][B], eps32, (w+, w-) as the backend's axpys produce them, the weights
    the backend's axpys leave); ``net.params`` hold the kernel's final weights afterwards."""
    from betty_amd.backend import get_backend

    be = get_backend()
    lib = _native.load()
    layout = be.layout(net.dirs)
    eps32, _, _ = be.darts_eps(layout, net.dirs, R)
    eps32 = eps32.reshape(1).contiguous()
    # the reference: darts.py's three in-place axpys on a copy of the weights
    w = [p.clone() for p in net.params]
    be.axpy_multi(layout, w, net.dirs, eps32[0], 1.0)
    wp = [t.clone() for t in w]
    be.axpy_multi(layout, w, net.dirs, eps32[0], -2.0)
    wm = [t.clone() for t in w]
    if restore:
        be.axpy_multi(layout, w, net.dirs, eps32[0], 1.0)

    dims_c = _dims(net.dims)
    n = int(lib.bhg_mlp_fd_ws_bytes(dims_c, net.L, net.B))
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    ce = torch.full((2, net.B), float("nan"), device=DEV)
    ptab, _pk = _native.ptr_array([p.data_ptr() for p in net.params])
    dtab, _dk = _native.ptr_array([d.data_ptr() for d in net.dirs])
    _native.check(lib.bhg_mlp_fd_forward(net.x.data_ptr(), net.y.data_ptr(), net.B, dims_c, net.L, ptab, dtab, eps32.data_ptr(),
                                         int(restore), ce[0].data_ptr(), ce[1].data_ptr(), ws.data_ptr(), n, _stream()),
                  "bhg_mlp_fd_forward")
    torch.cuda.synchronize()
    return ce, eps32, (wp, wm), w


def _check_ce(net, ce, wpm, what):
    """CE+ and CE- of the kernel against the fp64 forward at the fp32 perturbed weights: at most max(2 e_aten, floor) per sample, where
    e_aten is fp32 ATen's (F.linear) largest distance to the same truth, and never more than the plain cap."""
    for s, w in enumerate(wpm):
        z64 = _forward(net.x, w, torch.float64)
        truth = _ce(z64, net.y)
        z32 = _forward(net.x, w, torch.float32)
        e_aten = float((_ce(z32, net.y).double() - truth).abs().max())
        got = ce[s].double()
        assert torch.isfinite(got).all(), (what, s)
        err = (got - truth).abs()
        # the CE of a row is a difference of logits: its rounding is at the scale of the row's largest |z|
        zmax = z64.abs().amax(dim=1)
        floor = 1e-5 * (1.0 + truth.abs()) + 2.0 ** -21 * zmax
        bound = torch.clamp(floor, min=2.0 * e_aten)
        cap = 1e-4 * (1.0 + truth.abs()) + 2.0 ** -19 * zmax
        worst = int(torch.argmax(err - bound))
        assert bool((err <= bound).all()), (what, "+-"[s], worst, float(err[worst]), float(bound[worst]), e_aten)
        assert bool((err <= cap).all()), (what, "+-"[s], float((err / cap).max()))


def _check_weights(net, want, what):
    for i, (a, b) in enumerate(zip(net.params, want)):
        assert torch.equal(a, b), (what, i, float((a - b).abs().max()))


# (dims, batch, restore): every batch of 1..512 around the 128-row tiles (MT = 1..4), every width, class count and depth below, each
# of them at least once with more than one M tile
FWD_CASES = [
    ([1, 33, 10], 129, 1),
    ([3, 65, 1, 31, 257], 257, 0),
    ([31, 32, 1000], 384, 1),
    ([33, 2048, 2], 385, 0),
    ([100, 10, 1], 511, 1),
    ([1000, 257], 512, 0),
    ([3072, 65, 31, 32, 10], 256, 1),
    ([32, 31, 10], 128, 0),
    ([33] + [31] * 11 + [10], 257, 1),       # L = 12, narrow
    ([1000, 33, 1000], 385, 1),
    ([3072, 10], 1, 1),
    ([1, 1, 2], 2, 0),
    ([100, 2048, 257], 31, 1),
    ([32, 32, 10], 127, 1),
]


def test_fwd_cases_cover_the_sweep():
    """Every batch, K, hidden N, class count and depth the sweep is meant to reach is in FWD_CASES, each (but the small batches) with
    more than one M tile."""
    multi = [c for c in FWD_CASES if c[1] > TM]
    assert {1, 2, 31, 127, 128, 129, 256, 257, 384, 385, 511, 512} <= {b for _, b, _ in FWD_CASES}
    assert {1, 3, 31, 32, 33, 100, 1000, 3072} <= {k for d, _, _ in multi for k in d[:-1]}
    assert {1, 10, 31, 32, 33, 65, 2048} <= {n for d, _, _ in multi for n in d[1:-1]}
    assert {1, 2, 10, 257, 1000} <= {d[-1] for d, _, _ in multi}
    assert {1, 2, 4, 12} <= {len(d) - 1 for d, _, _ in multi}
    assert {0, 1} == {r for _, _, r in multi}
    assert {(b + TM - 1) // TM for _, b, _ in FWD_CASES} == {1, 2, 3, 4}


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B,restore", FWD_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_fd_forward_matches_fp64(dims, B, restore):
    net = _Net(dims, B, seed=B * 131 + sum(dims) + restore)
    ce, _, wpm, w_final = _run_fd_forward(net, restore)
    _check_weights(net, w_final, (dims, B, restore))
    _check_ce(net, ce, wpm, (dims, B, restore))


@pytest.mark.gpu
def test_fd_forward_large_logits():
    """|z| of about 1e3: the max shift of k_fd_ce's logsumexp (exp(z) itself overflows fp32 above 88)."""
    net = _Net([100, 65, 10], 129, seed=11)
    z = _forward(net.x, net.params, torch.float32)
    net.x.mul_(1e3 / float(z.abs().max()))
    assert float(_forward(net.x, net.params, torch.float32).abs().max()) > 500
    ce, _, wpm, w_final = _run_fd_forward(net, 1)
    _check_weights(net, w_final, "large logits")
    assert float(ce.abs().max()) > 10.0
    _check_ce(net, ce, wpm, "large logits")


@pytest.mark.gpu
def test_fd_forward_tied_maximum():
    """Two classes hold the same, largest logit in every row (identical weight rows and directions, a large common bias); labels on
    both tied classes and on others."""
    net = _Net([31, 33, 10], 257, seed=12)
    W, b, V, vb = net.params[2], net.params[3], net.dirs[2], net.dirs[3]
    W[4].copy_(W[7])
    V[4].copy_(V[7])
    b[7] += 5.0
    b[4].copy_(b[7])
    vb[4].copy_(vb[7])
    net.x[1].copy_(net.x[0])   # samples 0 and 1: the same row, labelled with either tied class
    net.y[:4] = torch.tensor([4, 7, 0, 9], device=DEV)
    z = _forward(net.x, net.params, torch.float64)
    assert torch.equal(z[:, 4], z[:, 7]) and bool((z[:, 4] >= z.amax(dim=1)).all())
    ce, _, wpm, w_final = _run_fd_forward(net, 1)
    _check_weights(net, w_final, "tied")
    _check_ce(net, ce, wpm, "tied")
    assert torch.equal(ce[:, 0], ce[:, 1])


# (K, N, B) of one layer (N classes) with several splits; the uneven ones leave the last split shorter
PARTITION_CASES = [(33, 33, 129), (970, 1024, 257), (2048, 64, 385), (3072, 2048, 512), (100, 10, 511), (3000, 2048, 256)]


def test_partition_cases_have_several_splits():
    s = [fd_splits(N, K) for K, N, _ in PARTITION_CASES]
    assert all(v > 1 for v in s) and MAX_SPLITS in s
    assert any(-(-K // TK) % fd_splits(N, K) for K, N, _ in PARTITION_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("K,N,B", PARTITION_CASES)
def test_fd_forward_split_k_partition(K, N, B):
    """Split K: every K column of W is written by exactly one split and summed exactly once.  With restore = 0 the final weights are
    w - eps v, so a column written twice or never differs from the axpys'.  Then a direction with one non-zero column per row,
    alternating over the columns, so that each K column's perturbation is seen alone in its row's CE."""
    net = _Net([K, N], B, seed=K + N + B)
    ce, _, wpm, w_final = _run_fd_forward(net, 0)
    _check_weights(net, w_final, ("dense", K, N, B))
    _check_ce(net, ce, wpm, ("dense", K, N, B))
    rows = torch.arange(N, device=DEV)
    for shift in range(0, K, N):
        net = _Net([K, N], B, seed=K + N + B)
        V = torch.zeros(N, K, device=DEV)
        V[rows, (rows + shift) % K] = 0.5 + torch.rand(N, device=DEV)
        net.dirs[0] = V
        ce, _, wpm, w_final = _run_fd_forward(net, shift % 2)
        _check_weights(net, w_final, ("one-hot", K, N, B, shift))
        _check_ce(net, ce, wpm, ("one-hot", K, N, B, shift))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: bhg_mwn_fd_vjp
# ---------------------------------------------------------------------------------------------------------------------------------
def _mwn_grads(net, ce, dtype):
    """d/d(params) of mean_i s(ce_i) ce_i for ce held fixed (the meta-weight-net half of the reweighting loss), by autograd."""
    ps = [p.detach().to(dtype).requires_grad_(True) for p in (net.l1.weight, net.l1.bias, net.l2.weight, net.l2.bias)]
    c = ce.detach().to(dtype)
    h = torch.relu(F.linear(c.reshape(-1, 1), ps[0], ps[1]))
    s = torch.sigmoid(F.linear(h, ps[2], ps[3])).reshape(-1)
    return torch.autograd.grad((s * c).mean(), ps)


def _vjp(lib, cep, cem, net, two_eps, accumulate, outs):
    ts = [t.detach().contiguous() for t in (net.l1.weight, net.l1.bias, net.l2.weight, net.l2.bias)]
    H = ts[0].shape[0]
    _native.check(lib.bhg_mwn_fd_vjp(cep.data_ptr(), cem.data_ptr(), cep.numel(), ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(),
                                     ts[3].data_ptr(), H, two_eps.data_ptr(), int(accumulate), outs[0].data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), outs[3].data_ptr(), _stream()), "bhg_mwn_fd_vjp")
    torch.cuda.synchronize()
    return outs


MWN_CASES = [(1, 1), (5, 2048), (100, 100), (512, 300), (1024, 64), (1025, 64), (2500, 257)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H", MWN_CASES)
def test_mwn_fd_vjp_matches_fp64(B, H):
    """(g- - g+) / (2 eps) at nearby CE+ and CE-, written and accumulated onto a .grad of order 1e2, against autograd in fp64."""
    lib = _native.load()
    torch.manual_seed(B * 17 + H)
    net = zoo.MWN(H).to(DEV)
    cep = (0.1 + 2.5 * torch.rand(B, device=DEV)).contiguous()
    cem = (cep + 1e-3 * (1.0 + 0.5 * torch.randn(B, device=DEV))).contiguous()   # a finite difference: a drift, and noise
    two_eps = torch.tensor([2e-3], device=DEV)
    te64 = float(two_eps)

    gp64, gm64 = _mwn_grads(net, cep, torch.float64), _mwn_grads(net, cem, torch.float64)
    gp32, gm32 = _mwn_grads(net, cep, torch.float32), _mwn_grads(net, cem, torch.float32)
    truth = [((m - p) / te64).reshape(-1) for p, m in zip(gp64, gm64)]
    aten = [((m - p) / two_eps).reshape(-1).double() for p, m in zip(gp32, gm32)]
    bounds = []
    for t, a, p, m in zip(truth, aten, gp64, gm64):
        e_aten = float((a - t).abs().max())
        # g+ and g- each carry a few ulp of themselves (no gradient here cancels: ce > 0, ReLU >= 0, and the kernel sums in double);
        # their difference keeps that absolute rounding, divided by 2 eps
        floor = 8.0 * U32 * (p.abs() + m.abs()).reshape(-1) / te64
        bounds.append(torch.clamp(floor, min=2.0 * e_aten))

    def check(got, what):
        for i, (g, t, bd) in enumerate(zip(got, truth, bounds)):
            err = (g.double().reshape(-1) - t).abs()
            assert torch.isfinite(g).all(), (what, i)
            j = int(torch.argmax(err - bd))
            assert bool((err <= bd).all()), (what, B, H, i, j, float(err[j]), float(bd[j]))

    shapes = [(H, 1), (H,), (1, H), (1,)]
    out = _vjp(lib, cep, cem, net, two_eps, 0, [torch.full(s, float("nan"), device=DEV) for s in shapes])
    check(out, "write")

    fill = [1e2 * torch.randn(s, device=DEV) for s in shapes]
    acc = _vjp(lib, cep, cem, net, two_eps, 1, [f.clone() for f in fill])
    fmax = max(float(f.abs().max()) for f in fill)
    ulp4 = 4.0 * 2.0 ** (math.floor(math.log2(fmax)) - 23)   # the rounding of the two fp32 additions onto the fill
    for i, (a, f, t, bd) in enumerate(zip(acc, fill, truth, bounds)):
        err = ((a.double() - f.double()).reshape(-1) - t).abs()
        assert bool((err <= bd + ulp4).all()), ("accumulate", B, H, i, float((err - bd - ulp4).max()))

    # the reference's order: (.grad + -(g+ / 2eps)) + g- / 2eps.  A zero CE makes a point's gradient exactly zero, so the kernel itself
    # returns -(g+ / 2eps) and g- / 2eps alone; the accumulated result is those two fp32 additions, bit for bit
    zero = torch.zeros_like(cep)
    neg_p = _vjp(lib, cep, zero, net, two_eps, 0, [torch.empty(s, device=DEV) for s in shapes])
    pos_m = _vjp(lib, zero, cem, net, two_eps, 0, [torch.empty(s, device=DEV) for s in shapes])
    for i, (a, f, n, m) in enumerate(zip(acc, fill, neg_p, pos_m)):
        assert torch.equal(a, (f + n) + m), ("accumulate order", B, H, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: end to end through hg.darts at the new shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def _reweight_problem(dims, B, H, seed, dtype=torch.float32, declare=False):
    torch.manual_seed(seed)
    inner, upper = zoo.MLP(dims), zoo.MWN(H)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, dims[0], generator=g)
    y = torch.randint(0, dims[-1], (B,), generator=g)
    vector = [0.01 * torch.randn(p.shape, generator=g) for p in inner.parameters()]
    inner, upper = inner.to(device=DEV, dtype=dtype), upper.to(device=DEV, dtype=dtype)
    vector = [v.to(device=DEV, dtype=dtype) for v in vector]
    prev = zoo.StubProblem("upper", upper, config=Config())
    curr = zoo.StubProblem("inner", inner, config=Config(type="darts", darts_alpha=R),
                           loss_fn=zoo.make_reweight_loss(prev, zoo.RIDGE["reweight"]), batch=(x.to(DEV, dtype), y.to(DEV)))
    if declare:
        from betty_amd.hypergradient.structured import SigmoidMLPWeightNet, WeightedCEMLP

        curr.hypergradient_structure = lambda p: WeightedCEMLP(
            curr, p, layers=list(curr.module.layers), weight_fn=lambda ce: p.fwd(ce.reshape(-1, 1)), ridge=zoo.RIDGE["reweight"],
            impl="hip", verify=False, weight_net=SigmoidMLPWeightNet(p.module.l1, p.module.l2))

        def boom(batch):
            raise AssertionError("the opaque path ran: training_step_exec was called")

        curr.training_step_exec = boom   # only the native hop can succeed
    return curr, prev, vector


# MT = 2, 3, 4 and an uneven split (K = 33 over 2 splits, K = 970 over 16)
E2E_SHAPES = [([1, 33, 10], 129), ([31, 32, 1000], 384), ([33, 2048, 2], 385), ([970, 1024, 10], 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B", E2E_SHAPES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_darts_native_hop_at_new_shapes(dims, B):
    """hg.darts through the native hop and through the opaque path (training_step_exec) on the same problem: the inner weights left
    behind are bit-identical, and the hypergradient is within 2x of the opaque fp32 result's distance to an fp64 truth (2e-3 floor),
    the rule of test_structured_fd.py::test_hip_cfg2_scale_agrees_with_the_opaque_path."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import hypergrad_oracle as horc

    seed = B + sum(dims)
    curr, prev, vector = _reweight_problem(dims, B, 16, seed, declare=True)
    got = [t.clone() for t in hg.darts(vector, curr, prev, False)]
    curr_o, prev_o, vector_o = _reweight_problem(dims, B, 16, seed)
    want = [t.clone() for t in hg.darts(vector_o, curr_o, prev_o, False)]
    for a, b in zip(curr.module.parameters(), curr_o.module.parameters()):
        assert torch.equal(a.data, b.data)
    curr64, prev64, vector64 = _reweight_problem(dims, B, 16, seed, dtype=torch.float64)
    truth = [t.detach().clone() for t in horc.darts(vector64, curr64, prev64, False)]
    np_ = lambda ts: [t.detach().double().cpu().numpy() for t in ts]
    e_ref, _ = rel_err(np_(want), np_(truth))
    e_got, _ = rel_err(np_(got), np_(truth))
    print(f"{dims} B={B}: darts vs fp64 truth: opaque {e_ref:.2e}, native {e_got:.2e}")
    assert e_got <= max(2e-3, 2.0 * e_ref), (e_got, e_ref)

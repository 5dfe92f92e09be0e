"""Restatement of the TILED scheme of csrc/bhg_attention_tiled.hip in plain tensor operations (the tests pass float64): the same
quantities as tests/attention_ref.py (its docstring has the notation), computed the way the two launches compute them, so that a
wrong identity shows without a GPU.  tests/test_attention_tiled_ref.py holds it to attention_ref.attention_backward_vjp.

Score tiles are BM = 64 queries x BN = 32 keys.  Per block of 64 query rows:
  (a) ONE online pass over the key tiles keeps a running row maximum m and five unnormalised sums, with e = exp(score - m):
          sum e      sum e gP      sum e T      sum e T gP      sum e (go av^T)
      When the maximum moves the sums are rescaled by exp(m_old - m_new).  While the maximum is still -inf (every key so far masked) the
      sums are empty and are left alone, and e is taken against 0 instead of m, so exp(-inf - 0) = 0 and nothing turns NaN.  At the end
          l = sum e     D = (sum e gP) / l     E = (sum e T) / l
          R = rowsum(P * bP) = (sum e T gP) / l - 2 D E + (sum e (go av^T)) / l
      (bP = T * (gP - D) - gP * E + go av^T summed against P, with rowsum(P) = 1).  A fully masked row ends with l = 0: NaN.
  (b) a second sweep recomputes the tile's raw products, forms P = exp(score - m) / l, gS, bgP, bS from the finished statistics and
      accumulates dq = s (bS k + gS ak) and dgo = bgP v + P av over the key tiles.
Per block of 32 keys, the second launch sweeps the query tiles with the same statistics and accumulates dv = bgP^T go and
dk = s (bS^T q + gS^T aq) over the query tiles.  Under `causal` the tiles wholly above the diagonal are skipped in both."""
import torch

import attention_ref

BM, BN = 64, 32


def _tile(q, k, v, go, aq, ak, av, mask, causal, scale, i0, i1, j0, j1):
    """(score, gP, T, W = go av^T) of the tile [i0, i1) x [j0, j1): (B, H, i1 - i0, j1 - j0) each."""
    qs, gos, ks, vs = q[..., i0:i1, :], go[..., i0:i1, :], k[..., j0:j1, :], v[..., j0:j1, :]
    sc = scale * (qs @ ks.transpose(-1, -2))
    if mask is not None:
        sc = sc + mask.expand(*sc.shape[:2], q.shape[2], k.shape[2])[..., i0:i1, j0:j1]
    if causal:
        i = torch.arange(i0, i1).view(-1, 1)
        j = torch.arange(j0, j1).view(1, -1)
        sc = sc.masked_fill(j > i, float("-inf"))
    gP = gos @ vs.transpose(-1, -2)
    T = torch.zeros_like(gP)
    if aq is not None:
        T = T + scale * (aq[..., i0:i1, :] @ ks.transpose(-1, -2))
    if ak is not None:
        T = T + scale * (qs @ ak[..., j0:j1, :].transpose(-1, -2))
    W = gos @ av[..., j0:j1, :].transpose(-1, -2) if av is not None else torch.zeros_like(gP)
    return sc, gP, T, W


def _key_tiles(i1, S, causal):
    """The key tiles a block of query rows ending at i1 sweeps: under `causal` those with a key j <= i1 - 1."""
    last = min(S, i1) if causal else S
    return [(j0, min(j0 + BN, S)) for j0 in range(0, last, BN)]


def row_statistics(q, k, v, go, aq, ak, av, mask=None, causal=False, scale=None):
    """(m, l, D, E, R), each (B, H, L, 1), by the online pass."""
    scale = attention_ref.default_scale(q.shape[-1]) if scale is None else scale
    B, H, L, _ = q.shape
    S = k.shape[2]
    out = [[] for _ in range(5)]
    for i0 in range(0, L, BM):
        i1 = min(i0 + BM, L)
        m = torch.full((B, H, i1 - i0, 1), float("-inf"), dtype=q.dtype)
        sums = [torch.zeros(B, H, i1 - i0, 1, dtype=q.dtype) for _ in range(5)]
        for j0, j1 in _key_tiles(i1, S, causal):
            sc, gP, T, W = _tile(q, k, v, go, aq, ak, av, mask, causal, scale, i0, i1, j0, j1)
            m_new = torch.maximum(m, sc.amax(-1, keepdim=True))
            empty = torch.isinf(m) & (m < 0)                                   # nothing summed yet: nothing to rescale
            f = torch.where(empty, torch.ones_like(m), torch.exp(torch.where(empty, torch.zeros_like(m), m) - torch.where(empty, torch.zeros_like(m), m_new)))
            e = torch.exp(sc - torch.where(torch.isinf(m_new) & (m_new < 0), torch.zeros_like(m_new), m_new))
            terms = (e, e * gP, e * T, e * (T * gP), e * W)
            sums = [s * f + t.sum(-1, keepdim=True) for s, t in zip(sums, terms)]
            m = m_new
        l = sums[0]
        D, E = sums[1] / l, sums[2] / l
        R = sums[3] / l - 2.0 * D * E + sums[4] / l
        for o, t in zip(out, (m, l, D, E, R)):
            o.append(t)
    return tuple(torch.cat(o, dim=2) for o in out)


def _tile_matrices(tile, stats, i0, i1):
    """(P, gS, bgP, bS) of a tile from its raw products and the finished statistics of its rows."""
    sc, gP, T, W = tile
    m, l, D, E, R = (t[..., i0:i1, :] for t in stats)
    P = torch.exp(sc - torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)) / l
    bP = T * (gP - D) - gP * E + W
    return P, P * (gP - D), P * (T - E), P * (bP - R)


def attention_backward_vjp(q, k, v, go, aq, ak, av, mask=None, causal=False, scale=None):
    """The signature and the result of attention_ref.attention_backward_vjp, by the tiled scheme."""
    scale = attention_ref.default_scale(q.shape[-1]) if scale is None else scale
    L, S = q.shape[2], k.shape[2]
    stats = row_statistics(q, k, v, go, aq, ak, av, mask, causal, scale)
    args = (q, k, v, go, aq, ak, av, mask, causal, scale)
    # launch 1 (b): blocks of query rows, sums over the key tiles
    dq, dgo = torch.zeros_like(q), torch.zeros_like(go)
    for i0 in range(0, L, BM):
        i1 = min(i0 + BM, L)
        for j0, j1 in _key_tiles(i1, S, causal):
            P, gS, bgP, bS = _tile_matrices(_tile(*args, i0, i1, j0, j1), stats, i0, i1)
            dq[..., i0:i1, :] += bS @ k[..., j0:j1, :]
            if ak is not None:
                dq[..., i0:i1, :] += gS @ ak[..., j0:j1, :]
            dgo[..., i0:i1, :] += bgP @ v[..., j0:j1, :]
            if av is not None:
                dgo[..., i0:i1, :] += P @ av[..., j0:j1, :]
    # launch 2: blocks of keys, sums over the query tiles
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for j0 in range(0, S, BN):
        j1 = min(j0 + BN, S)
        first = j0 // BM * BM if causal else 0          # the query tiles above hold rows i < j0 only
        for i0 in range(first, L, BM):
            i1 = min(i0 + BM, L)
            _, gS, bgP, bS = _tile_matrices(_tile(*args, i0, i1, j0, j1), stats, i0, i1)
            dv[..., j0:j1, :] += bgP.transpose(-1, -2) @ go[..., i0:i1, :]
            dk[..., j0:j1, :] += bS.transpose(-1, -2) @ q[..., i0:i1, :]
            if aq is not None:
                dk[..., j0:j1, :] += gS.transpose(-1, -2) @ aq[..., i0:i1, :]
    return scale * dq, scale * dk, dv, dgo

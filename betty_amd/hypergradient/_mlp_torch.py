"""ATen evaluation of the analytic MLP HVP — the twin of ``_mlp_hip.py`` that ``WeightedCEMLP(impl="torch")`` asks for: the same
formulas with ATen ops, device agnostic.  It is the math reference for the kernels (tests, ``bench.py --hvp analytic-aten``) and
carries the global-batch protocols phase by phase so the gloo tests can run them on a CPU; the package never takes it on its own."""
from __future__ import annotations

import torch
import torch.nn.functional as F


class _TorchMLPState:
    """ATen evaluation of the closed form (device agnostic; the math reference for the kernels)."""

    def __init__(self, spec, x, y):
        self.spec = spec
        Ws = [lin.weight.detach() for lin in spec.layers]
        bs = [lin.bias.detach() for lin in spec.layers]
        B = x.shape[0]
        hs, masks = [x.detach()], []
        h = hs[0]
        for l, (W, b) in enumerate(zip(Ws, bs)):
            a = torch.addmm(b, h, W.t())
            if l + 1 < len(Ws):
                m = (a > 0).to(a.dtype)
                h = a * m
                masks.append(m)
                hs.append(h)
            else:
                z = a
        logp = F.log_softmax(z, dim=1)
        p = logp.exp()
        ce = -logp.gather(1, y.reshape(-1, 1)).reshape(-1)
        self.sample_weight = spec.weight_fn(ce.detach())  # keeps the graph to prev's parameters
        sd = self.sample_weight.detach().reshape(-1) / B
        onehot = F.one_hot(y, z.shape[1]).to(z.dtype)
        self.err = p - onehot  # [B, C]
        deltas = [None] * len(Ws)
        deltas[-1] = sd[:, None] * self.err
        for l in range(len(Ws) - 1, 0, -1):
            deltas[l - 1] = masks[l - 1] * (deltas[l] @ Ws[l])
        self.Ws, self.hs, self.masks, self.p, self.sd, self.deltas, self.B = Ws, hs, masks, p, sd, deltas, B

    native_upper = False
    solution_free = False   # cg_global_phase always writes x (keep_x is not honoured)

    def upper_vjp(self, coeff, upper, retain_graph=False):
        return list(torch.autograd.grad(self.sample_weight, upper, grad_outputs=coeff.reshape(self.sample_weight.shape),
                                        retain_graph=retain_graph, allow_unused=retain_graph))   # (retain_graph: the structure check)

    def _r_forward(self, Vs, cs):
        Rh, Rhs = None, [None]
        for l, (W, V, c) in enumerate(zip(self.Ws, Vs, cs)):
            Ra = torch.addmm(c, self.hs[l], V.t())
            if Rh is not None:
                Ra = Ra + Rh @ W.t()
            if l + 1 < len(self.Ws):
                Rh = self.masks[l] * Ra
                Rhs.append(Rh)
        return Ra, Rhs  # Rz, [None, Rh_1, ..]

    def hvp(self, direction_views):
        Vs, cs = direction_views[0::2], direction_views[1::2]   # (the ridge part is the recurrence kernel's: spec.hvp_shift)
        Rz, Rhs = self._r_forward(Vs, cs)
        Rd = self.sd[:, None] * (self.p * Rz - self.p * (self.p * Rz).sum(1, keepdim=True))
        out = [None] * (2 * len(self.Ws))
        for l in range(len(self.Ws) - 1, -1, -1):
            HW = Rd.t() @ self.hs[l]
            if Rhs[l] is not None:
                HW = HW + self.deltas[l].t() @ Rhs[l]
            out[2 * l] = HW
            out[2 * l + 1] = Rd.sum(0)
            if l > 0:
                Rd = self.masks[l - 1] * (self.deltas[l] @ Vs[l] + Rd @ self.Ws[l])
        return out

    def mixed_coeff(self, dir_views, solve=None):
        if solve is not None:   # the factor-exchange solve: Rz(x) was accumulated, x = -cg_alpha * sum_k alpha_k p_k never existed
            if solve is not getattr(self, "_fx_token", None):
                raise RuntimeError("stale fused-solve token")
            Rz = (-solve[1]) * self._fx["Rzx"].to(self.err.dtype)
            return (self.err * Rz).sum(1) / self.B
        Rz, _ = self._r_forward(dir_views[0::2], dir_views[1::2])
        return (self.err * Rz).sum(1) / self.B

    # ---- global-batch CG, phase by phase: the math bhg_mlp_cg_global_phase implements, in ATen (tests: gloo, CPU) -----------------
    def fused_supported(self, layout) -> bool:
        want = []
        for W in self.Ws:
            want += [W.numel(), W.shape[0]]
        return tuple(want) == tuple(layout.numels)

    def cg_global_phase(self, layout, x, r, p, k, K, phase, world, php, cg_alpha, shift, keep_x=True):
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
        shapes = []
        for W in self.Ws:
            shapes += [W.shape, (W.shape[0],)]
        views = lambda flat: [flat[s: s + n].view(sh) for s, n, sh in zip(layout.starts, layout.numels, shapes)]
        dot = lambda a, b: float((a.double() * b.double()).sum())
        if phase == 0:      # BHG_CG_GLOBAL_CHAIN
            if k == 0:
                self._g = {"rr": dot(r, r)}
                self._g["pp"] = self._g["rr"]
            else:
                g = self._g
                beta = f32(g["rr_new"]) / f32(g["rr"])
                p.mul_(beta).add_(r)                    # cg.py:53 (the kernels form it lazily where they read it)
                b = float(beta)
                g["pp"] = g["rr_new"] + 2.0 * b * g["rp"] + b * b * g["pp_old"]
                g["rr"] = g["rr_new"]
            hv = self.hvp(views(p))
            self._hv = torch.zeros_like(p)
            for dst, h in zip(views(self._hv), hv):
                dst.copy_(h)
            php[0] = dot(p, self._hv)                   # this rank's p . H_data p
        elif phase == 1:    # BHG_CG_GLOBAL_UPDATE
            g = self._g
            den = float(cg_alpha) * (float(php[0]) / world + float(shift) * g["pp"])
            alpha = f32(g["rr"]) / f32(den)             # cg.py:47
            hp = self._hv + f32(shift) * p
            r.sub_(alpha * hp)                          # cg.py:50 on the local Hessian: the ranks' mean is the global r'
            x.add_(alpha * p)                           # cg.py:49
            if k == K - 1:
                x.mul_(-float(cg_alpha))                # cg.py:56 and the negation of cg.py:59/68
        else:               # BHG_CG_GLOBAL_DOTS, after the residual's exchange
            g = self._g
            g["rr_new"], g["rp"], g["pp_old"] = dot(r, r), dot(r, p), dot(p, p)

    def cg_global_finish(self, layout, K, cg_alpha, keep_x=True):
        return True

    # ---- global-batch CG, factor-exchange form: the math of csrc/mlp/fx.inc phase by phase, in ATen (tests: gloo, CPU).  Same slot
    # conventions as HipMLPState: every phase writes THIS rank's row of the buffer the caller gathers after it.
    def fx_supported(self, layout, world: int) -> bool:
        return self.fused_supported(layout) and len(self.Ws) >= 3

    def fx_buffers(self, world: int):
        held = self.__dict__.setdefault("_fx_bufs", {})
        if world not in held:
            L, B = len(self.Ws), self.B
            cf = sum(h.shape[1] for h in self.hs) * B + sum(d.shape[1] for d in self.deltas[1:]) * B
            sf = sum(W.shape[0] for W in self.Ws) * B + sum(W.shape[0] for W in self.Ws[:-1]) * B
            dev, dt = self.hs[0].device, self.hs[0].dtype
            held[world] = {"const": torch.zeros(world, cf, dtype=dt, device=dev), "slab": torch.zeros(world, sf, dtype=dt, device=dev),
                           "scal": torch.zeros(world, 3, dtype=torch.float64, device=dev), "xws": torch.zeros(1, dtype=torch.uint8, device=dev)}
        return held[world]

    def _fx_chain(self, st):
        """The R-chain on products-with-the-batch (Gf_p, Gb_p) and the narrow slices of the direction; returns Rz, [Rh_l], [Rd_l]."""
        L, Ws = len(self.Ws), self.Ws
        Rhs, Rh = [], None
        for l in range(L - 1):
            Ra = st["Gf_p"][l] + st["p_c"][l]
            if Rh is not None:
                Ra = Ra + Rh @ Ws[l].t()
            Rh = self.masks[l] * Ra
            Rhs.append(Rh)
        Rz = self.hs[L - 1] @ st["p_V"].t() + st["p_c"][L - 1] + Rh @ Ws[L - 1].t()
        Rd = self.sd[:, None] * (self.p * Rz - self.p * (self.p * Rz).sum(1, keepdim=True))
        Rds = [None] * L
        Rds[L - 1] = Rd
        for l in range(L - 1, 0, -1):
            Gb = self.deltas[l] @ st["p_V"] if l == L - 1 else st["Gb_p"][l]
            Rd = self.masks[l - 1] * (Gb + Rd @ Ws[l])
            Rds[l - 1] = Rd
        return Rz, Rhs, Rds

    def cg_fx_phase(self, rhs, k, K, phase, world, rank, cg_alpha, shift):
        L, B, G = len(self.Ws), self.B, world
        bufs = self.fx_buffers(world)
        dd = lambda a, b: float((a.double() * b.double()).sum())
        wide = range(L - 1)
        split_rows = lambda buf, widths: [list(torch.split(buf[g].view(B, -1), widths, 1)) for g in range(G)]
        if phase == 0:      # BEGIN
            bufs["const"][rank].copy_(torch.cat(self.hs + self.deltas[1:], 1).reshape(-1))
            self._fx = {}
            return
        st = self._fx
        if phase == 1:      # CHAIN
            if k == 0:
                widths = [h.shape[1] for h in self.hs] + [d.shape[1] for d in self.deltas[1:]]
                rows = split_rows(bufs["const"], widths)
                st["h_all"] = [torch.cat([rows[g][l] for g in range(G)], 0) for l in range(L)]
                st["d_all"] = [None] + [torch.cat([rows[g][L + l - 1] for g in range(G)], 0) for l in range(1, L)]
                vec = [t.detach() for t in rhs]
                st["r_c"] = [vec[2 * l + 1].clone() for l in range(L)]
                st["p_c"] = [t.clone() for t in st["r_c"]]
                st["r_V"] = vec[2 * (L - 1)].clone()
                st["p_V"] = st["r_V"].clone()
                st["Gf_r"] = [self.hs[l] @ vec[2 * l].t() for l in wide]
                st["Gb_r"] = [None] + [self.deltas[l] @ vec[2 * l] for l in range(1, L - 1)]
                st["Gf_p"] = [t.clone() for t in st["Gf_r"]]
                st["Gb_p"] = [None] + [t.clone() for t in st["Gb_r"][1:]]
                st["rr_w"] = sum(dd(vec[2 * l], vec[2 * l]) for l in wide)
                st["rp_w"] = st["pp_w"] = st["rr_w"]
                st["Rzx"] = torch.zeros(B, self.Ws[-1].shape[0], dtype=torch.float64, device=self.hs[0].device)
            else:
                self._fx_step(bufs, G, cg_alpha, shift, last=False)
            st["Rz"], st["Rhs"], st["Rds"] = self._fx_chain(st)
            bufs["slab"][rank].copy_(torch.cat(st["Rds"] + st["Rhs"], 1).reshape(-1))
            return
        if phase == 2:      # GRAM
            widths = [t.shape[1] for t in st["Rds"]] + [t.shape[1] for t in st["Rhs"]]
            rows = split_rows(bufs["slab"], widths)
            Rd_all = [torch.cat([rows[g][l] for g in range(G)], 0) for l in range(L)]
            Rh_all = [torch.cat([rows[g][L + l] for g in range(G)], 0) for l in range(L - 1)]
            h_all, d_all = st["h_all"], st["d_all"]
            Gf_raw, Gb_raw = [], [None]
            for l in wide:
                t = (self.hs[l] @ h_all[l].t()) @ Rd_all[l]
                if l >= 1:
                    t = t + (self.hs[l] @ Rh_all[l - 1].t()) @ d_all[l]
                Gf_raw.append(t / G)
            for l in range(1, L - 1):
                Gb_raw.append(((self.deltas[l] @ Rd_all[l].t()) @ h_all[l] + (self.deltas[l] @ d_all[l].t()) @ Rh_all[l - 1]) / G)
            st["Gf_raw"], st["Gb_raw"] = Gf_raw, Gb_raw
            st["raw_c"] = [Rd_all[l].sum(0) / G for l in range(L)]
            st["raw_V"] = (Rd_all[L - 1].t() @ h_all[L - 1] + d_all[L - 1].t() @ Rh_all[L - 2]) / G

            def share(Gf_u, Gb_u):
                return sum(dd(st["Rds"][l], Gf_u[l]) for l in wide) + sum(dd(st["Rhs"][l - 1], Gb_u[l]) for l in range(1, L - 1))

            bufs["scal"][rank].copy_(torch.tensor([share(st["Gf_r"], st["Gb_r"]), share(st["Gf_p"], st["Gb_p"]), share(Gf_raw, Gb_raw)],
                                                  dtype=torch.float64))
            return
        self._fx_step(bufs, G, cg_alpha, shift, last=True)   # END

    def _fx_step(self, bufs, G, cg_alpha, shift, last):
        """k_fx_step: alpha from the gathered shares and the narrow slices; recurrences; beta (cg.py:42-53 on batch-sized quantities)."""
        st, L = self._fx, len(self.Ws)
        dd = lambda a, b: float((a.double() * b.double()).sum())
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
        wide = range(L - 1)
        tot = bufs["scal"].sum(0)
        r_raw, p_raw, raw_raw = float(tot[0]) / G, float(tot[1]) / G, float(tot[2]) / G
        p_raw_n = sum(dd(st["p_c"][l], st["raw_c"][l]) for l in range(L)) + dd(st["p_V"], st["raw_V"])
        pp_n = sum(dd(t, t) for t in st["p_c"]) + dd(st["p_V"], st["p_V"])
        rr_n = sum(dd(t, t) for t in st["r_c"]) + dd(st["r_V"], st["r_V"])
        rr = st["rr_w"] + rr_n
        den = float(cg_alpha) * ((p_raw + p_raw_n) + float(shift) * (st["pp_w"] + pp_n))
        alpha = float(f32(rr) / f32(den))
        st["Rzx"] += alpha * st["Rz"].double()
        if last:
            return
        for l in range(L):
            st["r_c"][l] = st["r_c"][l] - alpha * (st["raw_c"][l] + shift * st["p_c"][l])
        st["r_V"] = st["r_V"] - alpha * (st["raw_V"] + shift * st["p_V"])
        for l in wide:
            st["Gf_r"][l] = st["Gf_r"][l] - alpha * (st["Gf_raw"][l] + shift * st["Gf_p"][l])
        for l in range(1, L - 1):
            st["Gb_r"][l] = st["Gb_r"][l] - alpha * (st["Gb_raw"][l] + shift * st["Gb_p"][l])
        rHp = r_raw + shift * st["rp_w"]
        pHp = p_raw + shift * st["pp_w"]
        HpHp = raw_raw + 2.0 * shift * p_raw + shift * shift * st["pp_w"]
        rr_w1 = st["rr_w"] - 2.0 * alpha * rHp + alpha * alpha * HpHp
        rp_w1 = st["rp_w"] - alpha * pHp
        rr_new = rr_w1 + sum(dd(t, t) for t in st["r_c"]) + dd(st["r_V"], st["r_V"])
        beta = float(f32(rr_new) / f32(rr))
        for l in range(L):
            st["p_c"][l] = st["r_c"][l] + beta * st["p_c"][l]
        st["p_V"] = st["r_V"] + beta * st["p_V"]
        for l in wide:
            st["Gf_p"][l] = st["Gf_r"][l] + beta * st["Gf_p"][l]
        for l in range(1, L - 1):
            st["Gb_p"][l] = st["Gb_r"][l] + beta * st["Gb_p"][l]
        st["pp_w"] = rr_w1 + 2.0 * beta * rp_w1 + beta * beta * st["pp_w"]
        st["rp_w"] = rr_w1 + beta * rp_w1
        st["rr_w"] = rr_w1

    def cg_fx_finish(self, layout, K, cg_alpha):
        self._fx_token = ("cg_fx", float(cg_alpha))
        return self._fx_token

    def neumann_fx_phase(self, rhs, k, K, phase, world, rank, alpha, shift):
        """neumann.py:59-66 on the global batch, factor-exchange form (bhg_mlp_neumann_fx_phase): no scalars; the direction lives in the
        p slots of the state; Rzx = sum_{k <= K} Rz(v_k)."""
        L = len(self.Ws)
        if phase in (0, 2) or (phase == 1 and k == 0):      # BEGIN, GRAM, and the first CHAIN are the CG form's
            return self.cg_fx_phase(rhs, k, K, phase, world, rank, alpha, shift)
        st = self._fx
        st["Rzx"] += st["Rz"].double()                      # Rz(v_{k-1}) (END: Rz(v_K))
        if phase == 3:
            return
        for l in range(L):
            st["p_c"][l] = st["p_c"][l] - alpha * (st["raw_c"][l] + shift * st["p_c"][l])
        st["p_V"] = st["p_V"] - alpha * (st["raw_V"] + shift * st["p_V"])
        for l in range(L - 1):
            st["Gf_p"][l] = st["Gf_p"][l] - alpha * (st["Gf_raw"][l] + shift * st["Gf_p"][l])
        for l in range(1, L - 1):
            st["Gb_p"][l] = st["Gb_p"][l] - alpha * (st["Gb_raw"][l] + shift * st["Gb_p"][l])
        st["Rz"], st["Rhs"], st["Rds"] = self._fx_chain(st)
        self.fx_buffers(world)["slab"][rank].copy_(torch.cat(st["Rds"] + st["Rhs"], 1).reshape(-1))

    def neumann_fx_finish(self, layout, K, alpha):
        self._fx_token = ("neumann_fx", float(alpha))
        return self._fx_token

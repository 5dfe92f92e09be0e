"""CPU stand-in for the finite-difference-HVP backend calls — TEST INFRASTRUCTURE.

``CpuCheckerBackend`` (tests/_cpu_checker_backend.py) plus the three calls ``FiniteDifferenceHVP`` and the solvers make on a gradient
pair: the perturbation from a snapshot and the cg / neumann steps, stated with separate fp32 ATen ops (the roundings the HIP kernels
promise: product rounded before the add, subtraction rounded before a true division) on top of the checker's one-table steps.
"""
import torch

from _cpu_checker_backend import CpuCheckerBackend, _f32


class CpuFdCheckerBackend(CpuCheckerBackend):
    name = "cpu-fd-checker"

    def __init__(self):
        super().__init__()
        self.calls = {"fd_perturb": 0, "cg_step_fd": 0, "neumann_step_fd": 0, "cg_step": 0, "neumann_step": 0}

    def fd_perturb(self, layout, weights, w0, direction, eps32, sign):
        self.calls["fd_perturb"] += 1
        a = torch.tensor(_f32(float(sign) * float(eps32)), dtype=torch.float32)
        for w, base, d in zip(weights, self._slices(layout, w0), self._prep(direction)):
            assert w.is_contiguous() and w.dtype == torch.float32
            w.copy_((base + a * d.reshape(-1)).view(w.shape))

    @staticmethod
    def _difference(grad_plus, grad_minus, two_eps):
        assert two_eps.dtype == torch.float32 and two_eps.dim() == 0
        return [(gp.to(torch.float32) - gm.to(torch.float32)) / two_eps for gp, gm in zip(grad_plus, grad_minus)]

    def cg_step(self, *a, **k):
        self.calls["cg_step"] += 1
        return super().cg_step(*a, **k)

    def neumann_step(self, *a, **k):
        self.calls["neumann_step"] += 1
        return super().neumann_step(*a, **k)

    def cg_step_fd(self, layout, grad_plus, grad_minus, two_eps, x, r, p, cg_alpha, it, out_scale=0.0, variant=None, hvp_shift=0.0):
        self.calls["cg_step_fd"] += 1
        self.calls["cg_step"] -= 1
        self.cg_step(layout, self._difference(grad_plus, grad_minus, two_eps), x, r, p, cg_alpha, it, out_scale=out_scale,
                     hvp_shift=hvp_shift)

    def neumann_step_fd(self, layout, grad_plus, grad_minus, two_eps, v, p, alpha, out_scale=0.0, hvp_shift=0.0):
        self.calls["neumann_step_fd"] += 1
        self.calls["neumann_step"] -= 1
        self.neumann_step(layout, self._difference(grad_plus, grad_minus, two_eps), v, p, alpha, out_scale=out_scale,
                          hvp_shift=hvp_shift)

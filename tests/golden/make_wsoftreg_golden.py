#!/usr/bin/env python
"""Generate tests/golden/wsoftreg.npz by running the REAL reference (leopard-ai/betty v0.2.1) on the seeded sample-weighted
softmax-regression instance of tests/wsoftreg_zoo.py: its own cg (K = 5 with cg_alpha = 1 and 0.1), neumann (K = 5, alpha = 0.25),
darts and sama.

Runs only in the build container (the reference does not exist on the GPU box).  The outputs are numbers, not code, in the layout
of make_softreg_golden.py: ``in/<name>`` the inputs and, per case,
    out/<case>/fp32/<i>       sync=False, fp32
    out/<case>/fp64/<i>       sync=False, everything in fp64
    out/<case>/w32/<i>        darts / sama: inner weights after the fp32 call

Usage:  PYTHONPATH=<reference checkout> python tests/golden/make_wsoftreg_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/

import wsoftreg_zoo  # noqa: E402

import betty.hypergradient  # noqa: E402,F401
from betty.configs import Config as RefConfig  # noqa: E402

REF = {name: getattr(sys.modules[f"betty.hypergradient.{name}"], name) for name in ("cg", "neumann", "darts", "sama")}


def run(case, inputs, dtype):
    curr, prev, vector = wsoftreg_zoo.build_case(case, inputs, RefConfig, device="cpu", dtype=dtype)
    out = REF[case.algo](vector, curr, prev, False)
    return [o.detach().clone() for o in out], [p.data.clone() for p in curr.trainable_parameters()]


def main():
    torch.set_num_threads(1)  # fixed reduction order for torch.dot / mm
    inputs = wsoftreg_zoo.seed_inputs()
    blob = {f"in/{k}": v for k, v in inputs.items()}
    for case in wsoftreg_zoo.CASES:
        r32, w32 = run(case, inputs, torch.float32)
        r64, _ = run(case, inputs, torch.float64)
        for i, t in enumerate(r32):
            blob[f"out/{case.name}/fp32/{i}"] = t.numpy()
        for i, t in enumerate(r64):
            blob[f"out/{case.name}/fp64/{i}"] = t.numpy()
        if case.algo in ("darts", "sama"):
            for i, t in enumerate(w32):
                blob[f"out/{case.name}/w32/{i}"] = t.numpy()
        a = torch.cat([t.reshape(-1).double() for t in r32])
        b = torch.cat([t.reshape(-1) for t in r64])
        print(f"{case.name:18s} |out|={b.norm().item():.4e}  fp32-vs-fp64 rel={((a - b).norm() / b.norm()).item():.2e} "
              f"max/max={((a - b).abs().max() / b.abs().max()).item():.2e}")
    path = os.path.join(HERE, "wsoftreg.npz")
    np.savez_compressed(path, **blob)
    print(f"wrote wsoftreg.npz ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()

"""Regenerates the CPU half of profiles/fd_hvp_accuracy.txt: the finite-difference cg / neumann solve restated in plain ATen ops
(tests/fd_hvp_ref.py) in fp32 and fp64 against the reference's fp64 goldens, per golden case and radius.  No GPU needed.
    python scripts/fd_hvp_accuracy.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import fd_hvp_ref  # noqa: E402
import zoo  # noqa: E402
from betty_amd import Config  # noqa: E402
from conftest import golden_list, load_golden, rel_err  # noqa: E402

torch.set_num_threads(1)
CASES = ["logreg_cg5", "logreg_cg3_a01", "logreg_neumann5", "reweight_cg20", "reweight_neumann10", "deep_cg6", "deep_neumann6",
         "imaml_cg10", "imaml_neumann6"]
print(f"{'case':<20} {'K':>3} {'radius':>8} {'fp32 restatement':>17} {'fp64 restatement':>17}")
for name in CASES:
    case = zoo.CASE_BY_NAME[name]
    inputs, outputs = load_golden(case.family)
    gold = golden_list(outputs, name, "fp64")
    K = case.cfg.get("cg_iterations", case.cfg.get("neumann_iterations"))
    radii = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4) if case.family == "imaml" else (1e-2, 1e-4, 1e-6) if case.family != "logreg" else (1e-2,)
    for R in radii:
        errs = []
        for dt in (torch.float32, torch.float64):
            c, p, v = zoo.build_case(case, inputs, Config, dtype=dt)
            errs.append(rel_err([t.numpy() for t in fd_hvp_ref.fd_solve(case.algo, v, c, p, R=R)], gold)[0])
        print(f"{name:<20} {K:>3} {R:>8.0e} {errs[0]:>17.3e} {errs[1]:>17.3e}")

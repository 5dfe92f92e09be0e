#!/usr/bin/env python
"""Generate tests/golden/cfg5_as_named.npz: outputs of the REAL reference (leopard-ai/betty at /root/reference) on BASELINE cfg 5
as named — its own DARTS supernet ``Network(16, 10, 8)`` (examples/neural_architecture_search/model_search.py:129-234; 1,930,618
parameters in 1,399 tensors) and ``Architecture(4)`` (model_search.py:302-317; 2 x 14 x 8 = 224), batch 64 x 3 x 32 x 32
(train_search.py:24), ``neumann`` K = 20, alpha = 0.01 (betty/hypergradient/neumann.py:8-66) — on the CPU, in fp32 (what the HIP
path is compared with) and in fp64 (the truth; |fp32 - fp64| is the reference's OWN rounding spread on this instance, stored as
``ref_spread`` and used by the GPU test as its noise floor).

The inputs are not stored: ``tests/zoo.cfg5_as_named_case`` regenerates them from the seed with the CPU generator; the file carries
fp64 checksums of every input tensor so the GPU test proves it rebuilt the very same problem.

Round 6 adds SHORT-HORIZON goldens of the same named network (K = 3): the fp32-vs-fp64 spread of the reference itself grows with the
number of Neumann terms (9.9e-4 at K = 20: below what fp32 resolves across devices) — at K = 3 it is far below north_star's rtol 1e-4,
so the GPU test can hold the product to 1e-4 against the reference's own CPU output there.

Usage:  python tests/golden/make_cfg5_golden.py            (build container only: needs /root/reference and the model files
                                                           staged by `make -C oracle ref`; 8 threads; K = 20: ~35 min)
        python tests/golden/make_cfg5_golden.py 3 [5 ...]  (adds / refreshes neumann<K> entries, keeps the others of the file as they are)
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zoo  # noqa: E402


def reference():
    sys.path.insert(0, "/root/reference")
    import betty.hypergradient  # noqa: F401
    from betty.configs import Config

    return sys.modules["betty.hypergradient.neumann"].neumann, Config


def run(dtype, K):
    fn, Config = reference()
    curr, prev, vector = zoo.cfg5_as_named_case(Config, torch.device("cpu"), dtype=dtype, K=K)
    out = fn(vector, curr, prev, False)
    return torch.cat([o.detach().reshape(-1) for o in out]), zoo.cfg5_checksums(curr, prev, vector) if dtype == torch.float32 else None


def main():
    assert zoo.nas_dir() is not None
    path = os.path.join(HERE, "cfg5_as_named.npz")
    Ks = [int(a) for a in sys.argv[1:]] or [zoo.CFG5_K]
    blob = {}
    if os.path.exists(path) and Ks != [zoo.CFG5_K]:
        old = np.load(path)
        blob = {k: old[k] for k in old.files}
    for K in Ks:
        t0 = time.time()
        r32, cs = run(torch.float32, K)
        t1 = time.time()
        r64, _ = run(torch.float64, K)
        spread = ((r32.double() - r64).norm() / r64.norm()).item()
        blob[f"neumann{K}/fp32"], blob[f"neumann{K}/fp64"] = r32.numpy(), r64.numpy()
        blob[f"neumann{K}/ref_spread"] = np.array(spread)
        assert "checksum" not in blob or np.array_equal(blob["checksum"], cs), "the seeded inputs changed under the committed golden"
        blob["checksum"] = cs
        print(f"cfg 5 as named, neumann K={K} alpha={zoo.CFG5_ALPHA}: |out| = {r64.norm().item():.6e}, {r32.numel()} floats; reference fp32-vs-fp64 "
              f"= {spread:.2e}   (fp32 {t1 - t0:.0f} s, fp64 {time.time() - t1:.0f} s, {torch.get_num_threads()} threads)", flush=True)
    np.savez_compressed(path, **blob)
    print(f"wrote cfg5_as_named.npz ({os.path.getsize(os.path.join(HERE, 'cfg5_as_named.npz')) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()

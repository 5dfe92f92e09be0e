#!/usr/bin/env python
"""Generate tests/golden/live_reference.npz: outputs of the REAL reference (leopard-ai/betty v0.2.1) on the problems the
oracle tests used to hand to a live checkout, so that those tests run from this repository alone:

    out/<case>/seed7/<i>        every reweight case of tests/zoo.py on zoo.seed_family_inputs("reweight", seed=7), sync=False, fp32
                                (tests/test_oracle.py::test_oracle_matches_live_reference_on_fresh_seed)
    out/fsdp_grad/ref/<i>       betty.hypergradient.utils.grad(..., is_fsdp=True) on test_oracle._fsdp_grad_case()
                                (tests/test_oracle.py::test_oracle_fsdp_grad_branch)
    out/fsdp_darts/rank<r>/<i>  darts under FSDP on two gloo ranks holding different shards of the direction, reweight_darts on the
                                committed reweight inputs (tests/test_distributed_cpu.py::test_darts_fsdp_branch_uses_the_norm_of_the_whole_sharded_vector)

Usage:  BETTY_SRC=<reference checkout> python tests/golden/make_live_golden.py
"""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
SRC = os.environ.get("BETTY_SRC")
OUT = os.path.join(HERE, "live_reference.npz")


def _paths():
    for p in (SRC, TESTS, os.path.join(os.path.dirname(TESTS), "oracle"), os.path.dirname(TESTS)):
        if p not in sys.path:
            sys.path.insert(0, p)


def _fsdp_darts_rank(rank, world, port, q):
    _paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zoo
        from conftest import load_golden

        import betty.hypergradient  # noqa: F401
        from betty.configs import Config as RefConfig

        case = zoo.CASE_BY_NAME["reweight_darts"]
        inputs, _ = load_golden(case.family)
        curr, prev, vector = zoo.build_case(case, inputs, RefConfig)
        curr._strategy = "fsdp"
        vector = [(rank + 1.0) * v for v in vector]   # as the test's worker: a different shard per rank
        out = sys.modules["betty.hypergradient.darts"].darts(vector, curr, prev, False)
        q.put((rank, [o.detach().numpy().copy() for o in out]))
    finally:
        dist.destroy_process_group()


def main():
    assert SRC and os.path.isdir(os.path.join(SRC, "betty")), "set BETTY_SRC to a checkout of the reference"
    _paths()
    torch.set_num_threads(1)   # fixed reduction order, as the tests run
    import zoo
    import test_oracle

    import betty.hypergradient  # noqa: F401
    from betty.configs import Config as RefConfig
    from betty.hypergradient.utils import grad as ref_grad

    blob = {}
    ref = {k: getattr(sys.modules[f"betty.hypergradient.{k}"], k) for k in ("cg", "neumann", "darts", "sama")}
    inputs = zoo.seed_family_inputs("reweight", seed=7)
    for case in [c for c in zoo.CASES if c.family == "reweight"]:
        curr, prev, vector = zoo.build_case(case, inputs, RefConfig)
        for i, t in enumerate(ref[case.algo](vector, curr, prev, False)):
            blob[f"out/{case.name}/seed7/{i}"] = t.detach().numpy()
    params, _, loss = test_oracle._fsdp_grad_case()
    for i, t in enumerate(ref_grad(loss, params, retain_graph=True, is_fsdp=True)):
        blob[f"out/fsdp_grad/ref/{i}"] = t.numpy()

    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fsdp_darts_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0, p.exitcode
    for r in range(world):
        for i, t in enumerate(results[r]):
            blob[f"out/fsdp_darts/rank{r}/{i}"] = t

    np.savez_compressed(OUT, **blob)
    print(f"wrote {os.path.relpath(OUT, os.path.dirname(TESTS))} ({len(blob)} arrays, {os.path.getsize(OUT) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()

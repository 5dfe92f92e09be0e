#!/usr/bin/env python
"""Do two builds of the library compute the same bits in the CG / Neumann recurrences at the sizes bench_kernels.py times?

    BHG_LIB=/path/to/libbhg.so python scripts/recurrence_bits.py dump --out DIR/parent.json [--extra 5000000]
    python scripts/recurrence_bits.py dump --out DIR/branch.json [--extra 5000000]        (one fresh process per library)
    python scripts/recurrence_bits.py compare DIR/parent.json DIR/branch.json

`dump` runs one seeded sequence per variant (stream, resident) and per shift (0, 0.3): cg_init, six cg_steps — the last with
out_scale != 0 — then neumann_init and three neumann_steps, the last with out_scale != 0.  The HVP producer is the diagonal
multiply of bench_kernels.py (element-wise torch ops: the same bits whatever the library).  It records the
sha256 of the raw bytes of x, r, p (v, p) and the published scalars as hex: the fixed-order fp64 dots make the kernels
deterministic, so two libraries that compute the same thing write the same file (the scalars after every CG step, the vectors
after the init, the first and the last step).  `compare` lists every record that differs
and exits 1 if there is one.  Sizes: default N = 10.03 M (register-only resident instance), --extra 5000000 (LDS-assisted),
--extra 12000000 (hybrid).
"""
import argparse
import hashlib
import json
import os
import sys

SIZES = [3072 * 2048, 2048, 2048 * 1536, 1536, 1536 * 384, 384, 384 * 10, 10]   # bench_kernels.py
SHIFTS = (0.0, 0.3)
CG_STEPS, NEUMANN_STEPS, OUT_SCALE = 6, 3, -0.5
# the steps after which the whole vectors are hashed (a device-to-host copy and a sha256 of 3 x 4 N bytes each); the scalars of
# EVERY CG step are recorded, and a step's r and p feed every later one, so the last step's hashes cover the ones in between
HASHED_CG, HASHED_NEUMANN = (0, CG_STEPS - 1), (0, NEUMANN_STEPS - 1)


def dump(args):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from betty_amd import _native
    from betty_amd.backend import get_backend

    dev = torch.device("cuda:0")
    be = get_backend()
    sizes = SIZES + ([args.extra] if args.extra > 0 else [])
    gen = torch.Generator().manual_seed(0)
    vec = [torch.randn(n, generator=gen).to(dev) for n in sizes]
    diag = [1.0 + 0.5 * torch.rand(n, generator=gen).to(dev) for n in sizes]
    hv = [torch.empty_like(v) for v in vec]
    lay = be.layout(vec)

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    def produce(views):   # H = diag: hv <- diag * direction
        torch._foreach_mul_(hv, 0.0)
        torch._foreach_addcmul_(hv, diag, views)

    records = {}
    for vname, variant in (("stream", _native.BHG_CG_STREAM), ("resident", _native.BHG_CG_RESIDENT)):
        for shift in SHIFTS:
            x, r, p = lay.state(3)
            be.cg_init(lay, vec, x, r, p)
            key = f"cg/{vname}/shift={shift}"
            records[f"{key}/init"] = dict(x=sha(x), r=sha(r), p=sha(p))
            pv = lay.views(p, vec)
            for k in range(CG_STEPS):
                produce(pv)
                be.cg_step(lay, hv, x, r, p, 1.0, k, OUT_SCALE if k == CG_STEPS - 1 else 0.0, variant=variant, hvp_shift=shift)
                records[f"{key}/step{k}"] = dict(scalars=[float(s).hex() for s in be.cg_scalars(lay).tolist()])
                if k in HASHED_CG:
                    records[f"{key}/step{k}"].update(x=sha(x), r=sha(r), p=sha(p))
            assert not be.cg_barrier_timed_out(lay), "grid barrier timed out"
    for shift in SHIFTS:   # (one Neumann kernel: no variants)
        v, p = lay.state(2)
        be.neumann_init(lay, vec, v, p)
        key = f"neumann/shift={shift}"
        records[f"{key}/init"] = dict(v=sha(v), p=sha(p))
        vv = lay.views(v, vec)
        for k in range(NEUMANN_STEPS):
            produce(vv)
            be.neumann_step(lay, hv, v, p, 0.01, OUT_SCALE if k == NEUMANN_STEPS - 1 else 0.0, hvp_shift=shift)
            if k in HASHED_NEUMANN:
                records[f"{key}/step{k}"] = dict(v=sha(v), p=sha(p))
    torch.cuda.synchronize()
    out = dict(N=sum(sizes), n_chunks=lay.n_chunks, lib=os.path.abspath(_native.LIB_PATH),
               lib_sha256=hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest(), records=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"recurrence_bits: N = {out['N']}, {len(records)} records from {out['lib']} ({out['lib_sha256'][:16]}) -> {args.out}")


def compare(args):
    a, b = (json.load(open(p)) for p in (args.a, args.b))
    assert a["N"] == b["N"] and a["n_chunks"] == b["n_chunks"], "the two dumps are of different problems"
    assert set(a["records"]) == set(b["records"]), "the two dumps hold different records"
    bad = [(k, f) for k in sorted(a["records"]) for f in a["records"][k] if a["records"][k][f] != b["records"][k].get(f)]
    n = sum(len(v) for v in a["records"].values())
    print(f"recurrence_bits: N = {a['N']}: {a['lib_sha256'][:16]} against {b['lib_sha256'][:16]}: "
          f"{n - len(bad)} of {n} fields in {len(a['records'])} records equal bit for bit")
    for k, f in bad:
        print(f"  DIFFERS: {k} {f}")
    sys.exit(1 if bad else 0)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("--out", required=True)
    d.add_argument("--extra", type=int, default=0)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    (dump if args.cmd == "dump" else compare)(args)


if __name__ == "__main__":
    main()

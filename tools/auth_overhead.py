"""What authentication costs a batched update step (one MI355X).

On one seeded synthetic stream (svoc.stream.SyntheticUpdateStream) two variants alternate in one process:

  (a) ``engine.step(inst, oracle_index, values)``            -- the unauthenticated tensor path (baseline)
  (b) ``ConsensusService.update_batch(inst, caller, values)`` -- one address-lookup launch, then the same step

at the c5 shape (1 M instances, 7 x 6, one update per instance, bf16) and the c3 shape (1024 instances,
256 x 4096, 64 updates per instance, fp32), and

  (c) the bare lookup (``Governance.resolve_oracles`` into a preallocated output) at those two shapes and at
      M = 4096 entries with K = 65,536 lookups, with its achieved bytes/s; the bytes come from the shapes:
      K x (40 + 32 x entries scanned), entries scanned = first match + 1 (the whole table for an unknown caller).

Times are device events around ``--iters`` calls after ``--warmup`` calls, ``--reps`` alternated repetitions;
the median and the min..max spread over the repetitions are reported.  No GPU: the script fails.

    python tools/auth_overhead.py --out auth_overhead.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from svoc.api import ConsensusService  # noqa: E402
from svoc.config import ConsensusConfig  # noqa: E402
from svoc.engine import ConsensusEngine  # noqa: E402
from svoc.governance import Governance  # noqa: E402
from svoc.stream import SyntheticUpdateStream  # noqa: E402

SHAPES = {
    "c5": dict(B=1 << 20, N=7, D=6, f=2, U=1, storage="bf16"),
    "c3": dict(B=1024, N=256, D=4096, f=32, U=64, storage="fp32"),
}


def random_table(B, M, dev, seed):
    """[B, M, 4] distinct-looking addresses (random 63-bit limbs)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(1, 1 << 62, (B, M, 4), generator=g, device=dev)


def build(shape, dev, seed=0) -> ConsensusService:
    cfg = ConsensusConfig(n_oracles=shape["N"], dimension=shape["D"], n_failing_oracles=shape["f"], constrained=True)
    svc = ConsensusService.__new__(ConsensusService)     # (no B-long host address lists)
    svc.cfg, svc.B = cfg, shape["B"]
    svc.engine = ConsensusEngine(cfg, shape["B"], device=dev, mode="fast", storage=shape["storage"])
    svc.gov = Governance(shape["B"], cfg.n_admins, shape["N"], dev, True, 2)
    svc.gov.oracle_addr.copy_(random_table(shape["B"], shape["N"], dev, 11 + seed))
    svc.engine.randomize(seed=seed)
    svc.engine.run_round()
    return svc


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters          # ms per call


def alternate(variants, warmup, iters, reps):
    """variants: {name: fn(i)} -> {name: {median_ms, min_ms, max_ms}}; the variants alternate rep by rep."""
    for fn in variants.values():
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def lookup_bytes(out, M):
    scanned = torch.where(out >= 0, out + 1, torch.full_like(out, M))
    return int(out.numel()) * 40 + 32 * int(scanned.sum())


def bare_lookup(gov, inst, caller, warmup, iters, reps):
    out = torch.empty(inst.numel(), dtype=torch.int64, device=inst.device)
    r = alternate({"lookup": lambda i: gov.resolve_oracles(inst, caller, out=out)}, warmup, iters, reps)["lookup"]
    nbytes = lookup_bytes(out, gov.N)
    r.update(K=int(inst.numel()), M=gov.N, B=gov.B, bytes=nbytes, found=int((out >= 0).sum()),
             gbytes_per_s=nbytes / (r["median_ms"] * 1e-3) / 1e9)
    return r


def run_shape(name, a, dev):
    shape = SHAPES[name]
    svc = build(shape, dev)
    e = svc.engine
    stream = SyntheticUpdateStream(shape["B"], shape["N"], shape["D"], shape["U"], shape["f"], pool=2, device=dev,
                                   seed=1, dtype=e.vdtype, failing=e.failing_mask)
    batches = [(inst, orc, vals, svc.gov.oracle_addr[inst, orc].contiguous()) for inst, orc, vals in stream.batches]
    # same stream, same state: the two variants must report the same statuses
    inst, orc, vals, caller = batches[0]
    same = bool(torch.equal(e.step(inst, orc, vals), svc.update_batch(inst, caller, vals)))
    step = alternate({
        "a_step_indices": lambda i: e.step(*batches[i % 2][:3]),
        "b_update_batch": lambda i: svc.update_batch(batches[i % 2][0], batches[i % 2][3], batches[i % 2][2]),
    }, a.warmup, a.iters, a.reps)
    ra, rb = step["a_step_indices"], step["b_update_batch"]
    rec = dict(shape=dict(shape, name=name), statuses_equal=same, step=step,
               overhead_ms=rb["median_ms"] - ra["median_ms"],
               overhead_pct=100.0 * (rb["median_ms"] / ra["median_ms"] - 1.0),
               lookup=bare_lookup(svc.gov, inst, caller, a.warmup, a.iters, a.reps))
    return rec


def run_wide(a, dev, B=256, M=4096, K=65536):
    gov = Governance(B, 0, M, dev, True, 2)
    gov.oracle_addr.copy_(random_table(B, M, dev, 5))
    g = torch.Generator(device=dev).manual_seed(6)
    inst = torch.randint(0, B, (K,), generator=g, device=dev)
    idx = torch.randint(0, M, (K,), generator=g, device=dev)
    caller = gov.oracle_addr[inst, idx].contiguous()
    return bare_lookup(gov, inst, caller, a.warmup, a.iters, a.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c5,c3,wide")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("auth_overhead: needs a GPU (a CPU timing says nothing about the MI355X)")
    dev = torch.device("cuda")
    rec = dict(kind="auth_overhead", device=torch.cuda.get_device_name(0), warmup=a.warmup, iters=a.iters,
               reps=a.reps, argv=sys.argv[1:])
    for name in a.shapes.split(","):
        rec[name] = run_wide(a, dev) if name == "wide" else run_shape(name, a, dev)
        print(json.dumps({name: rec[name]}), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

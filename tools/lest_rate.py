"""Rounds per second of the rank-weighted round beside the smooth-median fast fp32 round (one MI355X).

Two engines of one shape and seed, fp32 storage -- ``essence="rank_weighted"`` (consensus_fast_lest.hip: a full sort
of every column) and the default ``"smooth_median"`` (the window kernel: a selection network) -- alternate in one
process, each running ``run_round`` over every instance:

  c2   10,000 instances, 64 x 1024, f = 8, constrained
  c3    1,024 instances, 256 x 4096, f = 32, constrained

Times are device events around ``iters`` rounds (as many as fill ``--window`` seconds, found by a calibration call)
after ``--warmup`` rounds, ``--reps`` alternated repetitions; the median and the min..max spread over the
repetitions are reported as rounds/s (instances x rounds / time).  A round here is the prologue, the round kernel,
the restore hook and the epilogue of ``run_round`` -- the same launches for both engines but the round kernel.
No GPU: the script fails.

    python tools/lest_rate.py --out lest_rate.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from svoc.config import ConsensusConfig  # noqa: E402
from svoc.engine import ConsensusEngine  # noqa: E402

SHAPES = {
    "c2": dict(B=10000, N=64, D=1024, f=8),
    "c3": dict(B=1024, N=256, D=4096, f=32),
}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters          # ms per call


def engine(s, essence, sigma):
    cfg = ConsensusConfig(n_oracles=s["N"], dimension=s["D"], n_failing_oracles=s["f"], constrained=True,
                          essence=essence, rank_sigma=sigma)
    e = ConsensusEngine(cfg, s["B"], device="cuda", mode="fast", storage="fp32")
    e.randomize(seed=1)
    return e


def measure(name, s, args):
    engines = {"rank_weighted": engine(s, "rank_weighted", args.sigma), "smooth_median": engine(s, "smooth_median", 0.125)}
    fns = {k: (lambda e=e: e.run_round(only_touched=False)) for k, e in engines.items()}
    iters = {}
    for k, fn in fns.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(3, math.ceil(args.window * 1e3 / timed(fn, 3)))
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters[k]))
    out = dict(shape=name, **s, sigma=args.sigma)
    for k, e in engines.items():
        st = e.status.cpu()
        rate = sorted(s["B"] / (m * 1e-3) for m in ms[k])
        out[k] = dict(iters=iters[k], median_ms=statistics.median(ms[k]), rounds_per_s=statistics.median(rate),
                      rounds_per_s_min=rate[0], rounds_per_s_max=rate[-1], committed=int((st == 0).sum()))
    out["ratio"] = out["rank_weighted"]["rounds_per_s"] / out["smooth_median"]["rounds_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--sigma", type=float, default=0.125)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=2.0, help="seconds of work per timed repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lest_rate: no GPU (a rate measured anywhere else says nothing)")
    res = []
    for name in args.shapes.split(","):
        r = measure(name, SHAPES[name], args)
        print(json.dumps(r), flush=True)
        res.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

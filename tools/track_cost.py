"""What the per-oracle track record costs a step (one MI355X).

Two engines of one shape and seed, one built with ``track_oracles`` and one without, alternate in one process:

  c5        1 M instances, 7 x 6, bf16, one update per instance and step   (``engine.step``)
  c2_fp32   10,000 instances, 64 x 1024, fp32, one round per instance      (``run_round`` over every instance)
  exact     256 instances, 256 x 4096, exact wsad, one round per instance  (``run_round`` over every instance)

and, per shape, the bare ``track_update`` launch over every instance (all active, all OK) with its achieved
bytes/s.  The bytes come from the shapes: per instance active + status + a read-modify-write of rounds (13 B),
per oracle qr (4 B fast / 8 B exact) + reliable (1 B) + a read-modify-write of flagged, streak (int32) and score
(int64) (32 B) -- 41 B per oracle in exact mode, 37 B in fast mode, the "about 45 B" of the design.  ``--copy-rate``
runs the stream microbenchmark (tools/ubench/dma_rate, built from dma_rate.hip) and records its contiguous
16-KiB-tile rate next to them.

Times are device events around ``--iters`` calls after ``--warmup`` calls, ``--reps`` alternated repetitions;
the median and the min..max spread over the repetitions are reported.  No GPU: the script fails.

    python tools/track_cost.py --out track_cost.json
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from svoc.config import ConsensusConfig  # noqa: E402
from svoc.engine import ConsensusEngine  # noqa: E402
from svoc.stream import SyntheticUpdateStream  # noqa: E402

SHAPES = {
    "c5": dict(B=1 << 20, N=7, D=6, f=2, U=1, mode="fast", storage="bf16", iters=20),
    "c2_fp32": dict(B=10000, N=64, D=1024, f=8, U=0, mode="fast", storage="fp32", iters=10),
    "exact": dict(B=256, N=256, D=4096, f=32, U=0, mode="exact", storage="int32", iters=3),
}


def track_bytes(B: int, N: int, exact: bool) -> int:
    return B * (13 + N * ((8 if exact else 4) + 1 + 32))


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


def build(shape, dev, track):
    cfg = ConsensusConfig(n_oracles=shape["N"], dimension=shape["D"], n_failing_oracles=shape["f"], constrained=True,
                          track_oracles=track)
    e = ConsensusEngine(cfg, shape["B"], device=dev, mode=shape["mode"], storage=shape["storage"])
    e.randomize(seed=0)
    e.run_round()
    return e


def run_shape(name, a, dev):
    shape = SHAPES[name]
    iters = a.iters or shape["iters"]
    off, on = build(shape, dev, False), build(shape, dev, True)
    if shape["U"]:
        stream = SyntheticUpdateStream(shape["B"], shape["N"], shape["D"], shape["U"], shape["f"], pool=2, device=dev,
                                       seed=1, dtype=off.vdtype, failing=off.failing_mask)

        def step(e):
            return lambda i: e.step(*stream.batch(i))
    else:
        def step(e):
            def fn(i):
                e.touched.fill_(1)
                e.run_round()
            return fn
    r = alternate({"track_off": step(off), "track_on": step(on)}, a.warmup, iters, a.reps)
    # the record changes nothing else: same outputs, and one committed round counted per processed round
    same = all(bool(torch.equal(getattr(off, k), getattr(on, k))) for k in ("consensus", "rel", "reliable", "status"))
    rounds_ok = bool(torch.equal(on.track_record()["rounds"].long().sum(), on.metrics_fx[1]))
    on._active.fill_(1)
    on.status.zero_()
    bare = alternate({"track_update": lambda i: on._track_update()}, a.warmup, max(iters, 20), a.reps)["track_update"]
    nbytes = track_bytes(shape["B"], shape["N"], shape["mode"] == "exact")
    bare.update(bytes=nbytes, bytes_per_oracle=nbytes / (shape["B"] * shape["N"]),
                gbytes_per_s=nbytes / (bare["median_ms"] * 1e-3) / 1e9,
                gbytes_per_s_at_45B=45 * shape["B"] * shape["N"] / (bare["median_ms"] * 1e-3) / 1e9)
    return dict(shape=dict(shape, name=name, iters=iters), step=r, outputs_equal=same, rounds_match_metrics=rounds_ok,
                overhead_ms=r["track_on"]["median_ms"] - r["track_off"]["median_ms"],
                overhead_pct=100.0 * (r["track_on"]["median_ms"] / r["track_off"]["median_ms"] - 1.0),
                kernel=bare)


def copy_rate():
    """The stream microbenchmark's contiguous-tile rate without compute (variant 2, spin 0), TB/s."""
    exe = os.path.join(ROOT, "tools", "ubench", "dma_rate")
    if not os.path.exists(exe):
        return dict(error="tools/ubench/dma_rate not built (hipcc --offload-arch=gfx950 -O3 -Icsrc/include "
                          "tools/ubench/dma_rate.hip -o tools/ubench/dma_rate)")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300).stdout
    rates = {(int(m.group(1)), int(m.group(2))): float(m.group(3))
             for m in re.finditer(r"variant (\d) spin\s+(\d+): [\d.]+ us, ([\d.]+) TB/s", out)}
    if (2, 0) not in rates:
        return dict(error="no rate in the microbenchmark's output", output=out[-400:])
    return dict(contiguous_tbytes_per_s=rates[(2, 0)], row_pieces_tbytes_per_s=rates.get((0, 0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c5,c2_fp32,exact")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=0, help="calls per timed window (default: per shape)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copy-rate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_cost: needs a GPU (a CPU timing says nothing about the MI355X)")
    dev = torch.device("cuda")
    rec = dict(kind="track_cost", device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, argv=sys.argv[1:])
    if a.copy_rate:
        rec["copy_rate"] = copy_rate()
        print(json.dumps({"copy_rate": rec["copy_rate"]}), flush=True)
    for name in a.shapes.split(","):
        rec[name] = run_shape(name, a, dev)
        print(json.dumps({name: rec[name]}), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

"""Sequential model and case builder for the per-oracle track record (torch.ops.svoc.track_update; CPU only).

model_update is a plain loop over Python ints (exact mode) and NumPy float32 scalars (fast mode), written from
the definitions: for every instance with active != 0 and status == OK, rounds += 1; per oracle flagged += u and
streak = u ? streak + 1 : 0 with u = (reliable == 0); score += s_i with qmax = max_i qr_i and

    exact:  s_i = WSAD - trunc((qr_i * 1e6 + qmax // 2) / qmax);  qmax <= 0 -> WSAD, else qr_i < 0 -> 0
    fast:   s_i = int(clamp(f32(1 - f32(qr_i / qmax)), 0, 1) * 2^32);  qmax not positive finite -> 2^32, else a
            non-finite qr_i -> 0;  qmax ignores NaN (all NaN: -inf)

It shares no code with csrc/include/svoc/track.hpp.  matrix() lists the cases; make() builds one: three consecutive
calls (so streaks rise and reset and scores accumulate) and the model's record after each, built once, shared,
never modified.  Run lays a case out on a device, every track buffer carved out of a larger canary-filled
allocation; check() holds the assertions test_track_model.py (CPU op) and test_track_gpu.py (HIP kernel) share:
whole-tensor torch.equal, untouched rows and the canary borders included.  Nothing here imports GPU code.

Instance b of call c plays role (b + 5 * c) mod len(roles): with B >= len(roles) every call holds every role, a
smaller B walks through them over the calls.
"""
import collections
import functools

import numpy as np
import torch

OK, RELIABILITY_INTERVAL, ZERO_VARIANCE = 0, 6, 32
WSAD = 1_000_000
FAST_ONE = 1 << 32
CANARY32, CANARY64 = 0x5A3C69D2, 0x25C396E15A3C69D2
MARGIN = 64
CALLS = 3

NS = (1, 2, 7, 8, 9, 63, 64, 65, 130, 256)     # L = 1, 2, 8, 8, 16, 64, 64, 64 (+1), 64 x 3 (ragged), 64 x 4
BS = (1, 5, 37, 300)                           # partial group, partial wave, several waves, several workgroups
Case = collections.namedtuple("Case", "N B exact")

Q62 = (1 << 62) - 1
EXACT_ROLES = ("plain", "inactive", "zero_variance", "rel_interval", "all_reliable", "all_flagged", "ties",
               "max_last", "qmax0", "qmax1", "q62", "one_negative", "all_negative", "inactive_reverted", "wide")
FAST_ROLES = ("plain", "inactive", "zero_variance", "rel_interval", "all_reliable", "all_flagged", "ties",
              "max_last", "qmax0", "denormal", "inf", "one_nan", "all_nan", "inactive_reverted", "recip",
              "negative", "overflow")


def matrix():
    return [Case(N, B, exact) for exact in (True, False) for N in NS for B in BS]


def case_id(c):
    return f"{'exact' if c.exact else 'fast'}-N{c.N}-B{c.B}"


def lanes_of(N):
    L = 1
    while L < N and L < 64:
        L *= 2
    return L


# ----------------------------------------------------------------------------------------- the model

def score_exact(q, qmax):
    if qmax <= 0:
        return WSAD
    if q < 0:
        return 0
    return WSAD - (q * WSAD + qmax // 2) // qmax       # Python ints: unbounded, floor == trunc (all >= 0)


def score_fast(q, qmax):
    q, qmax = np.float32(q), np.float32(qmax)
    if not (qmax > 0 and np.isfinite(qmax)):
        return FAST_ONE
    if not np.isfinite(q):
        return 0
    with np.errstate(all="ignore"):
        s = np.float32(1) - np.float32(q / qmax)        # float32 / float32 and float32 - float32: one rounding each
    s = np.float32(min(max(s, np.float32(0)), np.float32(1)))
    return int(s * np.float32(4294967296.0))           # exact product, truncating conversion


def row_max(row, exact):
    if exact:
        return max(row)
    m = np.float32(-np.inf)
    for q in row:
        if not np.isnan(q) and q > m:
            m = q
    return m


def model_update(rec, active, status, reliable, qr, exact):
    """rec: dict(rounds [B], flagged / streak / score [B, N]) of nested Python lists, not modified; active,
    status: lists; reliable: [B][N] lists; qr: [B][N] Python ints or np.float32.  Returns the new record."""
    out = {k: ([r[:] for r in v] if k != "rounds" else v[:]) for k, v in rec.items()}
    for b in range(len(active)):
        if active[b] == 0 or status[b] != OK:
            continue
        out["rounds"][b] += 1
        qmax = row_max(qr[b], exact)
        for i, q in enumerate(qr[b]):
            u = 1 if reliable[b][i] == 0 else 0
            out["flagged"][b][i] += u
            out["streak"][b][i] = out["streak"][b][i] + 1 if u else 0
            out["score"][b][i] += score_exact(q, qmax) if exact else score_fast(q, qmax)
    return out


# ----------------------------------------------------------------------------------------- the cases

def recip_numerators(rng, qmax, n):
    """n float32 values q in (0, qmax) whose correctly rounded q / qmax differs from q * (1 / qmax) (what a
    reciprocal-and-multiply division computes), picked with NumPy's IEEE arithmetic."""
    out = []
    while len(out) < n:
        q = (qmax * rng.uniform(0.01, 0.99, 4096).astype(np.float32)).astype(np.float32)
        differ = (q / qmax) != (q * (np.float32(1) / qmax)).astype(np.float32)
        out += list(q[differ & (q < qmax) & (q > 0)])
    return out[:n]


def _exact_row(role, N, rng):
    big = lambda hi: [int(x) for x in rng.integers(0, hi, N, dtype=np.int64)]   # noqa: E731
    if role in ("plain", "inactive", "zero_variance", "rel_interval", "all_reliable", "all_flagged",
                "inactive_reverted"):
        return big(1 << 40)
    if role == "ties":
        row, m = big(1 << 30), (1 << 30) + 7
        for i in {0, N // 2, N - 1}:
            row[i] = m
        return row
    if role == "max_last":
        row = big(1 << 30)
        row[N - 1] = (1 << 31) + 3
        return row
    if role == "qmax0":
        return [0] * N
    if role == "qmax1":
        row = [int(x) for x in rng.integers(0, 2, N)]
        row[N - 1] = 1
        return row
    if role == "q62":       # qmax = 2^62 - 1 in the last cell, qmax - 1 beside it: the product needs 128 bits
        row = big(Q62)
        row[N - 1] = Q62
        if N > 1:
            row[0] = Q62 - 1
        if N > 2:
            row[1] = Q62
        return row
    if role == "one_negative":
        row = [x + 1 for x in big(1 << 40)]
        row[N // 2] = -5 if N > 1 else row[0]
        return row
    if role == "all_negative":
        return [-1 - x for x in big(1 << 40)]
    if role == "wide":
        return [int(x) for x in rng.integers(1 << 43, 1 << 62, N, dtype=np.int64)]
    raise ValueError(role)


def _fast_row(role, N, rng):
    f = np.float32
    rnd = lambda: [f(x) for x in rng.uniform(0.0, 0.3, N).astype(np.float32)]   # noqa: E731
    if role in ("plain", "inactive", "zero_variance", "rel_interval", "all_reliable", "all_flagged",
                "inactive_reverted"):
        return rnd()
    if role == "ties":
        row = rnd()
        for i in {0, N // 2, N - 1}:
            row[i] = f(0.5)
        return row
    if role == "max_last":
        row = rnd()
        row[N - 1] = f(0.75)
        return row
    if role == "qmax0":
        return [f(0)] * N
    if role == "denormal":  # qmax = 7 x the smallest denormal, the others smaller denormals and zero
        d = np.float32(1.401298464324817e-45)
        row = [f(d * f(int(k))) for k in rng.integers(0, 7, N)]
        row[N - 1] = f(d * f(7))
        return row
    if role == "inf":
        row = rnd()
        row[N - 1] = f(np.inf)
        return row
    if role == "one_nan":
        row = rnd()
        row[N - 1] = f(0.9)
        row[0] = f(np.nan) if N > 1 else row[0]
        return row
    if role == "all_nan":
        return [f(np.nan)] * N
    if role == "recip":     # one qmax per row (last cell), the picked numerators before it
        qm = f(rng.uniform(0.5, 4.0))
        if np.frexp(qm)[0] == 0.5:
            qm = f(qm * f(1.25))       # (a power of two has an exact reciprocal: nothing would differ)
        row = [f(x) for x in recip_numerators(rng, qm, 8)] * (N // 8 + 1)
        row = row[:N]
        row[N - 1] = qm
        return row
    if role == "negative":  # 1 - q / qmax above 1: clamped
        row = rnd()
        row[N - 1] = f(0.4)
        row[0] = f(-0.2) if N > 1 else row[0]
        return row
    if role == "overflow":  # q / qmax overflows to inf: 1 - inf = -inf, clamped to 0
        row = [f(0)] * N
        row[N - 1] = f(1e-40)
        if N > 1:
            row[0] = f(-3e38)
        if N > 2:
            row[1] = f(-np.inf)
        return row
    raise ValueError(role)


Built = collections.namedtuple("Built", "case calls start records roles")


@functools.lru_cache(maxsize=None)
def make(case):
    """calls: per call dict(active [B] u8, status [B] i32, reliable [B, N] u8, qr [B, N]) CPU tensors;
    start: the record before the first call (not all zero); records: the model's record after each call."""
    N, B, exact = case
    rng = np.random.default_rng(1000 * N + B + (500000 if exact else 0))
    roles = EXACT_ROLES if exact else FAST_ROLES
    rec = dict(rounds=[int(x) for x in rng.integers(0, 50, B)],
               flagged=[[int(x) for x in rng.integers(0, 9, N)] for _ in range(B)],
               streak=[[int(x) for x in rng.integers(0, 4, N)] for _ in range(B)],
               score=[[int(x) for x in rng.integers(0, 1 << 50, N)] for _ in range(B)])
    start, calls, records, used = rec, [], [], []
    for c in range(CALLS):
        active, status, reliable, qr, rl = [], [], [], [], []
        for b in range(B):
            role = roles[(b + 5 * c) % len(roles)]
            rl.append(role)
            active.append(0 if role in ("inactive", "inactive_reverted") else 1 + (b % 2) * 254)   # 1 or 255
            status.append({"zero_variance": ZERO_VARIANCE, "rel_interval": RELIABILITY_INTERVAL,
                           "inactive_reverted": ZERO_VARIANCE}.get(role, OK))
            if role == "all_reliable":
                reliable.append([1] * N)
            elif role == "all_flagged":
                reliable.append([0] * N)
            else:
                reliable.append([int(x) for x in rng.integers(0, 2, N)])
            qr.append(_exact_row(role, N, rng) if exact else _fast_row(role, N, rng))
        rec = model_update(rec, active, status, reliable, qr, exact)
        qt = (torch.tensor(qr, dtype=torch.int64) if exact
              else torch.from_numpy(np.array(qr, dtype=np.float32).reshape(B, N)))
        calls.append(dict(active=torch.tensor(active, dtype=torch.uint8), status=torch.tensor(status, dtype=torch.int32),
                          reliable=torch.tensor(reliable, dtype=torch.uint8), qr=qt))
        records.append(rec)
        used.append(rl)
    return Built(case, calls, start, records, used)


def record_tensors(rec):
    return dict(rounds=torch.tensor(rec["rounds"], dtype=torch.int32),
                flagged=torch.tensor(rec["flagged"], dtype=torch.int32),
                streak=torch.tensor(rec["streak"], dtype=torch.int32),
                score=torch.tensor(rec["score"], dtype=torch.int64))


# ----------------------------------------------------------------------------------------- a run on a device

def carve(t, device):
    """t on the device as a view inside a larger canary-filled buffer -> (view, whole)."""
    canary = CANARY64 if t.dtype == torch.int64 else CANARY32
    whole = torch.full((t.numel() + 2 * MARGIN,), canary, dtype=t.dtype, device=device)
    view = whole[MARGIN:MARGIN + t.numel()].view(t.shape)
    view.copy_(t)
    return view, whole


def borders_intact(whole):
    canary = CANARY64 if whole.dtype == torch.int64 else CANARY32
    edge = torch.cat([whole[:MARGIN], whole[-MARGIN:]]).cpu()
    return bool((edge == canary).all())


def check(case, device, op):
    """Run the case's three calls through ``op`` (torch.ops.svoc.track_update) on ``device``; after each call
    the whole record equals the model's, the inputs are unchanged and the canary borders intact."""
    built = make(case)
    bufs = {k: carve(v, device) for k, v in record_tensors(built.start).items()}
    for c, (call, want) in enumerate(zip(built.calls, built.records)):
        ins = {k: v.to(device) for k, v in call.items()}
        op(ins["active"], ins["status"], ins["reliable"], ins["qr"], bufs["rounds"][0], bufs["flagged"][0],
           bufs["streak"][0], bufs["score"][0])
        for k, w in record_tensors(want).items():
            got = bufs[k][0].cpu()
            assert torch.equal(got, w), (case_id(case), c, k, (got != w).nonzero()[:4].tolist())
            assert borders_intact(bufs[k][1]), (case_id(case), c, k, "canary")
        for k, v in call.items():   # bit patterns (NaN payloads included)
            idt = torch.int32 if v.dtype == torch.float32 else v.dtype
            assert torch.equal(ins[k].cpu().view(idt), v.view(idt)), (case_id(case), c, k, "input modified")

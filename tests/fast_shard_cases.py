"""D-sharded halves of the fast-mode kernels (MODE 1 / MODE 2) against fast_cases.ref64 (CPU only).

A D-sharded fast engine (svoc/parallel/dshard.py) runs every round as two launches per rank: mode 1 over the
rank's columns (c1 and the qr partials), an all-reduce of the partials, then mode 2 from the summed qr with the
global D as rel_dim.  Here one instance is cut into two unequal column shards; the expected outputs of a shard
are slices of ref64 over the WHOLE instance, the expected pass-1 partial is the fp64 sum over the shard's
columns.  Nothing is compared with a kernel's own whole round, and nothing here imports GPU code:
test_fast_shard_cases.py runs the matrix through the CPU twin, test_fast_shard_gpu.py through every HIP route.

Families: fast_cases' ("tie", False), ("tie", True) and ("signed", 8, -4) (data and reference from
fast_cases.make), and `cross` (cross_case below): constrained [0, 1] data whose f removed rows are decided by
shard B's columns alone, so that in shard A they sit wherever the builder puts them -- all below the pass-1
window, all above it, or as equal keys inside it.  cross_revert is the same data with an `active` mask and two
instances in which one shard-A column is constant over the reliable rows: shard A reverts with ZERO_VARIANCE
there, shard B (which cannot see that column) reports OK; dshard.py's shadow commit handles the rest.

Where the storage type has fewer than f values in (column's honest maximum, 1], the "above" columns of
cross_case repeat values instead of being distinct.  That is bf16 (2^-8 steps below 1.0) at 600 x 64, 1100 x 100
and 2100 x 64: the honest maxima lie near 0.7 - 0.8, which leaves 58 - 78, 50 - 73 and 50 - 59 values per column
for f = 64, 100 and 64.  Every other shape, and so every window-route shape (f <= 32), is asserted distinct.

cpu_launch and actual_route use the CPU op and the tensor-less route op of svoc.ops (as helpers.py does); no
device is touched.
"""
import collections
import functools
import math

import torch

import fast_cases as fc
from helpers import beta_oracles
from svoc import ops as svops
from svoc.status import Status

Case = collections.namedtuple("Case", "family N D f cut storage kind")
# family: fast_cases' tuples, ("cross",) or ("cross_revert",)
# kind: "win" (caller's workspace through both halves, hint 0), "two" (two-network kernel: mode 1 without a
#       workspace, mode 2 with a fresh one; hint -7 where the shape would take the window kernel), "mixed"
#       (mode 1 on the window kernel with a workspace, mode 2 under hint -7)

# (N, D, f, cut, lane groups, H)
WINDOW = [(20, 24, 6, 9, 1, 5),       # general merge; f + H > N/2: the zero-variance check compares every column
          (64, 40, 8, 13, 1, 5),      # s0 == 0 && f == 8: the 8-key merge
          (63, 24, 8, 9, 1, 5),       # the same merge, odd N
          (64, 40, 9, 13, 1, 17),
          (100, 24, 4, 9, 2, 5),
          (128, 40, 16, 13, 2, 17),
          (256, 24, 3, 9, 4, 5),
          (256, 40, 32, 13, 4, 17),   # at its bound (a = 16)
          (64, 40, 8, 1, 1, 5)]       # one-column shard: no second column in the pair
# (N, D, f, cut, lane groups): the two-network kernel by shape
TWO_ONLY = [(100, 24, 40, 9, 2), (300, 24, 30, 9, 8), (600, 16, 64, 5, 16), (1100, 16, 100, 5, 32),
            (2100, 16, 64, 5, 64)]
MIXED = (128, 40, 16, 13, 2, 17)
CANCEL_ROWS = [(64, 8), (128, 16), (256, 32)]   # (N, f) of the window rows rerun under SVOC_WIN_CANCEL
FAMILIES = [("tie", False), ("tie", True), ("signed", 8.0, -4.0), ("cross",)]
REVERT_ACTIVE = [1, 1, 0, 1, 1, 0]
KERNEL_WINDOW, KERNEL_TWO_NETWORK = 1, 2        # svoc.ops.KERNEL_*

SENT_F, SENT_U8, SENT_ST = -1234.5, 0xA5, -77   # prefill of every output buffer
FLOAT_OUTS = ("c1", "consensus", "skew", "kurt", "rel", "qr")
PASS2_OUTS = ("consensus", "skew", "kurt", "rel", "reliable")


def matrix():
    out = []
    for storage in ("bf16", "fp32"):
        for fam in FAMILIES:
            for N, D, f, cut, _, _ in WINDOW:
                out.append(Case(fam, N, D, f, cut, storage, "win"))
                out.append(Case(fam, N, D, f, cut, storage, "two"))
            for N, D, f, cut, _ in TWO_ONLY:
                out.append(Case(fam, N, D, f, cut, storage, "two"))
            out.append(Case(fam, *MIXED[:4], storage, "mixed"))
    return out


def revert_matrix():
    """cross_revert over every row whose batch holds the six instances of REVERT_ACTIVE."""
    return [c._replace(family=("cross_revert",)) for c in matrix()
            if c.family == ("cross",) and fc.batch_of(c.N) == len(REVERT_ACTIVE)]


def case_id(c):
    fam = c.family
    name = fam[0] if fam[0].startswith("cross") else fc.case_id((fam, c.N, c.D, c.f, c.storage)).split("-")[0]
    return "%s-%dx%dx%d-cut%d-%s-%s" % (name, c.N, c.D, c.f, c.cut, c.storage, c.kind)


def _table_row(c):
    for row in WINDOW + [MIXED]:
        if row[:3] == (c.N, c.D, c.f):
            return row[4], row[5]
    for row in TWO_ONLY:
        if row[:3] == (c.N, c.D, c.f):
            return row[4], 0
    raise KeyError(c)


def launch_args(c, mode):
    """(wave_hint, work) of one half: work is "caller" (the shard's persistent workspace), "fresh" (a new
    workspace per launch) or None."""
    if c.kind == "win":
        return 0, "caller"
    if c.kind == "mixed":
        return (0, "caller") if mode == 1 else (-7, "caller")
    hint = -7 if _table_row(c)[1] else 0
    return (hint, None) if mode == 1 else (hint, "fresh")


def expected_route(c, mode):
    """(kernel, lane_groups, win_h) the case states for one half.  win_h is the route's: the window half-width
    wherever the window kernel applies to the shape and workspace, also under hint -7."""
    lg, H = _table_row(c)
    if c.kind == "win" or (c.kind == "mixed" and mode == 1):
        return KERNEL_WINDOW, lg, H
    if c.kind == "mixed":
        return KERNEL_TWO_NETWORK, lg, H
    return KERNEL_TWO_NETWORK, lg, 0 if mode == 1 else H   # mode 1: no workspace, no window


def expected_coverage():
    """Every (kernel, lane_groups, win_h, constrained, storage, mode) the tables above state."""
    cov = set()
    for c in matrix():
        for mode in (1, 2):
            cov.add(expected_route(c, mode) + (c.family in (("tie", False), ("cross",)), c.storage, mode))
    return cov


# --------------------------------------------------------------------------------------------------- data
def _pick(cands, f):
    """f of the candidates, evenly spread and distinct where there are enough of them."""
    n = cands.numel()
    assert n >= 1
    if n >= f:
        return cands[torch.linspace(0, n - 1, f, dtype=torch.float64).round().long()], True
    return cands[torch.arange(f) % n], False


def cross_case(B, N, D, f, cut, seed, dtype):
    """Honest Beta(20, 20) rows rounded to the storage type; f random rows per instance that are all-0.0 /
    all-1.0 (alternating) in shard B's columns d >= cut and, in shard A's column d, by d % 4: 0 -- f values
    below every honest value; 1 -- f values above; 2 -- copies of the honest values at the f sorted ranks around
    the honest median; 3 -- left honest.  Returns fp64 data (every value representable in `dtype`), the
    expected mask and whether all the "below" / "above" values are distinct."""
    x, _ = beta_oracles(B, N, D, 0, seed=seed, dtype=torch.float64)
    x = x[:, :, :D].to(dtype).double()
    g = torch.Generator().manual_seed(seed + 1)
    up_step = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -12     # representable on (0.5, 1]
    below = torch.arange(1, 256, dtype=torch.float64) * 2.0 ** -10     # 8 significant bits, < 0.25
    above = torch.arange(1, int(0.5 / up_step) + 1, dtype=torch.float64) * up_step + 0.5
    expect = torch.ones(B, N, dtype=torch.bool)
    distinct = True
    R = N - f
    assert R >= f
    for b in range(B):
        rows = torch.randperm(N, generator=g)[:f]
        expect[b, rows] = False
        hon = x[b][expect[b]].clone()
        for d in range(D):
            if d >= cut:
                vals = (torch.arange(f) % 2).double()
            elif d % 4 == 0:
                vals, ok = _pick(below[below < hon[:, d].min()], f)
                distinct &= ok
            elif d % 4 == 1:
                assert hon[:, d].max() >= 0.5
                vals, ok = _pick(above[above > hon[:, d].max()], f)
                distinct &= ok
            elif d % 4 == 2:
                lo = R // 2 - f // 2
                vals = torch.sort(hon[:, d]).values[lo:lo + f]
            else:
                continue
            if d < cut:
                vals = vals[torch.randperm(f, generator=g)]
            x[b, rows, d] = vals
    assert torch.equal(x.to(dtype).double(), x) and x.min() >= 0 and x.max() <= 1
    return x, expect, distinct


def _revert_edit(x, expect, cut):
    """Instance 1: column cut - 1 constant (0.375) over the reliable rows; instance 3: column 0 alternating
    +0.0 / -0.0 over them.  Both in shard A."""
    x = x.clone()
    x[1, expect[1], cut - 1] = 0.375
    n = int(expect[3].sum())
    x[3, expect[3], 0] = torch.where(torch.arange(n) % 2 == 0, torch.tensor(0.0, dtype=torch.float64),
                                     torch.tensor(-0.0, dtype=torch.float64))
    return x


def _storage_parts(x, cut, dtype):
    """The two shards as the engine stores them: bf16 padded to ld % 8 == 0, fp32 contiguous (odd ld)."""
    parts = []
    for s in (x[:, :, :cut], x[:, :, cut:]):
        if dtype == torch.bfloat16:
            p = torch.zeros(s.shape[0], s.shape[1], (s.shape[2] + 7) // 8 * 8, dtype=dtype)
            p[:, :, :s.shape[2]] = s.to(dtype)
        else:
            p = s.to(dtype).contiguous()
            assert p.shape[2] % 2 == 1
        assert torch.equal(p[:, :, :s.shape[2]].double(), s.double())
        parts.append(p)
    return parts


def shard_status(x, ref, f, lo, hi):
    """The status a shard over columns [lo, hi) owes the reference, from the reference alone: the contract's
    checks in their order (reliability intervals, R >= 4, a reliable column of zero variance)."""
    B, N, D = x.shape
    st = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        r = ref["rel"][b]
        if not (0 <= float(r[0]) <= 1 and 0 <= float(r[1]) <= 1):
            st[b] = int(Status.RELIABILITY_INTERVAL)
        elif N - f < 4:
            st[b] = int(Status.TOO_FEW_RELIABLE)
        else:
            xr = x[b, ref["reliable"][b], lo:hi]
            if bool((xr == xr[:1]).all(0).any()):
                st[b] = int(Status.ZERO_VARIANCE)
    return st


@functools.lru_cache(maxsize=None)
def make(family, N, D, f, cut, storage):
    """Data, whole-instance reference and per-shard expectations of one (family, shape, cut, storage); built
    once, shared by every kind, never modified.  Asserts the conditions the reference itself must meet."""
    dtype, B = fc.DTYPES[storage], fc.batch_of(N)
    active, distinct = None, True
    if family[0].startswith("cross"):
        x, expect, distinct = cross_case(B, N, D, f, cut, N + D, dtype)
        constrained, scale, ms = True, 1.0, math.sqrt(D)
        if family[0] == "cross_revert":
            x = _revert_edit(x, expect, cut)
            active = torch.tensor(REVERT_ACTIVE, dtype=torch.uint8)
        ref = fc.ref64(x, f, constrained, ms)
        assert (fc.cut_gap(ref, f) > 0.5).all(), fc.cut_gap(ref, f)
    else:
        c0 = fc.make((family, N, D, f, storage))
        x, ref, expect = c0["x"][:, :, :D].double(), c0["ref"], c0["expect"]
        constrained, scale, ms = c0["constrained"], c0["scale"], c0["max_spread"]
        if family[0] == "tie":      # test_fast_signed_ties.test_preconditions, for these shapes
            tie, outside = fc.tie_group_gap(ref, f)
            assert (tie == 0).all() and (outside > 0.01).all(), (tie, outside)
        else:
            assert (fc.cut_gap(ref, f) >= 1e-4).all()
    if expect is not None:
        assert torch.equal(ref["reliable"], expect) and (~expect).sum(1).eq(f).all()
    bounds = [(0, cut), (cut, D)]
    assert cut != D - cut
    status = [shard_status(x, ref, f, lo, hi) for lo, hi in bounds]
    if family[0] == "cross_revert":
        zv = torch.zeros(B, dtype=torch.int32)
        zv[1] = zv[3] = int(Status.ZERO_VARIANCE)
        assert torch.equal(status[0], zv) and (status[1] == 0).all()
    else:
        assert (status[0] == 0).all() and (status[1] == 0).all(), status
    partial = [((x[:, :, lo:hi] - ref["c1"][:, None, lo:hi]) ** 2).sum(-1) for lo, hi in bounds]
    return dict(x=x, parts=_storage_parts(x, cut, dtype), bounds=bounds, ref=ref, expect=expect, active=active,
                status=status, partial=partial, constrained=constrained, max_spread=ms, scale=scale, N=N, D=D,
                f=f, cut=cut, storage=storage, distinct=distinct)


def make_case(c):
    return make(c.family, c.N, c.D, c.f, c.cut, c.storage)


# ------------------------------------------------------------------------------------------------ harness
_WORK = {"caller": svops.WORK_CALLER, "fresh": svops.WORK_CALLER, None: svops.WORK_NONE}   # what the binding sees


def actual_route(c, m, part, mode, f=None):
    """(kernel, lane_groups, win_h) route.hpp gives one half of case c on shard `part` (f: another n_failing)."""
    hint, work = launch_args(c, mode)
    lo, hi = m["bounds"][part]
    r = svops.fast_route(c.storage, c.N, hi - lo, m["parts"][part].shape[2], c.f if f is None else f,
                         m["constrained"], mode=mode, wave_hint=hint, work=_WORK[work])
    return r.kernel, r.lane_groups, r.win_h


def cpu_launch(part, x, a, mode, bufs):
    """sharded_round's launch over the CPU twin (one route: no hint, no workspace)."""
    o = bufs
    svops.ops().fast_round(x, a["active"], a["D"], a["f"], a["constrained"], a["max_spread"], o["c1"],
                           o["consensus"], o["skew"], o["kurt"], o["rel"], o["qr"], o["reliable"], o["status"],
                           0, mode, a["rel_dim"], False, None)
    return o


def fresh_outputs(B, N, D):
    o = {k: torch.full((B, D), SENT_F, dtype=torch.float32) for k in ("c1", "consensus", "skew", "kurt")}
    o["rel"] = torch.full((B, 2), SENT_F, dtype=torch.float32)
    o["qr"] = torch.full((B, N), SENT_F, dtype=torch.float32)
    o["reliable"] = torch.full((B, N), SENT_U8, dtype=torch.uint8)
    o["status"] = torch.full((B,), SENT_ST, dtype=torch.int32)
    return o


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _is_sentinel(o, k):
    return (o[k] == (SENT_U8 if k == "reliable" else SENT_ST if k == "status" else SENT_F)).all()


def _clone(o):
    return {k: v.clone() for k, v in o.items()}


def _args(m, i, f=None):
    lo, hi = m["bounds"][i]
    return dict(D=hi - lo, f=m["f"] if f is None else f, constrained=m["constrained"], max_spread=m["max_spread"],
                active=m["active"], rel_dim=m["D"])


def sharded_round(m, cut, launch, tag=""):
    """One round of make()'s case m as two column shards.  launch(part, x, args, mode, bufs) runs one half on
    shard `part` (0 / 1) over the storage tensor x with the output buffers prefilled from `bufs` (CPU tensors,
    left unmodified) and returns the buffers after the launch as CPU tensors.  Asserts every output of both
    modes against the reference, prints one FRAC line and returns (first, second, frac): the outputs after
    mode 1 and after mode 2 per shard, and the largest error of each toleranced output as a fraction of its
    bound."""
    assert cut == m["cut"]
    ref, x, N, D, B = m["ref"], m["x"], m["N"], m["D"], m["x"].shape[0]
    tol = fc.TOL[m["storage"]]
    act = torch.ones(B, dtype=torch.bool) if m["active"] is None else m["active"].bool()
    idle = ~act
    frac = collections.defaultdict(float)

    def worst(key, err, bound):
        # a non-finite error becomes inf and stays: Python's max() would drop a NaN, and NaN <= 1 must not pass
        v = float((err / bound).max())       # (torch's max propagates NaN)
        frac[key] = max(frac[key], v if math.isfinite(v) else math.inf)

    # ---- mode 1
    first = []
    for i, (lo, hi) in enumerate(m["bounds"]):
        o = launch(i, m["parts"][i], _args(m, i), 1, fresh_outputs(B, N, hi - lo))
        t = (tag, "mode 1", "shard %d" % i)
        assert (o["status"][act] == 0).all(), (t, o["status"])
        assert (o["c1"][act].double() == ref["c1"][act, lo:hi].float().double()).all(), (t, "c1")
        rtol, atol = tol["qr"]
        want = m["partial"][i][act]
        worst("qr1", (o["qr"][act].double() - want).abs(), atol * m["scale"] ** 2 + rtol * want.abs())
        for k in PASS2_OUTS:
            assert _is_sentinel(o, k), (t, k, "written by mode 1")
        for k in o:
            assert _is_sentinel({k: o[k][idle]}, k), (t, k, "inactive instance written")
        first.append(o)
    assert frac["qr1"] <= 1.0, (tag, "qr1", "error / bound = %.3g" % frac["qr1"])   # (pass 2 would run on it)
    # ---- the all-reduce: fp32 sum of the partials
    qr = torch.where(act[:, None], first[0]["qr"] + first[1]["qr"], torch.full_like(first[0]["qr"], SENT_F))
    # ---- mode 2
    second = []
    for i, (lo, hi) in enumerate(m["bounds"]):
        inp = _clone(first[i])
        inp["qr"] = qr.clone()
        o = launch(i, m["parts"][i], _args(m, i), 2, _clone(inp))
        t = (tag, "mode 2", "shard %d" % i)
        want_st = m["status"][i]
        assert torch.equal(o["status"][act], want_st[act]), (t, o["status"], want_st)
        assert _same_bits(o["c1"], inp["c1"]), (t, "c1 changed")
        assert _same_bits(o["qr"], inp["qr"]), (t, "qr != the summed input")
        for k in o:
            assert _is_sentinel({k: o[k][idle]}, k), (t, k, "inactive instance written")
        rev = act & (want_st != 0)
        for k in PASS2_OUTS:
            assert _is_sentinel({k: o[k][rev]}, k), (t, k, "written by a reverting shard")
        ok = act & (want_st == 0)
        mask = o["reliable"][ok].bool()
        assert (o["reliable"][ok] <= 1).all() and torch.equal(mask, ref["reliable"][ok]), (t, "reliable vs ref64")
        if m["expect"] is not None:
            assert torch.equal(mask, m["expect"][ok]), (t, "reliable vs constructed mask")
        cons, want = o["consensus"][ok].double(), ref["consensus"][ok, lo:hi]
        if m["constrained"]:
            assert (cons == want.float().double()).all(), (t, "consensus")
        else:   # fast_cases.check_round's forward bound of an fp32 sum of terms shifted by c1
            bound = N * 2.0 ** -24 * (x[ok][:, :, lo:hi] - ref["c1"][ok, None, lo:hi]).abs().mean(1) + fc._ulp32(want)
            worst("consensus", (cons - want).abs(), bound)
        for k in ("skew", "kurt"):
            rtol, atol = tol[k]
            want = ref[k][ok, lo:hi]
            worst(k, (o[k][ok].double() - want).abs(), atol + rtol * want.abs())
        rtol, atol = tol["rel"]      # the whole instance's: rel_dim is the global D
        worst("rel", (o["rel"][ok].double() - ref["rel"][ok]).abs(), atol + rtol * ref["rel"][ok].abs())
        second.append(o)
    print("FRAC %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(frac.items()))))
    for key, v in frac.items():
        assert v <= 1.0, (tag, key, "error / bound = %.3g" % v)
    return first, second, dict(frac)


def too_few_round(m, launch, second, tag=""):
    """Mode 2 again with f = N - 3 over the state `second` a sharded round left (its c1 and summed qr), every
    other output back at the sentinel: TOO_FEW_RELIABLE on every active instance, nothing written."""
    N, B = m["N"], m["x"].shape[0]
    act = torch.ones(B, dtype=torch.bool) if m["active"] is None else m["active"].bool()
    for i, (lo, hi) in enumerate(m["bounds"]):
        inp = fresh_outputs(B, N, hi - lo)
        inp["c1"], inp["qr"] = second[i]["c1"].clone(), second[i]["qr"].clone()
        o = launch(i, m["parts"][i], _args(m, i, f=N - 3), 2, _clone(inp))
        t = (tag, "f = N - 3", "shard %d" % i)
        assert (o["status"][act] == int(Status.TOO_FEW_RELIABLE)).all(), (t, o["status"])
        assert _is_sentinel({"status": o["status"][~act]}, "status"), t
        for k in inp:
            if k != "status":
                assert _same_bits(o[k], inp[k]), (t, k, "written by a reverting round")

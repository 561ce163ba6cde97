"""The fast-mode HIP kernels on rounds whose failing oracles send 2^20 .. 2^126, against ref64.

Every case of fast_extreme_cases.matrix() (data, reference and assertions pinned to the CPU twin by
test_fast_extreme.py) runs through each route, asserted with svoc.ops.fast_route before the launch: wave_hint 0
(the small kernel for N <= 16 bf16, the window kernels at lane groups 1 / 2 / 4 and both half-widths, the
two-network kernels for f > 32 or N > 256) and, for N <= 256, wave_hint -7 (the two-network kernels).  What the
kernels owe such a round: the all-rows-minus-removed power sums of the window kernels are inf - inf, NaN or fully
cancelled and every such column must reach the exact cleanup; rows whose qr is +inf tie with each other (and, in
the small kernel, with the padding rows) and are all removed; the first reliability is clamped to 0 and never
negative; a D-shard's qr partial is +inf before the all-reduce and mode 2 ranks on the sum.
"""
import math

import pytest
import torch

import fast_extreme_cases as xc
from helpers import fast_work, run_fast
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = xc.matrix()


def _cpu(o):
    return {k: v.cpu() for k, v in o.items()}


def expected_route(N, D, f, storage, hint):
    """(kernel, lane_groups, win_h) of a whole round, from the case tables."""
    shape = (N, D, f)
    if shape in xc.SMALL:
        assert storage == "bf16"
        return (svops.KERNEL_SMALL, 0, 0) if hint == 0 else (svops.KERNEL_TWO_NETWORK, 1, 5)
    if shape in xc.WINDOW:
        return (svops.KERNEL_WINDOW if hint == 0 else svops.KERNEL_TWO_NETWORK,) + xc.WINDOW_ROUTE[shape]
    return svops.KERNEL_TWO_NETWORK, xc.TWO_GROUPS[shape], 0      # (under either hint)


def _assert_route(N, D, f, storage, hint):
    r = svops.fast_route(storage, N, D, (D + 7) // 8 * 8, f, False, wave_hint=hint, work=svops.WORK_NONE)
    assert (r.kernel, r.lane_groups, r.win_h) == expected_route(N, D, f, storage, hint), (N, D, f, storage, hint, r)


def test_matrix_covers_every_route():
    got = set()
    for N, D, f, storage in CASES:
        for hint in (0, -7) if N <= 256 else (0,):
            got.add(expected_route(N, D, f, storage, hint) + (storage,))
    for storage in ("bf16", "fp32"):
        for lg, H in set(xc.WINDOW_ROUTE.values()):
            assert (svops.KERNEL_WINDOW, lg, H, storage) in got and (svops.KERNEL_TWO_NETWORK, lg, H, storage) in got
        for lg in xc.TWO_GROUPS.values():
            assert (svops.KERNEL_TWO_NETWORK, lg, 0, storage) in got
    assert set(xc.WINDOW_ROUTE.values()) == {(1, 5), (2, 5), (2, 17), (4, 17), (4, 5)}
    assert (svops.KERNEL_SMALL, 0, 0, "bf16") in got


@pytest.mark.parametrize("case", CASES, ids=xc.case_id)
def test_fast_kernels_vs_ref64(case):
    c = xc.make(case)
    N, D, f, storage = case
    hints = (0, -7) if N <= 256 else (0,)
    for h in hints:
        _assert_route(N, D, f, storage, h)
    xg = c["x"].to(DEV)
    outs = [run_fast(xg, D, f, False, c["max_spread"], wave_hint=h) for h in hints]
    torch.cuda.synchronize()
    outs = [_cpu(o) for o in outs]
    for h, o in zip(hints, outs):
        xc.check_extreme(o, c, "hint%d %s" % (h, xc.case_id(case)))
    if len(outs) == 2:      # the same order statistics in both kernels
        for k in ("c1", "reliable"):
            assert torch.equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------------------------------------ split modes
class GpuLaunch:
    """One half through the HIP op.  kind "win": hint 0 and one persistent workspace per shard through both
    halves; "two": the two-network kernel (hint -7 where the shape would take the window kernel), mode 1 without
    a workspace, mode 2 with a fresh one."""

    def __init__(self, kind, window_shape):
        self.kind, self.hint, self.work = kind, (-7 if kind == "two" and window_shape else 0), {}

    def work_kind(self, mode):
        return svops.WORK_CALLER if self.kind == "win" or mode == 2 else svops.WORK_NONE

    def __call__(self, part, x, a, mode, bufs):
        B = x.shape[0]
        if self.kind == "win":
            w = self.work.setdefault(part, fast_work(B, a["D"], DEV))
        else:
            w = fast_work(B, a["D"], DEV) if mode == 2 else None
        o = {k: v.to(DEV) for k, v in bufs.items()}
        svops.ops().fast_round(x.to(DEV), None, a["D"], a["f"], False, a["max_spread"], o["c1"], o["consensus"],
                               o["skew"], o["kurt"], o["rel"], o["qr"], o["reliable"], o["status"], self.hint, mode,
                               a["rel_dim"], False, w)
        torch.cuda.synchronize()
        return _cpu(o)


@pytest.mark.parametrize("case", xc.split_matrix(), ids=xc.case_id)
def test_split_modes_vs_ref64(case):
    N, D, f, cut, storage = case
    s = xc.make_split(case)
    window = (N, D, f) in xc.WINDOW
    res = {}
    for kind in ("win", "two") if window else ("two",):
        launch = GpuLaunch(kind, window)
        for mode in (1, 2):
            for part, (lo, hi) in enumerate(s["bounds"]):
                r = svops.fast_route(storage, N, hi - lo, s["parts"][part].shape[2], f, False, mode=mode,
                                     wave_hint=launch.hint, work=launch.work_kind(mode))
                if kind == "win":
                    want = (svops.KERNEL_WINDOW,) + xc.WINDOW_ROUTE[(N, D, f)]
                elif window:
                    want = (svops.KERNEL_TWO_NETWORK, xc.WINDOW_ROUTE[(N, D, f)][0],
                            0 if mode == 1 else xc.WINDOW_ROUTE[(N, D, f)][1])
                else:
                    want = (svops.KERNEL_TWO_NETWORK, xc.TWO_GROUPS[(N, D, f)], 0)
                assert (r.kernel, r.lane_groups, r.win_h) == want, (kind, mode, part, r)
        res[kind] = xc.shard_round(s, launch, "gpu split %s %s" % (kind, xc.case_id(case)))
    if len(res) == 2:
        for a, b in zip(res["win"], res["two"]):
            for k in ("c1", "reliable", "status"):
                assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ the clamp alone
@pytest.mark.parametrize("N,D,f,storage", xc.CLAMP_SHAPES)
def test_clamp_sweep(N, D, f, storage):
    """T0 (no overflow: sqrt(mean qr) >= max_spread all the same) and T2 (mean qr = inf) over max_spread values
    whose reciprocal product is below 1 (test_fast_extreme.test_clamp_constants): status 0, 0 <= rel1 <= atol --
    on the small kernel's reciprocal form (7 x 6, hint 0) and the division forms of the other kernels."""
    c = xc.make((N, D, f, storage))
    rows = xc.clamp_rows(c)
    xg = c["x"][rows].to(DEV)
    hints = (0, -7)
    for h in hints:
        _assert_route(N, D, f, storage, h)
    outs = [(ms, h, run_fast(xg, D, f, False, ms, wave_hint=h)) for ms in xc.clamp_spreads(D) for h in hints]
    torch.cuda.synchronize()
    assert math.isclose(xc.clamp_spreads(D)[0], c["max_spread"])
    for ms, h, o in outs:
        xc.check_clamp(_cpu(o), c, ms, "hint%d clamp" % h)

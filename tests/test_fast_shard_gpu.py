"""The fast-mode HIP kernels' D-sharded halves (MODE 1 / MODE 2) on two unequal column shards, against ref64.

Every case of fast_shard_cases.matrix() and revert_matrix() (data, reference and harness pinned to the CPU twin
by test_fast_shard_cases.py) runs through the route it states: the window kernels with the caller's workspace
through both halves, the two-network kernels (mode 1 without a workspace, mode 2 with a fresh one), and mode 1
on the window kernel followed by mode 2 on the two-network one.  The removed rows of a shard are chosen by the
other shard's columns, so the window kernels' pass-2 merge, sentinel shift, zero-variance pre-check and
all-minus-removed moments meet rows that are locally ordinary, far below, far above or equal to the median.
"""
import functools

import pytest
import torch

import fast_shard_cases as sc
from fast_shard_cases import actual_route, cpu_launch
from helpers import fast_work
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _groups(cases):
    """The cases of one (family, shape, cut, storage), every kind together: they share data and reference."""
    out = {}
    for c in cases:
        out.setdefault(c._replace(kind=""), []).append(c)
    return list(out.values())


GROUPS = _groups(sc.matrix() + sc.revert_matrix())
CANCEL = [c for c in sc.matrix() if c.family == ("cross",) and c.kind == "win" and (c.N, c.f) in sc.CANCEL_ROWS]


class GpuLaunch:
    """One half through the HIP op with the case's hint and workspace; the caller's workspace persists per shard."""

    def __init__(self, case):
        self.case, self.work = case, {}

    def __call__(self, part, x, a, mode, bufs):
        hint, work = sc.launch_args(self.case, mode)
        B = x.shape[0]
        if work == "caller":
            w = self.work.setdefault(part, fast_work(B, a["D"], DEV))
        else:
            w = fast_work(B, a["D"], DEV) if work == "fresh" else None
        o = {k: v.to(DEV) for k, v in bufs.items()}
        active = None if a["active"] is None else a["active"].to(DEV)
        svops.ops().fast_round(x.to(DEV), active, a["D"], a["f"], a["constrained"], a["max_spread"], o["c1"],
                               o["consensus"], o["skew"], o["kurt"], o["rel"], o["qr"], o["reliable"], o["status"],
                               hint, mode, a["rel_dim"], False, w)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def _cpu_statuses(key):
    m = sc.make_case(key)
    first, second, _ = sc.sharded_round(m, key.cut, cpu_launch, "cpu " + sc.case_id(key))
    return [o["status"] for o in first], [o["status"] for o in second]


def _run(case, m):
    tag = sc.case_id(case)
    for mode in (1, 2):
        for part in (0, 1):
            assert actual_route(case, m, part, mode) == sc.expected_route(case, mode), (tag, mode, part)
    launch = GpuLaunch(case)
    first, second, _ = sc.sharded_round(m, case.cut, launch, "gpu " + tag)
    cpu = _cpu_statuses(case._replace(kind=""))
    for got, want in zip((first, second), cpu):
        for i in (0, 1):
            assert torch.equal(got[i]["status"], want[i]), (tag, got[i]["status"], want[i])
    if case.family == ("cross",) and (case.kind == "two" or (case.kind == "win" and case.N == 20)):
        for part in (0, 1):
            kernel, _, H = actual_route(case, m, part, 2, f=case.N - 3)
            if case.kind == "win":
                assert (kernel, H) == (svops.KERNEL_WINDOW, 17)
            else:
                assert kernel == svops.KERNEL_TWO_NETWORK
        sc.too_few_round(m, launch, second, "gpu " + tag)
    return second


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: sc.case_id(g[0]._replace(kind="all")))
def test_hip_shards_vs_ref64(group):
    m = sc.make_case(group[0])
    res = {c.kind: _run(c, m) for c in group}
    if "win" in res:      # the same order statistics in both kernels, whichever ran which half
        for kind in set(res) - {"win"}:
            for a, b in zip(res["win"], res[kind]):
                for k in ("c1", "reliable", "status") + (("consensus",) if m["constrained"] else ()):
                    assert torch.equal(a[k], b[k]), (kind, k)


@pytest.mark.parametrize("cancel", ["1", "1e30"])
@pytest.mark.parametrize("case", CANCEL, ids=sc.case_id)
def test_hip_window_shards_cleanup_forced(case, cancel, monkeypatch):
    """The exact cleanup of the all-minus-removed moments on every column ("1") and on none ("1e30")."""
    monkeypatch.setenv("SVOC_WIN_CANCEL", cancel)
    _run(case, sc.make_case(case))

"""D-sharded fast rounds (mode 1 / mode 2 on two unequal column shards): model, harness and the CPU engine.

Runs without a GPU.  Building a case asserts the conditions its reference must meet (fast_shard_cases.make:
constructed mask, rank-cut gap, statuses); every case then runs through the CPU twin (reference_cpu.cpp
fast_round_one / fast_round_batch_cpu, modes 1 and 2) under the assertions test_fast_shard_gpu.py applies to
the HIP kernels.  The route each case states is asked of route.hpp through svoc.ops.fast_route, and the matrix
as a whole must cover every route the model's tables name.
"""
import pytest
import torch

import fast_shard_cases as sc
from fast_shard_cases import actual_route, cpu_launch
from svoc import ops as svops

CASES = sc.matrix()
REVERT = sc.revert_matrix()


def _one_per_data(cases):
    """The CPU engine has one route: one case per (family, shape, cut, storage)."""
    seen = {}
    for c in cases:
        seen.setdefault(c._replace(kind=""), c)
    return list(seen.values())


@pytest.mark.parametrize("case", _one_per_data(CASES + REVERT), ids=sc.case_id)
def test_cpu_engine_shards_vs_ref64(case):
    m = sc.make_case(case)
    _, second, _ = sc.sharded_round(m, case.cut, cpu_launch, "cpu " + sc.case_id(case))
    if case.family[0].startswith("cross"):
        sc.too_few_round(m, cpu_launch, second, "cpu " + sc.case_id(case))


@pytest.mark.parametrize("mode,key", [(1, "qr"), (2, "skew"), (2, "kurt"), (2, "rel"), (2, "consensus")])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_harness_rejects_a_non_finite_output(mode, key, value):
    """The toleranced outputs go through a running maximum: a NaN or inf in one element of one must fail."""
    fam = ("signed", 8.0, -4.0) if key == "consensus" else ("cross",)     # the mean is toleranced unconstrained
    m = sc.make(fam, 64, 40, 8, 13, "fp32")

    def launch(part, x, a, md, bufs):
        o = cpu_launch(part, x, a, md, bufs)
        if md == mode and part == 1:
            o[key][2, 1] = value
        return o

    with pytest.raises(AssertionError, match="'%s', 'error / bound = inf'" % ("qr1" if key == "qr" else key)):
        sc.sharded_round(m, 13, launch, "poisoned")


@pytest.mark.parametrize("case", CASES + REVERT, ids=sc.case_id)
def test_case_runs_on_the_route_it_states(case):
    m = sc.make_case(case)
    for mode in (1, 2):
        for part in (0, 1):
            assert actual_route(case, m, part, mode) == sc.expected_route(case, mode), (mode, part)


def test_matrix_covers_every_stated_route():
    want = sc.expected_coverage()
    got = set()
    for c in CASES:
        m = sc.make_case(c)
        for mode in (1, 2):
            for part in (0, 1):
                got.add(actual_route(c, m, part, mode) + (m["constrained"], c.storage, mode))
    assert got == want, (sorted(want - got), sorted(got - want))
    # the tables: both kernels, every lane-group width, both window half-widths, per storage and round form
    for storage in ("bf16", "fp32"):
        for cons in (True, False):
            for mode in (1, 2):
                for lg, H in ((1, 5), (1, 17), (2, 5), (2, 17), (4, 5), (4, 17)):
                    assert (svops.KERNEL_WINDOW, lg, H, cons, storage, mode) in got
                lgs = {k[1] for k in got if k[0] == svops.KERNEL_TWO_NETWORK and k[3:] == (cons, storage, mode)}
                assert lgs == {1, 2, 4, 8, 16, 32, 64}, (storage, cons, mode, lgs)
    assert (sc.KERNEL_WINDOW, sc.KERNEL_TWO_NETWORK) == (svops.KERNEL_WINDOW, svops.KERNEL_TWO_NETWORK)


def test_cross_family_puts_removed_rows_where_it_says():
    """The builder's own claims, on the data: the removed rows lie below / above every reliable value, or are
    equal keys around the reliable median, per shard-A column kind."""
    for c in CASES:
        if c.family != ("cross",) or c.kind == "mixed":
            continue
        m = sc.make_case(c)
        x, keep = m["x"], m["expect"]
        assert m["distinct"] or c.f > 32, sc.case_id(c)
        for b in range(x.shape[0]):
            hon, out = x[b, keep[b]], x[b, ~keep[b]]
            for d in range(c.cut):
                if d % 4 == 0:
                    assert out[:, d].max() < hon[:, d].min()
                elif d % 4 == 1:
                    assert out[:, d].min() > hon[:, d].max()
                elif d % 4 == 2:
                    s = torch.sort(hon[:, d]).values
                    lo = (c.N - c.f) // 2 - c.f // 2
                    assert torch.equal(torch.sort(out[:, d]).values, s[lo:lo + c.f])
                if d % 4 < 2 and m["distinct"]:
                    assert out[:, d].unique().numel() == c.f
            assert set(out[:, c.cut:].unique().tolist()) <= {0.0, 1.0}

"""Signed values and quadratic-risk ties at the rank cut: data, fp64 reference and the CPU fast engine.

Runs without a GPU.  For every case of fast_cases.matrix() it asserts the preconditions of the data
(conditions, not measurements: a shape or seed that misses one gets another seed, never a wider
threshold) and compares the CPU twin (reference_cpu.cpp fast_round_one: its own tie rule) with ref64
by the assertions the GPU test uses.  test_fast_signed_ties_gpu.py then runs the HIP kernels on the
same cached cases.
"""
import pytest
import torch

import fast_cases as fc
from helpers import run_fast

CASES = fc.matrix()


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_preconditions(case):
    c = fc.make(case)
    ref, f, N = c["ref"], c["f"], c["N"]
    assert c["x"].shape[0] == fc.batch_of(N) and torch.isfinite(c["x"]).all()
    if c["family"] == "signed":
        gap = fc.cut_gap(ref, f)
        assert (gap >= 1e-4).all(), gap
        x = c["x"][:, :, :c["D"]]
        assert (x < 0).any() and (x > 0).any()
        if c["structured"]:
            assert (ref["c1"][:, :2] == 0).all()
            assert (x[:, :, 1].double().var(dim=1) > 0).all() and (x[:, :, 2] <= -1).all()
            assert (x[:, :, 1] == 0).any() and torch.signbit(x[:, :, 1][x[:, :, 1] == 0]).any()
    else:
        t, k = fc.tie_params(N, f)
        assert 1 <= k < t
        tie, outside = fc.tie_group_gap(ref, f)
        assert (tie == 0).all(), tie                      # qr at sorted ranks R-1 and R exactly equal
        assert torch.equal(ref["reliable"], c["expect"])
        assert (outside > 0.01).all(), outside
        assert (~c["expect"]).sum(1).eq(f).all() and not c["expect"][:, 0].any() and c["expect"][:, N - 1].all()


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_cpu_engine_vs_ref64(case):
    c = fc.make(case)
    o = run_fast(c["x"], c["D"], c["f"], c["constrained"], c["max_spread"])
    fc.check_round(o, c, "cpu " + fc.case_id(case))


def test_ref64_agrees_with_fp32_reference():
    """ref64 against svoc.ops.torch_ref on ordinary [0, 1] data: the two references are written
    independently and must describe the same round."""
    from helpers import beta_oracles
    from svoc.ops import torch_ref
    for N, D, f, constrained in [(9, 5, 2, True), (64, 33, 8, False), (100, 24, 40, True)]:
        x, _ = beta_oracles(4, N, D, f, seed=N, dtype=torch.float32)
        a = fc.ref64(x[:, :, :D], f, constrained, 1.0)
        b = torch_ref.fast_round(x[:, :, :D], f, constrained, 1.0)
        assert torch.equal(a["reliable"], b["reliable"])
        assert torch.equal(a["c1"].float(), b["c1"])
        for k, tol in (("qr", 1e-5), ("consensus", 1e-6), ("rel", 1e-5), ("skew", 1e-3), ("kurt", 1e-3)):
            torch.testing.assert_close(a[k].float(), b[k], rtol=tol, atol=tol)

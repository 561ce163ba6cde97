"""consensus_fast_lest.hip where its centre leaves the honest rows: the cases and checks of lest_edge_cases, which
test_lest_edges.py pins to the CPU twin, on the kernel.  Family A runs the cancellation guard of pass 2 (the re-read
of a column about its reliable mean) in whole waves and in waves where only the odd columns take it; family B drives
it with first-read sums that are zero (2^40) or not finite (2^80); families C and D drive this kernel's instance of
the rank rule with qr = +inf and with ties at the cut.  The route is asserted before every launch."""
import pytest
import torch

import lest_cases as lc
import lest_edge_cases as ec
import test_lest_edges as cpu
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assert_route(shape):
    N, D, f = shape
    r = svops.lest_route("fp32", N, D, (D + 7) // 8 * 8, f, True)
    assert (r.supported, r.lane_groups) == (1, ec.LANES[N]), (shape, r)


def _run(c, work=None):
    _assert_route((c["N"], c["D"], c["f"]))
    return ec.run_case(svops.ops(), c, DEV, work)


@pytest.mark.parametrize("key", ec.a_matrix(), ids=ec.a_id)
def test_displaced_centre(key):
    c = ec.displaced_case(key)
    ec.check_displaced(_run(c), c)


@pytest.mark.parametrize("key", ec.a_matrix(), ids=ec.a_id)
def test_displaced_control(key):
    """The control instance of the batch (c1 central, no re-read): at M = 1024 it pins the fp64 accumulation of
    the kernel's weighted sum, see test_lest_edges.test_displaced_control."""
    c = ec.displaced_case(key)
    ec.check_control(_run(c), c)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lc.shape_id)
def test_displaced_centre_caller_workspace(shape):
    """The caller's workspace (the engine's) and the op's own temporary one give the same bits, re-reads included."""
    for M in ec.A_M:
        c = ec.displaced_case((shape, M, ("mean",), True))
        work = torch.empty(svops.fast_work_numel(lc.B, c["D"]), dtype=torch.int32, device=DEV)
        a, b = _run(c, work), _run(c)
        for k in a:
            assert torch.equal(a[k], b[k]), (c["tag"], k)
        ec.check_displaced(a, c)


@pytest.mark.parametrize("key", ec.b_matrix(), ids=ec.b_id)
def test_huge_displaced_centre(key):
    c = ec.huge_case(key)
    ec.check_huge(_run(c), c)


@pytest.mark.parametrize("key", ec.c_matrix(), ids=ec.c_id)
def test_extremes_behind_zero_weights(key):
    c = ec.zero_weight_case(key)
    ec.check_zero_weight(_run(c), c)


@pytest.mark.parametrize("key", ec.d_matrix(), ids=ec.d_id)
def test_rank_cut_ties(key):
    c = ec.tie_case(key)
    ec.check_tie(_run(c), c)


def test_engine_round_equals_op():
    cpu.engine_round_equals_op(DEV)

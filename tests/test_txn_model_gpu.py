"""The saved-batch transactional fast round on the GPU against the sequential model of txn_cases.py, driven at the
op level on one stream with a caller workspace, no engine: apply_updates(save), then fast_round(active, rst_*).
Where FastRoute.rollback is set the bf16 window kernel rolls the reverted instances back itself
(consensus_fast_win.hip, ``revert``: from the reliability check, the zero-variance pre-check, and the end of an
unconstrained pass 2); on every other route the binding launches the restore kernel after the round
(torch_ops.cpp) with its own instance index.  Every case's route is asserted before it runs; a failure names
the case, the instance's role, and the slot, oracle or column."""
import pytest
import torch

import txn_cases as tc
from helpers import fast_work
from svoc import ops as svops

pytestmark = pytest.mark.gpu

CASES = [pytest.param(c, id=tc.case_id(c)) for c in tc.CASES]


def _route(c):
    r = svops.fast_route(c.storage, c.N, c.D, tc.ld_of(c.D), c.f, c.constrained, c.legacy, 0, c.hint, svops.WORK_CALLER)
    assert (r.kernel, r.lane_groups, r.win_h, r.rollback) == (c.kernel, c.nseg, c.h, c.rollback), (tc.case_id(c), r)
    assert (tc.SMALL, tc.WINDOW, tc.TWO_NET) == (svops.KERNEL_SMALL, svops.KERNEL_WINDOW, svops.KERNEL_TWO_NETWORK)
    assert r.pruned == (c.storage == "fp32" and c.N == 256 and c.h == 17)
    return r


@pytest.mark.parametrize("c", CASES)
def test_saved_batch_round_matches_model(c):
    _route(c)
    m = tc.build(c)
    o = svops.ops()
    r = tc.Run(m, "cuda")
    r.apply(o)
    active = r.active()
    r.round(o, active, work=fast_work(tc.B, c.D, "cuda"), rollback=True)
    torch.cuda.synchronize()
    tag = "in-kernel roll-back" if c.rollback else "restore after the round"
    assert torch.equal(active.cpu().bool(), m["model"]["active"]), (tag, tc.case_id(c), "active")
    tc.check_saved(r, tag)
    tc.check(r, tag)

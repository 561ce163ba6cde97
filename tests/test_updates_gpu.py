"""The HIP update / restore / commit kernels (csrc/kernels/updates.hip) against the sequential model.

Every case of update_cases.matrix() runs through the kernels; the reference is the model of
update_cases.py (pinned to the CPU ops by test_updates_model.py), not the CPU twin and not another
GPU path.  All comparisons are on raw bytes: statuses, the whole state (padding columns and
untouched rows included), the canaries around every carved buffer, the winner workspace.

Save buffers: on the unique path every stored update holds its slot's pre-batch row and enabled
flag; on the last-writer path only each slot's winner does.  Every other update's flag is kNotSaved
and its saved row is still the canary.  The raw saved / saved_en of superseded updates are not
compared with the CPU twin: it saves update by update and legitimately holds rows there.
"""
import pytest
import torch

import update_cases as uc
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = uc.matrix()
SAVE_CASES = tuple(c for c in CASES if c.save)


@pytest.mark.parametrize("case", CASES, ids=uc.case_id)
def test_apply_vs_model(case):
    r = uc.Run(uc.make(case), DEV)
    r.apply(svops.ops())
    torch.cuda.synchronize()
    uc.check_apply(r, uc.case_id(case))


@pytest.mark.parametrize("inactive", [-1, uc.NOT_ACTIVE])
@pytest.mark.parametrize("case", SAVE_CASES + (uc.restore_grid_case(),), ids=uc.case_id)
def test_apply_then_restore_vs_model(case, inactive):
    """Round verdicts mixing OK, ZERO_VARIANCE (32) and RELIABILITY_INTERVAL (6) over an active mask
    with zeros.  The last case caps the restore grid at 64 workgroups: 257 threads take a second
    grid-stride iteration, a third of the instances reverted."""
    m = uc.make(case)
    r = uc.Run(m, DEV)
    r.apply(svops.ops())
    status, active = uc.round_status(m["B"], sparse=case.U > 10000)
    r.restore(svops.ops(), status, active, inactive)
    torch.cuda.synchronize()
    uc.check_restore(r, status, active, inactive, "%s inactive=%d" % (uc.case_id(case), inactive))
    assert torch.equal(r.touched.cpu(), m["model"]["touched"])
    assert bool(r.winner.eq(-1).all())


@pytest.mark.parametrize("cc", uc.COMMIT_CASES, ids=lambda cc: "%s-%dx%d-off%d" % (cc[0], cc[1], cc[2], cc[6]))
def test_commit_vs_model(cc):
    uc.run_commit(uc.make_commit(cc), svops.ops(), DEV, str(cc))

"""round_prologue / round_epilogue and the c1 commit kernels on the GPU (csrc/kernels/bookkeeping.hip) against
the plain models of tests/book_cases.py: the epilogue's grid-stride second pass above 512 x 256 instances, its
64-bit wave reduction, acc = None, bool and uint8 flags, views at an odd offset with canaries; commit_words and
commit_rows on their vector, word and grid-stride paths through exact_round."""
import pytest
import torch

import book_cases as bk
from svoc import ops as svops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", bk.book_matrix(), ids=bk.book_id)
def test_prologue_epilogue_gpu_match_model(case):
    bk.check_book(case, "cuda", svops.ops())


@pytest.mark.parametrize("case", bk.COMMIT_CASES, ids=bk.commit_id)
def test_commit_gpu_matches_golden_c1(case):
    """The golden c1 where the instance ran and the round succeeded, the sentinel everywhere else."""
    bk.check_commit(case, "cuda", svops.ops())


def test_bookkeeping_ops_refuse_a_host_tensor_among_device_tensors():
    """The dispatcher takes the HIP path when any argument is a device tensor; the bindings refuse the call before
    a kernel could read through a host pointer (every tensor position, the optional acc included)."""
    ops = svops.ops()
    B, N, d = 5, 7, "cuda"
    n_active = torch.full((B,), N, dtype=torch.int32, device=d)
    touched = torch.ones(B, dtype=torch.uint8, device=d)
    active = torch.zeros(B, dtype=torch.uint8, device=d)
    pro = [n_active, touched, active]
    for k in range(len(pro)):
        t = [(x.cpu() if i == k else x) for i, x in enumerate(pro)]
        with pytest.raises(RuntimeError):
            ops.round_prologue(t[0], t[1], N, True, t[2])
    status = torch.zeros(B, dtype=torch.int32, device=d)
    rel = torch.ones(B, 2, dtype=torch.float32, device=d)
    ca = torch.zeros(B, dtype=torch.uint8, device=d)
    acc = torch.zeros(4, dtype=torch.int64, device=d)
    active.fill_(1)
    epi = [active, status, rel, ca, touched, acc]
    for k in range(len(epi)):
        with pytest.raises(RuntimeError):
            ops.round_epilogue(*[(x.cpu() if i == k else x) for i, x in enumerate(epi)])
    torch.cuda.synchronize()
    assert not ca.any() and touched.all() and acc.tolist() == [0, 0, 0, 0]
    ops.round_epilogue(*epi)                               # the same call with every tensor on the device runs
    assert ca.all() and not touched.any() and acc.tolist() == [B << 32, B, B, 0]

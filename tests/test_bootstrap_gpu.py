"""torch.ops.svoc.bootstrap_oracles on the GPU (csrc/kernels/oracle_gen.hip) against the pure-Python model of
tests/boot_cases.py, fp32 bit patterns: the limits N = 256 (every lane of the workgroup), D = 16, C = 64, one
lane, 255 lanes, 300 workgroups, seeds with bit 63 set."""
import pytest
import torch

import boot_cases as bc
from svoc import ops as svops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_bootstrap_gpu_matches_model(case):
    bc.check(case, "cuda", svops.ops().bootstrap_oracles)


def test_bootstrap_refuses_a_host_tensor_among_device_tensors():
    """The dispatcher takes the HIP path when any argument is a device tensor; the binding refuses the call
    before a kernel could read through a host pointer."""
    op = svops.ops().bootstrap_oracles
    W, C, N, D = 2, 5, 7, 3
    a = [torch.full((W, C, 28), 0.5, device="cuda"), torch.tensor([3, 1, 2], dtype=torch.int32, device="cuda"),
         torch.full((W, N, D), bc.SENTINEL, device="cuda")]
    for k in range(len(a)):
        with pytest.raises(RuntimeError):
            op(*[(t.cpu() if i == k else t) for i, t in enumerate(a)], 2, 3, 1)
    torch.cuda.synchronize()
    assert (a[2] == bc.SENTINEL).all()

"""torch.ops.svoc.track_update on the GPU (csrc/kernels/track.hip) against the sequential model of
tests/track_cases.py: every lane-group size, ragged and multiple chunks, partial groups / waves and several
workgroups; three consecutive calls per case, whole-tensor equality, canary borders."""
import pytest
import torch

import track_cases as tc
from svoc import ops as svops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", tc.matrix(), ids=tc.case_id)
def test_track_update_gpu_matches_model(case):
    tc.check(case, "cuda", svops.ops().track_update)


def test_track_update_refuses_a_host_tensor_among_device_tensors():
    op = svops.ops().track_update
    B, N = 3, 7
    d = "cuda"
    a = [torch.ones(B, dtype=torch.uint8, device=d), torch.zeros(B, dtype=torch.int32, device=d),
         torch.ones(B, N, dtype=torch.uint8, device=d), torch.zeros(B, N, dtype=torch.float32, device=d),
         torch.zeros(B, dtype=torch.int32, device=d), torch.zeros(B, N, dtype=torch.int32, device=d),
         torch.zeros(B, N, dtype=torch.int32, device=d), torch.zeros(B, N, dtype=torch.int64, device=d)]
    for k in range(len(a)):
        with pytest.raises(RuntimeError):
            op(*[(t.cpu() if i == k else t) for i, t in enumerate(a)])
    torch.cuda.synchronize()
    assert a[4].tolist() == [0, 0, 0]

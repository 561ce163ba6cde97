"""torch.ops.svoc.track_update on the CPU (the scalar twin in csrc/include/svoc/track.hpp) against the sequential
model of tests/track_cases.py: three consecutive calls per case, whole-tensor equality, canary borders."""
import numpy as np
import pytest
import torch

import track_cases as tc
from svoc import ops as svops


@pytest.mark.parametrize("case", tc.matrix(), ids=tc.case_id)
def test_track_update_cpu_matches_model(case):
    tc.check(case, "cpu", svops.ops().track_update)


def test_case_matrix_reaches_what_it_claims():
    """The builder's own claims: every role in every call once B covers them, the lane-group sizes, a qmax in
    the last cell of the last chunk, the 128-bit product, and quotients an approximate reciprocal gets wrong."""
    assert {tc.lanes_of(N) for N in tc.NS} == {1, 2, 8, 16, 64}
    for exact, roles in ((True, tc.EXACT_ROLES), (False, tc.FAST_ROLES)):
        built = tc.make(tc.Case(130, 37, exact))
        for used in built.roles:
            assert set(used) == set(roles)
    b = tc.make(tc.Case(130, 37, True))
    rows = [b.calls[0]["qr"][i].tolist() for i, r in enumerate(b.roles[0]) if r == "q62"]
    assert rows and all(r[-1] == tc.Q62 and r[0] == tc.Q62 - 1 for r in rows)
    q, qmax = tc.Q62 - 1, tc.Q62
    wrapped = ((q * tc.WSAD + qmax // 2) + (1 << 63)) % (1 << 64) - (1 << 63)     # the product as an int64
    assert tc.WSAD - wrapped // qmax != tc.score_exact(q, qmax) == 0
    f = tc.make(tc.Case(130, 37, False))
    i = f.roles[0].index("recip")
    row = f.calls[0]["qr"][i].numpy()
    qm = row[-1]
    assert qm == row.max() and ((row[:-1] / qm) != (row[:-1] * (np.float32(1) / qm)).astype(np.float32)).all()
    i = f.roles[0].index("denormal")
    assert 0 < float(f.calls[0]["qr"][i].max()) < 1.2e-38


def test_track_update_refuses_bad_arguments():
    op = svops.ops().track_update
    B, N = 3, 7
    a = dict(active=torch.ones(B, dtype=torch.uint8), status=torch.zeros(B, dtype=torch.int32),
             reliable=torch.ones(B, N, dtype=torch.uint8), qr=torch.zeros(B, N, dtype=torch.int64),
             rounds=torch.zeros(B, dtype=torch.int32), flagged=torch.zeros(B, N, dtype=torch.int32),
             streak=torch.zeros(B, N, dtype=torch.int32), score=torch.zeros(B, N, dtype=torch.int64))
    order = ("active", "status", "reliable", "qr", "rounds", "flagged", "streak", "score")
    op(*[a[k] for k in order])
    assert a["rounds"].tolist() == [1, 1, 1]
    bad = [("status", a["status"].long()), ("qr", a["qr"].double()), ("score", a["score"].int()),
           ("flagged", torch.zeros(B, N + 1, dtype=torch.int32)), ("rounds", torch.zeros(B + 1, dtype=torch.int32)),
           ("streak", torch.zeros(N, B, dtype=torch.int32).t()), ("reliable", torch.ones(B, dtype=torch.uint8)),
           ("active", torch.ones(B + 2, dtype=torch.uint8))]
    for k, t in bad:
        with pytest.raises(RuntimeError):
            op(*[(t if n == k else a[n]) for n in order])
    assert a["rounds"].tolist() == [1, 1, 1]

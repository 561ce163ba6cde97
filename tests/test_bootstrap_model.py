"""torch.ops.svoc.bootstrap_oracles on the CPU (csrc/include/svoc/bootstrap.hpp through the loop in
csrc/bindings/generator_ops.cpp) against the pure-Python model of tests/boot_cases.py: the RNG stream, the slot
permutation and the distinct-comment draw, fp32 bit patterns, at the op's limits N = 256, D = 16, C = 64."""
import numpy as np
import pytest
import torch

import boot_cases as bc
from svoc import ops as svops


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_bootstrap_cpu_matches_model(case):
    bc.check(case, "cpu", svops.ops().bootstrap_oracles)


def test_model_primitives():
    """The model's own building blocks against published values and the case list's claims."""
    # splitmix64's reference stream from state 0 (Vigna, xoshiro.di.unimi.it/splitmix64.c)
    assert bc.splitmix64(0) == 0xE220A8397B1DCDAF
    assert bc.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    r = bc.Rng(123)
    u = [r.uniform() for _ in range(1000)]
    assert all(x.dtype == np.float32 and 0.0 <= x < 1.0 for x in u) and len(set(u)) > 990
    assert {c.N for c in bc.CASES} >= {1, 255, 256} and max(c.D for c in bc.CASES) == 16
    assert max(c.C for c in bc.CASES) == 64 and any(c.subset >= c.C == 64 for c in bc.CASES)
    assert any(c.f == c.N for c in bc.CASES) and any(c.seed < 0 for c in bc.CASES)
    # the keys tell windows and slots apart, and a seed above 2^63 is its int64 wrap
    assert len({bc.slot_key(7, w, j) for w in range(300) for j in range(256)}) == 300 * 256
    assert bc.CASES[3].seed & bc.M64 == (1 << 63) + 5
    # the data is what the issue asks for: scores in [0.01, 0.99], distinct labels inside [0, 28)
    for c in bc.CASES:
        b = bc.make(c)
        assert 0.01 <= float(b.scores.min()) and float(b.scores.max()) <= 0.99
        idx = b.label_idx.tolist()
        assert len(set(idx)) == c.D and all(0 <= i < 28 for i in idx)


def test_bootstrap_refuses_degenerate_arguments():
    """subset < 1 or C < 1 (a mean over no comment: NaN before the check existed), and n_failing outside [0, N]."""
    op = svops.ops().bootstrap_oracles
    W, C, N, D = 2, 5, 7, 3
    scores = torch.full((W, C, 28), 0.5)
    idx = torch.tensor([3, 1, 2], dtype=torch.int32)
    out = torch.full((W, N, D), bc.SENTINEL)
    for f, subset in ((2, 0), (2, -1), (2, -(1 << 40)), (-1, 3), (N + 1, 3), (1 << 40, 3)):
        with pytest.raises(RuntimeError):
            op(scores, idx, out, f, subset, 1)
    with pytest.raises(RuntimeError):
        op(scores[:, :0].contiguous(), idx, out, 2, 3, 1)           # C = 0
    assert (out == bc.SENTINEL).all()
    for f, subset in ((0, 1), (N, 1), (2, 1 << 40)):                # the edges of the accepted range
        out.fill_(bc.SENTINEL)
        op(scores, idx, out, f, subset, 1)
        assert torch.isfinite(out).all() and (out >= 0).all()
    # subset beyond C draws every comment once: equal scores -> every honest row is (1/3, 1/3, 1/3)
    assert int(((out - 1.0 / 3.0).abs() < 1e-6).all(-1).sum()) == W * (N - 2)


def test_pipeline_checks_label_indices(monkeypatch):
    """The op stays free of host synchronisation (c4 replays it in a captured graph), so the range of label_idx is
    checked where SentimentOraclePipeline builds it."""
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    from svoc.models import sentiment_oracle as so
    from svoc.models.encoder import EncoderConfig
    eng = ConsensusEngine(ConsensusConfig(n_oracles=7, dimension=6, n_failing_oracles=2), 2, device="cpu",
                          mode="fast", storage="fp32")
    so.SentimentOraclePipeline(eng, enc_cfg=EncoderConfig.tiny())
    monkeypatch.setattr(so, "ORACLE_LABEL_IDX", [20, 2, 3, 13, 19, 28])
    with pytest.raises(ValueError):
        so.SentimentOraclePipeline(eng, enc_cfg=EncoderConfig.tiny())

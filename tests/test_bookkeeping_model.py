"""round_prologue / round_epilogue on the CPU (csrc/include/svoc/bookkeeping.hpp through the loops in
csrc/bindings/bookkeeping_ops.cpp) against the torch model of tests/book_cases.py, and the commit cases'
expectation (the golden c1 where the instance ran and succeeded, the sentinel elsewhere) against the CPU
exact_round.  The same cases run on the GPU in tests/test_bookkeeping_gpu.py."""
import pytest
import torch

import book_cases as bk
from svoc import ops as svops
from svoc.status import Status


@pytest.mark.parametrize("case", bk.book_matrix(), ids=bk.book_id)
def test_prologue_epilogue_cpu_match_model(case):
    bk.check_book(case, "cpu", svops.ops())


@pytest.mark.parametrize("case", bk.COMMIT_CASES, ids=bk.commit_id)
def test_commit_expectation_matches_cpu_exact_round(case):
    bk.check_commit(case, "cpu", svops.ops())


def test_cases_reach_what_they_claim():
    """From the data and the model alone: every branch of the model is taken in both calls of every case large
    enough, one wave's rel2 sum passes 2^32, and the golden rounds hold one revert."""
    m = bk.book_matrix()
    assert {c.B for c in m} == set(bk.BOOK_BS) and max(bk.BOOK_BS) > 512 * 256
    for B in bk.BOOK_BS:
        sub = [c for c in m if c.B == B]
        assert {(c.fast, c.only_touched, c.as_bool) for c in sub if c.acc} == {(f, o, b) for f in (0, 1) for o in (0, 1)
                                                                               for b in (0, 1)}
        assert {c.sliced for c in sub} == {True, False} and {c.fast for c in sub if not c.acc} == {True, False}
    for c in m:
        if c.B < 255:
            continue
        _, rounds = bk.book_data(c)
        prev = torch.tensor(bk.ACC0)
        for r in rounds:
            act = r["want_active"].bool()
            ok = act & (r["status"] == 0)
            assert ok.any() and (act & ~ok).any() and (~act & (r["status"] == 0)).any()      # stale OK under inactive
            assert ((r["n_active"] == bk.N_ORACLES) & ~act).any() == c.only_touched
            assert ((r["want_acc"] - prev) > 0).all()
            # a wave = 64 consecutive instances: its rel2 sum needs more than 32 bits
            if c.fast:
                assert int(bk.model_rel2_fx(r["rel"][:64], ok[:64]).sum()) > 1 << 32
                assert not torch.isnan(r["rel"][ok, 1]).any() and torch.isnan(r["rel"][~ok, 1]).all()
                vals = set(r["rel"][ok, 1].tolist())
                assert {1.0, 1.0 - 2.0 ** -24, 0.0, -0.25, 1.5} <= vals
            else:
                assert {-5, 0, (1 << 40) + 3} <= set(r["rel"][ok, 1].tolist())
            if not c.as_bool:
                assert {0, 1, 2, 255} == set(r["touched"].tolist())
            prev = r["want_acc"]
    # rel2_fx at its edges
    rel = torch.tensor([[0, 1.0], [0, 1.0 - 2.0 ** -24], [0, 2.0 ** -33], [0, 2.0 ** -34], [0, -0.25], [0, 1.5]])
    assert bk.model_rel2_fx(rel, torch.ones(6, dtype=torch.bool)).tolist() == [1 << 32, (1 << 32) - 256, 1, 0, 0, 1 << 32]
    for D in sorted({c.D for c in bk.COMMIT_CASES}):
        g = bk.golden_rounds(D)
        want = [int(Status.OK)] * bk.N_GOLDEN
        want[bk.REVERT_AT] = int(Status.DIV_BY_ZERO)
        assert g.status == want
        assert len({tuple(r) for r in g.c1.tolist()}) == bk.N_GOLDEN          # distinct rounds (the revert: zeros)
    words = {c.D * 2 for c in bk.COMMIT_CASES}
    assert min(words) < 256 and 256 in words and any(w > 256 and w % 4 for w in words)
    assert any(c.B * 2 * c.D > 8192 * 256 and 2 * c.D < 256 for c in bk.COMMIT_CASES)
    assert any(c.B > 8192 and 2 * c.D >= 256 for c in bk.COMMIT_CASES)

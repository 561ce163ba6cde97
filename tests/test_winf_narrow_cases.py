"""The narrow-window model and cases of tests/winf_narrow_cases.py, checked on the CPU: the model is sound (a trusted
column's pass-2 pair lies inside the stored range) on the committed cases and on random removed sets, it reduces to the
N = 256, f = 32 model of tests/test_winf_narrow_gpu.py, and the cases bite -- by the fp64 reference alone, both halves
of the trust predicate are crossed wherever they can be."""
import numpy as np
import pytest
import torch

import route_cases
import winf_narrow_cases as wc
from svoc import ops as svops

H = wc.H


def test_stored_half_width():
    assert 1 <= wc.hs() < H and wc.kn() >= 1


def test_shapes_reach_the_narrow_round():
    """Every shape of the matrix is one a hinted fp32 round runs narrow, by the restatement here and by the op's own
    route (window kernel, H = 17, four lane groups); the H = 17 edges come from fast_win_h."""
    for N, f in wc.SHAPES:
        for D in wc.DS + tuple(d for d in wc.D_EDGES if d <= wc.MAX_D):
            assert wc.can_be_narrow("fp32", N, D, f, True, 0, True), (N, f, D)
            ld = (D + 7) // 8 * 8
            r = svops.fast_route("fp32", N, D, ld, f, True)
            assert (r.kernel, r.win_h, r.lane_groups) == (svops.KERNEL_WINDOW, H, 4), (N, f, D, r)
        assert svops.fast_win_h(N, f) == route_cases.fast_win_h(N, f) == H
    for N, f in wc.SHAPES_EDGE:
        assert route_cases.fast_win_h(N, f - 1) != H and svops.fast_win_h(N, f - 1) != H
    assert not wc.can_be_narrow("fp32", 256, 4104, 32, True, 0, True)
    assert not wc.can_be_narrow("fp32", 128, 64, 32, True, 0, True)
    assert not wc.can_be_narrow("fp32", 257, 64, 32, True, 0, True)
    assert not wc.can_be_narrow("fp32", 256, 64, 8, True, 0, True)       # H = 5
    assert not wc.can_be_narrow("bf16", 256, 64, 32, True, 0, True)
    assert not wc.can_be_narrow("fp32", 256, 64, 32, False, 0, True)
    assert not wc.can_be_narrow("fp32", 256, 64, 32, True, 1, True)
    assert not wc.can_be_narrow("fp32", 256, 64, 32, True, 0, False)


def test_sides_at_256():
    """At N = 256: f <= 20 can never fall back, f = 21 on the low side only, f >= 22 on both -- read off the model,
    and (256, 31) has no low sentinel yet is not the sentinel-free shape."""
    for f in range(wc.smallest_f_with_h17(256), 33):
        lo, hi = wc.sides(256, f)
        assert (lo, hi) == (f >= 21, f >= 22), (f, lo, hi)
    assert wc.low_sentinels(256, 31) == 0 and wc.low_sentinels(256, 32) == 0
    for N, f in wc.SHAPES:
        if f >= 22:
            assert wc.sides(N, f) == (True, True), (N, f)


def _extreme_column(N, f, value):
    """Honest rows at 0.5, the f removed rows at `value`: the column that fails a side if any can."""
    x = np.full((N, 1), 0.5, dtype=np.float32)
    removed = np.zeros(N, dtype=bool)
    removed[:f] = True
    x[:f] = value
    return bool(wc.untrusted_cols(wc.keys_of(x), removed, N, f)[0])


def test_sides_agree_with_the_model_on_extreme_columns():
    """sides() is a formula; the predicate itself, on all-high / all-low removed keys, says the same for every f with
    H = 17 at every N of the matrix."""
    for N in sorted({n for n, _ in wc.SHAPES}):
        for f in range(0, 33):
            if route_cases.fast_win_h(N, f) != H:
                continue
            lo, hi = wc.sides(N, f)
            assert _extreme_column(N, f, 1.0) == lo, (N, f)
            assert _extreme_column(N, f, 0.0) == hi, (N, f)


def test_reduces_to_the_anchor_model():
    """At N = 256, f = 32 the general model is the `_untrusted` of tests/test_winf_narrow_gpu.py."""
    for fam in wc.FAMILIES:
        for D in wc.DS:
            c = wc.make((fam, 256, 32, D))
            old = wc.untrusted_256x32(c["x"], c["removed"], D, c["ok"])
            assert np.array_equal(old, c["fallback"]), (fam, D)


@pytest.mark.parametrize("case", wc.matrix(), ids=wc.case_id)
def test_case_is_sound_and_bites(case):
    c = wc.make(case)
    fam, N, f, D = case
    x, removed, fb, ok = c["x"], c["removed"], c["fallback"], c["ok"]
    lo_can, hi_can = wc.sides(N, f)
    print(f"{wc.case_id(case)}: sh {wc.low_sentinels(N, f)} sides {(lo_can, hi_can)} committed {ok} "
          f"model fallback columns {fb.sum(1).tolist()}")
    # the removed rows are the planted failing rows
    for b in ok:
        assert torch.equal(removed[b], c["is_fail"][b]), b
    # soundness: trusted => the fp64 pair of the kept rows lies inside the stored range
    keys = wc.keys_of(x[:, :, :D].numpy())
    for b in ok:
        inside = wc.pair_inside(keys[b], removed[b].numpy(), N, f)
        assert inside[~fb[b]].all(), (b, np.nonzero(~inside & ~fb[b]))
    # the cases bite
    if f <= 20:
        assert fb.sum() == 0
    if fam in ("low", "high"):
        # all removed keys low: the pair moves up and the upper half fails, where it can
        expect = hi_can if fam == "low" else lo_can
        assert (fb[ok] == expect).all()
        if f >= 22:
            assert fb.all()
    if fam == "sym":
        assert ok == list(range(c["B"]))
        assert (fb.sum(1) <= D // 64).all()
    if fam == "split":
        k_of = np.full((c["B"], D), -1)
        for (b, col), k in c["planted"].items():
            k_of[b, col] = k
        for b in ok:
            ks_bad = sorted(k_of[b][(k_of[b] >= 0) & fb[b]].tolist())
            ks_ok = sorted(k_of[b][(k_of[b] >= 0) & ~fb[b]].tolist())
            # trusted planted columns, on each side that has untrusted ones
            assert ks_ok and (not lo_can or ks_ok[0] < f / 2) and (not hi_can or ks_ok[-1] > f / 2), (b, ks_ok)
            # few low keys: the lower half fails; few high keys: the upper half
            assert any(k < f / 2 for k in ks_bad) == lo_can, (b, ks_bad)
            assert any(k > f / 2 for k in ks_bad) == hi_can, (b, ks_bad)
            # ... and the boundary is a threshold in k on each side
            if lo_can:
                t = max(k for k in ks_bad if k < f / 2)
                assert all((k <= t) == (k in ks_bad) for k in range(0, f // 2 + 1)), (b, ks_bad)
            if hi_can:
                t = min(k for k in ks_bad if k > f / 2)
                assert all((k >= t) == (k in ks_bad) for k in range((f + 1) // 2, f + 1)), (b, ks_bad)
    if fam == "ties":
        assert ok == [0, 2]                                     # instance 1 reverts (zero variance)
        for b in ok:
            ks = keys[b].astype(np.int64)
            full = np.sort(ks, axis=0)
            w_lo, w_hi = wc.stored_ends(keys[b], N)
            # runs of equal keys straddle the stored ends in most columns
            lo_run = full[N // 2 - wc.hs() - 1] == w_lo
            hi_run = full[N // 2 + wc.hs()] == w_hi
            assert lo_run.mean() > 0.5 and hi_run.mean() > 0.5
            # column 5: the middle pair is a signed zero on either side
            assert {int(full[N // 2 - 1, 5]), int(full[N // 2, 5])} <= {0, 0x80000000}
            assert fb[b, 9] == hi_can                           # failing rows all at +-0.0: one-sided


def test_conservative_corner():
    """-0.0 has the key of the kernel's -inf sentinel.  No case of the matrix stores a -0.0 as its lowest key behind a
    sentinel at U'[KN - 1], so there the kernel's count is the model's; make_corner() has exactly one such column per
    instance, which the model trusts (its pair is a pair of -0.0, inside the stored range)."""
    for case in wc.matrix():
        assert not wc.make(case)["extra"].any(), case
    for N, f in wc.D_EDGE_SHAPES:
        for D in wc.D_EDGES:
            assert not wc.make_d_edge(N, f, D)["extra"].any(), (N, f, D)
    c = wc.make_corner()
    N, f, D = wc.CORNER
    assert wc.sides(N, f) == (False, False) and not c["fallback"].any()
    keys = wc.keys_of(c["x"][:, :, :D].numpy())
    for b in range(c["B"]):
        assert torch.equal(c["removed"][b], c["is_fail"][b])
        assert np.nonzero(c["extra"][b])[0].tolist() == [wc.CORNER_COLUMN]
        assert wc.pair_inside(keys[b], c["removed"][b].numpy(), N, f).all()
        assert c["ref"]["consensus"][b, wc.CORNER_COLUMN] == 0


@pytest.mark.parametrize("N,f", wc.SHAPES, ids=lambda v: str(v))
def test_random_removed_sets_are_sound(N, f):
    """A few hundred random columns per shape, each with its own removed set -- the lowest, the highest, a mix, or any
    f rows at all (not what a qr ranking would choose) -- on continuous and on tied data."""
    rng = np.random.default_rng(1000 * N + f)
    T = 400
    trusted = 0
    for t in range(T):
        kind = t % 4
        x = rng.beta(20, 20, size=(N, 1)).astype(np.float32)
        if kind == 1:
            x = (np.round(x * 16) / 16).astype(np.float32)
        elif kind == 2:
            x = (np.round(x * 4) / 4).astype(np.float32)
            x[rng.random((N, 1)) < 0.3] = -0.0
        order = np.argsort(x[:, 0], kind="stable")
        k = int(rng.integers(0, f + 1))
        pick = t % 3
        if pick == 0:        # k from the bottom, f - k from the top
            rows = np.concatenate([order[:k], order[N - (f - k):]])
        elif pick == 1:      # any rows
            rows = rng.permutation(N)[:f]
        else:                # k from the bottom, the rest anywhere
            rows = np.concatenate([order[:k], rng.permutation(order[k:])[:f - k]])
        removed = np.zeros(N, dtype=bool)
        removed[rows] = True
        assert removed.sum() == f
        if t % 5 == 0:       # removed values pushed outside the honest range
            x[removed] = rng.choice(np.array([0.0, 1.0], dtype=np.float32), size=(f, 1))
        keys = wc.keys_of(x)
        bad = wc.untrusted_cols(keys, removed, N, f)[0]
        if not bad:
            trusted += 1
            assert wc.pair_inside(keys, removed, N, f)[0], (t, kind, pick, k)
    print(f"({N}, {f}): {trusted} of {T} random columns trusted")
    assert trusted > T // 10


def test_d_edge_cases():
    """The D-edge cases: the model's fallback columns are the planted ones -- the cap's worth in instance 0 (hint
    stays narrow), one more in instance 1 -- and at D = 4096 they touch the first and last words of the bit mask."""
    for N, f in wc.D_EDGE_SHAPES:
        for D in wc.D_EDGES:
            c = wc.make_d_edge(N, f, D)
            print(f"d_edge {N}x{D}x{f}: model fallback columns {c['fallback'].sum(1).tolist()} cap {wc.hint_cap(D)}")
            for b in range(c["B"]):
                assert torch.equal(c["removed"][b], c["is_fail"][b])
                assert sorted(np.nonzero(c["fallback"][b])[0].tolist()) == sorted(c["planted"][b]), (N, f, D, b)
            if D <= wc.MAX_D:
                assert [wc.hint_after(int(n), D) for n in c["fallback"].sum(1)] == [1, 0]
            if D == 4096:
                assert set(wc.REDOW_COLUMNS) <= set(c["planted"][0])
                assert len(c["planted"][0]) == 64


def test_legacy_case():
    """The legacy round's case commits (both reliabilities inside [0, 1]), removes the planted rows and crosses both
    halves of the predicate."""
    c = wc.make_legacy(256, 24, 64)
    assert ((c["ref"]["rel"] > 0.05) & (c["ref"]["rel"] < 0.95)).all(), c["ref"]["rel"]
    assert torch.equal(c["removed"], c["is_fail"]) and not c["extra"].any()
    for b in range(c["B"]):
        ks = sorted(k for (bb, col), k in c["planted"].items() if bb == b and c["fallback"][b, col])
        assert ks and ks[0] == 0 and ks[-1] == c["f"], (b, ks)
        assert 0 < len(ks) < c["f"] + 1
    print("legacy: model fallback columns", c["fallback"].sum(1).tolist())


def test_stream_counters():
    fb = [np.zeros((2, 64), bool), np.ones((2, 64), bool), np.zeros((2, 64), bool), np.zeros((2, 64), bool)]
    # step 1 wide (sets the hint), step 2 narrow and falling back everywhere, step 3 wide, step 4 narrow
    assert wc.stream_counters(fb, 64) == (4, 128)

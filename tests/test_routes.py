"""The route ops (svoc.ops.fast_route / exact_route: csrc/include/svoc/route.hpp, the functions the dispatchers
switch on) against the plain-Python model of tests/route_cases.py, over a grid that holds every boundary on
every axis; and the sizing wrappers against launch.hpp's arithmetic as the model restates it.  No GPU needed: the
ops are pure functions of the shape."""
import pytest

import route_cases as rc
from svoc import ops as svops


def test_fast_route_matches_model():
    raw = svops.ops().fast_route
    n = 0
    for st, N, D, ld, f, c, lg, m, h, w in rc.fast_grid():
        got = tuple(raw(svops.STORAGE[st], N, D, ld, f, c, lg, m, h, w))
        want = tuple(rc.fast(st, N, D, ld, f, c, lg, m, h, w))
        assert got == want, ((st, N, D, ld, f, c, lg, m, h, w), svops.FastRoute(*got), want)
        n += 1
    assert n > 100_000


def test_fast_route_update_bounds():
    """U against the route's bounds: the fused path and the deferred commit take U exactly where their own guards
    (U <= 256 / 127, U * D * 4 B < 2^31, ld * 4 B < 2^24, D % 4 == 0) do -- on the U axis for every D of the grid and
    both ld edges, and for U * D just below and at 2^29."""
    shapes = [(D, (D + 7) // 8 * 8) for D in rc.DS] + [(D, ld) for D in (4, 512) for ld in rc.LD_EDGE]
    cases = [(D, ld, U) for D, ld in shapes for U in rc.US] + list(rc.ud_edge())
    # (at 2^29, and one column short of it: the nearest product below that an integer D gives)
    assert any(U * D == 1 << 29 for D, ld, U in cases) and any(0 < (1 << 29) - U * D <= U for D, ld, U in cases)
    for D, ld, U in cases:
        for N, f, c, h in ((64, 8, True, 0), (256, 32, True, 0), (256, 33, True, 0), (64, 8, False, 0), (64, 8, True, -7)):
            for st in (rc.BF16, rc.FP32):
                r = svops.fast_route(st, N, D, ld, f, c, wave_hint=h)
                m = rc.fast(st, N, D, ld, f, c, False, 0, h, rc.CALLER)
                assert (0 < U <= r.fused_max_u) == rc.fused_takes(m, D, ld, U), (st, N, D, ld, f, c, h, U, r)
                assert (0 < U <= r.defer_max_u) == rc.defer_takes(m, D, ld, U), (st, N, D, ld, f, c, h, U, r)


def test_exact_route_matches_model(monkeypatch):
    for env in ({}, {"SVOC_EXACT_WSAD_MIN_D": "1"}, {"SVOC_EXACT_I128": "1"}):
        for k in ("SVOC_EXACT_I128", "SVOC_EXACT_WSAD_ONLY", "SVOC_EXACT_WSAD_MIN_D"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        kw = dict(wsad_min_d=int(env.get("SVOC_EXACT_WSAD_MIN_D", 64)), force_i128="SVOC_EXACT_I128" in env)
        raw = svops.ops().exact_route
        for N, D, eb, f, c, lg, m in rc.exact_grid():
            got = tuple(raw(N, D, eb, f, c, lg, m))
            assert got == tuple(rc.exact(N, D, eb, f, c, lg, m, **kw)), ((N, D, eb, f, c, lg, m), env, got)


def test_named_tuples_carry_the_ops_fields():
    r = svops.fast_route("fp32", 256, 512, 512, 32, True)
    assert r == svops.FastRoute(kernel=svops.KERNEL_WINDOW, lane_groups=4, win_h=17, needs_work=1, pruned=1, rollback=0,
                                fused_max_u=256, defer_max_u=127)
    assert svops.fast_route("bf16", 16, 128, 128, 2, True).kernel == svops.KERNEL_SMALL
    assert svops.fast_route("bf16", 16, 128, 128, 2, True, wave_hint=4).needs_work == 1
    x = svops.exact_route(256, 64, 4, 32, True)
    assert x == svops.ExactRoute(column=1, lane_groups=4, win_h=17, verdict=1)


@pytest.mark.parametrize("D", [1, 2, 511, 512, 513, 4096])
def test_fast_work_words(D):
    assert svops.fast_work_words(D) == rc.fast_work_words(D)
    assert svops.fast_work_numel(3, D) == 3 * rc.fast_work_words(D)


def test_fast_win_h():
    for N in range(2, 257):
        for f in range(0, 41):
            assert svops.fast_win_h(N, f) == rc.fast_win_h(N, f), (N, f)

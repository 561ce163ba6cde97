"""A plain-Python model of the round-kernel routes (csrc/include/svoc/route.hpp), stated independently: the
conditions the engine and svoc.ops used to spell out themselves, kept here as the test's own restatement (as
exact_cases.py restates launch.hpp).  tests/test_routes.py compares the ops fast_route / exact_route with it."""
import itertools
from collections import namedtuple

BF16, FP32 = "bf16", "fp32"
NONE, CALLER, FRESH = 0, 1, 2          # the caller's workspace
SMALL, WINDOW, TWO_NETWORK = 0, 1, 2   # the kernel

Fast = namedtuple("Fast", "kernel lane_groups win_h needs_work pruned rollback fused_max_u defer_max_u")
Exact = namedtuple("Exact", "column lane_groups win_h verdict")


def groups(N):
    """Lane groups of 64 oracles: 1, 2, 4, ... 64."""
    for g in (1, 2, 4, 8, 16, 32):
        if N <= 64 * g:
            return g
    return 64


def fast_win_h(N, f):
    """The smallest window half-width of {5, 17} that covers the pass-2 middle pair; 0: none."""
    R = N - f
    a = N // 2 - (R // 2 if R >= 0 else -(-R // 2))   # (C's division truncates: f > N)
    need = max(a + 1, f - a + 1)
    return 5 if need <= 5 else 17 if need <= 17 else 0


def fast_work_words(D):
    """u32 words per instance: column pairs padded to 256, 2 columns each, (2 * 17 window keys + 4 power sums
    + 1 cleanup slot + 3 staged outputs) words per column."""
    pairs = ((D + 1) // 2 + 255) // 256 * 256
    return pairs * 2 * (2 * 17 + 4 + 1 + 3)


def fast(storage, N, D, ld, f, constrained, legacy, mode, wave_hint, work):
    small = storage == BF16 and mode == 0 and wave_hint == 0 and N <= 16 and D <= 128
    needs_work = int(not small and mode != 1)
    have = FRESH if (work == NONE and needs_work) else work     # the binding allocates a fresh one
    window = (have != NONE and 2 <= N <= 256 and D <= ld and 0 <= f <= 32 and f <= N - 2
              and not (mode == 2 and have == FRESH)
              and (N * ld * 4 < (1 << 31) if storage == FP32 else ld % 8 == 0))
    win_h = fast_win_h(N, f) if window else 0
    kernel = SMALL if small else WINDOW if (win_h and wave_hint != -7) else TWO_NETWORK
    whole = kernel == WINDOW and mode == 0
    rollback = int(whole and storage == BF16)
    pruned = int(whole and storage == FP32 and constrained and N == 256 and win_h == 17)
    fused = defer = 0
    if whole and storage == FP32 and constrained and ld * 4 < (1 << 24):
        fused = min(256, ((1 << 31) - 1) // (4 * D))       # the largest U <= 256 with U * D * 4 B < 2^31
        defer = min(127, fused) if D % 4 == 0 else 0
    return Fast(kernel, 0 if small else groups(N), win_h, needs_work, pruned, rollback, fused, defer)


def fused_takes(r, D, ld, U):
    """The fused path's own statement of its bounds on U (the dispatcher's guards of old)."""
    return r.fused_max_u > 0 and 0 < U <= 256 and U * D * 4 < (1 << 31) and ld * 4 < (1 << 24)


def defer_takes(r, D, ld, U):
    return fused_takes(r, D, ld, U) and U <= 127 and D % 4 == 0


def exact_win_h(N, f):
    from exact_cases import exact_win_h as h   # the exact model's own restatement
    return h(N, f)


def exact(N, D, elem_bytes, f, constrained, legacy, mode, wsad_min_d=64, force_i128=False):
    g = groups(N)
    column = int(not force_i128 and 4 <= N <= 4096 and not (N > 256 and mode != 0 and not constrained)
                 and not (N <= 32 and D < wsad_min_d) and N * D * elem_bytes < (1 << 31))
    if not column:
        return Exact(0, g, 0, 0)
    whole = mode == 0 and constrained and not legacy
    return Exact(1, g, exact_win_h(N, f) if whole else 0, int(whole and N <= 256))


# ---- the grid: every boundary on every axis (tests/test_routes.py)
NS = (2, 3, 4, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 4096)
DS = (1, 4, 63, 64, 128, 129, 130, 512)
FS = (0, 1, 5, 8, 32, 33, "N-2", "N-1")
MODES = (0, 1, 2)
HINTS = (0, 4, -7)
WORKS = (NONE, CALLER, FRESH)
US = (0, 1, 127, 128, 255, 256, 257)
LD_EDGE = ((1 << 22) - 8, 1 << 22)          # ld * 4 B just below and at 2^24 (multiples of 8: bf16 rows)


def f_of(N, f):
    return N - 2 if f == "N-2" else N - 1 if f == "N-1" else f


def fast_grid():
    """(storage, N, D, ld, f, constrained, legacy, mode, wave_hint, work): the full product of the shape axes with
    ld = D rounded up to 8, then the ld boundary against every other axis (D = 512, 4 rides along)."""
    for st, N, D, f, c, lg, m, h, w in itertools.product((BF16, FP32), NS, DS, FS, (False, True), (False, True), MODES,
                                                         HINTS, WORKS):
        yield st, N, D, (D + 7) // 8 * 8, f_of(N, f), c, lg, m, h, w
    for st, N, ld, f, c, lg, m, h, w in itertools.product((BF16, FP32), NS, LD_EDGE, FS, (False, True), (False, True),
                                                          MODES, HINTS, WORKS):
        for D in (4, 512):
            yield st, N, D, ld, f_of(N, f), c, lg, m, h, w


def ud_edge():
    """(D, ld, U): U * D just below and at 2^29 (U * D * 4 B against 2^31), for every U of the axis that can reach
    it with ld * 4 B < 2^24, and around it."""
    for U in US:
        if U <= 0:
            continue
        for D in {(1 << 29) // U - 1, (1 << 29) // U, -(-(1 << 29) // U), -(-(1 << 29) // U) + 1}:
            if 1 <= D < (1 << 22) - 8:
                yield D, (D + 7) // 8 * 8, U


def exact_grid():
    for N, D, eb, f, c, lg, m in itertools.product(NS, DS + (16, (1 << 31) // (8 * 256), (1 << 31) // (4 * 256)), (4, 8), FS,
                                                   (False, True), (False, True), MODES):
        yield N, D, eb, f_of(N, f), c, lg, m

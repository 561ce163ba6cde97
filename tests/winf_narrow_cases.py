"""Where the fp32 window kernel (consensus_fast_winf.hip) can run a narrow round, and which of its columns must then
fall back to the exact median: a plain numpy / Python model and the cases built on it (CPU only; nothing here
imports GPU code -- svoc.ops is asked for the stored half-width alone).

A narrow round stores and reads HS < H = 17 keys on either side of the column median (window planes KN = H - HS ..
H - 1).  Pass 2 finds its pair among the stored keys from U': `sh` keys of -inf, the f removed keys ascending, then
+inf up to 2H.  The kernel trusts a column iff U'[KN - 1] < w_lo and U'[2H - 2 - KN] > w_hi, both strict, where w_lo /
w_hi are the lowest / highest stored keys (full sorted positions N // 2 - HS and N // 2 - 1 + HS).  `untrusted` states
that on the kernel's keys: the value's word with the sign bit flipped, so -0.0 has key 0 and sorts just below +0.0.
-inf and +inf lie outside the keys (-1 and 2^32).  The kernel's own sentinels are the keys 0 and 2^32 - 1, and -0.0
has the key 0: where U'[KN - 1] is a sentinel and the lowest stored key is a -0.0, the kernel's strict compare fails
and the column takes the exact median although the model trusts it.  That is sound, only conservative;
`conservative_cols` names those columns, no case of the matrix has one, and `make_corner` builds the one case that does.

The removed rows come from fast_cases.ref64 (fp64, Python sort for the rank rule), never from a kernel's output.

tests/test_winf_narrow_cases.py checks the model's soundness and that the cases bite, on the CPU;
tests/test_winf_narrow_shapes_gpu.py runs the kernel against both.
"""
import functools

import numpy as np
import torch

from fast_cases import ref64
from helpers import beta_oracles
from route_cases import fast_win_h
from svoc import ops as svops

H = 17
MAX_D = 4096           # the kernel's LDS bit masks hold this many columns; wider rounds stay wide
KEY_NEG_INF, KEY_POS_INF = -1, 1 << 32


def hs():
    return svops.fast_win_narrow_hs()


def kn():
    return H - hs()


def can_be_narrow(storage, N, D, f, constrained, mode, has_hint):
    """A round of this shape runs narrow for an instance whose hint is set (launch_winf_k's instantiation, the
    binding's hand-over of the hint and the kernel's own D guard, restated)."""
    return (storage == "fp32" and constrained and mode == 0 and has_hint and 129 <= N <= 256 and 0 <= f <= 32
            and f <= N - 2 and fast_win_h(N, f) == H and D <= MAX_D)


def hint_cap(D):
    """Most fallback columns after which an instance's next round is still narrow."""
    return D // 64 if D <= MAX_D else -1     # (-1: no count is low enough -- the hint is written 0)


def low_sentinels(N, f):
    R = N - f
    return H - 1 - (N // 2 - R // 2)


def sides(N, f):
    """(low, high): whether any data at all can fail the lower / the upper half of the predicate.  Lower: U'[KN - 1]
    is a real key only when fewer than KN sentinels stand in front; upper: U'[2H - 2 - KN] is a real key only when
    the sentinels and the f removed keys reach past it."""
    sh = low_sentinels(N, f)
    return sh < kn(), sh + f > 2 * H - 2 - kn()


def keys_of(x):
    """x: float32 array -> the kernel's constrained sort keys (uint32)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) ^ np.uint32(0x80000000)


def u_prime(rem_keys, N, f):
    """rem_keys: [f, ...] uint32, any order -> U' [2H, ...] (int64, ascending)."""
    sh = low_sentinels(N, f)
    assert rem_keys.shape[0] == f and 0 <= sh and sh + f <= 2 * H, (N, f, sh)
    rest = rem_keys.shape[1:]
    lo = np.full((sh,) + rest, KEY_NEG_INF, dtype=np.int64)
    hi = np.full((2 * H - sh - f,) + rest, KEY_POS_INF, dtype=np.int64)
    return np.concatenate([lo, np.sort(rem_keys.astype(np.int64), axis=0), hi], axis=0)


def stored_ends(keys, N):
    """keys: [N, ...] uint32 -> (w_lo, w_hi) int64."""
    full = np.sort(keys.astype(np.int64), axis=0)
    return full[N // 2 - hs()], full[N // 2 - 1 + hs()]


def untrusted_cols(keys, removed, N, f):
    """keys: [N, C] uint32, removed: [N] bool with f rows set -> [C] bool, the columns that must fall back."""
    up = u_prime(keys[removed], N, f)
    w_lo, w_hi = stored_ends(keys, N)
    k = kn()
    return ~((up[k - 1] < w_lo) & (up[2 * H - 2 - k] > w_hi))


def conservative_cols(keys, N, f):
    """[C] bool: U'[KN - 1] is a -inf sentinel and the lowest stored key is -0.0 (module docstring)."""
    w_lo, _ = stored_ends(keys, N)
    return (w_lo == 0) & (low_sentinels(N, f) >= kn())


def untrusted(x, removed, D, only=None):
    """x: [B, N, >= D] float32 tensor, removed: [B, N] bool tensor -> [B, D] bool array.  `only`: the instances
    whose round commits (the others' rows stay False)."""
    B, N = x.shape[:2]
    keys = keys_of(x[:, :, :D].numpy())
    rem = removed.numpy().astype(bool)
    out = np.zeros((B, D), dtype=bool)
    for b in (range(B) if only is None else only):
        out[b] = untrusted_cols(keys[b], rem[b], N, int(rem[b].sum()))
    return out


def untrusted_256x32(x, removed, D, only=None):
    """The model of tests/test_winf_narrow_gpu.py (`_untrusted`), kept word for word in its arithmetic: at N = 256,
    f = 32 the general model must reduce to it."""
    N, F = 256, 32
    k = H - hs()
    keys = np.ascontiguousarray(x[:, :, :D].numpy()).view(np.uint32) ^ np.uint32(0x80000000)
    full = np.sort(keys, axis=1)
    w_lo, w_hi = full[:, N // 2 - hs(), :], full[:, N // 2 - 1 + hs(), :]
    rem_m = removed.numpy().astype(bool)
    out = np.zeros((x.shape[0], D), dtype=bool)
    for b in (range(x.shape[0]) if only is None else only):
        rem = np.sort(keys[b][rem_m[b]], axis=0)
        assert rem.shape[0] == F
        out[b] = ~((rem[k - 1] < w_lo[b]) & (rem[F - k] > w_hi[b]))
    return out


def pair_inside(keys, removed, N, f):
    """[C] bool: the kept rows' sorted ranks R/2 - 1 and R/2 both lie in [w_lo, w_hi] (as keys)."""
    R = N - f
    kept = np.sort(keys[~removed].astype(np.int64), axis=0)
    w_lo, w_hi = stored_ends(keys, N)
    return (kept[R // 2 - 1] >= w_lo) & (kept[R // 2] <= w_hi)


def zero_variance(x, removed, D):
    """[B] bool: some column's kept rows are all equal in value (the constrained round reverts)."""
    out = []
    for b in range(x.shape[0]):
        xr = x[b, :, :D][~removed[b]]
        out.append(bool((xr == xr[0]).all(0).any()))
    return out


# ------------------------------------------------------------------------------------------------ shapes
def smallest_f_with_h17(N):
    return next(f for f in range(0, 33) if fast_win_h(N, f) == H)


ANCHOR = (256, 32)
SHAPES_256 = [ANCHOR, (256, 31), (256, 24), (256, 22), (256, 21), (256, 20), (256, 12)]
SHAPES_SMALL = [(255, 32), (255, 21), (200, 24), (200, 21), (130, 30), (129, 32), (129, 22)]
SHAPES_EDGE = [(256, smallest_f_with_h17(256)), (129, smallest_f_with_h17(129))]
SHAPES = SHAPES_256 + SHAPES_SMALL + SHAPES_EDGE
DS = (64, 100)
B = 3
FAMILIES = ("sym", "low", "high", "split", "ties")     # low / high: every failing row at 0.0 / at 1.0


def matrix():
    return [(fam, N, f, D) for (N, f) in SHAPES for D in DS for fam in FAMILIES]


def case_id(c):
    return "%s-%dx%dx%d" % (c[0], c[1], c[3], c[2])


def seed_of(fam, N, f, D):
    return 1000 * FAMILIES.index(fam) + 7 * N + 3 * f + D


def _fail_rows(is_fail, b):
    return torch.nonzero(is_fail[b]).flatten()


def split_columns(D, f, b):
    """Column of the planted k = 0 .. f of instance b (distinct; the columns in between stay symmetric)."""
    step = max(1, D // (f + 1))
    assert step * (f + 1) <= D
    return [(3 + b + step * k) % D for k in range(f + 1)]


def _data(fam, N, f, D):
    x, is_fail = beta_oracles(B, N, D, f, seed=seed_of(fam, N, f, D), dtype=torch.float32)
    planted = {}
    if fam in ("low", "high"):
        v = 0.0 if fam == "low" else 1.0
        x[:, :, :D] = torch.where(is_fail[:, :, None], torch.tensor(v), x[:, :, :D])
    elif fam == "split":
        for b in range(B):
            rows = _fail_rows(is_fail, b)
            for k, c in enumerate(split_columns(D, f, b)):
                x[b, rows[:k], c] = 0.0
                x[b, rows[k:], c] = 1.0
                planted[(b, c)] = k
    elif fam == "ties":
        x[:, :, :D] = torch.round(x[:, :, :D] * 16) / 16
        for b in range(B):
            fr, hr = _fail_rows(is_fail, b), torch.nonzero(~is_fail[b]).flatten()
            nz = N // 2 + 2                    # the middle of column 5: a run of +0.0 and -0.0
            x[b, hr[:nz], 5] = 0.0
            x[b, hr[:nz:2], 5] = -0.0
            x[b, fr, 9] = 0.0                  # failing rows at +-0.0
            x[b, fr[::2], 9] = -0.0
            x[b, fr[:f // 2], 17] = 0.4375     # failing values inside the honest rows' grid
            x[b, fr[f // 2:], 17] = 0.5625
        x[1, :, 40] = 0.375                    # zero variance: instance 1 reverts
    return x, is_fail, planted


@functools.lru_cache(maxsize=None)
def make(case):
    """One matrix() entry: data, planted failing rows, fp64 reference, the instances that commit and the model's
    [B, D] fallback map (built once, shared, never modified)."""
    fam, N, f, D = case
    x, is_fail, planted = _data(fam, N, f, D)
    ref = ref64(x[:, :, :D], f, True, 1.0)
    removed = ~ref["reliable"]
    zv = zero_variance(x, removed, D)
    ok = [b for b in range(B) if not zv[b]]
    fb = untrusted(x, removed, D, ok)
    return dict(family=fam, N=N, f=f, D=D, B=B, x=x, is_fail=is_fail, planted=planted, ref=ref, removed=removed,
                ok=ok, fallback=fb, extra=conservative(x, D, N, f, ok), legacy=False)


def conservative(x, D, N, f, ok):
    """[B, D] bool: conservative_cols of the committed instances."""
    keys = keys_of(x[:, :, :D].numpy())
    out = np.zeros((x.shape[0], D), dtype=bool)
    for b in ok:
        out[b] = conservative_cols(keys[b], N, f)
    return out


CORNER = (256, 12, 64)
CORNER_COLUMN = 6


@functools.lru_cache(maxsize=None)
def make_corner():
    """Symmetric data at a shape that can never fall back by the model, with one column whose lower half is a run of
    -0.0 reaching past the lowest stored key (then a few +0.0): the kernel's sentinel and that key are equal."""
    N, f, D = CORNER
    x, is_fail = beta_oracles(B, N, D, f, seed=77, dtype=torch.float32)
    for b in range(B):
        hr = torch.nonzero(~is_fail[b]).flatten()
        x[b, hr[:N // 2 + 2], CORNER_COLUMN] = 0.0
        x[b, hr[:N // 2 - 3], CORNER_COLUMN] = -0.0
    ref = ref64(x[:, :, :D], f, True, 1.0)
    removed = ~ref["reliable"]
    ok = list(range(B))
    return dict(family="corner", N=N, f=f, D=D, B=B, x=x, is_fail=is_fail, planted={}, ref=ref, removed=removed,
                ok=ok, fallback=untrusted(x, removed, D), extra=conservative(x, D, N, f, ok), legacy=False)


# ------------------------------------------------------------------------------------------------ D edges
D_EDGE_SHAPES = [ANCHOR, (256, 24)]
D_EDGES = (1, 2, 33, 63, 127, 4096, 4104)
D_EDGE_B = 2
REDOW_COLUMNS = (0, 31, 32, 4064, 4095)     # first and last words of the kernel's 128-word bit mask


def d_edge_planted(D):
    """Per instance, the columns whose failing rows all sit at 1.0 (they fail the lower half of the predicate
    wherever it can fail): instance 0 exactly the cap's worth (its hint stays narrow), instance 1 one more."""
    cap = max(hint_cap(D), 0)
    if D == 4096:
        first = list(REDOW_COLUMNS)
    else:
        first = [c for c in (D - 1, 0, 31, 32) if 0 <= c < D]
    pool = first + [c for c in range(D) if c not in set(first)]
    if D > MAX_D:
        return [pool[:5], pool[:6]]
    return [pool[:cap], pool[:cap + 1]]


@functools.lru_cache(maxsize=None)
def make_d_edge(N, f, D):
    """Every column has f // 2 failing values at 0.0 and the rest at 1.0 (trusted, and a removed set no rounding can
    change), except the planted columns: all at 1.0."""
    x, is_fail = beta_oracles(D_EDGE_B, N, D, f, seed=5000 + N + f + D, dtype=torch.float32)
    planted = d_edge_planted(D)
    for b in range(D_EDGE_B):
        rows = _fail_rows(is_fail, b)
        x[b, rows[:f // 2], :D] = 0.0
        x[b, rows[f // 2:], :D] = 1.0
        for c in planted[b]:
            x[b, rows, c] = 1.0
    ref = ref64(x[:, :, :D], f, True, 1.0)
    removed = ~ref["reliable"]
    fb = untrusted(x, removed, D)
    ok = list(range(D_EDGE_B))
    return dict(family="d_edge", N=N, f=f, D=D, B=D_EDGE_B, x=x, is_fail=is_fail, planted=planted, ref=ref,
                removed=removed, ok=ok, fallback=fb, extra=conservative(x, D, N, f, ok), legacy=False)


@functools.lru_cache(maxsize=None)
def make_legacy(N, f, D):
    """A split case under the obsolete contracts' round (reliability without the / D, no moments).  Its reliability
    1 - 2 sqrt(mean qr) leaves [0, 1] on the unit-interval data, so the values are drawn in around 0.5 by a quarter:
    the planted keys sit at 0.375 / 0.625, still outside the honest rows."""
    x, is_fail, planted = _data("split", N, f, D)
    x = x.clone()
    x[:, :, :D] = 0.5 + (x[:, :, :D] - 0.5) * 0.25
    ref = ref64(x[:, :, :D], f, True, 1.0, legacy=True)
    removed = ~ref["reliable"]
    ok = list(range(B))
    return dict(family="legacy", N=N, f=f, D=D, B=B, x=x, is_fail=is_fail, planted=planted, ref=ref, removed=removed,
                ok=ok, fallback=untrusted(x, removed, D), extra=conservative(x, D, N, f, ok), legacy=True)


# ------------------------------------------------------------------------------------------------ streams
def hint_after(fallbacks, D):
    return int(fallbacks <= hint_cap(D))


def stream_counters(fallback_maps, D):
    """fallback_maps: per step the [B, D] model map of a stream whose rounds all commit, hints starting at zero.
    Returns (narrow rounds, their fallback columns), following each instance's hint from round to round."""
    Bn = fallback_maps[0].shape[0]
    hint = [0] * Bn
    rounds = cols = 0
    for fb in fallback_maps:
        for b in range(Bn):
            n = int(fb[b].sum())
            if hint[b]:
                rounds += 1
                cols += n
            hint[b] = hint_after(n, D)
    return rounds, cols

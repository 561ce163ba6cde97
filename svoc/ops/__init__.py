"""Native op loader: ``torch.ops.svoc.*`` from the in-tree ``svoc/_C.so``.

The shared object holds the gfx950 HIP kernels (csrc/kernels/*.hip), the bit-exact C++ CPU engines
(csrc/engine) and the torch bindings (csrc/bindings).  There is deliberately no silent fallback: if
the extension is missing on a GPU box every op raises, so a "passing" GPU run can never be a hidden
eager-PyTorch run.  Build with ``python csrc/build.py`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import os
import threading
from typing import NamedTuple

import torch

_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_C.so")
_lock = threading.Lock()
_loaded = False


class NativeExtensionMissing(RuntimeError):
    pass


def load(build_if_missing: bool = False) -> None:
    """Load ``svoc/_C.so`` into torch.ops (idempotent)."""
    global _loaded
    if _loaded:
        return
    with _lock:
        if _loaded:
            return
        if not os.path.exists(_LIB):
            if build_if_missing:
                from csrc_build import build  # type: ignore  # pragma: no cover
                build()
            else:
                raise NativeExtensionMissing(
                    f"{_LIB} not built: run `python csrc/build.py` (no eager fallback by design)")
        torch.ops.load_library(_LIB)
        _loaded = True


def available() -> bool:
    try:
        load()
        return True
    except Exception:
        return False


def lib_path() -> str:
    return _LIB


def ops():
    load()
    return torch.ops.svoc


from . import torch_ref  # noqa: E402,F401


# ---- routes (csrc/include/svoc/route.hpp): which kernel runs a round and what it supports.  The C++ functions the
# dispatchers switch on, asked through tensor-less ops; nothing about a kernel's limits is restated here.
STORAGE = {"bf16": 0, "fp32": 1}              # route.hpp FastStorage
WORK_NONE, WORK_CALLER, WORK_FRESH = 0, 1, 2  # route.hpp FastWork
KERNEL_SMALL, KERNEL_WINDOW, KERNEL_TWO_NETWORK = 0, 1, 2   # route.hpp FastKernel


class FastRoute(NamedTuple):
    kernel: int        # KERNEL_*
    lane_groups: int
    win_h: int         # the window kernel's half-width where it applies to the shape (0: it does not)
    needs_work: int    # the kernel needs a workspace (the binding allocates a fresh one per call without the caller's)
    pruned: int        # the pruned window network runs
    rollback: int      # the kernel rolls back a saved batch itself (fast_round's rst_saved)
    fused_max_u: int   # most updates per instance the fused path takes (0: none)
    defer_max_u: int   # ... and its deferred commit (0: none)


class ExactRoute(NamedTuple):
    column: int        # the column-parallel kernel applies (else the i128 kernel alone)
    lane_groups: int   # 1 / 2 / 4, or the wide groups 8 .. 64
    win_h: int
    verdict: int       # the verdict form of the column kernel applies


def fast_route(storage: str, N: int, D: int, ld: int, n_failing: int, constrained: bool, legacy: bool = False,
               mode: int = 0, wave_hint: int = 0, work: int = WORK_CALLER) -> FastRoute:
    """The route of a GPU fast round of this shape (route.hpp fast_route)."""
    return FastRoute(*ops().fast_route(STORAGE[storage], N, D, ld, n_failing, bool(constrained), bool(legacy), mode,
                                       wave_hint, work))


def exact_route(N: int, D: int, elem_bytes: int, n_failing: int, constrained: bool, legacy: bool = False,
                mode: int = 0) -> ExactRoute:
    """The route of a GPU exact round of this shape (route.hpp exact_route), under the environment switches
    ``SVOC_EXACT_I128`` / ``SVOC_EXACT_WSAD_MIN_D`` as they are set now (the op reads them, as exact_round does)."""
    return ExactRoute(*ops().exact_route(N, D, elem_bytes, n_failing, bool(constrained), bool(legacy), mode))


class LestRoute(NamedTuple):
    supported: int     # the rank-weighted kernel takes this shape
    lane_groups: int   # 1 / 2 / 4
    max_n: int         # most oracles it sorts per column
    needs_work: int    # it stages its outputs in the workspace


def lest_route(storage: str, N: int, D: int, ld: int, n_failing: int, constrained: bool, legacy: bool = False,
               mode: int = 0) -> LestRoute:
    """The route of a GPU rank-weighted round of this shape (route.hpp lest_route).  ``storage``: "bf16" / "fp32"."""
    return LestRoute(*ops().lest_route(STORAGE[storage], N, D, ld, n_failing, bool(constrained), bool(legacy), mode))


def fast_work_words(D: int) -> int:
    """u32 words per instance of the fast kernels' workspace (launch.hpp fast_work_words)."""
    return ops().fast_work_words(D)


def fast_work_numel(B: int, D: int) -> int:
    """Total int32 elements of the fast kernels' workspace (B instances)."""
    return B * fast_work_words(D)


def fast_win_h(N: int, f: int) -> int:
    """Window half-width of the one-network kernels (launch.hpp fast_win_h): 5, 17, or 0 (no window)."""
    return ops().fast_win_h(N, f)


def fast_win_narrow_hs() -> int:
    """Stored half-width of a narrow round of the fp32 window kernel (launch.hpp kWinfNarrowHs, of H = 17):
    ``fast_round(..., win_hint=<int32 [B]>)`` lets an instance whose hint is set store and read only that many keys
    on either side of the column median; every round writes the hint for the instance's next round."""
    return ops().fast_win_narrow_hs()

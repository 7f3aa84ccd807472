"""Shared pieces of tests/test_repair_solve.py and tests/test_gpu_repair_solve.py: erasure patterns,
their host coefficients ``G[erased] . inv(G[survivors])`` (computed once per pattern and cached; do not
modify), consistent stripes and guard-filled buffers.

The repair coefficients are unique whenever ``G[survivors]`` is invertible, so every comparison made
with these cases is exact. Only numpy, torch and the package's host code are used here; nothing in
this module touches a GPU unless a test passes ``device="cuda"``.
"""
from __future__ import annotations

import itertools
from functools import lru_cache

import numpy as np
import torch

import solver_cases as sc
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd.ops.gemm import pad_m, perm_tables_from_coeff

F = gf.GF256
GUARD = 0xA5


@lru_cache(maxsize=None)
def codec(k: int, n: int, matrix: str = "cauchy") -> ReedSolomon:
    """One codec per code for the coefficient helpers (its G is read only). Tests that call the
    repair methods build a codec of their own: plans are cached per codec."""
    return ReedSolomon(k, n, matrix=matrix)


def first_survivors(n: int, k: int, erased) -> tuple:
    """The default survivors of a pattern: the first k ids not erased."""
    er = set(erased)
    return tuple(i for i in range(n) if i not in er)[:k]


def all_patterns(n: int, p: int, emin: int = 1) -> list[tuple]:
    """Every pattern of emin..p erasures of an n-chunk code, ascending ids."""
    return [c for e in range(emin, p + 1) for c in itertools.combinations(range(n), e)]


@lru_cache(maxsize=None)
def _inverse(k: int, n: int, matrix: str, survivors: tuple):
    """inv(G[survivors]) of a named code, or None where it is singular (computed once)."""
    try:
        inv = F.invert(codec(k, n, matrix).G[list(survivors)])
    except gf.SingularMatrixError:
        return None
    inv.setflags(write=False)
    return inv


def host_coeff(code, survivors, erased):
    """``G[erased] . inv(G[survivors])`` (e x k) the way the host path computes it, or None for a
    singular pattern. ``code = (k, n, matrix)``."""
    k, n, matrix = code
    inv = _inverse(k, n, matrix, tuple(int(s) for s in survivors))
    if inv is None:
        return None
    return F.matmul(codec(k, n, matrix).G[[int(e) for e in erased]], inv)


def host_coeff_g(g: np.ndarray, survivors, erased) -> np.ndarray:
    """The same for a bare generator (no cache)."""
    return F.matmul(g[[int(e) for e in erased]], F.invert(g[[int(s) for s in survivors]]))


def sample_patterns(n: int, p: int, count: int, seed: int, emin: int = 1, emax: int | None = None) -> list[tuple]:
    """``count`` seeded patterns of emin..emax (default p) erasures, ascending ids, distinct."""
    rng = np.random.default_rng(seed)
    emax = p if emax is None else emax
    out: list[tuple] = []
    while len(out) < count:
        e = int(rng.integers(emin, emax + 1))
        er = tuple(sorted(int(i) for i in rng.choice(n, size=e, replace=False)))
        if er not in out:
            out.append(er)
    return out


# The wide codes: a seeded sample, first and last always 1 and p erasures (host inverses are slow)
WIDE = {(128, 160, "cauchy"): [(5,), (140,)] + sample_patterns(160, 32, 2, 160, 2, 31)
        + [tuple(range(3, 99, 3))] + sample_patterns(160, 32, 1, 161, 32, 32),
        (60, 64, "cauchy"): [(0,), (63,)] + sample_patterns(64, 4, 8, 64) + [(1, 30, 59, 62), (60, 61, 62, 63)]}

# Caller-chosen survivors that skip available natives: (code, survivors, erased)
CHOSEN = [((10, 14, "cauchy"), (13, 0, 12, 2, 3, 11, 5, 6, 10, 9), (7, 1)),
          ((10, 14, "cauchy"), (13, 12, 11, 10, 9, 8, 7, 6, 5, 4), (0, 1, 2, 3)),
          ((10, 14, "cauchy"), (0, 1, 2, 3, 4, 5, 6, 7, 8, 13), (10, 12)),       # native 9 left out, not erased
          ((10, 14, "cauchy"), (1, 2, 3, 4, 5, 6, 7, 8, 9, 12), (13,)),           # native 0 left out, parity erased
          ((4, 8, "cauchy"), (7, 6, 5, 4), (3, 0, 1, 2)),                         # no native survives; erased unsorted
          ((4, 8, "cauchy"), (4, 5, 6, 7), (0,)),
          ((3, 19, "cauchy"), (18, 1, 10), (0, 2, 3, 17)),
          ((60, 64, "cauchy"), tuple(range(2, 60)) + (63, 61), (0, 62, 1))]


def vandermonde_singular() -> list[tuple]:
    """The patterns of 1..4 erasures of the reference Vandermonde (10, 14) whose default survivors are
    singular, found with ``ReedSolomon.decode_matrix`` (the host path's own solve)."""
    from gpu_rscode_amd.models.rs import UnrecoverableError

    rs = ReedSolomon(10, 14, matrix="vandermonde")
    out = []
    for er in all_patterns(14, 4):
        try:
            rs.decode_matrix(first_survivors(14, 10, er))
        except UnrecoverableError:
            out.append(er)
    return out


# ---- the planted pivoting systems of tests/solver_cases.py (imported, not edited) --------------------
PIVOT_GOOD = sc.DS8            # scattered pivot order; the last is (128, 256) with a = 128
PIVOT_SINGULAR = sc.DS8_SINGULAR  # e = 70: a dependent column at 0, 1, 35 (the middle) and 69 (e - 1)


def pivot_codec(case) -> ReedSolomon:
    """A codec whose generator is the case's, assigned as ``rs.E`` / ``rs.G``."""
    g = sc.system(case)[0]
    rs = ReedSolomon(case.k, case.n, matrix="cauchy")
    rs.E = np.array(g[case.k:])
    rs.G = np.array(g)
    return rs


# ---- descriptors and tables ----------------------------------------------------------------------------
def table_block(coeff: np.ndarray | None, k: int, m_pad: int) -> np.ndarray:
    """The ``(k, m_pad, 8)`` uint32 table block of an e x k coefficient matrix (None: all zero)."""
    blk = np.zeros((k, m_pad, 8), dtype=np.uint32)
    if coeff is not None and len(coeff):
        blk[:, : coeff.shape[0]] = np.transpose(perm_tables_from_coeff(coeff.astype(np.uint8)), (1, 0, 2))
    return blk


def coeff_block(coeff: np.ndarray | None, k: int, m_pad: int) -> np.ndarray:
    blk = np.zeros((m_pad, k), dtype=np.uint8)
    if coeff is not None and len(coeff):
        blk[: coeff.shape[0]] = coeff
    return blk


def id_arrays(survivors, erased, m_pad: int | None = None):
    """int32 ``[npat, k]`` and ``[npat, m_pad]`` (padded with -1) of per-pattern id lists."""
    m_pad = pad_m(max(len(e) for e in erased)) if m_pad is None else m_pad
    sv = np.array([list(s) for s in survivors], dtype=np.int32)
    er = np.full((len(erased), m_pad), -1, dtype=np.int32)
    for q, e in enumerate(erased):
        er[q, : len(e)] = list(e)
    return sv, er


# ---- stripes -------------------------------------------------------------------------------------------
def consistent(g: np.ndarray, nstripes: int, ncols: int, seed: int) -> np.ndarray:
    """``[B, n, C]`` consistent stripes of the generator ``g`` (seeded random natives)."""
    n, k = g.shape
    data = np.random.default_rng(seed).integers(0, 256, size=(nstripes, k, ncols), dtype=np.uint8)
    flat = data.transpose(1, 0, 2).reshape(k, -1)
    par = F.gemm(g[k:], flat).reshape(n - k, nstripes, ncols).transpose(1, 0, 2)
    return np.concatenate([data, par], axis=1)


def damage(good: np.ndarray, erased, fill: int = 0xEE) -> np.ndarray:
    """``good`` with the rows ``erased[b]`` of stripe b overwritten."""
    bad = np.array(good)
    for b, ids in enumerate(erased):
        for i in ids:
            if i >= 0:
                bad[b, i] = fill
    return bad


def arena(host: np.ndarray, device: str):
    """``(buffer, stripes)``: a guard-filled ``[B, n, pitch]`` buffer (pitch a multiple of 16, at least
    16 guard bytes after each row) and its ``[B, n, C]`` view holding ``host``."""
    b, n, c = host.shape
    pitch = (c + 16 + 15) // 16 * 16
    buf = torch.full((b, n, pitch), GUARD, dtype=torch.uint8, device=device)
    stripes = buf[:, :, :c]
    stripes.copy_(torch.from_numpy(host))
    return buf, stripes


def assert_arena(buf: torch.Tensor, want: np.ndarray, what: str = "") -> None:
    """Every byte of the buffer: rows equal ``want``, everything past them is still the guard."""
    got = buf.cpu().numpy()
    c = want.shape[2]
    assert np.array_equal(got[:, :, :c], want), f"{what}: rows differ"
    assert (got[:, :, c:] == GUARD).all(), f"{what}: guard bytes overwritten"

"""The planted solver cases (tests/solver_cases.py) on the host: every case that
tests/test_gpu_solvers.py runs makes the kernels' pivot rule do what the case is there for, the host
solvers agree with the numpy oracle on it, and a solve that never searches for a pivot fails on it
while it passes on a Cauchy system of the same size."""
import numpy as np
import pytest

import solver_cases as sc
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import cpu, hip
from gpu_rscode_amd.gf import GF256
from gpu_rscode_amd.models.rs import UnrecoverableError

GOOD = [c for c in sc.all_cases() if c.good]
SINGULAR = [c for c in sc.all_cases() if not c.good]
EMBEDDED = [c for c in sc.all_cases() if c.k]


def _limit_cases():
    e = sc.limit_e(hip().decode_system16_supported)
    return sc.limit_case(e), sc.limit_case(e + 1)


def _rs(case) -> ReedSolomon:
    G = sc.system(case)[0]
    rs = ReedSolomon(case.k, case.n, matrix="cauchy", field="gf256" if case.w == 8 else "gf65536")
    rs.E = np.array(G[case.k:])
    rs.G = np.array(G)
    return rs


def _check_good(case):
    seq, failed = sc.sequence(case)
    assert failed is None, f"no pivot in column {failed}"
    assert sorted(seq) == list(range(case.e))
    assert not sc.sequence_gaps(seq, case.e, case.panels)


def _check_embedding(case):
    m = sc.matrix(case)[0]
    G, rows, erased = sc.system(case)
    k, n, e = case.k, case.n, case.e
    assert G.shape == (n, k) and np.array_equal(G[:k], np.eye(k, dtype=G.dtype))
    assert len(rows) == k and len(set(rows)) == k and all(0 <= r < n for r in rows)
    assert list(erased) == [i for i in range(k) if i not in set(rows)] and len(erased) == e
    assert list(rows) != sorted(rows) or k == 1
    assert np.array_equal(sc.system_matrix(G, k, rows, erased), m)


@pytest.mark.parametrize("case", GOOD, ids=str)
def test_good_case_makes_the_solvers_pivot(case):
    """The kernels' rule, simulated: a pivot in every column, at most 10 % of the columns take row c
    (a 1 x 1 system has no other order), and at every panel width the case runs with, every panel
    after the first takes a pivot row from above its own rows and, unless it is the last panel and
    has none, one from below them. A system of one panel needs only a non-identity order."""
    _check_good(case)
    if case.w == 16:  # no accidental zero pivot in 65,536 elements: the order is the planted one
        assert sc.sequence(case)[0] == sc.predicted_sequence(case.blocks, sc.matrix(case)[1])


@pytest.mark.parametrize("case", SINGULAR, ids=str)
def test_singular_case_fails_at_its_column(case):
    seq, failed = sc.sequence(case)
    assert failed == case.dep_col and len(seq) == case.dep_col


@pytest.mark.parametrize("case", EMBEDDED, ids=str)
def test_embedding_reads_back_the_planted_matrix(case):
    """The generator holds the planted matrix exactly where the kernels gather M from, and the
    survivor list is a shuffled, valid pattern whose missing natives are ``erased``."""
    _check_embedding(case)


def test_cases_at_the_one_workgroup_limit():
    """The two systems built around decode_system16_supported's own limit (e = k, n = 2 e) meet the
    same conditions; the first fits the one-workgroup kernel past 64 KiB of LDS, the second does not."""
    at, past = _limit_cases()
    sup = hip().decode_system16_supported
    assert sup(at.n, at.k, at.e) and not sup(past.n, past.k, past.e) and past.e == at.e + 1
    assert 4 * at.e * at.e > 65536  # (the e x 2e system alone, 2-byte symbols: past 64 KiB)
    for case in (at, past):
        _check_good(case)
        _check_embedding(case)
        rs = _rs(case)
        G, rows, erased = sc.system(case)
        assert np.array_equal(rs._erased_rows(rows, erased), sc.oracle_rows(case))


# ---- host solvers against the numpy oracle ----------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in sc.all_cases() if c.w == 8 and not c.k], ids=str)
def test_host_invert_matches_oracle(case):
    """gfrs::invert (bound as _cpu.invert) on the bare planted matrices; None for a singular one."""
    m = sc.matrix(case)[0]
    raw = cpu().invert(np.ascontiguousarray(m).tobytes(), case.e)
    if not case.good:
        assert raw is None
        with pytest.raises(gf.SingularMatrixError):
            GF256.invert(m)
        return
    got = np.frombuffer(raw, dtype=np.uint8).reshape(case.e, case.e)
    assert np.array_equal(got, sc.oracle_inverse(case))
    assert np.array_equal(GF256.matmul(m, got), np.eye(case.e, dtype=np.uint8))


@pytest.mark.parametrize("case", [c for c in EMBEDDED if c.w == 16], ids=str)
def test_host_gf16_decode_rows_match_oracle(case):
    """gfrs::gf16w::decode_rows (ReedSolomon._erased_rows, the reference of every w = 16 GPU test)
    equals rows ``erased`` of the numpy inverse of G[rows]; a singular system raises."""
    rs = _rs(case)
    G, rows, erased = sc.system(case)
    if not case.good:
        with pytest.raises(UnrecoverableError):
            rs._erased_rows(rows, erased)
        with pytest.raises(gf.SingularMatrixError):
            case.F.invert(G[list(rows)])
        return
    assert np.array_equal(rs._erased_rows(rows, erased), sc.oracle_rows(case))


@pytest.mark.parametrize("case", [c for c in EMBEDDED if c.w == 8], ids=str)
def test_host_decode_matrix_matches_oracle(case):
    """ReedSolomon.decode_matrix (gfrs::decode_matrix) for w = 8; a singular system raises."""
    rs = _rs(case)
    G, rows, erased = sc.system(case)
    if not case.good:
        with pytest.raises(UnrecoverableError):
            rs.decode_matrix(rows)
        with pytest.raises(gf.SingularMatrixError):
            GF256.invert(G[list(rows)])
        return
    assert np.array_equal(rs.decode_matrix(rows)[list(erased)], sc.oracle_rows(case))


# ---- the cases see what Cauchy cannot ---------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in GOOD if c.e > 1], ids=str)
def test_solve_without_pivot_search_fails_on_planted_and_passes_on_cauchy(case):
    """A Gauss-Jordan that takes row c as column c's pivot without searching stops at a zero pivot
    on every good planted case, and solves the Cauchy system of the same size exactly. (GF(2^8) has
    no Cauchy block past 128 x 128: the two largest gf_invert cases run the first half only.)"""
    F, e = case.F, case.e
    eye = np.eye(e, dtype=np.int64)
    with pytest.raises(sc.ZeroPivot):
        sc.solve_without_search(F, sc.matrix(case)[0], eye)
    if 2 * e <= F.order:
        c = F.cauchy(e, e)
        assert sc.pivot_sequence(F, c) == (list(range(e)), None)
        assert np.array_equal(sc.solve_without_search(F, c, eye), F.invert(c))

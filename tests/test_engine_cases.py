"""The engine cases of tests/engine_cases.py held to their stated conditions with the numpy oracle
alone (no GPU): a case that silently stopped testing anything fails here.

The counts come from an integer bit-matrix product (``engine_cases.counts``) that uses neither the
kernels nor the oracle's gemm; the selection and XOR expectations come straight from the input rows.
The table builders (``perm_tables_from_coeff``, the C++ ``gf16_perm_quad``) are pinned for every
coefficient of their field to the oracle's multiply on the basis symbols."""
import numpy as np
import pytest

import engine_cases as ec
from gpu_rscode_amd import gf
from gpu_rscode_amd._native import cpu
from gpu_rscode_amd.ops.gemm import perm_tables_from_coeff

# the values this project's polynomials (0x11D, 0x1100B) give, as a cross-check of the derivation
SAT8 = (245, 247, 196, 46, 144, 61, 122, 244)
SAT16 = (0xf007, 0x5003, 0xa006, 0x372e, 0x6e5c, 0xdcb8, 0xa97b, 0x42fd, 0x85fa, 0x1bff, 0x37fe, 0x6ffc, 0x5a02,
         0xb404, 0x7803, 0xf006)

# every (w, k, m) the GPU module runs the ladder on
LADDER_SHAPES = [(8, 128, 8), (8, 100, 17), (8, 256, 40), (8, 128, 16), (8, 128, 32), (8, 128, 20), (8, 128, 26),
                 (8, 128, 24), (16, 300, 40), (16, 300, 35), (16, 17, 20), (16, 64, 16)]


@pytest.mark.parametrize("w,want", [(8, SAT8), (16, SAT16)])
def test_saturating_coefficients(w, want):
    """c_b's bit-matrix row b is all ones, and no other element's is (the map c -> row b is a
    bijection onto GF(2)^w, checked by the rank in w = 16 and by the search in w = 8)."""
    F = ec.field(w)
    sat = ec.saturating(w)
    assert sat == want
    img = ec.bit_images(F, np.array(sat))
    for b in range(w):
        assert img[b, b, :].all()
        x = np.arange(F.order)
        par = np.zeros(F.order, dtype=np.int64)  # XOR of all bits of x
        for a in range(w):
            par ^= (x >> a) & 1
        assert np.array_equal((F.mul(sat[b], x) >> b) & 1, par)
    allrows = ec.bit_images(F, np.arange(F.order)).all(axis=2)  # [c, b]
    assert allrows.sum(axis=0).tolist() == [1] * w


def test_counts_and_oracle_gemm_agree_with_the_oracle():
    """On a small random case: parity of the integer counts == F.gemm == the cached-table gemm."""
    for w in (8, 16):
        F = ec.field(w)
        rng = np.random.default_rng(w)
        coeff = rng.integers(0, F.order, size=(5, 7))
        coeff[0, :2] = [0, 1]
        data = ec.random_symbols(w, 7, 300, 3)
        want = F.gemm(coeff, data)
        assert np.array_equal(ec.oracle_gemm(F, coeff, data), want)
        assert np.array_equal(ec.from_counts(F, ec.counts(F, coeff, data)), want)
    # and on a whole ladder shape, where the matrix holds 16 distinct coefficients in 340 entries
    F = ec.field(16)
    coeff, data = ec.ladder_coeff(16, 20, 17), ec.ladder_data(16, 17)
    assert np.array_equal(ec.oracle_gemm(F, coeff, data), F.gemm(coeff, data))


@pytest.mark.parametrize("w,k,m", LADDER_SHAPES)
def test_ladder_reaches_every_count(w, k, m):
    """On every saturating row the saturated bit's counts are exactly {w t} and {w t - 1}, the
    maximum over all bits is w k, at least 8 laps run, every output bit has a saturating row, and
    the outputs the counts give equal the oracle's."""
    F = ec.field(w)
    coeff, data = ec.ladder_coeff(w, m, k), ec.ladder_data(w, k)
    assert data.shape == (k, 16 * (k + 1) + 77) and data.shape[1] // (k + 1) >= 8
    cnt = ec.counts(F, coeff, data)
    want = ec.ladder_count_set(w, k)
    t, odd = ec.ladder_heights(k)
    assert {i % w for i in range(m)} == set(range(w))
    for i in range(m):
        b = i % w
        assert set(np.unique(cnt[i, b]).tolist()) == want, (i, b)
        assert np.array_equal(cnt[i, b], w * t - (odd & (t >= 1))), (i, b)  # column by column
    assert cnt.max() == w * k
    assert np.array_equal(ec.from_counts(F, cnt), ec.oracle_gemm(F, coeff, data))


def test_ladder_one_row_shapes_cover_every_bit():
    """The int8 engine's (k, m) = (255, 1): one row, so the case runs once per ``first`` = 0..7."""
    F, w, k = ec.field(8), 8, 255
    data = ec.ladder_data(w, k)
    for first in range(w):
        coeff = ec.ladder_coeff(w, 1, k, first)
        assert (coeff == ec.saturating(w)[first]).all()
        cnt = ec.counts(F, coeff, data)
        assert set(np.unique(cnt[0, first]).tolist()) == ec.ladder_count_set(w, k)
        assert cnt.max() == w * k


@pytest.mark.parametrize("w,k,m", [(8, 128, 32), (8, 256, 40), (16, 300, 40)])
def test_random_case_stays_below_half_the_range(w, k, m):
    """Why the ladder is needed: random operands of the same shape never reach half of w k."""
    F = ec.field(w)
    rng = np.random.default_rng(k + m)
    coeff = rng.integers(0, F.order, size=(m, k))
    data = ec.random_symbols(w, k, ec.ladder_ncols(k), k)
    assert ec.counts(F, coeff, data).max() < w * k // 2


# ---- B ------------------------------------------------------------------------------------------------
# every (field, engine) whose shape the GPU module runs: the tables are shared with it
STRUCT_ENGINES = [(w, e) for w in (8, 16) for e in sorted(ec.engines(w))]


def test_null_tail_exceptions_are_the_one_tile_kernels():
    """Only kernels that exist for a single tile of at most 4 rows (rows-in-flight at its own tile,
    GF(2^16) two groups per lane) may miss the whole null tile at the end."""
    short = {(w, e) for w, e in STRUCT_ENGINES if ec.engines(w)[e][1] < 2 * ec.engines(w)[e][3] + 2}
    assert short == ec.NULL_TAIL_ONE_ROW
    for w, e in short:
        k, m, _, tile = ec.engines(w)[e]
        assert m == tile <= 4


@pytest.mark.parametrize("w,engine", STRUCT_ENGINES)
def test_structured_cases_hold_their_conditions(w, engine):
    """The structured cases exactly as the GPU module builds them for this engine (same shape, tile
    and seed)."""
    k, m, _, tile = ec.engines(w)[engine]
    F = ec.field(w)
    seed = ec.engine_seed(w, engine)
    data = ec.random_symbols(w, k, 97, 11)
    assert not ec.structured("zero", w, m, k, tile, seed).any()
    assert (ec.structured("all_ones", w, m, k, tile, seed) == 1).all()
    # null rows and columns: exactly the stated ones, random (nonzero) elsewhere
    c = ec.structured("null_rows_cols", w, m, k, tile, seed)
    rows, cols = ec.null_layout(m, k, tile)
    live_r = [i for i in range(m) if i not in rows]
    live_c = [j for j in range(k) if j not in cols]
    assert live_r and live_c
    assert not c[rows].any() and not c[:, cols].any()
    assert (c[np.ix_(live_r, live_c)] != 0).all()
    assert 0 in rows and tile - 1 in rows  # first and last row of the first output tile
    if (w, engine) in ec.NULL_TAIL_ONE_ROW:
        assert rows == [0, m - 1]
    else:  # a whole tile's worth at the end, live rows between it and the first tile's null rows
        assert set(range(m - tile, m)) <= set(rows) and len(live_r) >= 2
        assert rows == sorted({0, tile - 1} | set(range(m - tile, m)))
    # selection: one unit entry per row, an injection until it wraps
    c = ec.structured("selection", w, m, k, tile, seed)
    pi = ec.selection_map(m, k, seed)
    assert (c.sum(axis=1) == 1).all() and (c[np.arange(m), pi] == 1).all()
    assert len(set(pi[:k].tolist())) == min(m, k)
    if m > k:
        assert np.array_equal(pi[k:], pi[: m - k])
    # thirds: zeros, ones and others all present, a third each on the larger matrices
    c = ec.structured("thirds", w, m, k, tile, seed)
    frac = [(c == 0).mean(), (c == 1).mean(), (c > 1).mean()]
    assert min(frac) > 0
    if m * k >= 1000:
        assert 0.28 < min(frac) and max(frac) < 0.39
    # the expectations that need no field arithmetic equal the oracle's
    for name in ec.STRUCTURED:
        c = ec.structured(name, w, m, k, tile, seed)
        exp = ec.structured_expect(name, w, m, k, seed, data)
        assert (exp is None) == (name in ("null_rows_cols", "thirds"))
        if exp is not None:
            assert np.array_equal(exp, ec.oracle_gemm(F, c, data)), name
    sel = ec.structured_expect("selection", w, m, k, seed, data)
    for i in range(m):
        assert np.array_equal(sel[i], data[pi[i]])
    assert np.array_equal(ec.structured_expect("all_ones", w, m, k, seed, data)[m - 1],
                          np.bitwise_xor.reduce(data, axis=0))


# ---- C ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 16])
def test_every_coefficient_case(w):
    """Every coefficient appears once; every impulse column has one nonzero input row; the table is
    the oracle's product; the expected output equals the oracle's gemm (w = 16: on three rows)."""
    F = ec.field(w)
    coeff, data, table = ec.every_coeff(w)
    n, per = ec.every_dims(w)
    assert sorted(coeff.reshape(-1).tolist()) == list(range(F.order))
    imp = data[:, : n * per]
    assert ((imp != 0).sum(axis=0) <= 1).all()
    for j in (0, 1, n - 1):
        vals = imp[j, per * j: per * (j + 1)].astype(np.int64)
        assert np.array_equal(vals, np.arange(per) if w == 8 else 1 << np.arange(per))
        assert not imp[j, : per * j].any() and not imp[j, per * (j + 1):].any()
    assert data.shape[1] - n * per == (1000 if w == 8 else 256)
    for i, j, v in [(0, 0, 1), (3, 7, per - 1), (n - 1, n - 1, per // 2), (n - 1, 0, 3)]:
        x = int(data[j, per * j + v])
        assert int(table[i, per * j + v]) == int(F.mul(int(coeff[i, j]), x))
    exp = ec.every_expect(w)
    rows = list(range(n)) if w == 8 else [0, 1, n - 1]
    assert np.array_equal(exp[rows], F.gemm(coeff[rows], data))


def test_perm_tables_every_gf256_coefficient():
    """The v_perm records of all 256 coefficients reproduce the oracle's product on every byte."""
    F = gf.GF256
    tabs = perm_tables_from_coeff(np.arange(256).reshape(16, 16)).reshape(256, 8)
    x = np.arange(256, dtype=np.uint8)
    for c in range(256):
        assert np.array_equal(gf.perm_apply(tabs[c], x), F.mul(c, x).astype(np.uint8)), c


def _apply_quads(quads: np.ndarray, x: int) -> np.ndarray:
    """The device lookup (gf.quad_apply16) of symbol x through N quads at once: (N,) uint16."""
    b = np.ascontiguousarray(quads.astype("<u4")).view(np.uint8).reshape(-1, 4, 32)

    def look(q, v):  # byte v through map q of every coefficient
        return b[:, q, v & 7] ^ b[:, q, 8 + ((v >> 3) & 7)] ^ b[:, q, 16 + (v >> 6)]
    lo, hi = x & 0xFF, x >> 8
    ol = look(0, lo) ^ look(2, hi)
    oh = look(1, lo) ^ look(3, hi)
    return ol.astype(np.uint16) | (oh.astype(np.uint16) << 8)


def test_perm_quads_every_gf65536_coefficient():
    """The C++ byte-map quadruple (gfrs::gf16w::perm_quad) of all 65,536 coefficients, applied as the
    kernel applies it, gives the oracle's product on the 16 basis symbols (hence on every symbol);
    the numpy builder gives the same records."""
    F = ec.field(16)
    h = cpu()
    quads = np.array([h.gf16_perm_quad(c) for c in range(65536)], dtype=np.uint32).reshape(65536, 4, 8)
    c = np.arange(65536)
    for e in range(16):
        assert np.array_equal(_apply_quads(quads, 1 << e), F.mul(c, 1 << e).astype(np.uint16)), e
    assert np.array_equal(_apply_quads(quads, 0xFFFF), F.mul(c, 0xFFFF).astype(np.uint16))
    for hi in range(0, 256, 32):
        part = np.arange(256 * hi, 256 * (hi + 32)).reshape(32, 256)
        assert np.array_equal(gf.perm_quads16(part).reshape(-1, 4, 8), quads[256 * hi: 256 * (hi + 32)]), hi

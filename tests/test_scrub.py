"""Scrub on CPU tensors: syndrome mask, corrupt-chunk location and heal against the numpy oracle
(``gf.scrub_oracle``), exactly. The case functions take the device, so tests/test_gpu_scrub.py runs
the same cases through the gfx950 kernels."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, UnrecoverableError, alloc_rows, flat_rows, gf

# (k, n, matrix). (3, 4) has p = 1 (nothing can be located), (20, 36) fills a 16-row output tile,
# (32, 52) needs two tiles and is beyond the locate kernel (p > 16): syndrome_mask only.
CODES = [(4, 6, "vandermonde"), (4, 6, "cauchy"), (10, 14, "vandermonde"), (10, 14, "cauchy"),
         (5, 8, "sys_vandermonde"), (3, 4, "vandermonde"), (20, 36, "vandermonde"), (32, 52, "cauchy")]
# tail only | one 16-byte group, with and without a tail byte | one workgroup span, with and without
# a tail | crosses a 65536-byte mask block | several blocks
SHAPES = [1, 15, 16, 17, 4096, 4101, 65536 + 3, 3 * 65536 + 4097]
BLOCKS = [4096, 65536]
GARBAGE = 0xA5


def code_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}"


@lru_cache(maxsize=None)
def codec(code) -> ReedSolomon:
    k, n, matrix = code
    return ReedSolomon(k, n, matrix=matrix)


@lru_cache(maxsize=None)
def host_stripe(code, ncols: int) -> np.ndarray:
    """A consistent [n, C] stripe, encoded by the numpy oracle; shared by every test, never modified."""
    k, n, _ = code
    rng = np.random.default_rng(1000 * n + ncols)
    data = rng.integers(0, 256, size=(k, ncols), dtype=np.uint8)
    out = np.vstack([data, gf.GF256.gemm(codec(code).E, data)])
    out.setflags(write=False)
    return out


def to_device(host: np.ndarray, device: str) -> torch.Tensor:
    """The stripe in alloc_rows storage whose pitch padding past C holds garbage."""
    t = alloc_rows(host.shape[0], host.shape[1], device, fill=GARBAGE)
    t.copy_(torch.from_numpy(np.array(host)))
    return t


def stripe_bytes(t) -> np.ndarray:
    rows = [t[i] for i in range(t.shape[0])] if isinstance(t, torch.Tensor) else t
    return np.stack([r.cpu().numpy() for r in rows])


def assert_matches_oracle(rs, stripe, host, block_bytes, locate=True):
    mask, votes, unlocated, bad = gf.scrub_oracle(rs.H, host, block_bytes)
    got_mask = rs.syndrome_mask(stripe, block_bytes)
    assert got_mask.dtype == torch.int32 and np.array_equal(got_mask.cpu().numpy(), mask)
    if not locate:
        return None
    rep = rs.scrub(stripe, block_bytes)
    assert np.array_equal(rep.mask.cpu().numpy(), mask)
    assert rep.votes.dtype == np.int64 and np.array_equal(rep.votes, votes)
    assert (rep.unlocated, rep.bad_columns) == (unlocated, bad)
    assert rep.clean == (bad == 0) and rep.suspects == [int(j) for j in np.nonzero(votes)[0]]
    return rep


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_clean(device, code, ncols):
    rs = codec(code)
    stripe = to_device(host_stripe(code, ncols), device)
    assert int((flat_rows(stripe) == GARBAGE).sum()) >= stripe.stride(0) - ncols  # the padding is garbage
    for bb in BLOCKS:
        mask = rs.syndrome_mask(stripe, bb)
        assert tuple(mask.shape) == (-(-ncols // bb),) and not mask.cpu().numpy().any()
        if rs.p > 16:
            with pytest.raises(NotImplementedError):
                rs.scrub(stripe, bb)
            continue
        rep = rs.scrub(stripe, bb)
        assert rep.clean and rep.bad_columns == 0 and rep.unlocated == 0 and rep.suspects == []
        assert not rep.votes.any() and not rep.mask.cpu().numpy().any()
        assert rs.heal(stripe, rep) is rep


def case_single_flip(device, code, ncols, bb):
    """One byte of chunk j flipped at column c, for every j and c in {0, block boundary, C - 1}: the
    mask is nonzero only in block c // bb, with exactly the bits {i : H[i][j] != 0}; one vote for j."""
    rs = codec(code)
    stripe = to_device(host_stripe(code, ncols), device)
    h = rs.H
    for j in range(rs.n):
        for c in sorted(c for c in {0, bb - 1, bb, ncols - 1} if c < ncols):
            stripe[j, c] ^= 0x5A
            mask = rs.syndrome_mask(stripe, bb).cpu().numpy()
            want = np.zeros(-(-ncols // bb), dtype=np.int64)
            want[c // bb] = sum(1 << (i % 32) for i in range(rs.p) if h[i, j])
            assert np.array_equal(mask.astype(np.int64) & 0xFFFFFFFF, want), (j, c)
            if rs.p <= 16:
                rep = rs.scrub(stripe, bb)
                assert rep.bad_columns == 1 and not rep.clean, (j, c)
                votes = np.zeros(rs.n, dtype=np.int64)
                if rs.p >= 2:
                    votes[j] = 1
                assert np.array_equal(rep.votes, votes), (j, c, rep.votes)
                assert rep.unlocated == (0 if rs.p >= 2 else 1)
                assert rep.suspects == ([j] if rs.p >= 2 else [])
            stripe[j, c] ^= 0x5A
    assert not rs.syndrome_mask(stripe, bb).cpu().numpy().any()


def case_chunk_overwritten(device, code, ncols):
    """A whole chunk replaced by seeded random bytes: every result equals the oracle's at both block
    sizes, votes[j] is the number of columns that differ, and heal restores the stripe bit-exactly."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    j = (3 * ncols + rs.n) % rs.n
    bad = np.array(good)
    bad[j] = np.random.default_rng(ncols).integers(0, 256, size=ncols, dtype=np.uint8)
    differ = int((bad[j] != good[j]).sum())
    stripe = to_device(bad, device)
    for bb in BLOCKS:
        rep = assert_matches_oracle(rs, stripe, bad, bb, locate=rs.p <= 16)
    if rs.p > 16:
        with pytest.raises(NotImplementedError):
            rs.scrub(stripe)
        return
    assert rep.bad_columns == differ
    if rs.p < 2:  # every bad column is counted, none located
        assert rep.unlocated == differ and rep.suspects == [] and not rep.votes.any()
        if differ:
            with pytest.raises(UnrecoverableError):
                rs.heal(stripe)
            assert np.array_equal(stripe_bytes(stripe), bad)
        return
    assert rep.votes[j] == differ and rep.unlocated == 0
    healed = rs.heal(stripe)
    assert healed.clean and healed.suspects == []
    assert np.array_equal(stripe_bytes(stripe), good)


def recoverable_pairs(rs):
    """Chunk pairs whose repair is solvable from the survivors reconstruct picks (the first k others)."""
    out = []
    for a in range(rs.n):
        for b in range(a + 1, rs.n):
            if rs.is_recoverable([i for i in range(rs.n) if i not in (a, b)][: rs.k]):
                out.append((a, b))
    return out


def case_two_chunks_disjoint(device, code, ncols=4101):
    rs = codec(code)
    good = host_stripe(code, ncols)
    pairs = recoverable_pairs(rs)
    picks = [pairs[0], pairs[len(pairs) // 2], pairs[-1]]  # native+native, mixed, parity side
    for a, b in picks:
        bad = np.array(good)
        bad[a, 5:105] ^= 0x11
        bad[b, 4090:4101] ^= 0xC3
        stripe = to_device(bad, device)
        rep = assert_matches_oracle(rs, stripe, bad, 4096)
        assert rep.suspects == [a, b] and rep.votes[a] == 100 and rep.votes[b] == 11 and rep.unlocated == 0
        assert rs.heal(stripe, rep).clean
        assert np.array_equal(stripe_bytes(stripe), good)


def case_two_chunks_same_column(device, code, ncols=4101):
    """Two chunks wrong in the same byte column: that column is unlocated, never a vote (these check
    matrices have no dependent column triples), and heal refuses without touching the stripe."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    cols = [0, 16, 4095, 4096, ncols - 1]
    for a, b in [(0, 1), (1, rs.k), (rs.k, rs.n - 1), (rs.k - 1, rs.n - 1)]:
        bad = np.array(good)
        for t, c in enumerate(cols):
            bad[a, c] ^= 1 + t
            bad[b, c] ^= 0x80 >> t
        stripe = to_device(bad, device)
        rep = assert_matches_oracle(rs, stripe, bad, 4096)
        assert rep.unlocated == len(cols) and rep.bad_columns == len(cols)
        assert not rep.votes.any() and rep.suspects == []
        with pytest.raises(UnrecoverableError):
            rs.heal(stripe)
        assert np.array_equal(stripe_bytes(stripe), bad)
        with pytest.raises(UnrecoverableError):
            rs.heal(stripe, rep)
        assert np.array_equal(stripe_bytes(stripe), bad)


def case_unaligned_rows(device, code, ncols):
    """Rows as separately allocated tensors, one starting at a 1-byte offset: the same results as the
    aligned stripe."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    bad[1, ncols // 2] ^= 0x77
    bad[rs.n - 1, ncols - 1] ^= 0x01
    for host in (good, bad):
        rows = []
        for i in range(rs.n):
            buf = torch.full((ncols + 17,), GARBAGE, dtype=torch.uint8, device=device)
            row = buf[1: 1 + ncols] if i == 2 else buf[16: 16 + ncols]
            row.copy_(torch.from_numpy(np.array(host[i])))
            rows.append(row)
        assert rows[2].data_ptr() % 16 != 0
        aligned = to_device(host, device)
        for bb in BLOCKS:
            rep = assert_matches_oracle(rs, rows, host, bb)
            ref = rs.scrub(aligned, bb)
            assert np.array_equal(rep.votes, ref.votes) and rep.suspects == ref.suspects
            assert (rep.clean, rep.bad_columns, rep.unlocated) == (ref.clean, ref.bad_columns, ref.unlocated)
            assert np.array_equal(rep.mask.cpu().numpy(), ref.mask.cpu().numpy())
    healed = rs.heal(rows)
    assert healed.clean and np.array_equal(stripe_bytes(rows), good)


def case_other_fields(device):
    for field, n in (("gf16", 6), ("gf65536", 6)):
        rs = ReedSolomon(4, n, matrix="cauchy", field=field)
        stripe = alloc_rows(n, 64, device, fill=0)
        for call in (rs.syndrome_mask, rs.scrub, rs.heal):
            with pytest.raises(NotImplementedError, match=field):
                call(stripe)


# ---- the CPU tests ------------------------------------------------------------------------------------
def test_oracle_on_a_hand_made_stripe():
    """scrub_oracle itself, on a code small enough to check by hand: H = [[1, 1, 1, 0], [1, 2, 0, 1]]."""
    h = gf.check_matrix(np.array([[1, 1], [1, 2]], dtype=np.uint8))
    assert h.tolist() == [[1, 1, 1, 0], [1, 2, 0, 1]] and gf.columns_independent(h)
    data = np.array([[7, 9, 200, 0, 1], [3, 3, 5, 0, 255]], dtype=np.uint8)
    stripe = np.vstack([data, gf.GF256.gemm(h[:, :2], data)])
    mask, votes, unl, bad = gf.scrub_oracle(h, stripe, 4096)
    assert mask.tolist() == [0] and votes.tolist() == [0, 0, 0, 0] and (unl, bad) == (0, 0)
    stripe[1, 0] ^= 1   # native 1: syndrome (1, 2) at column 0
    stripe[2, 3] ^= 9   # parity 0: syndrome (9, 0) at column 3
    stripe[0, 4] ^= 4   # native 0 and parity 1 at column 4: syndrome (4, 4 ^ 6) = (4, 2), no single chunk
    stripe[3, 4] ^= 6
    mask, votes, unl, bad = gf.scrub_oracle(h, stripe, 4096)
    assert mask.tolist() == [3] and votes.tolist() == [0, 1, 1, 0] and (unl, bad) == (1, 3)
    assert not gf.columns_independent(np.array([[1, 2, 1, 0], [3, 6, 0, 1]]))  # column 1 = 2 x column 0
    assert not gf.columns_independent(np.array([[1, 0, 1, 0], [3, 0, 0, 1]]))


@pytest.mark.parametrize("ncols", SHAPES)
@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_clean_stripe(code, ncols):
    case_clean("cpu", code, ncols)


@pytest.mark.parametrize("ncols,bb", [(17, 4096), (4101, 4096), (65536 + 3, 65536)])
@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_single_byte_flip(code, ncols, bb):
    case_single_flip("cpu", code, ncols, bb)


@pytest.mark.parametrize("ncols", SHAPES)
@pytest.mark.parametrize("code", CODES, ids=code_id)
def test_whole_chunk_overwritten(code, ncols):
    case_chunk_overwritten("cpu", code, ncols)


@pytest.mark.parametrize("code", [c for c in CODES if 2 <= c[1] - c[0] <= 16], ids=code_id)
def test_two_chunks_damaged_at_disjoint_columns(code):
    case_two_chunks_disjoint("cpu", code)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (10, 14, "cauchy"), (5, 8, "sys_vandermonde")], ids=code_id)
def test_two_chunks_damaged_in_the_same_column(code):
    case_two_chunks_same_column("cpu", code)


@pytest.mark.parametrize("ncols", [15, 4101, 65536 + 3])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (20, 36, "vandermonde")], ids=code_id)
def test_unaligned_rows(code, ncols):
    case_unaligned_rows("cpu", code, ncols)


def test_other_fields_raise():
    case_other_fields("cpu")


def test_dependent_check_columns_locate_nothing():
    """An encoding block with two proportional columns: every bad column is unlocated."""
    rs = ReedSolomon(4, 6, matrix="cauchy")
    e = np.array(rs.E)
    e[:, 1] = gf.GF256.mul(e[:, 0], 3)
    rs.E = e
    rs.G = np.vstack([np.eye(4, dtype=np.uint8), e])
    data = np.random.default_rng(5).integers(0, 256, size=(4, 300), dtype=np.uint8)
    host = np.vstack([data, gf.GF256.gemm(e, data)])
    host[3, 7] ^= 0x40
    rep = assert_matches_oracle(rs, to_device(host, "cpu"), host, 4096)
    assert (rep.bad_columns, rep.unlocated, rep.suspects) == (1, 1, [])


def test_block_bytes_is_checked():
    rs = codec((4, 6, "cauchy"))
    stripe = to_device(host_stripe((4, 6, "cauchy"), 17), "cpu")
    for bad in (0, 2048, 4097, 3 * 4096):
        with pytest.raises(ValueError):
            rs.syndrome_mask(stripe, bad)
    with pytest.raises(ValueError):
        rs.scrub(stripe[:5])

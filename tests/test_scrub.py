"""Scrub on CPU tensors: syndrome mask, corrupt-chunk location and heal against the numpy oracle
(``gf.scrub_oracle``), exactly. The case functions take the device, so tests/test_gpu_scrub.py runs
the same cases through the gfx950 kernels."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, UnrecoverableError, alloc_rows, flat_rows, gf
from gpu_rscode_amd.ops.scrub import ScrubPlan, cpu_scrub

# (k, n, matrix). (3, 4) has p = 1 (nothing can be located), (20, 36) fills a 16-row output tile,
# (32, 52) needs two tiles and is beyond the locate kernel (p > 16): syndrome_mask only.
CODES = [(4, 6, "vandermonde"), (4, 6, "cauchy"), (10, 14, "vandermonde"), (10, 14, "cauchy"),
         (5, 8, "sys_vandermonde"), (3, 4, "vandermonde"), (20, 36, "vandermonde"), (32, 52, "cauchy")]
# tail only | one 16-byte group, with and without a tail byte | one workgroup span, with and without
# a tail | crosses a 65536-byte mask block | several blocks
SHAPES = [1, 15, 16, 17, 4096, 4101, 65536 + 3, 3 * 65536 + 4097]
BLOCKS = [4096, 65536]
GARBAGE = 0xA5

# Codes for the parts of the kernels that CODES never reaches. p = 5, 6, 8: the 8-row tile, with and
# without padding rows ((9, 14) has the rows-in-flight kernel's n but m_pad = 8, so the general
# kernel). p = 9, 13, 15: the 16-row tile with padding rows. Odd n ((20, 35), (5, 7), (9, 13),
# (1, 3), (2, 3)): the last row of the two-rows-in-flight loop has no partner. (240, 256): the locate
# kernel's tables full. (128, 160): two full tiles, mask bits 0..31. (200, 256): p = 56, four tiles,
# rows 32.. fold onto bits 0..23. The last two are beyond the locate kernel: syndrome_mask only.
CODES_EDGE = [(9, 14, "cauchy"), (12, 18, "cauchy"), (8, 16, "vandermonde"), (7, 16, "cauchy"),
              (11, 24, "vandermonde"), (20, 35, "cauchy"), (5, 7, "vandermonde"), (9, 13, "cauchy"),
              (1, 3, "cauchy"), (1, 2, "vandermonde"), (2, 3, "cauchy"), (240, 256, "cauchy"),
              (128, 160, "cauchy"), (200, 256, "cauchy")]
# lone tail | one group and a tail | a workgroup edge | a mask-block edge; the wide codes (whose
# oracle costs the most) keep the two that hold a group, a tail and a workgroup edge
EDGE_SHAPES = [(c, s) for c in CODES_EDGE for s in ([1, 17, 4101, 65536 + 3] if c[1] <= 36 else [17, 4101])]
EDGE_FLIPS = [(c, s, bb) for c in CODES_EDGE
              for s, bb in ([(17, 4096), (4101, 4096), (65536 + 3, 65536)] if c[1] <= 36 else [(17, 4096)])]
EDGE_LOCATING = [c for c in CODES_EDGE if 2 <= c[1] - c[0] <= 16]
WIDEST = (200, 256, "cauchy")
# encoding blocks with zero entries: code -> (pivot row of native column j = 0, 1, .., further zeros)
SPARSE = {(20, 36, "cauchy"): ([0, 1, 3, 4, 7, 8, 11, 12, 14], [(5, 10), (9, 11), (15, 12), (2, 13), (13, 13)]),
          (12, 18, "cauchy"): ([0, 3, 4], []),
          (10, 14, "cauchy"): ([0, 1, 2], [])}
SPARSE_UNALIGNED = [(20, 36, "cauchy"), (12, 18, "cauchy")]
MIXED = [(10, 14, "cauchy"), (4, 6, "cauchy"), (20, 36, "cauchy")]
ALL_VALUES = [(10, 14, "vandermonde"), (12, 18, "cauchy"), (20, 36, "vandermonde")]
BLOCK_SIZE_CODES = [(10, 14, "vandermonde"), (12, 18, "cauchy")]


def code_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}"


def run_id(r):
    return "-".join(str(v) for v in r[0] + r[1:])


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
            for i in range(rs.p):
                if h[i, j]:
                    want[c // bb] |= 1 << (i % 32)
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
            # (every square block of a Cauchy matrix is invertible, so every pattern is recoverable:
            # no k x k inversion per pair, which at n = 256 would be 32640 of them)
            if rs.matrix == "cauchy" or rs.is_recoverable([i for i in range(rs.n) if i not in (a, b)][: rs.k]):
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


def unaligned_rows(host, device):
    """The stripe as separately allocated tensors, row 2 starting at a 1-byte offset."""
    ncols = host.shape[1]
    rows = []
    for i in range(host.shape[0]):
        buf = torch.full((ncols + 17,), GARBAGE, dtype=torch.uint8, device=device)
        row = buf[1: 1 + ncols] if i == 2 else buf[16: 16 + ncols]
        row.copy_(torch.from_numpy(np.array(host[i])))
        rows.append(row)
    assert rows[2].data_ptr() % 16 != 0
    return rows


def case_unaligned_rows(device, code, ncols):
    """Rows as separately allocated tensors, one starting at a 1-byte offset: the same results as the
    aligned stripe."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    bad[1, ncols // 2] ^= 0x77
    bad[rs.n - 1, ncols - 1] ^= 0x01
    for host in (good, bad):
        rows = unaligned_rows(host, device)
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


def case_wide_two_natives(device, code=WIDEST, ncols=4101):
    """p = 56: two natives damaged at different columns of one block. The mask word is the OR of both
    chunks' rows folded mod 32 (rows 32..55 land on bits 0..23), and scrub still refuses p > 16."""
    rs = codec(code)
    assert rs.p > 32
    bad = np.array(host_stripe(code, ncols))
    a, b = 3, rs.k - 50
    bad[a, 100] ^= 0x21
    bad[b, 3000] ^= 0x9C
    stripe = to_device(bad, device)
    word = 0
    for j in (a, b):
        for i in range(rs.p):
            if rs.H[i, j]:
                word |= 1 << (i % 32)
    mask = rs.syndrome_mask(stripe, 4096).cpu().numpy()
    assert (mask.astype(np.int64) & 0xFFFFFFFF).tolist() == [word, 0]
    assert np.array_equal(mask, gf.scrub_oracle(rs.H, bad, 4096)[0])
    with pytest.raises(NotImplementedError):
        rs.scrub(stripe, 4096)


# ---- check matrices the codecs never produce ----------------------------------------------------------
def scrub_with(device, h, rows, block_bytes, ident=None):
    """``(mask, votes, unlocated, bad_columns)`` of a stripe under any p x n check matrix ``h``: a
    ScrubPlan's two kernels on CUDA rows (``ident``, if given, is what the plan must have found for
    the trailing identity columns), cpu_scrub on CPU rows."""
    h = np.asarray(h, dtype=np.uint8)
    rows = [rows[i] for i in range(len(rows))]
    if torch.device(device).type == "cuda":
        plan = ScrubPlan(rows, h, block_bytes)
        assert ident is None or plan.ident == ident
        mask = plan.syndrome_mask().cpu().numpy()
        rep = plan.scrub()
        assert np.array_equal(rep.mask.cpu().numpy(), mask)
        return mask, rep.votes, rep.unlocated, rep.bad_columns
    ncols = min(r.numel() for r in rows)
    mask, votes, unlocated, bad = cpu_scrub(h, rows, ncols, block_bytes, codec(CODES[1])._cpu_gemm)
    return mask.numpy(), votes, unlocated, bad


def assert_scrub_with(device, h, rows, host, block_bytes, ident=None):
    mask, votes, unlocated, bad = gf.scrub_oracle(h, host, block_bytes)
    got = scrub_with(device, h, rows, block_bytes, ident)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], mask)
    assert np.array_equal(got[1], votes), (got[1], votes)
    assert (got[2], got[3]) == (unlocated, bad)
    return got


def encode_with(e, ncols, seed):
    """A consistent stripe of the systematic code with encoding block ``e``, by the numpy oracle."""
    data = np.random.default_rng(seed).integers(0, 256, size=(e.shape[1], ncols), dtype=np.uint8)
    return np.vstack([data, gf.GF256.gemm(e, data)])


def sparse_block(code):
    """The code's Cauchy block with rows 0..r-1 of native column j zeroed (r = SPARSE's pivot row of
    j) and a few zeros below the pivots: pivots in every word of the locate kernel's packed syndrome,
    and zero entries of H (whose log the kernel stores as 510). A pivot in row p - 1 would leave a
    multiple of an identity column, so p - 2 is the last one."""
    pivots, extra = SPARSE[code]
    e = np.array(codec(code).E)
    for j, r in enumerate(pivots):
        e[:r, j] = 0
    for i, j in extra:
        e[i, j] = 0
    h = gf.check_matrix(e)
    assert gf.columns_independent(h)
    assert [int(np.nonzero(h[:, j])[0][0]) for j in range(len(pivots))] == pivots
    return e


def mixed_check_matrix(code):
    """H' = M . H with a seeded invertible M (no zero entry): the same null space, so the code's
    stripes stay consistent, but the last p columns are M, not the identity."""
    rs = codec(code)
    rng = np.random.default_rng(77 + rs.n)
    while True:
        m = rng.integers(1, 256, size=(rs.p, rs.p), dtype=np.uint8)
        if gf.GF256.is_invertible(m):
            break
    h = gf.GF256.matmul(m, rs.H).astype(np.uint8)
    assert gf.columns_independent(h) and not np.array_equal(h[:, rs.k:], np.eye(rs.p, dtype=np.uint8))
    return h


def all_values_stripe(good):
    """Chunk j XORed with 1..255 at columns 255 j .. 255 j + 254: every error value in every chunk,
    one wrong chunk per column, the last 7 columns clean."""
    n = good.shape[0]
    assert good.shape[1] == 255 * n + 7
    bad = np.array(good)
    for j in range(n):
        bad[j, 255 * j: 255 * j + 255] ^= np.arange(1, 256, dtype=np.uint8)
    return bad


def case_all_error_values(device, h, good, ident=None, rows_of=to_device):
    """Every result equals the oracle's at both block sizes; under a systematic H with pairwise
    independent columns every one of the 255 n bad columns names its chunk."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    bad = all_values_stripe(good)
    stripe = rows_of(bad, device)
    for bb in BLOCKS:
        _, votes, unlocated, bad_columns = assert_scrub_with(device, h, stripe, bad, bb, ident)
        assert bad_columns == 255 * n
        if p >= 2 and np.array_equal(h[:, n - p:], np.eye(p, dtype=np.uint8)) and gf.columns_independent(h):
            assert votes.tolist() == [255] * n and unlocated == 0
    return votes, unlocated


def assert_clean_with(device, h, rows, host, ident=None):
    for bb in BLOCKS:
        mask, votes, unlocated, bad = assert_scrub_with(device, h, rows, host, bb, ident)
        assert not mask.any() and not votes.any() and (unlocated, bad) == (0, 0)


def case_all_values_codec(device, code):
    case_all_error_values(device, codec(code).H, host_stripe(code, 255 * code[1] + 7), ident=code[1] - code[0])


def case_sparse(device, code):
    e = sparse_block(code)
    h = gf.check_matrix(e)
    good = encode_with(e, 255 * code[1] + 7, 31)
    assert_clean_with(device, h, to_device(good, device), good, ident=code[1] - code[0])
    case_all_error_values(device, h, good, ident=code[1] - code[0])


def case_sparse_unaligned(device, code):
    """The sparse H on rows of which one starts at an odd address: the bytewise arms of both kernels
    (16-row tile and, with (12, 18), the 8-row tile, which no other unaligned case has)."""
    e = sparse_block(code)
    h = gf.check_matrix(e)
    good = encode_with(e, 255 * code[1] + 7, 32)
    assert_clean_with(device, h, unaligned_rows(good, device), good)
    case_all_error_values(device, h, good, rows_of=unaligned_rows)


def case_mixed(device, code):
    """A check matrix without an identity block: every multiply is done (ident = 0), natives are
    located as before, and damage on the parity side, whose columns of H' are no unit vectors, is
    unlocated, as the documented classification says."""
    rs = codec(code)
    h = mixed_check_matrix(code)
    good = host_stripe(code, 255 * rs.n + 7)
    assert_clean_with(device, h, to_device(good, device), good, ident=0)
    votes, unlocated = case_all_error_values(device, h, good, ident=0)
    if rs.p > 2:  # (with p = 2 a multiple of a column of H' may have a single nonzero byte)
        assert votes.tolist() == [255] * rs.k + [0] * rs.p and unlocated == 255 * rs.p


def case_dependent_columns(device):
    """An encoding block with two proportional columns (p = 2): every bad column is unlocated."""
    rs = ReedSolomon(4, 6, matrix="cauchy")
    e = np.array(rs.E)
    e[:, 1] = gf.GF256.mul(e[:, 0], 3)
    rs.E = e
    rs.G = np.vstack([np.eye(4, dtype=np.uint8), e])
    assert not gf.columns_independent(rs.H)
    data = np.random.default_rng(5).integers(0, 256, size=(4, 300), dtype=np.uint8)
    host = np.vstack([data, gf.GF256.gemm(e, data)])
    host[3, 7] ^= 0x40
    stripe = to_device(host, device)
    rep = assert_matches_oracle(rs, stripe, host, 4096)
    assert (rep.bad_columns, rep.unlocated, rep.suspects) == (1, 1, [])
    host[0, 299] ^= 0x01
    host[5, 16] ^= 0xFF
    stripe = to_device(host, device)
    _, votes, unlocated, bad = assert_scrub_with(device, rs.H, stripe, host, 4096, ident=2)
    assert not votes.any() and (unlocated, bad) == (3, 3)


def case_block_sizes(device, code):
    """One flipped byte on either side of every 16 KiB locate-span edge and in the last column, each
    in another chunk, at block sizes below, at and above the span, and one larger than the stripe
    (a single mask word that all four locate workgroups read)."""
    rs = codec(code)
    ncols = 3 * 16384 + 4097
    bad = np.array(host_stripe(code, ncols))
    hits = {0: 16383, rs.k - 1: 16384, rs.k: 32767, rs.n - 1: 32768, 1: ncols - 1}
    for j, c in hits.items():
        bad[j, c] ^= 0x80 | j
    stripe = to_device(bad, device)
    for bb in (4096, 8192, 16384, 32768, 1 << 20):
        rep = assert_matches_oracle(rs, stripe, bad, bb)
        assert rep.mask.numel() == -(-ncols // bb)
        assert rep.suspects == sorted(hits) and rep.votes.sum() == 5 and (rep.unlocated, rep.bad_columns) == (0, 5)


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
    case_dependent_columns("cpu")


# ---- the edge codes and the matrices no codec produces -----------------------------------------------
@pytest.mark.parametrize("code,ncols", EDGE_SHAPES, ids=map(run_id, EDGE_SHAPES))
def test_edge_clean_stripe(code, ncols):
    case_clean("cpu", code, ncols)


@pytest.mark.parametrize("code,ncols,bb", EDGE_FLIPS, ids=map(run_id, EDGE_FLIPS))
def test_edge_single_byte_flip(code, ncols, bb):
    case_single_flip("cpu", code, ncols, bb)


@pytest.mark.parametrize("code,ncols", EDGE_SHAPES, ids=map(run_id, EDGE_SHAPES))
def test_edge_whole_chunk_overwritten(code, ncols):
    case_chunk_overwritten("cpu", code, ncols)


@pytest.mark.parametrize("code", EDGE_LOCATING, ids=code_id)
def test_edge_two_chunks_damaged_at_disjoint_columns(code):
    case_two_chunks_disjoint("cpu", code)


def test_p56_two_natives_fold_into_one_word():
    case_wide_two_natives("cpu")


@pytest.mark.parametrize("code", ALL_VALUES, ids=code_id)
def test_every_error_value_in_every_chunk(code):
    case_all_values_codec("cpu", code)


@pytest.mark.parametrize("code", list(SPARSE), ids=code_id)
def test_sparse_check_matrix(code):
    case_sparse("cpu", code)


@pytest.mark.parametrize("code", SPARSE_UNALIGNED, ids=code_id)
def test_sparse_check_matrix_on_unaligned_rows(code):
    case_sparse_unaligned("cpu", code)


@pytest.mark.parametrize("code", MIXED, ids=code_id)
def test_check_matrix_without_identity_block(code):
    case_mixed("cpu", code)


@pytest.mark.parametrize("code", BLOCK_SIZE_CODES, ids=code_id)
def test_block_sizes_and_span_edges(code):
    case_block_sizes("cpu", code)


def test_block_bytes_is_checked():
    rs = codec((4, 6, "cauchy"))
    stripe = to_device(host_stripe((4, 6, "cauchy"), 17), "cpu")
    for bad in (0, 2048, 4097, 3 * 4096):
        with pytest.raises(ValueError):
            rs.syndrome_mask(stripe, bad)
    with pytest.raises(ValueError):
        rs.scrub(stripe[:5])

"""Batched scrub on CPU tensors: ``syndrome_mask_batch``, ``scrub_batch`` and ``heal_batch`` against the
numpy oracle (``gf.scrub_oracle``) applied stripe by stripe, exactly. The case functions take the
device, so tests/test_gpu_scrub_batch.py runs the same cases through the batched gfx950 kernels."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, flat_rows, gf
from test_scrub import GARBAGE, code_id, codec, host_stripe, stripe_bytes, to_device, unaligned_rows

# rows-in-flight kernel with the identity shortcut (two of them) | the general vec kernel at the
# rows-in-flight kernel's n | p = 17: two output tiles, mask bits 16 and up | p = 56: four tiles, rows
# 32.. fold onto bits 0..23. The last two are beyond the locate kernel: masks only.
CODES = [(4, 6, "cauchy"), (10, 14, "vandermonde"), (9, 14, "cauchy"), (19, 36, "cauchy"), (200, 256, "cauchy")]
LOCATING = [c for c in CODES if c[1] - c[0] <= 16]
BB = 4096
# (B, C): every B of {1, 2, 3, 257} and every C of {1, 15, 16, 17, 4096, 4101, 8192 + 3}: tail lanes
# only | a group with and without a tail | one workgroup span, with and without a tail | three mask
# words. nmask is 1, 2 or 3. Many stripes go with a short row, and once with a row of two mask words.
RUNS = [(1, 1), (2, 15), (3, 16), (257, 17), (2, 4096), (3, 4101), (3, 8192 + 3), (257, 4101)]
# the oracle's cost grows with n p C per stripe: (19, 36) leaves out the long rows of the large batch,
# (200, 256), whose oracle takes 0.3 s a stripe, keeps to three stripes
TALL_RUNS = [r for r in RUNS if r != (257, 4101)]
WIDE_RUNS = [(1, 1), (2, 15), (3, 16), (3, 17), (2, 4096), (3, 4101)]


def runs_of(codes):
    return [(c, b, s) for c in codes for b, s in (RUNS if c[1] <= 14 else TALL_RUNS if c[1] <= 36 else WIDE_RUNS)]


def run_id(r):
    return f"{code_id(r[0])}-B{r[1]}-C{r[2]}"


def host_batch(code, nstripes: int, ncols: int) -> np.ndarray:
    """[B, n, C]: B different consistent stripes, cut from one long stripe of test_scrub's (column
    ranges of a consistent stripe are consistent). Shared and read-only."""
    long = host_stripe(code, nstripes * ncols)
    return long.reshape(code[1], nstripes, ncols).transpose(1, 0, 2)


def batch_to_device(host: np.ndarray, device: str) -> torch.Tensor:
    """The batch as one [B, n, C] view of alloc_rows storage whose pitch padding holds garbage."""
    b, n, c = host.shape
    return to_device(np.ascontiguousarray(host).reshape(b * n, c), device).view(b, n, c)


@lru_cache(maxsize=None)
def check_matrix(code) -> np.ndarray:
    return codec(code).H


def oracle_batch(code, host: np.ndarray, block_bytes: int):
    """gf.scrub_oracle stripe by stripe: (mask [B, nmask], votes [B, n], unlocated [B], bad [B])."""
    res = [gf.scrub_oracle(check_matrix(code), np.ascontiguousarray(s), block_bytes) for s in host]
    nmask = -(-host.shape[2] // block_bytes)
    return (np.stack([r[0] for r in res]).reshape(len(res), nmask), np.stack([r[1] for r in res]),
            np.array([r[2] for r in res], dtype=np.int64), np.array([r[3] for r in res], dtype=np.int64))


def assert_report_equal(got, want):
    """Two ScrubReports, field for field."""
    assert (got.clean, got.bad_columns, got.unlocated, got.suspects) == \
        (want.clean, want.bad_columns, want.unlocated, want.suspects)
    assert got.votes.dtype == np.int64 and np.array_equal(got.votes, want.votes)
    assert got.mask.dtype == torch.int32 and np.array_equal(got.mask.cpu().numpy(), want.mask.cpu().numpy())


def assert_batch_matches_oracle(code, stripes, host, block_bytes=BB, parity=None, singles=None):
    """Every batched result equals the oracle's for that stripe; ``singles`` (the stripes as the
    single-stripe calls take them) are also scrubbed one by one on the same buffers, for the first,
    the last and every dirty stripe."""
    rs = codec(code)
    nstripes = host.shape[0]
    mask, votes, unlocated, bad = oracle_batch(code, host, block_bytes)
    got = rs.syndrome_mask_batch(stripes, parity, block_bytes)
    assert got.dtype == torch.int32 and tuple(got.shape) == mask.shape
    assert np.array_equal(got.cpu().numpy(), mask)
    if rs.p > 16:
        with pytest.raises(NotImplementedError):
            rs.scrub_batch(stripes, parity, block_bytes)
        return None
    rep = rs.scrub_batch(stripes, parity, block_bytes)
    assert rep.mask.dtype == torch.int32 and np.array_equal(rep.mask.cpu().numpy(), mask)
    assert rep.mask.device == got.device
    assert rep.votes.dtype == np.int64 and np.array_equal(rep.votes, votes)
    assert rep.unlocated.dtype == np.int64 and np.array_equal(rep.unlocated, unlocated)
    assert rep.bad_columns.dtype == np.int64 and np.array_equal(rep.bad_columns, bad)
    assert rep.clean.dtype == np.bool_ and np.array_equal(rep.clean, bad == 0)
    assert rep.dirty == [int(b) for b in np.nonzero(bad)[0]] and rep.unhealed == []
    assert len(rep.report) == nstripes
    for b in sorted({0, nstripes - 1, *rep.dirty}):
        one = rep.report[b]
        assert (one.clean, one.bad_columns, one.unlocated) == (bool(bad[b] == 0), int(bad[b]), int(unlocated[b]))
        assert np.array_equal(one.votes, votes[b]) and one.suspects == [int(j) for j in np.nonzero(votes[b])[0]]
        assert np.array_equal(one.mask.cpu().numpy(), mask[b])
        if singles is not None:
            assert_report_equal(one, rs.scrub(singles[b], block_bytes))
    return rep


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_clean(device, code, nstripes, ncols, block_bytes=BB):
    """1. A clean batch: every mask word zero, every stripe's report clean; the pitch padding holds
    garbage, so a kernel that reads past C fails here."""
    rs = codec(code)
    host = host_batch(code, nstripes, ncols)
    stripes = batch_to_device(host, device)
    assert int((flat_rows(stripes.view(-1, ncols)) == GARBAGE).sum()) >= stripes.stride(1) - ncols
    mask = rs.syndrome_mask_batch(stripes, block_bytes=block_bytes)
    assert tuple(mask.shape) == (nstripes, -(-ncols // block_bytes)) and not mask.cpu().numpy().any()
    rep = assert_batch_matches_oracle(code, stripes, host, block_bytes, singles=stripes)
    if rep is not None:
        assert rep.clean.all() and rep.dirty == [] and not rep.votes.any() and not rep.mask.cpu().numpy().any()
        assert all(rep.report[b].clean for b in range(nstripes))
        assert rs.heal_batch(stripes, report=rep) is rep and rep.unhealed == []


def dirty_stripes(nstripes: int, which: str) -> list[int]:
    """The stripes b = 1 mod 3, with stripe 0 dirty and the last one clean ("first") or the other
    way round ("last"); a batch of one is dirty either way."""
    rule = {b for b in range(nstripes) if b % 3 == 1}
    if which == "first":
        return sorted((rule - {nstripes - 1}) | {0})
    return sorted((rule - {0}) | {nstripes - 1})


def case_stripe_identity(device, code, nstripes, ncols, which):
    """2. One byte flipped in chunk b % n at column 37 b % C of the chosen stripes: their mask rows,
    votes and reports are the oracle's, and every other stripe's are zero."""
    rs = codec(code)
    bad = np.array(host_batch(code, nstripes, ncols))
    dirty = dirty_stripes(nstripes, which)
    for b in dirty:
        bad[b, b % rs.n, (37 * b) % ncols] ^= 0x5A
    stripes = batch_to_device(bad, device)
    rep = assert_batch_matches_oracle(code, stripes, bad, singles=stripes)
    mask = rs.syndrome_mask_batch(stripes, block_bytes=BB).cpu().numpy()
    assert [int(b) for b in np.nonzero(mask.any(axis=1))[0]] == dirty
    for b in dirty:  # the right word of the right row, and the bits the check matrix dictates
        want = np.zeros(mask.shape[1], dtype=np.int64)
        for i in np.nonzero(rs.H[:, b % rs.n])[0]:
            want[(37 * b) % ncols // BB] |= 1 << (int(i) % 32)
        assert np.array_equal(mask[b].astype(np.int64) & 0xFFFFFFFF, want), b
    if rep is not None:
        assert rep.dirty == dirty and rep.bad_columns.tolist() == [int(b in dirty) for b in range(nstripes)]
        for b in dirty:
            assert rep.votes[b].tolist() == [int(j == b % rs.n) for j in range(rs.n)] and rep.unlocated[b] == 0


def case_edges(device, code, ncols=8192 + 3):
    """3. Stripe 1 of 3: one byte of chunk j flipped at column 0, 4095, 4096 and C - 1 (a tail-byte
    lane), for every j: exactly the bits {i : H[i][j] != 0} in that word of that row, nothing else."""
    rs = codec(code)
    stripes = batch_to_device(host_batch(code, 3, ncols), device)
    h = rs.H
    for j in range(rs.n):
        for c in (0, 4095, 4096, ncols - 1):
            stripes[1, j, c] ^= 0x5A
            mask = rs.syndrome_mask_batch(stripes, block_bytes=BB).cpu().numpy()
            want = np.zeros((3, -(-ncols // BB)), dtype=np.int64)
            for i in range(rs.p):
                if h[i, j]:
                    want[1, c // BB] |= 1 << (i % 32)
            assert np.array_equal(mask.astype(np.int64) & 0xFFFFFFFF, want), (j, c)
            stripes[1, j, c] ^= 0x5A
    assert not rs.syndrome_mask_batch(stripes, block_bytes=BB).cpu().numpy().any()


def case_chunks_overwritten(device, code, nstripes, ncols):
    """4. Two stripes with a different whole chunk replaced by random bytes: votes are the number of
    differing columns, and heal_batch restores the batch bit for bit."""
    rs = codec(code)
    good = host_batch(code, nstripes, ncols)
    bad = np.array(good)
    hits = {0: 1, nstripes - 1: rs.n - 1} if nstripes > 1 else {0: 1}  # stripe -> chunk
    for b, j in hits.items():
        bad[b, j] = np.random.default_rng(100 * b + ncols).integers(0, 256, size=ncols, dtype=np.uint8)
        assert (bad[b, j] != good[b, j]).any()
    stripes = batch_to_device(bad, device)
    rep = assert_batch_matches_oracle(code, stripes, bad, singles=stripes)
    assert rep.dirty == sorted(hits)
    for b, j in hits.items():
        differ = int((bad[b, j] != good[b, j]).sum())
        assert rep.votes[b, j] == differ == rep.bad_columns[b] and rep.unlocated[b] == 0
        assert rep.report[b].suspects == [j]
    healed = rs.heal_batch(stripes)
    assert healed.clean.all() and healed.dirty == [] and healed.unhealed == []
    assert not healed.mask.cpu().numpy().any() and not healed.votes.any()
    assert np.array_equal(stripes.cpu().numpy(), good)


def mixed_batch(code, ncols):
    """(good, bad) of 5 stripes: clean | one chunk damaged | two chunks at disjoint columns | two
    chunks wrong in the same columns (test_scrub's case_two_chunks_same_column) | p + 1 chunks, each
    damaged at a column of its own."""
    rs = codec(code)
    good = host_batch(code, 5, ncols)
    bad = np.array(good)
    bad[1, 2, 40:140] ^= 0x3C
    bad[2, 0, 5:105] ^= 0x11
    bad[2, rs.n - 1, 4090:4101] ^= 0xC3
    for t, c in enumerate([0, 16, 4095, 4096, ncols - 1]):
        bad[3, 0, c] ^= 1 + t
        bad[3, 1, c] ^= 0x80 >> t
    for t in range(rs.p + 1):
        bad[4, 2 * t, 100 * t + 7] ^= 0x21 + t
    return good, bad


def case_mixed_heal(device, code, ncols=4101):
    """5. heal_batch repairs what heal's rule admits and leaves the rest byte for byte as it was,
    listed in ``unhealed``; nothing is raised."""
    rs = codec(code)
    good, bad = mixed_batch(code, ncols)
    _, votes, unlocated, bad_columns = oracle_batch(code, bad, 65536)
    assert bad_columns.tolist() == [0, 100, 111, 5, rs.p + 1]
    assert unlocated.tolist() == [0, 0, 0, 5, 0] and not votes[3].any()  # same column: unlocated, no vote
    assert [int((v > 0).sum()) for v in votes] == [0, 1, 2, 0, rs.p + 1]
    stripes = batch_to_device(bad, device)
    first = assert_batch_matches_oracle(code, stripes, bad, 65536, singles=stripes)
    assert first.dirty == [1, 2, 3, 4]
    healed = rs.heal_batch(stripes)
    assert healed is not first and healed.unhealed == [3, 4] and healed.dirty == [3, 4]
    after = stripes.cpu().numpy()
    assert np.array_equal(after[:3], good[:3]) and np.array_equal(after[3:], bad[3:])
    assert_report_equal(healed.report[3], first.report[3])
    assert_report_equal(healed.report[4], first.report[4])
    # with the first report handed in, and nothing left to repair: that report comes back
    again = rs.heal_batch(stripes, report=healed)
    assert again is healed and again.unhealed == [3, 4]
    assert np.array_equal(stripes.cpu().numpy(), after)


def assert_same_batch_report(a, b, order=None):
    order = list(range(len(a.clean))) if order is None else order
    assert np.array_equal(a.clean, b.clean[order]) and np.array_equal(a.bad_columns, b.bad_columns[order])
    assert np.array_equal(a.unlocated, b.unlocated[order]) and np.array_equal(a.votes, b.votes[order])
    assert np.array_equal(a.mask.cpu().numpy(), b.mask.cpu().numpy()[order])


def case_input_forms(device, code, ncols=4101):
    """6. One batch as a [B, n, C] tensor, as row lists with the stripes in reverse, as natives and
    encode_batch's parity in two allocations, and as every second stripe of a larger tensor."""
    rs = codec(code)
    nstripes = 3
    bad = np.array(host_batch(code, nstripes, ncols))
    bad[1, 2, 100] ^= 0x40
    bad[1, rs.n - 1, 4096] ^= 0x01
    bad[2, rs.k, ncols - 1] ^= 0x80
    whole = batch_to_device(bad, device)
    ref = assert_batch_matches_oracle(code, whole, bad, singles=whole)
    ref_mask = rs.syndrome_mask_batch(whole, block_bytes=BB).cpu().numpy()

    lists = [[whole[b, j] for j in range(rs.n)] for b in reversed(range(nstripes))]
    rep = assert_batch_matches_oracle(code, lists, bad[::-1], singles=lists)
    assert_same_batch_report(rep, ref, order=[2, 1, 0])
    assert np.array_equal(rs.syndrome_mask_batch(lists, block_bytes=BB).cpu().numpy(), ref_mask[::-1])
    per_stripe = [whole[b] for b in range(nstripes)]  # a sequence of [n, C] tensors
    assert_same_batch_report(rs.scrub_batch(per_stripe, block_bytes=BB), ref)

    good = host_batch(code, nstripes, ncols)
    data = batch_to_device(good[:, : rs.k], device)
    parity = rs.encode_batch(data)
    assert parity.data_ptr() != data.data_ptr() and tuple(parity.shape) == (nstripes, rs.p, ncols)
    assert np.array_equal(parity.cpu().numpy(), good[:, rs.k:])
    assert not rs.syndrome_mask_batch(data, parity, BB).cpu().numpy().any()
    data[1, 2, 100] ^= 0x40
    parity[1, rs.p - 1, 4096] ^= 0x01
    parity[2, 0, ncols - 1] ^= 0x80
    singles = [[data[b, j] for j in range(rs.k)] + [parity[b, i] for i in range(rs.p)] for b in range(nstripes)]
    rep = assert_batch_matches_oracle(code, data, bad, parity=parity, singles=singles)
    assert_same_batch_report(rep, ref)
    assert np.array_equal(rs.syndrome_mask_batch(data, parity, BB).cpu().numpy(), ref_mask)
    healed = rs.heal_batch(data, parity)
    assert healed.clean.all() and healed.unhealed == []
    assert np.array_equal(data.cpu().numpy(), good[:, : rs.k]) and np.array_equal(parity.cpu().numpy(), good[:, rs.k:])

    wide = np.array(host_batch(code, 2 * nstripes, ncols))
    wide[::2] = bad
    wide[1::2, 0, 7] ^= 0xFF  # the stripes in between are dirty and must not be looked at
    every_second = batch_to_device(wide, device)[::2]
    assert every_second.stride(0) == 2 * whole.stride(0)
    rep = assert_batch_matches_oracle(code, every_second, bad, singles=every_second)
    assert_same_batch_report(rep, ref)


def case_unaligned(device, code, ncols):
    """7. One row of one stripe starts at an odd address (the whole batch takes the byte form): the
    oracle's results."""
    rs = codec(code)
    bad = np.array(host_batch(code, 3, ncols))
    bad[1, 1, ncols // 2] ^= 0x77
    bad[2, rs.n - 1, ncols - 1] ^= 0x01
    aligned = batch_to_device(bad, device)
    lists = [[aligned[b, j] for j in range(rs.n)] for b in range(3)]
    lists[1] = unaligned_rows(bad[1], device)
    assert sum(r.data_ptr() % 16 != 0 for rows in lists for r in rows) == 1
    for bb in (BB, 65536):
        rep = assert_batch_matches_oracle(code, lists, bad, bb, singles=lists)
        assert_same_batch_report(rep, rs.scrub_batch(aligned, block_bytes=bb))
    healed = rs.heal_batch(lists)
    assert healed.clean.all() and np.array_equal(stripe_bytes(lists[1]), host_batch(code, 3, ncols)[1])


def case_slice_boundary(device, code=(4, 6, "cauchy"), nstripes=65537, ncols=16):
    """8. More stripes than one launch's grid.y holds: a flipped byte in the last stripe of the first
    slice and one in the first stripe of the second. Masks only; rows of one tensor."""
    rs = codec(code)
    long = host_stripe(code, nstripes * ncols)
    assert not gf.GF256.gemm(rs.H, long).any()  # every stripe cut from it is consistent
    bad = np.array(host_batch(code, nstripes, ncols))
    hits = {65534: (1, 3), 65535: (5, 0), 65536: (2, 15)}  # stripe -> (chunk, column)
    for b, (j, c) in hits.items():
        bad[b, j, c] ^= 0x5A
    stripes = torch.from_numpy(bad).to(device)
    mask = rs.syndrome_mask_batch(stripes, block_bytes=BB)
    assert mask.dtype == torch.int32 and tuple(mask.shape) == (nstripes, 1)
    mask = mask.cpu().numpy()
    assert np.nonzero(mask[:, 0])[0].tolist() == sorted(hits)
    for b in hits:
        assert np.array_equal(mask[b], gf.scrub_oracle(rs.H, bad[b], BB)[0]), b


def case_refusals(device):
    """11. What the calls refuse, with the buffers unchanged after each refusal."""
    for field in ("gf16", "gf65536"):
        rs = ReedSolomon(4, 6, matrix="cauchy", field=field)
        stripes = torch.full((2, 6, 64), 7, dtype=torch.uint8, device=device)
        for call in (rs.syndrome_mask_batch, rs.scrub_batch, rs.heal_batch):
            with pytest.raises(NotImplementedError, match=field):
                call(stripes)
        assert (stripes == 7).all()
    code = (19, 36, "cauchy")  # p = 17
    host = host_batch(code, 2, 17)
    stripes = batch_to_device(host, device)
    for call in (codec(code).scrub_batch, codec(code).heal_batch):
        with pytest.raises(NotImplementedError, match="p = 17"):
            call(stripes)
    assert not codec(code).syndrome_mask_batch(stripes).cpu().numpy().any()
    assert np.array_equal(stripes.cpu().numpy(), host)

    code = (10, 14, "vandermonde")
    rs = codec(code)
    bad = np.array(host_batch(code, 3, 4101))
    bad[1, 3, 9] ^= 0x10
    stripes = batch_to_device(bad, device)
    lists = [[stripes[b, j] for j in range(rs.n)] for b in range(3)]
    short = [list(rows) for rows in lists]
    short[2][5] = short[2][5][:4100]  # unequal row lengths
    fewer = [list(rows) for rows in lists]
    del fewer[1][13]  # a stripe of n - 1 rows
    elsewhere = [list(rows) for rows in lists]
    elsewhere[0][4] = torch.zeros(4101, dtype=torch.uint8, device="cpu" if torch.device(device).type != "cpu" else "meta")
    wrong = [short, fewer, elsewhere, stripes[:, :13], stripes[:, :, :4100].to(torch.int8), stripes[0],
             [[[1, 2, 3]] * rs.n], [stripes[0, :, 0]]]
    for arg in wrong:
        for call in (rs.syndrome_mask_batch, rs.scrub_batch, rs.heal_batch):
            with pytest.raises(ValueError):
                call(arg)
    data, parity = stripes[:, : rs.k], stripes[:, rs.k:]
    for d, p in ((data, parity[:2]), (data, parity[:, :3]), (data[:, :9], parity), (data, parity[:, :, :4100]),
                 (stripes, parity)):
        for call in (rs.syndrome_mask_batch, rs.scrub_batch, rs.heal_batch):
            with pytest.raises(ValueError):
                call(d, p)
    for bb in (0, 2048, 4097, 3 * 4096):
        with pytest.raises(ValueError):
            rs.syndrome_mask_batch(stripes, block_bytes=bb)
        with pytest.raises(ValueError):
            rs.scrub_batch(stripes, block_bytes=bb)
    assert np.array_equal(stripes.cpu().numpy(), bad)
    assert rs.scrub_batch(stripes).dirty == [1]


def case_trivial(device):
    """p = 0: all-zero results. B = 0: empty ones."""
    rs = ReedSolomon(4, 4)
    stripes = torch.full((3, 4, 5000), 9, dtype=torch.uint8, device=device)
    mask = rs.syndrome_mask_batch(stripes, block_bytes=BB)
    assert mask.dtype == torch.int32 and tuple(mask.shape) == (3, 2) and not mask.cpu().numpy().any()
    assert mask.device == stripes.device
    rep = rs.scrub_batch(stripes, block_bytes=BB)
    assert rep.clean.tolist() == [True] * 3 and rep.dirty == [] and rep.votes.shape == (3, 4) and not rep.votes.any()
    assert rs.heal_batch(stripes).clean.all()
    rs = codec((10, 14, "vandermonde"))
    for empty in (torch.zeros((0, 14, 4101), dtype=torch.uint8, device=device), []):
        mask = rs.syndrome_mask_batch(empty, block_bytes=BB)
        assert mask.dtype == torch.int32 and mask.shape[0] == 0 and mask.numel() == 0
        rep = rs.scrub_batch(empty, block_bytes=BB)
        assert rep.clean.shape == (0,) and rep.votes.shape == (0, 14) and rep.dirty == [] and len(rep.report) == 0
        assert rs.heal_batch(empty).unhealed == []
    assert tuple(rs.syndrome_mask_batch(torch.zeros((0, 14, 4101), dtype=torch.uint8, device=device),
                                        block_bytes=BB).shape) == (0, 2)


# ---- the CPU tests ------------------------------------------------------------------------------------
CLEAN_RUNS = runs_of(CODES)
IDENTITY_RUNS = [(c, b, s, w) for c, b, s in runs_of(CODES) for w in ("first", "last")
                 if c[1] <= 14 or (b, s) in ((257, 17), (3, 17), (3, 4101))]


def identity_id(r):
    return f"{run_id(r)}-{r[3]}"


@pytest.mark.parametrize("code,nstripes,ncols", CLEAN_RUNS, ids=map(run_id, CLEAN_RUNS))
def test_clean_batch(code, nstripes, ncols):
    case_clean("cpu", code, nstripes, ncols)


def test_clean_batch_with_64k_blocks():
    case_clean("cpu", (10, 14, "vandermonde"), 3, 8192 + 3, 65536)


@pytest.mark.parametrize("code,nstripes,ncols,which", IDENTITY_RUNS, ids=map(identity_id, IDENTITY_RUNS))
def test_stripe_identity(code, nstripes, ncols, which):
    case_stripe_identity("cpu", code, nstripes, ncols, which)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (19, 36, "cauchy")], ids=code_id)
def test_block_and_tile_edges(code):
    case_edges("cpu", code)


@pytest.mark.parametrize("nstripes,ncols", [(1, 17), (2, 15), (3, 4101), (257, 17)])
@pytest.mark.parametrize("code", LOCATING, ids=code_id)
def test_whole_chunks_overwritten_and_healed(code, nstripes, ncols):
    case_chunks_overwritten("cpu", code, nstripes, ncols)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (10, 14, "cauchy")], ids=code_id)
def test_mixed_heal(code):
    case_mixed_heal("cpu", code)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (9, 14, "cauchy")], ids=code_id)
def test_input_forms(code):
    case_input_forms("cpu", code)


@pytest.mark.parametrize("ncols", [15, 4101])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (9, 14, "cauchy")], ids=code_id)
def test_unaligned_rows(code, ncols):
    case_unaligned("cpu", code, ncols)


def test_slice_boundary_at_65537_stripes():
    case_slice_boundary("cpu")


def test_refusals():
    case_refusals("cpu")


def test_trivial_batches():
    case_trivial("cpu")

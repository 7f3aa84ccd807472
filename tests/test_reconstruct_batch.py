"""Batched repair on CPU tensors: ``ReedSolomon.reconstruct_batch`` against the numpy oracle
(``gf.reconstruct_oracle``, stripe by stripe) and against a loop of single ``reconstruct`` calls on
copies of the same buffers, exactly. The case functions take the device, so
tests/test_gpu_reconstruct_batch.py runs the same cases through the gfx950 kernel
(``csrc/kernels/gf_repair.hip``), where every stripe picks coefficient tables of its own."""
import itertools
import time
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_update as cases
import test_update_batch as ub
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import cpu
from gpu_rscode_amd.models.rs import UnrecoverableError
from gpu_rscode_amd.ops import BatchRepairPlan
from gpu_rscode_amd.ops.repair import check_repair_overlap, repair_batch_layout, repair_rows
from gpu_rscode_amd.ops.rows import StripeBatch

# (code, erasures per stripe): m_pad 1 | m_pad 2 | e = 3 padded to 4 | e = 5, two tiles | e = 17, padded tile
NARROW = [((4, 6, "cauchy"), 1), ((4, 6, "cauchy"), 2), ((10, 14, "cauchy"), 3), ((5, 10, "cauchy"), 5),
          ((19, 36, "cauchy"), 17)]
WIDE = [((128, 160, "cauchy"), 1), ((128, 160, "cauchy"), 32)]
# a lone tail byte | no group, 15 tail lanes | one group | a group and a tail byte | a block edge plus tail
SHAPES = [1, 15, 16, 17, 4101]
BIG = 65536 + 3  # past 64 KiB
BATCHES = [1, 2, 257]  # (3 runs with every shape)
RUNS = [(c, e, 3, s) for c, e in NARROW for s in SHAPES] + [(c, e, 2, BIG) for c, e in NARROW] \
    + [(c, e, b, 17) for c, e in NARROW for b in BATCHES] + [(c, e, b, 4101) for c, e in NARROW[:3] for b in BATCHES] \
    + [(c, e, 3, s) for c, e in WIDE for s in (17, 273)]


def run_id(r):
    return f"{cases.code_id(r[0])}-e{r[1]}-B{r[2]}-C{r[3]}"


def spread_patterns(n: int, nstripes: int, lo: int, hi: int, seed: int = 0) -> list[tuple]:
    """An erasure list per stripe, ``lo..hi`` distinct ids each, unsorted, natives and parity mixed; stripe
    b's first id is ``b % n``, and no list is repeated while the code has one left."""
    rng = np.random.default_rng(1000 * n + 10 * hi + seed)
    seen, out = set(), []
    for b in range(nstripes):
        for _ in range(50):
            e = lo + (b + int(rng.integers(0, hi - lo + 1))) % (hi - lo + 1)
            rest = [int(j) for j in rng.permutation(n) if j != b % n]
            ids = tuple([b % n] + rest[: e - 1]) if e else ()
            if tuple(sorted(ids)) not in seen:
                break
        seen.add(tuple(sorted(ids)))
        out.append(ids)
    return out


@lru_cache(maxsize=None)
def damaged(code, nstripes: int, ncols: int, erased: tuple, extra: tuple = ()) -> np.ndarray:
    """``ub.host_batch`` with the rows ``erased[b]`` of stripe b (and rows ``extra = ((b, row), ...)``)
    overwritten with noise; shared, never modified."""
    out = np.array(ub.host_batch(code, nstripes, ncols))
    rng = np.random.default_rng(17 * nstripes + ncols + len(erased))
    for b, ids in enumerate(erased):
        for i in ids:
            out[b, i] = rng.integers(0, 256, size=ncols, dtype=np.uint8)
    for b, i in extra:
        out[b, i] ^= rng.integers(1, 256, size=ncols, dtype=np.uint8)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def expected(code, nstripes: int, ncols: int, erased: tuple, extra: tuple = ()) -> np.ndarray:
    """``gf.reconstruct_oracle`` stripe by stripe on the damaged batch. Where only erased rows were
    damaged that is the consistent batch again: asserted, so the oracle is itself cross-checked."""
    bad, g = damaged(code, nstripes, ncols, erased, extra), cases.codec(code).G
    out = np.stack([gf.reconstruct_oracle(g, bad[b], erased[b]) for b in range(nstripes)])
    if not extra:
        assert np.array_equal(out, ub.host_batch(code, nstripes, ncols))
    out.setflags(write=False)
    return out


def as_tuples(erased) -> tuple:
    return tuple(tuple(int(i) for i in ids) for ids in erased)


def assert_recoverable(code, erased):
    """On the CPU: every pattern used is recoverable (cauchy codes are MDS, so all are)."""
    rs, (k, n, _) = cases.codec(code), code
    for ids in set(as_tuples(erased)):
        assert rs.is_recoverable([i for i in range(n) if i not in ids][:k]), ids


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_repair(device, code, nstripes, ncols, erased, shift=0, arg=None, extra=(), rs=None):
    """``reconstruct_batch(stripes, arg or erased)``: every stripe equals the oracle's, the pitch
    padding and every row not named are byte for byte what they were, and a loop of single
    ``reconstruct`` calls on a copy gives the same bytes. Returns the repaired tensor."""
    rs = rs or cases.codec(code)
    erased = as_tuples(erased)
    if device == "cpu":
        assert_recoverable(code, erased)
    bad, want = damaged(code, nstripes, ncols, erased, extra), expected(code, nstripes, ncols, erased, extra)
    for b, ids in enumerate(erased):  # (the oracle leaves rows not named alone: so must the call)
        keep = [i for i in range(code[1]) if i not in ids]
        assert np.array_equal(want[b, keep], bad[b, keep])
    sf, stripes = ub.to_batch(bad, device, shift)
    assert rs.reconstruct_batch(stripes, [list(ids) for ids in erased] if arg is None else arg) is stripes
    ub.assert_batch(stripes, want, "reconstruct_batch")
    cases.assert_padding(sf)
    lf, loop = ub.to_batch(bad, device, shift)
    for b, ids in enumerate(erased):
        rs.reconstruct(loop[b], list(ids))
    assert torch.equal(loop, stripes), "batch differs from a loop of single calls"
    return stripes


def case_every_stripe_its_own_pattern(device, nstripes=257, ncols=273):
    """(10, 14) has 1,470 patterns of 1..4 erasures: 257 stripes, 257 distinct ones, all four lengths."""
    code = (10, 14, "cauchy")
    every = [c for e in range(1, 5) for c in itertools.combinations(range(14), e)]
    assert len(every) == 1470
    order = np.random.default_rng(1470).permutation(len(every))[:nstripes]
    erased = tuple(every[int(i)] for i in order)
    assert len(set(erased)) == nstripes and {len(e) for e in erased} == {1, 2, 3, 4}
    case_repair(device, code, nstripes, ncols, erased)


def case_shared_list(device, code=(10, 14, "cauchy"), nstripes=4, ncols=4101):
    """A flat list gives what the same list repeated B times gives; ids are sorted and deduplicated."""
    shared = (12, 1, 9)
    for form in ([12, 1, 9], (12, 1, 9), np.array([12, 1, 9]), torch.tensor([9, 12, 1, 12]), [[12, 1, 9]] * nstripes,
                 np.tile(np.array([1, 9, 12, -1]), (nstripes, 1))):
        case_repair(device, code, nstripes, ncols, [shared] * nstripes, arg=form)


def case_kinds(device, code=(10, 14, "cauchy"), ncols=4101):
    """Natives only, parity only, and mixed, in one batch."""
    case_repair(device, code, 3, ncols, [(0, 3, 9), (10, 13), (2, 11, 12, 5)])


def case_mixed_lengths(device, code=(10, 14, "cauchy"), ncols=4101):
    """0..p erasures in one batch; the stripes with an empty list are corrupt (``extra``) and stay exactly
    so. The -1-padded array forms equal the ragged list form."""
    erased = [(), (13,), (4, 0), (9, 10, 1), (12, 3, 7, 11), ()]
    extra = ((0, 2), (5, 13))
    got = case_repair(device, code, 6, ncols, erased, extra=extra)
    arr = np.full((6, 5), -1, dtype=np.int64)
    for b, ids in enumerate(erased):
        arr[b, 5 - len(ids):] = ids  # (padding first, ids unsorted: the order does not matter)
    for form in (arr, arr.astype(np.int32), torch.from_numpy(arr), torch.from_numpy(arr.astype(np.int32)),
                 np.concatenate([arr, arr[:, -1:]], axis=1)):
        assert torch.equal(case_repair(device, code, 6, ncols, erased, arg=form, extra=extra), got)


def case_stripe_identity(device, nstripes, which, code=(10, 14, "cauchy"), ncols=4101):
    """One stripe of the batch is corrupt in chunk ``which % n``; every stripe b repairs chunk ``b % n``.
    Only that stripe changes: the batch is the consistent one again."""
    n = code[1]
    host = ub.host_batch(code, nstripes, ncols)
    bad = np.array(host)
    bad[which, which % n] ^= 0x5A
    sf, stripes = ub.to_batch(bad, device)
    cases.codec(code).reconstruct_batch(stripes, np.arange(nstripes)[:, None] % n)
    ub.assert_batch(stripes, host, f"stripe {which} of {nstripes}")
    cases.assert_padding(sf)


def case_round_trip(device, code, nstripes=257, ncols=273):
    """encode_batch, overwrite chunk b % n of stripe b, reconstruct_batch: the syndrome (existing code,
    independent of the repair) is all zero and the natives are the originals, in both stripe forms."""
    rs, (k, n, _) = cases.codec(code), code
    data = np.array(ub.host_batch(code, nstripes, ncols)[:, :k])
    ids = np.arange(nstripes)[:, None] % n
    # natives and parity= in allocations of their own
    df, nat = ub.to_batch(data, device)
    pf, par = ub.to_batch(np.zeros((nstripes, n - k, ncols), dtype=np.uint8), device)
    rs.encode_batch(nat, par)
    # one [B, n, C] tensor
    sf, stripes = ub.to_batch(np.zeros((nstripes, n, ncols), dtype=np.uint8), device)
    stripes[:, :k].copy_(nat)
    stripes[:, k:].copy_(par)
    noise = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(nstripes, ncols), dtype=np.uint8)).to(device)
    for b in range(nstripes):
        i = b % n
        stripes[b, i].copy_(noise[b])
        (nat[b, i] if i < k else par[b, i - k]).copy_(noise[b])
    assert rs.syndrome_mask_batch(stripes, block_bytes=4096).cpu().numpy().any(axis=1).all()
    assert rs.reconstruct_batch(stripes, ids) is stripes
    assert not rs.syndrome_mask_batch(stripes, block_bytes=4096).cpu().numpy().any()
    ub.assert_batch(stripes[:, :k], data, "natives, one tensor")
    assert rs.reconstruct_batch(nat, ids, parity=par) is nat
    assert not rs.syndrome_mask_batch(nat, par, block_bytes=4096).cpu().numpy().any()
    ub.assert_batch(nat, data, "natives, parity=")
    assert torch.equal(par, stripes[:, k:])
    cases.assert_padding(df, pf, sf)


def case_gf16(device, ncols=4101, nstripes=3):
    """A GF(16) code agrees with its own single ``reconstruct`` and gives the encoded stripes back."""
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf16")
    data = np.random.default_rng(16).integers(0, 256, size=(nstripes, 4, ncols), dtype=np.uint8)
    sf, stripes = ub.to_batch(np.zeros((nstripes, 6, ncols), dtype=np.uint8), device)
    stripes[:, :4].copy_(torch.from_numpy(data))
    for b in range(nstripes):
        rs.encode(stripes[b, :4], stripes[b, 4:])
    good = stripes.clone()
    erased = [(1, 4), (5,), (0, 3)]
    for b, ids in enumerate(erased):
        for i in ids:
            stripes[b, i].fill_(0xC3)
    loop = stripes.clone()
    rs.reconstruct_batch(stripes, erased)
    for b, ids in enumerate(erased):
        rs.reconstruct(loop[b], list(ids))
    assert torch.equal(stripes, loop) and torch.equal(stripes, good)
    cases.assert_padding(sf)


def case_one_unaligned_row(device, code=(10, 14, "cauchy"), nstripes=3, ncols=4101):
    """Stripes as lists of rows, one survivor row of one stripe a byte off a 16-byte boundary: the result is
    unchanged. Returns the codec (of its own) for a look at its plan."""
    rs = ReedSolomon(*code[:2], matrix=code[2])
    erased = as_tuples([(0, 11), (13,), (5, 6, 7)])
    bad, want = damaged(code, nstripes, ncols, erased), expected(code, nstripes, ncols, erased)
    sf, stripes = ub.to_batch(bad, device)
    off = cases.to_device(bad[1, 2:3], device, shift=1)
    rows = [[stripes[b, i] for i in range(code[1])] for b in range(nstripes)]
    rows[1][2] = off[0]
    assert rs.reconstruct_batch(rows, [list(e) for e in erased]) is rows
    ub.assert_batch(stripes, want)
    cases.assert_rows(off, bad[1, 2:3])
    cases.assert_padding(sf, off)
    return rs


@lru_cache(maxsize=None)
def singular_pattern():
    """Four erased ids of the (10, 14) reference Vandermonde code whose survivors are singular: the
    complement of the first of its 12 singular survivor sets."""
    rs = cases.codec((10, 14, "vandermonde"))
    bad = gf.GF256.singular_patterns(rs.G, 10)
    assert len(bad) == 12
    return tuple(i for i in range(14) if i not in bad[0])


def case_refusals(device):
    """Each refusal is raised before a byte is written."""
    code, nstripes, ncols = (10, 14, "cauchy"), 3, 273
    rs, host = cases.codec(code), ub.host_batch(code, 3, 273)
    sf, stripes = ub.to_batch(host, device)

    def refused(exc, match, *args, codec=rs, **kw):
        with pytest.raises(exc, match=match):
            codec.reconstruct_batch(*args, **kw)
        ub.assert_batch(stripes, host, match)
        cases.assert_padding(sf)

    for bad in ([14], [-2], [[0], [1], [14]], [[0], [-1, -2], [1]], np.array([[0], [1], [-2]]), [0.5], "ab",
                np.zeros((3, 1, 1), dtype=np.int64)):
        refused(ValueError, "erased", stripes, bad)
    refused(ValueError, "stripe 2", stripes, [[0], [], [3, 14]])
    refused(ValueError, "3 stripes", stripes, [[0], [1]])  # a wrong B
    refused(ValueError, "3 stripes", stripes, np.zeros((4, 1), dtype=np.int64))
    refused(UnrecoverableError, "stripe 1 has 5 erasures", stripes, [[0], [1, 2, 3, 4, 13], [2]])
    refused(UnrecoverableError, "more than p=4", stripes, [0, 1, 2, 3, 4])
    if device != "cpu":
        refused(ValueError, "CPU tensor", stripes, torch.zeros((3, 1), dtype=torch.int64, device=device))
    # a singular pattern of the reference Vandermonde code: the error names the stripe
    vand, sing = cases.codec((10, 14, "vandermonde")), singular_pattern()
    assert not vand.is_recoverable([i for i in range(14) if i not in sing])
    refused(UnrecoverableError, "stripe 2 cannot be repaired", stripes, [[0], [], list(sing)], codec=vand)
    # a stripe listed twice with something to write; written nowhere, it is no aliasing
    twice = [stripes[0], stripes[1], stripes[0]]
    refused(ValueError, "overlap", twice, [[3], [4], [5]])
    refused(ValueError, "overlap", twice, [[3], [4], [3]])
    rs.reconstruct_batch(twice, [[3], [4], []])
    ub.assert_batch(stripes, host)
    # a written row that is another stripe's survivor row
    flat = sf  # [3 * 14, C]: stripe 1 shifted down by one row shares 13 rows with stripe 0
    chained = [[flat[i] for i in range(14)], [flat[i] for i in range(13, 27)]]
    refused(ValueError, "overlap", chained, [[13], [5]])
    # rows: wrong counts, ragged lengths, not uint8, natives without parity
    refused(ValueError, "n=14", stripes[:, :13], [0])
    refused(ValueError, "rows", stripes[:, :10], [0], parity=stripes[:, 10:13])
    ragged = [[stripes[b, i] for i in range(14)] for b in range(3)]
    ragged[2][5] = ragged[2][5][:-1]
    refused(ValueError, "one length", ragged, [0])
    refused(ValueError, "uint8", torch.zeros((3, 14, 16), dtype=torch.int8, device=device), [0])
    refused(ValueError, "tensor", [0, 1, 2], [0])


def case_nothing_to_do(device):
    """B == 0, p == 0 with only empty lists, and all-empty lists return at once."""
    rs = cases.codec((10, 14, "cauchy"))
    empty = torch.zeros((0, 14, 64), dtype=torch.uint8, device=device)
    for er in ([], [3], np.zeros((0, 2), dtype=np.int64)):
        assert rs.reconstruct_batch(empty, er) is empty
    host = ub.host_batch((10, 14, "cauchy"), 3, 273)
    sf, stripes = ub.to_batch(host, device)
    before = len(rs._plans)
    for er in ([], [[], [], []], np.full((3, 2), -1), np.zeros((3, 0), dtype=np.int64)):
        assert rs.reconstruct_batch(stripes, er) is stripes
    assert len(rs._plans) == before
    ub.assert_batch(stripes, host)
    flat = ReedSolomon(4, 4)
    rows = torch.full((2, 4, 64), 7, dtype=torch.uint8, device=device)
    assert flat.reconstruct_batch(rows, [[], []]) is rows and flat.reconstruct_batch(rows, []) is rows
    with pytest.raises(UnrecoverableError):
        flat.reconstruct_batch(rows, [1])
    assert bool((rows == 7).all())


# ---- the cases on CPU tensors ----------------------------------------------------------------------
@pytest.mark.parametrize("code,e,nstripes,ncols", RUNS, ids=map(run_id, RUNS))
def test_codes_batches_and_row_lengths(code, e, nstripes, ncols):
    case_repair("cpu", code, nstripes, ncols, spread_patterns(code[1], nstripes, e, e))


def test_every_stripe_with_a_pattern_of_its_own():
    case_every_stripe_its_own_pattern("cpu")


def test_shared_list_equals_the_list_repeated():
    case_shared_list("cpu")


def test_natives_only_parity_only_and_mixed():
    case_kinds("cpu")


def test_mixed_lengths_and_the_padded_array_form():
    case_mixed_lengths("cpu")


@pytest.mark.parametrize("which", [0, 128, 256])
def test_stripe_identity(which):
    case_stripe_identity("cpu", 257, which)


@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "cauchy")], ids=cases.code_id)
def test_round_trip(code):
    case_round_trip("cpu", code)


def test_gf16_agrees_with_its_own_reconstruct():
    case_gf16("cpu")


def test_gf65536_loops_over_the_stripes():
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf65536")
    data = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(3, 4, 64), dtype=np.uint8))
    stripes = torch.zeros((3, 6, 64), dtype=torch.uint8)
    stripes[:, :4] = data
    for b in range(3):
        rs.encode(stripes[b, :4], stripes[b, 4:])
    good = stripes.clone()
    stripes[0, 5], stripes[1, 0], stripes[1, 4], stripes[2, 2] = 1, 2, 3, 4
    rs.reconstruct_batch(stripes, [[5], [0, 4], [2]])
    assert torch.equal(stripes, good)
    with pytest.raises(ValueError, match="even"):
        rs.reconstruct_batch(stripes[:, :, :63], [1])
    assert torch.equal(stripes, good)


def test_unaligned_rows():
    case_one_unaligned_row("cpu")
    code = (10, 14, "cauchy")
    case_repair("cpu", code, 3, 4101, spread_patterns(14, 3, 1, 4, seed=1), shift=1)


def test_refusals():
    case_refusals("cpu")


def test_nothing_to_do():
    case_nothing_to_do("cpu")


def test_oracle_is_the_generator_identity():
    """reconstruct_oracle on a consistent stripe changes nothing, whatever is erased, and refuses what
    cannot be solved."""
    code = (10, 14, "cauchy")
    host, g = cases.host_stripe(code, 273), cases.codec(code).G
    for erased in ([], [0], [13, 0, 13], [10, 11, 12, 13], [3, 4, 5, 12]):
        noisy = np.array(host)
        noisy[sorted(set(erased))] ^= 0xFF
        assert np.array_equal(gf.reconstruct_oracle(g, noisy, erased), host)
    with pytest.raises(ValueError):
        gf.reconstruct_oracle(g, host, [0, 1, 2, 3, 4])
    with pytest.raises(gf.SingularMatrixError):
        gf.reconstruct_oracle(cases.codec((10, 14, "vandermonde")).G, host, singular_pattern())


def test_layout_mirror_and_plan_is_gpu_only():
    for args in ((4, 1, 1, 1), (10, 4, 7, 3), (128, 32, 257, 257), (4, 2, 65537, 6), (19, 32, 3, 2)):
        assert dict(cpu().repair_batch_layout(*args)) == repair_batch_layout(*args)
    rows = torch.zeros((2, 6, 64), dtype=torch.uint8)
    pattern = ((1, 2, 3, 4), (0,), np.ones((1, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="GPU"):
        BatchRepairPlan(rows, [0, 0], [pattern])
    for pat, patterns in (([0], [pattern]), ([0, 1], [pattern]), ([0, 0], []), ([0, 0], [pattern, ((1, 2, 3), (0,), None)]),
                          ([0, 0], [((1, 2, 3, 0), (0,), None)]), ([0, 0], [((1, 2, 3, 4), (6,), None)]),
                          ([0, 0], [((1, 2, 3, 4), (), None)])):
        with pytest.raises(ValueError):
            BatchRepairPlan(rows, pat, patterns)


def test_a_batch_of_65537_stripes_builds_without_a_loop_over_rows():
    """Patterns, row addresses and aliasing of a tensor-form batch of 65,537 stripes with a pattern each:
    numpy on the pointer arrays, well under a second."""
    nstripes = 65537
    rs = ReedSolomon(4, 6, matrix="cauchy")
    t = torch.zeros((nstripes, 6, 32), dtype=torch.uint8)
    ids = np.stack([np.arange(nstripes) % 6, np.where(np.arange(nstripes) % 3 == 0, -1, (np.arange(nstripes) + 1) % 6)],
                   axis=1)
    t0 = time.perf_counter()
    batch = StripeBatch(t[:, :, :17], 6)
    pat, patterns = rs._erased_patterns(rs._erased_raw(ids, 6), nstripes)
    ins, outs = repair_rows(batch.ptrs(), pat, [(sv, er, None) for sv, er in patterns], 2)
    check_repair_overlap(ins, outs, 17)
    took = time.perf_counter() - t0
    assert took < 1.0, took
    assert ins.shape == (nstripes, 4) and outs.shape == (nstripes, 2) and len(patterns) == 6
    assert (outs[::3, 1] == 0).all() and outs[:, 0].all()
    outs[65536] = outs[6]  # the same stripe listed twice
    with pytest.raises(ValueError, match="overlap"):
        check_repair_overlap(ins, outs, 17)

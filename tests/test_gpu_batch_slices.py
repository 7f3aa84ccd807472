"""A batch past the grid.y limit on the MI355X: 65,537 stripes of the (4, 6) code, 17 byte columns each,
so every batched launcher of the scrub family (syndrome, locate, correct, checked, checked fix) runs
as two launches, of 65,535 stripes and of 2, and its second launch must find the rows, mask words and
counts of its own first stripe. One wrong byte in each of stripes 0, 65,534, 65,535 and 65,536 (the
first stripe, the last two of the first launch, the only damaged one of the second), in four chunks,
one of them a parity chunk and one byte in the tail column. The four damaged stripes are compared
with the numpy oracles, every other stripe's mask and counts with zero in one comparison.

Two layouts of the one tensor: rows 17 bytes apart (6.7 MB, rows at every alignment: the byte form of
the kernels) and 32 bytes apart (every row 16-byte aligned: one 16-byte group and one tail byte)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_reconstruct_checked as checked
from gpu_rscode_amd import gf
from test_scrub import codec
from test_scrub_batch import host_batch

pytestmark = pytest.mark.gpu

CODE = (4, 6, "cauchy")
NSTRIPES, NCOLS, BB = 65537, 17, 4096
HITS = {0: (1, 5, 0x33), 65534: (3, 16, 0x5A), 65535: (5, 0, 0x01), 65536: (2, 9, 0x80)}  # stripe: chunk, column, xor
ERASED = [0]  # for the checked repair: not among the damaged chunks
PITCHES = [17, 32]


@lru_cache(maxsize=None)
def hosts():
    """(good, bad, others): the clean batch, the damaged one (both read-only) and the clean stripes' index."""
    good = np.ascontiguousarray(host_batch(CODE, NSTRIPES, NCOLS))
    bad = good.copy()
    for b, (j, c, v) in HITS.items():
        bad[b, j, c] ^= v
    others = np.ones(NSTRIPES, dtype=bool)
    others[list(HITS)] = False
    for a in (good, bad, others):
        a.setflags(write=False)
    assert sorted({j for j, _, _ in HITS.values()}) == [1, 2, 3, 5] and NCOLS - 1 in {c for _, c, _ in HITS.values()}
    return good, bad, others


def on_device(host: np.ndarray, pitch: int) -> torch.Tensor:
    """[B, n, C] on the GPU with rows ``pitch`` bytes apart; the padding holds 0xA5."""
    b, n, c = host.shape
    store = torch.full((b, n, pitch), 0xA5, dtype=torch.uint8, device="cuda")
    view = store[:, :, :c]
    view.copy_(torch.from_numpy(np.array(host)))
    assert view.stride() == (n * pitch, pitch, 1)
    return view


@pytest.mark.parametrize("pitch", PITCHES)
def test_scrub_batch_past_the_grid_limit(pitch):
    rs = codec(CODE)
    good, bad, others = hosts()
    stripes = on_device(bad, pitch)
    mask = rs.syndrome_mask_batch(stripes, block_bytes=BB)
    assert mask.dtype == torch.int32 and tuple(mask.shape) == (NSTRIPES, 1)
    rep = rs.scrub_batch(stripes, block_bytes=BB)
    got_mask, rep_mask = mask.cpu().numpy(), rep.mask.cpu().numpy()
    for b in HITS:
        want_mask, votes, unlocated, nbad = gf.scrub_oracle(rs.H, bad[b], BB)
        assert np.array_equal(got_mask[b], want_mask) and np.array_equal(rep_mask[b], want_mask), b
        assert np.array_equal(rep.votes[b], votes) and (rep.unlocated[b], rep.bad_columns[b]) == (unlocated, nbad), b
        assert nbad == 1 and want_mask.any()
    assert not got_mask[others].any() and not rep_mask[others].any()
    assert not rep.votes[others].any() and not rep.unlocated[others].any() and not rep.bad_columns[others].any()
    assert rep.dirty == sorted(HITS)
    assert np.array_equal(stripes.cpu().numpy(), bad)


@pytest.mark.parametrize("pitch", PITCHES)
def test_correct_batch_past_the_grid_limit(pitch):
    rs = codec(CODE)
    good, bad, others = hosts()
    stripes = on_device(bad, pitch)
    rep = rs.correct_batch(stripes, max_errors=1, block_bytes=BB)
    rep_mask = rep.mask.cpu().numpy()
    now = stripes.cpu().numpy()
    for b in HITS:
        rows, fixed, by_weight, unc, nbad = gf.correct_oracle(rs.H, bad[b], 1)
        assert np.array_equal(rep_mask[b], gf.scrub_oracle(rs.H, bad[b], BB)[0]), b
        assert np.array_equal(rep.fixed_bytes[b], fixed) and np.array_equal(rep.by_weight[b], by_weight), b
        assert (rep.uncorrectable[b], rep.bad_columns[b]) == (unc, nbad) == (0, 1), b
        assert np.array_equal(now[b], rows), b
    assert not rep_mask[others].any() and not rep.fixed_bytes[others].any() and not rep.by_weight[others].any()
    assert not rep.uncorrectable[others].any() and not rep.bad_columns[others].any()
    assert rep.dirty == sorted(HITS)
    assert np.array_equal(now, good)


@pytest.mark.parametrize("pitch", PITCHES)
def test_reconstruct_checked_batch_past_the_grid_limit(pitch):
    rs = codec(CODE)
    good, bad, others = hosts()
    work = bad.copy()
    work[:, ERASED] = 0xC3  # the erased rows are outputs, never inputs
    stripes = on_device(work, pitch)
    rep = rs.reconstruct_checked_batch(stripes, ERASED, max_errors=1, block_bytes=BB)
    rep_mask = rep.mask.cpu().numpy()
    now = stripes.cpu().numpy()
    for b in HITS:
        checked.assert_report(rep.report[b], checked.oracle(rs.H, work[b], ERASED, 1, BB), now[b])
        assert rep.bad_columns[b] == 1, b
    assert not rep_mask[others].any() and not rep.fixed_bytes[others].any() and not rep.by_weight[others].any()
    assert not rep.uncorrectable[others].any() and not rep.bad_columns[others].any()
    assert rep.dirty == sorted(HITS)
    assert np.array_equal(now[others], good[others])

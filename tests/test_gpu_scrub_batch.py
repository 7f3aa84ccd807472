"""Batched scrub on the MI355X (the BATCH instantiations of csrc/kernels/gf_scrub.hip): the cases of
tests/test_scrub_batch.py on CUDA tensors, every result compared exactly with the numpy oracle
(``gf.scrub_oracle``) stripe by stripe and with the single-stripe ``scrub`` on the same buffers; then
the batched launchers called directly."""
import numpy as np
import pytest
import torch

import test_scrub_batch as cases
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import BatchScrubPlan, BatchScrubReport
from test_scrub import code_id, codec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("code,nstripes,ncols", cases.CLEAN_RUNS, ids=map(cases.run_id, cases.CLEAN_RUNS))
def test_clean_batch(code, nstripes, ncols):
    cases.case_clean("cuda", code, nstripes, ncols)


def test_clean_batch_with_64k_blocks():
    cases.case_clean("cuda", (10, 14, "vandermonde"), 3, 8192 + 3, 65536)


@pytest.mark.parametrize("code,nstripes,ncols,which", cases.IDENTITY_RUNS,
                         ids=map(cases.identity_id, cases.IDENTITY_RUNS))
def test_stripe_identity(code, nstripes, ncols, which):
    cases.case_stripe_identity("cuda", code, nstripes, ncols, which)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (19, 36, "cauchy")], ids=code_id)
def test_block_and_tile_edges(code):
    cases.case_edges("cuda", code)


@pytest.mark.parametrize("nstripes,ncols", [(1, 17), (2, 15), (3, 4101), (257, 17)])
@pytest.mark.parametrize("code", cases.LOCATING, ids=code_id)
def test_whole_chunks_overwritten_and_healed(code, nstripes, ncols):
    cases.case_chunks_overwritten("cuda", code, nstripes, ncols)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (10, 14, "cauchy")], ids=code_id)
def test_mixed_heal(code):
    cases.case_mixed_heal("cuda", code)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (9, 14, "cauchy")], ids=code_id)
def test_input_forms(code):
    cases.case_input_forms("cuda", code)


@pytest.mark.parametrize("ncols", [15, 4101])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (9, 14, "cauchy")], ids=code_id)
def test_unaligned_rows(code, ncols):
    cases.case_unaligned("cuda", code, ncols)


def test_one_unaligned_row_puts_the_whole_batch_on_the_byte_form():
    code = (10, 14, "vandermonde")
    rs = codec(code)
    host = cases.host_batch(code, 3, 4101)
    aligned = cases.batch_to_device(host, "cuda")
    lists = [[aligned[b, j] for j in range(rs.n)] for b in range(3)]
    assert not BatchScrubPlan(lists, rs.H, 4096).bytewise
    lists[2] = cases.unaligned_rows(host[2], "cuda")
    plan = BatchScrubPlan(lists, rs.H, 4096)
    assert plan.bytewise and (plan.batch, plan.ncols, plan.nmask, plan.ident) == (3, 4101, 2, 4)
    assert not plan.syndrome_mask().cpu().numpy().any()
    rep = plan.scrub()
    assert isinstance(rep, BatchScrubReport) and rep.clean.all()


def test_slice_boundary_at_65537_stripes():
    cases.case_slice_boundary("cuda")


def test_refusals():
    cases.case_refusals("cuda")


def test_trivial_batches():
    cases.case_trivial("cuda")


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (4, 6, "cauchy")], ids=code_id)
def test_general_kernel_matches_rows_in_flight_kernel(code, monkeypatch):
    """(10, 14) and (4, 6) batches take the batched rows-in-flight kernel by default, the parity rows
    XORed in unmultiplied; GFRS_TUNE=scrub_ident=0 multiplies them and scrub_rows=0 takes the batched
    general kernel. Same masks from all three."""
    nstripes, ncols = 5, 8192 + 3
    rs = codec(code)
    bad = np.array(cases.host_batch(code, nstripes, ncols))
    bad[1, 0, 4000:4200] ^= 0xFF
    bad[4, rs.n - 1, ncols - 1] ^= 0x02
    stripes = cases.batch_to_device(bad, "cuda")
    want = cases.oracle_batch(code, bad, 4096)[0]
    assert np.array_equal(rs.syndrome_mask_batch(stripes, block_bytes=4096).cpu().numpy(), want)
    for tune in ("scrub_ident=0", "scrub_rows=0"):
        monkeypatch.setenv("GFRS_TUNE", tune)
        assert np.array_equal(rs.syndrome_mask_batch(stripes, block_bytes=4096).cpu().numpy(), want), tune


def test_syndrome_mask_batch_on_a_side_stream_and_plan_reuse():
    """10. Two calls on one side stream, no sync in between: distinct fresh tensors, one cache entry."""
    code = (10, 14, "vandermonde")
    rs = ReedSolomon(10, 14)  # a codec of its own: the shared one may hold a plan for these very addresses
    bad = np.array(cases.host_batch(code, 3, 8192 + 3))
    bad[2, 4, 4096] ^= 0x10
    stripes = cases.batch_to_device(bad, "cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    m1 = rs.syndrome_mask_batch(stripes, block_bytes=4096, stream=side)
    m2 = rs.syndrome_mask_batch(stripes, block_bytes=4096, stream=side)
    assert len(rs._plans) == 1 and m1.data_ptr() != m2.data_ptr()
    plan = next(iter(rs._plans.values()))
    assert isinstance(plan, BatchScrubPlan) and not any(isinstance(v, torch.Tensor) and v.dim() > 1
                                                        for v in vars(plan).values())  # no hold on the buffers
    side.synchronize()
    want = cases.oracle_batch(code, bad, 4096)[0]
    assert np.array_equal(m1.cpu().numpy(), want) and np.array_equal(m2.cpu().numpy(), want)
    rep = rs.scrub_batch(stripes, block_bytes=4096, stream=side)
    assert len(rs._plans) == 1 and rep.dirty == [2] and rep.report[2].suspects == [4]


# ---- 9. the batched launchers, called directly ------------------------------------------------------
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 8  # guard words before and after the ranges the launchers may write


class Launch:
    """A valid plan of a dirty batch, with 0x5A-filled mask and counts buffers that carry guard words
    around the [B * nmask] and [B * (n + 2)] ranges, for direct launcher calls."""

    def __init__(self, code, nstripes=3, ncols=4101):
        self.rs = codec(code)
        self.n, self.p, self.nstripes, self.ncols = self.rs.n, self.rs.p, nstripes, ncols
        self.host = np.array(cases.host_batch(code, nstripes, ncols))
        for b in range(nstripes):
            self.host[b, (5 * b) % self.n, (997 * b + 4095) % ncols] ^= 0x31 + b
        self.host[nstripes - 1, 0, :40] ^= 0x0F
        self.stripes = cases.batch_to_device(self.host, "cuda")
        self.plan = BatchScrubPlan([[self.stripes[b, j] for j in range(self.n)] for b in range(nstripes)],
                                   self.rs.H, 4096)
        assert not self.plan.bytewise
        self.nmask = self.plan.nmask
        self.mask = torch.full((GUARD + nstripes * self.nmask + GUARD,), FILL32, dtype=torch.int32, device="cuda")
        self.counts = torch.full((GUARD + nstripes * (self.n + 2) + GUARD,), FILL64, dtype=torch.int64, device="cuda")
        self.loc = self.plan.loc if self.plan.loc is not None else torch.zeros(
            self.p * self.n + 2 * self.n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def syndrome(self, batch=None, block_bytes=4096, ident=None, refused=True):
        args = (int(self.plan.desc.data_ptr()), self.n, self.plan.m_pad, self.plan.ident if ident is None else ident,
                self.nstripes if batch is None else batch, self.ncols, False, block_bytes,
                int(self.mask.data_ptr()) + 4 * GUARD, torch.cuda.current_stream().cuda_stream)
        if not refused:
            return hip().syndrome_batched(*args)
        with pytest.raises(RuntimeError, match="gf_syndrome_batched"):
            hip().syndrome_batched(*args)
        self.untouched()

    def locate(self, batch=None, block_bytes=4096, p=None, refused=True):
        args = (int(self.plan.desc.data_ptr()), self.n, self.p if p is None else p,
                self.nstripes if batch is None else batch, self.ncols, False, block_bytes,
                int(self.mask.data_ptr()) + 4 * GUARD, int(self.loc.data_ptr()), True,
                int(self.counts.data_ptr()) + 8 * GUARD, torch.cuda.current_stream().cuda_stream)
        if not refused:
            return hip().locate_batched(*args)
        with pytest.raises(RuntimeError, match="gf_locate_batched"):
            hip().locate_batched(*args)
        self.untouched()

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.mask.cpu().numpy() == FILL32).all() and (self.counts.cpu().numpy() == FILL64).all()


@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (9, 14, "cauchy")], ids=code_id)
def test_batched_launchers_write_their_ranges_only(code):
    r = Launch(code)
    r.syndrome(refused=False)
    r.locate(refused=False)
    torch.cuda.synchronize()
    mask, counts = r.mask.cpu().numpy(), r.counts.cpu().numpy()
    for buf, fill in ((mask, FILL32), (counts, FILL64)):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all()
    want_mask, votes, unlocated, bad = cases.oracle_batch(code, r.host, 4096)
    assert bad.all() and want_mask.any(axis=1).all()  # a dirty batch
    assert np.array_equal(mask[GUARD:-GUARD].reshape(r.nstripes, r.nmask), want_mask)
    got = counts[GUARD:-GUARD].reshape(r.nstripes, r.n + 2)
    assert np.array_equal(got[:, : r.n], votes)
    assert np.array_equal(got[:, r.n], unlocated) and np.array_equal(got[:, r.n + 1], bad)


def test_batched_launchers_refuse_an_empty_batch_a_bad_block_size_and_a_bad_ident():
    r = Launch((4, 6, "cauchy"))  # m_pad = 2
    for batch in (0, -1):
        r.syndrome(batch=batch)
        r.locate(batch=batch)
    for bb in (2048, 12288):
        r.syndrome(block_bytes=bb)
        r.locate(block_bytes=bb)
    r.syndrome(ident=3)   # > m_pad, < n
    r.syndrome(ident=-1)
    r.locate(p=6)  # p == n
    r.locate(p=0)
    tall = Launch((19, 36, "cauchy"), ncols=17)  # p = 17: beyond the locate kernel's tile
    assert (tall.p, tall.plan.m_pad) == (17, 32)
    tall.locate()

"""Scrub on the MI355X (csrc/kernels/gf_scrub.hip): the cases of tests/test_scrub.py on CUDA tensors,
every result compared exactly with the numpy oracle (``gf.scrub_oracle``) or with the value the
check matrix dictates."""
import numpy as np
import pytest
import torch

import test_scrub as cases
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops.scrub import ScrubPlan

pytestmark = pytest.mark.gpu

LOCATING = [c for c in cases.CODES if 2 <= c[1] - c[0] <= 16]


@pytest.mark.parametrize("ncols", cases.SHAPES)
@pytest.mark.parametrize("code", cases.CODES, ids=cases.code_id)
def test_clean_stripe(code, ncols):
    cases.case_clean("cuda", code, ncols)


@pytest.mark.parametrize("ncols,bb", [(17, 4096), (4101, 4096), (65536 + 3, 65536)])
@pytest.mark.parametrize("code", cases.CODES, ids=cases.code_id)
def test_single_byte_flip(code, ncols, bb):
    cases.case_single_flip("cuda", code, ncols, bb)


@pytest.mark.parametrize("ncols", cases.SHAPES)
@pytest.mark.parametrize("code", cases.CODES, ids=cases.code_id)
def test_whole_chunk_overwritten(code, ncols):
    cases.case_chunk_overwritten("cuda", code, ncols)


@pytest.mark.parametrize("code", LOCATING, ids=cases.code_id)
def test_two_chunks_damaged_at_disjoint_columns(code):
    cases.case_two_chunks_disjoint("cuda", code)


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (10, 14, "cauchy"), (5, 8, "sys_vandermonde")],
                         ids=cases.code_id)
def test_two_chunks_damaged_in_the_same_column(code):
    cases.case_two_chunks_same_column("cuda", code)


@pytest.mark.parametrize("ncols", [15, 4101, 65536 + 3])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (20, 36, "vandermonde")],
                         ids=cases.code_id)
def test_unaligned_rows(code, ncols):
    cases.case_unaligned_rows("cuda", code, ncols)


def test_other_fields_raise():
    cases.case_other_fields("cuda")


@pytest.mark.parametrize("code", [(10, 14, "vandermonde"), (4, 6, "cauchy")], ids=cases.code_id)
def test_general_kernel_matches_rows_in_flight_kernel(code, monkeypatch):
    """(10, 14) and (4, 6) stripes take the rows-in-flight syndrome kernel by default, with the parity
    rows XORed in unmultiplied; GFRS_TUNE=scrub_ident=0 multiplies them by H's identity block and
    scrub_rows=0 takes the general two-rows-in-flight kernel. Same masks from all three."""
    ncols = 3 * 65536 + 4097
    rs = cases.codec(code)
    bad = np.array(cases.host_stripe(code, ncols))
    bad[0, 70000:70100] ^= 0xFF
    bad[rs.n - 1, ncols - 1] ^= 0x02
    stripe = cases.to_device(bad, "cuda")
    want = gf.scrub_oracle(rs.H, bad, 4096)[0]
    assert np.array_equal(rs.syndrome_mask(stripe, 4096).cpu().numpy(), want)
    for tune in ("scrub_ident=0", "scrub_rows=0"):
        monkeypatch.setenv("GFRS_TUNE", tune)
        assert np.array_equal(rs.syndrome_mask(stripe, 4096).cpu().numpy(), want), tune


def test_syndrome_mask_on_a_side_stream_and_plan_reuse():
    """syndrome_mask launches on the given stream without a host sync, and a repeated call on the same
    buffers reuses the cached plan (one entry per buffers and block size)."""
    code = (10, 14, "vandermonde")
    rs = ReedSolomon(10, 14)  # a codec of its own: the shared one may hold a plan for these very addresses
    bad = np.array(cases.host_stripe(code, 65536 + 3))
    bad[4, 65536] ^= 0x10
    stripe = cases.to_device(bad, "cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    m1 = rs.syndrome_mask(stripe, 65536, stream=side)
    m2 = rs.syndrome_mask(stripe, 65536, stream=side)
    assert len(rs._plans) == 1 and m1.data_ptr() != m2.data_ptr()
    side.synchronize()
    want = gf.scrub_oracle(rs.H, bad, 65536)[0]
    assert np.array_equal(m1.cpu().numpy(), want) and np.array_equal(m2.cpu().numpy(), want)
    rep = rs.scrub(stripe, 65536, stream=side)
    assert rep.suspects == [4] and rep.bad_columns == 1


# ---- the edge codes and the matrices no codec produces (tests/test_scrub.py) -------------------------
@pytest.mark.parametrize("code,ncols", cases.EDGE_SHAPES, ids=map(cases.run_id, cases.EDGE_SHAPES))
def test_edge_clean_stripe(code, ncols):
    cases.case_clean("cuda", code, ncols)


@pytest.mark.parametrize("code,ncols,bb", cases.EDGE_FLIPS, ids=map(cases.run_id, cases.EDGE_FLIPS))
def test_edge_single_byte_flip(code, ncols, bb):
    cases.case_single_flip("cuda", code, ncols, bb)


@pytest.mark.parametrize("code,ncols", cases.EDGE_SHAPES, ids=map(cases.run_id, cases.EDGE_SHAPES))
def test_edge_whole_chunk_overwritten(code, ncols):
    cases.case_chunk_overwritten("cuda", code, ncols)


@pytest.mark.parametrize("code", cases.EDGE_LOCATING, ids=cases.code_id)
def test_edge_two_chunks_damaged_at_disjoint_columns(code):
    cases.case_two_chunks_disjoint("cuda", code)


def test_p56_two_natives_fold_into_one_word():
    cases.case_wide_two_natives("cuda")


@pytest.mark.parametrize("code", cases.ALL_VALUES, ids=cases.code_id)
def test_every_error_value_in_every_chunk(code):
    cases.case_all_values_codec("cuda", code)


@pytest.mark.parametrize("code", list(cases.SPARSE), ids=cases.code_id)
def test_sparse_check_matrix(code):
    cases.case_sparse("cuda", code)


@pytest.mark.parametrize("code", cases.SPARSE_UNALIGNED, ids=cases.code_id)
def test_sparse_check_matrix_on_unaligned_rows(code):
    cases.case_sparse_unaligned("cuda", code)


@pytest.mark.parametrize("code", cases.MIXED, ids=cases.code_id)
def test_check_matrix_without_identity_block(code):
    cases.case_mixed("cuda", code)


def test_dependent_check_columns_locate_nothing():
    cases.case_dependent_columns("cuda")


@pytest.mark.parametrize("code", cases.BLOCK_SIZE_CODES, ids=cases.code_id)
def test_block_sizes_and_span_edges(code):
    cases.case_block_sizes("cuda", code)


# ---- the launchers refuse what they cannot run -----------------------------------------------------
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


class Refusal:
    """A valid plan of a small dirty stripe under the p x n check matrix ``h``, with 0x5A-filled mask
    and counts buffers (and a location table even where p > 16) for direct launcher calls."""

    def __init__(self, h, ncols=4101):
        h = np.asarray(h, dtype=np.uint8)
        self.p, self.n = h.shape
        self.ncols = ncols
        self.stripe = torch.full((self.n, ncols + 11), 7, dtype=torch.uint8, device="cuda")  # (rows at pitch 4112)
        self.plan = ScrubPlan([self.stripe[i, :ncols] for i in range(self.n)], h, 4096)
        assert not self.plan.bytewise
        self.mask = torch.full((8,), FILL32, dtype=torch.int32, device="cuda")
        self.counts = torch.full((self.n + 2,), FILL64, dtype=torch.int64, device="cuda")
        self.loc = torch.zeros(self.p * self.n + 2 * self.n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def syndrome(self, block_bytes=4096, ident=0, m_pad=None):
        with pytest.raises(RuntimeError, match="gf_syndrome"):
            hip().syndrome(int(self.plan.desc.data_ptr()), self.n, m_pad or self.plan.m_pad, ident, self.ncols, False,
                           block_bytes, int(self.mask.data_ptr()), torch.cuda.current_stream().cuda_stream)
        self.untouched()

    def locate(self, block_bytes=4096, p=None):
        with pytest.raises(RuntimeError, match="gf_locate"):
            hip().locate(int(self.plan.desc.data_ptr()), self.n, p or self.p, self.ncols, False, block_bytes,
                         int(self.mask.data_ptr()), int(self.loc.data_ptr()), True, int(self.counts.data_ptr()),
                         torch.cuda.current_stream().cuda_stream)
        self.untouched()

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.mask.cpu().numpy() == FILL32).all() and (self.counts.cpu().numpy() == FILL64).all()


def test_launchers_refuse_a_bad_block_size():
    r = Refusal(cases.codec((4, 6, "cauchy")).H)
    for bb in (2048, 12288):
        r.syndrome(block_bytes=bb, ident=2)
        r.locate(block_bytes=bb)


def test_syndrome_launcher_refuses_a_bad_ident():
    r = Refusal(cases.codec((4, 6, "cauchy")).H)  # m_pad = 2
    r.syndrome(ident=3)   # > m_pad, < n
    r.syndrome(ident=-1)
    tall = Refusal(np.array([[1, 2, 3], [1, 4, 5], [1, 6, 7], [1, 8, 9]]))  # n = 3, m_pad = 4
    assert (tall.plan.m_pad, tall.plan.ident) == (4, 0)
    tall.syndrome(ident=3)  # <= m_pad, >= n
    tall.syndrome(ident=4)


def test_locate_launcher_refuses_p_beyond_its_tile_or_the_stripe():
    r = Refusal(cases.codec((19, 36, "cauchy")).H)  # p = 17, m_pad = 32
    assert (r.p, r.plan.m_pad) == (17, 32)
    r.locate()
    tall = Refusal(np.array([[1, 2, 3], [1, 4, 5], [1, 6, 7], [1, 8, 9]]))
    tall.locate(p=4)  # p > n
    tall.locate(p=3)  # p == n (the descriptor's m_pad = 4 is what p = 3 pads to as well)

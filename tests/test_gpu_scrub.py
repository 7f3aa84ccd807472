"""Scrub on the MI355X (csrc/kernels/gf_scrub.hip): the cases of tests/test_scrub.py on CUDA tensors,
every result compared exactly with the numpy oracle (``gf.scrub_oracle``) or with the value the
check matrix dictates."""
import numpy as np
import pytest
import torch

import test_scrub as cases
from gpu_rscode_amd import ReedSolomon, gf

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

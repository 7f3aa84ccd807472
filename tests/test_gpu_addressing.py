"""Where in memory the bytes are (GPU): column offsets across 2^31 and 2^32, absolute addresses across
a 2^32 multiple, rows longer than 2^32 bytes, strides at the 32-bit limits of the GF(2^16)
matrix-core kernel, reversed and overlapping rows, and batched stripes more than 2^32 bytes apart.

Every assertion is bit-exact against the numpy oracle (windows, strides) or the torch table
reference of tests/addressing_cases.py (whole rows), and after every windowed run the WHOLE output and
copy buffers are checked on the device: a store whose offset wrapped modulo 2^31 or 2^32 lands near
the start of the buffer. The three 4.3 GiB buffers of addressing_cases.Buffers serve all of it; a
test skips only when the device has less free memory than they need.

The CPU test of the torch reference is the one test here that needs no GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import addressing_cases as ac
from gpu_rscode_amd import ReedSolomon, alloc_rows, gf
from gpu_rscode_amd.gf import GF256
from gpu_rscode_amd.ops import Gemm16Plan, GemmPlan, fill_random_
from gpu_rscode_amd.utils.tune import with_tune

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P31, P32, S_UNI = ac.P31, ac.P32, ac.S_UNI


# ---- the torch reference against the oracle (CPU) ---------------------------------------------------
@pytest.mark.parametrize("field,k,m,n,chunk", [(8, 5, 3, 1001, 64), (8, 1, 1, 7, 1 << 20), (8, 4, 2, 256, 256),
                                               (16, 3, 2, 2 * 501, 2 * 50), (16, 1, 1, 2, 2), (16, 4, 3, 2 * 64, 1 << 20)])
def test_torch_reference_matches_oracle(field, k, m, n, chunk):
    """The torch table reference of the whole-row cases equals ``GF256.gemm`` / ``gf.field(16).gemm``
    on CPU tensors, coefficients 0 and 1 included, with a last chunk shorter than the others; and the
    oracle with kept tables (wide GF(2^16) windows) is the plain one."""
    rng = np.random.default_rng(field * 100 + k)
    coeff = (ac.coeff8 if field == 8 else ac.coeff16)(m, k, k + m)
    if k >= 2:
        assert coeff[0, 0] == 0 and coeff[0, 1] == 1
    host = rng.integers(0, 256, size=(k, n), dtype=np.uint8)
    if field == 8:
        host[0, :256] = np.arange(256)[: min(n, 256)]  # every byte value
        want = GF256.gemm(coeff, host)
    else:
        want = np.ascontiguousarray(gf.field(16).gemm(coeff, host.view("<u2"))).view(np.uint8)
    assert np.array_equal(ac.oracle(field, coeff, host), want)
    rows = [torch.from_numpy(host[j].copy()) for j in range(k)]
    got = np.zeros((m, n), np.uint8)
    ends = []
    for s, e, ref in ac.torch_gemm_chunks(field, coeff, rows, chunk):
        got[:, s:e] = ref.numpy()
        ends.append(e)
    assert ends[-1] == n and len(ends) == -(-n // chunk)
    assert np.array_equal(got, want)
    outs = [torch.from_numpy(want[i].copy()) for i in range(m)]
    assert ac.whole_row_mismatches(field, coeff, rows, outs, chunk) == (0, -1)
    outs[m - 1][n - 1] ^= 0x40
    assert ac.whole_row_mismatches(field, coeff, rows, outs, chunk) == (1, (n - 1) // chunk * chunk)
    assert ac.first_other(torch.full((77,), 0x5A, dtype=torch.uint8), 0x5A) == -1
    t = torch.full((77,), 0x5A, dtype=torch.uint8)
    t[70] = 0
    assert ac.first_other(t, 0x5A) == 70


# ---- the buffers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def holder():
    b = ac.Buffers()
    yield b
    b.release()


@pytest.fixture
def bufs(holder):
    why = holder.acquire()
    if why:
        pytest.skip(why)
    return holder


@gpu
def test_input_buffer_is_random_past_4gib(bufs):
    """fill_random_ on a buffer longer than 2^32 bytes: the bytes past 2^32 are not a repeat of the
    first ones, and are as evenly spread as test_fill_random_deterministic_and_spread demands."""
    lo, hi = bufs.big[: 1 << 20], bufs.big[P32 : P32 + (1 << 20)]
    assert not torch.equal(lo, hi)
    for part in (lo, hi, bufs.big[-(1 << 20):]):
        hist = torch.bincount(part.long(), minlength=256).float()
        assert hist.min() > 0.8 * hist.mean()
    again = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    fill_random_(again, ac.SEED)
    assert torch.equal(again, lo)


# ---- 3. strides -------------------------------------------------------------------------------------
def _host_rows(rows):
    return np.stack([r.cpu().numpy() for r in rows])


@gpu
@pytest.mark.parametrize("k", [9, 17])
@pytest.mark.parametrize("stride", [1 << 28, (1 << 28) + 1024, 64])
def test_gf16_mfma_uniform_stride_limits(bufs, stride, k):
    """The GF(2^16) matrix-core kernel addresses uniform-stride rows through one buffer resource per
    K-step: 32-bit lane offsets up to 7 strides + 124 and num_records = live rows x stride. 2^28 is the
    largest stride of that form (num_records exactly 2^31 on a full step), 2^28 + 1024 the first on
    the pointer form; a stride under a wave's 128 columns (overlapping rows) would cut the last live
    row's columns off and takes the pointer form too. k = 9: the second K-step holds one live row;
    k = 17: two full steps and one row. Rows past k lie in the same random buffer and must
    contribute nothing."""
    m, C = 20, 1024 * 5 + 6
    rows = [bufs.big[j * stride : j * stride + C] for j in range(k)]
    coeff = ac.coeff16(m, k, stride % 1000 + k)
    out = alloc_rows(m, C, "cuda", fill=0x5A)
    plan = Gemm16Plan(rows, out, coeff, engine="mfma")
    assert plan.in_stride == stride
    plan.run()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ac.oracle(16, coeff, _host_rows(rows)))


def _reversed_inputs(k, C, seed):
    dev = alloc_rows(k, C, "cuda")
    dev.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(k, C), dtype=np.uint8)))
    rows = [dev[k - 1 - j] for j in range(k)]
    assert rows[1].data_ptr() < rows[0].data_ptr()
    return rows, _host_rows(rows)


@gpu
@pytest.mark.parametrize("k,m,form", [(40, 32, "v1"), (128, 16, "ar"), (128, 26, "tm"), (128, 32, "ar")])
@pytest.mark.parametrize("rows", ["reversed", "overlapping"])
def test_fp4_negative_and_short_uniform_stride(bufs, k, m, form, rows):
    """Every FP4 form on its uniform-stride path with the rows of one allocation listed in reverse
    (a negative stride), and with a stride shorter than the rows (views 272 bytes apart)."""
    C = 256 * 9 + 77
    if rows == "reversed":
        inputs, host = _reversed_inputs(k, C, k + m)
    else:
        inputs = [bufs.big[P32 - 4096 + 272 * j :][:C] for j in range(k)]  # (and across a 2^32 offset)
        host = _host_rows(inputs)
    coeff = ac.coeff8(m, k, k * m)
    out = alloc_rows(m, C, "cuda", fill=0x5A)
    plan = GemmPlan(inputs, out, coeff, engine="mfma")
    assert plan.fp4_form == form
    assert plan.in_stride == (272 if rows == "overlapping" else inputs[1].data_ptr() - inputs[0].data_ptr())
    assert rows == "overlapping" or plan.in_stride < 0
    plan.run()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), GF256.gemm(coeff, host))


@gpu
@pytest.mark.parametrize("engine", ["mfma_i8", "gf16_mfma", "valu"])
def test_reversed_rows_other_engines(engine):
    """Rows of one allocation in reverse on the int8 matrix-core engine, the GF(2^16) matrix-core
    engine (a non-positive stride takes its pointer form) and the default v_perm path."""
    C = 1024 * 3 + 522
    k, m = {"mfma_i8": (16, 4), "gf16_mfma": (17, 20), "valu": (6, 3)}[engine]
    inputs, host = _reversed_inputs(k, C, k)
    out = alloc_rows(m, C, "cuda", fill=0x5A)
    if engine == "gf16_mfma":
        coeff = ac.coeff16(m, k, 3)
        plan = Gemm16Plan(inputs, out, coeff, engine="mfma")
        want = ac.oracle(16, coeff, host)
    else:
        coeff = ac.coeff8(m, k, 3)
        plan = GemmPlan(inputs, out, coeff, engine="auto" if engine == "valu" else engine)
        assert plan.engine == engine
        want = GF256.gemm(coeff, host)
    if engine != "valu":
        assert plan.in_stride < 0
    plan.run()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


BSTRIDE = P32 + 4096


@gpu
@pytest.mark.parametrize("case", ["vperm", "fp4ar", "fp4ar_copy", "valu16", "gf16_mfma"])
def test_batched_stripes_more_than_4gib_apart(bufs, case):
    """B = 2 stripes whose rows are 2^32 + 4096 bytes apart, inputs, outputs and copies one
    as_strided view each: the batched v_perm kernel, the batched A-resident FP4 kernel (plain, and
    with fused copies of the first k - m inputs) and the batched GF(2^16) plan on both engines."""
    field = 16 if case in ("valu16", "gf16_mfma") else 8
    k, m = {"vperm": (10, 4), "fp4ar": (128, 32), "fp4ar_copy": (128, 26), "valu16": (64, 16), "gf16_mfma": (64, 16)}[case]
    C = 256 * 9 + (77 if field == 8 else 76)
    pitch = 2560
    assert BSTRIDE + k * pitch <= ac.IN_BYTES and BSTRIDE + m * pitch <= ac.OUT_BYTES and BSTRIDE + k * pitch <= ac.CPY_BYTES
    x = bufs.big.as_strided((2, k, C), (BSTRIDE, pitch, 1))
    y = bufs.out.as_strided((2, m, C), (BSTRIDE, pitch, 1))
    z = bufs.cpy.as_strided((2, k, C), (BSTRIDE, pitch, 1))
    ncopy = k - m if case == "fp4ar_copy" else 0
    copies = [[z[b, j] if j < ncopy else None for j in range(k)] for b in range(2)] if ncopy else None
    bufs.fill()
    if field == 8:
        coeff = ac.coeff8(m, k, 17)
        plan = GemmPlan(x, y, coeff, copies=copies, engine="mfma" if case.startswith("fp4") else "auto")
        assert plan.engine == ("mfma" if case.startswith("fp4") else "valu")
    else:
        coeff = ac.coeff16(m, k, 17)
        plan = Gemm16Plan(x, y, coeff, engine="mfma" if case == "gf16_mfma" else "valu16")
    assert plan.batch == 2 and (plan.in_bstride, plan.out_bstride) == (BSTRIDE, BSTRIDE)
    if case != "vperm" and case != "valu16":
        assert plan.in_stride == pitch
    plan.run()
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    got = y.cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], ac.oracle(field, coeff, xh[b])), b
    y.fill_(ac.FILL_OUT)
    if ncopy:
        assert np.array_equal(z[:, :ncopy].cpu().numpy(), xh[:, :ncopy])
        z[:, :ncopy].fill_(ac.FILL_CPY)
    bufs.assert_untouched(case)


# ---- 1. column windows ------------------------------------------------------------------------------
def _odd(k):
    return tuple(range(1, k, 2))


def _expect(**want):
    """A check_plan that asserts plan attributes."""
    def check(plan):
        for name, value in want.items():
            assert getattr(plan, name) == value, (name, getattr(plan, name))
    return check


@gpu
@pytest.mark.parametrize("case", ["vec_k6_copies", "vec_k32_tile16", "rows_latency", "byte_unaligned_rows",
                                  "byte_odd_col0", "ksplit", "lut", "mfma_i8"])
def test_windows_gf256_kernels(bufs, case):
    """The v_perm vec kernel (default path, with fused copies; and the 16-row tile with two groups per
    lane), the rows-in-flight kernel's latency form, the byte kernel (rows 3 bytes off alignment; odd
    column starts on aligned rows), the k-split kernel, the LDS-table kernel and the int8
    matrix-core engine over the windows of addressing_cases.window_case."""
    if case == "vec_k6_copies":
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c, copies=cp), k=6, m=3, copy_rows=_odd(6),
                       check_plan=_expect(engine="valu"))
    elif case == "vec_k32_tile16":
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c, engine="valu"), k=32, m=20,
                       run=lambda p, c0, n: p.run(col0=c0, ncols=n, vec=2, pf=2, nt=True))
    elif case == "rows_latency":
        ac.rows_kernel_windows(bufs)
    elif case == "byte_unaligned_rows":
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c), k=5, m=2, in_base=3,
                       check_plan=_expect(bytewise=True))
    elif case == "byte_odd_col0":
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c), k=5, m=2, shift=1,
                       check_plan=_expect(bytewise=False))
    elif case == "ksplit":
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c, engine="valu"), k=64, m=16)
    elif case == "lut":
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c, engine="lut"), k=10, m=4)
    else:
        ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c, engine="mfma_i8"), k=16, m=4)


@gpu
def test_windows_rows_kernel_throughput_form(holder):
    """The rows-in-flight kernel's throughput form (the headline's) over the same windows:
    GFRS_TUNE=rows_lat_groups=0 in a subprocess, as test_rows_kernel_forms_match_oracle (the
    threshold is read once). The subprocess makes its own buffers, so this process gives its own
    back first."""
    holder.release()
    code = ("import sys; sys.path[:0] = [%r, %r]; import addressing_cases as ac; ac.rows_throughput_main()"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=with_tune(rows_lat_groups="0"))
    if r.returncode == 0 and "ADDR-SKIP" in r.stdout:
        pytest.skip(r.stdout.strip())
    assert r.returncode == 0 and "ADDR-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    peak = int(r.stdout.rsplit("peak=", 1)[1].split()[0])
    print(f"subprocess peak device memory: {peak} bytes")
    assert peak <= ac.GIB16


_FP4_WINDOWS = [(40, 32, False, "v1"), (128, 12, False, "v1"), (128, 12, True, "v1"), (128, 16, False, "ar"),
                (128, 16, True, "ar"), (128, 32, False, "ar"), (128, 26, True, "tm"), (128, 20, False, "tm")]


@gpu
@pytest.mark.parametrize("layout", ["uniform", "scattered"])
@pytest.mark.parametrize("k,m,copy,form", _FP4_WINDOWS)
def test_windows_fp4_forms(bufs, k, m, copy, form, layout):
    """Each FP4 form (v1 LDS ring, A-resident, tile-major) on its shapes, computed DMA addresses
    (uniform stride) or the row-pointer table (scattered), with fused copies of the first k - m inputs
    on the forms that have them."""
    def check(plan):
        assert plan.engine == "mfma" and plan.fp4_form == form
        assert plan.in_stride == (S_UNI if layout == "uniform" else 0)

    ac.window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c, copies=cp, engine="mfma"), k=k, m=m, layout=layout,
                   copy_rows=tuple(range(k - m)) if copy else (), check_plan=check)


@gpu
@pytest.mark.parametrize("case", ["valu16", "valu16_copies", "symbol_kernel"])
def test_windows_gf16_vperm_kernels(bufs, case):
    """Gemm16Plan engine='valu16' over the windows: the 16-byte vector kernel on aligned rows (plain
    and with fused copies) and the one-symbol-per-lane kernel on rows 2 bytes off alignment."""
    def check(plan):
        assert plan.engine == "valu16" and plan.symwise == (case == "symbol_kernel")

    ac.window_case(bufs, lambda i, o, c, cp: Gemm16Plan(i, o, c, copies=cp, engine="valu16"), k=6, m=3, field=16,
                   in_base=2 if case == "symbol_kernel" else 0, copy_rows=_odd(6) if case == "valu16_copies" else (),
                   check_plan=check)


@gpu
@pytest.mark.parametrize("variant", ["uniform", "scattered", "copies"])
@pytest.mark.parametrize("k,m", [(17, 20), (300, 40)])
def test_windows_gf16_mfma(bufs, k, m, variant):
    """Gemm16Plan engine='mfma' over the windows: the buffer-resource form (uniform stride), the
    pointer form (scattered rows; with fused copies of every other row), one and several K passes.
    Window (a) starts 2 bytes off a 4-byte boundary: the v_perm-record route."""
    layout = "uniform" if variant == "uniform" else "scattered"

    def check(plan):
        assert plan.engine == "mfma" and plan.in_stride == (S_UNI if layout == "uniform" else 0)

    assert ac.WIN_A[0] % 4 == 2
    ac.window_case(bufs, lambda i, o, c, cp: Gemm16Plan(i, o, c, copies=cp, engine="mfma"), k=k, m=m, field=16,
                   layout=layout, copy_rows=_odd(k) if variant == "copies" else (), check_plan=check)


# ---- 2. whole rows longer than 2^32 bytes -----------------------------------------------------------
def _whole_row_case(bufs, field, k, m, make_plan, run, in_base=0):
    length = ac.WHOLE8 if field == 8 else ac.WHOLE16
    rows = [bufs.big[in_base + j * S_UNI :][:length] for j in range(k)]
    store = [bufs.out, bufs.cpy][:m]
    outs = [s[:length] for s in store]
    coeff = (ac.coeff8 if field == 8 else ac.coeff16)(m, k, 5 * k + m)
    bufs.fill()
    plan = make_plan(rows, outs, coeff)
    assert plan.ncols == length
    run(plan)
    torch.cuda.synchronize()
    bad, at = ac.whole_row_mismatches(field, coeff, rows, outs)
    assert bad == 0, f"{bad} wrong bytes, the first in the chunk at column {at} ({at:#x})"
    for s, fill in zip(store, (ac.FILL_OUT, ac.FILL_CPY)):  # nothing past the row end
        assert ac.first_other(s[length:], fill) < 0
    return plan


@gpu
@pytest.mark.parametrize("case", ["vec", "rows_throughput", "byte", "valu16"])
def test_whole_rows_longer_than_4gib(bufs, case):
    """Loop counters, grids and group counts on rows of 2^32 + 16,011 bytes (GF(2^16): 16,010), inputs
    overlapping views, outputs real rows, every output byte compared on the device with the torch
    reference. vec: the default configuration, k = 4, m = 2. rows_throughput: the rows-in-flight
    kernel with 2^28 groups, far above rows_lat_groups. byte: unaligned rows, more lanes than
    grid_cap(1) x 256, so the capped grid's stride loop runs. valu16: two groups per lane."""
    if case == "vec":
        _whole_row_case(bufs, 8, 4, 2, lambda i, o, c: GemmPlan(i, o, c), lambda p: p.run())
    elif case == "rows_throughput":
        _whole_row_case(bufs, 8, 10, 2, lambda i, o, c: GemmPlan(i, o, c), lambda p: p.run(vec=1, pf=0, nt=True))
    elif case == "byte":
        plan = _whole_row_case(bufs, 8, 2, 1, lambda i, o, c: GemmPlan(i, o, c), lambda p: p.run(), in_base=3)
        assert plan.bytewise and ac.WHOLE8 > (0xFFFFFFFF // 256 // 8 * 8) * 256
    else:
        _whole_row_case(bufs, 16, 3, 1, lambda i, o, c: Gemm16Plan(i, o, c, engine="valu16"), lambda p: p.run())


def _flip(t, col, bits):
    t[col : col + 1] ^= bits


@gpu
@pytest.mark.parametrize("k,n", [(2, 3), (1, 3)])
def test_scrub_rows_longer_than_4gib(bufs, k, n):
    """Scrub of three real rows of 2^32 + 16,011 bytes, parity from a GemmPlan (checked against the
    torch reference): the clean stripe gives an all-zero mask; one byte flipped at column 2^31 + 7 of
    chunk 0 and one at column 2^32 + 5 of the last parity chunk set exactly the two block words
    scrub_oracle sets on those blocks, and scrub counts those two columns. RS(2,3) has one parity
    chunk, so no column can be located (both are unlocated, as the oracle says); RS(1,3) names both
    chunks."""
    L, bb = ac.WHOLE8, 65536
    rs = ReedSolomon(k, n)
    store = [bufs.out, bufs.big, bufs.cpy] if k == 2 else [bufs.big, bufs.out, bufs.cpy]
    stripe = [s[:L] for s in store]
    bufs.fill()
    if k == 2:
        fill_random_(bufs.out, ac.SEED + 1)  # chunk 0 (the shared input buffer is chunk 1)
    GemmPlan(stripe[:k], stripe[k:], rs.E).run()
    torch.cuda.synchronize()
    assert ac.whole_row_mismatches(8, rs.E, stripe[:k], stripe[k:]) == (0, -1)
    mask = rs.syndrome_mask(stripe, bb)
    assert mask.numel() == -(-L // bb) == 65537 and not bool(mask.any().item())
    hits = [(0, P31 + 7, 0x21), (n - 1, P32 + 5, 0x80)]
    try:
        for chunk, col, bits in hits:
            _flip(stripe[chunk], col, bits)
        want_mask = np.zeros(mask.numel(), np.int32)
        votes, unlocated, bad = np.zeros(n, np.int64), 0, 0
        for _, col, _ in hits:
            b = col // bb
            blk = np.stack([r[b * bb : min(L, (b + 1) * bb)].cpu().numpy() for r in stripe])
            w, v, u, c = gf.scrub_oracle(rs.H, blk, bb)
            want_mask[b] = w[0]
            votes, unlocated, bad = votes + v, unlocated + u, bad + c
        assert bad == 2 and np.count_nonzero(want_mask) == 2
        assert np.array_equal(rs.syndrome_mask(stripe, bb).cpu().numpy(), want_mask)
        rep = rs.scrub(stripe, bb)
        assert np.array_equal(rep.mask.cpu().numpy(), want_mask)
        assert (rep.bad_columns, rep.unlocated) == (2, unlocated) and np.array_equal(rep.votes, votes)
        if k == 2:
            assert unlocated == 2 and rep.suspects == []
        else:
            assert unlocated == 0 and rep.suspects == [0, n - 1] and votes[0] == 1 and votes[n - 1] == 1
    finally:
        for chunk, col, bits in hits:  # (chunk 0 of RS(1,3) is the shared input buffer)
            _flip(stripe[chunk], col, bits)
    assert not bool(rs.syndrome_mask(stripe, bb).any().item())


@gpu
def test_zz_peak_device_memory(holder):
    """Last in the module: everything above stayed within 16 GiB of device memory."""
    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory of the module: {peak} bytes ({peak / 2**30:.2f} GiB)")
    assert peak <= ac.GIB16

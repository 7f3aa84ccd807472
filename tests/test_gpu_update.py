"""Partial-stripe writes on the MI355X (csrc/kernels/gf_update.hip): the cases of tests/test_update.py on
CUDA tensors, every result compared exactly with the numpy oracle (``gf.update_oracle``); then what
only the device has: streams and the plan cache, the launcher's refusals, a window past 2^32 bytes
and the C API."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import test_update as cases
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import UpdatePlan, build_desc, pad_m, perm_tables_from_coeff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("code,ncols,changed", cases.FULL, ids=map(cases.run_id, cases.FULL))
def test_update_and_update_delta(code, ncols, changed):
    cases.case_update("cuda", code, ncols, changed)


@pytest.mark.parametrize("code,ncols,changed", cases.SHORT, ids=map(cases.run_id, cases.SHORT))
def test_write(code, ncols, changed):
    cases.case_write("cuda", code, ncols, changed)


@pytest.mark.parametrize("col0,ncols", cases.WINDOWS)
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=cases.code_id)
def test_windows(code, col0, ncols):
    for changed in ((1,), tuple(range(code[0] - 1, -1, -1))[:9]):
        cases.case_window("cuda", code, col0, ncols, changed)


def test_default_window():
    cases.case_default_window("cuda")


@pytest.mark.parametrize("ncols", [15, 4101, 65536 + 3])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=cases.code_id)
def test_unaligned_rows(code, ncols):
    """Every row at +1 from a 16-byte boundary, and parity aligned with new not: the byte form."""
    k = code[0]
    for changed in ((k - 1,), tuple(range(min(k, 9)))):
        cases.case_update("cuda", code, ncols, changed, shift=1)
        cases.case_write("cuda", code, ncols, changed, shift=1)
        cases.case_update("cuda", code, ncols, changed, shift=0, shift_new=1)
        cases.case_write("cuda", code, ncols, changed, shift=0, shift_new=1)


@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (5, 10, "cauchy")], ids=cases.code_id)
def test_same_contents_and_two_updates_in_a_row(code):
    cases.case_noop_and_composition("cuda", code, 4101)


def test_gf16_field():
    cases.case_other_field("cuda", "gf16")


def test_gf65536_field_is_refused_on_the_device():
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf65536")
    rows = torch.full((7, 64), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError, match="gf65536"):
        rs.update(rows[4:6], [0], rows[:1], rows[6:])
    with pytest.raises(NotImplementedError, match="gf65536"):
        rs.update_delta(rows[4:6], [0], rows[6:])
    with pytest.raises(NotImplementedError, match="gf65536"):
        rs.write(rows[:6], [0], rows[6:])
    assert bool((rows == 0x5A).all())


def test_refusals():
    cases.case_refusals("cuda")


def test_no_parity_rows():
    cases.case_no_parity("cuda")


def test_byte_form_matches_vector_form():
    """A plan of aligned rows forced onto the byte form (as an odd col0 would) gives the same bytes."""
    code, c, ch = (10, 14, "vandermonde"), 4101, [9, 0, 4]
    rs = cases.codec(code)
    host, new = cases.host_stripe(code, c), cases.host_new(code, c)
    par, old_t, new_t = (cases.to_device(a, "cuda") for a in (host[10:], host[ch], new[ch]))
    plan = UpdatePlan(par, old_t, new_t, rs.E[:, ch])
    assert not plan.bytewise and plan.passes[0][0] == 3
    plan.bytewise = True
    plan.run()
    cases.assert_rows(par, cases.expected_parity(code, c, tuple(ch)))
    cases.assert_padding(par, old_t, new_t)


def test_update_on_a_side_stream_and_plan_reuse():
    """update launches on the given stream without a host sync, and a repeated call on the same buffers
    reuses the cached plan (one entry per buffers, form and changed list)."""
    code, c, ch = (10, 14, "vandermonde"), 65536 + 3, [7, 2]
    rs = ReedSolomon(10, 14)  # a codec of its own: the shared one may hold a plan for these very addresses
    host, new = cases.host_stripe(code, c), cases.host_new(code, c)
    par, old_t, new_t = (cases.to_device(a, "cuda") for a in (host[10:], host[ch], new[ch]))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rs.update(par, ch, old_t, new_t, stream=side)
    rs.update(par, ch, new_t, old_t, stream=side)  # back again: other rows in the old / new places
    assert len(rs._plans) == 2
    rs.update(par, ch, old_t, new_t, stream=side)
    rs.update(par, ch, old_t, new_t, col0=16, ncols=0, stream=side)
    assert len(rs._plans) == 2
    side.synchronize()
    cases.assert_rows(par, cases.expected_parity(code, c, tuple(ch)))
    stripe = cases.to_device(host, "cuda")
    torch.cuda.synchronize()
    n0 = len(rs._plans)
    rs.write(stripe, ch, new_t, stream=side)
    rs.write(stripe, ch, new_t, stream=side)  # the natives already hold new: a zero delta
    assert len(rs._plans) == n0 + 1
    side.synchronize()
    assert not rs.syndrome_mask(stripe, 4096).cpu().numpy().any()
    cases.assert_rows(stripe[10:], cases.expected_parity(code, c, tuple(ch)))


# ---- the launcher refuses what it cannot run -------------------------------------------------------
def test_launcher_refusals():
    rs = cases.codec((4, 6, "cauchy"))
    buf = torch.full((4, 4112), 0x5A, dtype=torch.uint8, device="cuda")
    plan = UpdatePlan(buf[:2, :4101], buf[2:3, :4101], buf[3:4, :4101], rs.E[:, [1]])
    assert plan.m_pad == 2 and not plan.bytewise
    desc = int(plan.passes[0][1].data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ok = dict(desc=desc, d=1, m_pad=2, col0=0, ncols=4101, pairs=True, store_new=False, bytewise=False, stream=s)
    for bad in (dict(d=0), dict(d=9), dict(pairs=False, store_new=True), dict(col0=-1), dict(col0=-16), dict(m_pad=3),
                dict(m_pad=0), dict(m_pad=24), dict(ncols=-1), dict(desc=0)):
        with pytest.raises(RuntimeError, match="gf_update"):
            hip().update(**{**ok, **bad})
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all()), bad
    hip().update(**{**ok, "ncols": 0})  # success, nothing launched
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


# ---- a window past 2^32 bytes ------------------------------------------------------------------------
def _all_fill(buf, lo, hi, value=0x5A, step=1 << 28):
    return all(bool(torch.all(buf[s: min(hi, s + step)] == value)) for s in range(lo, hi, step))


@pytest.mark.parametrize("form", ["vector", "byte"])
def test_window_past_4gib(form):
    """Rows are views of one 0x5A-filled buffer of 2^32 + 2^20 bytes, 16 KiB apart, so column 2^32 of
    the two parity rows, of old and of new all lie inside it and a window of 8,211 columns crosses
    that byte of each: the offsets are formed in 64 bits. The (4, 6) code, d = 1, straight through
    the launcher (views that overlap outside their windows are not a stripe the codec accepts)."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of device memory, {free >> 20} MiB are free")
    rs = cases.codec((4, 6, "cauchy"))
    total, gap, n = (1 << 32) + (1 << 20), 16384, 8211
    shift = 0 if form == "vector" else 1
    col0 = (1 << 32) - 4096 + 16
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf.fill_(0x5A)
    base = (-buf.data_ptr()) % 16 + shift
    starts = [base + i * gap for i in range(4)]  # parity 0, parity 1, old, new
    assert starts[-1] + col0 + n <= total and col0 < 1 << 32 < col0 + n
    rng = np.random.default_rng(32)
    host = rng.integers(0, 256, size=(4, n), dtype=np.uint8)
    for s, h in zip(starts, host):
        buf[s + col0: s + col0 + n].copy_(torch.from_numpy(h))
    ptrs = [int(buf.data_ptr()) + s for s in starts]
    assert all(q % 16 == shift for q in ptrs)
    coeff = rs.E[:, [2]]
    desc = torch.from_numpy(build_desc([ptrs[2]], ptrs[:2], [ptrs[3]], perm_tables_from_coeff(coeff))).cuda()
    hip().update(int(desc.data_ptr()), 1, pad_m(2), col0, n, True, False, shift != 0,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = np.array(host)
    want[:2] = gf.update_oracle(rs.E, host[:2], [2], host[2:3], host[3:4])
    for s, w, name in zip(starts, want, ("parity 0", "parity 1", "old", "new")):
        assert np.array_equal(buf[s + col0: s + col0 + n].cpu().numpy(), w), name
    # no stray store: below the first window, between the windows, above the last
    edges = [0] + [e for s in starts for e in (s + col0, s + col0 + n)] + [total]
    for lo, hi in zip(edges[0::2], edges[1::2]):
        assert _all_fill(buf, lo, hi), (lo, hi)
    del buf
    torch.cuda.empty_cache()


# ---- C API ------------------------------------------------------------------------------------------
LIB = os.path.join(ROOT, "lib", "libgfrs.so")
DEMO = os.path.join(ROOT, "bin", "gfrs_capi_demo")


def _lib():
    lib = ctypes.CDLL(LIB)
    vpp = ctypes.POINTER(ctypes.c_void_p)
    lib.gfrs_update_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_char_p, vpp, vpp, vpp, ctypes.c_int]
    lib.gfrs_update_run.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    lib.gfrs_update_destroy.argtypes = [ctypes.c_void_p]
    lib.gfrs_last_error.restype = ctypes.c_char_p
    return lib


def _ptrs(t):
    return (ctypes.c_void_p * t.shape[0])(*[int(t[i].data_ptr()) for i in range(t.shape[0])])


def test_capi_version():
    assert _lib().gfrs_api_version() == 4


@pytest.mark.parametrize("d", [1, 9])
def test_capi_update(d):
    code, c = (10, 14, "vandermonde"), 4101
    rs, lib = cases.codec(code), _lib()
    ch = [3] if d == 1 else [9, 1, 8, 2, 7, 3, 6, 4, 5]
    host, new = cases.host_stripe(code, c), cases.host_new(code, c)
    want = cases.expected_parity(code, c, tuple(ch))
    coeff = np.ascontiguousarray(rs.E[:, ch]).tobytes()
    # pair form, then delta form over a window, then a write into the stripe
    par, old_t, new_t = (cases.to_device(a, "cuda") for a in (host[10:], host[ch], new[ch]))
    torch.cuda.synchronize()
    u = ctypes.c_void_p()
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, 4, coeff, _ptrs(old_t), _ptrs(new_t), _ptrs(par), 0) == 0, \
        lib.gfrs_last_error()
    assert lib.gfrs_update_run(u, 0, c, None) == 0, lib.gfrs_last_error()
    assert lib.gfrs_update_run(u, 0, c, None) == 0  # twice: back to the old parity
    torch.cuda.synchronize()
    cases.assert_rows(par, host[10:], "two runs cancel")
    assert lib.gfrs_update_run(u, 0, c, None) == 0
    torch.cuda.synchronize()
    cases.assert_rows(par, want, "pair form")
    cases.assert_rows(old_t, host[ch])
    lib.gfrs_update_destroy(u)
    par2, delta = cases.to_device(host[10:], "cuda"), cases.to_device(host[ch] ^ new[ch], "cuda")
    torch.cuda.synchronize()
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, 4, coeff, _ptrs(delta), None, _ptrs(par2), 0) == 0
    assert lib.gfrs_update_run(u, 5, 4000, None) == 0
    torch.cuda.synchronize()
    expect = np.array(host[10:])
    expect[:, 5:4005] = want[:, 5:4005]
    cases.assert_rows(par2, expect, "delta form in a window")
    lib.gfrs_update_destroy(u)
    stripe = cases.to_device(host, "cuda")
    torch.cuda.synchronize()
    olds = (ctypes.c_void_p * d)(*[int(stripe[j].data_ptr()) for j in ch])
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, 4, coeff, olds, _ptrs(new_t), _ptrs(stripe[10:]), 1) == 0
    assert lib.gfrs_update_run(u, 0, c, None) == 0
    torch.cuda.synchronize()
    full = np.array(host)
    full[ch], full[10:] = new[ch], want
    cases.assert_rows(stripe, full, "store_new")
    lib.gfrs_update_destroy(u)
    cases.assert_padding(par, par2, stripe, old_t, new_t, delta)
    # refusals: GFRS_EINVAL (-1), nothing written
    assert lib.gfrs_update_create(ctypes.byref(u), 0, 0, 4, coeff, olds, None, _ptrs(par), 0) == -1
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, 4, coeff, _ptrs(delta), None, _ptrs(par), 1) == -1
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, 4, coeff, _ptrs(par2[:1].expand(d, c)), None, _ptrs(par2),
                                  0) == -1  # a delta row that is a parity row
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, 4, coeff, _ptrs(delta), None, _ptrs(par2), 0) == 0
    assert lib.gfrs_update_run(u, -1, 10, None) == -1 and lib.gfrs_update_run(u, 0, -1, None) == -1
    assert lib.gfrs_update_run(None, 0, 1, None) == -1
    lib.gfrs_update_destroy(u)
    lib.gfrs_update_destroy(None)
    torch.cuda.synchronize()
    cases.assert_rows(par2, expect)


def test_capi_demo_runs_the_update_section():
    out = subprocess.run([DEMO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "update" in out.stdout and "MISMATCH" not in out.stdout

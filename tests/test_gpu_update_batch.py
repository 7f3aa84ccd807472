"""Batched partial-stripe writes on the MI355X (the batched instantiations of csrc/kernels/gf_update.hip):
the cases of tests/test_update_batch.py on CUDA tensors, every result compared exactly with the numpy
oracle (``gf.update_oracle`` stripe by stripe) and with a loop of single ``update`` / ``write`` calls on
copies of the same buffers; then what only the device has: 65,537 stripes in two launches, the
launcher's refusals, streams and the plan cache, and stripes 2^32 + 4096 bytes apart."""
import numpy as np
import pytest
import torch

import test_update as cases
import test_update_batch as batch
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import BatchUpdatePlan, pad_m, perm_tables_from_coeff
from gpu_rscode_amd.ops.update import build_update_batch_desc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("code,nstripes,ncols", batch.RUNS, ids=map(batch.run_id, batch.RUNS))
def test_codes_batches_and_row_lengths(code, nstripes, ncols):
    batch.case_forms("cuda", code, nstripes, ncols)


@pytest.mark.parametrize("code,nstripes,d", batch.IDS_RUNS,
                         ids=[f"{cases.code_id(c)}-B{b}-d{d}" for c, b, d in batch.IDS_RUNS])
def test_per_stripe_ids(code, nstripes, d):
    ids = batch.spread_ids(code[0], nstripes, d)
    batch.case_forms("cuda", code, nstripes, 4101 if code != batch.WIDE else 273, ids)


def test_shared_list_equals_the_list_repeated():
    batch.case_shared_list("cuda")


@pytest.mark.parametrize("nstripes,which", [(3, 0), (3, 1), (3, 2), (257, 0), (257, 128), (257, 256)])
def test_stripe_identity(nstripes, which):
    batch.case_stripe_identity("cuda", nstripes, which)


@pytest.mark.parametrize("col0,nc", [(0, None), (16, 4000), (5, 100)])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (5, 10, "cauchy")], ids=cases.code_id)
def test_write_batch_forms(code, col0, nc):
    batch.case_write_forms("cuda", code, col0=col0, nc=nc)


@pytest.mark.parametrize("col0,ncols", cases.WINDOWS)
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=cases.code_id)
def test_windows(code, col0, ncols):
    batch.case_window("cuda", code, col0, ncols)


def test_one_unaligned_row():
    batch.case_one_unaligned_row("cuda")


@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=cases.code_id)
def test_every_row_unaligned(code):
    """Every row at +1 from a 16-byte boundary: the byte form with per-stripe ids, d = 2 and two passes."""
    batch.case_forms("cuda", code, 3, 4101, shift=1)
    batch.case_forms("cuda", code, 3, 15, batch.spread_ids(code[0], 3, min(code[0], 9)), shift=1)


def test_input_forms():
    batch.case_input_forms("cuda")


def test_refusals():
    batch.case_refusals("cuda")


def test_no_parity_rows_and_empty_batch():
    batch.case_no_parity_and_empty("cuda")


def test_gf16_agrees_with_its_own_encode_batch():
    batch.case_other_field("cuda", "gf16")


def test_gf65536_field_is_refused_on_the_device():
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf65536")
    rows = torch.full((2, 7, 64), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError, match="gf65536"):
        rs.update_batch(rows[:, 4:6], [0], rows[:, :1], rows[:, 6:])
    with pytest.raises(NotImplementedError, match="gf65536"):
        rs.update_delta_batch(rows[:, 4:6], [[0], [1]], rows[:, 6:])
    with pytest.raises(NotImplementedError, match="gf65536"):
        rs.write_batch(rows[:, :6], [0], rows[:, 6:])
    assert bool((rows == 0x5A).all())


# ---- more stripes than one launch's grid.y ------------------------------------------------------------
def test_65537_stripes_run_as_two_launches():
    """(4, 6), d = 1, C = 17 in rows of 32 bytes (the vector form with a tail byte), tensor form. Only
    stripes 0, 65,534, 65,535 and 65,536 get new contents (the last launch holds two stripes): those
    equal the oracle, every other byte of the buffer is unchanged, compared on the device."""
    code, nstripes, c = (4, 6, "cauchy"), 65537, 17
    rs, k = ReedSolomon(4, 6, matrix="cauchy"), 4
    rng = np.random.default_rng(65537)
    data = rng.integers(0, 256, size=(nstripes, k, c), dtype=np.uint8)
    par = gf.GF256.gemm(rs.E, data.transpose(1, 0, 2).reshape(k, -1)).reshape(2, nstripes, c).transpose(1, 0, 2)
    host = np.full((nstripes, 6, 32), cases.GARBAGE, dtype=np.uint8)
    host[:, :k, :c], host[:, k:, :c] = data, par
    ids = np.arange(nstripes, dtype=np.int64)[:, None] % k
    old = batch.pick(data, ids)
    new = np.array(old)
    touched = [0, 65534, 65535, 65536]
    new[touched] = rng.integers(0, 256, size=(4, 1, c), dtype=np.uint8)
    want = np.array(host)
    for b in touched:
        want[b, k:, :c] = gf.update_oracle(rs.E, par[b], list(ids[b]), old[b], new[b])
        assert not np.array_equal(want[b], host[b])
    buf = torch.from_numpy(host).cuda()
    old_t, new_t = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda()
    parity = buf[:, k:, :c]
    assert rs.update_batch(parity, ids, old_t, new_t) is parity
    (plan,) = [p for key, p in rs._plans.items() if key[0] == "updb"]
    assert plan.batch == nstripes and plan.bytewise  # (old / new rows of 17 bytes: the byte form) ...
    assert torch.equal(buf, torch.from_numpy(want).cuda())
    # ... and the vector form: every row at a multiple of 16
    buf.copy_(torch.from_numpy(host))
    wide = torch.full((2, nstripes, 1, 32), cases.GARBAGE, dtype=torch.uint8, device="cuda")
    wide[0, :, :, :c], wide[1, :, :, :c] = old_t, new_t
    rs.update_batch(parity, ids, wide[0, :, :, :c], wide[1, :, :, :c])
    plans = [p for key, p in rs._plans.items() if key[0] == "updb"]
    assert len(plans) == 2 and not plans[1].bytewise
    assert torch.equal(buf, torch.from_numpy(want).cuda())
    assert bool((wide[:, :, :, c:] == cases.GARBAGE).all())
    # write_batch over the same stripes: the natives too
    buf.copy_(torch.from_numpy(host))
    stripes = buf[:, :, :c]
    assert rs.write_batch(stripes, ids, wide[1, :, :, :c]) is stripes
    np.put_along_axis(want[:, :k, :c], ids[:, :, None], new, axis=1)
    assert torch.equal(buf, torch.from_numpy(want).cuda())


# ---- the launcher refuses what it cannot run -------------------------------------------------------
def test_launcher_refusals():
    """Invalid arguments only: hipErrorInvalidValue and nothing launched."""
    rs = cases.codec((4, 6, "cauchy"))
    buf = torch.full((2, 4, 4112), 0x5A, dtype=torch.uint8, device="cuda")
    plan = BatchUpdatePlan(buf[:, :2, :4101], buf[:, 2:3, :4101], buf[:, 3:4, :4101], changed=[[1], [3]], coeff=rs.E)
    assert plan.m_pad == 2 and plan.k == 4 and plan.batch == 2 and not plan.bytewise and len(plan.passes) == 1
    desc = int(plan.passes[0][1].data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ok = dict(desc=desc, k=4, d=1, m_pad=2, batch=2, col0=0, ncols=4101, pairs=True, store_new=False, bytewise=False,
              stream=s)
    for bad in (dict(desc=0), dict(batch=0), dict(batch=-1), dict(d=0), dict(d=9), dict(k=0), dict(k=-4), dict(k=257),
                dict(m_pad=3), dict(m_pad=0), dict(m_pad=24), dict(m_pad=272), dict(col0=-1), dict(col0=-16),
                dict(ncols=-1), dict(pairs=False, store_new=True)):
        with pytest.raises(RuntimeError, match="gf_update_batched"):
            hip().update_batched(**{**ok, **bad})
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all()), bad
    hip().update_batched(**{**ok, "ncols": 0})  # success, nothing launched
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())
    with pytest.raises(ValueError):
        BatchUpdatePlan(buf[:, :2], buf[:, 2:3], None, changed=[1], coeff=rs.E, store_new=True)
    with pytest.raises(ValueError):
        BatchUpdatePlan(buf[:, :2], buf[:, 2:3], buf[:, :1], changed=[1], coeff=rs.E)  # a parity row as new


def test_update_batch_on_a_side_stream_and_plan_reuse():
    """update_batch launches on the given stream without a host sync, and a repeated call on the same
    buffers and ids reuses the cached plan: two calls, one cache entry; other ids, another entry."""
    code, nstripes, c = (10, 14, "vandermonde"), 5, 65536 + 3
    rs, k = ReedSolomon(10, 14), 10  # a codec of its own: the shared one may hold a plan for these very addresses
    host, fresh = batch.host_batch(code, nstripes, c), batch.host_new_batch(code, nstripes, c)
    ids = batch.spread_ids(k, nstripes, 9)  # two passes
    old, new = batch.pick(host, ids), batch.pick(fresh, ids)
    (_, par), (_, old_t), (_, new_t) = (batch.to_batch(a, "cuda") for a in (host[:, k:], old, new))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rs.update_batch(par, ids, old_t, new_t, stream=side)
    assert len(rs._plans) == 1
    (plan,) = rs._plans.values()
    assert [d for d, _ in plan.passes] == [8, 1]
    rs.update_batch(par, ids.tolist(), new_t, old_t, stream=side)  # back again: other rows in the old / new places
    assert len(rs._plans) == 2
    rs.update_batch(par, torch.from_numpy(ids), old_t, new_t, stream=side)
    rs.update_batch(par, ids, old_t, new_t, col0=16, ncols=0, stream=side)
    assert len(rs._plans) == 2 and any(p is plan for p in rs._plans.values())
    side.synchronize()
    batch.assert_batch(par, batch.expected_batch(code, host, ids, old, new))
    ids2 = np.roll(ids, 1, axis=1)  # the same natives per stripe in another order: other rows, another plan
    _, par2 = batch.to_batch(host[:, k:], "cuda")
    torch.cuda.synchronize()
    rs.update_batch(par2, ids2, torch.roll(old_t, 1, 1), torch.roll(new_t, 1, 1), stream=side)
    assert len(rs._plans) == 3
    side.synchronize()
    assert torch.equal(par2, par)
    _, stripes = batch.to_batch(host, "cuda")
    torch.cuda.synchronize()
    rs.write_batch(stripes, ids, new_t, stream=side)
    rs.write_batch(stripes, ids, new_t, stream=side)  # the natives already hold new: a zero delta
    assert len(rs._plans) == 4
    side.synchronize()
    assert not rs.syndrome_mask_batch(stripes, block_bytes=4096).cpu().numpy().any()
    assert torch.equal(stripes[:, k:], par)
    # cached plans hold no buffer references
    for p in (p for p in rs._plans.values() if isinstance(p, BatchUpdatePlan)):
        assert not any(isinstance(v, torch.Tensor) or hasattr(v, "ptrs") for v in vars(p).values()), vars(p).keys()


def test_byte_form_matches_vector_form():
    """A plan of aligned rows forced onto the byte form (as an odd col0 would) gives the same bytes."""
    code, nstripes, c = (10, 14, "vandermonde"), 3, 4101
    rs, k = cases.codec(code), 10
    host, fresh = batch.host_batch(code, nstripes, c), batch.host_new_batch(code, nstripes, c)
    ids = batch.spread_ids(k, nstripes, 3, seed=1)
    old, new = batch.pick(host, ids), batch.pick(fresh, ids)
    (pf, par), (of, old_t), (nf, new_t) = (batch.to_batch(a, "cuda") for a in (host[:, k:], old, new))
    plan = BatchUpdatePlan(par, old_t, new_t, changed=ids, coeff=rs.E)
    assert not plan.bytewise and plan.passes[0][0] == 3
    plan.bytewise = True
    plan.run()
    batch.assert_batch(par, batch.expected_batch(code, host, ids, old, new))
    cases.assert_padding(pf, of, nf)


# ---- stripes more than 2^32 bytes apart ---------------------------------------------------------------
def _all_fill(buf, lo, hi, value=0x5A, step=1 << 28):
    return all(bool(torch.all(buf[s: min(hi, s + step)] == value)) for s in range(lo, hi, step))


@pytest.mark.parametrize("form", ["vector", "byte"])
def test_stripes_4gib_apart(form):
    """B = 2 stripes of the (4, 6) code whose rows are views of one 0x5A-filled buffer, the second
    stripe's 2^32 + 4096 bytes after the first's, C = 4101, d = 1 with another native in each stripe:
    row addresses and per-stripe pointer offsets are formed in 64 bits. Straight through the launcher,
    then the same batch as one strided tensor per argument through the codec."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of device memory, {free >> 20} MiB are free")
    rs = cases.codec((4, 6, "cauchy"))
    apart, gap, c = (1 << 32) + 4096, 8192, 4101
    total = apart + (1 << 20)
    shift = 0 if form == "vector" else 1
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf.fill_(0x5A)
    base = (-buf.data_ptr()) % 16 + shift
    # rows of stripe b: parity 0, parity 1, old, new
    starts = np.array([[base + b * apart + i * gap for i in range(4)] for b in range(2)], dtype=np.int64)
    assert starts.max() + c <= total
    rng = np.random.default_rng(33)
    host = rng.integers(0, 256, size=(2, 4, c), dtype=np.uint8)
    ids = np.array([[2], [0]])

    def load():
        buf.fill_(0x5A)
        for b in range(2):
            for i in range(4):
                buf[starts[b, i]: starts[b, i] + c].copy_(torch.from_numpy(host[b, i]))

    def check(what):
        for b in range(2):
            want = np.array(host[b])
            want[:2] = gf.update_oracle(rs.E, host[b, :2], list(ids[b]), host[b, 2:3], host[b, 3:4])
            for i in range(4):
                assert np.array_equal(buf[starts[b, i]: starts[b, i] + c].cpu().numpy(), want[i]), (what, b, i)
        edges = [0] + [e for s in starts.reshape(-1) for e in (int(s), int(s) + c)] + [total]
        for lo, hi in zip(edges[0::2], edges[1::2]):  # no stray store anywhere else
            assert _all_fill(buf, lo, hi), (what, lo, hi)

    load()
    ptrs = (starts + int(buf.data_ptr())).astype(np.uint64)
    assert all(int(q) % 16 == shift for q in ptrs.reshape(-1))
    desc = torch.from_numpy(build_update_batch_desc(ids, ptrs[:, 2:3], ptrs[:, 3:4], ptrs[:, :2],
                                                    perm_tables_from_coeff(rs.E))).cuda()
    hip().update_batched(int(desc.data_ptr()), 4, 1, pad_m(2), 2, 0, c, True, False, shift != 0,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check("launcher")
    load()
    par = buf.as_strided((2, 2, c), (apart, gap, 1), base)
    old = buf.as_strided((2, 1, c), (apart, gap, 1), base + 2 * gap)
    new = buf.as_strided((2, 1, c), (apart, gap, 1), base + 3 * gap)
    ReedSolomon(4, 6, matrix="cauchy").update_batch(par, ids, old, new)
    torch.cuda.synchronize()
    check("codec")
    del buf, par, old, new
    torch.cuda.empty_cache()

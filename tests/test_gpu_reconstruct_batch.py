"""Batched repair on the MI355X (csrc/kernels/gf_repair.hip): the cases of tests/test_reconstruct_batch.py
on CUDA tensors, every result compared exactly with the numpy oracle (``gf.reconstruct_oracle`` stripe
by stripe) and with a loop of single ``reconstruct`` calls on copies of the same buffers; then what only
the device has: 65,537 stripes in two launches, the launcher's refusals, streams and the plan cache,
stripes 2^32 + 4096 bytes apart, and ``heal_batch`` repairing with one batched call. Every launch gets
valid pointers and in-range pattern indices."""
import numpy as np
import pytest
import torch

import test_reconstruct_batch as rb
import test_update as cases
import test_update_batch as ub
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import BatchRepairPlan
from gpu_rscode_amd.ops.repair import build_repair_batch_desc, repair_tables

pytestmark = pytest.mark.gpu


def repair_plans(rs):
    return [p for key, p in rs._plans.items() if key[0] == "repb"]


@pytest.mark.parametrize("code,e,nstripes,ncols", rb.RUNS, ids=map(rb.run_id, rb.RUNS))
def test_codes_batches_and_row_lengths(code, e, nstripes, ncols):
    rb.case_repair("cuda", code, nstripes, ncols, rb.spread_patterns(code[1], nstripes, e, e))


def test_every_stripe_with_a_pattern_of_its_own():
    rb.case_every_stripe_its_own_pattern("cuda")


def test_shared_list_equals_the_list_repeated():
    rb.case_shared_list("cuda")


def test_natives_only_parity_only_and_mixed():
    rb.case_kinds("cuda")


def test_mixed_lengths_and_the_padded_array_form():
    rb.case_mixed_lengths("cuda")


@pytest.mark.parametrize("which", [0, 128, 256])
def test_stripe_identity(which):
    rb.case_stripe_identity("cuda", 257, which)


@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "cauchy")], ids=cases.code_id)
def test_round_trip(code):
    rb.case_round_trip("cuda", code)


def test_gf16_agrees_with_its_own_reconstruct():
    rb.case_gf16("cuda")
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf16")  # ... and it takes the kernel: a plan is cached
    rows = torch.zeros((2, 6, 64), dtype=torch.uint8, device="cuda")
    rs.reconstruct_batch(rows, [[0], [5]])
    assert len(repair_plans(rs)) == 1


def test_gf65536_loops_over_the_stripes_on_the_device():
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf65536")
    data = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(3, 4, 64), dtype=np.uint8)).cuda()
    stripes = torch.zeros((3, 6, 64), dtype=torch.uint8, device="cuda")
    stripes[:, :4] = data
    for b in range(3):
        rs.encode(stripes[b, :4], stripes[b, 4:])
    good = stripes.clone()
    stripes[0, 5], stripes[1, 0], stripes[1, 4], stripes[2, 2] = 1, 2, 3, 4
    rs.reconstruct_batch(stripes, [[5], [0, 4], [2]])
    assert torch.equal(stripes, good) and not repair_plans(rs)


# ---- alignment ---------------------------------------------------------------------------------------
def test_one_unaligned_row_puts_the_batch_on_the_byte_form():
    rs = rb.case_one_unaligned_row("cuda")
    (plan,) = repair_plans(rs)
    assert plan.bytewise and plan.batch == 3 and plan.m_pad == 4 and plan.npat == 3


@pytest.mark.parametrize("code,e", [((4, 6, "cauchy"), 2), ((10, 14, "cauchy"), 4), ((19, 36, "cauchy"), 17)],
                         ids=lambda v: cases.code_id(v) if isinstance(v, tuple) else f"e{v}")
def test_every_row_unaligned(code, e):
    """Every row at +1 from a 16-byte boundary: the byte form, 1..e erasures per stripe."""
    rb.case_repair("cuda", code, 3, 4101, rb.spread_patterns(code[1], 3, 1, e, seed=1), shift=1)
    rb.case_repair("cuda", code, 3, 15, rb.spread_patterns(code[1], 3, e, e, seed=2), shift=1)


@pytest.mark.parametrize("code,e", [((10, 14, "cauchy"), 3), ((5, 10, "cauchy"), 5)],
                         ids=lambda v: cases.code_id(v) if isinstance(v, tuple) else f"e{v}")
def test_byte_form_matches_vector_form(code, e):
    """A plan of aligned rows forced onto the byte form gives the same bytes as the vector form."""
    nstripes, c = 3, 4101
    rs, (k, n, _) = cases.codec(code), code
    erased = rb.as_tuples(rb.spread_patterns(n, nstripes, 1, e, seed=3))
    bad, want = rb.damaged(code, nstripes, c, erased), rb.expected(code, nstripes, c, erased)
    distinct = sorted(set(tuple(sorted(ids)) for ids in erased))
    patterns = []
    for er in distinct:
        sv = [i for i in range(n) if i not in er][:k]
        patterns.append((sv, er, gf.GF256.matmul(rs.G[list(er)], rs.decode_matrix(sv))))
    pat = [distinct.index(tuple(sorted(ids))) for ids in erased]
    got = []
    for force in (False, True):
        sf, stripes = ub.to_batch(bad, "cuda")
        plan = BatchRepairPlan(stripes, pat, patterns)
        assert not plan.bytewise and plan.batch == nstripes and plan.npat == len(distinct)
        plan.bytewise = force
        plan.run()
        ub.assert_batch(stripes, want, f"force={force}")
        cases.assert_padding(sf)
        got.append(stripes)
    assert torch.equal(*got)


def test_refusals():
    rb.case_refusals("cuda")


def test_nothing_to_do():
    rb.case_nothing_to_do("cuda")


# ---- more stripes than one launch's grid.y ------------------------------------------------------------
def test_65537_stripes_run_as_two_launches():
    """(4, 6), C = 17 in rows of 32 bytes (the vector form with a tail byte), tensor form. Only stripes
    0, 65,534, 65,535 and 65,536 are damaged, each in a chunk (and a pattern) of its own, and only they
    are named (the last launch holds two stripes); then every stripe repairs chunk b % 6. Either way the
    whole buffer, compared on the device, is the consistent one again."""
    nstripes, c, k = 65537, 17, 4
    rs = ReedSolomon(4, 6, matrix="cauchy")
    rng = np.random.default_rng(65537)
    data = rng.integers(0, 256, size=(nstripes, k, c), dtype=np.uint8)
    par = gf.GF256.gemm(rs.E, data.transpose(1, 0, 2).reshape(k, -1)).reshape(2, nstripes, c).transpose(1, 0, 2)
    host = np.full((nstripes, 6, 32), cases.GARBAGE, dtype=np.uint8)
    host[:, :k, :c], host[:, k:, :c] = data, par
    good = torch.from_numpy(host).cuda()
    touched = {0: [1], 65534: [4, 0], 65535: [5], 65536: [2, 3]}
    bad = np.array(host)
    for b, ids in touched.items():
        bad[b, ids, :c] ^= 0x3C
    buf = torch.from_numpy(bad).cuda()
    stripes = buf[:, :, :c]
    # every stripe in the launch, the damaged ones under their own patterns
    every = np.stack([np.arange(nstripes) % 6, np.full(nstripes, -1)], axis=1)
    for b, ids in touched.items():
        every[b, : len(ids)] = ids
        every[b, len(ids):] = -1
    assert rs.reconstruct_batch(stripes, every) is stripes
    (plan,) = repair_plans(rs)
    assert plan.batch == nstripes and not plan.bytewise and plan.m_pad == 2
    assert torch.equal(buf, good)
    # only the damaged stripes named: four stripes in the launch, the rest never read
    buf.copy_(torch.from_numpy(bad))
    few = np.full((nstripes, 2), -1)
    for b, ids in touched.items():
        few[b, : len(ids)] = ids
    rs.reconstruct_batch(stripes, few)
    assert len(repair_plans(rs)) == 2 and repair_plans(rs)[1].batch == 4
    assert torch.equal(buf, good)


# ---- the launcher refuses what it cannot run -------------------------------------------------------
def test_launcher_refusals():
    """Invalid arguments only: hipErrorInvalidValue and nothing launched."""
    rs = cases.codec((4, 6, "cauchy"))
    buf = torch.full((2, 6, 4112), 0x5A, dtype=torch.uint8, device="cuda")
    coeff = gf.GF256.matmul(rs.G[[0, 5]], rs.decode_matrix([1, 2, 3, 4]))
    plan = BatchRepairPlan(buf[:, :, :4101], [0, 0], [((1, 2, 3, 4), (0, 5), coeff)])
    assert plan.m_pad == 2 and plan.k == 4 and plan.batch == 2 and plan.npat == 1 and not plan.bytewise
    torch.cuda.synchronize()
    ok = dict(desc=int(plan.desc.data_ptr()), k=4, m_pad=2, batch=2, npat=1, ncols=4101, bytewise=False,
              stream=torch.cuda.current_stream().cuda_stream)
    for bad in (dict(desc=0), dict(batch=0), dict(batch=-1), dict(npat=0), dict(npat=-3), dict(k=0), dict(k=-4),
                dict(k=257), dict(m_pad=3), dict(m_pad=0), dict(m_pad=-2), dict(m_pad=24), dict(m_pad=272),
                dict(ncols=-1), dict(ncols=-16, bytewise=True)):
        with pytest.raises(RuntimeError, match="gf_repair_batched"):
            hip().repair_batched(**{**ok, **bad})
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all()), bad
    hip().repair_batched(**{**ok, "ncols": 0})  # success, nothing launched
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


def test_reconstruct_batch_on_a_side_stream_and_plan_reuse():
    """reconstruct_batch launches on the given stream without a host sync, and a repeated call on the same
    buffers and ids reuses the cached plan: two calls, one cache entry; other patterns, another entry."""
    code, nstripes, c = (10, 14, "cauchy"), 5, 65536 + 3
    rs = ReedSolomon(10, 14, matrix="cauchy")  # a codec of its own: the shared one may hold plans for these addresses
    erased = rb.as_tuples(rb.spread_patterns(14, nstripes, 1, 4, seed=7))
    bad, want = rb.damaged(code, nstripes, c, erased), rb.expected(code, nstripes, c, erased)
    _, stripes = ub.to_batch(bad, "cuda")
    arr = np.full((nstripes, 4), -1, dtype=np.int64)
    for b, ids in enumerate(erased):
        arr[b, : len(ids)] = ids
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rs.reconstruct_batch(stripes, arr, stream=side)
    assert len(rs._plans) == 1
    (plan,) = rs._plans.values()
    rs.reconstruct_batch(stripes, arr.copy(), stream=side)  # (the erased rows are rewritten with what they hold)
    rs.reconstruct_batch(stripes, torch.from_numpy(arr), stream=side)
    assert len(rs._plans) == 1 and next(iter(rs._plans.values())) is plan
    side.synchronize()
    ub.assert_batch(stripes, want)
    other = np.array(arr)
    other[0, 0] = (arr[0, 0] + 1) % 14 if len(erased[0]) == 1 else arr[0, 1]  # another pattern for stripe 0
    rs.reconstruct_batch(stripes, other, stream=side)
    assert len(rs._plans) == 2
    side.synchronize()
    ub.assert_batch(stripes, want)  # (consistent stripes: whatever is rewritten keeps its bytes)
    # cached plans hold no buffer references: the descriptor is the plan's own
    for p in rs._plans.values():
        held = {name for name, v in vars(p).items() if isinstance(v, torch.Tensor) or hasattr(v, "ptrs")}
        assert isinstance(p, BatchRepairPlan) and held == {"desc"}, held
        assert p.desc.numel() < 1 << 20


# ---- stripes more than 2^32 bytes apart ---------------------------------------------------------------
@pytest.mark.parametrize("form", ["vector", "byte"])
def test_stripes_4gib_apart(form):
    """B = 2 stripes of the (4, 6) code whose rows are views of one 0x5A-filled buffer, the second
    stripe's 2^32 + 4096 bytes after the first's, C = 4101, another pattern in each stripe: row addresses
    and per-stripe pointer and table offsets are formed in 64 bits. Straight through the launcher, then
    the same batch as one strided tensor through the codec."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of device memory, {free >> 20} MiB are free")
    rs = cases.codec((4, 6, "cauchy"))
    apart, gap, c, k, n = (1 << 32) + 4096, 8192, 4101, 4, 6
    total = apart + (1 << 20)
    shift = 0 if form == "vector" else 1
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf.fill_(0x5A)
    base = (-buf.data_ptr()) % 16 + shift
    starts = np.array([[base + b * apart + i * gap for i in range(n)] for b in range(2)], dtype=np.int64)
    assert starts.max() + c <= total
    host = np.stack([cases.host_stripe((4, 6, "cauchy"), c)] * 2)
    host[1, :k] ^= 0x11
    host[1, k:] = gf.GF256.gemm(rs.E, host[1, :k])
    erased = [(1, 4), (0,)]

    def load():
        buf.fill_(0x5A)
        for b in range(2):
            for i in range(n):
                row = host[b, i] if i not in erased[b] else host[b, i] ^ 0xFF
                buf[starts[b, i]: starts[b, i] + c].copy_(torch.from_numpy(np.ascontiguousarray(row)))

    def check(what):
        for b in range(2):
            for i in range(n):
                assert np.array_equal(buf[starts[b, i]: starts[b, i] + c].cpu().numpy(), host[b, i]), (what, b, i)
        edges = [0] + [e for s in starts.reshape(-1) for e in (int(s), int(s) + c)] + [total]
        for lo, hi in zip(edges[0::2], edges[1::2]):  # no stray store anywhere else
            assert all(bool(torch.all(buf[s: min(hi, s + (1 << 28))] == 0x5A)) for s in range(lo, hi, 1 << 28)), \
                (what, lo, hi)

    load()
    ptrs = (starts + int(buf.data_ptr())).astype(np.uint64)
    assert all(int(q) % 16 == shift for q in ptrs.reshape(-1))
    patterns = []
    for er in erased:
        sv = [i for i in range(n) if i not in er][:k]
        patterns.append((sv, er, gf.GF256.matmul(rs.G[list(er)], rs.decode_matrix(sv))))
    ins = np.stack([ptrs[b, patterns[b][0]] for b in range(2)])
    outs = np.array([[ptrs[0, 1], ptrs[0, 4]], [ptrs[1, 0], 0]], dtype=np.uint64)
    desc = torch.from_numpy(build_repair_batch_desc(ins, outs, np.array([0, 1]), repair_tables(patterns, k, 2))).cuda()
    hip().repair_batched(int(desc.data_ptr()), k, 2, 2, 2, c, shift != 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check("launcher")
    load()
    stripes = buf.as_strided((2, n, c), (apart, gap, 1), base)
    fresh = ReedSolomon(4, 6, matrix="cauchy")
    fresh.reconstruct_batch(stripes, [list(e) for e in erased])
    torch.cuda.synchronize()
    (plan,) = repair_plans(fresh)
    assert plan.bytewise == (shift != 0)
    check("codec")
    del buf, stripes
    torch.cuda.empty_cache()


# ---- heal_batch repairs with one batched call -----------------------------------------------------
def test_heal_batch_repairs_with_one_batched_call(monkeypatch):
    """One bad chunk in every stripe (chunk b % n): heal_batch ends clean, with one reconstruct_batch
    call and no reconstruct call."""
    code, nstripes, c = (10, 14, "cauchy"), 33, 4101
    rs = ReedSolomon(10, 14, matrix="cauchy")
    host = ub.host_batch(code, nstripes, c)
    erased = tuple((b % 14,) for b in range(nstripes))
    sf, stripes = ub.to_batch(rb.damaged(code, nstripes, c, erased), "cuda")
    calls = {"batch": 0, "single": 0}
    batched, single = rs.reconstruct_batch, rs.reconstruct

    def spy_batch(*a, **kw):
        calls["batch"] += 1
        return batched(*a, **kw)

    def spy_single(*a, **kw):
        calls["single"] += 1
        return single(*a, **kw)

    monkeypatch.setattr(rs, "reconstruct_batch", spy_batch)
    monkeypatch.setattr(rs, "reconstruct", spy_single)
    report = rs.heal_batch(stripes)
    assert report.clean.all() and not report.unhealed and not report.dirty
    assert calls == {"batch": 1, "single": 0}
    ub.assert_batch(stripes, host)
    cases.assert_padding(sf)

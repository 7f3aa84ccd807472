"""Variable-length batches on the GPU (``csrc/kernels/gf_varlen.hip`` through ``VarlenCodec`` and
``ops.varlen.VarlenPlan``): every case of tests/varlen_cases.py against the numpy oracle, the flat
grid when it strides, the byte form, one launch for 65,537 stripes, the plan cache, stream order and
graph capture.

All rows are views of one guard-filled arena whose host image is the oracle of every byte; the WHOLE
arena is compared, so a byte past a row's end, a byte of a neighbouring stripe or an unstored byte
shows, and the failure names the stripe, the row and the column. Comparisons are exact. Nothing here
provokes a fault: what the launcher must refuse is refused on the host before any launch.

Stream order and capture use the harness of tests/test_gpu_streams.py / tests/test_gpu_graphs.py
(``stream_cases.gated`` / ``captured``) with entries of this file's own: the table in
tests/stream_cases.py lists the entry points of ``ReedSolomon`` and ``ops.__all__`` only.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc
import varlen_cases as vc
from gpu_rscode_amd import VarlenCodec
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import varlen as ov
from gpu_rscode_amd.ops.varlen import BLOCK, GROUP, VarlenPlan

pytestmark = pytest.mark.gpu
IDS = [f"{c}-{b}" for c, b in vc.CASES]


@pytest.fixture
def launches(monkeypatch):
    """Counts the launches of the varlen kernel (calls of the binding that reach the launcher)."""
    real, calls = hip().varlen, []

    class Counting:
        def __getattr__(self, name):
            return getattr(hip(), name)

        def varlen(self, *a):
            calls.append(a)
            return real(*a)
    monkeypatch.setattr(ov, "hip", lambda: Counting())
    return calls


def fresh(code):
    """A codec of the test's own (an empty plan cache)."""
    k, n, matrix, field = vc.CODES[code]
    return vc.ReedSolomon(k, n, matrix=matrix, field=field)


# ---- every case against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("code,batch", vc.CASES, ids=IDS)
def test_encode_cases(code, batch, launches):
    rs, lengths = fresh(code), vc.lengths_of(batch)
    data, par, good = vc.encode_case(code, lengths, "cuda")
    assert VarlenCodec(rs).encode(data.arg, par.arg) is par.arg
    par.check(f"{code} {batch}: parity")
    data.check(f"{code} {batch}: data")
    assert len(launches) == (1 if any(lengths) else 0)
    if launches:
        assert launches[0][6] is False, "aligned rows run the vector form"
    # ... and a loop of single calls on copies
    for b in sorted(set(np.linspace(0, len(lengths) - 1, 12).astype(int).tolist())):
        if lengths[b]:
            single = rs.encode(torch.stack(data.arg[b]).clone())
            assert np.array_equal(single.cpu().numpy(), good[b][rs.k:]), f"stripe {b}"
    if batch == "equal":
        whole = rs.encode_batch(torch.stack([torch.stack(s) for s in data.arg]))
        assert torch.equal(whole, torch.stack([torch.stack(s) for s in par.arg]))


@pytest.mark.parametrize("code,batch", vc.CASES, ids=IDS)
def test_reconstruct_cases(code, batch, launches):
    rs, lengths = fresh(code), vc.lengths_of(batch)
    erased = vc.erasures(code, len(lengths))
    stripes, bad, want = vc.repair_case(code, lengths, erased, "cuda")
    copies = [torch.stack(s).clone() for s in stripes.arg]
    assert VarlenCodec(rs).reconstruct(stripes.arg, [list(e) for e in erased]) is stripes.arg
    stripes.check(f"{code} {batch}")
    assert len(launches) == (1 if any(c and e for c, e in zip(lengths, erased)) else 0)
    for b in sorted(set(np.linspace(0, len(lengths) - 1, 12).astype(int).tolist())):
        if lengths[b] and erased[b]:
            rs.reconstruct(copies[b], list(erased[b]))
            assert np.array_equal(copies[b].cpu().numpy(), want[b]), f"stripe {b}"
    if batch == "equal":
        whole = torch.from_numpy(np.stack(bad)).cuda()
        rs.reconstruct_batch(whole, [list(e) for e in erased])
        assert torch.equal(whole, torch.stack([torch.stack(s) for s in stripes.arg]))


@pytest.mark.parametrize("kind", ["natives", "parity"])
def test_reconstruct_natives_only_and_parity_only(kind):
    code = "c10_14"
    erased = vc.erasures(code, len(vc.LENGTHS), kind=kind)
    stripes, _, _ = vc.repair_case(code, vc.LENGTHS, erased, "cuda")
    VarlenCodec(fresh(code)).reconstruct(stripes.arg, [list(e) for e in erased])
    stripes.check(kind)


# ---- the grid when it strides, and the forms -----------------------------------------------------------
def _plan(rs, batch, erased, **kw):
    pat, patterns = rs._erased_patterns(rs._erased_raw([list(e) for e in erased], rs.n), len(erased))
    full = [(sv, er, rs.gf.matmul(rs.G[list(er)], rs.decode_matrix(sv)).astype(np.uint8)) for sv, er in patterns]
    ptrs = np.array([[r.data_ptr() for r in s] for s in batch.arg], dtype=np.uint64)
    return VarlenPlan(ptrs, batch.lengths, pat, full, "cuda", **kw)


@pytest.mark.parametrize("laps", [1, 2, 3])
@pytest.mark.parametrize("max_blocks", [1, 2, 3, 8])
def test_capped_grid_strides_over_the_work_items(max_blocks, laps, launches):
    """nblk one above ``laps`` laps of ``max_blocks`` workgroups: a stripe of two blocks first, then
    stripes of one block each, so one workgroup's lap holds work items of several stripes."""
    nblk = max_blocks * laps + 1
    short = (GROUP + 1, 300, 1, (BLOCK - 1) * GROUP, 48, 777)
    lengths = (BLOCK * GROUP + 1,) + tuple(short[i % len(short)] for i in range(nblk - 2))
    rs = fresh("c10_14")
    erased = tuple(e or (0, 13) for e in vc.erasures("c10_14", len(lengths)))
    stripes, _, _ = vc.repair_case("c10_14", lengths, erased, "cuda")
    plan = _plan(rs, stripes, erased)
    assert plan.nblk == nblk and not plan.bytewise
    plan.run(max_blocks=max_blocks)
    stripes.check(f"max_blocks {max_blocks}, {laps} laps")
    assert [(a[5], a[7]) for a in launches] == [(nblk, max_blocks)]


@pytest.mark.parametrize("max_blocks", [0, 2])
def test_one_row_off_alignment_puts_the_batch_on_the_byte_form(max_blocks, launches):
    lengths = vc.LENGTHS[:-1]
    erased = vc.erasures("c10_14", len(lengths))
    stripes, _, _ = vc.repair_case("c10_14", lengths, erased, "cuda", shift={(5, 2): 1})
    rs = fresh("c10_14")
    if max_blocks:
        plan = _plan(rs, stripes, erased)
        assert plan.bytewise
        plan.run(max_blocks=max_blocks)
    else:
        VarlenCodec(rs).reconstruct(stripes.arg, [list(e) for e in erased])
    stripes.check("one row a byte off")
    assert len(launches) == 1 and launches[0][6] is True


def test_a_zero_length_row_off_alignment_keeps_the_vector_form(launches):
    lengths = (GROUP + 1, 0, 300)
    data, par, _ = vc.encode_case("c4_6", lengths, "cuda", shift={(1, 0): 3})
    VarlenCodec(fresh("c4_6")).encode(data.arg, par.arg)
    par.check("parity")
    assert launches[0][6] is False


def test_byte_form_forced_on_aligned_rows(launches):
    lengths = vc.LENGTHS[:-1]
    erased = vc.erasures("c9_14", len(lengths))
    stripes, _, _ = vc.repair_case("c9_14", lengths, erased, "cuda")
    plan = _plan(fresh("c9_14"), stripes, erased, force_bytewise=True)
    assert plan.bytewise and plan.nblk == sum(-(-c // BLOCK) for c, e in zip(lengths, erased) if e)
    plan.run()
    stripes.check("forced byte form")
    assert launches[0][6] is True


@pytest.mark.parametrize("lead", [16, 7])
def test_packed_form(lead, launches):
    """Offsets that are multiples of 16 only by chance (the lengths are not): the byte form; with every
    length a multiple of 16 and a 16-byte lead, the vector form."""
    code = "c10_14"
    rs = fresh(code)
    for lengths, vector in ((vc.LENGTHS[:-1], False), ((16, 0, 4096, 48, 4112), lead == 16)):
        del launches[:]
        data, par, _ = vc.encode_case(code, lengths, "cuda", packed=True, lead=lead)
        VarlenCodec(rs).encode(data.arg, par.arg, offsets=data.offsets)
        par.check(f"packed encode, lead {lead}")
        erased = vc.erasures(code, len(lengths))
        stripes, _, _ = vc.repair_case(code, lengths, erased, "cuda", packed=True, lead=lead)
        VarlenCodec(rs).reconstruct(stripes.arg, [list(e) for e in erased], offsets=torch.from_numpy(stripes.offsets))
        stripes.check(f"packed reconstruct, lead {lead}")
        assert [a[6] for a in launches] == [not vector, not vector]


def test_natives_with_parity_in_another_allocation():
    code, lengths = "c10_14", (17, 0, 4097, 300)
    rs = fresh(code)
    erased = ((0, 12), (1,), (13, 11, 2, 3), ())
    good = vc.consistent(code, lengths)
    bad = vc.damaged(good, erased)
    nat, par = vc.Batch(rs.k, lengths, "cuda"), vc.Batch(rs.p, lengths, "cuda")
    nat.put([b[: rs.k] for b in bad])
    par.put([b[rs.k:] for b in bad])
    nat.upload()
    par.upload()
    VarlenCodec(rs).reconstruct(nat.arg, [list(e) for e in erased], parity=par.arg)
    nat.put([g[: rs.k] for g in good])
    par.put([g[rs.k:] for g in good])
    nat.check("natives")
    par.check("parity")


# ---- 65,537 stripes in one launch ------------------------------------------------------------------
def test_65537_stripes_run_as_one_launch(launches):
    code, nb = "c10_14", 65537
    rs = fresh(code)
    lengths = np.random.default_rng(65537).integers(1, 2 * GROUP + 2, size=nb)
    assert lengths.min() == 1 and lengths.max() == 33
    total = int(lengths.sum())
    data = np.random.default_rng(1).integers(0, 256, size=(rs.k, total), dtype=np.uint8)
    good = np.concatenate([data, vc.gemm(code, rs.E, data)])
    batch = vc.Batch(rs.n, lengths, "cuda", packed=True)
    before = good.copy()
    before[rs.k:] = vc.FRESH
    batch.put_packed(before)
    batch.upload()
    codec = VarlenCodec(rs)
    codec.encode(batch.arg[: rs.k], batch.arg[rs.k:], offsets=batch.offsets)
    batch.put_packed(good)
    batch.check("65,537 stripes, encode")
    assert len(launches) == 1 and launches[0][3] == nb and launches[0][5] == nb
    # a repair with four patterns dealt over the stripes; stripe b loses rows PATTERNS[b % 4]
    patterns = np.array([[0, 13], [5, -1], [10, 2], [-1, -1]])
    erased = patterns[np.arange(nb) % 4]
    lost = np.zeros((rs.n, nb), dtype=bool)
    for q, ids in enumerate(patterns):
        lost[[i for i in ids if i >= 0], q::4] = True
    bad = np.where(np.repeat(lost, lengths, axis=1), vc.FRESH, good).astype(np.uint8)
    batch.put_packed(bad)
    batch.upload()
    codec.reconstruct(batch.arg, erased, offsets=batch.offsets)
    batch.put_packed(good)
    batch.check("65,537 stripes, reconstruct")
    assert len(launches) == 2 and launches[1][3] == nb - nb // 4


# ---- round trip, and what the launcher refuses --------------------------------------------------------
def test_round_trip_leaves_a_zero_syndrome():
    code, lengths = "c10_14", (4095, 17, 0, 8191, 300)
    rs = fresh(code)
    data, par, _ = vc.encode_case(code, lengths, "cuda")
    codec = VarlenCodec(rs)
    codec.encode(data.arg, par.arg)
    stripes = [d + p for d, p in zip(data.arg, par.arg)]
    erased = [[0, 13], [4], [1], [9, 10, 11, 2], []]
    for s, e in zip(stripes, erased):
        for i in e:
            s[i].fill_(0x3C)
    dirty = [bool(rs.syndrome_mask(s).any()) for s, c in zip(stripes, lengths) if c]
    assert dirty == [True, True, True, False]
    codec.reconstruct(stripes, erased)
    for s, c in zip(stripes, lengths):
        if c:
            assert not rs.syndrome_mask(s).any()
    par.check("parity after the round trip")
    data.check("data after the round trip")


def test_launcher_refusals_return_errors_and_write_nothing():
    lengths = (17, 300)
    erased = ((0,), (13,))
    stripes, _, _ = vc.repair_case("c10_14", lengths, erased, "cuda")
    stripes.image[:] = stripes.buf.cpu().numpy()
    plan = _plan(fresh("c10_14"), stripes, erased)
    d, k, mp, nb, npat, nblk = int(plan.desc.data_ptr()), plan.k, plan.m_pad, plan.batch, plan.npat, plan.nblk
    for name, args in {
        "null desc": (0, k, mp, nb, npat, nblk, False, 0),
        "batch 0": (d, k, mp, 0, npat, nblk, False, 0),
        "npat 0": (d, k, mp, nb, 0, nblk, False, 0),
        "k 0": (d, 0, mp, nb, npat, nblk, False, 0),
        "k 257": (d, 257, mp, nb, npat, nblk, False, 0),
        "m_pad 0": (d, k, 0, nb, npat, nblk, False, 0),
        "m_pad 3": (d, k, 3, nb, npat, nblk, False, 0),
        "m_pad 257": (d, k, 257, nb, npat, nblk, False, 0),
        "nblk -1": (d, k, mp, nb, npat, -1, False, 0),
        "nblk 2^31": (d, k, mp, nb, npat, 2 ** 31, False, 0),
        "max_blocks -1": (d, k, mp, nb, npat, nblk, False, -1),
    }.items():
        with pytest.raises(RuntimeError, match="invalid"):
            hip().varlen(*args)
    hip().varlen(d, k, mp, nb, npat, 0, False, 0)  # nblk == 0: success, no launch
    stripes.check("after the refusals")
    with pytest.raises(ValueError):
        ov.varlen_blocks([2 ** 43], False)  # 2^31 work items: refused on the host


def test_rows_on_mixed_devices_are_refused_and_nothing_is_written(launches):
    """One CPU row among the GPU rows of one stripe, one stripe wholly on the CPU, and the parity rows on
    the CPU: ValueError before any launch, the whole arena as it was."""
    code, lengths = "c10_14", (40, 300, 17)
    rs = fresh(code)
    codec = VarlenCodec(rs)
    erased = ((0,), (1, 12), (13,))
    stripes, _, _ = vc.repair_case(code, lengths, erased, "cuda")
    stripes.image[:] = stripes.buf.cpu().numpy()  # the damaged state, which must stay
    rows = [list(s) for s in stripes.arg]
    ids = [list(e) for e in erased]
    for what, kw in {
        "one row": dict(stripes=[rows[0], [r.cpu() if j == 3 else r for j, r in enumerate(rows[1])], rows[2]]),
        "one stripe": dict(stripes=[rows[0], rows[1], [r.cpu() for r in rows[2]]]),
        "the parity": dict(stripes=[r[: rs.k] for r in rows], parity=[[x.cpu() for x in r[rs.k:]] for r in rows]),
    }.items():
        with pytest.raises(ValueError, match="one device"):
            codec.reconstruct(erased=ids, **kw)
        stripes.check(f"reconstruct, {what} on the CPU")
    data, par, _ = vc.encode_case(code, lengths, "cuda")
    par.image[:] = par.buf.cpu().numpy()
    d, p = [list(s) for s in data.arg], [list(s) for s in par.arg]
    for what, args in {
        "one data row": ([d[0], [r.cpu() if j == 9 else r for j, r in enumerate(d[1])], d[2]], p),
        "one parity row": (d, [p[0], p[1], [r.cpu() if j == 0 else r for j, r in enumerate(p[2])]]),
        "the parity": (d, [[r.cpu() for r in x] for x in p]),
    }.items():
        with pytest.raises(ValueError, match="one device"):
            codec.encode(*args)
        par.check(f"encode, {what} on the CPU")
        data.check(f"encode, {what} on the CPU")
    packed, ppar, _ = vc.encode_case(code, lengths, "cuda", packed=True)
    ppar.image[:] = ppar.buf.cpu().numpy()
    with pytest.raises(ValueError, match="one device"):
        codec.encode(packed.arg, ppar.arg.cpu(), offsets=packed.offsets)
    ppar.check("packed encode, the parity on the CPU")
    assert not launches and not rs._plans


# ---- the plan cache ------------------------------------------------------------------------------------
def test_repeat_call_runs_the_cached_plan_without_an_upload(monkeypatch, launches):
    code, lengths = "c10_14", (300, 17, 4097)
    rs = fresh(code)
    codec = VarlenCodec(rs)
    built = []
    real_init = VarlenPlan.__init__
    monkeypatch.setattr(VarlenPlan, "__init__", lambda self, *a, **kw: (built.append(1), real_init(self, *a, **kw))[1])
    data, par, good = vc.encode_case(code, lengths, "cuda")
    erased = [[0], [12, 3], [5]]
    stripes, bad, _ = vc.repair_case(code, lengths, tuple(tuple(e) for e in erased), "cuda")
    codec.encode(data.arg, par.arg)
    codec.reconstruct(stripes.arg, erased)
    assert (len(built), len(launches), len(rs._plans)) == (2, 2, 2)
    desc = [p.desc.data_ptr() for p in rs._plans.values()]
    par.put([np.full((rs.p, c), vc.FRESH, dtype=np.uint8) for c in lengths])
    par.upload()
    par.put([g[rs.k:] for g in good])
    want = stripes.image.copy()
    stripes.put(bad)
    stripes.upload()
    stripes.image[:] = want
    codec.encode(data.arg, par.arg)
    codec.reconstruct(stripes.arg, erased)
    par.check("cached encode")
    stripes.check("cached reconstruct")
    assert (len(built), len(launches), len(rs._plans)) == (2, 4, 2)
    assert [p.desc.data_ptr() for p in rs._plans.values()] == desc
    # one erased id changed, then one length: both miss
    codec.reconstruct(stripes.arg, [[0], [12, 4], [5]])
    assert len(built) == 3
    shorter = [stripes.arg[0], [r[:16] for r in stripes.arg[1]], stripes.arg[2]]
    codec.reconstruct(shorter, erased)
    codec.encode([data.arg[0], [r[:16] for r in data.arg[1]], data.arg[2]],
                 [par.arg[0], [r[:16] for r in par.arg[1]], par.arg[2]])
    assert len(built) == 5 and len(rs._plans) == 5


# ---- stream order and graph capture ------------------------------------------------------------------------
STREAM_LENGTHS = (4097, 0, 17, 8191, 300)
STREAM_ERASED = ((1, 12), (3,), (), (0, 3, 5, 13), (7,))


class ArenaOf:
    """A ``varlen_cases.Batch`` as the arena the stream harness takes (``image``, ``buf``, ``upload``)."""

    def __init__(self, batch):
        self.batch, self.image, self.buf = batch, batch.image, batch.buf

    def upload(self, image=None):
        self.buf.copy_(torch.from_numpy(np.array(self.image if image is None else image)).to(self.buf.device))


def _entry(name, packed):
    code = "c10_14"

    def build(dev):
        rs = fresh(code)
        codec = VarlenCodec(rs)
        batch = vc.Batch(rs.n, STREAM_LENGTHS, dev, packed=packed, lead=16)
        kw = batch.kw()
        if packed:
            natives, parity = batch.arg[: rs.k], batch.arg[rs.k:]
        else:
            natives, parity = [s[: rs.k] for s in batch.arg], [s[rs.k:] for s in batch.arg]

        def fill(seed):
            good = vc.consistent(code, STREAM_LENGTHS, seed)
            batch.put(vc.damaged(good, [tuple(range(rs.k, rs.n))] * len(good) if name == "encode" else STREAM_ERASED))

        def expect(seed):
            batch.put(vc.consistent(code, STREAM_LENGTHS, seed))
            return [], {}

        def call(s):
            if name == "encode":
                codec.encode(natives, parity, stream=s, **kw)
            else:
                codec.reconstruct(batch.arg, [list(e) for e in STREAM_ERASED], stream=s, **kw)
            return [], {}
        return sc.Built(ArenaOf(batch), fill, expect, call)
    api = (f"VarlenCodec.{name}", "VarlenPlan.run")
    return sc.Entry(f"varlen_{name}_{'packed' if packed else 'list'}", api, build, nosync=True, capture=True)


ENTRIES = {e.name: e for e in (_entry(n, p) for n in ("encode", "reconstruct") for p in (False, True))}


@pytest.mark.parametrize("spelling", ["arg", "current"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_cached_call_is_ordered_on_its_stream_and_makes_no_host_sync(name, spelling):
    sc.gated(ENTRIES[name], spelling)


@pytest.mark.parametrize("spelling", ["arg", "current"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_first_call_is_ordered_on_its_stream(name, spelling):
    sc.gated(ENTRIES[name], spelling, first=True)


def test_harness_catches_a_varlen_call_on_another_stream():
    with pytest.raises(AssertionError, match="arena differ|result"):
        sc.gated(ENTRIES["varlen_encode_list"], "arg", fault="stream")


@pytest.mark.parametrize("spelling", ["arg", "current"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_cached_call_is_captured_and_replays_on_fresh_data(name, spelling, launches):
    """Three replays on fresh data with an eager call in between. What is asserted: the results of every
    replay, and that the captured call reached the launcher exactly once. The graph's nodes are not
    inspected (the harness does not expose them): that it is a single chain follows from the cached
    call enqueuing that one launch and nothing else on the capturing stream, which is argued from the
    code of ``VarlenPlan.run`` (no copy, no memset; the plan's ready event was consumed by the warm-up
    call), not observed."""
    sc.captured(ENTRIES[name], spelling)
    # warm-up, the captured call, the eager call between the replays
    assert len(launches) == 3

"""The scrub of variable-length batches on the GPU (``csrc/kernels/gf_varlen_scrub.hip`` through
``VarlenCodec.syndrome_mask`` / ``scrub`` / ``heal`` and ``ops.varlen.VarlenScrubPlan``): the cases of
tests/varlen_scrub_cases.py against ``gf.scrub_oracle`` stripe by stripe, the flat grids when they stride,
the byte form, 65,537 stripes in one launch, the launchers called directly, the plan cache, stream order
and graph capture, a round trip through ``heal``, and addressing past 2^32.

All rows are views of one guard-filled arena: the guard value right after each row is nonzero, so a read
past ``len[b]`` shows as a dirty bit the oracle does not have, and after every call the whole arena must
equal its host image (a scrub reads only). In every damaged batch the words and counts of every OTHER
stripe must be zero: what a wrong ``mask_first`` or ``first_span`` would break. Comparisons are exact.
Nothing here provokes a fault: what the launchers must refuse is refused on the host before any launch.

Stream order and capture use the harness of tests/stream_cases.py (``gated`` / ``captured``) with entries
of this file's own: its table lists the entry points of ``ReedSolomon`` and ``ops.__all__`` only.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc
import varlen_cases as vc
import varlen_scrub_cases as sv
from gpu_rscode_amd import ReedSolomon, VarlenCodec, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import varlen as ov
from gpu_rscode_amd.ops.varlen import BLOCK, GROUP, VarlenScrubPlan
from test_varlen_scrub import heal_case, repairs  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
FULL = vc.FULL


@pytest.fixture
def launches(monkeypatch):
    """The launches of the two kernels (calls of the bindings that reach the launchers): name and arguments."""
    calls = []

    class Counting:
        def __getattr__(self, name):
            real = getattr(hip(), name)
            if name not in ("varlen_syndrome", "varlen_locate"):
                return real

            def counted(*a):
                calls.append((name, a))
                return real(*a)
            return counted
    monkeypatch.setattr(ov, "hip", lambda: Counting())
    return calls


def plan_of(code, batch, block_bytes=4096, **kw) -> VarlenScrubPlan:
    rows = sv.rows_of(batch)
    ptrs = np.array([[r.data_ptr() for r in rows(b)] for b in range(len(batch.lengths))], dtype=np.uint64)
    return VarlenScrubPlan(ptrs, batch.lengths, sv.codec(code).H, "cuda", block_bytes, **kw)


# ---- every code, the batches of encode, every block size ---------------------------------------------------
@pytest.mark.parametrize("batch", ["b1", "b2", "b3", "b257"])
@pytest.mark.parametrize("code", list(sv.LOCATING))
def test_damage(code, batch, launches):
    for bb in sv.BLOCKS:
        del launches[:]
        sv.run_damage("cuda", code, vc.BATCHES[batch], bb, True)
        # per damage case: syndrome_mask is one launch, scrub two; the single-stripe calls are not these kernels
        assert [name for name, _ in launches] == ["varlen_syndrome", "varlen_syndrome", "varlen_locate"] * 3
        assert all(a[7] is False for _, a in launches), "aligned rows run the vector form"


@pytest.mark.parametrize("batch", ["zero-first", "zero-middle", "zero-last", "ladder", "one-long-among-256"])
def test_damage_with_zero_length_stripes_and_the_ladder(batch):
    for bb in sv.BLOCKS:
        sv.run_damage("cuda", "c10_14", vc.BATCHES[batch], bb, True)


def test_a_batch_of_zero_length_stripes_launches_nothing(launches):
    rs = sv.fresh("c10_14")
    vl = VarlenCodec(rs)
    batch = sv.upload("c10_14", sv.consistent("c10_14", (0, 0, 0)), "cuda")
    m = vl.syndrome_mask(batch.arg)
    assert m.blocks.shape == (0,) and m.offsets.tolist() == [0, 0, 0, 0] and m.stripes.cpu().tolist() == [0, 0, 0]
    rep = vl.scrub(batch.arg)
    assert rep.clean.all() and rep.votes.shape == (3, 14) and not launches and not rs._plans
    assert vl.heal(batch.arg).dirty == []


@pytest.mark.parametrize("code", list(sv.LOCATING))
def test_single_flipped_bytes(code):
    n = sv.codec(code).n
    for bb in sv.BLOCKS:
        assert sv.flip_sweep("cuda", code, bb) == 8 * n


@pytest.mark.parametrize("code", ["c10_14", "c3_19"])
def test_every_error_value(code):
    for bb in sv.BLOCKS:
        sv.error_values("cuda", code, bb)


@pytest.mark.parametrize("code", list(sv.MASK_ONLY))
def test_codes_past_the_locate_tile_run_syndrome_mask_only(code):
    rs = sv.codec(code)
    assert rs.p > 16
    batches = [vc.WIDE_BATCH] if code == "c128_160" else [vc.BATCHES[b] for b in ("b1", "b2", "zero-middle", "b3")]
    for lengths in batches:
        sv.run_damage("cuda", code, lengths, 4096, False)
    for bb in sv.BLOCKS[1:]:
        sv.run_damage("cuda", code, batches[-1], bb, False)
    if code == "c19_36":
        assert sv.flip_sweep("cuda", code, 4096, locate=False) == 8 * rs.n
    batch = sv.upload(code, sv.consistent(code, vc.WIDE_BATCH), "cuda")
    with pytest.raises(NotImplementedError, match="p <= 16"):
        VarlenCodec(rs).scrub(batch.arg)
    with pytest.raises(NotImplementedError, match="p <= 16"):
        VarlenCodec(rs).heal(batch.arg)
    batch.check("refused")


# ---- launch shapes --------------------------------------------------------------------------------------------
def dirty_batch(code, lengths, hit, device="cuda", **kw):
    """(batch, its damaged stripes): one overwritten chunk, and a flipped last byte, in the stripes ``hit``."""
    good = sv.consistent(code, tuple(lengths))
    n = sv.codec(code).n
    bad = {}
    for b in hit:
        if not lengths[b]:
            continue
        a = sv.overwritten(good, b, (b + 2) % n) if b % 2 else np.array(good[b])
        a[(3 * b) % n, -1] ^= 0x80 >> (b % 8)
        bad[b] = a
    return sv.upload(code, [bad.get(b, good[b]) for b in range(len(good))], device, **kw), bad


@pytest.mark.parametrize("laps", [1, 2, 3])
@pytest.mark.parametrize("max_blocks", [1, 2, 3, 8])
def test_capped_grids_stride_over_the_work_items(max_blocks, laps, launches):
    """nblk one above ``laps`` laps of ``max_blocks`` workgroups: a stripe of two blocks first, then stripes
    of one block each, so one workgroup's lap holds items of several stripes; the cold pass strides too."""
    nblk = max_blocks * laps + 1
    short = (GROUP + 1, 300, 1, (BLOCK - 1) * GROUP, 48, 777)
    lengths = (FULL + 1,) + tuple(short[i % len(short)] for i in range(nblk - 2))
    hit = sorted({0, len(lengths) // 2, len(lengths) - 1})
    batch, bad = dirty_batch("c10_14", lengths, hit)
    plan = plan_of("c10_14", batch)
    nspan = len(lengths) + 1  # (spans of 4096 columns: the first stripe has two)
    assert plan.nblk == nblk and plan.nspan == nspan and not plan.bytewise
    want = sv.damaged_oracle("c10_14", lengths, 4096, bad)
    what = f"max_blocks {max_blocks}, {laps} laps"
    sv.check_mask(what, plan.syndrome_mask(max_blocks=max_blocks), want)
    sv.check_report(what, plan.scrub(max_blocks=max_blocks), want)
    batch.check(what)
    assert [(name, a[5], a[8]) for name, a in launches] == [
        ("varlen_syndrome", nblk, max_blocks), ("varlen_syndrome", nblk, max_blocks), ("varlen_locate", nspan, max_blocks)]


@pytest.mark.parametrize("code", ["c10_14", "c9_14"])
def test_one_row_off_alignment_puts_the_batch_on_the_byte_form(code, launches):
    lengths = vc.LENGTHS[:-1]
    batch, bad = dirty_batch(code, lengths, (1, 5, 10), shift={(5, 2): 1})
    rs = sv.fresh(code)
    want = sv.damaged_oracle(code, lengths, 4096, bad)
    sv.check_report("one row a byte off", VarlenCodec(rs).scrub(batch.arg, block_bytes=4096), want)
    sv.check_single("one row a byte off", rs, VarlenCodec(rs).scrub(batch.arg, block_bytes=4096), sv.rows_of(batch),
                    (5, 10), 4096)
    batch.check("one row a byte off")
    assert all(a[7] is True for _, a in launches) and len(launches) == 4


@pytest.mark.parametrize("code", ["c10_14", "c3_19", "c19_36"])
def test_byte_form_forced_on_aligned_rows(code, launches):
    lengths = vc.LENGTHS[:-1]
    batch, bad = dirty_batch(code, lengths, (1, 6, 10))
    plan = plan_of(code, batch, force_bytewise=True)
    assert plan.bytewise and plan.nblk == sum(-(-c // BLOCK) for c in lengths)
    want = sv.damaged_oracle(code, lengths, 4096, bad)
    sv.check_mask("forced byte form", plan.syndrome_mask(), want)
    sv.check_mask("forced byte form, capped", plan.syndrome_mask(max_blocks=3), want)
    if plan.p <= 16:
        sv.check_report("forced byte form", plan.scrub(), want)
    batch.check("forced byte form")
    assert all(a[7] is True for _, a in launches)


@pytest.mark.parametrize("lead", [16, 7])
def test_packed_form(lead, launches):
    """Offsets that are multiples of 16 only by chance (the lengths are not): the byte form; with every
    length a multiple of 16 and a 16-byte lead, the vector form."""
    code = "c10_14"
    rs = sv.fresh(code)
    for lengths, vector in ((vc.LENGTHS[:-1], False), ((16, 0, 4096, 48, 4112), lead == 16)):
        del launches[:]
        batch, bad = dirty_batch(code, lengths, (0, 2, 4), packed=True, lead=lead)
        want = sv.damaged_oracle(code, lengths, 4096, bad)
        rep = VarlenCodec(rs).scrub(batch.arg, offsets=torch.from_numpy(batch.offsets), block_bytes=4096)
        sv.check_report(f"packed, lead {lead}", rep, want)
        sv.check_mask(f"packed, lead {lead}", VarlenCodec(rs).syndrome_mask(batch.arg, offsets=batch.offsets, block_bytes=4096),
                      want)
        batch.check(f"packed, lead {lead}")
        assert [a[7] for _, a in launches] == [not vector] * 3


def test_a_zero_length_row_off_alignment_keeps_the_vector_form(launches):
    lengths = (GROUP + 1, 0, 300)
    batch, bad = dirty_batch("c4_6", lengths, (2,), shift={(1, 0): 3})
    sv.check_report("zero-length row off alignment", VarlenCodec(sv.fresh("c4_6")).scrub(batch.arg),
                    sv.damaged_oracle("c4_6", lengths, 65536, bad))
    assert [a[7] for _, a in launches] == [False, False]


def test_natives_with_parity_in_another_allocation():
    code, lengths = "c10_14", (17, 0, 4097, 300)
    rs = sv.fresh(code)
    good = sv.consistent(code, lengths)
    bad = {0: sv.overwritten(good, 0, 12), 2: sv.overwritten(good, 2, 3)}
    stripes = [bad.get(b, good[b]) for b in range(4)]
    nat, par = vc.Batch(rs.k, lengths, "cuda"), vc.Batch(rs.p, lengths, "cuda")
    nat.put([s[: rs.k] for s in stripes])
    par.put([s[rs.k:] for s in stripes])
    nat.upload()
    par.upload()
    rep = VarlenCodec(rs).scrub(nat.arg, parity=par.arg, block_bytes=4096)
    sv.check_report("natives and parity", rep, sv.damaged_oracle(code, lengths, 4096, bad))
    assert rep.report[0].suspects == [12] and rep.report[2].suspects == [3]
    nat.check("natives")
    par.check("parity")


# ---- 65,537 stripes in one launch -----------------------------------------------------------------------------
def test_65537_stripes_run_as_one_launch(launches):
    code, nb = "c10_14", 65537
    rs = sv.fresh(code)
    lengths = np.random.default_rng(65537).integers(1, 2 * GROUP + 2, size=nb)
    assert lengths.min() == 1 and lengths.max() == 33
    ends = np.cumsum(lengths)
    total = int(ends[-1])
    data = np.random.default_rng(1).integers(0, 256, size=(rs.k, total), dtype=np.uint8)
    full = np.concatenate([data, vc.gemm(code, rs.E, data)])
    # the undamaged batch: one oracle over all the columns side by side is zero, so every stripe's is
    assert gf.scrub_oracle(rs.H, full, 4096)[3] == 0
    dirty = [0, 1, 4097, 32768, 65535, 65536]
    want = sv.Want(rs.n, lengths, 4096)
    for i, b in enumerate(dirty):
        full[(3 * i) % rs.n, ends[b] - 1 - (i % int(lengths[b]))] ^= 1 + i
        want.set(b, full[:, ends[b] - lengths[b]: ends[b]], rs.H)
    batch = vc.Batch(rs.n, lengths, "cuda", packed=True)
    batch.put_packed(full)
    batch.upload()
    vl = VarlenCodec(rs)
    sv.check_mask("65,537 stripes", vl.syndrome_mask(batch.arg, offsets=batch.offsets, block_bytes=4096), want)
    rep = vl.scrub(batch.arg, offsets=batch.offsets, block_bytes=4096)
    sv.check_report("65,537 stripes", rep, want)
    assert rep.dirty == dirty
    batch.check("65,537 stripes")
    assert [(name, a[4], a[5]) for name, a in launches] == [("varlen_syndrome", nb, nb)] * 2 + [("varlen_locate", nb, nb)]


# ---- the launchers, called directly -----------------------------------------------------------------------------
FILL32, FILL64, GUARDW = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 8


class Launch:
    """A valid plan of a dirty batch, with 0x5A-filled mask and counts buffers that carry guard words
    around the [nwords + B] and [B * (n + 2)] ranges."""

    def __init__(self, code="c4_6", lengths=(FULL + 17, 0, 300)):
        self.code, self.lengths = code, lengths
        self.batch, self.bad = dirty_batch(code, lengths, (0, len(lengths) - 1))
        self.plan = p = plan_of(code, self.batch)
        self.mask = torch.full((GUARDW + p.nwords + p.batch + GUARDW,), FILL32, dtype=torch.int32, device="cuda")
        self.counts = torch.full((GUARDW + p.batch * (p.n + 2) + GUARDW,), FILL64, dtype=torch.int64, device="cuda")
        self.loc = p.loc if p.loc is not None else torch.zeros(p.p * p.n + 2 * p.n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def syndrome_args(self, **kw):
        p = self.plan
        a = dict(desc=int(p.desc.data_ptr()), n=p.n, m_pad=p.m_pad, ident=p.ident, batch=p.batch, nblk=p.nblk,
                 block_bytes=4096, bytewise=False, max_blocks=0, mask=int(self.mask.data_ptr()) + 4 * GUARDW,
                 nwords=p.nwords, stream=torch.cuda.current_stream().cuda_stream)
        a.update(kw)
        return a

    def locate_args(self, **kw):
        p = self.plan
        a = dict(desc=int(p.desc.data_ptr()), n=p.n, p=p.p, batch=p.batch, nblk=p.nblk, nspan=p.nspan, block_bytes=4096,
                 bytewise=False, max_blocks=0, mask=int(self.mask.data_ptr()) + 4 * GUARDW, loc=int(self.loc.data_ptr()),
                 locatable=True, counts=int(self.counts.data_ptr()) + 8 * GUARDW,
                 stream=torch.cuda.current_stream().cuda_stream)
        a.update(kw)
        return a

    def refused(self, which, **kw):
        with pytest.raises(RuntimeError, match=f"gf_varlen_{which}"):
            if which == "syndrome":
                hip().varlen_syndrome(**self.syndrome_args(**kw))
            else:
                hip().varlen_locate(**self.locate_args(**kw))
        torch.cuda.synchronize()
        assert (self.mask.cpu().numpy() == FILL32).all() and (self.counts.cpu().numpy() == FILL64).all(), (which, kw)


def test_launchers_write_their_ranges_only():
    r = Launch()
    p = r.plan
    hip().varlen_syndrome(**r.syndrome_args())
    hip().varlen_locate(**r.locate_args())
    torch.cuda.synchronize()
    mask, counts = r.mask.cpu().numpy(), r.counts.cpu().numpy()
    for buf, fill in ((mask, FILL32), (counts, FILL64)):
        assert (buf[:GUARDW] == fill).all() and (buf[-GUARDW:] == fill).all()
    want = sv.damaged_oracle(r.code, r.lengths, 4096, r.bad)
    assert want.bad[0] and want.bad[2] and not want.bad[1]
    assert np.array_equal(mask[GUARDW: GUARDW + p.nwords], want.blocks)
    assert np.array_equal(mask[GUARDW + p.nwords: -GUARDW], want.stripes)
    got = counts[GUARDW:-GUARDW].reshape(p.batch, p.n + 2)
    assert np.array_equal(got[:, : p.n], want.votes)
    assert np.array_equal(got[:, p.n], want.unlocated) and np.array_equal(got[:, p.n + 1], want.bad)
    r.batch.check("the launchers")
    # nblk == 0 / nspan == 0: the memsets, no launch
    r.mask.fill_(FILL32)
    r.counts.fill_(FILL64)
    hip().varlen_syndrome(**r.syndrome_args(nblk=0))
    hip().varlen_locate(**r.locate_args(nspan=0))
    torch.cuda.synchronize()
    assert not r.mask.cpu().numpy()[GUARDW:-GUARDW].any() and not r.counts.cpu().numpy()[GUARDW:-GUARDW].any()
    assert (r.mask.cpu().numpy()[:GUARDW] == FILL32).all() and (r.counts.cpu().numpy()[-GUARDW:] == FILL64).all()


def test_launchers_refuse_bad_arguments_and_store_nothing():
    r = Launch()  # (4, 6): m_pad = 2
    for kw in (dict(desc=0), dict(mask=0), dict(batch=0), dict(batch=-1), dict(n=0), dict(n=257), dict(m_pad=0),
               dict(m_pad=3), dict(m_pad=24), dict(m_pad=272), dict(ident=3), dict(ident=-1), dict(block_bytes=2048),
               dict(block_bytes=12288), dict(block_bytes=0), dict(nblk=-1), dict(nblk=2 ** 31), dict(nwords=-1),
               dict(max_blocks=-1)):
        r.refused("syndrome", **kw)
    for kw in (dict(desc=0), dict(mask=0), dict(loc=0), dict(counts=0), dict(batch=0), dict(p=0), dict(p=6), dict(p=17),
               dict(n=257), dict(block_bytes=2048), dict(block_bytes=12288), dict(nblk=-1), dict(nblk=2 ** 31),
               dict(nspan=-1), dict(nspan=2 ** 31), dict(max_blocks=-1)):
        r.refused("locate", **kw)
    tall = Launch("c19_36", (17, 300))  # p = 17: beyond the locate kernel's tile
    assert (tall.plan.p, tall.plan.m_pad) == (17, 32)
    tall.refused("locate")
    r.batch.check("after the refusals")
    for call in (ov.varlen_spans, ov.mask_offsets):
        with pytest.raises(ValueError):
            call([17], 2048)


# ---- the plan cache ------------------------------------------------------------------------------------------------
def test_repeat_call_runs_the_cached_plan_without_an_upload(monkeypatch, launches):
    code, lengths = "c10_14", (300, 17, 4097)
    rs = sv.fresh(code)
    vl = VarlenCodec(rs)
    built, uploads = [], []
    real_init, real_from = VarlenScrubPlan.__init__, torch.from_numpy
    monkeypatch.setattr(VarlenScrubPlan, "__init__", lambda self, *a, **kw: (built.append(1), real_init(self, *a, **kw))[1])
    batch, bad = dirty_batch(code, lengths, (1,))
    monkeypatch.setattr(ov.torch, "from_numpy", lambda a: (uploads.append(a.size), real_from(a))[1])
    want = sv.damaged_oracle(code, lengths, 65536, bad)
    sv.check_mask("first", vl.syndrome_mask(batch.arg), want)
    assert (len(built), len(rs._plans)) == (1, 1) and len(uploads) == 2  # the record and the locate operand
    desc = next(iter(rs._plans.values())).desc.data_ptr()
    del uploads[:]
    sv.check_mask("cached", vl.syndrome_mask(batch.arg), want)
    sv.check_report("cached", vl.scrub(batch.arg), want)  # the same plan serves both calls
    assert (len(built), len(rs._plans), uploads) == (1, 1, [])
    assert next(iter(rs._plans.values())).desc.data_ptr() == desc and len(launches) == 4
    plan = next(iter(rs._plans.values()))
    assert not any(isinstance(v, torch.Tensor) and v.dtype == torch.uint8 and v.data_ptr() == batch.buf.data_ptr()
                   for v in vars(plan).values())  # raw addresses only
    # another block size, one length changed: both miss
    vl.syndrome_mask(batch.arg, block_bytes=4096)
    vl.syndrome_mask([batch.arg[0], [r[:16] for r in batch.arg[1]], batch.arg[2]])
    assert len(built) == 3 and len(rs._plans) == 3


# ---- heal, and a round trip ----------------------------------------------------------------------------------------
def test_heal(repairs):  # noqa: F811
    heal_case("cuda", repairs)


def test_round_trip_encode_damage_heal_leaves_a_zero_syndrome():
    code, lengths = "c10_14", (4095, 17, 0, 8191, 300)
    rs = sv.fresh(code)
    vl = VarlenCodec(rs)
    data, par, good = vc.encode_case(code, lengths, "cuda")
    vl.encode(data.arg, par.arg)
    stripes = [d + p for d, p in zip(data.arg, par.arg)]
    for b, j in ((0, 13), (1, 4), (3, 9)):
        stripes[b][j].fill_(0x3C)
    first = vl.scrub(stripes, block_bytes=4096)
    assert first.dirty == [0, 1, 3] and [first.report[b].suspects for b in (0, 1, 3)] == [[13], [4], [9]]
    for b, c in enumerate(lengths):
        if c:
            assert torch.equal(first.report[b].mask, rs.syndrome_mask(stripes[b], block_bytes=4096)), b
    rep = vl.heal(stripes, report=first)
    assert rep.clean.all() and rep.unhealed == []
    m = vl.syndrome_mask(stripes)
    assert not m.blocks.any() and not m.stripes.any()
    par.check("parity after the round trip")
    data.check("data after the round trip")


# ---- stream order and graph capture ----------------------------------------------------------------------------------
STREAM_LENGTHS = (4097, 0, 17, 8191, 300)


class ArenaOf:
    """A ``varlen_cases.Batch`` as the arena the stream harness takes (``image``, ``buf``, ``upload``)."""

    def __init__(self, batch):
        self.batch, self.image, self.buf = batch, batch.image, batch.buf

    def upload(self, image=None):
        self.buf.copy_(torch.from_numpy(np.array(self.image if image is None else image)).to(self.buf.device))


def _stripes(seed):
    good = sv.consistent("c10_14", STREAM_LENGTHS, seed)
    if seed % 2:
        return list(good), {}
    bad = {3: np.array(good[3]), 4: sv.overwritten(good, 4, seed % 14, seed)}
    bad[3][2, 8190] ^= 0x40
    return [bad.get(b, good[b]) for b in range(len(good))], bad


def _entry(name, packed):
    code = "c10_14"

    def build(dev):
        rs = sv.fresh(code)
        vl = VarlenCodec(rs)
        batch = vc.Batch(rs.n, STREAM_LENGTHS, dev, packed=packed, lead=16)
        kw = batch.kw()

        def fill(seed):
            batch.put(_stripes(seed)[0])

        def expect(seed):
            want = sv.damaged_oracle(code, STREAM_LENGTHS, 4096, _stripes(seed)[1], seed)
            if name == "syndrome_mask":
                return [want.blocks, want.stripes], {}
            return [want.blocks], {"bad_columns": want.bad.tolist(), "votes": want.votes.tolist()}

        def call(s):
            if name == "syndrome_mask":
                m = vl.syndrome_mask(batch.arg, block_bytes=4096, stream=s, **kw)
                return [m.blocks, m.stripes], {}
            rep = vl.scrub(batch.arg, block_bytes=4096, stream=s, **kw)
            return [rep.mask.blocks], {"bad_columns": rep.bad_columns.tolist(), "votes": rep.votes.tolist()}
        return sc.Built(ArenaOf(batch), fill, expect, call)
    sync = name == "scrub"
    api = (f"VarlenCodec.{name}", f"VarlenScrubPlan.{name}")
    return sc.Entry(f"varlen_{name}_{'packed' if packed else 'list'}", api, build, nosync=not sync, capture=not sync,
                    why=sc.SYNCS if sync else "")


ENTRIES = {e.name: e for e in (_entry(n, p) for n in ("syndrome_mask", "scrub") for p in (False, True))}
MASKS = [n for n in ENTRIES if "syndrome_mask" in n]


@pytest.mark.parametrize("spelling", ["arg", "current"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_cached_call_is_ordered_on_its_stream_and_syndrome_mask_makes_no_host_sync(name, spelling):
    sc.gated(ENTRIES[name], spelling)


@pytest.mark.parametrize("spelling", ["arg", "current"])
@pytest.mark.parametrize("name", list(ENTRIES))
def test_first_call_is_ordered_on_its_stream(name, spelling):
    sc.gated(ENTRIES[name], spelling, first=True)


def test_harness_catches_a_call_on_another_stream():
    with pytest.raises(AssertionError, match="arena differ|result"):
        sc.gated(ENTRIES["varlen_syndrome_mask_list"], "arg", fault="stream")


@pytest.mark.parametrize("spelling", ["arg", "current"])
@pytest.mark.parametrize("name", MASKS)
def test_cached_syndrome_mask_is_captured_and_replays_on_fresh_data(name, spelling, launches):
    """Three replays on fresh data (clean and dirty seeds) with an eager call in between; the captured call
    reached the launcher once: the graph holds its memset and its one launch."""
    assert {s % 2 for s in sc.REPLAYS} == {0, 1}, "the replays see clean and dirty batches"
    sc.captured(ENTRIES[name], spelling)
    assert [n for n, _ in launches] == ["varlen_syndrome"] * 3  # warm-up, the captured call, the eager call


# ---- addressing past 2^32 ---------------------------------------------------------------------------------------------
def test_addressing_past_2_to_32():
    """One packed [2, 2^32 + 8192] tensor as the Cauchy RS(1, 2) code (E = [1]: the parity row is a copy
    of the data row), offsets [0, 4096, 2^32 + 4096, 2^32 + 8192]: the middle stripe has 2^20 column
    blocks and crosses column 2^32 of the tensor. The expected words come from the closed form: with
    E = [1] a flipped byte at column c sets bit 0 of its stripe's word c >> 16 and is one bad, unlocated
    column. Needs about 9 GiB of device memory."""
    need = 2 * (2 ** 32 + 8192) + (1 << 29)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need >> 20} MiB of device memory, {free >> 20} MiB are free")
    rs = ReedSolomon(1, 2, matrix="cauchy")
    assert rs.E.tolist() == [[1]]
    width, bb = 2 ** 32 + 8192, 65536
    t = torch.empty((2, width), dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for lo in range(0, width, step):
        hi = min(width, lo + step)
        t[0, lo:hi] = torch.randint(0, 256, (hi - lo,), dtype=torch.uint8, device="cuda")
    t[1].copy_(t[0])
    offsets = np.array([0, 4096, 2 ** 32 + 4096, 2 ** 32 + 8192], dtype=np.int64)
    flips = [(1, 2 ** 31 - 1), (1, 2 ** 31 + 7), (1, 2 ** 32 - 4097), (1, 2 ** 32 - 1), (2, 77)]
    # stripe column 2^32 - 4097 is tensor column 2^32 - 1, stripe column 2^32 - 1 the stripe's last byte
    for i, (b, c) in enumerate(flips):
        t[i % 2, int(offsets[b]) + c] ^= 1 + i
    nwords = [1, 65536, 1]
    want = [np.zeros(w, dtype=np.int32) for w in nwords]
    bad = np.zeros(3, dtype=np.int64)
    for b, c in flips:
        want[b][c >> 16] = 1
        bad[b] += 1
    vl = VarlenCodec(rs)
    m = vl.syndrome_mask(t, offsets=offsets, block_bytes=bb)
    assert m.offsets.tolist() == [0, 1, 65537, 65538]
    assert np.array_equal(m.blocks.cpu().numpy(), np.concatenate(want)), np.flatnonzero(m.blocks.cpu().numpy())
    assert m.stripes.cpu().tolist() == [0, 1, 1]
    rep = vl.scrub(t, offsets=offsets, block_bytes=bb)
    assert np.array_equal(rep.mask.blocks.cpu().numpy(), np.concatenate(want))
    assert rep.bad_columns.tolist() == bad.tolist() == [0, 4, 1] and rep.unlocated.tolist() == [0, 4, 1]
    assert not rep.votes.any() and rep.dirty == [1, 2]
    # a scrub reads only: the two rows still differ in exactly the flipped bytes
    differ = 0
    for lo in range(0, width, step):
        differ += int((t[0, lo: lo + step] != t[1, lo: lo + step]).sum())
    assert differ == len(flips)
    for i, (b, c) in enumerate(flips):
        x = int(offsets[b]) + c
        assert int(t[0, x] ^ t[1, x]) == 1 + i

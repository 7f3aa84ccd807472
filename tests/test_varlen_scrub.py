"""The scrub of variable-length batches without a GPU: the descriptor layout against the C++ one, the two
work lists and the mask offsets, a numpy replay of the hot kernel's lane and mask-word rules, and
``VarlenCodec.syndrome_mask`` / ``scrub`` / ``heal`` on CPU tensors against ``gf.scrub_oracle`` and against
``ReedSolomon.scrub`` stripe by stripe (tests/varlen_scrub_cases.py)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import varlen_cases as vc
import varlen_scrub_cases as sv
from gpu_rscode_amd import ReedSolomon, VarlenCodec
from gpu_rscode_amd._native import cpu
from gpu_rscode_amd.ops import varlen as ov
from gpu_rscode_amd.ops.varlen import BLOCK, GROUP, VarlenMask, VarlenScrubReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the record and the work lists ----------------------------------------------------------------------
def test_layout_equals_the_cpp_layout():
    for n, mp, batch, nblk, nspan in itertools.product((1, 2, 14, 19, 160, 256), (1, 2, 4, 8, 16, 32, 256),
                                                      (1, 2, 3, 257, 65537), (0, 1, 7, 2 ** 31 - 1), (0, 1, 5, 2 ** 31 - 1)):
        got, want = ov.varlen_scrub_layout(n, mp, batch, nblk, nspan), cpu().varlen_scrub_layout(n, mp, batch, nblk, nspan)
        assert got == want, (n, mp, batch, nblk, nspan, got, want)
        assert got["tab_off"] % 32 == 0 and got["len_off"] % 8 == 0 and got["blk_off"] % 4 == 0


def test_the_descriptor_holds_what_it_is_given():
    lengths = np.array([17, 0, 4097], dtype=np.int64)
    ptrs = np.arange(3 * 6, dtype=np.uint64).reshape(3, 6) * np.uint64(4096) + np.uint64(1 << 40)
    _, first, blk = ov.varlen_blocks(lengths, False)
    _, sfirst, span = ov.varlen_spans(lengths, 4096)
    off = ov.mask_offsets(lengths, 4096)
    tables = np.arange(6 * 2 * 8, dtype=np.uint32).reshape(6, 2, 8)
    buf = ov.build_varlen_scrub_desc(ptrs, lengths, first, sfirst, off[:-1], blk, span, tables)
    lay = ov.varlen_scrub_layout(6, 2, 3, blk.size, span.size)
    assert buf.size == lay["bytes"] and buf[:16].view("<i4").tolist() == [6, 2, 3, 0]

    def at(name, dt, count):
        return buf[lay[name]: lay[name] + count * np.dtype(dt).itemsize].view(dt)
    assert np.array_equal(at("in_off", "<u8", 18), ptrs.reshape(-1))
    assert at("len_off", "<i8", 3).tolist() == [17, 0, 4097]
    assert at("first_off", "<i8", 3).tolist() == first.tolist() == [0, 1, 1]
    assert at("span_first_off", "<i8", 3).tolist() == sfirst.tolist() == [0, 1, 1]
    assert at("mask_first_off", "<i8", 3).tolist() == [0, 1, 1]
    assert np.array_equal(at("tab_off", "<u4", 96), tables.reshape(-1))
    assert at("blk_off", "<i4", blk.size).tolist() == [0, 2, 2]
    assert at("span_off", "<i4", span.size).tolist() == [0, 2, 2]


@pytest.mark.parametrize("block_bytes", [4096, 8192, 16384, 65536])
def test_varlen_spans_names_every_stripe_and_span_once_and_in_order(block_bytes):
    span = min(block_bytes, 16384)
    for lengths in list(vc.BATCHES.values()) + [(16384, 16385, 0, 32768, 65539)]:
        ns, first, stripe = ov.varlen_spans(lengths, block_bytes)
        want = [(b, s) for b, c in enumerate(lengths) for s in range(-(-c // span))]
        assert [(int(b), w - int(first[b])) for w, b in enumerate(stripe)] == want
        assert stripe.dtype == np.int32 and ns.tolist() == [-(-c // span) for c in lengths]
        # every column of every stripe lies in exactly one of its spans, none past its end
        for b, c in enumerate(lengths):
            assert ns[b] * span >= c > (ns[b] - 1) * span or (c == 0 and ns[b] == 0)
    with pytest.raises(ValueError):
        ov.varlen_spans([3, -1], block_bytes)
    with pytest.raises(ValueError):
        ov.varlen_spans([2 ** 46], block_bytes)  # 2^32 spans: refused on the host


@pytest.mark.parametrize("block_bytes", [4096, 65536])
def test_mask_offsets_equal_their_closed_form(block_bytes):
    for lengths in list(vc.BATCHES.values()) + [(block_bytes, block_bytes + 1, 0, block_bytes - 1, 3 * block_bytes)]:
        off = ov.mask_offsets(lengths, block_bytes)
        assert off.dtype == np.int64 and off.shape == (len(lengths) + 1,)
        assert off.tolist() == [sum(-(-c // block_bytes) for c in lengths[:b]) for b in range(len(lengths) + 1)]
    for bad in (2048, 12288, 0):
        with pytest.raises(ValueError):
            ov.mask_offsets([1], bad)


@pytest.mark.parametrize("block_bytes", [4096, 65536])
def test_lane_rule_and_mask_word_rule_replayed(block_bytes):
    """The vector form's rule, lane by lane: lanes [0, len / 16) own a 16-byte group, the next len % 16 a
    tail byte, later lanes nothing; a wave's word is ``mask_first[b] + wave_block(first group of the
    wave)``. Every byte of every stripe lands in exactly one lane, every live lane of a wave in the word
    the rule names, nothing past ``len``. Then the byte form's."""
    bshift = block_bytes.bit_length() - 1
    lengths = np.array(vc.LENGTHS, dtype=np.int64)
    off = ov.mask_offsets(lengths, block_bytes)
    for bytewise in (False, True):
        nb, first, blk = ov.varlen_blocks(lengths, bytewise)
        owner = [np.zeros(c, dtype=np.int64) for c in lengths]
        for w, b in enumerate(blk):
            c, cb = int(lengths[b]), w - int(first[b])
            lane = cb * BLOCK + np.arange(BLOCK)
            if bytewise:
                lo, hi = lane, np.where(lane < c, lane + 1, lane)
                c0 = lane // 64 * 64
                word = off[b] + (np.where(c0 < c, c0, 0) >> bshift)
            else:
                groups, tail = c // GROUP, c % GROUP
                lo = np.where(lane < groups, lane * GROUP, groups * GROUP + (lane - groups))
                hi = np.where(lane < groups, lo + GROUP, np.where(lane - groups < tail, lo + 1, lo))
                g0 = lane // 64 * 64
                word = off[b] + ((np.minimum(g0, groups) * GROUP) >> bshift)  # wave_block
            live = hi > lo
            assert hi[live].max(initial=0) <= c, (b, "a lane past len")
            assert live.any(), (b, w, "a work item with no live lane")
            for x, y in zip(lo[live], hi[live]):
                owner[b][x:y] += 1
            # the word the rule names is the word of every column the lane owns, and one of the stripe's own
            assert np.array_equal(word[live], off[b] + (lo[live] >> bshift)), (b, w)
            assert np.array_equal(word[live], off[b] + ((hi[live] - 1) >> bshift)), (b, w)
            assert (word[live] < off[b + 1]).all() and (word[live] >= off[b]).all()
        assert all((o == 1).all() for o in owner), "every byte in exactly one lane"
        assert nb[0] == 0, "a stripe of length 0 has no work item"


# ---- CPU tensors against the oracle -----------------------------------------------------------------------
BATCHES = ["b1", "b2", "b3", "b257", "zero-first", "zero-middle", "zero-last", "zeros-only"]


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("code", ["c10_14", "c4_6"])
def test_cpu_batches(code, batch):
    sv.run_damage("cpu", code, vc.BATCHES[batch], 4096, True)


@pytest.mark.parametrize("code", ["c3_4", "c9_14", "c3_19", "v10_14"])
def test_cpu_other_codes(code):
    sv.run_damage("cpu", code, vc.BATCHES["zero-middle"], 65536, True)


@pytest.mark.parametrize("form", ["as2d", "packed", "parity"])
def test_cpu_input_forms(form):
    code, lengths = "c10_14", vc.BATCHES["zero-middle"]
    if form != "parity":
        sv.run_damage("cpu", code, lengths, 4096, True, **{form: True})
        return
    rs = sv.fresh(code)
    vl = VarlenCodec(rs)
    good = sv.consistent(code, lengths)
    bad = {2: sv.overwritten(good, 2, 11)}
    stripes = [bad.get(b, good[b]) for b in range(3)]
    want = sv.damaged_oracle(code, lengths, 4096, bad)
    for packed in (False, True):
        nat, par = vc.Batch(rs.k, lengths, "cpu", packed=packed), vc.Batch(rs.p, lengths, "cpu", packed=packed)
        for part, lo, hi in ((nat, 0, rs.k), (par, rs.k, rs.n)):
            part.put([s[lo:hi] for s in stripes])
            part.upload()
        sv.check_mask(form, vl.syndrome_mask(nat.arg, parity=par.arg, block_bytes=4096, **nat.kw()), want)
        rep = vl.scrub(nat.arg, par.arg, block_bytes=4096, **nat.kw())
        sv.check_report(form, rep, want)
        assert isinstance(rep, VarlenScrubReport) and isinstance(rep.mask, VarlenMask)
        assert rep.report[2].suspects == [11]
        nat.check(form)
        par.check(form)


def test_cpu_single_flips_and_error_values():
    assert sv.flip_sweep("cpu", "c4_6", 4096) == 6 * 8
    sv.error_values("cpu", "c10_14", 16384)


def test_cpu_mask_only_codes_and_p0():
    for code in ("c19_36", "c8_64"):
        rs = sv.fresh(code)
        lengths = (vc.FULL + 1, 0, 33)
        sv.run_damage("cpu", code, lengths, 4096, False)
        with pytest.raises(NotImplementedError, match="p <= 16"):
            VarlenCodec(rs).scrub([torch.zeros(rs.n, c, dtype=torch.uint8) for c in lengths])
    vl = VarlenCodec(ReedSolomon(4, 4))
    stripes = [torch.ones(4, c, dtype=torch.uint8) for c in (5000, 0, 3)]
    m = vl.syndrome_mask(stripes, block_bytes=4096)
    assert m.offsets.tolist() == [0, 2, 2, 3] and not m.blocks.any() and not m.stripes.any()
    rep = vl.scrub(stripes)
    assert rep.clean.all() and rep.votes.shape == (3, 4) and vl.heal(stripes).dirty == []
    none = vl.scrub([])
    assert none.clean.shape == (0,) and none.mask.offsets.tolist() == [0]
    with pytest.raises(NotImplementedError, match="gf256"):
        VarlenCodec(ReedSolomon(4, 6, matrix="cauchy", field="gf16")).syndrome_mask([torch.zeros(6, 4, dtype=torch.uint8)])


# ---- heal ---------------------------------------------------------------------------------------------------
@pytest.fixture
def repairs(monkeypatch):
    """Counts ``VarlenCodec.reconstruct`` calls (and what they erase) and ``ReedSolomon.reconstruct`` calls."""
    calls = {"varlen": [], "single": 0}
    real_v, real_s = VarlenCodec.reconstruct, ReedSolomon.reconstruct

    def varlen(self, stripes, erased, *a, **kw):
        calls["varlen"].append(np.array(erased))
        return real_v(self, stripes, erased, *a, **kw)

    def single(self, *a, **kw):
        calls["single"] += 1
        return real_s(self, *a, **kw)
    monkeypatch.setattr(VarlenCodec, "reconstruct", varlen)
    monkeypatch.setattr(ReedSolomon, "reconstruct", single)
    return calls


def heal_case(device: str, repairs) -> None:
    """33 stripes with one overwritten chunk each are repaired by ONE varlen repair call and the second
    report is clean but for the two stripes that cannot be: one with two wrong chunks in one column,
    one with more than p suspects, both left byte for byte and listed in ``unhealed``."""
    code = "c10_14"
    rs = sv.fresh(code)
    vl = VarlenCodec(rs)
    lengths = tuple(int(c) for c in np.random.default_rng(33).integers(1, 600, size=40)) + (0, vc.FULL + 17)
    good = sv.consistent(code, lengths)
    bad = {b: sv.overwritten(good, b, (3 * b) % rs.n) for b in range(33)}
    two = np.array(good[35])
    two[[2, 7], 0] ^= np.array([0x11, 0x2B], dtype=np.uint8)  # two wrong chunks in one column
    many = np.array(good[41])
    for j in range(rs.p + 1):
        many[j, 100 * j] ^= 0x40  # p + 1 suspects, each column located
    bad.update({35: two, 41: many})
    batch = sv.upload(code, [bad.get(b, good[b]) for b in range(len(good))], device)
    first = vl.scrub(batch.arg)
    assert first.dirty == list(range(33)) + [35, 41]
    assert first.report[35].unlocated == 1 and len(first.report[41].suspects) == rs.p + 1
    rep = vl.heal(batch.arg, report=first)
    assert isinstance(rep, VarlenScrubReport) and rep.unhealed == [35, 41] and rep.dirty == [35, 41]
    assert len(repairs["varlen"]) == 1 and repairs["single"] == (0 if device == "cuda" else 33)
    erased = repairs["varlen"][0]
    assert erased.shape == (len(lengths), rs.p)
    assert [b for b in range(len(lengths)) if (erased[b] >= 0).any()] == list(range(33))
    batch.put([bad.get(b, good[b]) if b in (35, 41) else good[b] for b in range(len(good))])
    batch.check("after heal")
    sv.check_report("after heal", vl.scrub(batch.arg), sv.damaged_oracle(code, lengths, 65536, {35: two, 41: many}))
    # nothing healable left: no repair call, the same stripes unhealed; and a clean batch makes none
    del repairs["varlen"][:]
    again = vl.heal(batch.arg)
    assert again.unhealed == [35, 41] and not repairs["varlen"]
    batch.check("after the second heal")
    clean = sv.upload(code, good, device)
    rep = vl.heal(clean.arg)
    assert rep.clean.all() and rep.unhealed == [] and not repairs["varlen"]
    clean.check("a clean batch")


def test_cpu_heal(repairs):
    heal_case("cpu", repairs)


def test_cpu_heal_packed_with_parity(repairs):
    code, lengths = "c4_6", (300, 0, 17, 4097)
    rs = sv.fresh(code)
    good = sv.consistent(code, lengths)
    bad = [sv.overwritten(good, 0, 5), good[1], good[2], sv.overwritten(good, 3, 1)]
    nat, par = vc.Batch(rs.k, lengths, "cpu", packed=True), vc.Batch(rs.p, lengths, "cpu", packed=True)
    for part, lo, hi, src in ((nat, 0, rs.k, bad), (par, rs.k, rs.n, bad)):
        part.put([s[lo:hi] for s in src])
        part.upload()
    rep = VarlenCodec(rs).heal(nat.arg, par.arg, offsets=nat.offsets)
    assert rep.clean.all() and rep.unhealed == [] and len(repairs["varlen"]) == 1
    nat.put([g[: rs.k] for g in good])
    par.put([g[rs.k:] for g in good])
    nat.check("natives")
    par.check("parity")


# ---- plan keys and refusals ------------------------------------------------------------------------------------
def test_plan_keys_name_every_address_every_length_and_the_block_size():
    vl = VarlenCodec(sv.codec("c4_6"))
    buf = torch.zeros(6, 1024, dtype=torch.uint8)
    base = [[buf[j, :100] for j in range(6)], [buf[j, 512:700] for j in range(6)]]

    def key(stripes, block_bytes=4096, offsets=None, parity=None):
        s, par = vl._parts("stripes", stripes, 6 if parity is None else 4, parity, offsets)
        return vl._scrub_key(s, par, block_bytes)
    k0 = key(base)
    assert key([list(s) for s in base]) == k0
    shorter = [base[0], [r[:187] for r in base[1]]]
    moved = [base[0], [buf[j, 512:700] if j != 3 else buf[j, 513:701] for j in range(6)]]
    assert len({k0, key(shorter), key(moved), key(base, 8192)}) == 4
    p0 = key(buf, offsets=[0, 100, 300])
    assert len({p0, key(buf, offsets=[0, 100, 301]), key(buf, offsets=[0, 101, 300]), key(buf, offsets=[1, 100, 300]),
                key(buf[:, 1:], offsets=[0, 100, 300]), key(buf, 65536, offsets=[0, 100, 300])}) == 6
    n0 = key([s[:4] for s in base], parity=[s[4:] for s in base])
    assert n0 != k0 and n0 != key([s[:4] for s in base], parity=[base[0][4:], [buf[4, 512:700], buf[5, 513:701]]])


def test_refusals_leave_the_buffers_unchanged():
    code, lengths = "c4_6", (300, 17)
    rs = sv.fresh(code)
    vl = VarlenCodec(rs)
    good = sv.consistent(code, lengths)
    batch = sv.upload(code, [sv.overwritten(good, 0, 2), good[1]], "cpu")
    rows = batch.arg
    for what, kw in {
        "block_bytes 2048": dict(stripes=rows, block_bytes=2048),
        "block_bytes 12288": dict(stripes=rows, block_bytes=12288),
        "five rows": dict(stripes=[rows[0][:5], rows[1]]),
        "two lengths in a stripe": dict(stripes=[rows[0][:5] + [rows[0][5][:7]], rows[1]]),
        "int32 rows": dict(stripes=[[r.view(torch.int32) if r.numel() % 4 == 0 else r for r in rows[0]], rows[1]]),
        "a tensor without offsets": dict(stripes=torch.zeros(6, 40, dtype=torch.uint8)),
        "offsets past the end": dict(stripes=torch.zeros(6, 40, dtype=torch.uint8), offsets=[0, 41]),
        "offsets that decrease": dict(stripes=torch.zeros(6, 40, dtype=torch.uint8), offsets=[0, 30, 20]),
        "parity of other lengths": dict(stripes=[s[:4] for s in rows], parity=[[r[:9] for r in rows[0][4:]], rows[1][4:]]),
        "parity of three rows": dict(stripes=[s[:4] for s in rows], parity=[s[3:] for s in rows]),
    }.items():
        for call in (vl.syndrome_mask, vl.scrub, vl.heal):
            if call == vl.heal and "block_bytes" in kw:
                continue
            with pytest.raises(ValueError):
                call(**kw)
            batch.check(what)
    assert not rs._plans


def test_bench_script_runs_on_the_cpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "varlen_scrub_bench.py"), "--device", "cpu"],
                         capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "syndrome_mask" in out.stdout and "heal" in out.stdout

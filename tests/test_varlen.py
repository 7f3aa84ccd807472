"""Variable-length batches on CPU tensors (``VarlenCodec``, ``ops.varlen``): the descriptor layout, the
flat work list, the results against the numpy oracles, the refusals and the plan-cache keys. The
kernel's side of the same cases is tests/test_gpu_varlen.py.

Comparisons are exact. Every batch lives in a guard-filled arena (``varlen_cases.Batch``) whose host
image is the oracle of every byte, so padding, unnamed rows and other stripes are checked with the
results.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import varlen_cases as vc
from gpu_rscode_amd import ReedSolomon, UnrecoverableError, VarlenCodec, gf
from gpu_rscode_amd._native import cpu
from gpu_rscode_amd.ops.varlen import BLOCK, GROUP, build_varlen_desc, varlen_blocks, varlen_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the descriptor --------------------------------------------------------------------------------
def test_layout_mirror_equals_the_native_one():
    for k, m_pad, batch, npat, nblk in itertools.product((1, 3, 10, 256), (1, 2, 4, 8, 16, 256), (1, 2, 7, 65537),
                                                         (1, 3, 300), (0, 1, 5, 8, 70000)):
        lay = varlen_layout(k, m_pad, batch, npat, nblk)
        assert lay == dict(cpu().varlen_layout(k, m_pad, batch, npat, nblk)), (k, m_pad, batch, npat, nblk)
        assert lay["tab_off"] % 32 == 0 and lay["len_off"] % 8 == 0 and lay["first_off"] % 8 == 0
        assert lay["blk_off"] + 4 * nblk <= lay["tab_off"] and lay["bytes"] == lay["tab_off"] + 32 * npat * k * m_pad


def test_descriptor_bytes_hold_the_arrays_where_the_layout_says():
    k, mp, nb, npat = 3, 2, 4, 2
    lengths = np.array([17, 0, 4095, 300])
    _, first, blk = varlen_blocks(lengths, False)
    ins = np.arange(nb * k, dtype=np.uint64).reshape(nb, k) * 16 + 4096
    outs = np.arange(nb * mp, dtype=np.uint64).reshape(nb, mp) * 16 + 8192
    tab = np.arange(npat * k * mp * 8, dtype=np.uint32).reshape(npat, k, mp, 8)
    buf = build_varlen_desc(ins, outs, np.array([1, 0, 0, 1]), lengths, first, blk, tab)
    lay = varlen_layout(k, mp, nb, npat, blk.size)
    assert buf.size == lay["bytes"]
    assert buf[:16].view("<i4").tolist() == [k, mp, nb, npat]

    def at(name, dt, count):
        return buf[lay[name]: lay[name] + count * np.dtype(dt).itemsize].view(dt)
    assert np.array_equal(at("in_off", "<u8", nb * k), ins.reshape(-1))
    assert np.array_equal(at("out_off", "<u8", nb * mp), outs.reshape(-1))
    assert at("len_off", "<i8", nb).tolist() == lengths.tolist()
    assert at("first_off", "<i8", nb).tolist() == first.tolist()
    assert at("pat_off", "<i4", nb).tolist() == [1, 0, 0, 1]
    assert at("blk_off", "<i4", blk.size).tolist() == blk.tolist()
    assert np.array_equal(at("tab_off", "<u4", tab.size), tab.reshape(-1))


# ---- the work list ---------------------------------------------------------------------------------
LENGTH_SETS = [vc.LENGTHS, vc.LENGTHS[::-1], (0, 0, 0), (0,), (), (5,), vc.BATCHES["b257"],
               vc.BATCHES["one-long-among-256"]]


@pytest.mark.parametrize("bytewise", [False, True], ids=["vector", "bytes"])
@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=[f"set{i}" for i in range(len(LENGTH_SETS))])
def test_blocks_list_every_stripe_block_once_and_in_order(lengths, bytewise):
    n = np.array(lengths, dtype=np.int64)
    nb, first, blk = varlen_blocks(lengths, bytewise)
    lanes = n if bytewise else n // GROUP + n % GROUP
    assert nb.tolist() == [-(-int(v) // BLOCK) for v in lanes]
    assert first.tolist() == [int(nb[:b].sum()) for b in range(n.size)]
    assert blk.dtype == np.int32 and nb.dtype == np.int64 and first.dtype == np.int64
    assert int(nb.sum()) == blk.size
    want = [(b, cb) for b in range(n.size) for cb in range(int(nb[b]))]
    got = [(int(b), w - int(first[b])) for w, b in enumerate(blk)]
    assert got == want
    assert not set(blk.tolist()) & set(np.nonzero(n == 0)[0].tolist())


def test_blocks_refuse_negative_lengths():
    with pytest.raises(ValueError):
        varlen_blocks([4, -1], False)


@pytest.mark.parametrize("bytewise", [False, True], ids=["vector", "bytes"])
def test_lane_rule_covers_each_stripe_exactly_once(bytewise):
    """A numpy replay of the kernel's lane rule for every work item: lane g < ngroups owns bytes [16g,
    16g + 16), lanes [ngroups, ngroups + tail) one byte each (byte form: lane c < len owns byte c).
    Every byte of [0, len[b]) is owned once and nothing past it."""
    for lengths in (vc.LENGTHS, vc.BATCHES["b257"]):
        nb, first, blk = varlen_blocks(lengths, bytewise)
        owned = [np.zeros(c + 2 * GROUP, dtype=np.int32) for c in lengths]
        for w, b in enumerate(blk.tolist()):
            c = lengths[b]
            g = (w - int(first[b])) * BLOCK + np.arange(BLOCK)
            if bytewise:
                np.add.at(owned[b], g[g < c], 1)
                continue
            ngroups, tail = divmod(c, GROUP)
            for lane in g[g < ngroups]:
                owned[b][GROUP * lane: GROUP * lane + GROUP] += 1
            t = g[(g >= ngroups) & (g - ngroups < tail)]
            np.add.at(owned[b], GROUP * ngroups + (t - ngroups), 1)
        for b, c in enumerate(lengths):
            assert (owned[b][:c] == 1).all() and not owned[b][c:].any(), (b, c)


# ---- results on CPU tensors ------------------------------------------------------------------------
@pytest.mark.parametrize("code,batch", vc.CASES, ids=[f"{c}-{b}" for c, b in vc.CASES])
def test_encode_equals_the_oracle_and_rs_encode(code, batch):
    rs, lengths = vc.codec(code), vc.lengths_of(batch)
    data, par, good = vc.encode_case(code, lengths, "cpu")
    codec = VarlenCodec(rs)
    assert codec.encode(data.arg, par.arg) is par.arg
    par.check(f"{code} {batch}: parity")
    data.check(f"{code} {batch}: data")
    for b, g in enumerate(good):
        if g.shape[1]:
            single = rs.encode(torch.from_numpy(np.array(g[: rs.k])))
            assert np.array_equal(single.numpy(), g[rs.k:]), b


# mixed erasures on every case; natives only and parity only on the ladder (every length) of every code
REPAIRS = ([(c, b, "mixed") for c, b in vc.CASES]
           + [(c, b, kind) for c, b in vc.CASES if b in ("ladder", "wide") for kind in ("natives", "parity")])


@pytest.mark.parametrize("code,batch,kind", REPAIRS, ids=["-".join(r) for r in REPAIRS])
def test_reconstruct_equals_the_oracle(code, batch, kind):
    rs, lengths = vc.codec(code), vc.lengths_of(batch)
    erased = vc.erasures(code, len(lengths), kind=kind)
    if kind == "mixed" and len(lengths) > rs.p:
        assert {len(e) for e in erased} == set(range(rs.p + 1)), "0..p erasures in one batch"
    stripes, bad, want = vc.repair_case(code, lengths, erased, "cpu")
    assert VarlenCodec(rs).reconstruct(stripes.arg, [list(e) for e in erased]) is stripes.arg
    stripes.check(f"{code} {batch} {kind}")
    good = vc.consistent(code, tuple(lengths))
    for b, w in enumerate(want):  # (a consistent stripe comes back whole)
        assert np.array_equal(w, good[b]), b


def test_reconstruct_257_distinct_patterns():
    rs = vc.codec("c10_14")
    erased = tuple(itertools.islice(itertools.combinations(range(rs.n), 3), 257))
    lengths = vc.BATCHES["b257"]
    assert len(set(erased)) == 257
    stripes, _, _ = vc.repair_case("c10_14", lengths, erased, "cpu")
    VarlenCodec(rs).reconstruct(stripes.arg, np.array(erased))
    stripes.check("257 patterns")


def test_erased_forms_agree():
    """Flat ids shared by every stripe, a padded [B, e] array, a CPU tensor and a ragged list."""
    rs, lengths = vc.codec("c10_14"), (17, 300, 4097)
    for erased, arg in (([(3, 12)] * 3, [3, 12]),
                        ([(3, 12), (0,), ()], np.array([[3, 12], [0, -1], [-1, -1]])),
                        ([(3, 12), (0,), ()], torch.tensor([[12, 3, 3], [0, -1, -1], [-1, -1, -1]])),
                        ([(3, 12), (0,), ()], [[12, 3], [0], []])):
        stripes, _, _ = vc.repair_case("c10_14", lengths, erased, "cpu")
        VarlenCodec(rs).reconstruct(stripes.arg, arg)
        stripes.check(str(arg))


@pytest.mark.parametrize("form", ["packed", "2d"])
def test_other_forms_give_the_list_forms_result(form):
    code, lengths = "c10_14", vc.LENGTHS[:-1]
    rs = vc.codec(code)
    kw = dict(packed=True) if form == "packed" else dict(as2d=True)
    data, par, _ = vc.encode_case(code, lengths, "cpu", **kw)
    VarlenCodec(rs).encode(data.arg, par.arg, **data.kw())
    par.check(f"encode, {form}")
    data.check(f"encode data, {form}")
    erased = vc.erasures(code, len(lengths))
    stripes, _, _ = vc.repair_case(code, lengths, erased, "cpu", **kw)
    VarlenCodec(rs).reconstruct(stripes.arg, [list(e) for e in erased], **stripes.kw())
    stripes.check(f"reconstruct, {form}")


def test_natives_with_parity_in_another_allocation():
    code, lengths = "c10_14", (17, 0, 4097, 300)
    rs = vc.codec(code)
    erased = ((0, 12), (1,), (13, 11, 2, 3), ())
    good = vc.consistent(code, lengths)
    bad = vc.damaged(good, erased)
    nat, par = vc.Batch(rs.k, lengths), vc.Batch(rs.p, lengths)
    nat.put([b[: rs.k] for b in bad])
    par.put([b[rs.k:] for b in bad])
    nat.upload()
    par.upload()
    VarlenCodec(rs).reconstruct(nat.arg, [list(e) for e in erased], parity=par.arg)
    nat.put([g[: rs.k] for g in good])
    par.put([g[rs.k:] for g in good])
    nat.check("natives")
    par.check("parity")


def test_allocated_parity_has_the_form_of_the_data():
    code, lengths = "c4_6", (17, 0, 4097)
    rs = vc.codec(code)
    good = vc.consistent(code, lengths)
    data, _, _ = vc.encode_case(code, lengths, "cpu")
    par = VarlenCodec(rs).encode(data.arg)
    assert isinstance(par, list) and [tuple(p.shape) for p in par] == [(rs.p, c) for c in lengths]
    for p, g in zip(par, good):
        assert np.array_equal(p.numpy(), g[rs.k:])
    packed, _, _ = vc.encode_case(code, lengths, "cpu", packed=True)
    par = VarlenCodec(rs).encode(packed.arg, offsets=packed.offsets)
    assert tuple(par.shape) == (rs.p, packed.arg.shape[1])
    for b, g in enumerate(good):
        assert np.array_equal(par[:, packed.offsets[b]: packed.offsets[b + 1]].numpy(), g[rs.k:])


def test_other_fields_on_cpu_tensors():
    """gf65536 runs on CPU tensors through the codec's own calls (even lengths: 16-bit symbols)."""
    rs = ReedSolomon(4, 6, matrix="cauchy", field="gf65536")
    lengths = (18, 0, 4098)
    rng = np.random.default_rng(5)
    data = [torch.from_numpy(rng.integers(0, 256, size=(4, c), dtype=np.uint8)) for c in lengths]
    par = VarlenCodec(rs).encode(data)
    for d, p in zip(data, par):
        if d.shape[1]:
            assert torch.equal(p, rs.encode(d.clone()))
    stripes = [torch.cat([d, p]) for d, p in zip(data, par)]
    want = [s.clone() for s in stripes]
    erased = [[0, 5], [1], [2, 3]]
    for s, e in zip(stripes, erased):
        s[e] = vc.FRESH
    VarlenCodec(rs).reconstruct(stripes, erased)
    assert all(torch.equal(s, w) for s, w in zip(stripes, want))
    with pytest.raises(ValueError):
        VarlenCodec(rs).encode([torch.zeros((4, 7), dtype=torch.uint8)])


# ---- refusals: ValueError, nothing written ---------------------------------------------------------
def _refusal_batch():
    lengths = (40, 300, 17)
    erased = ((0,), (1, 12), (13,))
    stripes, _, _ = vc.repair_case("c10_14", lengths, erased, "cpu")
    stripes.image[:] = stripes.buf.numpy()  # the image: the damaged state, which must stay
    return stripes, [list(e) for e in erased]


def _rows(batch):
    return [list(s) for s in batch.arg]


def _meta(row: torch.Tensor) -> torch.Tensor:
    return torch.empty(row.shape, dtype=torch.uint8, device="meta")


REFUSALS = {
    "row-count": lambda s, e: (dict(stripes=[r[:13] for r in _rows(s)], erased=e), ValueError),
    "row-count-one-stripe": lambda s, e: (dict(stripes=[_rows(s)[0], _rows(s)[1][:13], _rows(s)[2]], erased=e), ValueError),
    "row-lengths": lambda s, e: (dict(stripes=[_rows(s)[0], [r[:299] if j == 4 else r for j, r in enumerate(_rows(s)[1])],
                                               _rows(s)[2]], erased=e), ValueError),
    "dtype": lambda s, e: (dict(stripes=[[r.view(torch.int8) for r in _rows(s)[0]]] + _rows(s)[1:], erased=e), ValueError),
    "strided": lambda s, e: (dict(stripes=[_rows(s)[0], [r[::2] if j == 2 else r[:150] for j, r in enumerate(_rows(s)[1])],
                                           _rows(s)[2]], erased=e), ValueError),
    "not-rows": lambda s, e: (dict(stripes=[_rows(s)[0], 7, _rows(s)[2]], erased=e), ValueError),
    "tensor-without-offsets": lambda s, e: (dict(stripes=torch.zeros((14, 64), dtype=torch.uint8), erased=[0]), ValueError),
    "id-range": lambda s, e: (dict(stripes=_rows(s), erased=[[0], [14], [1]]), ValueError),
    "id-negative": lambda s, e: (dict(stripes=_rows(s), erased=np.array([[0], [-2], [1]])), ValueError),
    "id-count": lambda s, e: (dict(stripes=_rows(s), erased=[[0], [1]]), ValueError),
    "id-float": lambda s, e: (dict(stripes=_rows(s), erased=np.array([[0.5], [1.0], [2.0]])), ValueError),
    "too-many": lambda s, e: (dict(stripes=_rows(s), erased=[[0], [1, 2, 3, 4, 5], [6]]), UnrecoverableError),
    "listed-twice": lambda s, e: (dict(stripes=[_rows(s)[0], _rows(s)[1], _rows(s)[0]], erased=[[0], [1], [0]]), ValueError),
    "written-row-overlaps": lambda s, e: (dict(stripes=[_rows(s)[0], _rows(s)[1],
                                                        [s.buf[int(s.off[1, 1]) + 290: int(s.off[1, 1]) + 307]] + _rows(s)[2][1:]],
                                               erased=[[], [1], [13]]), ValueError),
    # rows on mixed devices: a "meta" row stands in for a row on a GPU (its device is looked at, never its bytes)
    "devices-in-one-stripe": lambda s, e: (dict(stripes=[_rows(s)[0], [_meta(r) if j == 3 else r for j, r in enumerate(_rows(s)[1])],
                                                         _rows(s)[2]], erased=e), ValueError),
    "devices-across-stripes": lambda s, e: (dict(stripes=[_rows(s)[0], _rows(s)[1], [_meta(r) for r in _rows(s)[2]]],
                                                 erased=e), ValueError),
    "devices-natives-and-parity": lambda s, e: (dict(stripes=[r[:10] for r in _rows(s)], erased=e,
                                                     parity=[[_meta(x) for x in r[10:]] for r in _rows(s)]), ValueError),
    "parity-count": lambda s, e: (dict(stripes=[r[:10] for r in _rows(s)], erased=e, parity=[r[10:13] for r in _rows(s)]),
                                  ValueError),
    "parity-lengths": lambda s, e: (dict(stripes=[r[:10] for r in _rows(s)], erased=e,
                                         parity=[[x[:16] for x in r[10:]] for r in _rows(s)]), ValueError),
    "parity-stripes": lambda s, e: (dict(stripes=[r[:10] for r in _rows(s)], erased=e,
                                         parity=[r[10:] for r in _rows(s)][:2]), ValueError),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_reconstruct_refusals_write_nothing(what):
    stripes, erased = _refusal_batch()
    kwargs, exc = REFUSALS[what](stripes, erased)
    with pytest.raises(exc):
        VarlenCodec(vc.codec("c10_14")).reconstruct(**kwargs)
    stripes.check(what)


def test_singular_pattern_names_the_first_such_stripe():
    rs = vc.codec("v10_14")
    bad_pattern = next(s for s in itertools.combinations(range(rs.n), rs.k) if not gf.GF256.is_invertible(rs.G[list(s)]))
    lost = [i for i in range(rs.n) if i not in bad_pattern]
    lengths = (40, 300, 17)
    stripes, _, _ = vc.repair_case("v10_14", lengths, ((0,), (), ()), "cpu")
    stripes.image[:] = stripes.buf.numpy()
    with pytest.raises(UnrecoverableError, match="stripe 1"):
        VarlenCodec(rs).reconstruct(stripes.arg, [[0], lost, lost])
    stripes.check("singular")


OFFSETS_BAD = {
    "decreasing": [16, 80, 40, 200],
    "negative": [-16, 40, 100, 200],
    "past-the-end": [16, 80, 100, 100000],
    "two-d": [[16, 80], [100, 200]],
    "float": [16.0, 80.0, 100.0, 200.0],
    "empty": [],
    "string": "offsets",
}


@pytest.mark.parametrize("what", list(OFFSETS_BAD))
def test_bad_offsets_are_refused(what):
    lengths = (40, 300, 17)
    data, par, _ = vc.encode_case("c10_14", lengths, "cpu", packed=True)
    par.image[:] = par.buf.numpy()
    with pytest.raises(ValueError):
        VarlenCodec(vc.codec("c10_14")).encode(data.arg, par.arg, offsets=OFFSETS_BAD[what])
    par.check(what)
    data.check(what)


def test_packed_rows_on_mixed_devices_are_refused():
    lengths = (40, 300, 17)
    data, par, _ = vc.encode_case("c10_14", lengths, "cpu", packed=True)
    par.image[:] = par.buf.numpy()
    codec = VarlenCodec(vc.codec("c10_14"))
    with pytest.raises(ValueError, match="one device"):
        codec.encode(data.arg, torch.empty(par.arg.shape, dtype=torch.uint8, device="meta"), offsets=data.offsets)
    with pytest.raises(ValueError, match="one device"):
        codec.reconstruct(data.arg, [0], parity=torch.empty(par.arg.shape, dtype=torch.uint8, device="meta"),
                          offsets=data.offsets)
    par.check("packed, parity on another device")
    data.check("packed, parity on another device")


def test_encode_refusals_write_nothing():
    rs = vc.codec("c10_14")
    lengths = (40, 300, 17)
    data, par, _ = vc.encode_case("c10_14", lengths, "cpu")
    par.image[:] = par.buf.numpy()
    codec = VarlenCodec(rs)
    d, p = [list(s) for s in data.arg], [list(s) for s in par.arg]
    for name, args in {
        "data-row-count": ([r[:9] for r in d], p),
        "parity-row-count": (d, [r[:3] for r in p]),
        "lengths": (d, [p[0], [x[:299] for x in p[1]], p[2]]),
        "stripes": (d, p[:2]),
        "parity-is-data": (d, [p[0], d[1][:4], p[2]]),
        "parity-twice": (d, [p[0], p[1], [x[:17] for x in p[1]]]),
        "packed-and-list": (data.arg, par.buf[:2048].view(4, 512)),
        "devices-in-one-stripe": ([d[0], [_meta(r) if j == 9 else r for j, r in enumerate(d[1])], d[2]], p),
        "devices-across-stripes": ([[_meta(r) for r in d[0]], d[1], d[2]], p),
        "devices-data-and-parity": (d, [[_meta(r) for r in x] for x in p]),
        "devices-in-the-parity": (d, [p[0], p[1], [_meta(r) if j == 0 else r for j, r in enumerate(p[2])]]),
    }.items():
        with pytest.raises(ValueError):
            codec.encode(*args)
        par.check(name)
        data.check(name)
    with pytest.raises(TypeError):
        VarlenCodec(object())


def test_cuda_id_tensors_and_wide_fields_are_refused_by_device():
    """What depends on a device without needing one: the id tensor's device is looked at before its
    contents (a "meta" tensor stands in for a GPU one), and gf65536 rows on a GPU are refused by the
    device check alone."""
    stripes, erased = _refusal_batch()
    with pytest.raises(ValueError, match="CPU tensor"):
        VarlenCodec(vc.codec("c10_14")).reconstruct(stripes.arg, torch.zeros((3, 1), dtype=torch.int64, device="meta"))
    stripes.check("meta ids")
    wide = VarlenCodec(ReedSolomon(4, 6, field="gf65536"))
    with pytest.raises(NotImplementedError):
        wide._check_device(type("Part", (), {"device": torch.device("cuda")})())


# ---- plan-cache keys: equal keys only for equal layouts ---------------------------------------------
BUF = torch.zeros(1 << 16, dtype=torch.uint8)
KEY_LENGTHS = (48, 100, 16)


def _key_args(lengths=KEY_LENGTHS, base=0, moved=None, erased=((1, 12), (0,), (13, 2)), packed=False):
    """Stripes of 14 rows over one buffer: list form (rows 128 bytes apart, ``moved`` = one (stripe,
    row) 64 bytes further on) or packed form (offsets from ``base``)."""
    if packed:
        t = BUF[: 14 * 1024].view(14, 1024)
        return t, np.concatenate([[base], base + np.cumsum(lengths)]), erased
    rows, at = [], base
    for b, c in enumerate(lengths):
        rows.append([BUF[at + 128 * j + (64 if moved == (b, j) else 0):][:c] for j in range(14)])
        at += 14 * 128
    return rows, None, erased


def _keys(stripes, offsets, erased):
    """(everything a plan takes from the rows, the ids' bytes, the repair key, the encode key)"""
    codec = VarlenCodec(vc.codec("c10_14"))
    s, par = codec._parts("stripes", stripes, 14, None, offsets)
    raw = codec.rs._erased_raw([list(e) for e in erased], 14)
    d, p = codec._parts("data", [r[:10] for r in stripes] if offsets is None else stripes[:10], 10,
                        [r[10:] for r in stripes] if offsets is None else stripes[10:], offsets)
    ptrs = codec._ptrs(s, par)
    assert np.array_equal(ptrs, codec._ptrs(d, p))
    layout = (ptrs.shape, ptrs.tobytes(), s.lengths.tobytes())
    return layout, raw.tobytes(), codec._repair_key(s, par, raw), codec._encode_key(d, p)


KEY_PAIRS = {
    "one-length": (dict(), dict(lengths=(48, 99, 16))),
    "one-row-pointer": (dict(), dict(moved=(1, 3))),
    "one-parity-row-pointer": (dict(), dict(moved=(2, 12))),
    "one-erased-id": (dict(), dict(erased=((1, 12), (0,), (13, 3)))),
    "one-offset": (dict(packed=True), dict(packed=True, base=16)),
    "one-length-packed": (dict(packed=True), dict(packed=True, lengths=(48, 101, 16))),
    "lengths-that-sum-alike": (dict(packed=True), dict(packed=True, lengths=(47, 101, 16))),
}


@pytest.mark.parametrize("what", list(KEY_PAIRS))
def test_plan_keys_differ_where_the_layouts_do(what):
    a, b = (_keys(*_key_args(**kw)) for kw in KEY_PAIRS[what])
    assert (a[0], a[1]) != (b[0], b[1]), "the pair is not what the test means it to be"
    assert a[2] != b[2]
    assert (a[3] != b[3]) == (a[0] != b[0])  # (the erased ids are no part of an encode)


def test_equal_layouts_have_equal_keys():
    for kw in (dict(), dict(packed=True)):
        a, b = _keys(*_key_args(**kw)), _keys(*_key_args(**kw))
        assert a == b and hash(a[2]) == hash(b[2]) and {a[3]: 1}[b[3]] == 1
    # rows given as [14, C] tensors or as lists of rows: one layout, one key
    rows, _, erased = _key_args()
    two_d = [BUF.as_strided((14, c), (128, 1), BUF.storage_offset() + 14 * 128 * b) for b, c in enumerate(KEY_LENGTHS)]
    assert _keys(two_d, None, erased)[2] == _keys(rows, None, erased)[2]
    # offsets as a list, an int32 array or a tensor
    t, off, erased = _key_args(packed=True)
    codec = VarlenCodec(vc.codec("c10_14"))
    for other in (off.tolist(), off.astype(np.int32), torch.from_numpy(off)):
        assert _keys(t, other, erased) == _keys(t, off, erased)


# ---- the bench script ------------------------------------------------------------------------------
def test_bench_script_runs_on_cpu_tensors():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "varlen_bench.py"), "--device", "cpu",
                          "--objects", "6", "--min-bytes", "64", "--max-bytes", "512", "--rounds", "2", "--iters", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json

    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["device"] == "cpu" and res["objects"] == 6
    for name in ("varlen_encode", "loop_encode", "padded_encode_batch", "varlen_reconstruct_1", "varlen_reconstruct_4",
                 "loop_reconstruct_1", "uniform_varlen_encode", "uniform_encode_batch", "uniform_varlen_reconstruct_1",
                 "uniform_reconstruct_batch_1"):
        assert res["timings"][name]["median_us"] > 0, name

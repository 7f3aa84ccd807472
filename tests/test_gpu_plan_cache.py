"""The codec's plan cache on the MI355X: two calls that start at one base pointer.

Every GPU call of ``ReedSolomon`` goes through ``rs._plans``; on a hit nothing is looked at again, and the
cached plan holds raw row addresses, batch strides and coefficient tables. A key that says less than its
plan depends on is silent: the kernel writes correct bytes to the previous caller's addresses and the
new caller's output keeps what was in it. So here every tensor handed to the codec is an
``as_strided`` view of ONE arena, two calls share every base pointer and differ in one property, and
after each call the whole arena is compared on the device with a host mirror: the views the call may
write hold the numpy oracle's bytes, every other byte the guard value or the input put there. Both
layouts of a pair lie wholly inside the arena (asserted where a view is made), so a stale plan shows
as wrong bytes in a live allocation, never as an access outside one.

Oracles only: ``gf.GF256.gemm`` / ``gf.field(16).gemm``, ``gf.reconstruct_oracle``, ``gf.scrub_oracle``,
``gf.correct_oracle``, and for updates the oracle's parity of the updated natives; a decode must give
back the natives that were encoded.

Shapes: B = 3 stripes of C = 1000 bytes (a ragged tail after the 16-byte vectors; 1002 for GF(2^16)),
(4, 6) and, where two errors per column need p >= 4, (10, 14) Cauchy codes; row pitches 1024 and 1280
(16-byte aligned) and 1031 (later rows off alignment: the byte form on the very base pointer where the
other layout took the vector form; 1030 for GF(2^16), whose rows must be 2-byte aligned); batch strides
``rows x pitch`` and 4096 more. A column-block size can only matter to a mask past 4096 columns, so
those pairs also run at C = 5000."""
import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, gf

pytestmark = pytest.mark.gpu

ARENA_BYTES, REGION, GUARD = 1 << 20, 1 << 18, 0x5A  # four regions, one per argument of a call
B = 3
ALIGNED, WIDER, ODD = 1024, 1280, 1031
GAP = 4096
CODE, CODE2 = (4, 6, "cauchy"), (10, 14, "cauchy")
FIELDS = ["gf256", "gf65536"]


# ---- the arena ------------------------------------------------------------------------------------------
class View:
    """A view of the arena (``t``) and the same view of the host mirror (``h``)."""

    def __init__(self, t: torch.Tensor, h: np.ndarray):
        self.t, self.h = t, h

    def put(self, a: np.ndarray) -> None:
        """Input bytes: on the device and in the mirror."""
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.h[...] = a

    def rows(self, b=None) -> list[torch.Tensor]:
        t = self.t if b is None else self.t[b]
        return [t[i] for i in range(t.shape[0])]

    def lists(self) -> list[list[torch.Tensor]]:
        return [self.rows(b) for b in range(self.t.shape[0])]

    def __getitem__(self, idx) -> "View":
        return View(self.t[idx], self.h[idx])


class Arena:
    def __init__(self):
        self.buf = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.want = np.empty(ARENA_BYTES, dtype=np.uint8)
        self.reset()

    def reset(self) -> None:
        self.buf.fill_(GUARD)
        self.want.fill(GUARD)

    def view(self, shape, strides, off: int) -> View:
        last = off + sum((n - 1) * s for n, s in zip(shape, strides))
        assert off >= 0 and min(shape) > 0 and min(strides) > 0 and last < ARENA_BYTES, "a view outside the arena"
        return View(self.buf.as_strided(shape, strides, off),
                    np.lib.stride_tricks.as_strided(self.want[off:], shape, strides))

    def rows(self, region: int, nrows: int, ncols: int, pitch: int = ALIGNED, off: int = 0) -> View:
        """[nrows, ncols] at the start of a region (+ ``off`` bytes)."""
        assert off + nrows * pitch <= REGION
        return self.view((nrows, ncols), (pitch, 1), region * REGION + off)

    def batch(self, region: int, nb: int, nrows: int, ncols: int, pitch: int = ALIGNED, gap: int = 0) -> View:
        """[nb, nrows, ncols] at the start of a region, stripes ``nrows x pitch + gap`` bytes apart."""
        assert nb * (nrows * pitch + gap) <= REGION
        return self.view((nb, nrows, ncols), (nrows * pitch + gap, pitch, 1), region * REGION)

    def check(self, what) -> None:
        """One compare of the whole arena with the mirror, on the device."""
        torch.cuda.synchronize()
        want = torch.from_numpy(self.want).cuda()
        if torch.equal(self.buf, want):
            return
        bad = torch.nonzero(self.buf != want).flatten().cpu().numpy()
        got = self.buf.cpu().numpy()
        starts = bad[np.concatenate([[True], np.diff(bad) > 1])]
        runs = "; ".join(f"region {o // REGION} + {o % REGION} (got {got[o]:#04x}, want {self.want[o]:#04x})"
                         for o in starts[:8].tolist())
        raise AssertionError(f"{what}: {bad.size} bytes of the arena differ from the oracle and the guard, in "
                             f"{starts.size} runs starting at {runs}")


@pytest.fixture(scope="module")
def arena():
    return Arena()


# ---- codecs, data and oracles ---------------------------------------------------------------------------
def codec(code=CODE, field: str = "gf256") -> ReedSolomon:
    k, n, matrix = code
    return ReedSolomon(k, n, matrix=matrix, field=field)


def row_bytes(rs) -> int:
    return 1002 if rs.wide else 1000


def odd_pitch(rs) -> int:
    return ODD - 1 if rs.wide else ODD


def noise(seed, *shape) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def parity_of(rs, data: np.ndarray, e=None) -> np.ndarray:
    """The oracle's parity of [k, C] natives (or of [B, k, C]) under ``e`` (default ``rs.E``)."""
    e = rs.E if e is None else e
    data = np.ascontiguousarray(data)
    if data.ndim == 3:
        return np.stack([parity_of(rs, d, e) for d in data])
    if rs.wide:
        return np.ascontiguousarray(gf.field(16).gemm(e, data.view("<u2")).astype("<u2")).view(np.uint8)
    return gf.GF256.gemm(e, data)


def stripe_of(rs, data: np.ndarray, e=None) -> np.ndarray:
    return np.concatenate([data, parity_of(rs, data, e)], axis=-2)


def pair(rs, first, second, grows: bool = True) -> None:
    """Call 1, call 2 (which must miss), call 1 again (which must hit); each checks itself."""
    n0 = len(rs._plans)
    first()
    n1 = len(rs._plans)
    assert n1 > n0, "the first call cached no plan"
    second()
    n2 = len(rs._plans)
    assert n2 > n1 or not grows, "the second call ran the first call's plan: a right result by luck"
    first()
    assert len(rs._plans) == n2, "the first call, repeated, missed"


def other(x: dict, changes: dict, what: str) -> dict:
    return dict(x, **changes[what])


# ---- (a) encode -----------------------------------------------------------------------------------------
def encode_call(arena, rs, form, C, dp, pp, seed):
    def run():
        arena.reset()
        d, p = arena.rows(0, rs.k, C, dp), arena.rows(1, rs.p, C, pp)
        host = noise(seed, rs.k, C)
        d.put(host)
        parity = p.rows() if form == "rows" else p.t
        got = rs.encode(d.t if form == "2d" else d.rows(), parity)
        assert got is parity
        p.h[...] = parity_of(rs, host)
        arena.check(("encode", form, C, dp, pp))
    return run


@pytest.mark.parametrize("what", ["data-pitch", "parity-pitch", "C", "data-unaligned", "parity-unaligned"])
@pytest.mark.parametrize("form", ["2d", "list-data", "rows"])  # keys enc2d, encL, enc
@pytest.mark.parametrize("field", FIELDS)
def test_encode(arena, field, form, what):
    rs = codec(field=field)
    x = dict(C=row_bytes(rs), dp=ALIGNED, pp=ALIGNED)
    y = other(x, {"data-pitch": dict(dp=WIDER), "parity-pitch": dict(pp=WIDER), "C": dict(C=x["C"] - 64),
                  "data-unaligned": dict(dp=odd_pitch(rs)), "parity-unaligned": dict(pp=odd_pitch(rs))}, what)
    pair(rs, encode_call(arena, rs, form, seed=1, **x), encode_call(arena, rs, form, seed=2, **y))


def encode_batch_call(arena, rs, seed, nb=B, C=1000, pc=None, dp=ALIGNED, dg=0, pp=ALIGNED, pg=0):
    pc = C if pc is None else pc

    def run():
        arena.reset()
        d, p = arena.batch(0, nb, rs.k, C, dp, dg), arena.batch(1, nb, rs.p, pc, pp, pg)
        host = noise(seed, nb, rs.k, C)
        d.put(host)
        assert rs.encode_batch(d.t, p.t) is p.t
        p.h[...] = parity_of(rs, host)[:, :, :pc]
        arena.check(("encode_batch", nb, C, pc, dp, dg, pp, pg))
    return run


@pytest.mark.parametrize("what", ["data-batch-stride", "data-pitch", "parity-batch-stride", "parity-pitch", "B",
                                  "parity-unaligned", "parity-C"])
@pytest.mark.parametrize("field", FIELDS)
def test_encode_batch(arena, field, what):
    """``parity-batch-stride`` and ``parity-pitch``: the key once named the parity's base pointer alone,
    and the second call's parity was written at the first call's strides."""
    rs = codec(field=field)
    x = dict(C=row_bytes(rs))
    y = other(x, {"data-batch-stride": dict(dg=GAP), "data-pitch": dict(dp=WIDER), "parity-batch-stride": dict(pg=GAP),
                  "parity-pitch": dict(pp=WIDER), "B": dict(nb=2), "parity-unaligned": dict(pp=odd_pitch(rs)),
                  "parity-C": dict(pc=x["C"] - 64)}, what)
    pair(rs, encode_batch_call(arena, rs, 1, **x), encode_batch_call(arena, rs, 2, **y))


# ---- (a) decode -----------------------------------------------------------------------------------------
IDS_X, IDS_Y = [0, 2, 4, 5], [5, 1, 3, 0]  # natives 1 and 3 lost; native 2 lost, another order


def decode_call(arena, rs, form, seed, ids=IDS_X, sp=ALIGNED, op=ALIGNED, dev=False):
    def run():
        arena.reset()
        C = row_bytes(rs)
        s, o = arena.rows(0, rs.k, C, sp), arena.rows(1, rs.k, C, op)
        host = noise(seed, rs.k, C)
        s.put(stripe_of(rs, host)[ids])
        out = o.rows() if form == "rows" else o.t
        rs.last_status = None
        assert rs.decode(s.t if form == "2d" else s.rows(), ids, out, device_invert=dev) is out
        o.h[...] = host
        arena.check(("decode", form, ids, sp, op, dev))
        assert rs.last_status is None or int(rs.last_status.item()) == 0
    return run


@pytest.mark.parametrize("what", ["ids", "survivors-pitch", "out-pitch", "out-unaligned", "device-invert"])
@pytest.mark.parametrize("form", ["2d", "list-survivors", "rows"])  # keys dec2d, decL, dec
@pytest.mark.parametrize("field", FIELDS)
def test_decode(arena, field, form, what):
    rs = codec(field=field)
    y = other({}, {"ids": dict(ids=IDS_Y), "survivors-pitch": dict(sp=WIDER), "out-pitch": dict(op=WIDER),
                   "out-unaligned": dict(op=odd_pitch(rs)), "device-invert": dict(dev=True)}, what)
    pair(rs, decode_call(arena, rs, form, 1), decode_call(arena, rs, form, 2, **y))


def decode_batch_call(arena, rs, seed, ids=IDS_X, sp=ALIGNED, sg=0, op=ALIGNED, og=0):
    def run():
        arena.reset()
        C = row_bytes(rs)
        s, o = arena.batch(0, B, rs.k, C, sp, sg), arena.batch(1, B, rs.k, C, op, og)
        host = noise(seed, B, rs.k, C)
        s.put(stripe_of(rs, host)[:, ids])
        assert rs.decode_batch(s.t, ids, o.t) is o.t
        o.h[...] = host
        arena.check(("decode_batch", ids, sp, sg, op, og))
    return run


@pytest.mark.parametrize("what", ["ids", "survivors-batch-stride", "survivors-pitch", "out-batch-stride", "out-pitch",
                                  "out-unaligned"])
@pytest.mark.parametrize("field", FIELDS)
def test_decode_batch(arena, field, what):
    rs = codec(field=field)
    y = other({}, {"ids": dict(ids=IDS_Y), "survivors-batch-stride": dict(sg=GAP), "survivors-pitch": dict(sp=WIDER),
                   "out-batch-stride": dict(og=GAP), "out-pitch": dict(op=WIDER),
                   "out-unaligned": dict(op=odd_pitch(rs))}, what)
    pair(rs, decode_batch_call(arena, rs, 1), decode_batch_call(arena, rs, 2, **y))


# ---- (a) reconstruct ------------------------------------------------------------------------------------
def reconstruct_call(arena, rs, seed, erased, survivors=None, junk=(), pitch=ALIGNED, form="2d"):
    """Rows ``erased`` and ``junk`` hold garbage; the ``junk`` rows must not be read and stay as they are."""
    def run():
        arena.reset()
        s = arena.rows(0, rs.n, 1000, pitch)
        truth = stripe_of(rs, noise(seed, rs.k, 1000))
        broken = np.array(truth)
        broken[list(erased) + list(junk)] = noise(seed + 100, len(erased) + len(junk), 1000)
        s.put(broken)
        rs.reconstruct(s.t if form == "2d" else s.rows(), erased, survivors)
        if survivors is None:
            s.h[...] = gf.reconstruct_oracle(rs.G, broken, erased)
        else:  # (any k intact rows of an MDS code give back the stripe that was encoded)
            s.h[list(erased)] = truth[list(erased)]
        arena.check(("reconstruct", erased, survivors, junk, pitch, form))
    return run


@pytest.mark.parametrize("what", ["erased", "survivors", "pitch", "unaligned", "list"])
def test_reconstruct(arena, what):
    rs = codec()
    if what == "survivors":  # the default survivors are 0, 2, 3, 4: the other call must not read row 4
        x, y = dict(erased=[1], junk=[5]), dict(erased=[1], survivors=[0, 2, 3, 5], junk=[4])
    else:
        x = dict(erased=[1, 4])
        y = other(x, {"erased": dict(erased=[0, 5]), "pitch": dict(pitch=WIDER), "unaligned": dict(pitch=ODD),
                      "list": dict(form="rows")}, what)
    # (a list of the same rows is the same call: the key names the rows, so it may share the plan)
    pair(rs, reconstruct_call(arena, rs, 1, **x), reconstruct_call(arena, rs, 2, **y), grows=what != "list")


class Stripes:
    """B stripes of n rows of the arena as the batched calls take them: one ``[B, n, C]`` tensor in region
    0 (``split`` None); its natives and its parity rows as two arguments (``"same"``: the same
    addresses); or the natives where they were and the parity in region 1 (``"moved"``). ``form``:
    tensors, or lists of stripes of row tensors."""

    def __init__(self, arena, rs, nb=B, C=1000, pitch=ALIGNED, gap=0, split=None, form="tensor"):
        n, k = rs.n, rs.k
        self.k, self.split, self.form = k, split, form
        self.whole = arena.batch(0, nb, n, C, pitch, gap)
        self.nat, self.par = self.whole[:, :k], self.whole[:, k:]
        if split == "moved":
            self.whole, self.par = None, arena.batch(1, nb, n - k, C, pitch, gap)

    def put(self, full: np.ndarray) -> None:
        self.nat.put(full[:, : self.k])
        self.par.put(full[:, self.k:])

    def expect(self, full: np.ndarray) -> None:
        self.nat.h[...] = full[:, : self.k]
        self.par.h[...] = full[:, self.k:]

    def poke(self, b: int, j: int, col, value) -> None:
        """Damage on the device alone."""
        (self.nat if j < self.k else self.par).t[b, j if j < self.k else j - self.k, col] = value

    def args(self):
        """(stripes, parity) for the codec."""
        f = (lambda v: v.t) if self.form == "tensor" else (lambda v: v.lists())
        return (f(self.whole), None) if self.split is None else (f(self.nat), f(self.par))


LAYOUTS = {"batch-stride": dict(gap=GAP), "pitch": dict(pitch=WIDER), "unaligned": dict(pitch=ODD),
           "parity-apart": dict(split="same"), "parity-moved": dict(split="moved")}


def reconstruct_batch_call(arena, rs, seed, erased, **layout):
    def run():
        arena.reset()
        s = Stripes(arena, rs, **layout)
        truth = stripe_of(rs, noise(seed, B, rs.k, 1000))
        ids = np.asarray(erased)
        per = [[int(e) for e in (ids if ids.ndim == 1 else ids[b]) if e >= 0] for b in range(B)]
        broken = np.array(truth)
        for b in range(B):
            broken[b, per[b]] = noise(seed + 100 + b, len(per[b]), 1000)
        s.put(broken)
        stripes, parity = s.args()
        assert rs.reconstruct_batch(stripes, erased, parity) is stripes
        s.expect(np.stack([gf.reconstruct_oracle(rs.G, broken[b], per[b]) for b in range(B)]))
        assert np.array_equal(np.concatenate([s.nat.h, s.par.h], axis=1), truth)  # (MDS: the oracle restores it)
        arena.check(("reconstruct_batch", erased, layout))
    return run


@pytest.mark.parametrize("what", ["one-stripes-ids", "shared-list-or-array"] + list(LAYOUTS))
@pytest.mark.parametrize("form", ["tensor", "lists"])
def test_reconstruct_batch(arena, form, what):
    rs = codec()
    ids = np.array([[1, 4], [0, -1], [2, 3]])
    x = dict(erased=ids, form=form)
    if what == "one-stripes-ids":
        y = dict(x, erased=np.array([[1, 4], [0, -1], [2, 5]]))
    elif what == "shared-list-or-array":  # the same ids for every stripe, said twice: one plan or two
        x, y = dict(x, erased=[1, 4]), dict(x, erased=np.array([[1, 4]] * B))
    elif what == "parity-moved":          # the natives at the same addresses in both calls
        x, y = dict(x, split="same"), dict(x, split="moved")
    else:
        y = dict(x, **LAYOUTS[what])
    pair(rs, reconstruct_batch_call(arena, rs, 1, **x), reconstruct_batch_call(arena, rs, 2, **y),
         grows=what != "shared-list-or-array")


# ---- (a) the scrub family -------------------------------------------------------------------------------
def damage(seed, n: int, C: int, chunks: int = 1):
    """[(chunk, columns, xor values)]: ``chunks`` chunks wrong in a few dozen columns each, the last column
    of the row among them."""
    rng = np.random.default_rng(seed)
    out = []
    for j in rng.choice(n, size=chunks, replace=False).tolist():
        cols = np.unique(np.concatenate([rng.integers(0, C, size=40), [C - 1]]))
        out.append((j, cols, rng.integers(1, 256, size=cols.size, dtype=np.uint8)))
    return out


def check_scrub_report(rep, h, rows, block_bytes):
    mask, votes, unlocated, bad = gf.scrub_oracle(h, rows, block_bytes)
    assert np.array_equal(rep.mask.cpu().numpy(), mask)
    assert (rep.bad_columns, rep.unlocated, rep.clean) == (bad, unlocated, bad == 0)
    assert np.array_equal(rep.votes, votes) and rep.suspects == np.nonzero(votes)[0].tolist()


def scrub_call(arena, rs, op, seed, C=1000, block_bytes=65536, pitch=ALIGNED, perm=None, form="2d", enc_e=None,
               broken=True):
    """``syndrome_mask`` / ``scrub`` / ``heal`` of one stripe with one chunk wrong. ``perm``: row i of the
    stripe is row ``perm[i]`` of the region (a list of rows in another order of allocation). ``enc_e``:
    the matrix the stripe was encoded with, if not the codec's."""
    def run():
        arena.reset()
        s = arena.rows(0, rs.n, C, pitch)
        order = list(range(rs.n)) if perm is None else list(perm)
        truth = stripe_of(rs, noise(seed, rs.k, C), enc_e)
        rows = np.array(truth)
        for j, cols, x in damage(seed, rs.n, C) if broken else []:
            rows[j, cols] ^= x
        phys = np.empty_like(rows)
        phys[order] = rows
        s.put(phys)
        stripe = s.t if form == "2d" and perm is None else [s.t[i] for i in order]
        if op == "syndrome_mask":
            mask = rs.syndrome_mask(stripe, block_bytes)
            assert np.array_equal(mask.cpu().numpy(), gf.scrub_oracle(rs.H, rows, block_bytes)[0])
        elif op == "scrub":
            check_scrub_report(rs.scrub(stripe, block_bytes), rs.H, rows, block_bytes)
        else:
            rep = rs.heal(stripe)
            assert rep.clean and rep.bad_columns == 0
            s.h[order] = truth
        arena.check((op, C, block_bytes, pitch, perm, form))
    return run


SCRUB_PERM = [3, 0, 5, 1, 4, 2]


def without(ops, whats, missing):
    """(op, what) pairs, less those for which the call has no such argument."""
    return [(op, what) for op in ops for what in whats if what not in missing.get(op, ())]


BLOCKS = ("block-bytes", "block-bytes-5000")


@pytest.mark.parametrize("op,what", without(["syndrome_mask", "scrub", "heal"],
                                            BLOCKS + ("pitch", "unaligned", "list", "list-order"), {"heal": BLOCKS}))
def test_scrub_single(arena, op, what):
    rs = codec()
    if what.startswith("block-bytes"):
        x = dict(C=5000 if what.endswith("5000") else 1000, pitch=5120 if what.endswith("5000") else ALIGNED)
        x, y = dict(x, block_bytes=4096), dict(x, block_bytes=65536)
    else:
        x = {}
        y = other(x, {"pitch": dict(pitch=WIDER), "unaligned": dict(pitch=ODD), "list": dict(form="rows"),
                      "list-order": dict(perm=SCRUB_PERM)}, what)
    pair(rs, scrub_call(arena, rs, op, 1, **x), scrub_call(arena, rs, op, 2, **y), grows=what != "list")


def scrub_batch_call(arena, rs, op, seed, C=1000, block_bytes=65536, enc_e=None, broken=True, **layout):
    """The batched forms: stripe 0 clean, stripes 1 and 2 with one wrong chunk each."""
    def run():
        arena.reset()
        s = Stripes(arena, rs, C=C, **layout)
        truth = stripe_of(rs, noise(seed, B, rs.k, C), enc_e)
        rows = np.array(truth)
        for b in range(1, B) if broken else []:
            for j, cols, x in damage(seed + b, rs.n, C):
                rows[b, j, cols] ^= x
        s.put(rows)
        stripes, parity = s.args()
        oracle = [gf.scrub_oracle(rs.H, rows[b], block_bytes) for b in range(B)]
        if op == "syndrome_mask_batch":
            mask = rs.syndrome_mask_batch(stripes, parity, block_bytes)
            assert np.array_equal(mask.cpu().numpy(), np.stack([o[0] for o in oracle]))
        elif op == "scrub_batch":
            rep = rs.scrub_batch(stripes, parity, block_bytes)
            assert rep.dirty == [b for b in range(B) if oracle[b][3]]
            for b in range(B):
                check_scrub_report(rep.report[b], rs.H, rows[b], block_bytes)
        else:
            rep = rs.heal_batch(stripes, parity)
            assert bool(rep.clean.all()) and rep.dirty == [] and rep.unhealed == []
            s.expect(truth)
        arena.check((op, C, block_bytes, layout))
    return run


@pytest.mark.parametrize("op,what", without(["syndrome_mask_batch", "scrub_batch", "heal_batch"],
                                            BLOCKS + ("lists",) + tuple(LAYOUTS), {"heal_batch": BLOCKS}))
def test_scrub_batch(arena, op, what):
    rs = codec()
    if what.startswith("block-bytes"):
        x = dict(C=5000, pitch=5120) if what.endswith("5000") else {}
        x, y = dict(x, block_bytes=4096), dict(x, block_bytes=65536)
    elif what == "parity-moved":
        x, y = dict(split="same"), dict(split="moved")
    else:
        x = {}
        y = dict(form="lists") if what == "lists" else LAYOUTS[what]
    pair(rs, scrub_batch_call(arena, rs, op, 1, **x), scrub_batch_call(arena, rs, op, 2, **y))


# ---- (a) correct ----------------------------------------------------------------------------------------
def flips(seed, n: int, C: int):
    """[(chunk, column, xor value)]: one wrong byte in each of six columns (the first and the last among
    them) and two wrong chunks in each of three more."""
    rng = np.random.default_rng(seed)
    cols = np.concatenate([[0, C - 1], 1 + rng.choice(C - 2, size=7, replace=False)]).tolist()
    out = [(int(rng.integers(0, n)), c, int(rng.integers(1, 256))) for c in cols[:6]]
    for c in cols[6:]:
        j1, j2 = rng.choice(n, size=2, replace=False).tolist()
        out += [(j1, c, int(rng.integers(1, 256))), (j2, c, int(rng.integers(1, 256)))]
    return out


def check_correct_report(rep, oracle):
    _, fixed, by_weight, unc, bad = oracle
    assert (rep.bad_columns, rep.uncorrectable, rep.clean) == (bad, unc, bad == 0)
    assert np.array_equal(rep.fixed_bytes, fixed) and np.array_equal(rep.by_weight, by_weight)


def correct_call(arena, rs, seed, max_errors=2, C=1000, block_bytes=65536, pitch=ALIGNED, form="2d"):
    def run():
        arena.reset()
        s = arena.rows(0, rs.n, C, pitch)
        rows = stripe_of(rs, noise(seed, rs.k, C))
        for j, c, x in flips(seed, rs.n, C):
            rows[j, c] ^= x
        s.put(rows)
        oracle = gf.correct_oracle(rs.H, rows, max_errors)
        assert oracle[2][max_errors] > 0 and (oracle[3] > 0) == (max_errors == 1)  # (the case is what it says)
        rep = rs.correct(s.t if form == "2d" else s.rows(), max_errors, block_bytes)
        check_correct_report(rep, oracle)
        assert np.array_equal(rep.mask.cpu().numpy(), gf.scrub_oracle(rs.H, rows, block_bytes)[0])
        s.h[...] = oracle[0]
        arena.check(("correct", max_errors, C, block_bytes, pitch, form))
    return run


CORRECT = {"max-errors": (dict(max_errors=1), dict(max_errors=2)),
           "block-bytes": (dict(block_bytes=4096), dict(block_bytes=65536)),
           "block-bytes-5000": (dict(C=5000, pitch=5120, block_bytes=4096),
                                dict(C=5000, pitch=5120, block_bytes=65536)),
           "pitch": ({}, dict(pitch=WIDER)), "unaligned": ({}, dict(pitch=ODD))}


@pytest.mark.parametrize("what", list(CORRECT) + ["list"])
def test_correct(arena, what):
    rs = codec(CODE2)
    x, y = CORRECT.get(what, ({}, dict(form="rows")))
    pair(rs, correct_call(arena, rs, 1, **x), correct_call(arena, rs, 2, **y), grows=what != "list")


def correct_batch_call(arena, rs, seed, max_errors=2, C=1000, block_bytes=65536, **layout):
    def run():
        arena.reset()
        s = Stripes(arena, rs, C=C, **layout)
        rows = stripe_of(rs, noise(seed, B, rs.k, C))
        for b in range(1, B):  # (stripe 0 is clean)
            for j, c, x in flips(seed + b, rs.n, C):
                rows[b, j, c] ^= x
        s.put(rows)
        oracle = [gf.correct_oracle(rs.H, rows[b], max_errors) for b in range(B)]
        stripes, parity = s.args()
        rep = rs.correct_batch(stripes, parity, max_errors, block_bytes)
        assert rep.dirty == [1, 2]
        for b in range(B):
            check_correct_report(rep.report[b], oracle[b])
        s.expect(np.stack([o[0] for o in oracle]))
        arena.check(("correct_batch", max_errors, C, block_bytes, layout))
    return run


@pytest.mark.parametrize("what", list(CORRECT) + ["lists", "batch-stride", "parity-apart", "parity-moved"])
def test_correct_batch(arena, what):
    rs = codec(CODE2)
    if what == "parity-moved":
        x, y = dict(split="same"), dict(split="moved")
    else:
        x, y = CORRECT.get(what) or ({}, dict(form="lists") if what == "lists" else LAYOUTS[what])
    pair(rs, correct_batch_call(arena, rs, 1, **x), correct_batch_call(arena, rs, 2, **y))


# ---- (a) update, update_delta, write --------------------------------------------------------------------
def update_call(arena, rs, op, seed, changed=(1, 3), sp=ALIGNED, op_=ALIGNED, np_=ALIGNED, own_old=False, col0=0,
                ncols=None, raises=None, stripe_form="2d"):
    """One partial-stripe write of natives ``changed``. The stripe lies in region 0 (pitch ``sp``), the
    old rows (``update``; ``own_old``: the stripe's own native rows instead) or the deltas in region 1
    (pitch ``op_``), the new rows in region 2 (pitch ``np_``). Expected: inside the window the oracle's
    parity of the updated natives (and for ``write`` the new natives), outside it what was there."""
    def run():
        arena.reset()
        C, d = 1000, len(changed)
        s, o, w = arena.rows(0, rs.n, C, sp), arena.rows(1, d, C, op_), arena.rows(2, d, C, np_)
        data, new = noise(seed, rs.k, C), noise(seed + 50, d, C)
        s.put(stripe_of(rs, data))
        after = np.array(data)
        after[list(changed)] = new
        parity = s.t[rs.k:]
        if op == "update":
            old = [s.t[j] for j in changed] if own_old else o.t
            if not own_old:
                o.put(data[list(changed)])
            w.put(new)
            call = lambda: rs.update(parity, list(changed), old, w.t, col0, ncols)  # noqa: E731
        elif op == "update_delta":
            o.put(data[list(changed)] ^ new)
            call = lambda: rs.update_delta(parity, list(changed), o.t, col0, ncols)  # noqa: E731
        else:
            w.put(new)
            stripe = s.t if stripe_form == "2d" else s.rows()
            call = lambda: rs.write(stripe, list(changed), w.t, col0, ncols)  # noqa: E731
        if raises is not None:
            with pytest.raises(ValueError, match=raises):
                call()
        else:
            call()
            c1 = C if ncols is None else col0 + ncols
            want = stripe_of(rs, after)
            if op != "write":
                want[: rs.k] = data
            s.h[:, col0:c1] = want[:, col0:c1]
        arena.check((op, changed, sp, op_, np_, own_old, col0, ncols, stripe_form))
    return run


@pytest.mark.parametrize("op,what", without(
    ["update", "update_delta", "write"],
    ["changed-order", "parity-pitch", "old-pitch", "new-pitch", "old-unaligned", "one-id", "old-rows-of-the-stripe"],
    {"update_delta": ("new-pitch", "old-rows-of-the-stripe"),
     "write": ("old-pitch", "old-unaligned", "old-rows-of-the-stripe")}))
def test_update_single(arena, op, what):
    rs = codec()
    y = other({}, {"changed-order": dict(changed=(3, 1)), "parity-pitch": dict(sp=WIDER), "old-pitch": dict(op_=WIDER),
                   "new-pitch": dict(np_=WIDER), "old-unaligned": dict(op_=ODD), "one-id": dict(changed=(1, 2)),
                   "old-rows-of-the-stripe": dict(own_old=True)}, what)
    pair(rs, update_call(arena, rs, op, 1), update_call(arena, rs, op, 2, **y))


def test_update_pair_form_against_write_form_on_the_same_rows(arena):
    """``update`` with the stripe's own natives as the old rows, then ``write`` into that stripe: the same
    parity, old and new rows, and the write also stores the natives."""
    rs = codec()
    pair(rs, update_call(arena, rs, "update", 1, own_old=True), update_call(arena, rs, "write", 2))
    count = len(rs._plans)
    update_call(arena, rs, "write", 3, stripe_form="rows")()  # (the same rows as a list: the same plan)
    update_call(arena, rs, "update", 4, own_old=True)()
    assert len(rs._plans) == count


@pytest.mark.parametrize("op", ["update", "update_delta", "write"])
def test_update_window_on_a_cached_plan(arena, op):
    """The window is an argument of the launch, not of the plan: a hit runs the cached plan over another
    window, and refuses one outside the rows as the first call would, with nothing written."""
    rs = codec()
    update_call(arena, rs, op, 1)()
    count = len(rs._plans)
    for col0, ncols in ((16, 100), (5, 33), (999, 1), (512, None)):
        update_call(arena, rs, op, 2 + col0, col0=col0, ncols=ncols)()
    update_call(arena, rs, op, 3, col0=990, ncols=11, raises="outside rows of 1000")()
    update_call(arena, rs, op, 4, col0=-16, ncols=16, raises="outside rows of 1000")()
    update_call(arena, rs, op, 5, col0=1001, raises="outside rows of 1000")()
    assert len(rs._plans) == count
    fresh = codec()  # ... as a first call refuses it
    update_call(arena, fresh, op, 3, col0=990, ncols=11, raises="outside rows of 1000")()
    assert len(fresh._plans) == 0


# ---- (a) the batched updates ----------------------------------------------------------------------------
IDS_B = [[1, 3], [0, 2], [3, 1]]


def update_batch_call(arena, rs, op, seed, ids=IDS_B, pp=ALIGNED, pg=0, op_=ALIGNED, og=0, np_=ALIGNED, ng=0,
                      col0=0, ncols=None, **layout):
    """The batched forms. ``update_batch`` / ``update_delta_batch``: the parity rows in region 0, the old
    rows or deltas in region 1, the new rows in region 2. ``write_batch``: the stripes as ``Stripes`` lays
    them out (regions 0 and 1), the new rows in region 2."""
    def run():
        arena.reset()
        C = 1000
        a = np.asarray(ids.numpy() if isinstance(ids, torch.Tensor) else ids)
        per = np.broadcast_to(a, (B, a.shape[-1])).astype(np.int64)
        d = per.shape[1]
        w = arena.batch(2, B, d, C, np_, ng)
        data, new = noise(seed, B, rs.k, C), noise(seed + 50, B, d, C)
        old = np.take_along_axis(data, per[:, :, None], axis=1)
        after = np.array(data)
        np.put_along_axis(after, per[:, :, None], new, axis=1)
        c1 = C if ncols is None else col0 + ncols
        if op == "write_batch":
            s = Stripes(arena, rs, **layout)
            s.put(stripe_of(rs, data))
            w.put(new)
            stripes, parity = s.args()
            assert rs.write_batch(stripes, ids, w.t, parity, col0, ncols) is stripes
            want = stripe_of(rs, after)
            s.nat.h[:, :, col0:c1] = want[:, : rs.k, col0:c1]
            s.par.h[:, :, col0:c1] = want[:, rs.k:, col0:c1]
        else:
            p, o = arena.batch(0, B, rs.p, C, pp, pg), arena.batch(1, B, d, C, op_, og)
            p.put(parity_of(rs, data))
            if op == "update_batch":
                o.put(old)
                w.put(new)
                assert rs.update_batch(p.t, ids, o.t, w.t, col0, ncols) is p.t
            else:
                o.put(old ^ new)
                assert rs.update_delta_batch(p.t, ids, o.t, col0, ncols) is p.t
            p.h[:, :, col0:c1] = parity_of(rs, after)[:, :, col0:c1]
        arena.check((op, np.asarray(per).tolist(), pp, pg, op_, og, np_, ng, col0, ncols, layout))
    return run


UPDB = {"one-stripes-ids": dict(ids=[[1, 3], [0, 2], [3, 0]]), "ids-order": dict(ids=[[3, 1], [0, 2], [3, 1]]),
        "parity-pitch": dict(pp=WIDER), "parity-batch-stride": dict(pg=GAP), "old-pitch": dict(op_=WIDER),
        "old-batch-stride": dict(og=GAP), "old-unaligned": dict(op_=ODD), "new-pitch": dict(np_=WIDER),
        "new-batch-stride": dict(ng=GAP)}


@pytest.mark.parametrize("op,what", without(["update_batch", "update_delta_batch"], list(UPDB),
                                            {"update_delta_batch": ("new-pitch", "new-batch-stride")}))
def test_update_batch(arena, op, what):
    rs = codec()
    pair(rs, update_batch_call(arena, rs, op, 1), update_batch_call(arena, rs, op, 2, **UPDB[what]))


@pytest.mark.parametrize("what", ["one-stripes-ids", "ids-order", "new-pitch", "new-batch-stride", "lists"]
                         + list(LAYOUTS))
def test_write_batch(arena, what):
    rs = codec()
    if what == "parity-moved":
        x, y = dict(split="same"), dict(split="moved")
    else:
        x = {}
        y = UPDB.get(what) or (dict(form="lists") if what == "lists" else LAYOUTS[what])
    pair(rs, update_batch_call(arena, rs, "write_batch", 1, **x), update_batch_call(arena, rs, "write_batch", 2, **y))


@pytest.mark.parametrize("op", ["update_batch", "update_delta_batch", "write_batch"])
def test_update_batch_ids_as_list_array_and_tensor(arena, op):
    """The same ids as a nested list, an int32 array and an int64 tensor (one plan or three), one list for
    every stripe against that list per stripe, and a window on the cached plan."""
    rs = codec()
    forms = [IDS_B, np.array(IDS_B, dtype=np.int32), torch.tensor(IDS_B, dtype=torch.int64),
             np.asfortranarray(np.array(IDS_B, dtype=np.int64)), np.array(IDS_B, dtype=np.uint8)]
    for seed, ids in enumerate(forms):
        update_batch_call(arena, rs, op, seed, ids=ids)()
    count = len(rs._plans)
    update_batch_call(arena, rs, op, 7, ids=IDS_B)()
    update_batch_call(arena, rs, op, 8, ids=np.array(IDS_B), col0=16, ncols=100)()
    update_batch_call(arena, rs, op, 9, ids=np.array(IDS_B), col0=5, ncols=33)()
    assert len(rs._plans) == count
    with pytest.raises(ValueError, match="outside rows of 1000"):
        update_batch_call(arena, rs, op, 9, ids=np.array(IDS_B), col0=990, ncols=11)()
    arena.check("a refused window wrote nothing")
    update_batch_call(arena, rs, op, 10, ids=[2, 0])()
    update_batch_call(arena, rs, op, 11, ids=np.array([[2, 0]] * B))()
    update_batch_call(arena, rs, op, 12, ids=[0, 2])()
    update_batch_call(arena, rs, op, 13, ids=IDS_B)()


# ---- (b) reassigning the matrices -----------------------------------------------------------------------
def swap_matrices(rs, code) -> None:
    k, n, _ = code
    new = ReedSolomon(k, n, matrix="sys_vandermonde")
    assert not np.array_equal(new.E, rs.E)
    rs.E = new.E
    rs.G = new.G


@pytest.mark.parametrize("op", ["encode_batch", "reconstruct_batch", "scrub_batch", "correct_batch", "write_batch",
                                "update"])
def test_reassigning_the_matrices_drops_every_cached_plan(arena, op):
    """A cached plan's tables hold the old matrix's coefficients, and no key names the matrix. The calls
    below compute their oracles from ``rs.E`` / ``rs.G`` / ``rs.H`` when they run, so the second run
    must follow the new matrix on the very views of the first."""
    code = CODE2 if op == "correct_batch" else CODE
    rs = codec(code)
    old_e = rs.E
    call = {"encode_batch": lambda: encode_batch_call(arena, rs, 1),
            "reconstruct_batch": lambda: reconstruct_batch_call(arena, rs, 1, np.array([[1, 4], [0, -1], [2, 3]])),
            # a stripe that is consistent under the old matrix: clean before, dirty as the oracle says after
            "scrub_batch": lambda: scrub_batch_call(arena, rs, "scrub_batch", 1, enc_e=old_e, broken=False),
            "correct_batch": lambda: correct_batch_call(arena, rs, 1),
            "write_batch": lambda: update_batch_call(arena, rs, "write_batch", 1),
            "update": lambda: update_call(arena, rs, "update", 1)}[op]()
    call()
    call()  # (a hit)
    assert len(rs._plans) > 0
    swap_matrices(rs, code)
    assert len(rs._plans) == 0 and len(rs._upd_keys) == 0
    if op == "scrub_batch":
        h = gf.check_matrix(rs.E)
        stripe = stripe_of(rs, noise(1, B, rs.k, 1000), old_e)
        assert all(gf.scrub_oracle(h, stripe[b])[3] > 0 for b in range(B))  # (the case is what it says)
    call()
    call()


# ---- (c) eviction ---------------------------------------------------------------------------------------
SET_BYTES = 16 << 10  # six buffer sets per region


def test_eviction_under_the_two_keys_of_the_2d_encode(arena):
    """Capacity 4, six buffer sets, two rounds: each call stores its plan under two keys, so the second
    round finds every plan evicted and every fast key stale or gone."""
    rs = codec()
    rs._plans.capacity = 4
    for rnd in range(2):
        for i in range(6):
            arena.reset()
            d, p = arena.rows(0, rs.k, 1000, off=i * SET_BYTES), arena.rows(1, rs.p, 1000, off=i * SET_BYTES)
            host = noise(10 * rnd + i, rs.k, 1000)
            d.put(host)
            for _ in range(2):  # (a miss, then a hit on the fast key)
                rs.encode(d.t, p.t)
                assert len(rs._plans) <= 4
            p.h[...] = parity_of(rs, host)
            arena.check(("encode", rnd, i))
    assert len(rs._plans) == 4


def test_update_again_after_its_plan_was_evicted(arena):
    """``_upd_keys`` remembers the plan key of a repeated update; after five other buffer sets that key
    names an evicted plan, and the call must build it again."""
    rs = codec()
    rs._plans.capacity = 4

    def update(i, seed):
        arena.reset()
        off = i * SET_BYTES
        p, o, w = (arena.rows(r, 2, 1000, off=off) for r in range(3))
        data, new = noise(seed, rs.k, 1000), noise(seed + 50, 2, 1000)
        after = np.array(data)
        after[[1, 3]] = new
        p.put(parity_of(rs, data))
        o.put(data[[1, 3]])
        w.put(new)
        rs.update(p.t, [1, 3], o.t, w.t)
        p.h[...] = parity_of(rs, after)
        arena.check(("update", i, seed))
        assert len(rs._plans) <= 4

    update(0, 1)
    update(0, 2)
    (key,) = rs._plans
    for i in range(1, 6):
        update(i, 10 + i)
    assert key not in rs._plans and key in rs._upd_keys.values()
    update(0, 3)
    assert key in rs._plans and len(rs._plans) == 4
    update(0, 4)


# ---- (d) every plan on one stripe at once ---------------------------------------------------------------
STEPS = ["write", "write_batch", "update", "reconstruct", "reconstruct_batch", "correct", "correct_batch", "heal",
         "heal_batch", "scrub_batch"]


def test_forty_steps_on_one_batch(arena):
    """A model-based sequence on one ``[3, 14, 1000]`` batch of a (10, 14) Cauchy code, whose distance 5
    lets every damage below be undone: after each step the stripes equal the numpy mirror's natives and
    the oracle's parity of them, nothing else in the arena has moved, and ``scrub_batch`` calls the batch
    clean. The plans of all the ops then sit in the cache for the same addresses."""
    rs = codec(CODE2)
    k, n, C = rs.k, rs.n, 1000
    rng = np.random.default_rng(40)
    arena.reset()
    s = Stripes(arena, rs, C=C)
    new = arena.batch(2, B, 4, C)
    natives = noise(0, B, k, C)
    s.put(stripe_of(rs, natives))
    order = rng.permutation(np.repeat(np.arange(len(STEPS)), 4))
    assert order.size == 40
    for step, which in enumerate(order.tolist()):
        op = STEPS[which]
        b = int(rng.integers(0, B))
        if op in ("write", "write_batch", "update"):
            d = int(rng.integers(1, 5))
            ids = np.stack([rng.permutation(k)[:d] for _ in range(B)])
            fresh = noise(1000 + step, B, d, C)
            new[:, :d].put(fresh)
            if op == "write_batch":
                rs.write_batch(s.whole.t, ids, new.t[:, :d])
                np.put_along_axis(natives, ids[:, :, None], fresh, axis=1)
            else:
                ch = ids[b].tolist()
                if op == "write":
                    rs.write(s.whole.t[b], ch, new.t[b, :d])
                else:
                    rs.update(s.par.t[b], ch, [s.nat.t[b, j] for j in ch], new.t[b, :d])
                    for t, j in enumerate(ch):  # (update leaves the natives to the caller)
                        s.nat.t[b, j].copy_(new.t[b, t])
                natives[b, ch] = fresh[b]
        elif op in ("reconstruct", "reconstruct_batch"):
            erased = np.full((B, 4), -1, dtype=np.int64)
            for q in range(B) if op == "reconstruct_batch" else [b]:
                lost = rng.permutation(n)[: int(rng.integers(1, 5))]
                erased[q, : lost.size] = lost
                for j in lost.tolist():
                    s.whole.t[q, j].copy_(torch.from_numpy(noise(2000 + 20 * step + j, C)))
            if op == "reconstruct":
                rs.reconstruct(s.whole.t[b], [int(e) for e in erased[b] if e >= 0])
            else:
                rs.reconstruct_batch(s.whole.t, erased)
        elif op in ("correct", "correct_batch"):
            for q in range(B) if op == "correct_batch" else [b]:
                for j, c, x in flips(3000 + 10 * step + q, n, C):
                    s.poke(q, j, c, int(s.whole.h[q, j, c]) ^ x)  # (the mirror holds the right byte)
            rep = rs.correct(s.whole.t[b]) if op == "correct" else rs.correct_batch(s.whole.t)
            assert not np.any(rep.uncorrectable) and int(np.sum(rep.by_weight)) == (9 if op == "correct" else 9 * B)
        elif op in ("heal", "heal_batch"):
            for q in range(B) if op == "heal_batch" else [b]:
                j = int(rng.integers(0, n))
                s.whole.t[q, j].copy_(torch.from_numpy(noise(4000 + 10 * step + q, C)))
            rep = rs.heal(s.whole.t[b]) if op == "heal" else rs.heal_batch(s.whole.t)
            assert np.all(rep.clean)
        s.expect(stripe_of(rs, natives))
        arena.check((step, op))
        rep = rs.scrub_batch(s.whole.t)
        assert bool(rep.clean.all()) and rep.dirty == [], (step, op)
    ops = {key[0] if isinstance(key[0], str) else key[0][0] for key in rs._plans}
    assert {"upd", "updb", "rep", "repb", "scrub", "scrubb", "correct", "correctb"} <= ops, ops

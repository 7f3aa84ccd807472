"""What a plan-cache key must say (``gpu_rscode_amd/ops/rows.py``, ``models/rs.py``). CPU only.

A cached plan stores raw row addresses, so a part's ``key`` may be equal for two parts only if a plan
built from one is right for the other: the same ``[B, r]`` row addresses, the same counts and the same
row lengths. Every pair below lies in one byte buffer, shares its base pointer where it can and
differs in exactly one property; two layouts that are equal must have equal keys whatever Python
objects they were built from (else a repeat call never hits). Then the LRU dictionary itself."""
import numpy as np
import pytest
import torch

from gpu_rscode_amd.models.rs import _PlanCache
from gpu_rscode_amd.ops.rows import ListPart, PickPart, StripeBatch, TensorPart

BUF = torch.zeros(1 << 16, dtype=torch.uint8)
B, R, C, PITCH = 3, 4, 100, 128  # the base layout: 3 stripes of 4 rows of 100 bytes, 128 bytes apart
K, N = 4, 6                      # the stripes of a StripeBatch: 4 natives, 2 parity rows


def view(b=B, r=R, c=C, bstride=None, pitch=PITCH, off=0) -> torch.Tensor:
    """(the batch stride does not follow ``pitch``: rows of neighbouring stripes may overlap, which no part minds)"""
    return BUF.as_strided((b, r, c), (r * PITCH if bstride is None else bstride, pitch, 1), off)


def layout(part) -> tuple:
    """Everything a plan takes from a part."""
    ptrs = np.asarray(part.ptrs())
    lens = getattr(part, "lens", part.ncols)
    return (part.nstripes, part.n if isinstance(part, StripeBatch) else part.nrows, part.ncols,
            lens if isinstance(lens, int) else (lens.shape, lens.tobytes()), ptrs.shape, ptrs.dtype.str, ptrs.tobytes())


def check_pair(a, b, differ: bool | None = True) -> None:
    """Equal keys only for equal layouts. ``differ`` True: the pair's layouts are different (so the keys
    must be); False: they are equal and the keys must be equal and hash alike; None: equal layouts that
    may have one key or two."""
    assert (layout(a) != layout(b)) == bool(differ), "the pair is not what the test means it to be"
    if a.key == b.key:
        assert layout(a) == layout(b), (a.key, b.key)
    if differ is False:
        assert a.key == b.key and hash(a.key) == hash(b.key)
        assert {a.key: 1}[b.key] == 1


# one property each: the keyword arguments of view() for the second layout of a pair
VIEWS = {
    "batch-stride": dict(bstride=R * PITCH + 64),
    "row-stride": dict(pitch=160),
    "offset": dict(off=16),
    "B": dict(b=2),
    "rows": dict(r=3, bstride=R * PITCH),
    "C": dict(c=90),
}


def as_lists(t: torch.Tensor):
    return [[t[b, j] for j in range(t.shape[1])] for b in range(t.shape[0])]


def as_stripes(t: torch.Tensor):
    return [t[b] for b in range(t.shape[0])]


@pytest.mark.parametrize("what", list(VIEWS))
def test_tensor_part(what):
    check_pair(TensorPart(view(), "x"), TensorPart(view(**VIEWS[what]), "x"))


@pytest.mark.parametrize("form", [as_lists, as_stripes], ids=["rows", "2d"])
@pytest.mark.parametrize("what", list(VIEWS))
def test_list_part(what, form):
    check_pair(ListPart(form(view()), "x"), ListPart(form(view(**VIEWS[what])), "x"))


def test_list_part_two_stripes_of_three_rows_against_three_of_two():
    """The same six row tensors in the same order: equal pointer bytes, another [B, r] shape."""
    rows = [BUF[i * PITCH: i * PITCH + C] for i in range(6)]
    a = ListPart([rows[0:3], rows[3:6]], "x")
    b = ListPart([rows[0:2], rows[2:4], rows[4:6]], "x")
    assert a.ptrs().tobytes() == b.ptrs().tobytes() and a.ptrs().shape != b.ptrs().shape
    check_pair(a, b)
    # ... and with lengths of their own (the ragged form keeps a [B, r] array of them)
    ragged = [r[: C - 8 * i] for i, r in enumerate(rows)]
    check_pair(ListPart([ragged[0:3], ragged[3:6]], "x", ragged=True),
               ListPart([ragged[0:2], ragged[2:4], ragged[4:6]], "x", ragged=True))
    check_pair(ListPart([rows], "x"), ListPart([[r] for r in rows], "x"))


def test_list_part_one_rows_pointer_and_one_rows_length():
    base = as_lists(view())
    moved = as_lists(view())
    moved[1][2] = BUF[40 * PITCH: 40 * PITCH + C]
    check_pair(ListPart(base, "x"), ListPart(moved, "x"))
    swapped = as_lists(view())
    swapped[0][1], swapped[0][2] = swapped[0][2], swapped[0][1]
    check_pair(ListPart(base, "x"), ListPart(swapped, "x"))
    # a single stripe's rows may differ in length: the shortest counts, and each length is the plan's business
    rows = base[0]
    even = ListPart([rows], "x", ragged=True)
    short1 = ListPart([[rows[0], rows[1][:90], rows[2], rows[3]]], "x", ragged=True)
    short2 = ListPart([[rows[0], rows[1], rows[2][:90], rows[3]]], "x", ragged=True)
    all90 = ListPart([[r[:90] for r in rows]], "x", ragged=True)
    assert (even.ncols, short1.ncols, short2.ncols, all90.ncols) == (100, 90, 90, 90)
    for a, b in ((even, short1), (short1, short2), (short1, all90), (even, all90)):
        check_pair(a, b)


def test_equal_layouts_from_other_objects_have_equal_keys():
    check_pair(TensorPart(view(), "x"), TensorPart(view(), "y"), differ=False)
    for form in (as_lists, as_stripes):
        check_pair(ListPart(form(view()), "x"), ListPart(form(view()), "x"), differ=False)
    check_pair(ListPart(as_lists(view()), "x"), ListPart(as_stripes(view()), "x"), differ=False)
    check_pair(ListPart(as_lists(view()), "x"), ListPart(tuple(tuple(s) for s in as_lists(view())), "x"), differ=False)
    rows = as_lists(view())[0]
    check_pair(ListPart([rows], "x", ragged=True), ListPart([view()[0]], "x"), differ=False)
    ragged = [rows[0], rows[1][:90], rows[2], rows[3]]
    check_pair(ListPart([ragged], "x", ragged=True), ListPart([list(r[:] for r in ragged)], "x", ragged=True),
               differ=False)
    ids = [[0, 2], [1, 3], [3, 0]]
    check_pair(PickPart(TensorPart(view(), "x"), np.array(ids, dtype=np.int32)),
               PickPart(TensorPart(view(), "x"), np.array(ids, dtype=np.int64)), differ=False)
    # (a strided id array: its bytes in memory are not the ids' bytes)
    wide = np.array([[0, 9, 2, 9], [1, 9, 3, 9], [3, 9, 0, 9]], dtype=np.int64)
    check_pair(PickPart(TensorPart(view(), "x"), np.array(ids)), PickPart(TensorPart(view(), "x"), wide[:, ::2]),
               differ=False)
    check_pair(StripeBatch(view(r=N), N), StripeBatch(view(r=N), N), differ=False)
    check_pair(StripeBatch(view(r=N)[:, :K], N, view(r=N)[:, K:], K),
               StripeBatch(view(r=N)[:, :K], N, as_stripes(view(r=N)[:, K:]), K), differ=None)


@pytest.mark.parametrize("what", list(VIEWS))
def test_pick_part_source(what):
    ids = np.array([[0, 2], [1, 0], [2, 1]])
    other = view(**VIEWS[what])
    # (rows 0..2 of a source of three rows per stripe are those of the source of four: one layout, one key or two)
    differ = None if what == "rows" else True
    check_pair(PickPart(TensorPart(view(), "x"), ids), PickPart(TensorPart(other, "x"), ids[: other.shape[0]]), differ)
    check_pair(PickPart(ListPart(as_lists(view()), "x"), ids),
               PickPart(ListPart(as_lists(other), "x"), ids[: other.shape[0]]), differ)


def test_pick_part_ids_and_tag():
    src = TensorPart(view(), "x")
    ids = np.array([[0, 2], [1, 0], [2, 1]])
    one = np.array(ids)
    one[1, 1] = 3
    check_pair(PickPart(src, ids), PickPart(src, one))
    check_pair(PickPart(src, ids), PickPart(src, ids[:, ::-1]))                   # the same rows in another order
    check_pair(PickPart(src, ids), PickPart(src, ids[:, :1]))                     # fewer rows per stripe
    check_pair(PickPart(src, np.array([[1, 3]] * 3)), PickPart(src, np.array([[1], [3], [1]])))
    # a tag stands in for the ids' bytes: equal ids under two tags may or may not share a key, and the
    # key of a tagged part is not that of an untagged one
    a, b = PickPart(src, ids, tag="parity"), PickPart(src, ids, tag="other")
    check_pair(a, b, differ=None)
    check_pair(a, PickPart(src, ids), differ=None)
    check_pair(a, PickPart(src, np.array(ids), tag="parity"), differ=False)
    assert a.key != b.key and a.key != PickPart(src, ids).key
    # ... but never for another number of rows per stripe (the parity rows of a code with another p)
    check_pair(PickPart(src, np.array([[2, 3]] * 3), tag="parity"), PickPart(src, np.array([[3]] * 3), tag="parity"))
    # nor for another source
    check_pair(PickPart(src, ids, tag="parity"), PickPart(TensorPart(view(off=16), "x"), ids, tag="parity"))


SPLIT = [False, True]


def batch(split: bool, parity_kw=None, lists: bool = False, **kw) -> StripeBatch:
    """B stripes of N rows: one [B, N, C] view, or (``split``) its natives and, 16 KiB further on, a
    parity part of its own (``parity_kw``: that part's view())."""
    form = as_lists if lists else (lambda t: t)
    if not split:
        return StripeBatch(form(view(**{"r": N, **kw})), N)
    par = dict(kw, r=N - K, off=(1 << 14) + kw.get("off", 0))
    par.update(parity_kw or {})
    return StripeBatch(form(view(**{"r": K, **kw})), N, form(view(**par)), K)


@pytest.mark.parametrize("lists", [False, True], ids=["tensor", "lists"])
@pytest.mark.parametrize("split", SPLIT, ids=["whole", "natives+parity"])
@pytest.mark.parametrize("what", [w for w in VIEWS if w != "rows"])
def test_stripe_batch(what, split, lists):
    check_pair(batch(split, lists=lists), batch(split, lists=lists, **VIEWS[what]))


@pytest.mark.parametrize("lists", [False, True], ids=["tensor", "lists"])
@pytest.mark.parametrize("what", ["batch-stride", "row-stride", "offset"])
def test_stripe_batch_parity_part_alone(what, lists):
    kw = {"batch-stride": dict(bstride=(N - K) * PITCH + 64), "row-stride": dict(pitch=160),
          "offset": dict(off=(1 << 14) + 16)}[what]
    check_pair(batch(True, lists=lists), batch(True, kw, lists=lists))


def test_stripe_batch_whole_against_natives_and_parity_at_the_same_addresses():
    """The same rows named as one part or as two: one layout; the keys may differ (two plans), but each
    must still tell its own layouts apart."""
    t = view(r=N)
    whole, two = StripeBatch(t, N), StripeBatch(t[:, :K], N, t[:, K:], K)
    assert layout(whole) == layout(two)
    moved = StripeBatch(t[:, :K], N, view(r=N - K, off=1 << 14), K)
    check_pair(two, moved)
    check_pair(whole, moved)
    # natives [B, 4, C] + parity [B, 2, C] against natives [B, 3, C] + parity [B, 3, C] of a (3, 6) code
    check_pair(two, StripeBatch(t[:, :3], N, t[:, 3:], 3), differ=None)


# ---- the LRU dictionary --------------------------------------------------------------------------------
def test_cache_get_refreshes_recency():
    c = _PlanCache(capacity=3)
    for key in "abc":
        c[key] = key.upper()
    assert c.get("a") == "A" and c.get("zz") is None and c.get("zz", 7) == 7
    c["d"] = "D"  # b is now the least recently used
    assert list(c) == ["c", "a", "d"] and "b" not in c
    assert c.get("c") == "C"
    c["e"] = "E"
    assert list(c) == ["d", "c", "e"]


def test_cache_evicts_only_the_least_recently_used():
    c = _PlanCache(capacity=4)
    for i in range(4):
        c[i] = object()
    kept = {i: c[i] for i in (1, 2, 3)}  # (plain indexing is no use: 0 stays the oldest)
    c[4] = object()
    assert len(c) == 4 and 0 not in c and all(c[i] is v for i, v in kept.items())
    c[2] = kept[2]  # storing again refreshes too, and evicts nothing
    assert len(c) == 4 and list(c) == [1, 3, 4, 2]
    c[5] = object()
    assert list(c) == [3, 4, 2, 5]


def test_cache_one_plan_under_two_keys_survives_the_eviction_of_one():
    c = _PlanCache(capacity=3)
    plan = object()
    c["rows"] = plan
    c["fast"] = plan
    c["x"] = object()
    assert c.get("fast") is plan  # "rows" is the oldest
    c["y"] = object()
    assert "rows" not in c and c.get("fast") is plan and len(c) == 3
    c["rows"] = plan  # what a miss under the evicted key does: the same plan again, "x" goes
    assert list(c) == ["y", "fast", "rows"] and c.get("rows") is c.get("fast")


def test_cache_capacity_can_be_lowered_live():
    c = _PlanCache()
    assert c.capacity == 512
    for i in range(600):
        c[i] = i
    assert len(c) == 512 and next(iter(c)) == 88
    c.capacity = 4
    assert len(c) == 512  # nothing is dropped until the next insert
    c.get(100)
    c["new"] = 0
    assert list(c) == [598, 599, 100, "new"]
    c.capacity = 1
    c["one"] = 1
    assert list(c) == ["one"]

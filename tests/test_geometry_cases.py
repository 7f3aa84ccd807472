"""The geometry cases of tests/test_gpu_geometry.py are what they claim, and the check behind them
can fail (CPU only; tests/geometry_cases.py).

1. The mirror of make_grid + map_block visits every (tile, column block) exactly once.
2. The derived case lists hit their classes: every tail residue, split tail lanes, a block of tail
   lanes only, each block mapping at one and at several tiles, a ragged last lap with the tail lanes
   in it, every window route, a remainder off the 16-byte grid, blocks with 0 / 1 / an even / an odd
   number of chunks, a chunk run across a stripe boundary, every tail_valid value.
3. The whole sweep passes against the numpy reference engine (the replayed stores of the mirror).
4. The sweep fails against numpy engines with one planted geometry fault each, in the family named.
"""
import numpy as np
import pytest

import engine_cases as ec
import geometry_cases as gc


# ---- 1. mapping mirror ------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles", range(1, 17))
def test_mapping_visits_every_tile_and_column_block_once(ntiles):
    for max_blocks in (0, 1, 2, 3, 8, 9):
        for nblk in range(1, 41):
            for items in {(nblk - 1) * gc.KBLOCK + 1, nblk * gc.KBLOCK}:
                g = gc.make_grid(items, ntiles, max_blocks)
                assert g.nblk == nblk and 1 <= g.ncb <= nblk and g.blocks % ntiles == 0
                assert g.ncb == (nblk if max_blocks == 0 else min(nblk, max_blocks))
                live, dead = gc.visits(g, ntiles)
                assert sorted((t, cb) for t, cb, _ in live) == [(t, cb) for t in range(ntiles) for cb in range(nblk)]
                assert len(dead) == g.blocks - g.ncb * ntiles
                assert (gc.mapping(g, ntiles) == "plain") == (g.ncb < 8)


def test_grid_cap_and_slots_mirror():
    assert gc.grid_cap(1) == (2 ** 32 - 1) // 256 // 8 * 8 and gc.grid_cap(3) % 8 == 0
    assert gc.grid_cap(3) * 3 * 256 <= 2 ** 32 - 1
    assert gc.persistent_slots(2, 1, 5) == 8 and gc.persistent_slots(2, 1, 17) == 24
    assert gc.persistent_slots(2, 1, 10 ** 6) == 512 and gc.persistent_slots(1, 3, 10 ** 6) == 80
    assert [gc.persistent_slots(2, 1, n, gc.ONE_SLOT) for n in (1, 5)] == [1, 1]
    assert gc.persistent_slots(2, 3, 5, gc.ONE_SLOT) == 8  # the knob reaches one M-group only
    assert gc.geometry16(20, 12)[1] == 3 and gc.geometry16(20, 8) == (2, 1)
    assert [gc.fp4_route(128, m, False) for m in (12, 16, 20, 26, 32)] == ["v1", "ar", "tm", "tm", "ar"]
    assert gc.fp4_route(128, 32, True) == "tm" and gc.fp4_route(100, 17, True) == "v1"
    assert [gc.fp4_route(128, 24, True, f) for f in ("v1", "ar", "tm")] == ["v1", "ar", "tm"]


def test_mirror_constants_are_the_sources():
    """The defaults and units the mirror copies, read from the sources they come from: a changed
    threshold or chunk size fails here instead of moving the cases off their edges unnoticed."""
    import os
    import re

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")

    def src(*path):
        with open(os.path.join(root, *path)) as f:
            return f.read()

    def value(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return eval(re.sub(r"int64_t\((\d+)\)", r"\1", m.group(1)), {})  # "int64_t(1) << 22" -> 1 << 22

    gemm, gemm16 = src("kernels", "gf_gemm.hip"), src("kernels", "gf_gemm16.hip")
    t = gc.TUNE_DEFAULT
    for key in ("rows_lat_groups", "short_lanes", "ksplit_lanes"):
        assert value(gemm, rf'tune_int\("{key}", ([^;]+?)\)\)?;') == t[key], key
    assert value(gemm16, r'tune_int\("gf16_short_groups", (\d+)\)') == t["gf16_short_groups"]
    assert value(gemm16, r'tune_int\("gf16_vec_g", (\d+)\)') == 2
    assert value(src("include", "gfrs", "device_cache.h"), r'tune_int\("fp4_free_cus", (\d+)\)') == t["fp4_free_cus"]
    assert value(src("include", "gfrs", "perm_device.h"), r"constexpr int kBlock = (\d+);") == gc.KBLOCK
    assert value(gemm, r"constexpr int kSplit = (\d+);") == 8 and "<<<dim3(unsigned(ncb * ntiles), batch), 64 * kSplit" in gemm
    assert value(src("kernels", "gf_gemm_lut.hip"), r"std::min<int64_t>\(nblk, (\d+)\)") == gc.LUT_MAX_NCB
    chunk = lambda e, k, m, cp=True: gc.chunk_of(gc.ENGINES[e], k, m, cp)  # noqa: E731
    assert value(src("kernels", "gf_mfma_fp4.hip"), r"constexpr int kBlockCols = (\d+);") == chunk("mfma_v1", 128, 12)
    assert value(src("kernels", "gf_mfma_fp4tm.hip"), r"constexpr int kBlockCols = (\d+);") == chunk("mfma_tm", 128, 20)
    kcw = value(src("kernels", "gf_mfma_fp4ar.hip"), r"constexpr int kCW = (\d+);")
    assert (4 * kcw, 2 * kcw) == (chunk("mfma_ar", 128, 16), chunk("mfma_ar", 128, 32, False))
    assert value(src("kernels", "gf_mfma.hip"), r"constexpr int kCols = (\d+);") == chunk("mfma_i8", 32, 20, False)
    m16 = src("kernels", "gf_mfma16.hip")
    assert value(m16, r"constexpr int kWaveBytes = (\d+);") * value(m16, r"constexpr int kWaves = (\d+);") == \
        chunk("mfma", 20, 12)
    from gpu_rscode_amd.ops import gemm as ops_gemm
    assert all((gc.tile_for(m), gc.pad_m(m)) == (ops_gemm.tile_for(m), ops_gemm.pad_m(m)) for m in range(1, 257))


# ---- 2. class coverage ------------------------------------------------------------------------------
def _tags(name, families=gc.FAMILIES, m=None):
    e = gc.ENGINES[name]
    tags, kernels, routes = set(), set(), set()
    for f in families:
        for c in gc.cases(name, f):
            if m is not None and c.m != m:
                continue
            for _, copy in gc.layouts(e):
                if gc.runs(e, c.k, c.m, copy):
                    cl = gc.classify(e, c, copy != "none")
                    tags |= cl["tags"]
                    kernels |= set(cl["kernels"])
                    routes.add(cl["route"])
    return tags, kernels, routes


def test_every_engine_has_geometry_cases():
    bases = {e.base for e in gc.ENGINES.values()}
    assert bases == set(ec.ENGINES8) | set(ec.ENGINES16)
    for e in gc.ENGINES.values():
        shape = (ec.ENGINES8 if e.w == 8 else ec.ENGINES16)[e.base]
        if "+forced" not in e.name and e.name not in ("mfma+one_slot", "batched_mfma+one_slot"):  # (one M-group: m = 8)
            assert (e.k, e.m) == shape[:2], e.name
        assert sum(len(gc.cases(e.name, f)) for f in gc.FAMILIES) > 0, e.name
        assert len({c for f in gc.FAMILIES for c in gc.cases(e.name, f)}) == sum(len(gc.cases(e.name, f)) for f in e.families)
    reached = set()
    for name in gc.ENGINES:
        reached |= _tags(name)[1]
    assert reached >= {"vec_v1", "vec_v2", "byte", "byte_serial", "rows", "rows_lat", "ksplit", "lut", "i8", "fp4_v1",
                       "fp4_ar", "fp4_tm", "vec16_g1", "vec16_g2", "sym", "mfma16"}
    # the vec kernel on wide k at 16- and 8-row tiles, the narrowed tile, the forced and the routed FP4 forms
    wide = gc.ENGINES["valu_wide+vec"]
    assert {(l.kernel, l.mt) for m in (wide.m, wide.m1) for l in gc.plan(wide, gc.Case("T", wide.k, m, 4096, 0, 4096))} == \
        {("vec_v2", 16), ("vec_v1", 8)}
    narrow = gc.ENGINES["valu_wide+narrow"]
    assert [(l.kernel, l.mt) for l in gc.plan(narrow, gc.Case("T", narrow.k, narrow.m, 4096, 0, 4096))] == [("vec_v1", 1)]
    for f in ("v1", "ar", "tm"):
        for name in (f"mfma_{f}", f"mfma_{f}+forced", f"mfma_{f}+one_slot"):
            assert f"fp4_{f}" in _tags(name, ("L",))[1], name


def test_refused_shapes_are_not_listed():
    """The rows kernel exists for k in {4, 8, 10, 16} and tiles of at most 4 rows and takes no grid cap;
    GF(2^16) windows are whole symbols; batched plans take no max_blocks; the int8 engine no copies."""
    for e in gc.ENGINES.values():
        for f in gc.FAMILIES:
            for c in gc.cases(e.name, f):
                assert 0 <= c.col0 and c.n > 0 and c.col0 + c.n <= c.nrow
                if e.w == 16:
                    assert c.nrow % 2 == 0 and c.col0 % 2 == 0 and c.n % 2 == 0
                if c.max_blocks:
                    assert e.batch == 1 and e.kind in ("valu", "valu16") and (e.cfg is None or e.cfg[1] > 0)
                if e.cfg is not None and e.cfg[1] <= 0:
                    mt = gc.tile_for(gc.pad_m(c.m)) if e.cfg[1] == 0 else -e.cfg[1]
                    assert c.k in (4, 8, 10, 16) and mt <= 4 and gc.pad_m(c.m) % mt == 0
        if e.kind == "i8":
            assert e.copies == ("none",)


LANE_ENGINES = [n for n, e in gc.ENGINES.items() if "B" in e.families]


@pytest.mark.parametrize("name", LANE_ENGINES)
def test_tail_and_block_classes(name):
    e = gc.ENGINES[name]
    tags, kernels, _ = _tags(name, ("T", "B", "S"))
    kern = gc._first_lane_kernel(e, e.m)
    if kern not in ("byte", "byte_serial", "sym", "ksplit", "lut"):  # these have no tail lanes
        u = gc.unit(e, e.m)
        gb = 16 if kern == "vec16_g2" else u
        assert {f"tail_{t}" for t in range(e.sym, gb, e.sym)} <= tags, "every tail residue"
        assert {"tail_split", "tail_only_block"} <= tags
    else:  # the ragged bytes are the byte kernel's second launch (k-split, LDS tables) or lanes like any other
        if kern in ("ksplit", "lut"):
            assert "byte" in kernels and "remainder" in tags
    several = not e.one_tile_only
    one = e.m1 is not None or e.one_tile_only
    want = set()
    kinds = ("plain",) if kern == "ksplit" else ("dealt_unpadded", "dealt_padded") if kern == "lut" else ("plain", "dealt_unpadded", "dealt_padded")
    for how in kinds:
        want |= {f"{how}_several"} if several else set()
        want |= {f"{how}_one"} if one else set()
    assert want <= tags, sorted(want - tags)
    if "S" in e.families:
        s_tags = _tags(name, ("S",))[0]
        assert "laps" in s_tags
        if kern not in ("byte", "byte_serial", "sym"):
            assert "ragged_lap_with_tail" in s_tags


def test_capped_grids_have_ragged_last_laps():
    for name, e in gc.ENGINES.items():
        ragged = 0
        for c in gc.cases(name, "S"):
            cl = gc.classify(e, c)
            assert cl["nblk"] in {c.max_blocks - 1, c.max_blocks, c.max_blocks + 1, 2 * c.max_blocks + 1, 3 * c.max_blocks - 1}
            ragged += cl["nblk"] > cl["ncb"] and cl["nblk"] % cl["ncb"] != 0
        assert ragged >= 8 or "S" not in e.families, name


def test_block_edges_give_the_column_block_counts_of_the_issue():
    for name in ("vec", "valu16_g1", "rows_k10_pf-1"):
        e = gc.ENGINES[name]
        for m in (e.m, e.m1):
            ncbs = {gc.classify(e, c)["ncb"] for c in gc.cases(name, "B") if c.m == m}
            assert ncbs >= {1, 2, 7, 8, 9, 10, 17}, (name, m, sorted(ncbs))


WINDOW_ROUTES = {
    "vec": {"vec_v2", "byte"}, "valu_wide": {"ksplit", "byte"}, "byte": {"byte"}, "lut": {"lut", "byte"},
    "mfma_i8": {"i8", "byte"}, "mfma_v1": {"fp4_v1", "byte"}, "mfma_ar": {"fp4_ar", "byte"},
    "mfma_tm": {"fp4_tm", "byte"}, "batched_valu": {"vec_v2", "byte"}, "batched_fp4": {"fp4_ar", "byte"},
    "valu16_g1": {"vec16_g1", "sym"}, "valu16_g2": {"vec16_g2", "sym"}, "sym": {"sym"}, "mfma": {"mfma16", "sym"},
    "batched_valu16": {"vec16_g1", "sym"}, "batched_mfma": {"mfma16", "sym"},
}


def test_every_window_route():
    """col0 off the engine's grid falls to the byte or symbol kernel (FP4: odd col0; LDS tables and
    v_perm: col0 % 16; int8 and the GF(2^16) matrix cores: col0 % 4)."""
    for name, e in gc.ENGINES.items():
        if "W" not in e.families:
            continue
        routes = _tags(name, ("W",))[2]
        want = WINDOW_ROUTES.get(name, {"rows_lat", "byte"} if e.base.startswith("rows") else None)
        assert routes == want, (name, routes)
        ch = gc.chunk_of(e, e.k, e.m)
        starts = {0, 16, 16 * 256, 1, 2, 4, 15, 17} | ({ch + 2} if ch else set())
        assert {c.col0 for c in gc.cases(name, "W")} == {c0 for c0 in starts if e.w == 8 or c0 % 2 == 0}, name
        ends = {(c.col0 + c.n) - c.nrow for c in gc.cases(name, "W")}
        assert ends == ({0, -1, -16, -17} if e.w == 8 else {0, -16})
    for name in ("mfma_v1", "mfma_ar", "mfma_tm", "mfma_i8", "batched_fp4"):  # (col0 = 2, 4 or chunk + 2)
        assert "remainder_off_grid" in _tags(name, ("W",))[0], name


CHUNK_ENGINES = [n for n, e in gc.ENGINES.items() if "L" in e.families]


@pytest.mark.parametrize("name", CHUNK_ENGINES)
def test_chunk_classes(name):
    e = gc.ENGINES[name]
    tags = _tags(name, ("L",))[0]
    one_slot = dict(e.tune).get("fp4_free_cus", 0) > 0
    if one_slot:
        assert {"chunks_even", "chunks_odd"} <= tags
        assert "crosses_stripe" in tags if e.batch > 1 else "chunks_1" in tags
    elif "+forced" not in name:
        assert {"chunks_0", "chunks_1"} <= tags
    if e.kind == "mfma16":
        assert {"tail_valid_0", "tail_valid_2", "tail_valid_4"} <= tags
        # (at the default slots no block of the batched launch has two chunks: at most 9 chunks on 16
        # slots; the chunk run across a stripe boundary is batched_mfma+one_slot's, asserted above)
    else:
        assert "remainder" in tags


def test_one_slot_reaches_one_group_only():
    for name, e in gc.ENGINES.items():
        if dict(e.tune).get("fp4_free_cus", 0):
            for c in gc.cases(name, "L"):
                for l in gc.plan(e, c):
                    if isinstance(l, gc.Chunks):
                        assert l.groups == 1 and l.slots == 1, (name, str(c))


# ---- 3. the reference engine ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.ENGINES))
def test_reference_engine_passes_the_whole_sweep(name):
    for family in gc.ENGINES[name].families:
        assert gc.sweep(name, family, gc.numpy_engine()) == []


def test_oracle_is_the_fields_gemm():
    for w, k, m in ((8, 5, 3), (16, 4, 2)):
        coeff, data, want = gc.oracle(w, k, m, 64)
        F = ec.field(w)
        sym = data.view(ec.sym_dtype(w)) if w == 16 else data
        assert np.array_equal(gc.as_bytes(F.matmul(coeff, sym).astype(ec.sym_dtype(w))), want)


# ---- 4. broken engines ------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", sorted(gc.FAULTS))
def test_planted_fault_is_caught_by_its_family(fault):
    name, family = gc.FAULTS[fault]
    failures = gc.sweep(name, family, gc.numpy_engine(fault), stop_at_first=True)
    assert failures, f"{fault}: the {family} cases of {name} did not notice"
    assert name in failures[0] and f"{family}:" in failures[0]


# the place of the first differing byte. The padding block's and the phantom chunk's stores lie past
# the end of output row 0 and its guard: the first byte they spoil is in a later output row
FAULT_CLASS = {
    "tail_as_group": "guard", "tail_block_dropped": "inside the window", "padded_blocks_live": "output row 1",
    "ragged_lap_skipped": "inside the window", "remainder_at_col0": "inside the window",
    "even_run_last_dropped": "inside the window", "phantom_stored": "output row 4", "stripe_not_wrapped": "guard",
    "window_rounded_down": "outside the window", "copies_tile_gt0": "copy row",
}


@pytest.mark.parametrize("fault", sorted(gc.FAULTS))
def test_a_failure_names_the_place(fault):
    """The first differing byte is translated into a row kind, a row, a column and its place."""
    name, family = gc.FAULTS[fault]
    msg = gc.sweep(name, family, gc.numpy_engine(fault), stop_at_first=True)[0]
    assert " row " in msg and "column" in msg and "class [" in msg and FAULT_CLASS[fault] in msg, msg


def test_faults_cover_the_list():
    assert len(gc.FAULTS) == 10 and {f for _, f in gc.FAULTS.values()} == {"T", "B", "S", "W", "L"}

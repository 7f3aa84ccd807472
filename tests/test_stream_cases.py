"""The stream-case table (tests/stream_cases.py) held to its conditions, without a GPU.

* Completeness: every public callable of ``ReedSolomon`` and of what ``gpu_rscode_amd.ops`` exports
  that takes ``stream=`` is reached by at least one entry, so an entry point added later fails here
  until it has stream cases.
* Every entry whose op has a CPU form runs on CPU tensors against its oracle: a wrong expectation in
  the table shows here. Entries without one (the plan classes, the device solves) still get their
  oracle evaluated, so it cannot raise or disagree with itself on the GPU only.
* The cases the issue names are in the table, and docs/API.md lists the table's verdicts.
"""
import os
import re

import numpy as np
import pytest

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMED = [
    "decode_pure_copy", "decode_batch_no_native_erased", "syndrome_mask_p0", "syndrome_mask_batch_p0",
    "syndrome_mask_batch_zero_columns", "update_p0", "write_p0", "update_window", "write_window",
    "decode_device_invert", "decode_device_invert_gf65536", "pattern_decoder", "gf_invert", "fill_random_",
    "gen_matrix_device_cauchy", "gen_matrix_device_vandermonde", "solve_patterns",
    "gemm8_vec", "gemm8_byte", "gemm8_rows_k10_pf0", "gemm8_lut", "gemm8_mfma_i8", "gemm8_mfma_v1", "gemm8_mfma_ar",
    "gemm8_mfma_tm", "gemm16_valu16", "gemm16_mfma", "encode_batch", "encode_batch_mfma", "encode_batch_gf65536_mfma",
    "decode_batch_mfma",
]


def test_every_stream_entry_point_has_a_case():
    api, covered = sc.stream_api(), sc.covered_api()
    assert len(api) >= 40, sorted(api)  # (the walk itself found the entry points)
    assert not api - covered, f"no stream case for {sorted(api - covered)}: add entries to tests/stream_cases.py"
    covered -= {"ReedSolomon.heal", "ReedSolomon.heal_batch"}  # (no stream argument: they run on the current one)
    assert not covered - api, f"entries name entry points that take no stream: {sorted(covered - api)}"


def test_completeness_check_sees_a_deleted_entry(monkeypatch):
    entries = {k: v for k, v in sc.ENTRIES.items() if "ReedSolomon.decode_batch" not in v.api}
    assert len(entries) < len(sc.ENTRIES)
    monkeypatch.setattr(sc, "ENTRIES", entries)
    assert sc.stream_api() - sc.covered_api() == {"ReedSolomon.decode_batch"}


def test_named_cases_are_in_the_table():
    assert not [n for n in NAMED if n not in sc.ENTRIES]
    assert len(sc.singular4()) == 4
    for e in sc.ENTRIES.values():
        assert e.spellings and set(e.spellings) <= {"arg", "current"}
        if not e.capture or not e.nosync:
            assert e.why, e.name
        if e.capture:
            assert e.nosync, e.name  # (a call that syncs cannot be captured)
        if e.left_out:  # an entry that a GPU harness skips says why, and the API table does not call it covered
            assert e.why and set(e.left_out) <= {"capture", "first"}, e.name
    assert [n for n, e in sc.ENTRIES.items() if e.left_out] == ["syndrome_mask_batch"]
    row = next(r for r in sc.doc_rows() if r[0] == "syndrome_mask_batch")
    assert row[2:] == ("yes", "no")


@pytest.mark.parametrize("name", [n for n, e in sc.ENTRIES.items() if e.cpu])
def test_entry_on_cpu_tensors(name):
    sc.run_plain(sc.ENTRIES[name], "cpu", sc.REAL)
    if sc.ENTRIES[name].capture:  # the odd seed of a replay sequence too
        sc.run_plain(sc.ENTRIES[name], "cpu", sc.REPLAYS[0])


def test_seeds_make_distinct_inputs_and_results():
    """A call that read the stale inputs must be visible: for every CPU entry that writes into the
    arena, the stale and the real seed lead to different bytes."""
    for name, e in sc.ENTRIES.items():
        if not e.cpu or name.startswith(("syndrome", "scrub")):
            continue
        b = e.build("cpu")
        imgs = []
        for seed in (sc.STALE, sc.REAL):
            b.fill(seed)
            b.expect(seed)
            imgs.append(b.arena.image.copy())
        assert not np.array_equal(*imgs), name


def test_fill_random_oracle_is_the_published_splitmix64():
    # splitmix64's first outputs from state 0 (Vigna's reference implementation), as x = 0, gamma, ...
    assert sc._splitmix64(0) == 0xE220A8397B1DCDAF
    assert sc._splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    a = sc.fill_random_oracle(4099, 12345)
    assert a.shape == (4099,) and a.dtype == np.uint8 and len(set(a.tolist())) == 256


def test_mask_oracle_marks_the_block_of_a_wrong_byte():
    rs = sc._rs(10, 14)
    s = sc.consistent(rs, 1, sc.C, 1)[0]
    assert not sc.mask_oracle(rs.H, s).any()
    s[12, sc.C - 1] ^= 1  # parity chunk 2: syndrome row 2 alone, second block
    assert sc.mask_oracle(rs.H, s).tolist() == [0, 4]


def test_api_document_lists_the_table():
    text = open(os.path.join(ROOT, "docs", "API.md"), encoding="utf-8").read()
    rows = re.findall(r"^\| `([a-z0-9_]+)` \| (.+?) \| (yes|no) \| (yes|no) \|$", text, flags=re.M)
    got = [(n, api.replace("`", ""), s, c) for n, api, s, c in rows]
    assert got == sc.doc_rows(), "docs/API.md: regenerate the stream table with stream_cases.doc_table()"


"""Row arguments (``gpu_rscode_amd/ops/rows.py``) and the aliasing rule of the parity update
(``ops/update.py``): the rule against an all-pairs oracle, the row-length licence of a single stripe,
and which names the package's modules import from each other. CPU only."""
import ast
import pathlib

import numpy as np
import pytest
import torch

import gpu_rscode_amd
from gpu_rscode_amd.ops.rows import batch_part, stripe_part
from gpu_rscode_amd.ops.update import check_overlap, check_overlap_batch

LENGTHS = (0, 1, 15, 16, 17, 33)
FORMS = {"pair": (2, False), "delta": (0, False), "write": (2, True)}  # form -> (new rows, old rows written)


def brute_force(groups, first_written: bool) -> bool:
    """Is the layout refused? All pairs of (kind, start, length) spans, the four rules: a parity row
    overlaps nothing; new overlaps no old; old overlaps no old when the old rows are written."""
    spans = [(kind, a, a + n) for kind, rows in enumerate(groups) for a, n in rows if n > 0]
    for x, (ka, a0, a1) in enumerate(spans):
        for kb, b0, b1 in spans[x + 1:]:
            if a0 < b1 and b0 < a1:
                kinds = {ka, kb}
                if 0 in kinds or kinds == {1, 2} or (first_written and kinds == {1}):
                    return True
    return False


def refuses(fn, *args) -> bool:
    try:
        fn(*args)
    except ValueError as e:
        assert "overlap" in str(e)
        return True
    return False


def both_forms(buf: torch.Tensor, groups, first_written: bool) -> bool:
    """The verdict of the single-stripe wrapper and of the array form (each kind's rows as stripes of
    one row, with their lengths), which must agree."""
    base = buf.data_ptr()
    par, old, new = ([buf[a: a + n] for a, n in rows] for rows in groups)
    single = refuses(check_overlap, par, old, new if new else None, first_written)
    addr = [np.array([[base + a] for a, _ in rows], dtype=np.uint64).reshape(-1, 1) for rows in groups]
    lens = [np.array([[n] for _, n in rows], dtype=np.int64).reshape(-1, 1) for rows in groups]
    if not groups[2]:
        addr[2] = None
        del lens[2]
    assert refuses(check_overlap_batch, *addr, lens, first_written) == single
    return single


@pytest.mark.parametrize("form", list(FORMS))
def test_overlap_rule_against_all_pairs(form):
    """2,000 seeded layouts of 2 parity, 2 old and 2 new rows (none in the delta form) in one 512-byte
    buffer. The form's share of refusals lies in 10..90 %, so neither verdict is the only one seen."""
    nnew, first_written = FORMS[form]
    rng = np.random.default_rng(sorted(FORMS).index(form))
    buf = torch.zeros(512, dtype=torch.uint8)
    refused = 0
    for _ in range(2000):
        groups = []
        for count in (2, 2, nnew):
            lens = rng.choice(LENGTHS, size=count)
            groups.append([(int(rng.integers(0, 512 - n + 1)), int(n)) for n in lens])
        want = brute_force(groups, first_written)
        assert both_forms(buf, groups, first_written) == want, (form, groups)
        refused += want
    assert 200 <= refused <= 1800, refused


def test_overlap_containment_and_empty_rows():
    buf = torch.zeros(512, dtype=torch.uint8)
    # a parity row inside an old row that is not its neighbour in start order
    assert both_forms(buf, [[(8, 1)], [(0, 33), (4, 1)], []], False)
    assert both_forms(buf, [[(8, 1)], [(0, 33), (4, 1)], [(100, 33), (200, 1)]], False)
    assert not both_forms(buf, [[(40, 1)], [(0, 33), (4, 1)], []], False)  # (old may overlap old: only read)
    assert both_forms(buf, [[(40, 1)], [(0, 33), (4, 1)], [(100, 1), (200, 1)]], True)  # ... unless written
    # rows of no bytes overlap nothing, wherever they start
    assert not both_forms(buf, [[(7, 0), (7, 0)], [(7, 0), (0, 0)], [(7, 0), (3, 0)]], True)
    assert not both_forms(buf, [[(0, 33), (40, 0)], [(8, 0), (33, 16)], [(16, 0), (49, 17)]], True)
    # the equal-length batch call: one length for every row
    addr = np.array([[0], [64]], dtype=np.uint64) + np.uint64(buf.data_ptr())
    check_overlap_batch(addr, addr + np.uint64(16), addr + np.uint64(32), 16, True)
    assert refuses(check_overlap_batch, addr, addr + np.uint64(16), addr + np.uint64(32), 17, True)
    assert refuses(check_overlap_batch, addr, addr + np.uint64(16), addr + np.uint64(32), np.int64(17), True)
    check_overlap_batch(addr, addr + np.uint64(16), addr + np.uint64(16), 0)


def test_single_stripe_rows_may_differ_in_length():
    """The shortest row of a single stripe counts; a batch, even of one stripe, needs one length."""
    rows = [torch.zeros(c, dtype=torch.uint8) for c in (4100, 4101, 4117)]
    part = stripe_part(rows, "rows")
    assert (part.nstripes, part.nrows, part.ncols) == (1, 3, 4100)
    assert part.lens.tolist() == [[4100, 4101, 4117]] and all(a is b for a, b in zip(part.rows(0), rows))
    assert part.ptrs().tolist() == [[r.data_ptr() for r in rows]]
    with pytest.raises(ValueError, match="one length"):
        batch_part([rows], "rows")
    same = batch_part([[r[:4100] for r in rows]], "rows")
    assert (same.nstripes, same.nrows, same.ncols, same.lens) == (1, 3, 4100, 4100)


def test_no_module_imports_another_modules_private_names():
    root = pathlib.Path(gpu_rscode_amd.__file__).parent
    files = sorted(root.rglob("*.py"))
    assert len(files) > 10
    found = []
    for path in files:
        for node in ast.walk(ast.parse(path.read_text())):
            # names taken from a module of this package (`from . import _build` takes a module)
            if isinstance(node, ast.ImportFrom) and node.module and (
                    node.level > 0 or node.module.split(".")[0] == "gpu_rscode_amd"):
                found += [f"{path.relative_to(root)}: from {'.' * node.level}{node.module} import {a.name}"
                          for a in node.names if a.name.startswith("_")]
    assert not found, found

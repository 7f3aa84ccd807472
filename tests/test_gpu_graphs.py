"""Graph capture and replay of every capturable call (GPU): the cases of tests/stream_cases.py.

``stream_cases.captured``: a warm-up call builds and caches the plan; the call is captured once on
the side stream (``capture_error_mode="global"``, both spellings of the stream); the graph is
replayed three times, each time after the inputs and the in-place rows were overwritten with fresh
data of that replay's seed, and after each replay the whole arena and the returned tensors are
compared exactly with the oracle. One eager call on the same buffers runs between the second and
the third replay. This fails when the call does anything a capture refuses, when a kernel, memset or
copy stays outside the graph (stale bytes after a replay), or when something that depends on the
data was fixed on the host at capture time: the second replay is the odd one (a flipped byte for the
syndrome masks, a singular pattern for the device-built decode, which must leave status 1 and the
output rows untouched).

Calls that sync by design are not captured; ``Entry.why`` says why. No test captures a cache miss.

Not covered: ``syndrome_mask_batch`` (``Entry.left_out``, listed "no" in docs/API.md). Its captured
graph returned, from the second replay on, non-zero bytes in the first 16 of the 24 bytes of its
[3, 2] mask on clean stripes; the single-stripe form (8 bytes) replays right and is covered.

A plan that was built but never run waits, at its first launch, for the event recorded after its
descriptor upload; without a warm-up call that wait falls inside the captured region. This runtime
captures it (the wait on an event recorded outside the capture adds no node), and the replays must be
right: ``test_never_run_plan_is_captured_with_its_ready_wait``.
"""
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

CASES = [(name, sp) for name, e in sc.ENTRIES.items() if e.capture and "capture" not in e.left_out
         for sp in ("arg", "current")]


@pytest.mark.parametrize("name,spelling", CASES)
def test_captured_call_replays_on_fresh_data(name, spelling):
    sc.captured(sc.ENTRIES[name], spelling)


@pytest.mark.parametrize("name", ["encode_2d", "update"])
def test_harness_catches_a_call_left_out_of_the_graph(name):
    with pytest.raises(AssertionError, match="arena differ"):
        sc.captured(sc.ENTRIES[name], "arg", fault=True)


def test_uncapturable_entries_say_why():
    for e in sc.ENTRIES.values():
        assert e.capture or e.why, e.name


FRESH = [("gemm8_vec", "arg"), ("gemm8_vec", "current"), ("gemm8_mfma_v1", "arg"), ("gemm16_valu16", "arg"),
         ("gemm16_mfma", "current")]


@pytest.mark.parametrize("name,spelling", FRESH)
def test_never_run_plan_is_captured_with_its_ready_wait(name, spelling):
    """Entries whose plan is built beforehand, captured with no warm-up call: the plan's first launch,
    and with it the wait for its ready event, is the captured one."""
    sc.captured(sc.ENTRIES[name], spelling, fresh_plan=True)

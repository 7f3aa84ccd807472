"""Stream order of every asynchronous call (GPU): the cases of tests/stream_cases.py behind a gate.

The existing side-stream tests synchronise the side stream and then read results on the default
stream, which waits for both: work enqueued on the wrong stream passes them. Here the side stream is
first blocked by a gate: a long ``torch.cuda._sleep``, then the device copies that replace the stale
contents of the arena with the real inputs (and restore the rows an in-place call writes). The call
is made while the gate is pending, a snapshot of the whole arena and of the returned tensors is
enqueued behind it on the side stream, and the snapshot is compared exactly with the numpy oracle of
the real inputs. A launch, memset or copy that is not ordered on the side stream reads stale inputs
or is overwritten by the gate's copies.

Both spellings run: ``stream=side`` with the default stream current, and ``stream=None`` inside
``with torch.cuda.stream(side)``; each on a cached plan (one call before the gate) and as the first
call. For entries documented as free of host syncs an event recorded on the side stream right after
the cached call returns must still be pending: a call that had synchronised would have waited for the
gate. "No host sync" is a property of a call on a cached plan and is asserted there only: every first
call builds a plan, and the upload of its descriptor from pageable memory blocks the host. Every test
asserts from its own events that its gate lasted at least 50 ms.

The masks that torch zero-fills (p = 0 codecs): a block of the mask's size is filled with 0xFF on the
side stream and freed before the gate, so that a mask that reads zero there was zero-filled. This does
not show a zero-fill issued on the default stream when ``stream=side`` is passed (that block comes from
the default stream's pool and is filled at once): the degenerate paths of ``_scrub``, ``_correct`` and
``_reconstruct_checked`` still fill on the current stream, and no test here decides whether that matters.

The gate: ``stream_cases.gate_cycles`` times one ``_sleep`` per process and scales it to 100 ms.
Measured on the MI355X: 2,395,399 cycles per millisecond (20,000,000 cycles took 8.35 ms), so the gate
is about 287 million cycles. Known intermittent failure: once in about 1,500 gates the events of a gate
of these 287 million cycles were 18.0 ms apart (the first launch of the process on the third stream ran
beside it) and the test failed its own "the gate lasted ..." assertion; gates otherwise measure about
120 ms. Whether the sleep was short or the event times were wrong is not known: the assertion message
now also gives the host time from enqueuing the gate to the end of the side stream, which tells the
two apart. A failure with that message is the gate's, not the case's.

Three streams per process: the default, the side stream and one more for the planted fault.
"""
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

CASES = [(name, sp) for name, e in sc.ENTRIES.items() for sp in e.spellings]


@pytest.mark.parametrize("name,spelling", CASES)
def test_cached_call_is_ordered_on_its_stream(name, spelling):
    sc.gated(sc.ENTRIES[name], spelling)


@pytest.mark.parametrize("name,spelling", [c for c in CASES if "first" not in sc.ENTRIES[c[0]].left_out])
def test_first_call_is_ordered_on_its_stream(name, spelling):
    sc.gated(sc.ENTRIES[name], spelling, first=True)


# ---- the harness must catch planted faults ------------------------------------------------------------
@pytest.mark.parametrize("name", ["encode_2d", "update", "syndrome_mask", "decode_pure_copy"])
def test_harness_catches_a_call_on_another_stream(name):
    with pytest.raises(AssertionError, match="arena differ|result"):
        sc.gated(sc.ENTRIES[name], "arg", fault="stream")


def test_harness_catches_a_host_sync():
    with pytest.raises(AssertionError, match="host sync"):
        sc.gated(sc.ENTRIES["encode_2d"], "arg", fault="sync")


def test_gate_is_long_enough_and_streams_are_three():
    cycles = sc.gate_cycles()
    side, other = sc.streams()
    assert sc.streams() == (side, other)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        t0.record()
        torch.cuda._sleep(cycles)
        t1.record()
    t1.synchronize()
    assert t0.elapsed_time(t1) >= sc.GATE_MIN_MS

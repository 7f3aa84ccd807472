#!/usr/bin/env python3
"""Time the fused syndrome check against the checks the codec had before it.

One process, one device-resident stripe in ``alloc_rows`` buffers (default: the headline shape,
k=10, n=14, C = 107,374,183). After a warm-up of every call it alternates, round by round,

  * ``syndrome_mask``                  (n rows read, nothing stored on a clean stripe),
  * ``syndrome_mask`` with the parity rows multiplied by H's identity block (GFRS_TUNE=scrub_ident=0)
    and on the general kernel (GFRS_TUNE=scrub_rows=0): the A/B of the two kernel choices,
  * ``verify(data, parity)``           (k rows read and p written by the encode, 2 p read back),
  * ``encode``                         (k rows read, p written),

each timed with device events over ``--reps`` calls, and prints the median and the spread (min,
max) over the rounds. Then ``scrub`` on the clean stripe and on the stripe with one whole chunk
overwritten. Prints one JSON object (also written to ``--out``).

``--batch B`` measures the batched scrub of small objects instead: B stripes of ``--cols`` bytes per
chunk, natives and ``encode_batch``'s parity in two allocations. Round by round it alternates

  * (a) one ``syndrome_mask_batch`` call                      (one memset and one launch for B stripes),
  * (b) a loop of B ``syndrome_mask`` calls on the same stripes (the API there was before; plans
    cached and warm),
  * (c) ``encode_batch`` on the same natives                   (the same number of rows moved),

each timed with device events over a window of ``--reps`` calls (a call of (b) is the whole loop, and
its window holds ``--reps`` / 8 of them), and, for (a) and (b), by the host clock around the same
window ended by a synchronise: launch gaps are what the batched call removes. Then ``scrub_batch``
on the clean batch and with one chunk of one stripe overwritten.

``--correct`` measures error correction per byte column against the calls it stands next to, at the
same shape (with ``--batch B``: B stripes per call, the ``_batch`` forms). In interleaved rounds of
one call each, timed with device events around the call (its one sync included):

  * ``scrub`` and ``correct`` on the clean stripe (``correct`` launches what ``scrub`` launches there);
  * with one byte wrong in every 4 KiB of one chunk: ``scrub``, ``correct`` and ``heal`` (which
    rebuilds the whole chunk and scrubs twice);
  * with two whole chunks overwritten, the pair search on every column: ``correct`` next to
    ``reconstruct`` of those two chunks as erasures.

A call that repairs is handed a freshly damaged stripe every time; the damage is not timed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n", type=int, default=14)
    ap.add_argument("--matrix", default="vandermonde")
    ap.add_argument("--cols", type=int, default=107_374_183, help="bytes per chunk")
    ap.add_argument("--block-bytes", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=21, help="alternations of the timed calls")
    ap.add_argument("--reps", type=int, default=40, help="calls per timed window")
    ap.add_argument("--scrub-reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=0, help="B > 0: the batched scrub of B stripes of --cols bytes")
    ap.add_argument("--correct", action="store_true", help="time correct next to scrub, heal and reconstruct")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    return ap.parse_args(argv)


def spread(ms: list[float]) -> dict:
    return {"median_us": round(statistics.median(ms) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2),
            "max_us": round(max(ms) * 1e3, 2)}


def emit(res: dict, out: str | None) -> None:
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main_batch(args) -> int:
    import torch

    from gpu_rscode_amd import ReedSolomon
    from gpu_rscode_amd.models.rs import row_pitch
    from gpu_rscode_amd.ops import fill_random_

    k, n, C, bb, B = args.k, args.n, args.cols, args.block_bytes, args.batch
    p = n - k
    rs = ReedSolomon(k, n, matrix=args.matrix)
    pitch = row_pitch(C, "cuda")
    base = torch.empty(B * k * pitch, dtype=torch.uint8, device="cuda")
    fill_random_(base, seed=1)
    data = base.as_strided((B, k, C), (k * pitch, pitch, 1))
    parity = rs.encode_batch(data)
    stripes = [[data[b, j] for j in range(k)] + [parity[b, i] for i in range(p)] for b in range(B)]

    def loop():
        for rows in stripes:
            rs.syndrome_mask(rows, bb)

    calls = {
        "syndrome_mask_batch": (lambda: rs.syndrome_mask_batch(data, parity, bb), args.reps),
        "syndrome_mask_loop": (loop, max(1, args.reps // 8)),
        "encode_batch": (lambda: rs.encode_batch(data, parity), args.reps),
    }

    def window(fn, reps) -> tuple[float, float]:
        """(device-event ms, host-clock ms to the end of a synchronise) per call"""
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        s.record()
        for _ in range(reps):
            fn()
        t.record()
        torch.cuda.synchronize()
        return s.elapsed_time(t) / reps, (time.perf_counter() - w0) * 1e3 / reps

    # the batch is consistent, by both checks, and both give the same masks
    mask = rs.syndrome_mask_batch(data, parity, bb)
    assert tuple(mask.shape) == (B, -(-C // bb)) and not bool(mask.any().item())
    assert not any(bool(rs.syndrome_mask(rows, bb).any().item()) for rows in stripes)
    for fn, _ in calls.values():  # warm-up: code objects, every plan, the allocator's blocks
        window(fn, 2)
    dev = {name: [] for name in calls}
    wall = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, (fn, reps) in calls.items():
            d, w = window(fn, reps)
            dev[name].append(d)
            wall[name].append(w)
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "block_bytes": bb, "batch": B},
           "rounds": args.rounds, "reps": {name: reps for name, (_, reps) in calls.items()},
           "device": torch.cuda.get_device_name(0)}
    for name in calls:
        res[name] = spread(dev[name])
    for name in ("syndrome_mask_batch", "syndrome_mask_loop"):
        res[name + "_wall"] = spread(wall[name])
    med = {name: statistics.median(ms) for name, ms in dev.items()}
    res["loop_over_batch"] = round(med["syndrome_mask_loop"] / med["syndrome_mask_batch"], 2)
    res["loop_over_batch_wall"] = round(statistics.median(wall["syndrome_mask_loop"]) /
                                        statistics.median(wall["syndrome_mask_batch"]), 2)
    res["batch_median_below_loop_min"] = bool(med["syndrome_mask_batch"] < min(dev["syndrome_mask_loop"]))
    res["batch_over_encode_batch"] = round(med["syndrome_mask_batch"] / med["encode_batch"], 3)
    res["syndrome_mask_batch_TBps"] = round(B * n * C / (med["syndrome_mask_batch"] * 1e-3) / 1e12, 3)
    res["encode_batch_TBps"] = round(B * n * C / (med["encode_batch"] * 1e-3) / 1e12, 3)

    if p > 16:  # beyond the locate kernel: masks only
        res["scrub_batch"] = "not available for p > 16"
        emit(res, args.out)
        return 0
    # scrub_batch (both kernels and the one sync): clean, then one chunk of one stripe overwritten
    rep = rs.scrub_batch(data, parity, bb)
    assert rep.clean.all() and rep.dirty == []
    res["scrub_batch_clean"] = spread([window(lambda: rs.scrub_batch(data, parity, bb), 1)[0]
                                       for _ in range(args.scrub_reps)])
    vb, vj = B // 2, min(3, k - 1)
    saved = data[vb, vj].clone()
    fill_random_(data[vb, vj][: C // 16 * 16], seed=99)
    rep = rs.scrub_batch(data, parity, bb)
    assert rep.dirty == [vb] and rep.report[vb].suspects == [vj] and rep.unlocated[vb] == 0
    res["scrub_batch_one_bad_chunk"] = spread([window(lambda: rs.scrub_batch(data, parity, bb), 1)[0]
                                               for _ in range(args.scrub_reps)])
    res["scrub_batch_one_bad_chunk"]["bad_columns"] = int(rep.bad_columns[vb])
    healed = rs.heal_batch(data, parity, rep)
    assert healed.clean.all() and healed.unhealed == [] and torch.equal(data[vb, vj], saved)
    emit(res, args.out)
    return 0


def main_correct(args) -> int:
    import torch

    from gpu_rscode_amd import ReedSolomon
    from gpu_rscode_amd.models.rs import row_pitch
    from gpu_rscode_amd.ops import fill_random_

    k, n, C, bb, B = args.k, args.n, args.cols, args.block_bytes, max(1, args.batch)
    p = n - k
    batched = args.batch > 0
    rs = ReedSolomon(k, n, matrix=args.matrix)
    pitch = row_pitch(C, "cuda")
    base = torch.empty(B * n * pitch, dtype=torch.uint8, device="cuda")
    fill_random_(base, seed=1)
    stripes = base.as_strided((B, n, C), (n * pitch, pitch, 1))
    rs.encode_batch(stripes[:, :k], stripes[:, k:])
    arg = stripes if batched else stripes[0]
    scrub = (lambda: rs.scrub_batch(arg, block_bytes=bb)) if batched else (lambda: rs.scrub(arg, bb))
    correct = (lambda: rs.correct_batch(arg, block_bytes=bb)) if batched else (lambda: rs.correct(arg, block_bytes=bb))
    heal = (lambda: rs.heal_batch(arg)) if batched else (lambda: rs.heal(arg))
    va, vb = min(3, k - 1), n - 2  # a native and a parity chunk

    def reconstruct():
        return rs.reconstruct_batch(arg, [va, vb]) if batched else rs.reconstruct(arg, erased=[va, vb])

    def timed(fn) -> float:
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t)

    def rounds(calls: dict, count: int, before=None) -> dict:
        times = {name: [] for name in calls}
        for _ in range(count):
            for name, fn in calls.items():
                if before is not None:
                    before()
                times[name].append(timed(fn))
        return times

    def all_clean(rep) -> bool:
        return bool(rep.clean.all()) if batched else rep.clean

    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "block_bytes": bb, "batch": args.batch},
           "rounds": args.rounds, "damaged_rounds": args.scrub_reps, "device": torch.cuda.get_device_name(0)}
    assert all_clean(scrub()) and all_clean(correct())
    rounds({"scrub": scrub, "correct": correct}, 2)  # warm-up
    clean = rounds({"scrub": scrub, "correct": correct}, args.rounds)
    res["clean"] = {name: spread(ms) for name, ms in clean.items()}
    res["clean"]["correct_median_above_scrub_max"] = bool(statistics.median(clean["correct"]) > max(clean["scrub"]))

    good = stripes[:, [va, vb]].clone()

    def restore():
        stripes[:, va].copy_(good[:, 0])
        stripes[:, vb].copy_(good[:, 1])

    def scatter():  # one byte wrong in every 4 KiB of chunk va
        restore()
        stripes[:, va, ::4096] ^= 0x5A

    scatter()
    rep = correct()
    per_stripe = -(-C // 4096)
    assert int(rep.uncorrectable.sum() if batched else rep.uncorrectable) == 0
    assert int(rep.by_weight[..., 1].sum()) == B * per_stripe and all_clean(scrub())
    scatter()
    assert all_clean(heal()) and torch.equal(stripes[:, va], good[:, 0])
    times = rounds({"scrub": scrub, "correct": correct, "heal": heal}, args.scrub_reps, before=scatter)
    res["one_byte_per_4k_of_one_chunk"] = {name: spread(ms) for name, ms in times.items()}
    res["one_byte_per_4k_of_one_chunk"]["wrong_bytes"] = B * per_stripe

    def overwrite():  # two whole chunks replaced by random bytes
        for b in range(B):
            fill_random_(stripes[b, va][: C // 16 * 16], seed=98 + 2 * b)
            fill_random_(stripes[b, vb][: C // 16 * 16], seed=99 + 2 * b)

    if p >= 4:
        overwrite()
        rep = correct()
        res["two_chunks_overwritten"] = {"by_weight": [int(v) for v in rep.by_weight.reshape(-1, 3).sum(axis=0)],
                                         "uncorrectable": int(rep.uncorrectable.sum() if batched else rep.uncorrectable)}
        overwrite()
        reconstruct()
        assert torch.equal(stripes[:, [va, vb]], good)
        times = rounds({"correct": correct, "reconstruct": reconstruct}, args.scrub_reps, before=overwrite)
        res["two_chunks_overwritten"].update({name: spread(ms) for name, ms in times.items()})
    restore()
    assert all_clean(scrub())
    emit(res, args.out)
    return 0


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch

    from gpu_rscode_amd import ReedSolomon, alloc_rows, flat_rows
    from gpu_rscode_amd.ops import fill_random_

    if not torch.cuda.is_available():
        print("scrub_bench.py needs a GPU", file=sys.stderr)
        return 2
    if args.correct:
        return main_correct(args)
    if args.batch > 0:
        return main_batch(args)
    k, n, C, bb = args.k, args.n, args.cols, args.block_bytes
    p = n - k
    rs = ReedSolomon(k, n, matrix=args.matrix)
    data = alloc_rows(k, C, "cuda")
    parity = alloc_rows(p, C, "cuda")
    fill_random_(flat_rows(data), seed=1)
    rs.encode(data, parity)
    stripe = [data[i] for i in range(k)] + [parity[i] for i in range(p)]

    def window(fn, reps) -> float:
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / reps

    def tuned_mask(tune):
        def call():
            os.environ["GFRS_TUNE"] = tune
            try:
                return rs.syndrome_mask(stripe, bb)
            finally:
                del os.environ["GFRS_TUNE"]
        return call

    general_mask = tuned_mask("scrub_rows=0")
    base_tune = os.environ.pop("GFRS_TUNE", None)
    if base_tune:
        print(f"ignoring GFRS_TUNE={base_tune}", file=sys.stderr)
    calls = {
        "syndrome_mask": lambda: rs.syndrome_mask(stripe, bb),
        "syndrome_mask_multiplied_identity": tuned_mask("scrub_ident=0"),
        "syndrome_mask_general": general_mask,
        "verify": lambda: rs.verify(data, parity),
        "encode": lambda: rs.encode(data, parity),
    }
    # the stripe is consistent, by both checks
    assert not bool(rs.syndrome_mask(stripe, bb).any().item()) and not bool(general_mask().any().item())
    assert rs.verify(data, parity)
    for fn in calls.values():  # warm-up: code objects, plans, the allocator's blocks
        window(fn, 3)
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, args.reps))
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "block_bytes": bb},
           "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name, ms in times.items():
        res[name] = spread(ms)
    med = {name: statistics.median(ms) for name, ms in times.items()}
    res["verify_over_syndrome_mask"] = round(med["verify"] / med["syndrome_mask"], 3)
    res["bytes_predict_verify_over_syndrome_mask"] = round((k + 3 * p) / n, 3)
    res["syndrome_mask_over_encode"] = round(med["syndrome_mask"] / med["encode"], 3)
    res["syndrome_mask_TBps"] = round(n * C / (med["syndrome_mask"] * 1e-3) / 1e12, 3)
    res["encode_TBps"] = round(n * C / (med["encode"] * 1e-3) / 1e12, 3)

    # scrub (both kernels and the one sync): clean, then chunk 3 overwritten
    rep = rs.scrub(stripe, bb)
    assert rep.clean
    res["scrub_clean"] = spread([window(lambda: rs.scrub(stripe, bb), 1) for _ in range(args.scrub_reps)])
    victim = min(3, n - 1)
    fill_random_(stripe[victim][: C // 16 * 16], seed=99)
    rep = rs.scrub(stripe, bb)
    assert rep.suspects == [victim] and rep.unlocated == 0, (rep.suspects, rep.unlocated)
    res["scrub_one_bad_chunk"] = spread([window(lambda: rs.scrub(stripe, bb), 1) for _ in range(args.scrub_reps)])
    res["scrub_one_bad_chunk"]["bad_columns"] = rep.bad_columns
    healed = rs.heal(stripe, rep)
    assert healed.clean and rs.verify(data, parity)
    emit(res, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Time the checked repair against the calls it replaces, on the same buffers.

One process. Per shape a device-resident (k, n) stripe of ``cols``-byte chunks, encoded, with the
first ``e`` natives lost. After one untimed call of each (checked against the clean stripe) and a
warm-up, it alternates round by round

  * ``checked``              ``reconstruct_checked``: n - e rows read, e written, the counts synced,
  * ``reconstruct``          the blind rebuild (k rows read, e written),
  * ``syndrome_mask``        the check of the whole stripe (n rows read),
  * ``reconstruct_correct``  ``reconstruct`` then ``correct(max_errors=2)`` (e = 1 only: with more
                             rebuilt chunks a wrong survivor byte is beyond ``correct``),

each window timed by device events and by the host clock around a synchronise. ``survivors: clean``
leaves the survivors as encoded; ``survivors: corrupt`` puts one wrong byte into every 4 KiB of one
survivor before every call, outside the timed window. The batched shape runs
``reconstruct_checked_batch`` against ``reconstruct_batch`` + ``syndrome_mask_batch``. Prints one
JSON object per shape and a last line ``{"device", "results": [...]}``; ``gate`` is whether, on clean
survivors, ``checked`` took less than ``reconstruct`` plus ``syndrome_mask`` (medians of the same
run). ``--device cpu`` runs small shapes on CPU tensors (host clock only).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BIG = 107_374_183  # the flagship chunk: 1 GiB / 10 natives, rounded up


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--code", default="10:14", help="k:n")
    ap.add_argument("--matrix", default="cauchy")
    ap.add_argument("--cols", type=int, default=None, help="bytes per chunk of the single-stripe shapes")
    ap.add_argument("--stripes", type=int, default=None, help="stripes of the batched shape")
    ap.add_argument("--batch-cols", type=int, default=None, help="bytes per chunk of the batched shape")
    ap.add_argument("--rounds", type=int, default=None, help="alternations of the timed calls")
    ap.add_argument("--reps", type=int, default=None, help="calls per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines here")
    args = ap.parse_args(argv)
    small = args.device == "cpu"
    for name, big, little in (("cols", BIG, 20011), ("stripes", 256, 4), ("batch_cols", 65536, 4099),
                              ("rounds", 9, 2), ("reps", 5, 1)):
        if getattr(args, name) is None:
            setattr(args, name, little if small else big)
    return args


def ms(values: list[float]) -> float:
    return round(statistics.median(values), 4)


class Timer:
    def __init__(self, torch, device: str, reps: int):
        self.torch, self.cuda, self.reps = torch, device == "cuda", reps

    def window(self, fn, before=None, reps=None) -> tuple[float, float]:
        """(device-event ms, host-clock ms) per call; ``before`` runs ahead of every call, untimed."""
        torch, reps = self.torch, reps or self.reps
        ev = host = 0.0
        for _ in range(reps if before else 1):
            if before:
                before()
            if self.cuda:
                s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            if self.cuda:
                s.record()
            for _ in range(1 if before else reps):
                fn()
            if self.cuda:
                t.record()
                torch.cuda.synchronize()
            host += (time.perf_counter() - t0) * 1e3
            ev += s.elapsed_time(t) if self.cuda else 0.0
        return ev / reps, host / reps

    def rounds(self, calls: dict, rounds: int, before=None) -> dict:
        for fn in calls.values():  # warm-up: code objects, plans, the allocator's blocks
            self.window(fn, before, 2)
        times = {name: ([], []) for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                ev, host = self.window(fn, before)
                times[name][0].append(ev)
                times[name][1].append(host)
        return times


def summarise(times: dict, cuda: bool) -> dict:
    out = {}
    for name, (ev, host) in times.items():
        use = ev if cuda else host
        out[f"{name}_ms"] = ms(use)
        out[f"{name}_min_max_ms"] = [round(min(use), 4), round(max(use), 4)]
        out[f"{name}_host_ms"] = ms(host)
    return out


def bench_stripe(torch, rs, C: int, e: int, corrupt: bool, args) -> dict:
    from gpu_rscode_amd import alloc_rows

    k, n, dev = rs.k, rs.n, args.device
    stripe = alloc_rows(n, C, dev)
    gen = torch.Generator().manual_seed(e)
    step = 1 << 24
    for j in range(k):
        if dev == "cuda":
            from gpu_rscode_amd.ops import fill_random_

            fill_random_(stripe[j], seed=100 * e + j)
            continue
        for c0 in range(0, C, step):
            stripe[j, c0: c0 + step].copy_(torch.randint(0, 256, (min(step, C - c0),), dtype=torch.uint8, generator=gen))
    rs.encode(stripe[:k], stripe[k:])
    erased = list(range(e))
    victim = k - 1  # a survivor every rebuild reads
    good = stripe.clone()
    bad_row = good[victim].clone()
    bad_row[::4096] ^= 0x5A

    def before():
        stripe[victim].copy_(bad_row)

    # once, untimed: the checked repair gives back the clean stripe, with and without the damage
    for j in erased:
        stripe[j].fill_(0)
    assert rs.reconstruct_checked(stripe, erased).clean and torch.equal(stripe, good), "reconstruct_checked is wrong"
    nbad = (C + 4095) // 4096
    if n - k - e >= 2:
        before()
        rep = rs.reconstruct_checked(stripe, erased)
        assert (int(rep.by_weight[1]), rep.uncorrectable) == (nbad, 0) and torch.equal(stripe, good)

    def pair():
        rs.reconstruct(stripe, erased)
        rs.correct(stripe, max_errors=2)

    calls = {"checked": lambda: rs.reconstruct_checked(stripe, erased),
             "reconstruct": lambda: rs.reconstruct(stripe, erased),
             "syndrome_mask": lambda: rs.syndrome_mask(stripe)}
    if e == 1 and n - k >= 4:
        calls["reconstruct_correct"] = pair
    times = Timer(torch, dev, args.reps).rounds(calls, args.rounds, before if corrupt else None)
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "erasures": e,
                     "survivors": "corrupt" if corrupt else "clean"}, "rounds": args.rounds, "reps": args.reps}
    res.update(summarise(times, dev == "cuda"))
    res["reconstruct_plus_mask_ms"] = round(res["reconstruct_ms"] + res["syndrome_mask_ms"], 4)
    res["checked_over_reconstruct_plus_mask"] = round(res["checked_ms"] / res["reconstruct_plus_mask_ms"], 3)
    res["checked_TBps_over_n_rows"] = round(n * C / (res["checked_ms"] * 1e-3) / 1e12, 3)
    res["bytes_predict"] = round(n / (k + e + n), 3)
    if not corrupt:
        res["gate"] = res["checked_ms"] < res["reconstruct_plus_mask_ms"]
    if corrupt:
        before()
        rs.reconstruct_checked(stripe, erased)
    assert torch.equal(stripe, good), "the stripe is not the clean one after the timed calls"
    return res


def bench_batch(torch, rs, C: int, B: int, args) -> dict:
    k, n, dev = rs.k, rs.n, args.device
    pitch = (C + 255) // 256 * 256
    base = torch.randint(0, 256, (B * n * pitch,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    stripes = base.to(dev).as_strided((B, n, C), (n * pitch, pitch, 1))
    rs.encode_batch(stripes[:, :k], stripes[:, k:])
    good = stripes.clone()
    erased = [0]
    stripes[:, 0].fill_(0)
    rep = rs.reconstruct_checked_batch(stripes, erased)
    assert bool(rep.clean.all()) and torch.equal(stripes, good), "reconstruct_checked_batch is wrong"

    def pair():
        rs.reconstruct_batch(stripes, erased)
        rs.syndrome_mask_batch(stripes)

    calls = {"checked": lambda: rs.reconstruct_checked_batch(stripes, erased),
             "reconstruct": lambda: rs.reconstruct_batch(stripes, erased),
             "syndrome_mask": lambda: rs.syndrome_mask_batch(stripes),
             "reconstruct_then_mask": pair}
    times = Timer(torch, dev, args.reps).rounds(calls, args.rounds)
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "stripes": B, "erasures": 1,
                     "survivors": "clean"}, "rounds": args.rounds, "reps": args.reps}
    res.update(summarise(times, dev == "cuda"))
    res["reconstruct_plus_mask_ms"] = round(res["reconstruct_ms"] + res["syndrome_mask_ms"], 4)
    res["checked_over_reconstruct_plus_mask"] = round(res["checked_ms"] / res["reconstruct_plus_mask_ms"], 3)
    assert torch.equal(stripes, good)
    return res


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch

    from gpu_rscode_amd import ReedSolomon

    if args.device == "cuda" and not torch.cuda.is_available():
        print("checked_repair_bench.py --device cuda needs a GPU", file=sys.stderr)
        return 2
    base_tune = os.environ.pop("GFRS_TUNE", None)
    if base_tune:
        print(f"ignoring GFRS_TUNE={base_tune}", file=sys.stderr)
    k, n = (int(v) for v in args.code.split(":"))
    rs = ReedSolomon(k, n, matrix=args.matrix)
    results = []
    for corrupt in (False, True):
        for e in (1, 2):
            results.append(bench_stripe(torch, rs, args.cols, e, corrupt, args))
            print(json.dumps(results[-1]), flush=True)
            if args.device == "cuda":
                torch.cuda.empty_cache()
    results.append(bench_batch(torch, rs, args.batch_cols, args.stripes, args))
    print(json.dumps(results[-1]), flush=True)
    name = torch.cuda.get_device_name(0) if args.device == "cuda" else "cpu"
    last = json.dumps({"device": name, "results": results,
                       "gate": all(r["gate"] for r in results if "gate" in r)})
    print(last, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in results) + "\n" + last + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

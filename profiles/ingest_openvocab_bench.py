"""Open-vocabulary ingest: scan + hash + intern against scan + hash + probe.

The byte-stream shape of bench.py: every step is a device buffer of
`--batch` newline-terminated 8-byte tokens (default 4M, 36 MB) over a
known vocabulary of `--vocab` words (default 50k).  A step is

    pw_scan_positions -> spans -> pw_varlen_hash_se -> dictionary

where the dictionary is either the closed-world probe of the parent commit
(ops.DeviceHashTable.probe on a table built from the known vocabulary,
untouched by this work: "probe") or DeviceDictionary.intern_hashes
("intern").  Three measurements, each in a child process of its own under
a time limit, the next one started only if the last one ended well:

  new=0     probe and intern steps alternate on the same buffers, so the
            two are compared inside one run; the block is repeated to show
            the run-to-run spread of either
  new=0.01  intern only; 1 % of every step's tokens are words no earlier
  new=0.05  step held (half as many distinct new words as new tokens)

Reported per measurement: ms/step (host clock around a step that ends in a
device synchronise; median, min..max), the blocking device->host reads the
dictionary made per step (the scan's own read of its match count is common
to both paths and not counted), the new words interned, and the time of
the deferred sync_host() that brings the host pool up to date afterwards.
Codes are checked against the known layout before timing.

    python profiles/ingest_openvocab_bench.py [--batch N] [--vocab V]
        [--steps K] [--warmup W] [--repeats R]

Needs a GPU and reads nothing outside the repository.  Not part of the
test suite.  Prints one JSON line per measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WW = 8  # token width in bytes


def word_bytes(prefix: int, ids: np.ndarray) -> np.ndarray:
    """(len(ids), WW) uint8: a prefix letter and the id as 7 digits."""
    out = np.empty((len(ids), WW), dtype=np.uint8)
    out[:, 0] = prefix
    pw10 = 10 ** np.arange(WW - 2, -1, -1, dtype=np.int64)
    out[:, 1:] = (ids[:, None] // pw10) % 10 + ord("0")
    return out


class Stream:
    """Seeded wire buffers: known words `w…`, never-seen words `n…`."""

    def __init__(self, batch: int, vocab: int, new_frac: float, seed: int):
        self.batch, self.vocab, self.new_frac = batch, vocab, new_frac
        self.rng = np.random.default_rng(seed)
        self.vocab_bytes = word_bytes(ord("w"), np.arange(vocab, dtype=np.int64))
        self.next_new = 0

    def step(self):
        """(wire bytes, known-word code per row or -1 for a new word)."""
        codes = self.rng.integers(0, self.vocab, size=self.batch)
        msg = np.empty((self.batch, WW + 1), dtype=np.uint8)
        msg[:, :WW] = self.vocab_bytes[codes]
        msg[:, WW] = 10
        n_new = int(self.batch * self.new_frac)
        if n_new:
            rows = self.rng.choice(self.batch, size=n_new, replace=False)
            fresh = max(1, n_new // 2)
            ids = self.next_new + self.rng.integers(0, fresh, size=n_new)
            self.next_new += fresh
            msg[rows, :WW] = word_bytes(ord("n"), ids)
            codes[rows] = -1
        return msg.reshape(-1), codes


def child(args) -> None:
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ingest_openvocab_bench: no GPU; nothing is measured on the CPU")
    from pathway_amd import ops
    from pathway_amd.engine.column import StringPool
    from pathway_amd.internals.api import TAG_STR

    dev = torch.device("cuda:0")
    new_frac = args.child
    stream = Stream(args.batch, args.vocab, new_frac, args.seed)
    pool = StringPool()
    pool.codes([bytes(r).decode() for r in stream.vocab_bytes])
    d = pool.device_dictionary(dev)
    plo, phi = pool.hash_tensors(dev)
    closed = ops.DeviceHashTable(plo[: args.vocab], phi[: args.vocab])
    total = args.warmup + args.steps * args.repeats
    staged = torch.empty(args.batch * (WW + 1), dtype=torch.uint8, device=dev)

    def run(mode: str, buf):
        nl = ops.scan_positions_gpu(buf, 10)
        starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), nl[:-1] + 1])
        lo, hi = ops.varlen_hash_se_gpu(buf, starts, nl, TAG_STR)
        if mode == "probe":
            return closed.probe(lo, hi)[0]
        return d.intern_hashes(lo, hi, buf, starts, nl)

    modes = ["probe", "intern"] if new_frac == 0 else ["intern"]
    times = {m: [[] for _ in range(args.repeats)] for m in modes}
    syncs0 = None
    for s in range(total):
        wire, known = stream.step()
        staged.copy_(torch.from_numpy(wire))
        torch.cuda.synchronize()
        if s == args.warmup:
            syncs0 = d.blocking_syncs
        for m in modes if s % 2 == 0 else modes[::-1]:
            t0 = time.perf_counter()
            codes = run(m, staged)
            torch.cuda.synchronize()
            dt_ms = (time.perf_counter() - t0) * 1e3
            if s >= args.warmup:
                times[m][(s - args.warmup) // args.steps].append(dt_ms)
            elif s == 0:
                # results first: known words keep their codes, new words
                # (intern only) get codes past the known vocabulary
                k = torch.from_numpy(known).to(dev)
                is_known = k >= 0
                assert torch.equal(codes[is_known], k[is_known]), m
                if m == "intern":
                    assert bool((codes[~is_known] >= args.vocab).all())
    dict_syncs = d.blocking_syncs - syncs0
    t0 = time.perf_counter()
    size = len(pool)  # drains: the deferred host sync
    sync_s = time.perf_counter() - t0
    out = {
        "new_frac": new_frac,
        "batch": args.batch,
        "vocab": args.vocab,
        "steps_per_repeat": args.steps,
        "table_slots": {
            "probe": closed.nslots,
            "intern_front": d.front.nslots,
            "intern_open": d.table.nslots,
        },
        "dictionary_blocking_syncs_per_step": dict_syncs / (args.steps * args.repeats),
        "new_words": size - args.vocab,
        "deferred_sync_host_s": sync_s,
        "ms_per_step": {
            m: [
                {"median": statistics.median(r), "min": min(r), "max": max(r)}
                for r in reps
            ]
            for m, reps in times.items()
        },
    }
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--limit", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--child", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    for frac in (0.0, 0.01, 0.05):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(frac)]
        for name in ("batch", "vocab", "steps", "warmup", "repeats", "seed"):
            cmd += [f"--{name}", str(getattr(args, name))]
        # a fresh process per measurement; a fault, an abort or a time
        # limit ends the whole run, nothing more is started on the GPU
        rc = subprocess.run(cmd, timeout=args.limit).returncode
        if rc != 0:
            raise SystemExit(f"measurement new={frac} ended with status {rc}")


if __name__ == "__main__":
    main()

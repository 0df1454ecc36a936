"""Op-level timing of the ingest kernels at the benchmark's shapes.

    PYTHONPATH=. python profiles/ingest_kernels_bench.py

One JSON line per op: median and max-min (ms) of 30 calls, each timed from
the host with a device synchronize on both sides (so `scan_positions_gpu`
includes its host read, as in the benchmark's step).

    hash        varlen_hash_se_gpu, 4M tokens of 10 bytes plus newline
    probe_50k   DeviceHashTable.probe, 4M queries into 50k keys (2^17 slots)
    probe_1m    the same into 1M keys (2^21 slots, past every L2)
    scan        scan_positions_gpu over the 44 MB wire buffer

Only the public ops API is used, so the same file runs on an older tree.
"""

from __future__ import annotations

import json
import statistics
import time

import torch

from pathway_amd import ops
from pathway_amd.internals.api import TAG_STR

N = 4_000_000
WW = 10
CALLS = 30
WARMUP = 5


def timed(name: str, fn, **extra) -> None:
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({
        "op": name,
        "median_ms": round(statistics.median(ms), 4),
        "max_minus_min_ms": round(max(ms) - min(ms), 4),
        "min_ms": round(min(ms), 4),
        "calls": CALLS,
        **extra,
    }), flush=True)


def main() -> None:
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

    # wire buffer: 4M tokens of 10 lower-case letters, each ended by \n
    vocab = 50_000
    words = torch.randint(97, 123, (vocab, WW), dtype=torch.uint8, device=dev,
                          generator=g)
    pick = torch.randint(0, vocab, (N,), device=dev, generator=g)
    wire = torch.full((N, WW + 1), 10, dtype=torch.uint8, device=dev)
    wire[:, :WW] = words[pick]
    wire = wire.reshape(-1).contiguous()

    timed("scan", lambda: ops.scan_positions_gpu(wire, 10), bytes=wire.numel())

    nl = ops.scan_positions_gpu(wire, 10)
    assert nl.numel() == N
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                        nl[:-1] + 1])
    timed("hash", lambda: ops.varlen_hash_se_gpu(wire, starts, nl, TAG_STR),
          tokens=N)

    qlo, qhi = ops.varlen_hash_se_gpu(wire, starts, nl, TAG_STR)
    voff = torch.arange(vocab + 1, dtype=torch.int64, device=dev) * WW
    vlo, vhi = ops.varlen_hash_gpu(words.reshape(-1).contiguous(), voff, TAG_STR)
    ht = ops.DeviceHashTable(vlo, vhi)
    codes, found = ht.probe(qlo, qhi)
    assert bool(found.all()) and torch.equal(vlo[codes], qlo)
    timed("probe_50k", lambda: ht.probe(qlo, qhi), queries=N, keys=vocab,
          nslots=ht.nslots)

    big = 1_000_000
    blo = torch.randint(-(1 << 62), 1 << 62, (big,), device=dev, generator=g)
    bhi = torch.randint(-(1 << 62), 1 << 62, (big,), device=dev, generator=g)
    ht_big = ops.DeviceHashTable(blo, bhi)
    bq = torch.randint(0, big, (N,), device=dev, generator=g)
    bqlo, bqhi = blo[bq], bhi[bq]
    codes, found = ht_big.probe(bqlo, bqhi)
    assert bool(found.all()) and torch.equal(blo[codes], bqlo)
    timed("probe_1m", lambda: ht_big.probe(bqlo, bqhi), queries=N, keys=big,
          nslots=ht_big.nslots)


if __name__ == "__main__":
    main()

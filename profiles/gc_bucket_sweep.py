"""Op-level timings of ops.group_combine_gpu for profiles/wordcount_r07.md
and wordcount_r10.md: a sweep of bucket_bits x table_capacity x layout
(partition, or sort and gather) at the timed size of bench.py (4M
rows, 50k distinct keys, one sum), and the bad case, an all-distinct 4M-row
batch with the bucket path forced on (wasted pass, then the prefix path)
and off.  Medians of 20 calls after 3 warm-up calls, host sync included.

    PYTHONPATH=. python profiles/gc_bucket_sweep.py
"""

import json
import statistics
import time

import torch

from pathway_amd import ops

N, VOCAB, REPS = 4_000_000, 50_000, 20


def timed(keys, contribs, **kw):
    before = {k: ops.gc_path_counts[k] for k in ("prefix", "fallback", "bucket")}
    ts = []
    for i in range(REPS + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.group_combine_gpu(keys, contribs, **kw)
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    path = [k for k, v in before.items() if ops.gc_path_counts[k] != v]
    return round(statistics.median(ts), 4), "+".join(path)


def main():
    g = torch.Generator(device="cpu").manual_seed(1)
    table = torch.randint(-(1 << 63), (1 << 63) - 1, (VOCAB, 2), generator=g)
    keys = table[torch.randint(0, VOCAB, (N,), generator=g)].cuda()
    ones = [torch.ones(N, dtype=torch.int64, device="cuda")]
    ms, path = timed(keys, ones, bucket=False)
    print(json.dumps({"case": "50k distinct", "bucket": False, "ms": ms, "path": path}))
    for bits in (6, 8, 9, 10, 12):
        for cap in (512, 1024, 2048):
            # both layouts where the partition serves the bucket count
            for part in ((True, False) if bits <= ops.GC_PART_MAX_BITS else (False,)):
                ms, path = timed(keys, ones, bucket=True, bucket_bits=bits,
                                 table_capacity=cap, partition=part)
                print(json.dumps({"case": "50k distinct", "bucket_bits": bits,
                                  "table_capacity": cap,
                                  "layout": "partition" if part else "gather",
                                  "ms": ms, "path": path}))
    distinct = torch.randint(-(1 << 63), (1 << 63) - 1, (N, 2), generator=g).cuda()
    for on in (False, True):
        ms, path = timed(distinct, ones, bucket=on)
        print(json.dumps({"case": "all distinct", "bucket": on, "ms": ms, "path": path}))


if __name__ == "__main__":
    main()

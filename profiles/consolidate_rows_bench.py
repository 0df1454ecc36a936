"""Op-level times at the consolidation's size (profiles/wordcount_r08.md):
100k rows, all distinct, one sum.

  - ops.group_combine_gpu on the prefix path and on the bucket path
  - ops.consolidate_rows_gpu, with the prefix sort on 32, 24 and 16 bits

Median and minimum of 30 calls, the call's host read included.

  PYTHONPATH=. python profiles/consolidate_rows_bench.py
"""

import time

import torch

from pathway_amd import ops

N = 100_000


def med(f, reps=30):
    for _ in range(5):
        f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    g = torch.Generator().manual_seed(1)
    keys = torch.randint(
        -(2**63), 2**63 - 1, (N, 2), generator=g, dtype=torch.int64
    ).cuda()
    diffs = torch.ones(N, dtype=torch.int64, device="cuda")
    for name, kw in [("prefix", dict(bucket=False)), ("bucket", dict(bucket=True))]:
        c0 = ops.gc_path_counts["bucket"]
        m, lo = med(lambda: ops.group_combine_gpu(keys, [diffs], **kw))
        took = ops.gc_path_counts["bucket"] - c0
        print(
            f"group_combine_gpu {name}: median {m:.4f} ms, min {lo:.4f} ms, "
            f"bucket path taken {took} times"
        )
    desc = [(ops.RI_INT64_TAGGED, diffs, 2, None)]
    for pb in (32, 24, 16):
        m, lo = med(
            lambda: ops.consolidate_rows_gpu(
                keys, desc, diffs, prefix_bits=pb, gather_keys=True
            )
        )
        print(
            f"consolidate_rows_gpu prefix_bits={pb}: median {m:.4f} ms, "
            f"min {lo:.4f} ms"
        )


if __name__ == "__main__":
    main()

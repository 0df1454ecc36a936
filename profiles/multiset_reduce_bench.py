"""Step times of the multiset reducers (profiles/multiset_r09.md).

Drives a GroupReduceNode directly, through the node API alone, so the same
script runs on this tree and on a checkout of an earlier commit:

  - one step of --store rows (default 4M) over --groups groups (100k) whose
    sizes follow a Zipf law (p ~ 1/rank), so that a few dozen groups hold
    more than SEG_SELECT_LONG rows and the largest about 8 % of the store;
  - then pairs of timed steps: --delta (200k) new rows, and the withdrawal
    of the same rows (same row keys, same values: the store returns to its
    size and no weight goes negative);
  - one reduce each for min+max on an int column, argmax on a float column,
    latest on a string column (ordered by a column of the row) and
    count_distinct on a string column.

Every step is timed with a synchronise on both sides.  Reported per reduce:
median, min and max of the insert steps and of the withdrawal steps, and,
for one more insert step, the kernel launches (torch.profiler) and the
synchronising host reads (torch's sync-debug mode) of the whole step.

  PYTHONPATH=. python profiles/multiset_reduce_bench.py [--reps 10 --warmup 3]

With --ops it times the two kernels alone instead, on a store laid out the
same way (ranges of Zipf sizes, 60k of them queried in random order with the
largest among them): seg_select_gpu over its `long_rows` threshold, and
seg_distinct_gpu over its table capacity, on a column of 1000 distinct
values and on one whose values are all distinct.  Median and minimum of 30
calls, a synchronise on both sides.
"""

import argparse
import json
import time
import warnings

import torch

from pathway_amd.engine import nodes
from pathway_amd.engine.batch import DeltaBatch
from pathway_amd.engine.column import StringColumn, TensorColumn
from pathway_amd.internals import dtype as dt
from pathway_amd.internals import expression as ex

DEV = "cuda:0"


def ref(name):
    return ex.ColumnReference(None, name)


REDUCES = {
    "min+max": {"mn": ("min", [ref("v")], {}), "mx": ("max", [ref("v")], {})},
    "argmax": {"am": ("argmax", [ref("f"), ref("id")], {})},
    "latest(str)": {"la": ("latest", [ref("s"), ref("ts")], {})},
    "count_distinct(str)": {"cd": ("count_distinct", [ref("s")], {})},
}


class Source:
    def __init__(self, groups, seed=5):
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        p = 1.0 / torch.arange(1, groups + 1, dtype=torch.float64, device=DEV)
        self.cdf = torch.cumsum(p / p.sum(), 0)
        self.groups = groups
        self.words = StringColumn.from_strings([f"w{i}" for i in range(1000)], DEV)
        self.next_id = 0

    def batch(self, n, time_, sign=1, like=None):
        if like is not None:
            cols, keys = like
        else:
            u = torch.rand(n, generator=self.gen, device=DEV, dtype=torch.float64)
            grp = torch.searchsorted(self.cdf, u).clamp_(max=self.groups - 1)
            rid = torch.arange(self.next_id, self.next_id + n, device=DEV)
            self.next_id += n
            cols = {
                "g": TensorColumn(grp, dt.INT),
                "v": TensorColumn(
                    torch.randint(-(10**6), 10**6, (n,), generator=self.gen, device=DEV),
                    dt.INT,
                ),
                "f": TensorColumn(
                    torch.rand(n, generator=self.gen, device=DEV, dtype=torch.float64),
                    dt.FLOAT,
                ),
                "s": self.words.take(
                    torch.randint(0, 1000, (n,), generator=self.gen, device=DEV)
                ),
                "ts": TensorColumn(rid, dt.INT),
            }
            keys = torch.stack([rid, rid * 7 + 1], dim=1)
        diffs = torch.full((keys.shape[0],), sign, dtype=torch.int64, device=DEV)
        return DeltaBatch(keys, cols, diffs, time_), (cols, keys)


def timed(node, batch, t):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    node.step(t, [batch])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "n": len(ts)}


def run(name, calls, args):
    src = Source(args.groups)
    node = nodes.GroupReduceNode(None, {"g": ref("g")}, calls, DEV)
    t = 0
    b, _ = src.batch(args.store, t)
    fill_ms = timed(node, b, t)
    ins, ret = [], []
    for i in range(args.warmup + args.reps):
        t += 2
        b, like = src.batch(args.delta, t)
        a = timed(node, b, t)
        t += 2
        b, _ = src.batch(args.delta, t, sign=-1, like=like)
        r = timed(node, b, t)
        if i >= args.warmup:
            ins.append(a)
            ret.append(r)
    # one more insert step, counted and not timed
    t += 2
    b, _ = src.batch(args.delta, t)
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                node.step(t, [b])
                torch.cuda.synchronize()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    reads = sum("synchroniz" in str(w.message).lower() for w in caught)
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    launches = sum(1 for e in kernels if "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    store = node.multiset_store
    out = {
        "reduce": name,
        "store_rows": int(store.weights.shape[0]),
        "min_weight": int(store.weights.min()),
        "fill_ms": round(fill_ms, 3),
        "insert_ms": {k: round(v, 3) for k, v in stats(ins).items()},
        "withdraw_ms": {k: round(v, 3) for k, v in stats(ret).items()},
        "launches_per_step": launches,
        "sync_reads_per_step": reads,
    }
    counts = getattr(__import__("pathway_amd.ops", fromlist=["ops"]), "multiset_path_counts", None)
    if counts is not None:
        out["path_counts"] = dict(counts)
    print(json.dumps(out), flush=True)


def med(f, reps=30):
    for _ in range(5):
        f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4)


def op_sweep(args):
    from pathway_amd import ops

    gen = torch.Generator(device=DEV).manual_seed(11)
    p = 1.0 / torch.arange(1, args.groups + 1, dtype=torch.float64, device=DEV)
    sizes = (p / p.sum() * args.store).to(torch.int64)
    hi_all = torch.cumsum(sizes, 0)
    lo_all = hi_all - sizes
    m = int(hi_all[-1])
    pick = torch.randperm(args.groups, generator=gen, device=DEV)[:60_000]
    pick[0] = 0  # the largest group
    lo, hi = lo_all[pick].contiguous(), hi_all[pick].contiguous()
    w = torch.randint(0, 3, (m,), generator=gen, device=DEV)
    ki = torch.randint(-(10**6), 10**6, (m,), generator=gen, device=DEV)
    kf = torch.rand(m, generator=gen, device=DEV, dtype=torch.float64)
    codes = torch.randint(0, 1000, (m,), generator=gen, device=DEV)
    ident = torch.arange(m, device=DEV)
    print(json.dumps({"rows": m, "ranges": 60_000, "largest": int(sizes[0]),
                      "ranges_over_4096": int((sizes[pick] > 4096).sum())}))
    for long_rows in (256, 1024, 4096, 16384, 65536, 1 << 40):
        t = med(lambda: ops.seg_select_gpu(lo, hi, w, ki, ops.SEG_MAX, long_rows=long_rows))
        print(json.dumps({"op": "seg_select MAX int64", "long_rows": long_rows, "median_min_ms": t}))
    t = med(lambda: ops.seg_select_gpu(lo, hi, w, kf, ops.SEG_MAX))
    print(json.dumps({"op": "seg_select MAX float64", "median_min_ms": t}))
    t = med(lambda: ops.seg_select_gpu(lo, hi, w, None, ops.SEG_FIRST))
    print(json.dumps({"op": "seg_select FIRST", "median_min_ms": t}))
    for cap in (1024, 4096, 8192):
        for name, vals in (("1000 values", codes), ("all distinct", ident)):
            t = med(lambda: ops.seg_distinct_gpu(lo, hi, w, vals, table_capacity=cap))
            st = ops.seg_distinct_gpu(lo, hi, w, vals, table_capacity=cap)[2]
            print(json.dumps({"op": "seg_distinct", "values": name, "capacity": cap,
                              "median_min_ms": t, "given_up": int(st.sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=4_000_000)
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--delta", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="name of one reduce")
    ap.add_argument("--ops", action="store_true", help="time the kernels alone")
    args = ap.parse_args()
    if args.ops:
        return op_sweep(args)
    for name, calls in REDUCES.items():
        if args.only in (None, name):
            run(name, calls, args)


if __name__ == "__main__":
    main()

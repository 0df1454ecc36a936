"""Step time of a float `avg` group reduce (profiles/float_reduce_r12.md).

Drives a GroupReduceNode directly, through the node API alone, so the same
script runs on this tree and on a checkout of an earlier commit.  Per shape
(rows x groups: 4M x 50k, 4M x 1, 4M x 2M by default) one node reduces
`avg` over a float64 column of gauss(0,1) * 10^uniform(-8,8) values; after
--warmup steps, --reps steps of fresh rows over the same groups are timed
one by one, each with a synchronise on both sides and its batch made before
the clock starts.  Reported per shape: median, min and max of the step
times, the spread (max - min), and the largest deviation of the emitted
averages of the last step from a float64 mean of the rows so far, relative
to the mean of |x| (a sanity figure, not a bound).

  PYTHONPATH=. python profiles/float_reduce_bench.py [--reps 9 --warmup 3]

--chunk T sets ops.SEG_SUM_F64_CHUNK, where the tree has it, for choosing T.
"""

import argparse
import json
import time

import torch

from pathway_amd.engine import nodes
from pathway_amd.engine.batch import DeltaBatch
from pathway_amd.engine.column import TensorColumn
from pathway_amd.internals import dtype as dt
from pathway_amd.internals import expression as ex

DEV = "cuda:0"


def ref(name):
    return ex.ColumnReference(None, name)


class Source:
    def __init__(self, rows, groups, seed=5):
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.rows, self.groups, self.next_id = rows, groups, 0

    def batch(self, time_):
        n = self.rows
        grp = torch.randint(0, self.groups, (n,), generator=self.gen, device=DEV)
        x = torch.randn(n, generator=self.gen, device=DEV, dtype=torch.float64)
        e = torch.rand(n, generator=self.gen, device=DEV, dtype=torch.float64)
        x = x * torch.pow(10.0, e * 16 - 8)
        rid = torch.arange(self.next_id, self.next_id + n, device=DEV)
        self.next_id += n
        cols = {"g": TensorColumn(grp, dt.INT), "x": TensorColumn(x, dt.FLOAT)}
        keys = torch.stack([rid, rid * 7 + 1], dim=1)
        diffs = torch.ones(n, dtype=torch.int64, device=DEV)
        return DeltaBatch(keys, cols, diffs, time_)


def run(rows, groups, args):
    src = Source(rows, groups)
    node = nodes.GroupReduceNode(
        None, {"g": ref("g")}, {"a": ("avg", [ref("x")], {})}, DEV
    )
    sums = torch.zeros(groups, dtype=torch.float64, device=DEV)
    cnts = torch.zeros(groups, dtype=torch.float64, device=DEV)
    mags = torch.zeros((), dtype=torch.float64, device=DEV)
    ts, out = [], None
    for i in range(args.warmup + args.reps):
        b = src.batch(2 * i)
        g, x = b.columns["g"].tensor, b.columns["x"].tensor
        sums.index_add_(0, g, x)
        cnts.index_add_(0, g, torch.ones_like(x))
        mags += x.abs().sum()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = node.step(2 * i, [b])
        torch.cuda.synchronize()
        if i >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    new = (out.diffs > 0).nonzero(as_tuple=True)[0]
    g = out.columns["g"].tensor.index_select(0, new)
    a = out.columns["a"].tensor.index_select(0, new)
    want = sums.index_select(0, g) / cnts.index_select(0, g)
    scale = mags / cnts.sum()
    dev = float(((a - want).abs().max() / scale).item())
    ts.sort()
    res = {
        "rows": rows,
        "groups": groups,
        "groups_emitted": int(new.shape[0]),
        "step_ms": {
            "median": round(ts[len(ts) // 2], 3),
            "min": round(ts[0], 3),
            "max": round(ts[-1], 3),
            "spread": round(ts[-1] - ts[0], 3),
            "n": len(ts),
        },
        "max_dev_vs_float64_mean": dev,
    }
    from pathway_amd import ops

    if hasattr(ops, "f64_combine_counts"):
        res["f64_combine_counts"] = dict(ops.f64_combine_counts)
        res["chunk"] = ops.SEG_SUM_F64_CHUNK
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--groups", type=int, nargs="*", default=[50_000, 1, 2_000_000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=None)
    args = ap.parse_args()
    if args.chunk is not None:
        from pathway_amd import ops

        if hasattr(ops, "SEG_SUM_F64_CHUNK"):
            ops.SEG_SUM_F64_CHUNK = args.chunk
    for groups in args.groups:
        run(args.rows, groups, args)


if __name__ == "__main__":
    main()

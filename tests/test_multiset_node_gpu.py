"""GPU tests of the multiset reducers' device path at node level: a
GroupReduceNode is driven through the same steps with the path on
(pw_seg_select / pw_seg_distinct) and with _PW_NO_MULTISET_DEVICE forcing
the torch chain and the per-group host loop, and must emit the same batches
step for step.  Retractions withdraw rows an earlier step inserted (same row
key, same values), so store weights cancel and never go negative.  Values
are compared, not column classes: the host path infers its classes from the
values."""

import pytest
import torch

gpu = pytest.mark.gpu
requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


def _ref(name):
    from pathway_amd.internals import expression as ex

    return ex.ColumnReference(None, name)


def _all_reducers():
    return {
        "min_v": ("min", [_ref("v")], {}),
        "max_v": ("max", [_ref("v")], {}),
        "min_f": ("min", [_ref("f")], {}),
        "max_f": ("max", [_ref("f")], {}),
        "argmin_v": ("argmin", [_ref("v"), _ref("id")], {}),
        "argmax_f": ("argmax", [_ref("f"), _ref("id")], {}),
        # ordered by a column of the row, which a retraction repeats
        "earliest_s": ("earliest", [_ref("s"), _ref("ts")], {}),
        "latest_s": ("latest", [_ref("s"), _ref("tf")], {}),
        "latest_f": ("latest", [_ref("f"), _ref("ts")], {}),
        "any_s": ("any", [_ref("s")], {}),
        "any_v": ("any", [_ref("v")], {}),
        "nd_s": ("count_distinct", [_ref("s")], {}),
        "nd_v": ("count_distinct_approximate", [_ref("v")], {}),
        "uniq_w": ("unique", [_ref("w")], {}),
    }


def _drive(reducer_calls, steps=6, rows=3000, ngroups=300):
    """`steps` steps of `rows` rows over `ngroups` groups.  Step 0 inserts;
    every later step retracts rows/2 live rows and inserts rows/2 new ones.
    The last group gets five rows in step 0 that step 1 withdraws.  Returns
    (emitted batches, retracted input rows, least store weight seen)."""
    from pathway_amd.engine import nodes
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import StringColumn, TensorColumn
    from pathway_amd.internals import dtype as dt

    words = StringColumn.from_strings([f"ms_word_{i}" for i in range(40)], DEV)
    gnames = StringColumn.from_strings([f"ms_group_{i}" for i in range(ngroups)], DEV)
    node = nodes.GroupReduceNode(None, {"g": _ref("g")}, reducer_calls, DEV)
    gen = torch.Generator().manual_seed(77)
    live = torch.zeros((0, 4), dtype=torch.int64)  # row id, g, v, word
    live_f = torch.zeros((0,), dtype=torch.float64)
    next_id, retracted, least_w, out = 0, 0, None, []
    for step in range(steps):
        n_ins = rows if step == 0 else rows // 2
        ids = torch.arange(next_id, next_id + n_ins)
        next_id += n_ins
        grp = torch.randint(0, ngroups - 1, (n_ins,), generator=gen)
        if step == 0:
            grp[:5] = ngroups - 1
        ins = torch.stack(
            [
                ids,
                grp,
                torch.randint(-50, 50, (n_ins,), generator=gen),
                torch.randint(0, 40, (n_ins,), generator=gen),
            ],
            dim=1,
        )
        # quarter steps: ties, for argmax and latest
        ins_f = torch.randint(-40, 40, (n_ins,), generator=gen).to(torch.float64) / 4
        if step == 0:
            part, part_f = ins, ins_f
            diffs = torch.ones(n_ins, dtype=torch.int64)
        else:
            pick = torch.randperm(live.shape[0], generator=gen)[: rows // 2]
            if step == 1:
                gone = (live[:, 1] == ngroups - 1).nonzero(as_tuple=True)[0]
                pick = torch.cat([gone, pick[~torch.isin(pick, gone)]])[: rows // 2]
            keep = torch.ones(live.shape[0], dtype=torch.bool)
            keep[pick] = False
            part = torch.cat([live[pick], ins])
            part_f = torch.cat([live_f[pick], ins_f])
            diffs = torch.cat(
                [-torch.ones(pick.shape[0], dtype=torch.int64), torch.ones(n_ins, dtype=torch.int64)]
            )
            retracted += int(pick.shape[0])
            live, live_f = live[keep], live_f[keep]
        live, live_f = torch.cat([live, ins]), torch.cat([live_f, ins_f])
        order = torch.randperm(part.shape[0], generator=gen)
        part, part_f, diffs = part[order].to(DEV), part_f[order].to(DEV), diffs[order].to(DEV)
        rid = part[:, 0].contiguous()
        batch = DeltaBatch(
            torch.stack([rid, rid * 7 + 1], dim=1),
            {
                "g": TensorColumn(part[:, 1].contiguous(), dt.INT),
                "w": gnames.take(part[:, 1].contiguous()),
                "v": TensorColumn(part[:, 2].contiguous(), dt.INT),
                "f": TensorColumn(part_f, dt.FLOAT),
                "s": words.take(part[:, 3].contiguous()),
                "ts": TensorColumn(rid, dt.INT),
                "tf": TensorColumn(rid.to(torch.float64) * 0.5, dt.FLOAT),
            },
            diffs,
            2 * step,
        )
        out.append(node.step(2 * step, [batch]))
        w_min = int(node.multiset_store.weights.min())
        least_w = w_min if least_w is None else min(least_w, w_min)
    return out, retracted, least_w


def _compare(new, old):
    assert len(new) == len(old)
    for step, (bn, bo) in enumerate(zip(new, old)):
        assert (bn is None) == (bo is None), step
        if bn is None:
            continue
        assert torch.equal(bn.keys, bo.keys), step
        assert torch.equal(bn.diffs, bo.diffs), step
        assert list(bn.columns) == list(bo.columns), step
        for name in bn.columns:
            assert bn.columns[name].to_pylist() == bo.columns[name].to_pylist(), (
                step,
                name,
            )


@gpu
@requires_cuda
def test_node_every_reducer_matches_host_path(monkeypatch):
    from pathway_amd import ops
    from pathway_amd.engine import nodes

    counts = ops.multiset_path_counts
    reducers = _all_reducers()
    monkeypatch.setattr(nodes, "_PW_NO_MULTISET_DEVICE", False)
    c0 = dict(counts)
    new, retracted, least_w = _drive(reducers)
    c1 = dict(counts)
    # 6 steps, old and new rows, but no old rows before the first merge
    assert c1["select"] - c0["select"] == 11 * 11
    assert c1["distinct"] - c0["distinct"] == 11 * 3
    assert c1["host"] == c0["host"] and c1["torch"] == c0["torch"]

    monkeypatch.setattr(nodes, "_PW_NO_MULTISET_DEVICE", True)
    old, _, _ = _drive(reducers)
    c2 = dict(counts)
    assert c2["select"] == c1["select"] and c2["distinct"] == c1["distinct"]
    assert c2["torch"] - c1["torch"] == 11 * 4
    assert c2["host"] - c1["host"] == 11 * 10

    _compare(new, old)
    assert all(b is not None for b in new)
    # the run holds retractions that cancel, and a group that disappears
    assert retracted == 5 * 1500 and least_w == 1
    assert any(bool((b.diffs < 0).any()) for b in new)
    assert "ms_group_299" in new[0].columns["uniq_w"].to_pylist()
    assert "ms_group_299" not in [
        v for v, d in zip(new[1].columns["uniq_w"].to_pylist(), new[1].diffs.tolist()) if d > 0
    ]


@gpu
@requires_cuda
def test_node_unique_broken_gives_error_as_on_host(monkeypatch):
    """`unique` over a column that is unique per group runs on the device;
    the step that breaks it for one group falls back as a whole and emits
    ERROR for that group, as the host path does."""
    from pathway_amd import ops
    from pathway_amd.engine import nodes
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import TensorColumn
    from pathway_amd.internals import dtype as dt
    from pathway_amd.internals.api import ERROR

    def run():
        node = nodes.GroupReduceNode(
            None, {"g": _ref("g")}, {"u": ("unique", [_ref("u")], {})}, DEV
        )
        out = []
        for step in range(3):
            g = torch.arange(10, dtype=torch.int64, device=DEV).repeat(3)
            u = g * 10
            if step == 2:
                g, u = g[:4].clone(), u[:4].clone()
                u[3] = 999
            rid = torch.arange(len(g), dtype=torch.int64, device=DEV) + 100 * step
            out.append(
                node.step(
                    2 * step,
                    [
                        DeltaBatch(
                            torch.stack([rid, rid + 5], dim=1),
                            {"g": TensorColumn(g, dt.INT), "u": TensorColumn(u, dt.INT)},
                            torch.ones_like(g),
                            2 * step,
                        )
                    ],
                )
            )
        return out

    counts = ops.multiset_path_counts
    monkeypatch.setattr(nodes, "_PW_NO_MULTISET_DEVICE", False)
    c0 = dict(counts)
    new = run()
    c1 = dict(counts)
    # new rows of step 0, both calls of step 1, old rows of step 2 ...
    assert c1["distinct"] - c0["distinct"] == 4
    assert c1["host"] - c0["host"] == 1  # ... and its new rows on the host
    monkeypatch.setattr(nodes, "_PW_NO_MULTISET_DEVICE", True)
    old = run()
    assert counts["distinct"] == c1["distinct"]
    _compare(new, old)
    assert new[1] is None  # same values again: nothing changes
    vals = new[2].columns["u"].to_pylist()
    assert vals == [30, ERROR] and new[2].diffs.tolist() == [-1, 1]

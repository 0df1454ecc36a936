"""GPU tests of float sum / avg in GroupReduceNode: double-double (hi, lo)
state per group, batches reduced by ops.group_combine_mixed_gpu, against
math.fsum over each group's live rows under the bound of tests/dd_cases.py.
N and sum|x| of the bound count every contribution a group has received
since it last came into being, retractions included."""

import math
import random
from fractions import Fraction

import pytest
import torch

from tests.dd_cases import avg_bound, check_sum

gpu = pytest.mark.gpu
requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"

EMPTIED = 299  # the group that step 1 empties and step 3 refills


def _ref(name):
    from pathway_amd.internals import expression as ex

    return ex.ColumnReference(None, name)


def _reducers():
    return {
        "fs": ("sum", [_ref("f")], {}),
        "fa": ("avg", [_ref("f")], {}),
        "va": ("avg", [_ref("v")], {}),
        "vs": ("sum", [_ref("v")], {}),
    }


def _node(device=None, reducers=None):
    from pathway_amd.engine import nodes

    return nodes.GroupReduceNode(
        None, {"g": _ref("g")}, reducers or _reducers(), device or DEV
    )


def _batch(rows, time, device=None, mask=None):
    """rows: (row id, group, v, f, diff)."""
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import TensorColumn
    from pathway_amd.internals import dtype as dt

    device = device or DEV
    i64 = lambda j: torch.tensor([r[j] for r in rows], dtype=torch.int64, device=device)  # noqa: E731
    rid = i64(0)
    f = torch.tensor([r[3] for r in rows], dtype=torch.float64, device=device)
    m = None if mask is None else torch.tensor(mask, dtype=torch.bool, device=device)
    return DeltaBatch(
        torch.stack([rid, rid * 7 + 1], dim=1),
        {
            "g": TensorColumn(i64(1), dt.INT),
            "v": TensorColumn(i64(2), dt.INT),
            "f": TensorColumn(f, dt.FLOAT, m),
        },
        i64(4),
        time,
    )


def _stream(steps=6, rows=3000, ngroups=300, seed=5):
    """Step 0 inserts `rows` rows; every later step retracts rows/2 live
    rows (same id, same values) and inserts rows/2 new ones.  Group EMPTIED
    has five rows from step 0, all withdrawn in step 1, gets nothing in
    step 2 and four new rows in step 3."""
    rng = random.Random(seed)
    live, next_id, out = {}, 0, []
    for step in range(steps):
        n_ins = rows if step == 0 else rows // 2
        ins = []
        for j in range(n_ins):
            g = rng.randrange(ngroups - 1)
            if (step == 0 and j < 5) or (step == 3 and j < 4):
                g = EMPTIED
            f = rng.gauss(0, 1) * 10 ** rng.uniform(-8, 8)
            if rng.random() < 0.02:
                f = rng.choice([1e16, -1e16, 1.0])
            ins.append((next_id, g, rng.randrange(-50, 50), f, 1))
            next_id += 1
        part = list(ins)
        if step > 0:
            ids = sorted(live)
            rng.shuffle(ids)
            gone = [i for i in ids if live[i][1] == EMPTIED] if step == 1 else []
            pick = (gone + [i for i in ids if i not in set(gone)])[: rows // 2]
            part += [live.pop(i)[:4] + (-1,) for i in pick]
        for r in ins:
            live[r[0]] = r
        rng.shuffle(part)
        out.append(part)
    return out


class Model:
    """Per group: live rows, and the count and magnitude of everything it
    has received since it came into being."""

    def __init__(self):
        self.live, self.n_adds, self.sum_abs = {}, {}, {}

    def apply(self, part):
        for rid, g, v, f, d in part:
            rows = self.live.setdefault(g, {})
            if d > 0:
                rows[rid] = (v, f)
            else:
                del rows[rid]
            self.n_adds[g] = self.n_adds.get(g, 0) + 1
            self.sum_abs[g] = self.sum_abs.get(g, 0.0) + abs(f)
        for g in [g for g, rows in self.live.items() if not rows]:
            del self.live[g], self.n_adds[g], self.sum_abs[g]

    def check(self, out, what):
        """Every row the step inserts into its output holds the group's
        values over its live rows."""
        assert out is not None
        cols = {n: c.to_pylist() for n, c in out.columns.items()}
        seen = set()
        for i, d in enumerate(out.diffs.tolist()):
            if d < 0:
                continue
            g = cols["g"][i]
            seen.add(g)
            rows = list(self.live[g].values())
            fs = [f for _v, f in rows]
            vs = [v for v, _f in rows]
            n, sa = self.n_adds[g], self.sum_abs[g]
            check_sum(cols["fs"][i], fs, n_adds=n, sum_abs=sa, what=(what, g, "sum"))
            exact = math.fsum(fs)
            err = abs(Fraction(cols["fa"][i]) - Fraction(exact) / len(fs))
            assert err <= avg_bound(exact, len(fs), n, sa), (what, g, "avg")
            assert cols["vs"][i] == sum(vs), (what, g)
            assert cols["va"][i] == sum(vs) / len(vs), (what, g)
        return seen


def _drive(node, stream, model=None, what=""):
    out = []
    for step, part in enumerate(stream):
        b = node.step(2 * step, [_batch(part, 2 * step, device=node.device)])
        out.append(b)
        if model is not None:
            model.apply(part)
            touched = {r[1] for r in part if r[1] in model.live}
            # random values: no touched group keeps its old output row
            assert touched <= model.check(b, (what, step))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert torch.equal(x.keys, y.keys) and torch.equal(x.diffs, y.diffs)
        assert list(x.columns) == list(y.columns)
        for name in x.columns:
            tx, ty = x.columns[name].tensor, y.columns[name].tensor
            assert torch.equal(tx, ty), name


@pytest.fixture(scope="module")
def stream():
    return _stream()


@gpu
@requires_cuda
def test_retracting_the_large_value_leaves_the_small_one():
    node = _node(reducers={"s": ("sum", [_ref("f")], {}), "a": ("avg", [_ref("f")], {})})
    first = node.step(0, [_batch([(1, 7, 0, 1e16, 1), (2, 7, 0, 1.0, 1)], 0)])
    assert first.columns["s"].to_pylist() == [1e16]
    out = node.step(2, [_batch([(1, 7, 0, 1e16, -1)], 2)])
    new = [i for i, d in enumerate(out.diffs.tolist()) if d > 0]
    assert len(new) == 1
    assert out.columns["s"].to_pylist()[new[0]] == 1.0
    assert out.columns["a"].to_pylist()[new[0]] == 1.0


@gpu
@requires_cuda
def test_insert_retract_stream_meets_the_bound(stream):
    from pathway_amd import ops

    before = dict(ops.f64_combine_counts)
    node = _node()
    model = Model()
    out = _drive(node, stream, model, "stream")
    assert ops.f64_combine_counts["native"] == before["native"] + len(stream)
    assert ops.f64_combine_counts["chain"] == before["chain"]
    assert set(node.add_accs) == {"__w__", "vs", "fs", "fs__c", "fa__sum", "fa__sum__c", "va__sum", "va__sum__c"}
    # the group emptied in step 1 left the output then, and came back in
    # step 3 with the sum of its four new rows alone
    g1 = out[1].columns["g"].to_pylist()
    assert [d for g, d in zip(g1, out[1].diffs.tolist()) if g == EMPTIED] == [-1]
    assert EMPTIED not in out[2].columns["g"].to_pylist()
    g3 = out[3].columns["g"].to_pylist()
    at = g3.index(EMPTIED)
    assert out[3].diffs.tolist()[at] == 1 and g3.count(EMPTIED) == 1
    fresh = [r[3] for r in stream[3] if r[1] == EMPTIED]
    assert len(fresh) == 4 and model.n_adds[EMPTIED] <= 4 + len(stream)
    check_sum(out[3].columns["fs"].to_pylist()[at], fresh, what="refilled")


@gpu
@requires_cuda
def test_same_stream_twice_emits_the_same_bits(stream):
    _same(_drive(_node(), stream), _drive(_node(), stream))


@gpu
@requires_cuda
def test_steps_of_one_and_two_rows():
    node, model = _node(), Model()
    parts = [
        [(1, 3, 4, 1e16, 1)],
        [(2, 3, -9, 1.0, 1), (3, 5, 2, -2.5e-7, 1)],
        [(1, 3, 4, 1e16, -1)],
        [(4, 5, 1, 3.25, 1), (3, 5, 2, -2.5e-7, -1)],
    ]
    out = _drive(node, parts, model, "small")
    last3 = out[2]
    new = [i for i, d in enumerate(last3.diffs.tolist()) if d > 0]
    assert [last3.columns["fs"].to_pylist()[i] for i in new] == [1.0]
    assert out[3].columns["fs"].to_pylist()[-1] == 3.25


@gpu
@requires_cuda
def test_masked_values_are_left_out():
    node = _node(reducers={"s": ("sum", [_ref("f")], {}), "a": ("avg", [_ref("f")], {})})
    rows = [(i, i % 3, 0, float(i) + 0.5, 1) for i in range(12)]
    mask = [i % 4 != 1 for i in range(12)]
    out = node.step(0, [_batch(rows, 0, mask=mask)])
    got = dict(zip(out.columns["g"].to_pylist(), out.columns["s"].to_pylist()))
    want = {}
    for (i, g, _v, f, _d), m in zip(rows, mask):
        want[g] = want.get(g, 0.0) + (f if m else 0.0)
    assert got == want


@gpu
@requires_cuda
def test_switch_off_keeps_one_float64(monkeypatch, stream):
    """With the switch on, the stream runs on one float64 per group.  The
    plain-float64 tolerance rel=1e-9 is taken relative to the larger of
    |exact| and the sum of |x| the group has received: the stream puts
    1e16 into groups and takes it out again, after which a single float64
    cannot be within 1e-9 of an exact sum of order 1e8."""
    from pathway_amd import ops
    from pathway_amd.engine import nodes

    monkeypatch.setattr(nodes, "_PW_NO_F64_COMBINE", True)
    before = dict(ops.f64_combine_counts)
    node = _node()
    model = Model()
    for step, part in enumerate(stream):
        out = node.step(2 * step, [_batch(part, 2 * step)])
        model.apply(part)
        cols = {n: c.to_pylist() for n, c in out.columns.items()}
        for i, d in enumerate(out.diffs.tolist()):
            if d < 0:
                continue
            rows = list(model.live[cols["g"][i]].values())
            exact = math.fsum(f for _v, f in rows)
            # plain float64: relative to the magnitudes that went in
            scale = max(model.sum_abs[cols["g"][i]], abs(exact))
            assert abs(cols["fs"][i] - exact) <= 1e-9 * scale
            assert abs(cols["fa"][i] - exact / len(rows)) <= 1e-9 * scale
            assert cols["vs"][i] == sum(v for v, _f in rows)
    assert not [n for n in node.add_accs if n.endswith("__c")]
    assert ops.f64_combine_counts == before


def _round_trip(node, device):
    from pathway_amd.persistence import operator_snapshot as snap

    state = snap.node_state_save(node)
    other = _node(device=device)
    snap.node_state_load(other, state, device)
    return state, other


@gpu
@requires_cuda
def test_snapshot_gpu_to_gpu_continues_identically(stream):
    node = _node()
    _drive(node, stream[:3])
    _state, other = _round_trip(node, DEV)
    assert set(other.add_accs) == set(node.add_accs)
    rest = [(s, part) for s, part in enumerate(stream) if s >= 3]
    a = [node.step(2 * s, [_batch(p, 2 * s)]) for s, p in rest]
    b = [other.step(2 * s, [_batch(p, 2 * s)]) for s, p in rest]
    _same(a, b)


@gpu
@requires_cuda
def test_snapshot_without_low_parts_restores(stream):
    """A state without `__c` entries is all the restored node knows: one
    float64 per group.  What it emits afterwards is held against the fsum
    of that float and the signed contributions since, which is the exact
    value of what the node was given."""
    from pathway_amd.persistence import operator_snapshot as snap

    node = _node()
    _drive(node, stream[:3])
    state = snap.node_state_save(node)
    for name in [n for n in state["add_accs"] if n.endswith("__c")]:
        del state["add_accs"][name]
    other = _node()
    snap.node_state_load(other, state, DEV)
    assert set(other.add_accs) == set(node.add_accs)
    assert not bool(other.add_accs["fs__c"].any())
    assert torch.equal(other.add_accs["fs"], node.add_accs["fs"])
    groups = other.add_carried["g"].to_pylist()
    given = {g: [x] for g, x in zip(groups, other.add_accs["fs"].tolist())}
    weight = dict(zip(groups, other.add_accs["__w__"].tolist()))
    for s in range(3, len(stream)):
        out = other.step(2 * s, [_batch(stream[s], 2 * s)])
        for _rid, g, _v, f, d in stream[s]:
            given.setdefault(g, []).append(d * f)
            weight[g] = weight.get(g, 0) + d
        for g in [g for g, w in weight.items() if w == 0]:
            del given[g], weight[g]
        cols = {n: c.to_pylist() for n, c in out.columns.items()}
        checked = 0
        for i, d in enumerate(out.diffs.tolist()):
            if d > 0:
                g = cols["g"][i]
                check_sum(cols["fs"][i], given[g], what=("stripped", s, g))
                checked += 1
        assert checked > 100


@gpu
@requires_cuda
def test_snapshot_gpu_state_into_cpu_node(stream):
    node = _node()
    _drive(node, stream[:3])
    want = {
        n: (node.add_accs[n] + node.add_accs[f"{n}__c"]).cpu()
        for n in ("fs", "fa__sum", "va__sum")
    }
    _state, other = _round_trip(node, "cpu")
    assert not [n for n in other.add_accs if n.endswith("__c")]
    for n, t in want.items():
        assert torch.equal(other.add_accs[n], t)
    # and it goes on as a CPU node does
    out = other.step(6, [_batch(stream[3], 6, device="cpu")])
    assert out is not None and not [n for n in other.add_accs if n.endswith("__c")]


@gpu
@requires_cuda
def test_more_than_eight_accumulators_take_the_chain(stream):
    """Nine contributions (the weight and eight float sums) are more than
    the combiner takes: the torch chain sums them, the state still holds
    (hi, lo) pairs, with plain float64 accuracy."""
    from pathway_amd import ops

    before = dict(ops.f64_combine_counts)
    node = _node(reducers={f"s{i}": ("sum", [_ref("f")], {}) for i in range(8)})
    model = Model()
    for step, part in enumerate(stream[:2]):
        out = node.step(2 * step, [_batch(part, 2 * step)])
        model.apply(part)
        groups = out.columns["g"].to_pylist()
        for name in ("s0", "s7"):
            vals = out.columns[name].to_pylist()
            for i, d in enumerate(out.diffs.tolist()):
                if d > 0:
                    exact = math.fsum(f for _v, f in model.live[groups[i]].values())
                    scale = max(model.sum_abs[groups[i]], abs(exact))
                    assert abs(vals[i] - exact) <= 1e-9 * scale
    assert ops.f64_combine_counts["chain"] == before["chain"] + 2
    assert ops.f64_combine_counts["native"] == before["native"]
    assert "s3__c" in node.add_accs

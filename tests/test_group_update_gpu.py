"""GPU tests of the group update (pw_group_update_*): one merge walk over
the unique-sorted reduce state and the unique-sorted consolidated delta
that writes both the merged state and the emitted old/new rows.  Every op
case is checked against a CPU model written here (a dict from key to
accumulators) and against the chain the walk replaces (lookup_gpu,
merge_consolidate_gpu, lookup_gpu again, the presence / unchanged masks).
The node cases run a GroupReduceNode with the path on and forced off.
All values are integers: every comparison is exact."""

import pytest
import torch

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


# ------------------------------------------------------------- op level --

def _tensors(rows, nacc):
    """{(w0, w1): [acc...]} -> (words, accs) sorted by key, on the device."""
    ks = sorted(rows)
    words = [
        torch.tensor([k[i] for k in ks], dtype=torch.int64, device=DEV)
        for i in range(2)
    ]
    accs = [
        torch.tensor([rows[k][c] for k in ks], dtype=torch.int64, device=DEV)
        for c in range(nacc)
    ]
    return words, accs


def _model(A, B, nacc, slots):
    """The rules of the step on dicts.  Returns what group_update_gpu
    returns, as python lists."""
    a_keys = sorted(A)
    row_of = {k: i for i, k in enumerate(a_keys)}
    m = len(a_keys)
    state = {k: (list(v), row_of[k]) for k, v in A.items()}
    rets, inss = [], []
    for j, k in enumerate(sorted(B)):
        matched = k in state
        old = list(state[k][0]) if matched else [0] * nacc
        new = [o + d for o, d in zip(old, B[k])]
        src = state[k][1] if matched else m + j
        old_p, new_p = old[0] > 0, new[0] > 0
        unchanged = old_p and new_p and all(old[c] == new[c] for c in slots)
        if old_p and not unchanged:
            rets.append((k, -1, old, src))
        if new_p and not unchanged:
            inss.append((k, 1, new, src))
        if new[0] != 0:
            state[k] = (new, src)
        elif matched:
            del state[k]
    s_keys = sorted(state)
    out = rets + inss
    return (
        [[k[i] for k in s_keys] for i in range(2)],
        [[state[k][0][c] for k in s_keys] for c in range(nacc)],
        [state[k][1] for k in s_keys],
        [list(r[0]) for r in out],
        [r[1] for r in out],
        [[r[2][c] for r in out] for c in sorted(set(slots))],
        [r[3] for r in out],
    )


def _chain(aw, aa, bw, ba, slots):
    """The chain the walk replaces, op for op."""
    from pathway_amd import ops

    m, n = aw[0].shape[0], bw[0].shape[0]

    def rows_of(words, accs):
        if words[0].shape[0] == 0:
            z = torch.zeros(n, dtype=torch.int64, device=DEV)
            return z, z.bool(), [z for _ in accs]
        pos, found = ops.lookup_gpu(words, bw)
        return pos, found, [a.index_select(0, pos) * found for a in accs]

    pos, found, old = rows_of(aw, aa)
    ow, oa, rep = ops.merge_consolidate_gpu(aw, aa, bw, ba)
    _pos2, _found2, new = rows_of(ow, oa)
    old_p, new_p = old[0] > 0, new[0] > 0
    unchanged = old_p & new_p
    for c in slots:
        unchanged = unchanged & (old[c] == new[c])
    ridx = (old_p & ~unchanged).nonzero(as_tuple=True)[0]
    iidx = (new_p & ~unchanged).nonzero(as_tuple=True)[0]
    changed = torch.stack(bw, dim=1)
    src = torch.where(found, pos, m + torch.arange(n, device=DEV))
    return (
        ow,
        oa,
        rep,
        torch.cat([changed.index_select(0, ridx), changed.index_select(0, iidx)]),
        torch.cat([torch.full_like(ridx, -1), torch.ones_like(iidx)]),
        [
            torch.cat([old[c].index_select(0, ridx), new[c].index_select(0, iidx)])
            for c in sorted(set(slots))
        ],
        torch.cat([src.index_select(0, ridx), src.index_select(0, iidx)]),
    )


def _check(A, B, nacc, slots):
    """Run the op on (A, B); compare with the model and the chain.
    Returns (state rows, retractions, insertions)."""
    from pathway_amd import ops

    aw, aa = _tensors(A, nacc)
    bw, ba = _tensors(B, nacc)
    got = ops.group_update_gpu(aw, aa, bw, ba, slots)
    ref = _chain(aw, aa, bw, ba, slots)
    torch.cuda.synchronize()
    model = _model(A, B, nacc, slots)
    names = ("words", "accs", "rep", "keys", "diffs", "vals", "src")
    for name, g, r, mo in zip(names, got, ref, model):
        if isinstance(g, list):
            assert len(g) == len(r) == len(mo), name
            for gi, ri, mi in zip(g, r, mo):
                assert gi.dtype == torch.int64 and gi.cpu().tolist() == mi, name
                assert torch.equal(gi, ri), name
        else:
            assert g.dtype == torch.int64, name
            if name == "keys":
                assert tuple(g.shape) == (len(mo), 2)
            assert g.cpu().tolist() == mo, name
            assert torch.equal(g, r.reshape(g.shape)), name
    diffs = got[4].cpu().tolist()
    assert diffs == sorted(diffs)  # retractions first
    return got[2].shape[0], diffs.count(-1), diffs.count(1)


def _rand_rows(g, count, nacc, keyspace, w1_only=False, zero_ok=False):
    rows = {}
    while len(rows) < count:
        v = int(torch.randint(-keyspace, keyspace, (1,), generator=g))
        k = (5, v) if w1_only else (v // 3, v % 3 - 1)
        acc = torch.randint(-3, 4, (nacc,), generator=g).tolist()
        if acc[0] == 0 and not zero_ok:
            acc[0] = 2  # a state row never has weight 0
        rows[k] = acc
    return rows


@gpu
@requires_cuda
@pytest.mark.parametrize(
    "A, B, slots, expect",
    [
        # first step (m = 0), n = 1
        ({}, {(1, 1): [2, 7]}, [0, 1], (1, 0, 1)),
        # m = 1, n = 1, matched; then unmatched on either side
        ({(1, 1): [2, 7]}, {(1, 1): [1, 1]}, [0, 1], (1, 1, 1)),
        ({(1, 1): [2, 7]}, {(0, 9): [1, 1]}, [0, 1], (2, 0, 1)),
        ({(1, 1): [2, 7]}, {(1, 2): [1, 1]}, [0, 1], (2, 0, 1)),
        # the weight goes to 0: the row leaves the state, retraction only
        ({(1, 1): [2, 7], (3, 0): [1, 1]}, {(1, 1): [-2, -7]}, [0, 1], (1, 1, 0)),
        # negative weight going positive: insertion only, carried from A
        ({(1, 1): [-1, 4]}, {(1, 1): [3, 1]}, [0, 1], (1, 0, 1)),
        # present going negative: retraction only, the row stays in the state
        ({(1, 1): [1, 4]}, {(1, 1): [-3, 0]}, [0, 1], (1, 1, 0)),
        # all-zero delta row, matched and unmatched: nothing happens
        ({(1, 1): [1, 4]}, {(1, 1): [0, 0], (2, 2): [0, 0]}, [0, 1], (1, 0, 0)),
        # the sum moves, the weight does not
        ({(1, 1): [1, 4]}, {(1, 1): [0, 5]}, [0, 1], (1, 1, 1)),
        # no count exposed and only the weight moves: no output
        ({(1, 1): [1, 4]}, {(1, 1): [2, 0]}, [1], (1, 0, 0)),
        # ... but the same delta with count exposed is a change
        ({(1, 1): [1, 4]}, {(1, 1): [2, 0]}, [0, 1], (1, 1, 1)),
        # no slot exposed: presence alone decides
        ({(1, 1): [1, 4]}, {(1, 1): [2, 3], (2, 0): [1, 0]}, [], (2, 0, 1)),
        # unmatched delta with weight <= 0: state row, no output
        ({}, {(1, 1): [-1, 3], (1, 2): [0, 3]}, [0, 1], (1, 0, 0)),
        # negative words, signed order, word1-only neighbours
        (
            {(-5, -1): [1, 1], (-5, 0): [1, 1], (-5, 1): [1, 1], (4, -9): [1, 1]},
            {(-5, 0): [1, 0], (-(1 << 62), 3): [1, 2], (4, -10): [1, 2]},
            [0, 1],
            (6, 1, 3),
        ),
    ],
)
def test_rules(A, B, slots, expect):
    nacc = len(next(iter(B.values())))
    assert _check(A, B, nacc, slots) == expect


@gpu
@requires_cuda
def test_matched_none_below_above():
    g = torch.Generator().manual_seed(11)
    A = _rand_rows(g, 40, 2, 200)
    ks = sorted(A)
    deltas = torch.randint(-3, 4, (40, 2), generator=g).tolist()
    all_matched = {k: d for k, d in zip(ks, deltas)}
    assert _check(A, all_matched, 2, [0, 1])[0] <= 40
    none_matched = {(k[0], k[1] + 10): d for k, d in zip(ks, deltas)}
    _check(A, none_matched, 2, [0, 1])
    below = {(k[0] - 1000, k[1]): d for k, d in zip(ks, deltas)}
    _check(A, below, 2, [0, 1])
    above = {(k[0] + 1000, k[1]): d for k, d in zip(ks, deltas)}
    _check(A, above, 2, [0, 1])


@gpu
@requires_cuda
@pytest.mark.parametrize("total", [7, 8, 9, 2047, 2048, 2049, 4100])
@pytest.mark.parametrize("nacc", [1, 2, 8])
def test_sizes(total, nacc):
    """m + n on both sides of the 8-row chunk and the 256-thread block."""
    g = torch.Generator().manual_seed(total * 10 + nacc)
    m = total // 2
    n = total - m
    A = _rand_rows(g, m, nacc, total)
    B = _rand_rows(g, n, nacc, total, zero_ok=True)
    slots = [c for c in range(nacc) if c % 3 != 2]
    kept, nret, nins = _check(A, B, nacc, slots)
    if total > 100:
        assert nret > 0 and nins > 0 and kept < total


@gpu
@requires_cuda
def test_dense_fully_matched():
    """m = n = 1030 on the same keys: every match straddles or touches a
    chunk boundary somewhere, so the skip rule fires in most threads."""
    g = torch.Generator().manual_seed(5)
    A = _rand_rows(g, 1030, 2, 1200)
    B = {
        k: torch.randint(-3, 4, (2,), generator=g).tolist() for k in A
    }
    _check(A, B, 2, [0, 1])


@gpu
@requires_cuda
def test_word1_only_differences():
    g = torch.Generator().manual_seed(6)
    A = _rand_rows(g, 300, 2, 400, w1_only=True)
    B = _rand_rows(g, 300, 2, 400, w1_only=True, zero_ok=True)
    kept, nret, nins = _check(A, B, 2, [1])
    assert nret > 0 and nins > 0


# ----------------------------------------------------------- node level --

def _column_parts(col):
    from pathway_amd.engine.column import PointerColumn, StringColumn, TensorColumn

    if isinstance(col, StringColumn):
        return {"class": "str", "dtype": col.dtype, "pool": col.pool, "t": col.codes}
    if isinstance(col, PointerColumn):
        return {"class": "ptr", "dtype": col.dtype, "t": col.pairs}
    assert isinstance(col, TensorColumn), type(col)
    return {"class": "tensor", "dtype": col.dtype, "t": col.tensor, "mask": col.mask}


def _same_column(a, b, where):
    pa, pb = _column_parts(a), _column_parts(b)
    assert list(pa) == list(pb), where
    for k in pa:
        if isinstance(pa[k], torch.Tensor):
            assert isinstance(pb[k], torch.Tensor), (where, k)
            assert pa[k].dtype == pb[k].dtype, (where, k)
            assert torch.equal(pa[k], pb[k]), (where, k)
        elif k == "pool":
            assert pa[k] is pb[k], (where, k)
        else:
            assert pa[k] == pb[k], (where, k)


def _drive(reducer_calls, steps=6, rows=3000, nkeys=500):
    """Six steps of a GroupReduceNode grouped by an int column and the
    string it determines; returns per step (emitted batch, state)."""
    from pathway_amd.engine import nodes
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import StringColumn, TensorColumn
    from pathway_amd.internals import dtype as dt
    from pathway_amd.internals import expression as ex

    names = StringColumn.from_strings([f"gu_word_{i}" for i in range(nkeys)], DEV)
    node = nodes.GroupReduceNode(
        None,
        {"g": ex.ColumnReference(None, "g"), "w": ex.ColumnReference(None, "w")},
        reducer_calls,
        DEV,
    )
    g = torch.Generator().manual_seed(2024)
    trace = []
    for step in range(steps):
        grp = torch.randint(0, nkeys, (rows,), generator=g).to(DEV)
        val = torch.randint(-50, 50, (rows,), generator=g).to(DEV)
        # step 0 only inserts; later steps retract about as often
        p_neg = 0.0 if step == 0 else 0.5
        diffs = torch.where(
            torch.rand(rows, generator=g) < p_neg, torch.tensor(-1), torch.tensor(1)
        ).to(torch.int64).to(DEV)
        seq = torch.arange(step * rows, (step + 1) * rows, dtype=torch.int64, device=DEV)
        batch = DeltaBatch(
            torch.stack([seq, seq * 7 + 1], dim=1),
            {
                "g": TensorColumn(grp, dt.INT),
                "w": names.take(grp),
                "v": TensorColumn(val, dt.INT),
            },
            diffs,
            2 * step,
        )
        out = node.step(2 * step, [batch])
        state = (
            [t.clone() for t in node.add_keys],
            {k: t.clone() for k, t in node.add_accs.items()},
            dict(node.add_carried),
        )
        trace.append((out, state))
    torch.cuda.synchronize()
    return trace


def _compare_traces(new, old):
    assert len(new) == len(old)
    for step, ((bn, sn), (bo, so)) in enumerate(zip(new, old)):
        assert (bn is None) == (bo is None), step
        if bn is not None:
            assert bn.time == bo.time and bn.consolidated and bo.consolidated
            assert torch.equal(bn.keys, bo.keys), step
            assert torch.equal(bn.diffs, bo.diffs), step
            assert list(bn.columns) == list(bo.columns), step
            for name in bn.columns:
                _same_column(bn.columns[name], bo.columns[name], (step, name))
        for a, b in zip(sn[0], so[0]):
            assert torch.equal(a, b), step
        assert list(sn[1]) == list(so[1]), step
        for name in sn[1]:
            assert sn[1][name].dtype == so[1][name].dtype
            assert torch.equal(sn[1][name], so[1][name]), (step, name)
        assert list(sn[2]) == list(so[2]), step
        for name in sn[2]:
            _same_column(sn[2][name], so[2][name], (step, "carried", name))


def _count_calls(monkeypatch):
    from pathway_amd import ops

    calls = []
    real = ops.group_update_gpu

    def counted(*args):
        calls.append(args[2][0].shape[0])
        return real(*args)

    monkeypatch.setattr(ops, "group_update_gpu", counted)
    return calls


@gpu
@requires_cuda
def test_node_count_and_sum_matches_chain(monkeypatch):
    from pathway_amd.engine import nodes
    from pathway_amd.internals import expression as ex

    reducers = {
        "c": ("count", [], {}),
        "s": ("sum", [ex.ColumnReference(None, "v")], {}),
    }
    calls = _count_calls(monkeypatch)
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_UPDATE", False)
    new = _drive(reducers)
    assert len(calls) == 6
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_UPDATE", True)
    old = _drive(reducers)
    assert len(calls) == 6  # the switch forced the chain
    _compare_traces(new, old)
    # the run exercises retractions, rows leaving and negative weights
    assert all(b is not None for b, _ in new)
    assert any(bool((b.diffs < 0).any()) for b, _ in new)
    assert any(bool((s[1]["__w__"] < 0).any()) for _, s in new)
    assert new[-1][1][0][0].shape[0] < 500


@gpu
@requires_cuda
def test_node_sum_only_matches_chain(monkeypatch):
    """No count reducer: slot 0 decides presence only."""
    from pathway_amd.engine import nodes
    from pathway_amd.internals import expression as ex

    reducers = {"s": ("sum", [ex.ColumnReference(None, "v")], {})}
    calls = _count_calls(monkeypatch)
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_UPDATE", False)
    new = _drive(reducers, steps=3)
    assert len(calls) == 3
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_UPDATE", True)
    old = _drive(reducers, steps=3)
    assert len(calls) == 3
    _compare_traces(new, old)


@gpu
@requires_cuda
def test_node_avg_takes_the_chain(monkeypatch):
    """An avg reducer is not the fused path's kind: the chain runs, with
    the same results whatever the switch says."""
    from pathway_amd.engine import nodes
    from pathway_amd.internals import expression as ex

    reducers = {
        "c": ("count", [], {}),
        "a": ("avg", [ex.ColumnReference(None, "v")], {}),
    }
    calls = _count_calls(monkeypatch)
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_UPDATE", False)
    new = _drive(reducers, steps=3)
    assert calls == []
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_UPDATE", True)
    old = _drive(reducers, steps=3)
    _compare_traces(new, old)
    assert all(b is not None for b, _ in new)

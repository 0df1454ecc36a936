"""GPU tests of the fused consolidation (pw_row_ident, pw_consolidate_rows):
the 128-bit row identity of every row in one kernel, then a prefix sort of
the identities, the diff sum per identity and the drop of the identities
that cancel, with one device-to-host read.  The hash is checked against the
torch formulation on CPU tensors (the CPU branch of hashing.hash128_words),
the op against a dict model on those CPU identities, and consolidate_batch
and a WordCount graph against the chain the call replaces
(PW_NO_CONSOLIDATE_FUSED=1).  All values are integers (the float column's
too): every comparison is exact."""

import warnings

import pytest
import torch

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"
N_OP = 2049
SIZES = [2049, 4097, 70001]


def _rand64(g, *shape):
    return torch.randint(-(2**63), 2**63 - 1, shape, generator=g, dtype=torch.int64)


# ------------------------------------------------------- op level: hash --

def _cpu_cols(g, n):
    """One CPU column of every kind: name -> (descriptor parts, (lo, hi))."""
    from pathway_amd.engine import hashing

    nlo, nhi = hashing.none_value_hash_scalar("cpu")
    cols = {}
    pay = _rand64(g, n)
    tag = hashing.TAG_INT
    cols["int"] = (
        ("int", pay, tag, None),
        hashing.hash128_words([torch.full_like(pay, tag), pay]),
    )
    pay2 = torch.randint(-5, 5, (n,), generator=g)
    mask = torch.rand(n, generator=g) < 0.7
    assert bool(mask.any()) and not bool(mask.all())
    lo, hi = hashing.hash128_words([torch.full_like(pay2, hashing.TAG_DURATION), pay2])
    cols["masked"] = (
        ("int", pay2, hashing.TAG_DURATION, mask),
        (torch.where(mask, lo, nlo), torch.where(mask, hi, nhi)),
    )
    pool_lo, pool_hi = _rand64(g, 37), _rand64(g, 37)
    codes = torch.randint(-1, 37, (n,), generator=g)
    assert bool((codes < 0).any()) and bool((codes == 36).any())
    safe = codes.clamp_min(0)
    cols["pool"] = (
        ("pool", codes, pool_lo, pool_hi),
        (
            torch.where(codes >= 0, pool_lo[safe], nlo),
            torch.where(codes >= 0, pool_hi[safe], nhi),
        ),
    )
    pairs = _rand64(g, n, 2)
    cols["ptr"] = (("ptr", pairs), hashing.pointer_value_hash(pairs))
    plo, phi = _rand64(g, n), _rand64(g, n)
    cols["pre"] = (("pre", plo, phi), (plo, phi))
    return cols


def _desc(parts):
    from pathway_amd import ops
    from pathway_amd.engine import hashing

    kind = parts[0]
    if kind == "int":
        m = parts[3].to(DEV) if parts[3] is not None else None
        return (ops.RI_INT64_TAGGED, parts[1].to(DEV), parts[2], m)
    if kind == "pool":
        return (ops.RI_POOL_CODE, *(t.to(DEV) for t in parts[1:]))
    if kind == "ptr":
        return (ops.RI_POINTER, parts[1].to(DEV), hashing.TAG_POINTER)
    return (ops.RI_PRECOMPUTED, parts[1].to(DEV), parts[2].to(DEV))


def _cpu_ident(keys, hashes):
    """(n,2) identities by the torch formulation, on CPU tensors."""
    from pathway_amd.engine import hashing

    n = keys.shape[0]
    if hashes:
        v0, v1 = hashing.hash128_words([w for lo_hi in hashes for w in lo_hi])
    else:
        v0 = v1 = torch.zeros(n, dtype=torch.int64)
    c0, c1 = hashing.hash128_words([keys[:, 0], keys[:, 1], v0, v1])
    return torch.stack([c0, c1], dim=1)


LAYOUTS = {
    "int": ["int"],
    "masked": ["masked"],
    "pool": ["pool"],
    "ptr": ["ptr"],
    "pre": ["pre"],
    "all_four": ["int", "pool", "ptr", "pre"],
    "none": [],
    "ten": ["int", "masked", "pool", "ptr", "pre", "pre", "ptr", "pool", "masked", "int"],
}


@gpu
@requires_cuda
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_row_ident_matches_torch_formulation(layout):
    from pathway_amd import ops

    g = torch.Generator().manual_seed(81)
    cols = _cpu_cols(g, N_OP)
    keys = _rand64(g, N_OP, 2)
    names = LAYOUTS[layout]
    want = _cpu_ident(keys, [cols[c][1] for c in names])
    got = ops.row_ident_gpu(keys.to(DEV), [_desc(cols[c][0]) for c in names])
    assert got.dtype == torch.int64 and got.shape == (N_OP, 2)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------ op level: group + drop --

def _model(ckeys, diffs):
    """rows, wsum of consolidate_rows_gpu from CPU identities, on dicts."""
    groups = {}
    for row, (ident, d) in enumerate(zip(map(tuple, ckeys.tolist()), diffs.tolist())):
        first, total = groups.get(ident, (row, 0))
        groups[ident] = (first, total + d)
    live = sorted((k, v) for k, v in groups.items() if v[1] != 0)
    return [v[0] for _, v in live], [v[1] for _, v in live]


@gpu
@requires_cuda
@pytest.mark.parametrize(
    "opts, path",
    [
        ({}, "fused"),
        # 8 rows a prefix run: every run goes through the repair
        ({"prefix_bits": 8}, "fused"),
        # runs of ~1000 rows against a limit of 2: the 64-bit sort takes over
        ({"prefix_bits": 1, "max_run": 2}, "overflow"),
    ],
)
def test_rows_and_sums_match_model(opts, path):
    from pathway_amd import ops

    g = torch.Generator().manual_seed(82)
    cols = _cpu_cols(g, N_OP)
    # 600 distinct rows drawn 2049 times: duplicates that add, cancel and stay
    r = torch.randint(0, 600, (N_OP,), generator=g)
    keys = _rand64(g, N_OP, 2)[r]
    (_, codes, pool_lo, pool_hi), (plo, phi) = cols["pool"]
    (_, pay, tag, mask), (mlo, mhi) = cols["masked"]
    parts = [("pool", codes[r], pool_lo, pool_hi), ("int", pay[r], tag, mask[r])]
    diffs = torch.randint(-1, 2, (N_OP,), generator=g)
    ckeys = _cpu_ident(keys, [(plo[r], phi[r]), (mlo[r], mhi[r])])
    want_rows, want_w = _model(ckeys, diffs)
    assert len(set(map(tuple, ckeys.tolist()))) == len(set(r.tolist()))
    assert 300 < len(want_rows) < len(set(r.tolist()))
    assert max(want_w) > 1 and min(want_w) < -1
    before = dict(ops.consolidate_path_counts)
    descs = [_desc(p) for p in parts]
    rows, wsum = ops.consolidate_rows_gpu(keys.to(DEV), descs, diffs.to(DEV), **opts)
    assert rows.dtype == torch.int64 and wsum.dtype == torch.int64
    assert rows.tolist() == want_rows
    assert wsum.tolist() == want_w
    # the same call handing out the rows' keys as well
    rows2, wsum2, out_keys = ops.consolidate_rows_gpu(
        keys.to(DEV), descs, diffs.to(DEV), gather_keys=True, **opts
    )
    assert torch.equal(rows2, rows) and torch.equal(wsum2, wsum)
    assert torch.equal(out_keys.cpu(), keys[want_rows])
    after = ops.consolidate_path_counts
    assert after["fused"] == before["fused"] + 2
    assert after["overflow"] == before["overflow"] + 2 * (path == "overflow")


# ---------------------------------------------------------- batch level --

_NAMES = None


def _names():
    global _NAMES
    if _NAMES is None:
        from pathway_amd.engine.column import StringColumn

        _NAMES = StringColumn.from_strings(
            [None] + [f"cr_word_{i}" for i in range(3000)], DEV
        )
    return _NAMES


def _wordcount_batch(g, keys, counts, diffs, order=None):
    """A (word, count) batch; the word is a function of the key."""
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import TensorColumn
    from pathway_amd.internals import dtype as dt

    words = (keys[:, 0] % 3001 + 3001) % 3001
    if order is None:
        order = torch.randperm(keys.shape[0], generator=g)
    keys, words, counts, diffs = (t[order].to(DEV) for t in (keys, words, counts, diffs))
    return DeltaBatch(
        keys,
        {"word": _names().take(words), "count": TensorColumn(counts, dt.INT)},
        diffs,
        4,
    )


def _both(monkeypatch, batch):
    """consolidate_batch through the fused call and through the chain."""
    from pathway_amd import ops
    from pathway_amd.engine import nodes

    c0 = dict(ops.consolidate_path_counts)
    monkeypatch.setattr(nodes, "_PW_NO_CONSOLIDATE_FUSED", False)
    new = nodes.consolidate_batch(batch)
    c1 = dict(ops.consolidate_path_counts)
    monkeypatch.setattr(nodes, "_PW_NO_CONSOLIDATE_FUSED", True)
    old = nodes.consolidate_batch(batch)
    c2 = dict(ops.consolidate_path_counts)
    return new, old, (c0, c1, c2)


def _assert_fused_then_chain(counts):
    c0, c1, c2 = counts
    assert (c1["fused"], c1["chain"]) == (c0["fused"] + 1, c0["chain"])
    assert (c2["fused"], c2["chain"]) == (c1["fused"], c1["chain"] + 1)
    assert c2["overflow"] == c0["overflow"]


def _column_tensors(col):
    from pathway_amd.engine.column import PointerColumn, StringColumn, TensorColumn

    if isinstance(col, StringColumn):
        return [col.codes]
    if isinstance(col, PointerColumn):
        return [col.pairs]
    assert isinstance(col, TensorColumn), type(col)
    return [col.tensor] + ([col.mask] if col.mask is not None else [])


def _assert_same_batch(new, old):
    assert (new is None) == (old is None)
    if new is None:
        return
    assert new.time == old.time and new.consolidated == old.consolidated
    assert new.keys.dtype == old.keys.dtype and torch.equal(new.keys, old.keys)
    assert new.diffs.dtype == old.diffs.dtype and torch.equal(new.diffs, old.diffs)
    assert list(new.columns) == list(old.columns)
    for name in new.columns:
        a, b = new.columns[name], old.columns[name]
        assert type(a) is type(b) and a.dtype == b.dtype, name
        ta, tb = _column_tensors(a), _column_tensors(b)
        assert len(ta) == len(tb), name
        for x, y in zip(ta, tb):
            assert x.dtype == y.dtype and torch.equal(x, y), name


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_all_distinct(monkeypatch, n):
    g = torch.Generator().manual_seed(n)
    batch = _wordcount_batch(
        g, _rand64(g, n, 2), torch.randint(0, 9, (n,), generator=g),
        torch.randint(1, 3, (n,), generator=g),
    )
    new, old, counts = _both(monkeypatch, batch)
    _assert_fused_then_chain(counts)
    _assert_same_batch(new, old)
    assert len(new) == n


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_old_new_pairs_both_survive(monkeypatch, n):
    g = torch.Generator().manual_seed(n + 1)
    m = n // 2
    base = _rand64(g, m + n % 2, 2)
    old_count = torch.randint(1, 50, (m,), generator=g)
    keys = torch.cat([base[:m], base])
    counts = torch.cat([old_count, old_count + 1, old_count[: n % 2] + 7])
    diffs = torch.cat([-torch.ones(m, dtype=torch.int64),
                       torch.ones(m + n % 2, dtype=torch.int64)])
    new, old, counts_ = _both(monkeypatch, _wordcount_batch(g, keys, counts, diffs))
    _assert_fused_then_chain(counts_)
    _assert_same_batch(new, old)
    assert len(new) == n
    assert int((new.diffs < 0).sum()) == m


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_duplicates_add(monkeypatch, n):
    g = torch.Generator().manual_seed(n + 2)
    triples = (n % 2) + 2 * (n // 10)  # n - 3 * triples is even
    doubles = (n - 3 * triples) // 2
    base = _rand64(g, doubles + triples, 2)
    cnt = torch.randint(0, 9, (doubles + triples,), generator=g)
    idx = torch.cat([torch.arange(doubles).repeat(2),
                     torch.arange(doubles, doubles + triples).repeat(3)])
    assert idx.shape[0] == n
    new, old, counts = _both(
        monkeypatch,
        _wordcount_batch(g, base[idx], cnt[idx], torch.ones(n, dtype=torch.int64)),
    )
    _assert_fused_then_chain(counts)
    _assert_same_batch(new, old)
    assert len(new) == doubles + triples
    assert int((new.diffs == 2).sum()) == doubles
    assert int((new.diffs == 3).sum()) == triples


def _cancelling(g, n, survivors):
    """n rows: `survivors` single rows, the rest exact duplicates whose
    diffs sum to zero (pairs +1/-1, and one +1/+1/-2 if the rest is odd)."""
    rest = n - survivors
    triple = rest % 2
    pairs = (rest - 3 * triple) // 2
    base = _rand64(g, survivors + pairs + triple, 2)
    cnt = torch.randint(0, 9, (base.shape[0],), generator=g)
    p = torch.arange(survivors, survivors + pairs)
    t = torch.arange(survivors + pairs, survivors + pairs + triple)
    idx = torch.cat([torch.arange(survivors), p, p, t, t, t])
    one = torch.ones
    diffs = torch.cat([
        one(survivors, dtype=torch.int64), one(pairs, dtype=torch.int64),
        -one(pairs, dtype=torch.int64), one(2 * triple, dtype=torch.int64),
        -2 * one(triple, dtype=torch.int64),
    ])
    assert idx.shape[0] == n == diffs.shape[0]
    return _wordcount_batch(g, base[idx], cnt[idx], diffs)


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_duplicates_cancel_among_survivors(monkeypatch, n):
    g = torch.Generator().manual_seed(n + 3)
    survivors = n // 3
    new, old, counts = _both(monkeypatch, _cancelling(g, n, survivors))
    _assert_fused_then_chain(counts)
    _assert_same_batch(new, old)
    assert len(new) == survivors


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_every_row_cancels(monkeypatch, n):
    g = torch.Generator().manual_seed(n + 4)
    new, old, counts = _both(monkeypatch, _cancelling(g, n, 0))
    _assert_fused_then_chain(counts)
    assert new is None and old is None


@gpu
@requires_cuda
def test_one_long_run(monkeypatch):
    g = torch.Generator().manual_seed(5)
    n = 2049
    keys = _rand64(g, 1, 2).expand(n, 2).contiguous()
    batch = _wordcount_batch(
        g, keys, torch.full((n,), 6), torch.ones(n, dtype=torch.int64)
    )
    new, old, counts = _both(monkeypatch, batch)
    _assert_fused_then_chain(counts)
    _assert_same_batch(new, old)
    assert len(new) == 1 and new.diffs.tolist() == [n]


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_float_and_bool_columns(monkeypatch, n):
    """Float and bool tensors go in as PRECOMPUTED value hashes."""
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import TensorColumn
    from pathway_amd.internals import dtype as dt

    g = torch.Generator().manual_seed(n + 6)
    m = n - n // 4
    base = _rand64(g, m, 2)
    f = torch.randint(-4, 4, (m,), generator=g).to(torch.float64) / 4
    b = torch.rand(m, generator=g) < 0.5
    # the first n - m rows twice: exact duplicates that add
    idx = torch.cat([torch.arange(m), torch.arange(n - m)])[
        torch.randperm(n, generator=g)
    ]
    batch = DeltaBatch(
        base[idx].to(DEV),
        {
            "f": TensorColumn(f[idx].to(DEV), dt.FLOAT),
            "b": TensorColumn(b[idx].to(DEV), dt.BOOL),
        },
        torch.ones(n, dtype=torch.int64, device=DEV),
        4,
    )
    new, old, counts = _both(monkeypatch, batch)
    _assert_fused_then_chain(counts)
    _assert_same_batch(new, old)
    assert len(new) == m and int((new.diffs == 2).sum()) == n - m


@gpu
@requires_cuda
def test_eleven_columns_take_the_chain(monkeypatch):
    from pathway_amd import ops
    from pathway_amd.engine import nodes
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import TensorColumn
    from pathway_amd.internals import dtype as dt

    g = torch.Generator().manual_seed(7)
    n = 2049
    keys = _rand64(g, n // 2 + 1, 2).repeat(2, 1)[:n]
    cols = {
        f"c{j}": TensorColumn((keys[:, 0] % (j + 2)).to(DEV), dt.INT)
        for j in range(11)
    }
    batch = DeltaBatch(
        keys.to(DEV), cols, torch.ones(n, dtype=torch.int64, device=DEV), 4
    )
    monkeypatch.setattr(nodes, "_PW_NO_CONSOLIDATE_FUSED", False)
    before = dict(ops.consolidate_path_counts)
    out = nodes.consolidate_batch(batch)
    after = ops.consolidate_path_counts
    assert after["chain"] == before["chain"] + 1
    assert after["fused"] == before["fused"]
    assert len(out) == n // 2 + 1 and int((out.diffs == 2).sum()) == n // 2
    # ten of them fit
    ten = DeltaBatch(batch.keys, dict(list(cols.items())[:10]), batch.diffs, 4)
    new, old, counts = _both(monkeypatch, ten)
    _assert_fused_then_chain(counts)
    _assert_same_batch(new, old)


# ----------------------------------------------------------- sync count --

@gpu
@requires_cuda
def test_one_device_to_host_read():
    """torch warns about every blocking device-to-host read in "warn"
    sync-debug mode; the all-distinct 70 001-row call makes exactly one."""
    from pathway_amd import ops
    from pathway_amd.engine import nodes

    n = 70001
    g = torch.Generator().manual_seed(8)
    batch = _wordcount_batch(
        g, _rand64(g, n, 2), torch.randint(0, 9, (n,), generator=g),
        torch.ones(n, dtype=torch.int64),
    )
    descs = nodes._row_ident_descs(batch)
    ops.consolidate_rows_gpu(batch.keys, descs, batch.diffs)  # sizes its temp
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rows, wsum = ops.consolidate_rows_gpu(batch.keys, descs, batch.diffs)
            reads_call = len(caught)
            # the counter counts: a read of our own is one more
            int(wsum[0])
            reads_probe = len(caught) - reads_call
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert reads_probe == 1
    assert reads_call == 1, [str(w.message) for w in caught]
    assert rows.shape[0] == n


# ----------------------------------------------------------- node level --

def _wordcount_trace(steps=4, rows=5000, vocab=3000):
    """groupby(word).reduce(word, count) -> select -> OutputNode; the
    batches the sink receives, step by step."""
    from pathway_amd.engine import nodes
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.runtime import OutputNode
    from pathway_amd.internals import expression as ex

    reduce_node = nodes.GroupReduceNode(
        None, {"word": ex.ColumnReference(None, "word")},
        {"count": ("count", [], {})}, DEV,
    )
    select = nodes.ExprMapNode(
        None,
        {"word": ex.ColumnReference(None, "word"),
         "count": ex.ColumnReference(None, "count")},
        DEV,
    )
    delivered = []
    sink = OutputNode(None, delivered.append, DEV)
    g = torch.Generator().manual_seed(9)
    trace = []
    for step in range(steps):
        codes = torch.randint(1, vocab + 1, (rows,), generator=g).to(DEV)
        seq = torch.arange(step * rows, (step + 1) * rows, dtype=torch.int64, device=DEV)
        batch = DeltaBatch(
            torch.stack([seq, seq * 7 + 1], dim=1),
            {"word": _names().take(codes)},
            torch.ones(rows, dtype=torch.int64, device=DEV),
            2 * step,
        )
        out = select.step(2 * step, [reduce_node.step(2 * step, [batch])])
        assert out is not None and not out.consolidated and len(out) > 2048
        before = len(delivered)
        sink.step(2 * step, [out])
        trace.append(delivered[before] if len(delivered) > before else None)
    return trace


@gpu
@requires_cuda
def test_wordcount_sink_receives_the_same_batches(monkeypatch):
    from pathway_amd import ops
    from pathway_amd.engine import nodes

    before = dict(ops.consolidate_path_counts)
    monkeypatch.setattr(nodes, "_PW_NO_CONSOLIDATE_FUSED", False)
    new = _wordcount_trace()
    mid = dict(ops.consolidate_path_counts)
    monkeypatch.setattr(nodes, "_PW_NO_CONSOLIDATE_FUSED", True)
    old = _wordcount_trace()
    after = ops.consolidate_path_counts
    assert mid["fused"] == before["fused"] + 4 and mid["chain"] == before["chain"]
    assert after["fused"] == mid["fused"] and after["chain"] == mid["chain"] + 4
    assert len(new) == len(old) == 4
    for a, b in zip(new, old):
        assert a is not None
        _assert_same_batch(a, b)
    # later steps carry retractions
    assert bool((new[-1].diffs < 0).any())

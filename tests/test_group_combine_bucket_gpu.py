"""GPU tests of the group combine's bucket path (pw_gc_bucket_*): one radix
pass on the top `bucket_bits` of word0, then one workgroup per bucket that
aggregates its rows in an LDS table and emits the bucket's unique keys in
order.  Every case is checked against a CPU model (lex sort, boundary mask,
index_add_, smallest row per segment), against group_combine_gpu with the
bucket path off, and against `ops.gc_path_counts`: a case meant for the
bucket path fails if the call quietly took another one.  All values are
integers: every comparison is exact."""

import functools

import pytest
import torch

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

_PATHS = ("prefix", "fallback", "full", "bucket")
_MIN64, _MAX64 = -(1 << 63), (1 << 63) - 1


def _rand64(g, n):
    return torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, generator=g)


def _contribs(g, n, nacc=2):
    """Mixed-sign contributions; from the third column on they are large
    enough for the sums to wrap past 2^63."""
    cols = []
    for a in range(nacc):
        if a == 0:
            c = torch.where(
                torch.rand(n, generator=g) < 0.3, torch.tensor(-1), torch.tensor(2)
            ).to(torch.int64)
        elif a == 1:
            c = torch.randint(-9, 9, (n,), generator=g)
        else:
            c = torch.randint(-(1 << 62), 1 << 62, (n,), generator=g) * 2 + a
        cols.append(c)
    return cols


def _reference(k0, k1, contribs):
    """CPU model: lex sort, boundary mask, index_add_; plus the smallest
    input row of every segment."""
    from pathway_amd.engine.state import lex_sort_words

    n = k0.shape[0]
    perm = lex_sort_words([k0, k1])
    s0 = k0.index_select(0, perm)
    s1 = k1.index_select(0, perm)
    starts = torch.ones(n, dtype=torch.bool)
    starts[1:] = (s0[1:] != s0[:-1]) | (s1[1:] != s1[:-1])
    seg = torch.cumsum(starts.to(torch.int64), 0) - 1
    fidx = starts.nonzero(as_tuple=True)[0]
    nseg = int(fidx.numel())
    sums = []
    for c in contribs:
        acc = torch.zeros(nseg, dtype=torch.int64)
        acc.index_add_(0, seg, c.index_select(0, perm))
        sums.append(acc)
    min_row = torch.full((nseg,), n, dtype=torch.int64)
    min_row.scatter_reduce_(0, seg, perm, "amin")
    return s0.index_select(0, fidx), s1.index_select(0, fidx), sums, min_row


class _Case:
    """Keys, contributions and the CPU reference of one input, built once
    and shared by the tests that use it."""

    def __init__(self, k0, k1, g, nacc=2):
        self.k0, self.k1 = k0, k1
        self.n = k0.shape[0]
        self.contribs = _contribs(g, self.n, nacc)
        self.ref = _reference(k0, k1, self.contribs)


def _counts():
    from pathway_amd import ops

    return {k: ops.gc_path_counts[k] for k in _PATHS}


def _call(case, expect, keys_dev=None, **kw):
    """One group_combine_gpu call, compared with the CPU model; `expect` is
    the one path whose count must rise, by one."""
    from pathway_amd import ops

    if keys_dev is None:
        keys_dev = torch.stack([case.k0, case.k1], dim=1).cuda()
    before = _counts()
    uk0, uk1, first, accs = ops.group_combine_gpu(
        keys_dev, [c.cuda() for c in case.contribs], **kw
    )
    after = _counts()
    delta = {k: after[k] - before[k] for k in _PATHS}
    want = dict.fromkeys(_PATHS, 0)
    want[expect] = 1
    assert delta == want
    r0, r1, rsums, rmin = case.ref
    assert uk0.shape[0] == r0.shape[0]
    assert torch.equal(uk0.cpu(), r0)
    assert torch.equal(uk1.cpu(), r1)
    assert len(accs) == len(case.contribs)
    for got, ref in zip(accs, rsums):
        assert got.dtype == torch.int64
        assert torch.equal(got.cpu(), ref)
    assert first.dtype == torch.int64
    assert torch.equal(first.cpu(), rmin)
    return uk0, uk1, first, accs


def _run(case, expect="bucket", keys_dev=None, **kw):
    """The call with the bucket path on (expected to end on `expect`) and
    the same call with it off: both equal the CPU model and each other."""
    got = _call(case, expect, keys_dev=keys_dev, bucket=True, **kw)
    off_kw = {k: v for k, v in kw.items() if k in ("prefix_bits", "max_run", "max_dirty")}
    off = _call(case, "prefix", keys_dev=keys_dev, bucket=False, **off_kw)
    for a, b in zip(got[:3], off[:3]):
        assert torch.equal(a, b)
    for a, b in zip(got[3], off[3]):
        assert torch.equal(a, b)
    return got


def _top8(b):
    """A signed word0 whose top 8 bits, sign flipped, are bucket b of 256."""
    return ((b ^ 0x80) - 256 if (b ^ 0x80) >= 128 else (b ^ 0x80)) << 56


def _in_bucket(g, count, b):
    """`count` random word0 values in bucket b (of 256): distinct low bits."""
    low = torch.randperm(1 << 20, generator=g)[:count] * 0x3FFFFFFFF7 + 11
    return _top8(b) | (low & ((1 << 56) - 1))


def _rows(g, t0, t1, n, every=True):
    """n rows drawn from the key table (t0, t1); every key at least once."""
    m = t0.shape[0]
    ids = torch.randint(0, m, (n,), generator=g)
    if every:
        assert n >= m
        ids[torch.randperm(n, generator=g)[:m]] = torch.arange(m)
    return t0[ids], t1[ids]


# ------------------------------------------------------------ tiny, ragged --

@functools.lru_cache(maxsize=None)
def _ragged(n):
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    m = 300 if n == 5000 else max(1, (n + 1) // 2)
    t0, t1 = _rand64(g, m) * 4 + 1, _rand64(g, m)
    k0, k1 = _rows(g, t0, t1, n)
    case = _Case(k0, k1, g)
    assert case.ref[0].shape[0] == m
    return case


@gpu
@requires_cuda
@pytest.mark.parametrize("bits", [1, 4, 8])
@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 5000])
def test_tiny_and_ragged_sizes(n, bits):
    _run(_ragged(n), bucket_bits=bits)


# --------------------------------------------------- empty and full buckets --

@functools.lru_cache(maxsize=None)
def _bucket_use(which):
    g = torch.Generator(device="cpu").manual_seed(7)
    used = {"one": [0x5A], "ends": [0, 255], "few": [3, 128, 200]}[which]
    t0 = torch.cat([_in_bucket(g, 60, b) for b in used])
    t1 = _rand64(g, t0.shape[0])
    k0, k1 = _rows(g, t0, t1, 4099)
    case = _Case(k0, k1, g)
    top = ((k0 >> 56) + 128).unique().tolist()  # sign-flipped top byte
    assert top == used
    return case


@gpu
@requires_cuda
@pytest.mark.parametrize("which", ["one", "ends", "few"])
def test_empty_and_full_buckets(which):
    _run(_bucket_use(which))


# -------------------------------------------------------------- sign order --

@gpu
@requires_cuda
@pytest.mark.parametrize("bits", [1, 8])
def test_sign_order(bits):
    g = torch.Generator(device="cpu").manual_seed(11)
    w0s = [_MIN64, -1, 0, _MAX64]
    w1s = [_MIN64, -5, -1, 0, 7, _MAX64]
    t0 = torch.tensor([a for a in w0s for _ in w1s], dtype=torch.int64)
    t1 = torch.tensor([b for _ in w0s for b in w1s], dtype=torch.int64)
    k0, k1 = _rows(g, t0, t1, 2049)
    case = _Case(k0, k1, g)
    uk0, uk1, _, _ = _run(case, bucket_bits=bits)
    # signed lexicographic order, spelled out
    assert uk0.cpu().tolist() == [a for a in w0s for _ in w1s]
    assert uk1.cpu().tolist() == [b for _ in w0s for b in w1s]


# ------------------------------------------ same word0, different word1 ----

@gpu
@requires_cuda
def test_same_word0_different_word1():
    g = torch.Generator(device="cpu").manual_seed(13)
    w0 = _in_bucket(g, 40, 0x91)
    # 40 word0 values x 5 word1 values, both signs
    a0 = w0.repeat_interleave(5)
    a1 = torch.tensor([-(1 << 62), -3, 0, 3, 1 << 62], dtype=torch.int64).repeat(40)
    # same low 32 bits of word0 (and the same bucket), different word1
    low = 0x1234ABCD
    mid = torch.arange(1, 41, dtype=torch.int64) << 32
    b0 = _top8(0x91) | mid | low
    b1 = _rand64(g, 40)
    # the same full word0 as one of those, word1 off by one
    c0, c1 = b0[:10].clone(), b1[:10] + 1
    t0, t1 = torch.cat([a0, b0, c0]), torch.cat([a1, b1, c1])
    k0, k1 = _rows(g, t0, t1, 5000)
    case = _Case(k0, k1, g)
    assert case.ref[0].shape[0] == 250
    _run(case)


# -------------------------------------------- duplicates under contention --

@gpu
@requires_cuda
def test_three_keys_65536_rows_repeatable():
    g = torch.Generator(device="cpu").manual_seed(17)
    t0 = _in_bucket(g, 2, 0x33)
    t0 = torch.cat([t0, t0[:1]])          # two keys share word0
    t1 = torch.tensor([5, -5, 6], dtype=torch.int64)
    k0, k1 = _rows(g, t0, t1, 65_536)
    case = _Case(k0, k1, g)
    assert case.ref[0].shape[0] == 3
    keys_dev = torch.stack([k0, k1], dim=1).cuda()
    runs = [_call(case, "bucket", keys_dev=keys_dev, bucket=True) for _ in range(4)]
    for r in runs[1:]:
        for a, b in zip(r[:3], runs[0][:3]):
            assert torch.equal(a, b)
        for a, b in zip(r[3], runs[0][3]):
            assert torch.equal(a, b)
    # bucket path off: ~43k rows tie on one word0, over the repair's max_run
    _call(case, "fallback", keys_dev=keys_dev, bucket=False)


# ------------------------------------------------------------ capacity edge --

@functools.lru_cache(maxsize=None)
def _one_bucket(distinct, n):
    g = torch.Generator(device="cpu").manual_seed(19 + distinct)
    t0 = _in_bucket(g, distinct, 0xC4)
    k0, k1 = _rows(g, t0, _rand64(g, distinct), n)
    return _Case(k0, k1, g)


@gpu
@requires_cuda
@pytest.mark.parametrize("distinct,expect", [(32, "bucket"), (33, "prefix")])
def test_capacity_edge(distinct, expect):
    from pathway_amd import ops

    assert int(ops.GC_BUCKET_MAX_LOAD * 64) == 32
    _run(_one_bucket(distinct, 2049), expect=expect, table_capacity=64)


@gpu
@requires_cuda
@pytest.mark.parametrize("n,expect", [(1000, "bucket"), (1001, "prefix")])
def test_max_bucket_rows_edge(n, expect):
    _run(_one_bucket(20, n), expect=expect, max_bucket_rows=1000)


# ------------------------------------------------------------ nacc 0 and 8 --

@gpu
@requires_cuda
@pytest.mark.parametrize("nacc", [0, 8])
def test_nacc_0_and_8(nacc):
    g = torch.Generator(device="cpu").manual_seed(23)
    t0, t1 = _rand64(g, 300) * 4 + 2, _rand64(g, 300)
    k0, k1 = _rows(g, t0, t1, 5000)
    case = _Case(k0, k1, g, nacc=nacc)
    if nacc:
        # precondition: some exact sum lies outside int64, so it wrapped
        big = case.contribs[2].tolist()
        exact = {}
        for a, b, v in zip(k0.tolist(), k1.tolist(), big):
            exact[(a, b)] = exact.get((a, b), 0) + v
        assert any(not _MIN64 <= s <= _MAX64 for s in exact.values())
        assert any(bool((c < 0).any()) and bool((c > 0).any()) for c in case.contribs)
    _run(case)


# ----------------------------------------------------------- strided input --

@gpu
@requires_cuda
def test_strided_and_offset_input():
    case = _ragged(5000)
    g = torch.Generator(device="cpu").manual_seed(29)
    keys = torch.stack([case.k0, case.k1], dim=1)
    wide = torch.stack([_rand64(g, 10000), _rand64(g, 10000)], dim=1)
    wide[::2] = keys
    every_other = wide.cuda()[::2]
    assert every_other.stride() == (4, 1)
    _run(case, keys_dev=every_other)
    tall = torch.cat([wide[:3], keys]).cuda()
    tail = tall[3:]
    assert tail.stride() == (2, 1) and tail.storage_offset() == 6
    _run(case, keys_dev=tail)


# -------------------------------------------------------------- node level --

def _run_stream(n, vocab_per_step):
    """groupby(word).reduce(count, sum) over len(vocab_per_step) steps of n
    rows; step s draws its words from the first vocab_per_step[s] words of
    the pool.  Returns the emitted DeltaBatches."""
    import pathway_amd as pw
    from pathway_amd.engine import hashing
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import (
        GLOBAL_STRING_POOL,
        StringColumn,
        TensorColumn,
    )
    from pathway_amd.engine.nodes import InputNode
    from pathway_amd.engine.runtime import OutputNode, Runtime
    from pathway_amd.internals import dtype as dt
    from pathway_amd.internals.api import TAG_INT
    from pathway_amd.internals.table import Table
    from pathway_amd.internals.universe import Universe

    dev = torch.device("cuda:0")
    pool_codes = torch.from_numpy(
        GLOBAL_STRING_POOL.codes([f"gcb{i:05d}" for i in range(max(vocab_per_step))])
    )
    g = torch.Generator(device="cpu").manual_seed(31)
    picks, vals = [], []
    for v in vocab_per_step:
        ids = torch.randperm(v, generator=g)[:n] if v >= n else torch.randint(
            0, v, (n,), generator=g
        )
        picks.append(pool_codes[ids])
        vals.append(torch.randint(-50, 50, (n,), generator=g))

    class Source:
        def next_time(self):
            return None

        def pull(self, t, d):
            step = t // 2
            seq = torch.arange(step * n, (step + 1) * n, dtype=torch.int64, device=d)
            klo, khi = hashing.value_hash_words(seq, TAG_INT)
            cols = {
                "word": StringColumn(picks[step].to(d), GLOBAL_STRING_POOL, dt.STR),
                "val": TensorColumn(vals[step].to(d), dt.INT),
            }
            diffs = torch.ones(n, dtype=torch.int64, device=d)
            return DeltaBatch(torch.stack([klo, khi], dim=1), cols, diffs, t)

    words = Table(InputNode(Source(), dev), {"word": dt.STR, "val": dt.INT}, Universe())
    res = words.groupby(pw.this.word).reduce(
        pw.this.word,
        count=pw.reducers.count(),
        total=pw.reducers.sum(pw.this.val),
    )
    out = []
    rt = Runtime([OutputNode(res._node, out.append, dev)], device=dev)
    for s in range(len(vocab_per_step)):
        rt.step_once(2 * s)
    torch.cuda.synchronize()
    return out


def _batch_tensors(b):
    from pathway_amd.engine.column import PointerColumn, StringColumn, TensorColumn

    ts = {"__keys__": b.keys, "__diffs__": b.diffs}
    for name, col in b.columns.items():
        if isinstance(col, StringColumn):
            ts[name] = col.codes
        elif isinstance(col, PointerColumn):
            ts[name] = col.pairs
        else:
            assert isinstance(col, TensorColumn), type(col)
            ts[name] = col.tensor
    return ts


def _spy_paths(monkeypatch):
    """Record, per group_combine_gpu call, which path's count rose."""
    from pathway_amd import ops

    paths = []
    real = ops.group_combine_gpu

    def spy(keys_n2, contribs):
        before = _counts()
        res = real(keys_n2, contribs)
        after = _counts()
        paths.append([k for k in _PATHS if after[k] != before[k]])
        return res

    monkeypatch.setattr(ops, "group_combine_gpu", spy)
    return paths


def _device(monkeypatch):
    from pathway_amd.internals.config import pathway_config

    monkeypatch.setenv("PW_DEVICE", "cuda:0")
    monkeypatch.setattr(pathway_config, "device", "cuda:0")


@gpu
@requires_cuda
def test_node_stream_equals_switched_off(monkeypatch):
    from pathway_amd.engine import nodes

    _device(monkeypatch)
    paths = _spy_paths(monkeypatch)
    n = 4099
    monkeypatch.setattr(nodes, "_PW_NO_GC_BUCKET", False)
    on = _run_stream(n, [300, 300, 300])
    assert paths == [["bucket"]] * 3
    del paths[:]
    monkeypatch.setattr(nodes, "_PW_NO_GC_BUCKET", True)
    off = _run_stream(n, [300, 300, 300])
    assert paths == [["prefix"]] * 3
    assert len(on) == len(off) == 3
    for bn, bo in zip(on, off):
        assert bn.time == bo.time
        tn, to = _batch_tensors(bn), _batch_tensors(bo)
        assert list(tn) == list(to)
        for name in tn:
            assert torch.equal(tn[name], to[name]), name


@gpu
@requires_cuda
def test_node_backs_off_after_overflow(monkeypatch):
    """With 16-entry tables a bucket holds 8 distinct keys.  Step 2's 4096
    distinct words (16 a bucket) overflow: it is redone on the prefix path
    and the node skips the bucket path for the next 4 steps, then takes it
    again."""
    from pathway_amd import ops
    from pathway_amd.engine import nodes

    _device(monkeypatch)
    monkeypatch.setattr(nodes, "_PW_NO_GC_BUCKET", False)
    monkeypatch.setattr(ops, "gc_bucket_capacity", lambda nacc: 16)
    assert nodes._GC_BUCKET_BACKOFF_MIN == 4
    paths = _spy_paths(monkeypatch)
    n = 4096
    small = 100
    _run_stream(n, [small, n] + [small] * 5)
    assert paths == [["bucket"], ["prefix"]] + [["prefix"]] * 4 + [["bucket"]]

"""GPU tests of the group-combine path (pw_gc_*): interleaved (n,2) keys +
contributions -> (unique keys, sums, first row), against the CPU path
(lex_sort_words on CPU tensors, boundary mask, index_add_).  All values are
integers: every comparison is exact."""

import pytest
import torch

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

# just over the 2048 fast-path threshold; none a multiple of 64 or 256;
# the last spans ~3900 blocks of 256 rows
SIZES = (2049, 4099, 65_539, 1_000_003)

_GOLDEN = 0x9E3779B185EBCA87 - (1 << 64)  # the xxhash prime as signed int64


def _rand64(g, n):
    return torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, generator=g)


def _contribs(g, n):
    """The weight/value mix of test_seg_reduce_matches_reference."""
    w = torch.where(
        torch.rand(n, generator=g) < 0.3, torch.tensor(-1), torch.tensor(2)
    ).to(torch.int64)
    v = torch.randint(-9, 9, (n,), generator=g)
    return [w, v]


def _keys(case, n, g):
    """(k0, k1) CPU int64 words, unsorted."""
    if case == "dup37":
        ids = torch.randint(0, 37, (n,), generator=g)
        k0 = ids * _GOLDEN + 7  # wraps: both signs
        return k0, k0 * 3 + 1
    if case == "distinct":
        # word0 is a bijection of the row index (odd multiplier mod 2^64)
        k0 = torch.randperm(n, generator=g) * _GOLDEN + 7
        return k0, _rand64(g, n)
    if case == "single":
        return torch.full((n,), -5, dtype=torch.int64), torch.full(
            (n,), 11, dtype=torch.int64
        )
    if case == "signed":
        # 80 keys around zero covering all four sign combinations of
        # (word0, word1); word1 is a function of word0, so no two distinct
        # keys share word0
        k0 = torch.randint(-40, 40, (n,), generator=g)
        k1 = (k0 % 7 - 3) * ((1 << 61) + 12345)
        k0 = k0 * ((1 << 57) + 3)
        return k0, k1
    raise AssertionError(case)


def _reference(k0, k1, contribs):
    """CPU path: lex sort, boundary mask, index_add_; plus the smallest
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


def _check(keys_dev, k0, k1, contribs, smallest_first=True):
    from pathway_amd import ops

    uk0, uk1, first, accs = ops.group_combine_gpu(
        keys_dev, [c.cuda() for c in contribs]
    )
    r0, r1, rsums, rmin = _reference(k0, k1, contribs)
    assert uk0.shape[0] == r0.shape[0]
    assert torch.equal(uk0.cpu(), r0)
    assert torch.equal(uk1.cpu(), r1)
    assert len(accs) == len(contribs)
    for got, ref in zip(accs, rsums):
        assert torch.equal(got.cpu(), ref)
    first = first.cpu()
    assert first.dtype == torch.int64
    assert bool(((first >= 0) & (first < k0.shape[0])).all())
    # the representative is a row of the input carrying the segment's key
    assert torch.equal(k0.index_select(0, first), r0)
    assert torch.equal(k1.index_select(0, first), r1)
    if smallest_first:
        assert torch.equal(first, rmin)


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["dup37", "distinct", "single", "signed"])
def test_group_combine_matches_cpu_path(case, n):
    g = torch.Generator(device="cpu").manual_seed(11 + n)
    k0, k1 = _keys(case, n, g)
    contribs = _contribs(g, n)
    keys = torch.stack([k0, k1], dim=1).cuda()  # interleaved (n,2)
    assert keys.stride() == (2, 1)
    _check(keys, k0, k1, contribs)


def _collision_keys(n, g):
    """Forced word0 collisions built as in test_sort_repair_collisions:
    200 colliding pairs + one run of 4 equal word0, distinct word1, every
    colliding key occurring once."""
    k0 = _rand64(g, n)
    k1 = _rand64(g, n)
    dup = torch.randint(0, n, (200,), generator=g)
    k0[dup] = k0[(dup + 1) % n]
    k0[10:14] = k0[10].clone()
    return k0, k1


@gpu
@requires_cuda
@pytest.mark.parametrize("n", [65_539, 1_000_003])
def test_group_combine_word0_collisions(n):
    g = torch.Generator(device="cpu").manual_seed(11)
    k0, k1 = _collision_keys(n, g)
    # precondition on the built input: the bound the repair guarantees
    # (equal-word0 runs of at most 4, all full keys distinct)
    s0 = k0.sort().values
    run = torch.ones(n, dtype=torch.int64)
    for d in (1, 2, 3, 4):
        run[d:] += (s0[d:] == s0[:-d]).to(torch.int64)
    assert int(run.max()) == 4
    assert int((s0[1:] == s0[:-1]).sum()) >= 200
    keys = torch.stack([k0, k1], dim=1).cuda()
    # all keys distinct: one row per segment, so first_row is fully
    # determined and _check pins it through the key equality
    _check(keys, k0, k1, _contribs(g, n))


@gpu
@requires_cuda
def test_group_combine_input_layouts():
    n = 4099
    g = torch.Generator(device="cpu").manual_seed(5)
    k0, k1 = _keys("dup37", n, g)
    contribs = _contribs(g, n)
    # column-sliced view of a wider tensor: rows 32 B apart -> the
    # .contiguous() fallback
    wide = torch.stack([_rand64(g, n), k0, k1, _rand64(g, n)], dim=1).cuda()
    view = wide[:, 1:3]
    assert view.stride() == (4, 1)
    _check(view, k0, k1, contribs)
    # row-sliced view: rows 16 B apart at a storage offset -> used in place
    tall = torch.cat(
        [torch.stack([_rand64(g, 3), _rand64(g, 3)], dim=1),
         torch.stack([k0, k1], dim=1)]
    ).cuda()
    tail = tall[3:]
    assert tail.stride() == (2, 1) and tail.storage_offset() == 6
    _check(tail, k0, k1, contribs)
    # no contribution columns at all: keys and first rows only
    _check(tall[3:], k0, k1, [])


def _run_wordcount_stream(n, vocab_n):
    """3-step groupby(word, id=wkey).reduce(count) stream; step 3 retracts
    half of step 1's rows.  Returns the emitted DeltaBatches."""
    import pathway_amd as pw
    from pathway_amd.engine import hashing
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import (
        GLOBAL_STRING_POOL,
        PointerColumn,
        StringColumn,
    )
    from pathway_amd.engine.nodes import InputNode
    from pathway_amd.engine.runtime import OutputNode, Runtime
    from pathway_amd.internals import dtype as dt
    from pathway_amd.internals.api import TAG_INT
    from pathway_amd.internals.table import Table
    from pathway_amd.internals.universe import Universe

    dev = torch.device("cuda:0")
    pool_codes = torch.from_numpy(
        GLOBAL_STRING_POOL.codes([f"gcw{i:04d}" for i in range(vocab_n)])
    )
    plo, phi = GLOBAL_STRING_POOL.hash_tensors(dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    picks = [
        pool_codes[torch.randint(0, vocab_n, (n,), generator=g)] for _ in range(3)
    ]
    half = n // 2
    picks[2][half:] = picks[0][: n - half]  # rows retracted in step 3

    class Source:
        def next_time(self):
            return None

        def pull(self, t, d):
            step = t // 2
            codes = picks[step].to(d)
            seq = torch.arange(step * n, (step + 1) * n, dtype=torch.int64, device=d)
            diffs = torch.ones(n, dtype=torch.int64, device=d)
            if step == 2:
                seq[half:] = torch.arange(n - half, dtype=torch.int64, device=d)
                diffs[half:] = -1
            klo, khi = hashing.value_hash_words(seq, TAG_INT)
            cols = {
                "word": StringColumn(codes, GLOBAL_STRING_POOL, dt.STR),
                "wkey": PointerColumn(
                    torch.stack(
                        [plo.index_select(0, codes), phi.index_select(0, codes)],
                        dim=1,
                    )
                ),
            }
            return DeltaBatch(torch.stack([klo, khi], dim=1), cols, diffs, t)

    words = Table(
        InputNode(Source(), dev), {"word": dt.STR, "wkey": dt.POINTER}, Universe()
    )
    counts = words.groupby(pw.this.word, id=pw.this.wkey).reduce(
        pw.this.word, count=pw.reducers.count()
    )
    out = []
    rt = Runtime([OutputNode(counts._node, out.append, dev)], device=dev)
    for t in (0, 2, 4):
        rt.step_once(t)
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


@gpu
@requires_cuda
def test_group_reduce_node_matches_old_branch(monkeypatch):
    from pathway_amd import ops
    from pathway_amd.engine import nodes
    from pathway_amd.internals.config import pathway_config

    calls = []
    real = ops.group_combine_gpu

    def counted(keys_n2, contribs):
        calls.append(keys_n2.shape[0])
        return real(keys_n2, contribs)

    monkeypatch.setattr(ops, "group_combine_gpu", counted)
    monkeypatch.setenv("PW_DEVICE", "cuda:0")
    monkeypatch.setattr(pathway_config, "device", "cuda:0")
    n = 4099
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_COMBINE", False)
    new = _run_wordcount_stream(n, 300)
    assert calls == [n, n, n]
    monkeypatch.setattr(nodes, "_PW_NO_GROUP_COMBINE", True)
    old = _run_wordcount_stream(n, 300)
    assert calls == [n, n, n]  # the switch forced the old branch

    assert len(new) == len(old) == 3
    assert any(bool((b.diffs < 0).any()) for b in new)
    for bn, bo in zip(new, old):
        assert bn.time == bo.time
        tn, to = _batch_tensors(bn), _batch_tensors(bo)
        assert list(tn) == list(to)
        for name in tn:
            assert torch.equal(tn[name], to[name]), name

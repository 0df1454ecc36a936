"""GPU tests of the group combine's prefix-sort path (pw_gc_prefix_*): the
sort sees only the top `prefix_bits` of word0, and the rows that tie on
that prefix are repaired on the device.  Every case is checked against the
CPU path (lex_sort_words, boundary mask, index_add_, smallest row per
segment) and against `ops.gc_path_counts`, which says whether the prefix
path held or the batch was redone with the 64-bit sort.  All values are
integers: every comparison is exact."""

import functools

import pytest
import torch

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

_GOLDEN = 0x9E3779B185EBCA87 - (1 << 64)  # the xxhash prime as signed int64


def _rand64(g, n):
    return torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, generator=g)


def _contribs(g, n):
    w = torch.where(
        torch.rand(n, generator=g) < 0.3, torch.tensor(-1), torch.tensor(2)
    ).to(torch.int64)
    v = torch.randint(-9, 9, (n,), generator=g)
    return [w, v]


def _w0(hi, lo):
    """word0 from a signed top half and an unsigned low half."""
    return (hi << 32) | lo


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


def _tied_runs(k0, k1, prefix_bits=32):
    """(start, length) in sorted order of every prefix run that holds more
    than one distinct key: the runs the device has to repair."""
    from pathway_amd.engine.state import lex_sort_words

    perm = lex_sort_words([k0, k1])
    s0 = k0.index_select(0, perm)
    s1 = k1.index_select(0, perm)
    pref = s0 >> (64 - prefix_bits)  # arithmetic shift keeps the order
    n = k0.shape[0]
    new_run = torch.ones(n, dtype=torch.bool)
    new_run[1:] = pref[1:] != pref[:-1]
    new_key = torch.ones(n, dtype=torch.bool)
    new_key[1:] = (s0[1:] != s0[:-1]) | (s1[1:] != s1[:-1])
    run_id = torch.cumsum(new_run.to(torch.int64), 0) - 1
    nrun = int(run_id[-1]) + 1
    keys_in_run = torch.zeros(nrun, dtype=torch.int64).index_add_(
        0, run_id, new_key.to(torch.int64)
    )
    length = torch.bincount(run_id, minlength=nrun)
    start = new_run.nonzero(as_tuple=True)[0]
    tied = keys_in_run > 1
    return list(zip(start[tied].tolist(), length[tied].tolist()))


class _Case:
    """Keys, contributions and the CPU reference of one input, built once
    and shared by the tests that use it."""

    def __init__(self, k0, k1, g):
        self.k0, self.k1 = k0, k1
        self.n = k0.shape[0]
        self.contribs = _contribs(g, self.n)
        self.ref = _reference(k0, k1, self.contribs)


def _run(case, keys_dev=None, contribs=None, expect=None, **kw):
    """Run group_combine_gpu, compare with the reference, and check which
    path gc_path_counts says it took."""
    from pathway_amd import ops

    if keys_dev is None:
        keys_dev = torch.stack([case.k0, case.k1], dim=1).cuda()
    if contribs is None:
        contribs = case.contribs
    before = dict(ops.gc_path_counts)
    uk0, uk1, first, accs = ops.group_combine_gpu(
        keys_dev, [c.cuda() for c in contribs], **kw
    )
    after = dict(ops.gc_path_counts)
    r0, r1, rsums, rmin = case.ref
    assert uk0.shape[0] == r0.shape[0]
    assert torch.equal(uk0.cpu(), r0)
    assert torch.equal(uk1.cpu(), r1)
    assert len(accs) == len(contribs)
    for got, ref in zip(accs, rsums):
        assert torch.equal(got.cpu(), ref)
    assert first.dtype == torch.int64
    assert torch.equal(first.cpu(), rmin)
    if expect is not None:
        delta = {k: after[k] - before[k] for k in after}
        want = {"prefix": 0, "fallback": 0, "full": 0}
        want[expect] = 1
        assert delta == want
    return uk0, uk1, first, accs


# 9 keys in three tied groups + 28 keys with a prefix of their own
_A_HI, _B_HI, _C_HI = 0x12345678, -0x20000000, -1
_TIED_KEYS = [
    # A: one top half, three low halves (one with its top bit set)
    (_w0(_A_HI, 5), 77),
    (_w0(_A_HI, 0x80000001), -3),
    (_w0(_A_HI, 0xFFFFFFFF), 1 << 40),
    # B: one negative word0, word1 of both signs
    (_w0(_B_HI, 0x1234), 9),
    (_w0(_B_HI, 0x1234), -7),
    # C: both kinds of tie under one negative prefix
    (_w0(_C_HI, 3), 100),
    (_w0(_C_HI, 3), -100),
    (_w0(_C_HI, 0x90000000), 5),
    (_w0(_C_HI, 0x90000000), -(1 << 62)),
]


@functools.lru_cache(maxsize=None)
def _interleaved(n):
    g = torch.Generator(device="cpu").manual_seed(23 + n)
    t0 = torch.tensor([k[0] for k in _TIED_KEYS], dtype=torch.int64)
    t1 = torch.tensor([k[1] for k in _TIED_KEYS], dtype=torch.int64)
    f0 = torch.arange(1, 29, dtype=torch.int64) * _GOLDEN + 7
    table0 = torch.cat([t0, f0])
    table1 = torch.cat([t1, f0 * 3 + 1])
    assert table0.shape[0] == 37
    ids = torch.randint(0, 37, (n,), generator=g)
    case = _Case(table0[ids], table1[ids], g)
    # precondition: exactly the three built groups tie, at 32 and at 24 bits
    for bits in (32, 24):
        runs = _tied_runs(case.k0, case.k1, bits)
        assert len(runs) == 3, runs
    assert bool((case.k0 < 0).any()) and bool((case.k1 < 0).any())
    return case


@gpu
@requires_cuda
@pytest.mark.parametrize("n", [2049, 4099, 65_539])
def test_interleaved_prefix_ties(n):
    case = _interleaved(n)
    longest = max(length for _, length in _tied_runs(case.k0, case.k1))
    if n == 65_539:
        assert longest > 2048  # ~5k rows: over max_run
        _run(case, expect="fallback")
    else:
        assert longest <= 2048
        _run(case, expect="prefix")


@gpu
@requires_cuda
def test_interleaved_prefix_bits_24():
    _run(_interleaved(4099), expect="prefix", prefix_bits=24)


@gpu
@requires_cuda
def test_full_sort_equals_default():
    case = _interleaved(4099)
    got = _run(case, expect="prefix")
    full = _run(case, expect="full", full_sort=True)
    for a, b in zip(got[:3], full[:3]):
        assert torch.equal(a, b)
    for a, b in zip(got[3], full[3]):
        assert torch.equal(a, b)


@gpu
@requires_cuda
def test_prefix_path_no_contribs_and_row_slice():
    case = _interleaved(2049)
    g = torch.Generator(device="cpu").manual_seed(5)
    tall = torch.cat(
        [torch.stack([_rand64(g, 3), _rand64(g, 3)], dim=1),
         torch.stack([case.k0, case.k1], dim=1)]
    ).cuda()
    tail = tall[3:]
    assert tail.stride() == (2, 1) and tail.storage_offset() == 6
    _run(case, keys_dev=tail, expect="prefix")
    _run(case, contribs=[], expect="prefix")


def _rows_from_counts(keys, counts, g):
    """Rows of `keys` (list of (word0, word1)), key j repeated counts[j]
    times, in random order."""
    k0 = torch.tensor([k[0] for k in keys], dtype=torch.int64)
    k1 = torch.tensor([k[1] for k in keys], dtype=torch.int64)
    ids = torch.repeat_interleave(
        torch.arange(len(keys)), torch.tensor(counts, dtype=torch.int64)
    )
    ids = ids[torch.randperm(ids.shape[0], generator=g)]
    return k0[ids], k1[ids]


def _fillers(g, count, lo_hi, hi_hi):
    """`count` keys with distinct top halves in [lo_hi, hi_hi)."""
    his = (torch.randperm(hi_hi - lo_hi, generator=g)[:count] + lo_hi).tolist()
    los = torch.randint(0, 1 << 32, (count,), generator=g).tolist()
    k1s = _rand64(g, count).tolist()
    return [(_w0(h, l), k) for h, l, k in zip(his, los, k1s)]


@functools.lru_cache(maxsize=None)
def _placement():
    n = 4099
    g = torch.Generator(device="cpu").manual_seed(41)
    lowest, highest = -(1 << 31), (1 << 31) - 1
    keys = [
        # 100 rows at sorted position 0
        (_w0(lowest, 9), 4), (_w0(lowest, 8), -4),
        # 60 rows from position 100 + 130 = 230: over the 256-row boundary
        (_w0(0, 1), -1), (_w0(0, 1), 1), (_w0(0, 0x80000000), 0),
        # 80 rows up to position n
        (_w0(highest, 0xFFFFFFFF), 2), (_w0(highest, 0), 3),
    ]
    counts = [50, 50, 20, 20, 20, 40, 40]
    below = _fillers(g, 130, -1_000_000, -1000)
    above = _fillers(g, n - sum(counts) - 130, 1000, 3_000_000)
    keys += below + above
    counts += [1] * (len(below) + len(above))
    k0, k1 = _rows_from_counts(keys, counts, g)
    assert k0.shape[0] == n
    case = _Case(k0, k1, g)
    assert _tied_runs(k0, k1) == [(0, 100), (230, 60), (n - 80, 80)]
    return case


@gpu
@requires_cuda
def test_run_placement():
    _run(_placement(), expect="prefix")


def _runs_case(run_rows, n, seed):
    """One tied run per entry of run_rows (two keys of one prefix, the
    rows split between them), the rest of the n rows distinct fillers."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    keys, counts = [], []
    for j, rows in enumerate(run_rows):
        hi = -5000 + 17 * j
        keys += [(_w0(hi, 0xF0000000), j), (_w0(hi, 7), -j)]
        counts += [rows // 2, rows - rows // 2]
    fill = _fillers(g, n - sum(counts), 1000, 3_000_000)
    keys += fill
    counts += [1] * len(fill)
    k0, k1 = _rows_from_counts(keys, counts, g)
    case = _Case(k0, k1, g)
    assert sorted(length for _, length in _tied_runs(k0, k1)) == sorted(run_rows)
    return case


@gpu
@requires_cuda
@pytest.mark.parametrize("rows,expect", [(64, "prefix"), (65, "fallback")])
def test_max_run_edge(rows, expect):
    _run(_runs_case([rows], 2049, 7), expect=expect, max_run=64)


@gpu
@requires_cuda
@pytest.mark.parametrize("runs,expect", [(4, "prefix"), (5, "fallback")])
def test_max_dirty_edge(runs, expect):
    _run(_runs_case([6] * runs, 2049, 9), expect=expect, max_dirty=4)


@gpu
@requires_cuda
def test_one_prefix_all_keys_distinct():
    n = 2049
    g = torch.Generator(device="cpu").manual_seed(13)
    k0 = _w0(-77, 0) | (torch.randperm(n, generator=g) * 2_000_003)
    case = _Case(k0, _rand64(g, n), g)
    assert _tied_runs(case.k0, case.k1) == [(0, n)]
    _run(case, expect="fallback")

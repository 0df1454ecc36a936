"""GPU tests of ops.group_combine_mixed_gpu: group_combine_gpu's result on
the int64 columns, double-double sums of the float64 columns through the
same permutation, the same bits on every sort path."""

import random

import pytest
import torch

from tests.dd_cases import check_sum, values

gpu = pytest.mark.gpu
requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


def _case(n, nkeys, seed, shared_word0=0):
    """n rows over nkeys keys; the first `shared_word0` keys share word0
    and differ in word1 only."""
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    key0 = torch.randint(-(2**62), 2**62, (nkeys,), generator=g)
    key1 = torch.randint(-(2**62), 2**62, (nkeys,), generator=g)
    key0[:shared_word0] = key0[0]
    which = torch.randint(0, nkeys, (n,), generator=g)
    which[:nkeys] = torch.arange(nkeys)  # every key present
    which = which[torch.randperm(n, generator=g)]
    keys = torch.stack([key0[which], key1[which]], dim=1)
    ints = torch.randint(-1000, 1000, (n,), generator=g)
    f1 = values(rng, n)
    f2 = values(rng, n, spikes=False)
    return which.tolist(), keys, ints, f1, f2


def _mixed(keys, ints, floats, **kw):
    from pathway_amd import ops

    return ops.group_combine_mixed_gpu(
        keys.to(DEV),
        [ints.to(DEV)],
        [torch.tensor(f, dtype=torch.float64, device=DEV) for f in floats],
        **kw,
    )


def _check_floats(which, keys, res, floats):
    uk0, uk1, first_row, _accs, f_hi, f_lo = res
    rows_of = {}
    for row, k in enumerate(which):
        rows_of.setdefault(k, []).append(row)
    first = first_row.tolist()
    assert len(first) == len(rows_of)
    for c, f in enumerate(floats):
        hi, lo = f_hi[c].tolist(), f_lo[c].tolist()
        for seg, row in enumerate(first):
            rows = rows_of[which[row]]
            assert rows[0] == row  # the key's smallest row
            assert hi[seg] == hi[seg] + lo[seg]
            check_sum(hi[seg] + lo[seg], [f[r] for r in rows], what=(c, seg))


@gpu
@requires_cuda
def test_int_part_equals_group_combine_and_floats_meet_the_bound():
    from pathway_amd import ops

    which, keys, ints, f1, f2 = _case(5000, 300, 1)
    before = dict(ops.gc_path_counts)
    res = _mixed(keys, ints, [f1, f2])
    assert ops.gc_path_counts["prefix"] == before["prefix"] + 1
    ref = ops.group_combine_gpu(keys.to(DEV), [ints.to(DEV)], bucket=False)
    for got, want in zip(res[:3], ref[:3]):
        assert torch.equal(got, want)
    assert len(res[3]) == 1 and torch.equal(res[3][0], ref[3][0])
    assert res[0].shape[0] == 300
    _check_floats(which, keys, res, [f1, f2])


@gpu
@requires_cuda
def test_every_sort_path_gives_the_same_bits():
    """50 keys share word0 in runs far longer than max_run=64, so the
    prefix path and the 64-bit sort both overflow into the two stable
    sorts; with the default max_run the prefix path holds."""
    from pathway_amd import ops

    which, keys, ints, f1, f2 = _case(5000, 300, 2, shared_word0=50)
    paths, mixed = ops.gc_path_counts, ops.gc_mixed_path_counts

    p0, m0 = dict(paths), dict(mixed)
    default = _mixed(keys, ints, [f1, f2])
    assert paths["prefix"] == p0["prefix"] + 1
    assert mixed["sorted"] == m0["sorted"] + 1

    p1, m1 = dict(paths), dict(mixed)
    full = _mixed(keys, ints, [f1, f2], full_sort=True)
    assert paths["full"] == p1["full"] + 1 and paths["prefix"] == p1["prefix"]
    assert mixed["sorted"] == m1["sorted"] + 1

    p2, m2 = dict(paths), dict(mixed)
    two = _mixed(keys, ints, [f1, f2], max_run=64)
    assert paths["fallback"] == p2["fallback"] + 1
    assert mixed["two_sorts"] == m2["two_sorts"] + 1
    assert mixed["sorted"] == m2["sorted"]

    _check_floats(which, keys, default, [f1, f2])
    for other in (full, two):
        for got, want in zip(other[:3], default[:3]):
            assert torch.equal(got, want)
        assert torch.equal(other[3][0], default[3][0])
        for c in range(2):
            assert torch.equal(other[4][c], default[4][c])
            assert torch.equal(other[5][c], default[5][c])


@gpu
@requires_cuda
@pytest.mark.parametrize("n", [2, 3])
def test_smallest_batches(n):
    for nkeys in (1, n):
        which, keys, ints, f1, f2 = _case(n, nkeys, 10 + n)
        res = _mixed(keys, ints, [f1, f2])
        assert res[0].shape[0] == nkeys
        _check_floats(which, keys, res, [f1, f2])
        sums = {}
        for k, v in zip(which, ints.tolist()):
            sums[k] = sums.get(k, 0) + v
        got = {which[r]: v for r, v in zip(res[2].tolist(), res[3][0].tolist())}
        assert got == sums

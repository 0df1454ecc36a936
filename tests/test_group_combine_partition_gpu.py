"""GPU tests of the bucket path's partition layout (k_gc_part_count, _scan,
_scatter and the in-order k_gc_bucket_agg): the rows are moved into bucket
order instead of being sorted by bucket and gathered.

The reference is a CPU one: numpy lexsort of signed (k0, k1),
np.add.reduceat with uint64 wraparound, np.minimum.reduceat of the row
index.  Every whole call is also compared array for array with the same
call under partition=False, and the taken path and layout are asserted
through ops.gc_path_counts and ops.gc_bucket_layout_counts.  All values
are integers: every comparison is exact."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

_PATHS = ("prefix", "fallback", "full", "bucket")
_LAYOUTS = ("partition", "gather")
_MIN64, _MAX64 = -(1 << 63), (1 << 63) - 1


def _tile():
    from pathway_amd import ops

    return ops.GC_PART_TILE


def _sizes():
    t = _tile()
    return [2, 3, t - 1, t, t + 1, 3 * t + 17]


_SIZE_IDS = ["2", "3", "tile-1", "tile", "tile+1", "3tile+17"]


def _rng(seed):
    return np.random.default_rng(seed)


def _rand64(rng, n):
    return rng.integers(_MIN64, _MAX64, size=n, dtype=np.int64, endpoint=True)


def _contribs(rng, n, nacc):
    """Column 0: -1 and 2; column 1: 2^63-1 and -1, so its sums wrap; the
    others: distinct random mixed-sign columns, so that a swap shows."""
    cols = []
    for a in range(nacc):
        if a == 0:
            c = np.where(rng.random(n) < 0.3, -1, 2).astype(np.int64)
        elif a == 1:
            c = np.where(rng.random(n) < 0.5, _MAX64, -1).astype(np.int64)
        else:
            c = _rand64(rng, n) | 1
            c[::7] = a
        cols.append(c)
    return cols


def _bucket_ids(k0, bits):
    top = (k0.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    return ((top ^ np.uint32(0x80000000)) >> np.uint32(32 - bits)).astype(np.int64)


def _reference(k0, k1, contribs):
    """numpy lexsort of signed (k0, k1), uint64 sums, smallest row."""
    n = k0.shape[0]
    perm = np.lexsort((k1, k0))
    s0, s1 = k0[perm], k1[perm]
    starts = np.ones(n, dtype=bool)
    starts[1:] = (s0[1:] != s0[:-1]) | (s1[1:] != s1[:-1])
    idx = np.flatnonzero(starts)
    sums = [
        np.add.reduceat(c[perm].view(np.uint64), idx).view(np.int64) for c in contribs
    ]
    first = np.minimum.reduceat(perm.astype(np.int64), idx)
    return s0[idx], s1[idx], sums, first


class _Case:
    def __init__(self, k0, k1, rng, nacc=2, contribs=None):
        self.k0, self.k1 = k0, k1
        self.n = k0.shape[0]
        self.contribs = _contribs(rng, self.n, nacc) if contribs is None else contribs
        self.ref = _reference(k0, k1, self.contribs)

    def keys_dev(self):
        return torch.from_numpy(np.stack([self.k0, self.k1], axis=1)).cuda()

    def contribs_dev(self):
        return [torch.from_numpy(c).cuda() for c in self.contribs]


def _snapshot():
    from pathway_amd import ops

    return (
        {k: ops.gc_path_counts[k] for k in _PATHS},
        dict(ops.gc_bucket_layout_counts),
    )


def _call(case, path, layout, keys_dev=None, **kw):
    """One group_combine_gpu call against the reference; `path` is the one
    path whose count must rise, `layout` the bucket layout (or None)."""
    from pathway_amd import ops

    if keys_dev is None:
        keys_dev = case.keys_dev()
    p0, l0 = _snapshot()
    uk0, uk1, first, accs = ops.group_combine_gpu(
        keys_dev, case.contribs_dev(), bucket=True, **kw
    )
    p1, l1 = _snapshot()
    assert {k: p1[k] - p0[k] for k in _PATHS} == {k: int(k == path) for k in _PATHS}
    assert {k: l1[k] - l0[k] for k in _LAYOUTS} == {
        k: int(k == layout) for k in _LAYOUTS
    }
    r0, r1, rsums, rfirst = case.ref
    got = [uk0, uk1, first] + list(accs)
    assert all(t.dtype == torch.int64 for t in got)
    got = [t.cpu().numpy() for t in got]
    assert len(accs) == len(case.contribs)
    for g, r in zip(got, [r0, r1, rfirst] + rsums):
        assert g.shape == r.shape
        assert np.array_equal(g, r)
    return got


def _run(case, path="bucket", keys_dev=None, **kw):
    """partition=True (ending on `path`) and partition=False: both equal the
    reference, and each other array for array."""
    on = _call(
        case, path, "partition" if path == "bucket" else None,
        keys_dev=keys_dev, partition=True, **kw,
    )
    off = _call(
        case, path, "gather" if path == "bucket" else None,
        keys_dev=keys_dev, partition=False, **kw,
    )
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)
    return on


def _rows(rng, t0, t1, n):
    """n rows drawn from the key table; every key at least once if n allows."""
    m = t0.shape[0]
    ids = rng.integers(0, m, size=n)
    if n >= m:
        ids[rng.permutation(n)[:m]] = np.arange(m)
    return t0[ids], t1[ids]


# ------------------------------------------------------ the partition alone --

@functools.lru_cache(maxsize=None)
def _part_case(n, nacc):
    rng = _rng(1000 + n + nacc)
    return _Case(_rand64(rng, n), _rand64(rng, n), rng, nacc=nacc)


@gpu
@requires_cuda
@pytest.mark.parametrize("nacc", [0, 1, 8])
@pytest.mark.parametrize("bits", [1, 4, 8])
@pytest.mark.parametrize("size", range(6), ids=_SIZE_IDS)
def test_partition_alone(size, bits, nacc):
    from pathway_amd import ops

    n = _sizes()[size]
    case = _part_case(n, nacc)
    bstart, pkeys, prow, paccs = ops.gc_partition_gpu(
        case.keys_dev(), case.contribs_dev(), bits
    )
    bstart = bstart.cpu().numpy()
    pkeys, prow = pkeys.cpu().numpy(), prow.cpu().numpy()
    paccs = [p.cpu().numpy() for p in paccs]
    ids = _bucket_ids(case.k0, bits)
    want = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=1 << bits))])
    assert np.array_equal(bstart, want)
    assert pkeys.shape == (n, 2) and prow.shape == (n,) and len(paccs) == nacc
    # every row exactly once
    assert np.array_equal(np.sort(prow), np.arange(n))
    # every row in its own bucket's range, with its own key and contributions:
    # sorted by row inside a bucket, both sides are the same list of tuples
    pos_bucket = np.searchsorted(bstart, np.arange(n), side="right") - 1
    assert np.array_equal(pos_bucket, ids[prow])
    assert np.array_equal(pkeys[:, 0], case.k0[prow])
    assert np.array_equal(pkeys[:, 1], case.k1[prow])
    for a in range(nacc):
        assert np.array_equal(paccs[a], case.contribs[a][prow])


# ------------------------------------------------ small and cross-tile sizes --

@functools.lru_cache(maxsize=None)
def _sized_case(n, distinct):
    rng = _rng(2000 + n + (distinct if distinct else 7))
    m = n if distinct is None else min(distinct, n)
    t0, t1 = _rand64(rng, m), _rand64(rng, m)
    k0, k1 = _rows(rng, t0, t1, n)
    return _Case(k0, k1, rng)


@gpu
@requires_cuda
@pytest.mark.parametrize("distinct", [3, 200, None], ids=["3", "200", "n"])
@pytest.mark.parametrize("size", range(6), ids=_SIZE_IDS)
def test_small_and_cross_tile_sizes(size, distinct):
    n = _sizes()[size]
    _run(_sized_case(n, distinct))


# ------------------------------------------------------ one key across tiles --

@gpu
@requires_cuda
def test_one_key_across_tiles():
    t = _tile()
    n = 4 * t
    rng = _rng(31)
    t0 = np.array([5 << 56, 5 << 56, -(7 << 55)], dtype=np.int64)
    t1 = np.array([1, -1, 9], dtype=np.int64)
    ids = rng.integers(1, 3, size=n)      # keys 1 and 2 everywhere ...
    ids[0] = 0                            # ... key 0 at row 0 ...
    ids[3 * t + 5] = 0                    # ... and again in the last tile
    ids[:t] = np.where(ids[:t] == 2, 1, ids[:t])
    ids[t - 1] = 2                        # key 2 first at the end of tile 0
    case = _Case(t0[ids], t1[ids], rng)
    got = _run(case)
    assert sorted(got[2].tolist()) == [0, 1, t - 1]
    assert got[2].tolist() == case.ref[3].tolist()


# ---------------------------------------------------------- extreme buckets --

@gpu
@requires_cuda
@pytest.mark.parametrize("bits", [1, 4, 8])
def test_extreme_buckets_only(bits):
    rng = _rng(37 + bits)
    n = _tile() + 133
    lowspan = 1 << (64 - bits)
    lo = _MIN64 + rng.integers(0, min(lowspan, 1 << 40), size=20)
    hi = _MAX64 - rng.integers(0, min(lowspan, 1 << 40), size=20)
    t0 = np.concatenate([[_MIN64, _MAX64], lo, hi]).astype(np.int64)
    t1 = _rand64(rng, t0.shape[0])
    k0, k1 = _rows(rng, t0, t1, n)
    assert sorted(set(_bucket_ids(k0, bits).tolist())) == [0, (1 << bits) - 1]
    _run(_Case(k0, k1, rng), bucket_bits=bits)


@gpu
@requires_cuda
def test_all_rows_in_one_bucket():
    rng = _rng(41)
    n = 2 * _tile() + 9
    t0 = (0x3C << 56) | rng.integers(0, 1 << 50, size=100)
    t0 = t0.astype(np.int64)
    k0, k1 = _rows(rng, t0, _rand64(rng, 100), n)
    assert len(set(_bucket_ids(k0, 8).tolist())) == 1
    _run(_Case(k0, k1, rng), max_bucket_rows=n)


# ------------------------------------------------------ contribution values --

@gpu
@requires_cuda
def test_contribution_values_nacc_8():
    rng = _rng(43)
    n = _tile() + 77
    t0, t1 = _rand64(rng, 150), _rand64(rng, 150)
    k0, k1 = _rows(rng, t0, t1, n)
    cols = _contribs(rng, n, 8)
    cols[2] = np.full(n, -1, dtype=np.int64)
    cols[3] = np.full(n, _MAX64, dtype=np.int64)
    assert len({c.tobytes() for c in cols}) == 8
    case = _Case(k0, k1, rng, contribs=cols)
    # precondition: some exact sum lies outside int64, so it wrapped
    exact = {}
    for a, b, v in zip(k0.tolist(), k1.tolist(), cols[3].tolist()):
        exact[(a, b)] = exact.get((a, b), 0) + v
    assert any(not _MIN64 <= s <= _MAX64 for s in exact.values())
    _run(case)


# ----------------------------------------------------- non-contiguous input --

@gpu
@requires_cuda
def test_strided_and_offset_input():
    case = _sized_case(_tile() + 1, 200)
    rng = _rng(47)
    keys = np.stack([case.k0, case.k1], axis=1)
    wide = np.stack([_rand64(rng, 2 * case.n), _rand64(rng, 2 * case.n)], axis=1)
    wide[::2] = keys
    every_other = torch.from_numpy(wide).cuda()[::2]
    assert every_other.stride() == (4, 1)
    _run(case, keys_dev=every_other)
    tall = torch.from_numpy(np.concatenate([wide[:3], keys])).cuda()
    tail = tall[3:]
    assert tail.stride() == (2, 1) and tail.storage_offset() == 6
    _run(case, keys_dev=tail)
    # rows 16 B apart that start 8 B off a 16-B boundary
    flat = torch.from_numpy(np.concatenate([[0], keys.reshape(-1)])).cuda()
    odd = flat[1:].view(-1, 2)
    assert odd.data_ptr() % 16 == 8
    _run(case, keys_dev=odd)


# ----------------------------------------------------------- overflow edges --

@functools.lru_cache(maxsize=None)
def _one_bucket(distinct, n):
    rng = _rng(19 + distinct)
    low = rng.permutation(1 << 20)[:distinct].astype(np.int64) * 0x3FFFFFFFF7 + 11
    top = np.int64((0xC4 ^ 0x80) << 56)  # bucket 0xC4 of 256
    t0 = top | (low & ((1 << 56) - 1))
    k0, k1 = _rows(rng, t0, _rand64(rng, distinct), n)
    assert set(_bucket_ids(k0, 8).tolist()) == {0xC4}
    return _Case(k0, k1, rng)


@gpu
@requires_cuda
@pytest.mark.parametrize("distinct,path", [(32, "bucket"), (33, "prefix")])
def test_capacity_edge(distinct, path):
    from pathway_amd import ops

    assert int(ops.GC_BUCKET_MAX_LOAD * 64) == 32
    _run(_one_bucket(distinct, 2049), path=path, table_capacity=64)


@gpu
@requires_cuda
@pytest.mark.parametrize("n,path", [(1000, "bucket"), (1001, "prefix")])
def test_max_bucket_rows_edge(n, path):
    _run(_one_bucket(20, n), path=path, max_bucket_rows=1000)


# ------------------------------------------------------------ repeatability --

@gpu
@requires_cuda
def test_repeatable():
    case = _sized_case(3 * _tile() + 17, 200)
    keys_dev = case.keys_dev()
    a = _call(case, "bucket", "partition", keys_dev=keys_dev, partition=True)
    b = _call(case, "bucket", "partition", keys_dev=keys_dev, partition=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---------------------------------------------------- defaults and switches --

@gpu
@requires_cuda
def test_default_layout_and_wide_buckets():
    case = _sized_case(_tile() + 1, 200)
    _call(case, "bucket", "partition")
    # more than 8 bucket bits keep the sort-and-gather layout
    _call(case, "bucket", "gather", bucket_bits=10, partition=True)


_CHILD = """
import torch
from pathway_amd import ops
g = torch.Generator().manual_seed(5)
keys = torch.randint(-(1 << 62), 1 << 62, (5000, 2), generator=g)
keys[:, 0] = keys[torch.randint(0, 50, (5000,), generator=g), 0]
ops.group_combine_gpu(keys.cuda(), [torch.ones(5000, dtype=torch.int64).cuda()],
                      bucket=True)
print("LAYOUT", ops.gc_path_counts["bucket"], ops.gc_bucket_layout_counts)
"""


@gpu
@requires_cuda
def test_environment_switch():
    env = dict(os.environ, PW_NO_GC_PARTITION="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, "-c", _CHILD], env=env, cwd=root,
        capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("LAYOUT")][-1]
    assert line == "LAYOUT 1 {'partition': 0, 'gather': 1}"

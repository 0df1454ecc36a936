"""Device interning on the GPU: the k_ht_intern_* kernels against a python
first-occurrence oracle on raw 128-bit keys, then DeviceDictionary and the
plaintext reader on cuda:0 against the host StringPool."""

from __future__ import annotations

import pytest
import torch

from pathway_amd.engine.column import StringPool
from tests.device_dict_cases import (
    PLAINTEXT_OK,
    assert_pool_equal,
    oracle_codes,
    read_rows,
    spans_of,
    write_files,
)

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU"),
]

DEV = "cuda:0"
PW_BLOCK = 256  # threads per block of the kernels (pw_kernels.hip)
SIZES = [1, 63, 64, 65, PW_BLOCK - 1, PW_BLOCK + 1, 4097]
CAP = 1 << 15  # dictionary array capacity of the raw harness


class RawDict:
    """ops.DeviceHashTable.intern on raw keys, starting from the 16-slot
    minimum table, next to the python oracle of the same key sequence.
    `front_keys` are known beforehand (codes 0, 1, ...) and live in a
    read-only front table only."""

    def __init__(self, front_keys=()):
        from pathway_amd import ops

        empty = torch.empty(0, dtype=torch.int64, device=DEV)
        self.table = ops.DeviceHashTable(empty, empty)
        assert self.table.nslots == 16
        self.pool_lo = torch.zeros(CAP, dtype=torch.int64, device=DEV)
        self.pool_hi = torch.zeros(CAP, dtype=torch.int64, device=DEV)
        self.oracle: dict[tuple[int, int], int] = {}
        self.rebuilds = 0
        self.front, self.nfront = None, len(front_keys)
        if front_keys:
            self.oracle = {k: i for i, k in enumerate(front_keys)}
            assert len(self.oracle) == self.nfront
            self.pool_lo[: self.nfront] = torch.tensor([k[0] for k in front_keys])
            self.pool_hi[: self.nfront] = torch.tensor([k[1] for k in front_keys])
            self.front = ops.DeviceHashTable(
                self.pool_lo[: self.nfront], self.pool_hi[: self.nfront]
            )

    def intern(self, keys: list[tuple[int, int]]) -> torch.Tensor:
        size, n, nf = len(self.oracle), len(keys), self.nfront
        if not self.table.fits(size - nf + n):
            self.table.rebuild(
                size - nf + n, self.pool_lo[nf:size], self.pool_hi[nf:size]
            )
            if nf:  # rebuild numbers the keys from 0: shift past the front's
                tv = self.table.tab_val
                tv[tv >= 0] += nf
            self.rebuilds += 1
        want, first_rows = [], []
        for i, k in enumerate(keys):
            if k not in self.oracle:
                self.oracle[k] = len(self.oracle)
                first_rows.append(i)
            want.append(self.oracle[k])
        lo = torch.tensor([k[0] for k in keys], dtype=torch.int64, device=DEV)
        hi = torch.tensor([k[1] for k in keys], dtype=torch.int64, device=DEV)
        codes, rows, n_new = self.table.intern(
            lo, hi, size, self.pool_lo, self.pool_hi, front=self.front
        )
        self.table.check_error()
        assert codes.shape == (n,) and codes.dtype == torch.int64
        assert int(n_new) == len(first_rows)
        assert codes.tolist() == want
        assert rows[: len(first_rows)].tolist() == first_rows
        self.check_table()
        return codes

    def check_table(self) -> None:
        """probe() agrees with every code handed out, unknown keys miss,
        the dictionary arrays hold the keys by code, no key sits in two
        slots and no slot is left pending."""
        keys = list(self.oracle)
        size = len(keys)
        lo = torch.tensor([k[0] for k in keys] + [77, -1], dtype=torch.int64, device=DEV)
        hi = torch.tensor([k[1] for k in keys] + [-77, -9], dtype=torch.int64, device=DEV)
        nf = self.nfront
        vals, found = self.table.probe(lo, hi)
        assert vals.tolist() == [-1] * nf + list(range(nf, size)) + [-1, -1]
        assert found.tolist() == [False] * nf + [True] * (size - nf) + [False, False]
        if nf:  # the front table is never written
            fvals, _ = self.front.probe(lo, hi)
            assert fvals.tolist() == list(range(nf)) + [-1] * (size - nf + 2)
        assert self.pool_lo[:size].tolist() == [k[0] for k in keys]
        assert self.pool_hi[:size].tolist() == [k[1] for k in keys]
        tv = self.table.tab_val
        used = tv != -1
        assert int((tv < -1).sum()) == 0
        assert int(used.sum()) == size - nf
        assert sorted(tv[used].tolist()) == list(range(nf, size))
        slot_keys = set(zip(self.table.tab_lo[used].tolist(),
                            self.table.tab_hi[used].tolist()))
        assert slot_keys == set(keys[nf:])


def raw_sequence(n: int) -> list[list[tuple[int, int]]]:
    distinct = [(1000 + 3 * i, 7) for i in range(n)]
    return [
        [(42, 42)] * n,  # one key: maximum contention inside a wave
        distinct,
        [(5, i) for i in range(n)],  # equal lo, different hi: one home slot
        [(-1, i) for i in range(n)],  # home is the last slot: probing wraps
        # half known, half new, interleaved, the new ones twice each
        [distinct[i] if i % 2 else (2_000_000 + i // 4, 3) for i in range(n)],
        [],
        [(42, 42)] + distinct[: n // 2] + [(-1, n), (-1, n)],
    ]


@pytest.mark.parametrize("n", SIZES)
def test_intern_kernels_match_first_occurrence_oracle(n):
    d = RawDict()
    for keys in raw_sequence(n):
        d.intern(keys)
    if n >= 63:  # the 16-slot table was outgrown several times
        assert d.rebuilds >= 3


@pytest.mark.parametrize("n", [65, 4097])
def test_intern_kernels_with_front_table(n):
    """Keys of a read-only front table keep their codes and stay out of
    the open table; everything else is interned past them."""
    seq = raw_sequence(n)
    d = RawDict(front_keys=seq[1][: n // 2] + [(42, 42), (-1, 0), (5, 1)])
    for keys in seq:
        d.intern(keys)


def test_intern_is_deterministic():
    runs = []
    for _ in range(2):
        d = RawDict()
        runs.append([d.intern(keys) for keys in raw_sequence(4097)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _lines(n: int) -> list[str]:
    """n lines over about n/3 distinct words, with empty lines, duplicates
    and non-ASCII words."""
    words = []
    for i in range(n):
        j = (i * 7919) % (n // 3)
        words.append("" if j % 50 == 0 else f"w{j}é" if j % 11 == 0 else f"word{j}")
    return words


@pytest.mark.parametrize("drain_every", [None, 4])
def test_dictionary_growth_many_small_batches(drain_every):
    """315 distinct tokens arrive 40 rows at a time: the open table (sized
    for two batches) fills and is folded into the front table again and
    again, with and without host drains in between."""
    batches = [[f"t{(i * 31 + b * 17) % (13 * (b + 1))}" for i in range(40)]
               for b in range(30)]
    want, oracle = oracle_codes(batches)
    pool = StringPool()
    d = pool.device_dictionary(DEV)
    assert d.native and d.table.nslots == 16 and d.front.nslots == 16
    sizes = set()
    for i, (b, w) in enumerate(zip(batches, want)):
        assert d.intern_spans(*spans_of(b, DEV)).tolist() == w
        sizes.add(d.front.nslots)
        if drain_every and i % drain_every == drain_every - 1:
            assert len(pool) > max(w)  # drains
    assert len(sizes) >= 3
    assert d.table.fits(2 * 40)
    d.sync_host()
    assert_pool_equal(pool, oracle)
    lo, hi = pool.hash_tensors(DEV)
    n = len(oracle._strs)
    assert d.encode(lo[:n], hi[:n]).tolist() == list(range(n))


def test_intern_spans_end_to_end_and_buffer_reuse():
    lines = _lines(5000)
    batches = [lines[:1700], lines[1700:3400], lines[3400:]]
    want, oracle = oracle_codes(batches)
    pool = StringPool()
    d = pool.device_dictionary(DEV)
    for b, w in zip(batches, want):
        buf, starts, ends = spans_of(b, DEV)
        codes = d.intern_spans(buf, starts, ends)
        buf.zero_()  # the caller's staging buffer is reused right away
        assert codes.tolist() == w
    assert pool._strs == []  # the host pool has not been touched yet
    lo, hi = pool.hash_tensors(DEV)
    n = len(oracle._strs)
    assert lo.shape[0] >= n
    # closed-world probe of tokens that only the open table holds so far
    assert d.encode(lo[:n], hi[:n]).tolist() == list(range(n))
    d.sync_host()
    assert_pool_equal(pool, oracle)
    assert lo[:n].tolist() == oracle._hash_lo and hi[:n].tolist() == oracle._hash_hi


def test_host_strings_between_device_batches():
    batches = [["b", "a", "b", ""], ["x"], ["x", "h", "a", "ż"]]
    want, oracle = oracle_codes(batches)
    pool = StringPool()
    d = pool.device_dictionary(DEV)
    assert d.intern_spans(*spans_of(batches[0], DEV)).tolist() == want[0]
    assert pool.code("x") == want[1][0]
    assert d.intern_spans(*spans_of(batches[2], DEV)).tolist() == want[2]
    assert len(pool) == len(oracle)
    assert_pool_equal(pool, oracle)
    lo, hi = pool.hash_tensors(DEV)
    assert d.encode(lo[: len(pool)], hi[: len(pool)]).tolist() == list(range(len(pool)))


@pytest.mark.parametrize("case", sorted(PLAINTEXT_OK))
def test_plaintext_device_equals_host_on_gpu(case, tmp_path, monkeypatch):
    monkeypatch.setenv("PW_DEVICE", DEV)
    path = write_files(tmp_path, PLAINTEXT_OK[case])
    host = read_rows(path, "host", monkeypatch)
    assert read_rows(path, "device", monkeypatch) == host

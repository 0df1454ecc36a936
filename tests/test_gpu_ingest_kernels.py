"""Ingest kernels on the GPU: the register-only token hash
(k_varlen_hash_se / k_varlen_hash), the one-array hash table
(k_ht_build / k_ht_probe) and the newline scan (scan_positions_gpu) at
its block-count boundaries."""

from __future__ import annotations

import functools
import random

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

# ------------------------------------------------------------------ hash --

LENGTHS = (0, 1, 3, 4, 7, 8, 9, 15, 16, 23, 24, 25, 31, 32, 55, 56, 57, 63,
           64, 88, 121, 300)
N_TOKENS = 4097
HASH_NS = (0, 1, 255, 256, 257, 4097)


@functools.lru_cache(maxsize=None)
def _tokens():
    """4097 ASCII tokens whose lengths cycle through LENGTHS in a shuffled
    order (two zero lengths side by side: consecutive newlines), with
    their expected 128-bit hashes (hash128(serialize_value(w)))."""
    from pathway_amd.internals.api import hash128, serialize_value

    rnd = random.Random(11)
    lens = []
    while len(lens) < N_TOKENS:
        block = list(LENGTHS) + [0]
        rnd.shuffle(block)
        lens.extend(block)
    lens = lens[:N_TOKENS]
    lens[5] = lens[6] = 0  # consecutive empty tokens
    alphabet = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    words = ["".join(rnd.choice(alphabet) for _ in range(n)) for n in lens]
    want = [hash128(serialize_value(w)) for w in words]
    return words, want


def _signed(x: int) -> int:
    return x - (1 << 64) if x >= (1 << 63) else x


def _expected(n: int):
    _, want = _tokens()
    lo = torch.tensor([_signed(a) for a, _ in want[:n]], dtype=torch.int64)
    hi = torch.tensor([_signed(b) for _, b in want[:n]], dtype=torch.int64)
    return lo, hi


def _wire_se(n: int):
    """newline-joined wire of the first n tokens, no trailing newline, so
    the last token ends on the buffer's final byte"""
    words, _ = _tokens()
    wire = "\n".join(words[:n]).encode()
    starts, ends, pos = [], [], 0
    for w in words[:n]:
        starts.append(pos)
        ends.append(pos + len(w))
        pos += len(w) + 1
    return wire, starts, ends


def test_token_starts_cover_every_residue():
    """the mix puts token starts on every residue mod 8, for every length"""
    words, _ = _tokens()
    _, starts, _ = _wire_se(N_TOKENS)
    seen = {(len(w), s % 8) for w, s in zip(words, starts)}
    for n in LENGTHS:
        assert {r for (m, r) in seen if m == n} == set(range(8)), n
    assert len(words[5]) == 0 and len(words[6]) == 0


def _dev_bytes(data: bytes, shift: int) -> torch.Tensor:
    """data on the device, as a view `shift` bytes into a larger buffer"""
    host = np.frombuffer(b"#" * shift + data, dtype=np.uint8).copy()
    return torch.from_numpy(host).cuda()[shift:]


@gpu
@requires_cuda
@pytest.mark.parametrize("shift", (0, 1, 2, 3))
def test_varlen_hash_se(shift):
    from pathway_amd import ops
    from pathway_amd.internals.api import TAG_STR

    for n in HASH_NS:
        wire, starts, ends = _wire_se(n)
        buf = _dev_bytes(wire, shift)
        assert buf.numel() == (ends[-1] if n else 0)
        st = torch.tensor(starts, dtype=torch.int64, device="cuda")
        en = torch.tensor(ends, dtype=torch.int64, device="cuda")
        lo, hi = ops.varlen_hash_se_gpu(buf, st, en, TAG_STR)
        want_lo, want_hi = _expected(n)
        assert torch.equal(lo.cpu(), want_lo), (shift, n)
        assert torch.equal(hi.cpu(), want_hi), (shift, n)


@gpu
@requires_cuda
@pytest.mark.parametrize("shift", (0, 1, 2, 3))
def test_varlen_hash_offsets(shift):
    from pathway_amd import ops
    from pathway_amd.internals.api import TAG_STR

    words, _ = _tokens()
    for n in HASH_NS:
        data = "".join(words[:n]).encode()
        offs = [0]
        for w in words[:n]:
            offs.append(offs[-1] + len(w))
        buf = _dev_bytes(data, shift)
        assert buf.numel() == offs[-1]
        off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        lo, hi = ops.varlen_hash_gpu(buf, off, TAG_STR)
        want_lo, want_hi = _expected(n)
        assert torch.equal(lo.cpu(), want_lo), (shift, n)
        assert torch.equal(hi.cpu(), want_hi), (shift, n)


# ----------------------------------------------------------------- probe --

NQ = 4097


def _keys(m: int):
    """m distinct 128-bit keys; every 4th shares its home slot (low bits of
    lo) with the key before it, so one of the two is displaced"""
    from pathway_amd import ops

    g = torch.Generator().manual_seed(100 + m)
    nslots = ops.DeviceHashTable.slots_for(m)
    klo = torch.randperm(1 << 22, generator=g)[:m] * 7919 + 13
    khi = torch.randint(-(1 << 62), 1 << 62, (m,), generator=g)
    idx = torch.arange(3, max(m, 3), 4)
    klo[idx] = klo[idx - 1] + nslots * (1 + idx)
    vals = torch.randint(0, 1 << 40, (m,), generator=g)
    if m >= 4:
        mask = nslots - 1
        pairs = set(zip(klo.tolist(), khi.tolist()))
        assert len(pairs) == m  # distinct keys
        homes = (klo & mask).unique().numel()
        assert m - homes >= m // 4  # at least that many keys are displaced
    return klo.cuda(), khi.cuda(), vals.cuda(), nslots


def _check_table(ht, klo, khi, vals, m):
    """hits (with repeats, some through a chain), both kinds of misses"""
    mask = ht.nslots - 1
    assert ht.tab_lo.shape == ht.tab_hi.shape == ht.tab_val.shape == (ht.nslots,)
    assert ht.tab_lo.dtype == ht.tab_hi.dtype == ht.tab_val.dtype == torch.int64
    tab_lo, tab_hi, tab_val = ht.tab_lo.cpu(), ht.tab_hi.cpu(), ht.tab_val.cpu()
    assert int((tab_val >= 0).sum()) == m
    g = torch.Generator().manual_seed(7 + m)
    if m:
        qi = torch.randint(0, m, (NQ,), generator=g).cuda()
        qlo, qhi = klo[qi], khi[qi]
        got, found = ht.probe(qlo, qhi)
        assert bool(found.all())
        assert torch.equal(got, vals[qi])
        if m >= 1000:
            home = (qlo & mask).cpu()
            other = (tab_lo[home] != qlo.cpu()) | (tab_hi[home] != qhi.cpu())
            assert int(other.sum()) > 0  # hits whose home holds another key
        # misses whose home slot is occupied: a stored lo with another hi
        got, found = ht.probe(qlo, qhi + 1)
        assert not bool(found.any()) and bool((got == -1).all())
        assert bool((tab_val[(qlo & mask).cpu()] >= 0).all())
    # misses whose home slot is empty
    empty = (tab_val == -1).nonzero(as_tuple=True)[0]
    pick = empty[torch.randint(0, empty.numel(), (NQ,), generator=g)]
    mlo = (pick + ht.nslots * 5).cuda()
    mhi = torch.randint(-(1 << 62), 1 << 62, (NQ,), generator=g).cuda()
    got, found = ht.probe(mlo, mhi)
    assert not bool(found.any()) and bool((got == -1).all())


@gpu
@requires_cuda
@pytest.mark.parametrize("m", (0, 1, 1000, 50_000))
def test_hash_table_probe(m):
    from pathway_amd import ops

    klo, khi, vals, nslots = _keys(m)
    ht = ops.DeviceHashTable(klo, khi, vals)
    assert ht.nslots == nslots
    _check_table(ht, klo, khi, vals, m)

    # filled by two insert calls
    h = m // 2
    ht2 = ops.DeviceHashTable(klo[:h], khi[:h], vals[:h], reserve=m)
    ht2.insert(klo[h:], khi[h:], vals[h:])
    assert ht2.nslots == nslots
    _check_table(ht2, klo, khi, vals, m)

    # rebuilt for twice the size: values are the row indices
    ht2.rebuild(2 * m, klo, khi)
    assert ht2.nslots == ops.DeviceHashTable.slots_for(2 * m)
    _check_table(ht2, klo, khi, torch.arange(m, device="cuda"), m)

    # in-place updates through the column views reach the table
    tv = ht.tab_val
    tv[tv >= 0] += 17
    _check_table(ht, klo, khi, vals + 17, m)
    ht.tab_val.fill_(-1)
    if m:
        got, found = ht.probe(klo[:NQ], khi[:NQ])
        assert not bool(found.any()) and bool((got == -1).all())
    _check_table(ht, klo[:0], khi[:0], vals[:0], 0)


# ------------------------------------------------------------------ scan --

SCAN_NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 2048 * 4096 + 4097)


@gpu
@requires_cuda
def test_scan_positions_sizes():
    from pathway_amd import ops

    g = torch.Generator(device="cuda").manual_seed(3)
    for n in SCAN_NS:
        buf = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda",
                            generator=g)
        if n:
            buf[n - 1] = 10  # a match on the final byte
        got = ops.scan_positions_gpu(buf, 10)
        ref = (buf == 10).nonzero(as_tuple=True)[0]
        assert got.dtype == torch.int64 and torch.equal(got, ref), n


@gpu
@requires_cuda
def test_scan_positions_all_none_sliced():
    from pathway_amd import ops

    for n in (17, 4097, 3 * 4096 + 5):
        full = torch.full((n,), 10, dtype=torch.uint8, device="cuda")
        assert torch.equal(ops.scan_positions_gpu(full, 10),
                           torch.arange(n, device="cuda"))
        none = torch.full((n,), 65, dtype=torch.uint8, device="cuda")
        got = ops.scan_positions_gpu(none, 10)
        assert got.shape == (0,) and got.dtype == torch.int64
    g = torch.Generator(device="cuda").manual_seed(4)
    buf = torch.randint(0, 16, (100_003,), dtype=torch.uint8, device="cuda",
                        generator=g)
    for k in (1, 2, 3, 16):
        sub = buf[k:]
        ref = (sub == 10).nonzero(as_tuple=True)[0]
        assert torch.equal(ops.scan_positions_gpu(sub, 10), ref), k

"""Inputs and oracles for the device tests of the arrange-path primitives
(tests/test_arrange_prims_gpu.py): hash128_words / value_hash,
merge_consolidate, partition, radix_sort64 and the fused gather.  Checked on
the CPU by tests/test_arrange_cases_cpu.py.  Nothing here touches a GPU.

Rows are tuples of signed Python ints, one per 64-bit word, ordered as
Python orders tuples: lexicographically and signed.  Sums are Python ints
reduced modulo 2^64 and read as signed.  Every comparison the tests make is
exact.

Sizes follow the launch geometry in ops/csrc/hip/pw_kernels.hip and the
wrappers in ops/__init__.py; the CPU test holds each against its source:

  hash, value hash   grid-stride, at most MAX_GRID blocks of BLOCK threads;
                     GRID_TRIP rows take a second trip
  merge-consolidate  MC_CHUNK diagonals per thread, BLOCK threads per block
  partition          at most PART_MAX_BLOCKS blocks, each a contiguous chunk
                     walked BLOCK rows at a time; at GRID_TRIP the chunk is
                     longer than BLOCK.  At most PART_MAX_DEST destinations
  radix sort         blocks of one wave (RS_LANES); RS_BLOCK_ROWS rows per
                     block until RS_MAX_BLOCKS blocks, then longer chunks
  gather             grid-stride, at most GATHER_MAX_GRID blocks of BLOCK;
                     GATHER_COLS columns per launch
"""

from __future__ import annotations

import random
import struct

import torch

from pathway_amd.internals import api
from tests.state_prims_cases import (  # noqa: F401  (re-exported for the tests)
    BLOCK,
    GRID_TRIP,
    INT64_MAX,
    INT64_MIN,
    MAX_GRID,
    SPECIALS,
    columns,
    wrap64,
)

MASK64 = (1 << 64) - 1


def unsigned(row: tuple) -> tuple:
    """The row as an unsigned comparison would read it."""
    return tuple(v & MASK64 for v in row)


def full_range(shape, seed: int) -> torch.Tensor:
    """Random int64 over all of int64 (INT64_MAX itself excepted)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(INT64_MIN, INT64_MAX, shape, generator=g)


# -------------------------------------------------------------- row hashes --

HASH_MAX_WORDS = 20
HASH_W = tuple(range(1, HASH_MAX_WORDS + 1))
#: widths with an empty tail after the 4-word stripes
HASH_W_NO_TAIL = (8, 12, 16, 20)
HASH_SMALL_N = 257
HASH_GRID_W = (1, 4, 20)
HASH_SIZES = (0, 1, 255, 256, 257)


def hash_rows(W: int) -> list[tuple]:
    """HASH_SMALL_N rows of W words: each of SPECIALS in every word position
    (the other words small and distinct), the all-zero row, the row of all
    one bits, the row of ones, and full-range random rows."""
    rnd = random.Random(1000 + W)
    rows = []
    for p in range(W):
        for v in SPECIALS:
            rows.append(tuple(v if j == p else j + 2 for j in range(W)))
    rows += [(0,) * W, (-1,) * W, (1,) * W]
    while len(rows) < HASH_SMALL_N:
        rows.append(tuple(rnd.randrange(INT64_MIN, INT64_MAX + 1) for _ in range(W)))
    return rows


def py_hash128(row: tuple) -> tuple[int, int]:
    """(lo, hi) of a row of words, as signed int64: api.xxh64 over the words
    packed little-endian, at the two seeds."""
    data = b"".join(struct.pack("<q", v) for v in row)
    return (
        wrap64(api.xxh64(data, api.SEED_LO)),
        wrap64(api.xxh64(data, api.SEED_HI)),
    )


def hash_grid_words(W: int) -> list[torch.Tensor]:
    """W full-range random words of GRID_TRIP rows; the last row, which
    only the second grid trip reaches, is all INT64_MIN."""
    t = full_range((W, GRID_TRIP), 2000 + W)
    t[:, -1] = INT64_MIN
    return [t[j] for j in range(W)]


#: every tag hashing.column_value_hash hands to value_hash_words
VALUE_TAGS = (
    api.TAG_BOOL,
    api.TAG_INT,
    api.TAG_FLOAT,
    api.TAG_DT_NAIVE,
    api.TAG_DT_UTC,
    api.TAG_DURATION,
)
VALUE_N = (1, 257, GRID_TRIP)


def value_payload(n: int) -> torch.Tensor:
    """n payload words: SPECIALS first (as many as fit), then random."""
    t = full_range((n,), 3000 + n)
    k = min(n, len(SPECIALS))
    t[:k] = torch.tensor(SPECIALS[:k], dtype=torch.int64)
    return t


# ------------------------------------------------------- merge-consolidate --

MC_CHUNK = 8
MC_NW = (1, 2, 3, 4)
MC_NACC = (1, 8)
MC_TOTALS = (7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4100)

_MC_POOL = {
    1: SPECIALS + (-2, 2, -100, 100, 2**62, -(2**62), 3, -3, 7),
    2: SPECIALS + (-2, 2),
    3: SPECIALS,
    4: SPECIALS,
}


def mc_sides(nw: int) -> tuple[list[tuple], list[tuple]]:
    """(A rows, B rows), each unique and sorted.  Every row is a tuple over
    a small pool that holds SPECIALS, so rows tie in their leading words and
    every word position decides comparisons inside A, inside B and between
    them; about a third of the rows are in both sides."""
    import itertools

    rnd = random.Random(40 + nw)
    a, b = [], []
    for r in sorted(itertools.product(_MC_POOL[nw], repeat=nw)):
        side = rnd.choice("ABX")
        if nw > 1 and all(v == INT64_MAX for v in r[1:]):
            side = "A"  # the last row under its word 0 ...
        if nw > 1 and all(v == INT64_MIN for v in r[1:]):
            side = "B"  # ... meets the first row under the next
        if len(set(r)) == 1 and r[0] in SPECIALS:
            side = "X"  # so that each side has every special in every word
        if side in "AX":
            a.append(r)
        if side in "BX":
            b.append(r)
    return a, b


_BIG = 2**62


def mc_accs(a_rows, b_rows, nacc: int, nwc: int | None = None):
    """(a_accs, b_accs): nacc lists per side.  Over the matched pairs, in
    turn: slot 0 cancels while the others do not; slot 0 survives while all
    others cancel; slot 0 crosses 2^63; plain values.  Every fifth unmatched
    row of each side has 0 in slot 0 and non-zero elsewhere."""
    nwc = nwc or (len(a_rows[0]) if a_rows else len(b_rows[0]) if b_rows else 1)
    in_a = {r[:nwc]: i for i, r in enumerate(a_rows)}
    a_accs = [[0] * len(a_rows) for _ in range(nacc)]
    b_accs = [[0] * len(b_rows) for _ in range(nacc)]
    matched_a = set()
    k = 0
    for j, r in enumerate(b_rows):
        i = in_a.get(r[:nwc])
        if i is None:
            continue
        matched_a.add(i)
        kind = k % 4
        k += 1
        for c in range(nacc):
            if kind == 0:  # slot 0 cancels, the others do not
                av, bv = (5 + j, -(5 + j)) if c == 0 else (c + 1, j + 1)
            elif kind == 1:  # slot 0 survives, every other slot cancels
                av, bv = (3, 4) if c == 0 else (-(c + j + 1), c + j + 1)
            elif kind == 2:  # the sum crosses 2^63
                av, bv = (_BIG + j + c, _BIG) if c % 2 == 0 else (-_BIG - 1 - j, -_BIG)
            else:
                av, bv = (j % 7 + 1, c - 3)
            a_accs[c][i], b_accs[c][j] = av, bv
    for rows, accs, matched in (
        (a_rows, a_accs, matched_a),
        (b_rows, b_accs, {j for j, r in enumerate(b_rows) if r[:nwc] in in_a}),
    ):
        u = 0
        for i in range(len(rows)):
            if i in matched:
                continue
            for c in range(nacc):
                if c == 0:
                    accs[c][i] = 0 if u % 5 == 0 else (u % 3) - 4
                else:
                    accs[c][i] = 11 * c + i
            u += 1
    return a_accs, b_accs


def mc_oracle(a_rows, a_accs, b_rows, b_accs, nwc: int | None = None):
    """(rows, accs, rep) of the merge: a dict from the comparison prefix to
    [words, accumulators, source row], the A row winning on a match; sums
    wrapped; rows whose slot 0 sums to 0 dropped; signed lexicographic
    order; rep indexes concat([A, B])."""
    nacc = len(a_accs)
    nw = len(a_rows[0]) if a_rows else (len(b_rows[0]) if b_rows else 0)
    nwc = nwc or nw
    m = len(a_rows)
    table: dict = {}
    for i, r in enumerate(a_rows):
        assert r[:nwc] not in table, "A must be unique in its comparison prefix"
        table[r[:nwc]] = [r, [a_accs[c][i] for c in range(nacc)], i]
    seen_b = set()
    for j, r in enumerate(b_rows):
        assert r[:nwc] not in seen_b, "B must be unique in its comparison prefix"
        seen_b.add(r[:nwc])
        e = table.get(r[:nwc])
        if e is None:
            table[r[:nwc]] = [r, [b_accs[c][j] for c in range(nacc)], m + j]
        else:
            e[1] = [wrap64(e[1][c] + b_accs[c][j]) for c in range(nacc)]
    rows, accs, rep = [], [[] for _ in range(nacc)], []
    for prefix in sorted(table):
        r, acc, src = table[prefix]
        if acc[0] == 0:
            continue
        rows.append(r)
        for c in range(nacc):
            accs[c].append(acc[c])
        rep.append(src)
    return rows, accs, rep


def mc_key_row(k: int, nw: int) -> tuple:
    """Row number k of nw words, increasing in k: the trailing words are
    the base-3 digits of k (less one), word 0 the rest, negative at first."""
    digits = []
    for _ in range(nw - 1):
        digits.append(k % 3 - 1)
        k //= 3
    return (k - 2,) + tuple(reversed(digits))


def _mc_unit_accs(a_keys, b_keys, nacc):
    """Slot 0 is +1 in A and, in B, -1 on every third key (which cancels a
    match) and +2 otherwise; the other slots differ per row."""
    a = [[1 if c == 0 else c * 100 + k for k in a_keys] for c in range(nacc)]
    b = [
        [(-1 if k % 3 == 0 else 2) if c == 0 else -c * 7 - k for k in b_keys]
        for c in range(nacc)
    ]
    return a, b


MC_SHAPES = (
    "empty",
    "only_b",
    "only_a",
    "one_matched",
    "one_unmatched",
    "a_below_b",
    "a_above_b",
    "interleave",
    "identical_1030",
) + tuple(f"total_{t}" for t in MC_TOTALS)


def mc_shape_keys(shape: str) -> tuple[list[int], list[int]]:
    """(A keys, B keys) as sorted unique row numbers for mc_key_row."""
    if shape == "empty":
        return [], []
    if shape == "only_b":
        return [], [4]
    if shape == "only_a":
        return [4], []
    if shape == "one_matched":
        return [4], [4]
    if shape == "one_unmatched":
        return [5], [4]
    if shape == "a_below_b":
        return list(range(0, 21)), list(range(21, 40))
    if shape == "a_above_b":
        return list(range(21, 40)), list(range(0, 21))
    if shape == "interleave":
        return list(range(0, 40, 2)), list(range(1, 40, 2))
    if shape == "identical_1030":
        return list(range(1030)), list(range(1030))
    total = int(shape.split("_")[1])
    rnd = random.Random(total)
    m = total // 2 + (total % 3)
    n = total - m
    return sorted(rnd.sample(range(total), m)), sorted(rnd.sample(range(total), n))


def mc_shape_case(shape: str, nw: int, nacc: int):
    a_keys, b_keys = mc_shape_keys(shape)
    a_accs, b_accs = _mc_unit_accs(a_keys, b_keys, nacc)
    return (
        [mc_key_row(k, nw) for k in a_keys],
        a_accs,
        [mc_key_row(k, nw) for k in b_keys],
        b_accs,
    )


def mc_tail_function_case():
    """4-word sides whose words 2 and 3 are a function of words 0 and 1, so
    comparing 2 words or 4 gives the same merge."""
    a2, b2 = mc_sides(2)

    def full(r):
        return r + (wrap64(r[0] * 0x9E3779B97F4A7C15 + r[1]), r[0] ^ r[1])

    return [full(r) for r in a2], [full(r) for r in b2]


def mc_tail_differs_case():
    """4-word sides, each sorted and unique over all 4 words and over the
    first 2, where the B row (1, 2, ...) shares A's first two words and
    carries another tail: comparing 2 words merges the two (A's tail is
    kept), comparing 4 keeps both."""
    a_rows = [(-5, 0, 1, 1), (1, 2, 10, 11), (1, 3, 0, 0), (INT64_MAX, -1, 4, 4)]
    b_rows = [(INT64_MIN, 7, 2, 2), (1, 2, 99, -98), (1, 4, 0, 0), (2, 0, -3, 3)]
    a_accs = [[1, 2, 3, 4], [10, 20, 30, 40]]
    b_accs = [[5, 6, 7, 8], [50, 60, 70, 80]]
    return a_rows, a_accs, b_rows, b_accs


# --------------------------------------------------------------- partition --

PART_MAX_DEST = 64
PART_MAX_BLOCKS = 2048
PART_WORLDS = (1, 2, 63, 64)
PART_N = (0, 1, 255, 256, 257, PART_MAX_BLOCKS * BLOCK + 257)
PART_PATTERNS = (
    "all_first",
    "all_last",
    "one_unused",
    "round_robin",
    "ascending",
    "descending",
)


def partition_dest(pattern: str, n: int, world: int) -> torch.Tensor:
    """n destinations in [0, world)."""
    i = torch.arange(n, dtype=torch.int64)
    if pattern == "all_first":
        return torch.zeros(n, dtype=torch.int64)
    if pattern == "all_last":
        return torch.full((n,), world - 1, dtype=torch.int64)
    if pattern == "one_unused":
        # round-robin over every destination but world // 2
        if world == 1:
            return torch.zeros(n, dtype=torch.int64)
        d = i % (world - 1)
        return d + (d >= world // 2).to(torch.int64)
    if pattern == "round_robin":
        return i % world
    if pattern == "ascending":
        return (i * world) // max(n, 1)
    if pattern == "descending":
        return ((i * world) // max(n, 1)).flip(0)
    raise ValueError(pattern)


def check_partition(dest: torch.Tensor, world: int, perm: torch.Tensor, counts: torch.Tensor):
    """What partition_gpu promises; the order inside a destination is free."""
    n = dest.shape[0]
    assert perm.dtype == torch.int64 and counts.dtype == torch.int64
    assert perm.shape == (n,) and counts.shape == (world,)
    assert torch.equal(counts, torch.bincount(dest, minlength=world)), "counts"
    assert torch.equal(torch.sort(perm).values, torch.arange(n)), "perm is no permutation"
    grouped = dest.index_select(0, perm)
    assert bool((grouped[1:] >= grouped[:-1]).all()), "rows not grouped by destination"


# -------------------------------------------------------------- radix sort --

RS_LANES = 64
RS_BLOCK_ROWS = 64 * 64
RS_MAX_BLOCKS = 1024
RS_N = (2, 63, 64, 65, 4095, 4096, 4097, 8193)
RS_N_CAP = RS_BLOCK_ROWS * RS_MAX_BLOCKS + 1
RS_KEY_SETS = (
    ("specials", "all_equal", "sorted", "reversed", "random")
    + tuple(f"pass_{p}" for p in range(8))
)


def radix_keys(name: str, n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(500 + n)
    if name == "specials":
        # each of SPECIALS over and over, shuffled
        t = torch.tensor(SPECIALS, dtype=torch.int64)[torch.arange(n) % len(SPECIALS)]
        return t[torch.randperm(n, generator=g)]
    if name == "all_equal":
        return torch.full((n,), -7, dtype=torch.int64)
    if name in ("sorted", "reversed", "random"):
        t = full_range((n,), 600 + n)
        t[0], t[n - 1] = INT64_MAX, INT64_MIN
        if n >= 8:  # one key comes twice
            t[n // 2] = t[n // 3]
        if name == "random":
            return t
        t = torch.sort(t).values
        return t if name == "sorted" else t.flip(0)
    if name.startswith("pass_"):
        # only the digit of pass p differs: d << 8p, every d with duplicates
        p = int(name.split("_")[1])
        d = torch.arange(n, dtype=torch.int64) % 256
        d = d[torch.randperm(n, generator=g)]
        return d << (8 * p)  # p = 7 shifts into the sign bit
    raise ValueError(name)


def radix_cap_keys() -> torch.Tensor:
    """RS_N_CAP keys: full-range random, every key of the first half once
    more in the second, INT64_MIN and INT64_MAX among them, shuffled."""
    n = RS_N_CAP
    t = full_range((n,), 77)
    t[n // 2 : 2 * (n // 2)] = t[: n // 2]
    t[0], t[1] = INT64_MIN, INT64_MAX
    g = torch.Generator().manual_seed(78)
    return t[torch.randperm(n, generator=g)]


# ------------------------------------------------------------------ gather --

GATHER_COLS = 8
GATHER_MAX_GRID = 4096
GATHER_TRIP = GATHER_MAX_GRID * BLOCK + 257
GATHER_SRC_N = 1000
GATHER_NCOLS = (1, 8, 9, 16)
GATHER_M = (0, 1, 255, 256, 257)
#: gather_all goes through the fused kernel above this many index rows
GATHER_ALL_SWITCH = 2048

#: float64 bit patterns that must come through untouched: quiet and
#: signalling NaNs with payloads, of both signs; -0.0; infinities; the
#: smallest denormal
_FLOAT_BITS = (
    0x7FF8000000000000,
    0x7FF8000000000001,
    0x7FF0000000000001,
    0xFFF8DEADBEEF0001,
    0xFFF0000000000002,
    0x8000000000000000,
    0x0000000000000000,
    0x7FF0000000000000,
    0xFFF0000000000000,
    0x0000000000000001,
)


def gather_int_col(n: int, seed: int) -> torch.Tensor:
    t = full_range((n,), 700 + seed)
    k = min(n, len(SPECIALS))
    t[:k] = torch.tensor(SPECIALS[:k], dtype=torch.int64)
    return t


def gather_float_col(n: int, seed: int) -> torch.Tensor:
    """float64 whose first rows are _FLOAT_BITS, the rest random bits."""
    bits = full_range((n,), 800 + seed)
    k = min(n, len(_FLOAT_BITS))
    bits[:k] = torch.tensor([wrap64(b) for b in _FLOAT_BITS[:k]], dtype=torch.int64)
    return bits.view(torch.float64)


def gather_fused_cols(ncols: int, n: int = GATHER_SRC_N) -> list[torch.Tensor]:
    """ncols contiguous 8-byte columns, int64 and float64 in turn."""
    return [
        gather_int_col(n, c) if c % 2 == 0 else gather_float_col(n, c)
        for c in range(ncols)
    ]


def gather_mixed_cols(n: int = GATHER_SRC_N) -> list[torch.Tensor]:
    """Fused columns with, between them, columns the kernel cannot take:
    int32, bool, 2-D (n, 2) and a strided 8-byte view."""
    strided = gather_int_col(2 * n, 21)[::2]
    assert not strided.is_contiguous()
    return [
        gather_int_col(n, 10),
        gather_int_col(n, 11).to(torch.int32),
        gather_float_col(n, 12),
        gather_int_col(n, 13) > 0,
        gather_int_col(2 * n, 14).reshape(n, 2),
        strided,
        gather_float_col(n, 15),
        gather_int_col(n, 16),
    ]


def gather_index(kind: str, m: int, n: int = GATHER_SRC_N) -> torch.Tensor:
    if kind == "random":
        g = torch.Generator().manual_seed(900 + m)
        idx = torch.randint(0, n, (m,), generator=g)
        if m >= 2:  # both ends of the source
            idx[0], idx[m - 1] = n - 1, 0
        return idx
    if kind == "all_equal":
        return torch.full((m,), n - 1, dtype=torch.int64)
    if kind == "identity":
        assert m == n
        return torch.arange(n, dtype=torch.int64)
    if kind == "reversed":
        assert m == n
        return torch.arange(n - 1, -1, -1, dtype=torch.int64)
    raise ValueError(kind)


def gather_oracle(idx: torch.Tensor, cols: list[torch.Tensor]) -> list[torch.Tensor]:
    return [c.index_select(0, idx) for c in cols]


def bits(t: torch.Tensor) -> torch.Tensor:
    """A tensor for exact comparison: float64 as its int64 bit pattern."""
    return t.view(torch.int64) if t.dtype == torch.float64 else t

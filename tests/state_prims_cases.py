"""Inputs and oracles for the device tests of the sorted-state primitives
(tests/test_state_prims_gpu.py): searchsorted / lookup / key_range,
run_starts, pool_hash, seg_reduce_words, sort_repair and hash_agg.  Checked
on the CPU by tests/test_state_prims_cpu.py.

Rows are tuples of signed Python ints, one per 64-bit word, compared as
Python compares tuples: lexicographically and signed.  The search oracle is
bisect over a list of such tuples; sums are Python ints reduced modulo 2^64
and read as signed, which is what a 64-bit atomic add computes.

Two sizes come from the launch geometry of the kernels, 2048 blocks of 256
threads at the most: GRID_TRIP = 2048 * 256 + 257 rows make a grid-stride
loop take a second trip, and 256 / 64 are the block / wave sizes at which
the segmented reduce changes path.
"""

from __future__ import annotations

import bisect
import random

import torch

INT64_MIN = -(2**63)
INT64_MAX = 2**63 - 1
SPECIALS = (INT64_MIN, -1, 0, 1, INT64_MAX)

BLOCK = 256
WAVE = 64
MAX_GRID = 2048
GRID_TRIP = MAX_GRID * BLOCK + 257


def wrap64(v: int) -> int:
    """v modulo 2^64, read as a signed 64-bit integer."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def columns(rows: list[tuple], nw: int, device="cpu") -> list[torch.Tensor]:
    """Rows as nw parallel int64 word tensors (the kernels' layout)."""
    if not rows:
        return [torch.zeros(0, dtype=torch.int64, device=device) for _ in range(nw)]
    t = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), nw)
    return [t[:, j].contiguous().to(device) for j in range(nw)]


# ------------------------------------------------ searchsorted and friends --

SEARCH_NW = (1, 2, 3, 4)
SEARCH_M = (1, 2, 3, 1000)
SEARCH_NQ = (1, 1000, GRID_TRIP)


def sorted_side(nw: int, m: int) -> list[tuple]:
    """m sorted rows of nw words.  At m = 1000: runs of equal rows of
    lengths 1, 2 and 7, rows differing only in the last word, rows
    differing only in the first word, and each of SPECIALS in every word
    position.  The three small sides keep a sign change at every bound."""
    if m == 1:
        return [(-1,) * nw]
    if m == 2:
        return [(INT64_MIN,) * nw, (INT64_MAX,) * nw]
    if m == 3:
        return [(-1,) * nw, (-1,) * nw, (0,) * (nw - 1) + (1,)]
    rnd = random.Random(100 + nw)
    rows = []
    for p in range(nw):
        for v in SPECIALS:
            if v == 0:
                continue  # the all-zero row comes once, below
            rows.append(tuple(v if j == p else 0 for j in range(nw)))
    rows.append((0,) * nw)
    for x in (-3, 5, 9):
        rows.append((7,) * (nw - 1) + (x,))
        rows.append((x,) + (7,) * (nw - 1))
    rows += [(11,) * nw] * 2 + [(-13,) * nw] * 7
    pool = SPECIALS + (-2, 2, 3, 100, -100)
    while len(rows) < m:
        if rnd.random() < 0.5:
            r = tuple(rnd.choice(pool) for _ in range(nw))
        else:
            r = tuple(rnd.randrange(INT64_MIN, INT64_MAX + 1) for _ in range(nw))
        # for nw > 1 leave room below and above every row
        extreme = nw > 1 and r in ((INT64_MIN,) * nw, (INT64_MAX,) * nw)
        if r not in rows and not extreme:
            rows.append(r)
    assert len(rows) == m
    return sorted(rows)


def base_queries(sorted_rows: list[tuple]) -> list[tuple]:
    """Every sorted row; each with its last word one less and one more
    (where that does not leave int64); the lowest and the highest row
    there is, which for nw > 1 lie below and above every sorted row."""
    nw = len(sorted_rows[0])
    out = [(INT64_MIN,) * nw, (INT64_MAX,) * nw]
    for r in sorted_rows:
        out.append(r)
        if r[-1] > INT64_MIN:
            out.append(r[:-1] + (r[-1] - 1,))
        if r[-1] < INT64_MAX:
            out.append(r[:-1] + (r[-1] + 1,))
    return out


def queries(sorted_rows: list[tuple], nq: int) -> list[tuple]:
    """nq of the base queries: a spread of them where nq is smaller, and
    all of them over and over where it is larger."""
    base = base_queries(sorted_rows)
    if nq <= len(base):
        step = len(base) / nq
        return [base[int(i * step)] for i in range(nq)]
    return [base[i % len(base)] for i in range(nq)]


def query_columns(sorted_rows: list[tuple], nq: int) -> list[torch.Tensor]:
    """queries() as word tensors, without a Python list of nq rows."""
    nw = len(sorted_rows[0])
    base = base_queries(sorted_rows)
    if nq <= len(base):
        return columns(queries(sorted_rows, nq), nw)
    idx = torch.arange(nq) % len(base)
    return [c.index_select(0, idx) for c in columns(base, nw)]


def bisect_oracle(sorted_rows: list[tuple], qs: list[tuple]):
    left = [bisect.bisect_left(sorted_rows, q) for q in qs]
    right = [bisect.bisect_right(sorted_rows, q) for q in qs]
    return left, right


def lookup_expected(left: torch.Tensor, right: torch.Tensor, m: int):
    """(pos, found) of lookup: the insertion position clamped into the
    table, which callers index with, and whether the row is there."""
    return left.clamp(max=m - 1), left < right


# -------------------------------------------------------------- run starts --

RUN_STARTS_NW = (1, 2, 3, 4)
RUN_STARTS_N = (1, 2, 257, GRID_TRIP)


def run_start_words(nw: int, n: int) -> list[torch.Tensor]:
    """Rows where row i equals its predecessor (i % (nw + 2) >= nw) or
    differs from it in exactly the one word i % (nw + 2); word 0 starts at
    INT64_MAX - 1 so that it wraps to INT64_MIN on the way."""
    i = torch.arange(n, dtype=torch.int64)
    change = i % (nw + 2)
    words = []
    for p in range(nw):
        w = torch.cumsum(((change == p) & (i > 0)).to(torch.int64), 0)
        words.append(w + (INT64_MAX - 1) if p == 0 else w - 5)
    return words


# --------------------------------------------------------------- pool hash --

POOL_SIZE = 1000
POOL_N = (0, 1, GRID_TRIP)
#: both with the top bit set, as unsigned 64-bit values
NONE_LO = 0x8000000000000001
NONE_HI = 0xFEDCBA9876543210


def pool_case(n: int, first_code: int = -1):
    """(codes, pool_lo, pool_hi): codes cycle through -1, INT64_MIN, 0,
    POOL_SIZE - 1 and random codes; half of the pool hashes are negative."""
    g = torch.Generator().manual_seed(77)
    pool_lo = torch.randint(INT64_MIN, INT64_MAX, (POOL_SIZE,), generator=g)
    pool_hi = torch.randint(INT64_MIN, INT64_MAX, (POOL_SIZE,), generator=g)
    pool_lo[0], pool_lo[POOL_SIZE - 1] = INT64_MIN, -1
    pool_hi[0], pool_hi[POOL_SIZE - 1] = -2, INT64_MIN + 1
    codes = torch.randint(0, POOL_SIZE, (n,), generator=g)
    edge = torch.tensor([-1, INT64_MIN, 0, POOL_SIZE - 1])
    codes[0::5] = edge[torch.arange(codes[0::5].shape[0]) % 4]
    if n:
        codes[0] = first_code
    return codes, pool_lo, pool_hi


def pool_oracle(codes, pool_lo, pool_hi):
    safe = codes.clamp(min=0)
    none_lo = torch.tensor(wrap64(NONE_LO), dtype=torch.int64)
    none_hi = torch.tensor(wrap64(NONE_HI), dtype=torch.int64)
    lo = torch.where(codes >= 0, pool_lo.index_select(0, safe), none_lo)
    hi = torch.where(codes >= 0, pool_hi.index_select(0, safe), none_hi)
    return lo, hi


# -------------------------------------------------------------- seg reduce --

SEG_NW = (1, 2, 3, 4, 8)
SEG_NACC = (0, 1, 8)
SEG_N = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
SEG_PATTERNS = ("all_equal", "all_distinct", "wave_block_edges", "last_word", "first_word")

#: run bounds of "wave_block_edges": a run over lanes 63..64 of the first
#: wave and a run over rows 255..256, the last of block 0 and first of 1
_EDGE_BOUNDS = (0, 63, 65, 255, 257)


def seg_rows(pattern: str, nw: int, n: int) -> list[tuple]:
    if pattern == "all_equal":
        return [(INT64_MIN,) + (5,) * (nw - 1)] * n
    if pattern == "all_distinct":
        return [(i - 3,) * nw for i in range(n)]
    if pattern == "wave_block_edges":
        return [(bisect.bisect_right(_EDGE_BOUNDS, i),) * nw for i in range(n)]
    if pattern == "last_word":
        return [(7,) * (nw - 1) + (i // 3 - 2,) for i in range(n)]
    if pattern == "first_word":
        return [(i // 5 - 2,) + (7,) * (nw - 1) for i in range(n)]
    raise ValueError(pattern)


_CONTRIB_CYCLE = (2**62 - 1, 2**62 + 3, -(2**62), 1, -1, -(2**62) - 5, 0, 12345)


def seg_contribs(nacc: int, n: int) -> list[list[int]]:
    """nacc columns of n contributions; two neighbours near +-2^62 wrap."""
    return [
        [_CONTRIB_CYCLE[(i + 3 * a) % len(_CONTRIB_CYCLE)] + (i % 7) * a for i in range(n)]
        for a in range(nacc)
    ]


def seg_oracle(rows: list[tuple], contribs: list[list[int]]):
    """(unique rows, first row index of each, per-accumulator wrapped sums)."""
    uniq, first = [], []
    sums = [[] for _ in contribs]
    for i, r in enumerate(rows):
        if i == 0 or r != rows[i - 1]:
            uniq.append(r)
            first.append(i)
            for s in sums:
                s.append(0)
        for s, c in zip(sums, contribs):
            s[-1] = wrap64(s[-1] + c[i])
    return uniq, first, sums


# ------------------------------------------------------------- sort repair --

REPAIR_N = (2, 3, 8, 9, 64, 65)
#: starts every length of 2, 3 and 4 at an even and at an odd row
_RUN_CYCLE = (1, 4, 2, 3, 4, 3, 1, 2)


def repair_runs(n: int) -> list[int]:
    """Lengths (1..4) of the equal-k0 runs that tile n rows; the last run
    ends at row n - 1 and has two rows or more."""
    if n == 2:
        return [2]
    if n == 3:
        return [1, 2]
    out, total, i = [], 0, 0
    while total < n:
        length = min(_RUN_CYCLE[i % len(_RUN_CYCLE)], n - total)
        out.append(length)
        total += length
        i += 1
    if out[-1] == 1:  # merge a trailing single row into the run before it
        out[-2:] = [out[-2] + 1] if out[-2] < 4 else [out[-2] - 1, 2]
    return out


def repair_case(runs: list[int]):
    """(k0, k1) lists: k0 ascending and constant over each run, negative
    at first; k1 strictly descending inside each run, the worst case."""
    k0, k1 = [], []
    for r, length in enumerate(runs):
        for j in range(length):
            k0.append(-50 + 7 * r)
            k1.append((r % 3) - 3 * j)
    return k0, k1


def run_bounds(k0: list[int]) -> list[tuple[int, int]]:
    out, s = [], 0
    for i in range(1, len(k0) + 1):
        if i == len(k0) or k0[i] != k0[s]:
            out.append((s, i))
            s = i
    return out


def check_repair(k0, k1_before, k0_after, k1_after, perm):
    """After a repair: k1 ascending inside each run, perm records the
    moves, k0 and rows of single-row runs untouched."""
    n = len(k0)
    assert k0_after == k0
    assert sorted(perm) == list(range(n))
    assert [k1_before[p] for p in perm] == k1_after
    for s, e in run_bounds(k0):
        assert k1_after[s:e] == sorted(k1_before[s:e]), f"run [{s},{e}) not repaired"
        assert sorted(perm[s:e]) == list(range(s, e)), f"run [{s},{e}) leaked rows"
        if e - s == 1:
            assert perm[s] == s and k1_after[s] == k1_before[s]


LEX_N = 2049


def lex_case():
    """(k0, k1) of LEX_N rows just above lex_sort_words' fast-path
    threshold, with several word-0 runs of 2, 3 and 4 rows scattered over
    the input and all of int64 in use."""
    g = torch.Generator().manual_seed(2049)
    k0 = torch.randint(INT64_MIN, INT64_MAX, (LEX_N,), generator=g)
    k1 = torch.randint(INT64_MIN, INT64_MAX, (LEX_N,), generator=g)
    pos = torch.randperm(LEX_N, generator=g)
    at = 0
    for rep in range(6):
        for length in (2, 3, 4):
            k0[pos[at : at + length]] = k0[pos[at]].item()
            at += length
    return k0, k1


# ---------------------------------------------------------------- hash agg --


def hash_agg_capacity(n: int) -> int:
    """Slots of hash_agg_gpu's table for n rows when no estimate is given."""
    return 1 << max(10, (2 * n - 1).bit_length())


def chain_keys(n: int) -> list[int]:
    """n distinct word-0 values that all hash to slot 0 of the table."""
    cap = hash_agg_capacity(n)
    return [j * cap for j in range(n)]


def hash_agg_oracle(k0, k1, contribs):
    """{(k0, k1): [wrapped sums]} over lists of Python ints."""
    out: dict = {}
    for i, key in enumerate(zip(k0, k1)):
        acc = out.setdefault(key, [0] * len(contribs))
        for a, c in enumerate(contribs):
            acc[a] = wrap64(acc[a] + c[i])
    return out


def merge_slots(uk0, uk1, accs):
    """The kernel's output slots merged per key: one key may own two slots
    for a moment and the caller adds them up."""
    return hash_agg_oracle(uk0, uk1, accs)

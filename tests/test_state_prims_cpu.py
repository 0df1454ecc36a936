"""CPU checks of tests/state_prims_cases.py: the inputs hold the edges
the GPU tests are there for, and the oracles agree with each other and with
the engine's CPU paths."""

import pytest
import torch

from tests import state_prims_cases as C


def test_grid_trip_is_past_one_full_grid():
    assert C.GRID_TRIP == 524288 + 257
    assert C.GRID_TRIP > C.MAX_GRID * C.BLOCK + C.BLOCK


def test_wrap64():
    assert C.wrap64(2**63) == C.INT64_MIN
    assert C.wrap64(-(2**63) - 1) == C.INT64_MAX
    assert C.wrap64(2**62 + 2**62) == C.INT64_MIN
    t = torch.tensor([2**62, 2**62, 5], dtype=torch.int64)
    assert int(t.sum()) == C.wrap64(2**63 + 5)


# ------------------------------------------------ searchsorted and friends --


@pytest.mark.parametrize("nw", C.SEARCH_NW)
def test_sorted_side_holds_every_edge(nw):
    for m in C.SEARCH_M:
        rows = C.sorted_side(nw, m)
        assert len(rows) == m and rows == sorted(rows)
        assert all(len(r) == nw for r in rows)
        # an unsigned comparison orders every one of these sides differently
        unsigned = sorted(rows, key=lambda r: tuple(v & (2**64 - 1) for v in r))
        assert m == 1 or unsigned != rows
    rows = C.sorted_side(nw, 1000)
    runs = {e - s for s, e in C.run_bounds(rows)}
    assert {1, 2, 7} <= runs
    for p in range(nw):
        assert set(C.SPECIALS) <= {r[p] for r in rows}
    pairs = list(zip(rows, rows[1:]))
    assert any(a[:-1] == b[:-1] and a[-1] != b[-1] for a, b in pairs)
    if nw > 1:
        firsts = {}
        for r in rows:
            firsts.setdefault(r[1:], set()).add(r[0])
        assert any(len(v) > 1 for v in firsts.values())


@pytest.mark.parametrize("nw", C.SEARCH_NW)
def test_queries_hit_miss_and_bracket(nw):
    rows = C.sorted_side(nw, 1000)
    base = C.base_queries(rows)
    assert set(rows) <= set(base)
    assert (C.INT64_MIN,) * nw in base and (C.INT64_MAX,) * nw in base
    left, right = C.bisect_oracle(rows, base)
    assert 0 in left and 1000 in right
    if nw > 1:  # a query below and a query above every row
        assert 0 in right and 1000 in left
    assert any(l == r for l, r in zip(left, right))  # misses
    assert any(r - l == 7 for l, r in zip(left, right))  # the run of 7
    for nq in (1, 1000):
        qs = C.queries(rows, nq)
        assert len(qs) == nq
        assert [tuple(t) for t in torch.stack(C.query_columns(rows, nq), 1).tolist()] == qs
    cols = C.query_columns(rows, 5000)
    assert [tuple(t) for t in torch.stack(cols, 1).tolist()] == C.queries(rows, 5000)
    assert C.query_columns(rows, C.GRID_TRIP)[0].shape[0] == C.GRID_TRIP


@pytest.mark.parametrize("nw", C.SEARCH_NW)
def test_cpu_searchsorted_words_agrees_with_bisect(nw):
    """The CPU path of searchsorted_words serves as the oracle at
    GRID_TRIP queries; here it is held against bisect."""
    from pathway_amd.engine.state import searchsorted_words

    for m in C.SEARCH_M:
        rows = C.sorted_side(nw, m)
        qs = C.base_queries(rows)
        left, right = C.bisect_oracle(rows, qs)
        s, q = C.columns(rows, nw), C.columns(qs, nw)
        assert searchsorted_words(s, q, "left").tolist() == left
        assert searchsorted_words(s, q, "right").tolist() == right
        pos, found = C.lookup_expected(torch.tensor(left), torch.tensor(right), m)
        assert pos.tolist() == [min(l, m - 1) for l in left]
        assert found.tolist() == [q_ in set(rows) for q_ in qs]


# -------------------------------------------------------------- run starts --


@pytest.mark.parametrize("nw", C.RUN_STARTS_NW)
def test_run_start_words_change_one_word_at_a_time(nw):
    from pathway_amd.engine.state import rows_ne

    words = C.run_start_words(nw, 257)
    rows = torch.stack(words, 1)
    ndiff = (rows[1:] != rows[:-1]).sum(1)
    assert set(ndiff.tolist()) == {0, 1}
    for p in range(nw):
        only_p = (rows[1:, p] != rows[:-1, p]) & (ndiff == 1)
        assert bool(only_p.any())
    assert bool((words[0] < 0).any()) and bool((words[0] > 0).any())  # wrapped
    starts = rows_ne(words)
    assert starts.tolist() == [True] + (ndiff > 0).tolist()
    assert rows_ne(C.run_start_words(nw, 1)).tolist() == [True]
    assert rows_ne(C.run_start_words(nw, 2)).tolist() == [True, nw > 1]


# --------------------------------------------------------------- pool hash --


def test_pool_case_holds_every_code():
    codes, lo, hi = C.pool_case(C.GRID_TRIP)
    assert {-1, C.INT64_MIN, 0, C.POOL_SIZE - 1} <= set(codes[:50].tolist())
    assert int(codes.max()) == C.POOL_SIZE - 1
    assert bool((lo < 0).any()) and bool((hi < 0).any())
    assert C.NONE_LO >> 63 == 1 and C.NONE_HI >> 63 == 1
    want_lo, want_hi = C.pool_oracle(codes, lo, hi)
    for i in range(50):
        c = int(codes[i])
        assert int(want_lo[i]) == (int(lo[c]) if c >= 0 else C.wrap64(C.NONE_LO))
        assert int(want_hi[i]) == (int(hi[c]) if c >= 0 else C.wrap64(C.NONE_HI))
    for first in (-1, C.INT64_MIN, 0, C.POOL_SIZE - 1):
        assert C.pool_case(1, first)[0].tolist() == [first]
    assert C.pool_case(0)[0].shape == (0,)


# -------------------------------------------------------------- seg reduce --


@pytest.mark.parametrize("nw", C.SEG_NW)
def test_seg_patterns_and_oracle(nw):
    n = 1025
    assert len(C.run_bounds(C.seg_rows("all_equal", nw, n))) == 1
    assert len(C.run_bounds(C.seg_rows("all_distinct", nw, n))) == n
    bounds = C.run_bounds(C.seg_rows("wave_block_edges", nw, n))
    assert (63, 65) in bounds and (255, 257) in bounds
    rows = C.seg_rows("last_word", nw, n)
    assert len({r[:-1] for r in rows}) == 1 and len({r[-1] for r in rows}) > 300
    rows = C.seg_rows("first_word", nw, n)
    assert len({r[1:] for r in rows}) == 1 and len({r[0] for r in rows}) > 200
    for pattern in C.SEG_PATTERNS:
        for n in C.SEG_N:
            rows = C.seg_rows(pattern, nw, n)
            assert len(rows) == n
            contribs = C.seg_contribs(8, n)
            uniq, first, sums = C.seg_oracle(rows, contribs)
            assert [rows[i] for i in first] == uniq
            assert len(set(uniq)) == len(uniq)
            if n == 0:
                assert uniq == [] and sums == [[]] * 8
                continue
            # the oracle against index_add_, which wraps like the atomic
            starts = torch.zeros(n, dtype=torch.int64)
            starts[first] = 1
            seg = torch.cumsum(starts, 0) - 1
            for s, c in zip(sums, contribs):
                ref = torch.zeros(len(uniq), dtype=torch.int64)
                ref.index_add_(0, seg, torch.tensor(c, dtype=torch.int64))
                assert ref.tolist() == s


def test_seg_contribs_wrap():
    rows = C.seg_rows("all_equal", 1, 64)
    contribs = C.seg_contribs(2, 64)
    _, _, sums = C.seg_oracle(rows, contribs)
    for s, c in zip(sums, contribs):
        assert abs(sum(c)) >= 2**63 or s[0] == sum(c)
    assert any(abs(sum(c[:2])) >= 2**63 for c in C.seg_contribs(8, 2))


# ------------------------------------------------------------- sort repair --


def test_repair_runs_cover_lengths_parities_and_the_end():
    starts = set()
    for n in C.REPAIR_N:
        runs = C.repair_runs(n)
        assert sum(runs) == n and all(1 <= r <= 4 for r in runs)
        assert runs[-1] >= 2, "a run must end at row n - 1"
        at = 0
        for r in runs:
            starts.add((r, at % 2))
            at += r
        k0, k1 = C.repair_case(runs)
        assert k0 == sorted(k0) and min(k0) < 0 and min(k1) < 0
        assert [e - s for s, e in C.run_bounds(k0)] == runs
        for s, e in C.run_bounds(k0):
            assert all(k1[i] > k1[i + 1] for i in range(s, e - 1))
        # check_repair accepts the repaired rows and rejects the input
        perm, k1_after = [], []
        for s, e in C.run_bounds(k0):
            perm += list(range(e - 1, s - 1, -1))
            k1_after += k1[s:e][::-1]
        C.check_repair(k0, k1, k0, k1_after, perm)
        with pytest.raises(AssertionError):
            C.check_repair(k0, k1, k0, k1, list(range(n)))
    assert starts >= {(r, p) for r in (2, 3, 4) for p in (0, 1)}


def test_lex_case_has_forced_runs():
    k0, k1 = C.lex_case()
    assert k0.shape == (C.LEX_N,) and C.LEX_N > 2048
    lengths = [e - s for s, e in C.run_bounds(sorted(k0.tolist()))]
    assert max(lengths) == 4
    assert all(lengths.count(L) >= 6 for L in (2, 3, 4))
    rows = list(zip(k0.tolist(), k1.tolist()))
    assert len(set(rows)) == C.LEX_N
    # the engine's own CPU sort gives the order the device must give
    from pathway_amd.engine.state import lex_sort_words

    perm = lex_sort_words([k0, k1]).tolist()
    assert [rows[p] for p in perm] == sorted(rows)


# ---------------------------------------------------------------- hash agg --


def test_chain_keys_share_a_slot():
    for n in (400, 600):
        cap = C.hash_agg_capacity(n)
        keys = C.chain_keys(n)
        assert len(set(keys)) == n and {k & (cap - 1) for k in keys} == {0}
        assert C.INT64_MIN not in keys and max(keys) < 2**63
    assert C.hash_agg_capacity(400) == 1024 and C.hash_agg_capacity(600) == 2048
    # a chain of 400 fits the probe bound of 512, one of 600 does not
    assert 400 <= 512 < 600


def test_hash_agg_oracle_wraps_and_merges():
    got = C.hash_agg_oracle([1, 1, 2], [5, 5, 5], [[2**62, 2**62, 1]])
    assert got == {(1, 5): [C.INT64_MIN], (2, 5): [1]}
    assert C.merge_slots([1, 2, 1], [5, 5, 5], [[3, 1, -3]]) == {(1, 5): [0], (2, 5): [1]}

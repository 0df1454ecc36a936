"""GPU tests of the sorted-state primitives at their edges, each kernel
called directly and compared exactly with a plain Python oracle: signed
multi-word search, run starts, pool hash, the segmented reduce at wave and
block bounds, the odd-even sort repair and the hash aggregation's probe
chain.  Inputs and oracles are in tests/state_prims_cases.py."""

import pytest
import torch

from tests import state_prims_cases as C

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


def _dev(cols):
    return [c.to(DEV) for c in cols]


# ------------------------------------------------ searchsorted and friends --


@gpu
@requires_cuda
@pytest.mark.parametrize("m", C.SEARCH_M)
@pytest.mark.parametrize("nw", C.SEARCH_NW)
def test_search_lookup_key_range(nw, m):
    from pathway_amd import ops
    from pathway_amd.engine.state import searchsorted_words

    rows = C.sorted_side(nw, m)
    s_cpu = C.columns(rows, nw)
    s = _dev(s_cpu)
    for nq in C.SEARCH_NQ:
        q_cpu = C.query_columns(rows, nq)
        if nq <= 1000:
            left, right = (
                torch.tensor(x) for x in C.bisect_oracle(rows, C.queries(rows, nq))
            )
        else:
            left = searchsorted_words(s_cpu, q_cpu, "left")
            right = searchsorted_words(s_cpu, q_cpu, "right")
        q = _dev(q_cpu)
        where = f"nw={nw} m={m} nq={nq}"
        assert torch.equal(ops.searchsorted_gpu(s, q, "left").cpu(), left), where
        assert torch.equal(ops.searchsorted_gpu(s, q, "right").cpu(), right), where
        lo, hi = ops.key_range_gpu(s, q)
        assert torch.equal(lo.cpu(), left) and torch.equal(hi.cpu(), right), where
        pos, found = ops.lookup_gpu(s, q)
        want_pos, want_found = C.lookup_expected(left, right, m)
        assert torch.equal(found.cpu(), want_found), where
        assert torch.equal(pos.cpu(), want_pos), where


# -------------------------------------------------------------- run starts --


@gpu
@requires_cuda
@pytest.mark.parametrize("nw", C.RUN_STARTS_NW)
def test_run_starts(nw):
    from pathway_amd import ops
    from pathway_amd.engine.state import rows_ne

    for n in C.RUN_STARTS_N:
        words = C.run_start_words(nw, n)
        want = rows_ne(words)
        got = ops.run_starts_gpu(_dev(words))
        assert got.dtype == torch.bool
        assert torch.equal(got.cpu(), want), f"nw={nw} n={n}"


# --------------------------------------------------------------- pool hash --


@gpu
@requires_cuda
def test_pool_hash():
    from pathway_amd import ops

    cases = [C.pool_case(n) for n in C.POOL_N]
    cases += [C.pool_case(1, c) for c in (C.INT64_MIN, 0, C.POOL_SIZE - 1)]
    for codes, pool_lo, pool_hi in cases:
        want_lo, want_hi = C.pool_oracle(codes, pool_lo, pool_hi)
        lo, hi = ops.pool_hash_gpu(
            codes.to(DEV), pool_lo.to(DEV), pool_hi.to(DEV), C.NONE_LO, C.NONE_HI
        )
        assert lo.shape == codes.shape and hi.shape == codes.shape
        assert torch.equal(lo.cpu(), want_lo), f"n={codes.shape[0]}"
        assert torch.equal(hi.cpu(), want_hi), f"n={codes.shape[0]}"


# -------------------------------------------------------------- seg reduce --


@gpu
@requires_cuda
@pytest.mark.parametrize("nw", C.SEG_NW)
def test_seg_reduce_words(nw):
    from pathway_amd import ops

    for pattern in C.SEG_PATTERNS:
        for n in C.SEG_N:
            rows = C.seg_rows(pattern, nw, n)
            words = C.columns(rows, nw, DEV)
            all_contribs = C.seg_contribs(max(C.SEG_NACC), n)
            for nacc in C.SEG_NACC:
                contribs = all_contribs[:nacc]
                uniq, first, sums = C.seg_oracle(rows, contribs)
                got_words, got_first, got_sums = ops.seg_reduce_words_gpu(
                    words,
                    [torch.tensor(c, dtype=torch.int64, device=DEV) for c in contribs],
                )
                where = f"{pattern} nw={nw} n={n} nacc={nacc}"
                assert len(got_words) == nw and len(got_sums) == nacc, where
                assert got_first.dtype == torch.int64, where
                assert got_first.cpu().tolist() == first, where
                got_rows = list(zip(*(w.cpu().tolist() for w in got_words)))
                assert got_rows == uniq, where
                for a in range(nacc):
                    assert got_sums[a].dtype == torch.int64
                    assert got_sums[a].cpu().tolist() == sums[a], f"{where} acc {a}"


@gpu
@requires_cuda
def test_seg_reduce_limits():
    from pathway_amd import ops

    col = torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        ops.seg_reduce_words_gpu([col] * 9, [col])
    with pytest.raises(RuntimeError):
        ops.seg_reduce_words_gpu([col], [col] * 9)
    # no rows: empty outputs of the right count, type and device
    none = col[:0]
    words, first, sums = ops.seg_reduce_words_gpu([none] * 3, [none] * 2)
    assert [tuple(t.shape) for t in words + [first] + sums] == [(0,)] * 6
    assert all(t.dtype == torch.int64 and t.is_cuda for t in words + [first] + sums)


# ------------------------------------------------------------- sort repair --


def _repair(k0, k1, passes=None):
    from pathway_amd import ops

    n = len(k0)
    k0_t = torch.tensor(k0, dtype=torch.int64, device=DEV)
    k1_t = torch.tensor(k1, dtype=torch.int64, device=DEV)
    perm = torch.arange(n, dtype=torch.int64, device=DEV)
    if passes is None:
        ops.sort_repair_gpu(k0_t, k1_t, perm)
    else:
        ops.sort_repair_gpu(k0_t, k1_t, perm, passes=passes)
    return k0_t.cpu().tolist(), k1_t.cpu().tolist(), perm.cpu().tolist()


@gpu
@requires_cuda
@pytest.mark.parametrize("n", C.REPAIR_N)
def test_sort_repair_runs_up_to_four(n):
    k0, k1 = C.repair_case(C.repair_runs(n))
    k0_after, k1_after, perm = _repair(k0, k1)
    C.check_repair(k0, k1, k0_after, k1_after, perm)


@gpu
@requires_cuda
@pytest.mark.parametrize("length", (5, 8))
def test_sort_repair_longer_run_with_as_many_passes(length):
    for start in (0, 1):  # the run starts at an even and at an odd row
        k0, k1 = C.repair_case([1] * start + [length, 1, 2])
        k0_after, k1_after, perm = _repair(k0, k1, passes=length)
        C.check_repair(k0, k1, k0_after, k1_after, perm)


@gpu
@requires_cuda
def test_lex_sort_words_just_above_the_fast_path_threshold():
    from pathway_amd.engine.state import lex_sort_words

    k0, k1 = C.lex_case()
    perm = lex_sort_words([k0.to(DEV), k1.to(DEV)]).cpu()
    assert sorted(perm.tolist()) == list(range(C.LEX_N))
    rows = list(zip(k0.tolist(), k1.tolist()))
    assert [rows[p] for p in perm.tolist()] == sorted(rows)


# ---------------------------------------------------------------- hash agg --


def _hash_agg(k0, k1, contribs, **kw):
    """hash_agg_gpu over Python lists; the merged {key: sums} or None.
    Checks on the way that each slot's representative is a row of its key."""
    from pathway_amd import ops

    t = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)  # noqa: E731
    out = ops.hash_agg_gpu(t(k0), t(k1), [t(c) for c in contribs], **kw)
    if out is None:
        return None
    uk0, uk1, accs, rep = out
    uk0, uk1, rep = uk0.cpu().tolist(), uk1.cpu().tolist(), rep.cpu().tolist()
    assert len(accs) == len(contribs)
    for a, b, r in zip(uk0, uk1, rep):
        assert 0 <= r < len(k0) and (k0[r], k1[r]) == (a, b), "representative row"
    return C.merge_slots(uk0, uk1, [a.cpu().tolist() for a in accs])


@gpu
@requires_cuda
def test_hash_agg_tiny_and_single_key():
    assert _hash_agg([], [], [[], []]) == {}
    assert _hash_agg([-7], [9], [[5], [-(2**62)]]) == {(-7, 9): [5, -(2**62)]}
    n = 10_000
    k0, k1 = [-(2**62) - 1] * n, [3] * n
    contribs = [[1] * n, [2**62 + i for i in range(n)]]
    assert _hash_agg(k0, k1, contribs) == C.hash_agg_oracle(k0, k1, contribs)


@gpu
@requires_cuda
def test_hash_agg_shared_word0_and_zero_sums():
    # three keys share word 0 and differ in word 1, rows interleaved; the
    # third key's contributions cancel and it is still emitted, with zeros
    n = 3000
    k0 = [12345] * n
    k1 = [(-1, 1, 2**62)[i % 3] for i in range(n)]
    contribs = [
        [(1, 2, 1 if (i // 3) % 2 else -1)[i % 3] for i in range(n)],
        [(i, -i, (7 if (i // 3) % 2 else -7))[i % 3] for i in range(n)],
    ]
    want = C.hash_agg_oracle(k0, k1, contribs)
    assert len(want) == 3 and want[(12345, 2**62)] == [0, 0]
    assert _hash_agg(k0, k1, contribs) == want


@gpu
@requires_cuda
def test_hash_agg_accumulator_limit():
    n = 500
    k0 = [i % 37 - 18 for i in range(n)]
    k1 = [(i % 37) * 11 + 1 for i in range(n)]
    contribs = C.seg_contribs(8, n)
    assert _hash_agg(k0, k1, contribs) == C.hash_agg_oracle(k0, k1, contribs)
    with pytest.raises(RuntimeError):
        _hash_agg(k0, k1, contribs + [[1] * n])


@gpu
@requires_cuda
def test_hash_agg_probe_chain():
    # every key lands on slot 0: a chain of 400 is within the 512 probes a
    # row may take, a chain of 600 is not and the call reports it
    k0 = C.chain_keys(400)
    k1 = [j + 1 for j in range(400)]
    contribs = [[j - 200 for j in range(400)]]
    assert _hash_agg(k0, k1, contribs) == C.hash_agg_oracle(k0, k1, contribs)
    k0 = C.chain_keys(600)
    assert _hash_agg(k0, [1] * 600, [[1] * 600]) is None


@gpu
@requires_cuda
def test_hash_agg_estimate_too_small_returns_none():
    g = torch.Generator().manual_seed(5)
    k0 = torch.randint(-(2**62), 2**62, (2000,), generator=g).tolist()
    assert len(set(k0)) == 2000
    assert _hash_agg(k0, [1] * 2000, [[1] * 2000], expected_uniques=1) is None

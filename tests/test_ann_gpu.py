"""GPU tests of the ANN indexes (engine/ann.py) where a query has fewer
than k live candidates: deleted rows, a short probed IVF list next to a
long one, sparse LSH buckets.  The top-k kernel leaves such slots unfilled
and search() must report them invalid.  Data and checks are in
tests/topk_gemm_cases.py; scores are exact integers on both devices."""

import pytest
import torch

from tests.topk_gemm_cases import (
    ANN_METRIC,
    IVF_FAR_ROWS,
    NEG_INF,
    ann_flat_case,
    ann_ivf_case,
    ann_lsh_case,
    build_ann_state,
    check_ann_invariants,
    hits,
    make_ivf_state,
    make_lsh_state,
)

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


@pytest.fixture
def topk_calls(monkeypatch):
    """Counts the launches of the top-k kernel: these tests are about it."""
    from pathway_amd import ops

    calls = []
    real = ops.topk_gpu

    def spy(scores, k):
        calls.append((tuple(scores.shape), k))
        return real(scores, k)

    monkeypatch.setattr(ops, "topk_gpu", spy)
    return calls


@gpu
@requires_cuda
def test_flat_deleted_rows_match_cpu(topk_calls):
    from pathway_amd.engine.ann import FlatIndexState

    keys, vecs, deleted, queries, k = ann_flat_case()
    cpu = build_ann_state(FlatIndexState("cpu", ANN_METRIC), keys, vecs, deleted)
    dev = build_ann_state(FlatIndexState(DEV, ANN_METRIC), keys, vecs, deleted)
    want = cpu.search(queries, k)
    got = dev.search(queries.to(DEV), k)
    assert topk_calls == [((3, 40), 32)]
    assert got[1].shape == want[1].shape == (3, 32)
    live = 40 - deleted.numel()
    assert got[2].sum(1).tolist() == want[2].sum(1).tolist() == [live] * 3
    assert hits(*got) == hits(*want)
    assert bool((got[1].cpu()[~got[2].cpu()] == NEG_INF).all())
    check_ann_invariants(keys, vecs, deleted, queries, *got)


@gpu
@requires_cuda
def test_ivf_short_list_next_to_long_list(topk_calls):
    keys, vecs, deleted, queries, k = ann_ivf_case()
    st = build_ann_state(make_ivf_state(DEV), keys, vecs, deleted)
    assert st.centroids is not None and st.clustered == 40
    sizes = (st.list_offsets[1:] - st.list_offsets[:-1]).tolist()
    assert sorted(sizes) == [2, 38], sizes
    ids, scores, valid = st.search(queries.to(DEV), k)
    assert topk_calls == [((2, 38), k)]
    check_ann_invariants(keys, vecs, deleted, queries, ids, scores, valid)
    got = hits(ids, scores, valid)
    far = sorted(
        (-1 if r == IVF_FAR_ROWS[0] else -3, *keys[r].tolist()) for r in IVF_FAR_ROWS
    )
    # the first query reaches the two far rows and nothing else
    assert got[0] == far
    assert valid.sum(1).tolist() == [2, k]


@gpu
@requires_cuda
def test_lsh_sparse_buckets(topk_calls):
    keys, vecs, deleted, queries, k = ann_lsh_case()
    st = build_ann_state(make_lsh_state(DEV), keys, vecs, deleted)
    ids, scores, valid = st.search(queries.to(DEV), k)
    assert len(topk_calls) == 1 and topk_calls[0][0][1] > k
    check_ann_invariants(keys, vecs, deleted, queries, ids, scores, valid)
    counts = valid.sum(1).tolist()
    # some query fills every slot and some query cannot
    assert max(counts) == k and min(counts) < k, counts

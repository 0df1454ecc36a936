"""GPU tests of BM25 on the device: the pw_bm25_score kernel against the
float64 host scores, its run-to-run determinism, and the TantivyBM25
pipeline on the GPU against PW_BM25=host.  Corpus, queries, comparison
rule and the derivation of the tolerance (rtol 2e-6, atol 0) are in
tests/bm25_cases.py."""

import pytest
import torch

from pathway_amd.ops import BM25_TILE
from tests.bm25_cases import QUERIES, RTOL, close, doc_key, fill, make_texts

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


# the tile edge, the tail tile and the binary-search bounds
SIZES = [1, BM25_TILE - 1, BM25_TILE, BM25_TILE + 1, 2 * BM25_TILE + 1]


def _score_batch(state, queries):
    """Dense (len(queries), n) scores of one ops.bm25_score launch over
    the state's compiled postings, with the arguments of the launch."""
    import numpy as np

    from pathway_amd import ops

    keys, offsets, _, pidx, ptf, norm = state._compile()
    terms = [state._query_terms(q) for q in queries]
    q_off = np.zeros(len(queries) + 1, dtype=np.int32)
    np.cumsum([t.size for t, _ in terms], out=q_off[1:])
    args = (
        offsets,
        pidx,
        ptf,
        norm,
        torch.from_numpy(q_off).to(DEV),
        torch.from_numpy(np.concatenate([t for t, _ in terms])).to(DEV),
        torch.from_numpy(np.concatenate([i for _, i in terms])).to(DEV),
        state.k1,
    )
    return keys, ops.bm25_score(*args), args


@gpu
@requires_cuda
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_host_scores(n):
    from pathway_amd import ops
    from pathway_amd.stdlib.indexing.bm25 import _BM25DeviceState, _BM25State

    texts = make_texts(n)
    oracle = fill(_BM25State(), texts)
    state = fill(_BM25DeviceState(device=DEV), texts)
    keys, scores, args = _score_batch(state, QUERIES)
    assert scores.shape == (len(QUERIES), n) and scores.dtype == torch.float32
    assert keys == [doc_key(i) for i in range(n)]
    q_off = args[4].tolist()
    if n > 1000:  # every word of the corpus is in use
        assert [b - a for a, b in zip(q_off, q_off[1:])] == [1, 2, 4, 8, 0]
    got = scores.cpu().tolist()
    for qi, q in enumerate(QUERIES):
        want = dict(oracle.search(q, n))  # float64, the docs that score
        bad = [
            (i, got[qi][i], want.get(doc_key(i), 0.0))
            for i in range(n)
            if not close(got[qi][i], want.get(doc_key(i), 0.0))
        ]
        assert not bad, f"n={n} query {q!r}: {len(bad)} off, first {bad[:3]}"
    assert not any(got[-1])  # the all-unknown row is written, as zeros
    # the torch path of the op, the second reference, on the same arrays:
    # both are within 15u of the exact score, so within 30u < RTOL of
    # each other
    cpu_args = [a.cpu() if isinstance(a, torch.Tensor) else a for a in args]
    ref = ops.bm25_score(*cpu_args)
    torch.testing.assert_close(scores.cpu(), ref, rtol=RTOL, atol=0)


@gpu
@requires_cuda
def test_kernel_is_deterministic():
    from pathway_amd import ops
    from pathway_amd.stdlib.indexing.bm25 import _BM25DeviceState

    n = 2 * BM25_TILE + 1
    state = fill(_BM25DeviceState(device=DEV), make_texts(n))
    _, first, args = _score_batch(state, QUERIES)
    second = ops.bm25_score(*args)
    assert torch.equal(first, second)


@pytest.fixture
def on_gpu():
    from pathway_amd.internals.config import pathway_config

    pathway_config.device = DEV
    try:
        yield
    finally:
        pathway_config.device = None


@gpu
@requires_cuda
@pytest.mark.parametrize("filtered", [False, True])
def test_pipeline_matches_host(on_gpu, monkeypatch, filtered):
    from tests.bm25_cases import check_pipeline

    check_pipeline(10, filtered, monkeypatch)


@gpu
@requires_cuda
@pytest.mark.parametrize("segments", [1, 2, 3])
def test_state_on_gpu_k_paths(on_gpu, segments):
    """k <= 32 (pw_topk: one stage up to _TOPK_SEG docs, two stages over
    2 and 3 segments beyond, the last one nearly all padding), k = 40
    (torch.topk) and the filter fallback on one GPU state, against the
    host oracle."""
    from pathway_amd.stdlib.indexing.bm25 import (
        _TOPK_SEG,
        _BM25DeviceState,
        _BM25State,
    )
    from tests.bm25_cases import check_hits

    n = {1: 4097, 2: _TOPK_SEG + 1, 3: 2 * _TOPK_SEG + 5}[segments]
    texts = make_texts(n)
    payloads = [{"ok": i % 64 == 63} for i in range(n)]
    oracle = fill(_BM25State(), texts, payloads)
    state = fill(_BM25DeviceState(device=DEV), texts, payloads)
    flt = "ok == `true`"
    qs = QUERIES + ["all w1 w2", "all w0 w1", "solo", "all w5", "w9 w3"]
    ks = [10] * len(QUERIES) + [40, 2, 10, 32, 1]
    fs = [None] * len(QUERIES) + [None, flt, None, None, None]
    for q, k, f, hits in zip(qs, ks, fs, state.search_batch(qs, ks, fs)):
        check_hits(hits, oracle, q, k, f)


@gpu
@requires_cuda
def test_hybrid_index_on_gpu(on_gpu, monkeypatch):
    from pathway_amd.debug import table_from_rows, table_to_dicts
    from pathway_amd.internals.schema import schema_from_types
    from pathway_amd.stdlib.indexing import HybridIndex, TantivyBM25

    monkeypatch.delenv("PW_BM25", raising=False)
    docs = table_from_rows(
        schema_from_types(text=str), [("alpha beta",), ("gamma delta",)]
    )
    queries = table_from_rows(schema_from_types(q=str), [("alpha",)])
    hybrid = HybridIndex([TantivyBM25(docs.text)])
    reply = hybrid.query_as_of_now(queries.q, number_of_matches=1)
    keys, cols = table_to_dicts(reply)
    ids = cols["_pw_index_reply_ids"][keys[0]]
    dkeys, dcols = table_to_dicts(docs)
    assert dcols["text"][ids[0]] == "alpha beta"

"""CPU checks of tests/topk_gemm_cases.py: the oracles agree with plain
Python, the inputs have the properties the GPU tests rely on, and the
conditions under which the GEMM comparison is exact really hold."""

import math

import pytest
import torch

from tests import topk_gemm_cases as C

NEG = C.NEG_INF


# ------------------------------------------------------------------ top-k --


@pytest.mark.parametrize("content", C.TOPK_CONTENTS)
def test_topk_oracle_is_a_plain_sort(content):
    """The oracle against sorted() per row, and check_topk accepts what
    torch.topk itself returns once unfilled slots are marked -1."""
    for nq, m, k in C.TOPK_SHAPES:
        if m > 300:
            continue
        s = C.topk_scores(content, nq, m, k)
        assert s.shape == (nq, m) and s.dtype == torch.float32
        ref = C.topk_oracle(s, k)
        for q in range(nq):
            row = [NEG if math.isnan(v) else v for v in s[q].tolist()]
            assert ref[q].tolist() == sorted(row, reverse=True)[:k]
        clean = torch.where(torch.isnan(s), torch.full_like(s, C.NEG_INF), s)
        vals, idx = torch.topk(clean, k, dim=1)
        idx = torch.where(vals > C.NEG_INF, idx, torch.full_like(idx, -1))
        C.check_topk(s, k, vals, idx)


def test_topk_contents_have_their_edges():
    for nq, m, k in C.TOPK_SHAPES:
        if nq == 0:
            continue
        s = C.topk_scores("all_equal", nq, m, k)
        assert bool((s == s[0, 0]).all())
        s = C.topk_scores("heavy_ties", nq, m, k)
        assert set(s.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        s = C.topk_scores("few_finite", nq, m, k)
        finite = torch.isfinite(s).sum(1).tolist()
        counts = C.few_finite_counts(k)
        assert finite == [counts[q % len(counts)] for q in range(nq)]
        assert bool((s[~torch.isfinite(s)] == NEG).all())
        assert not C.topk_scores("transposed", nq, m, k).is_contiguous() or min(nq, m) == 1
        if m >= 6:
            s = C.topk_scores("inf_and_lowest", nq, m, k)
            assert bool((s == float("inf")).any(1).all())
            assert bool((s == C.F32_LOWEST).any(1).all())
            s = C.topk_scores("nan", nq, m, k)
            assert bool(torch.isnan(s).any(1).all())
            assert bool(torch.isfinite(s).any(1).all())
    # with 3 or more queries every count of finite entries appears
    assert C.few_finite_counts(32) == [0, 1, 31]
    assert C.few_finite_counts(1) == [0]


def test_check_topk_rejects_wrong_results():
    s = C.topk_scores("few_finite", 3, 33, 32)
    vals = C.topk_oracle(s, 32)
    idx = torch.topk(s, 32, dim=1).indices
    good = torch.where(vals > NEG, idx, torch.full_like(idx, -1))
    C.check_topk(s, 32, vals, good)
    # a finite sentinel in an unfilled slot
    bad = torch.where(vals > NEG, vals, torch.full_like(vals, -3.4e38))
    with pytest.raises(AssertionError):
        C.check_topk(s, 32, bad, good)
    # an index for an unfilled slot
    with pytest.raises(AssertionError):
        C.check_topk(s, 32, vals, idx.clamp(min=0))
    # a repeated index
    s = C.topk_scores("all_equal", 5, 255, 7)
    vals = C.topk_oracle(s, 7)
    with pytest.raises(AssertionError):
        C.check_topk(s, 7, vals, torch.zeros(5, 7, dtype=torch.int64))


# -------------------------------------------------------------------- ANN --


def test_ann_scores_are_small_integers():
    for case in (C.ann_flat_case, C.ann_ivf_case, C.ann_lsh_case):
        keys, vecs, deleted, queries, k = case()
        assert C.ANN_METRIC != "cos"
        assert torch.equal(vecs, vecs.round()) and torch.equal(queries, queries.round())
        worst = max(abs(s) for row in C.exact_scores(vecs, queries) for s in row)
        assert worst < 2**24
        assert 0 in deleted.tolist(), "row 0 must be dead: a clamped -1 points at it"
        assert len({tuple(r) for r in keys.tolist()}) == keys.shape[0]


def test_flat_case_on_cpu():
    from pathway_amd.engine.ann import FlatIndexState

    keys, vecs, deleted, queries, k = C.ann_flat_case()
    st = C.build_ann_state(FlatIndexState("cpu", C.ANN_METRIC), keys, vecs, deleted)
    # tombstoned, not compacted: the dead rows stay in the scored matrix
    assert st.keys.shape[0] == 40 and st.dead == 10 and len(st) < k < 40
    ids, scores, valid = st.search(queries, k)
    assert valid.sum(1).tolist() == [30] * 3
    C.check_ann_invariants(keys, vecs, deleted, queries, ids, scores, valid)
    # all live rows come back, so the result is the exact ranking
    exact = C.exact_scores(vecs, queries)
    dead = set(deleted.tolist())
    for q, row in enumerate(C.hits(ids, scores, valid)):
        assert sorted(s for s, _, _ in row) == sorted(
            exact[q][i] for i in range(40) if i not in dead
        )


def test_ivf_case_first_query_has_fewer_than_k_candidates():
    keys, vecs, deleted, queries, k = C.ann_ivf_case()
    st = C.build_ann_state(C.make_ivf_state("cpu"), keys, vecs, deleted)
    assert st.centroids is not None and st.clustered == 40 and st.dead == 3
    sizes = (st.list_offsets[1:] - st.list_offsets[:-1]).tolist()
    assert sorted(sizes) == [2, 38]
    far_list = sizes.index(2)
    rows = st.list_rows[st.list_offsets[far_list] : st.list_offsets[far_list + 1]]
    assert sorted(rows.tolist()) == sorted(C.IVF_FAR_ROWS)
    probe = st._scores_against(queries, st.centroids).argmax(1).tolist()
    assert probe == [far_list, 1 - far_list]
    assert 2 < k < 38 - 3
    ids, scores, valid = st.search(queries, k)
    assert scores.shape == (2, k)
    assert valid.sum(1).tolist() == [2, k]
    C.check_ann_invariants(keys, vecs, deleted, queries, ids, scores, valid)


def test_lsh_case_has_short_and_full_queries():
    keys, vecs, deleted, queries, k = C.ann_lsh_case()
    st = C.build_ann_state(C.make_lsh_state("cpu"), keys, vecs, deleted)
    ids, scores, valid = st.search(queries, k)
    # wider than k, or the device search would not take the kernel
    assert scores.shape[1] == k
    counts = valid.sum(1).tolist()
    assert max(counts) == k and min(counts) < k, counts
    C.check_ann_invariants(keys, vecs, deleted, queries, ids, scores, valid)


def test_ann_invariants_reject_a_bogus_hit():
    keys, vecs, deleted, queries, k = C.ann_ivf_case()
    st = C.build_ann_state(C.make_ivf_state("cpu"), keys, vecs, deleted)
    ids, scores, valid = st.search(queries, k)
    # what an unfilled device slot used to look like: row 0's key, "valid"
    scores = scores.clone()
    scores[0, 2:] = -3.4e38
    with pytest.raises(AssertionError):
        C.check_ann_invariants(
            keys, vecs, deleted, queries, ids, scores, scores > C.NEG_INF
        )


# ------------------------------------------------------------------- GEMM --


@pytest.mark.parametrize("shape", list(C.GEMM_SHAPES))
def test_gemm_results_are_bf16_values(shape):
    a, bt, bias, c, cb = C.ternary_case(*shape)
    M, N, K = shape
    assert a.shape == (M, K) and bt.shape == (N, K) and bias.shape == (N,)
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert set(bt.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert int(bias.abs().max()) <= 8 and torch.equal(bias, bias.round())
    # the condition under which the device result must be bit-exact
    assert int(c.abs().max()) <= 256 and int(cb.abs().max()) <= 256
    for t in (c, cb):
        assert torch.equal(t.to(torch.bfloat16).to(torch.int64), t)
    # the reference against a float64 product of the same inputs
    assert torch.equal((a.double() @ bt.double().T).to(torch.int64), c)
    # inside the range GELU_ATOL was measured over
    assert int(cb.abs().max()) <= C.GELU_RANGE
    assert c.count_nonzero() > c.numel() // 2


def test_dense_case_is_asymmetric():
    a, bt, c, want = C.dense_case()
    M, N, K = C.DENSE_SHAPE
    assert a.shape == (M, K) and bt.shape == (N, K)
    assert torch.equal(a.double() @ bt.double().T, c.double())
    # a transposed, row-shifted or column-shifted result is a different one
    assert not torch.equal(c[:N, :M], c.T[:N, :M])
    assert not torch.equal(c[1:], c[:-1]) and not torch.equal(c[:, 1:], c[:, :-1])
    assert not torch.equal(c[:-1, 1:], c[1:, :-1])
    assert c.count_nonzero() > c.numel() // 2
    assert torch.equal(want.to(torch.float64), c.to(torch.float64).to(torch.bfloat16).double())


def test_gelu_atol_is_measured():
    worst = C.gelu_fp32_worst(-C.GELU_RANGE, C.GELU_RANGE)
    assert worst <= C.GELU_FP32_WORST
    assert worst >= C.GELU_FP32_WORST / 2, "the recorded figure is stale"
    assert C.GELU_ATOL == 4 * C.GELU_FP32_WORST
    # check_gelu accepts the float32 formula rounded to bf16 and rejects a
    # result that is one bf16 step off
    x = torch.arange(-C.GELU_RANGE, C.GELU_RANGE + 1)
    got = C.gelu_kernel_formula_f32(x).to(torch.bfloat16)
    C.check_gelu(got, x)
    off = got.clone()
    assert off[C.GELU_RANGE + 3].item() == 3.0  # gelu(3) = 2.996
    off[C.GELU_RANGE + 3] = 3.015625
    with pytest.raises(AssertionError):
        C.check_gelu(off, x)

"""GPU tests of the top-k and bf16 GEMM kernels at their edges: top-k
against torch.topk on the CPU copy of the same scores, GEMM bit-exact
against an int64 matmul.  Inputs, oracles and the derivation of the GELU
bound are in tests/topk_gemm_cases.py."""

import pytest
import torch

from tests import topk_gemm_cases as C

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


# ------------------------------------------------------------------ top-k --


@gpu
@requires_cuda
@pytest.mark.parametrize("content", C.TOPK_CONTENTS)
def test_topk_matches_torch(content):
    from pathway_amd import ops

    for nq, m, k in C.TOPK_SHAPES:
        scores = C.topk_scores(content, nq, m, k)
        vals, idx = ops.topk_gpu(scores.to(DEV), k)
        try:
            C.check_topk(scores, k, vals.cpu(), idx.cpu())
        except AssertionError as e:
            raise AssertionError(f"{content} {(nq, m, k)}: {e}") from e


@gpu
@requires_cuda
def test_topk_unfilled_slots_are_minus_inf_minus_one():
    from pathway_amd import ops

    scores = torch.full((3, 40), C.NEG_INF)
    scores[1, 39] = C.F32_LOWEST
    scores[2, 5] = float("nan")
    vals, idx = ops.topk_gpu(scores.to(DEV), 4)
    assert vals.cpu().tolist() == [
        [C.NEG_INF] * 4,
        [C.F32_LOWEST] + [C.NEG_INF] * 3,
        [C.NEG_INF] * 4,
    ]
    assert idx.cpu().tolist() == [[-1] * 4, [39, -1, -1, -1], [-1] * 4]


@gpu
@requires_cuda
def test_topk_k_over_32_raises():
    from pathway_amd import ops

    with pytest.raises(RuntimeError):
        ops.topk_gpu(torch.zeros(2, 64, device=DEV), 33)


# ------------------------------------------------------------------- GEMM --


@gpu
@requires_cuda
@pytest.mark.parametrize("shape", list(C.GEMM_SHAPES), ids=str)
def test_gemm_bit_exact(shape):
    from pathway_amd import ops

    a, bt, bias, c, cb = C.ternary_case(*shape)
    a_d, bt_d = a.to(DEV), bt.to(DEV)
    got = ops.gemm_bias_act_gpu(a_d, bt_d, None, act="none").cpu()
    assert got.dtype == torch.bfloat16 and got.shape == c.shape
    assert torch.equal(got, c.to(torch.bfloat16)), (
        f"{int((got.to(torch.int64) != c).sum())} wrong elements without bias"
    )
    got = ops.gemm_bias_act_gpu(a_d, bt_d, bias.to(DEV), act="none").cpu()
    assert torch.equal(got, cb.to(torch.bfloat16)), (
        f"{int((got.to(torch.int64) != cb).sum())} wrong elements with bias"
    )


@gpu
@requires_cuda
@pytest.mark.parametrize("shape", list(C.GEMM_SHAPES), ids=str)
def test_gemm_gelu_within_half_ulp(shape):
    from pathway_amd import ops

    a, bt, bias, c, cb = C.ternary_case(*shape)
    got = ops.gemm_bias_act_gpu(a.to(DEV), bt.to(DEV), bias.to(DEV), act="gelu")
    C.check_gelu(got.cpu(), cb)
    got = ops.gemm_bias_act_gpu(a.to(DEV), bt.to(DEV), None, act="gelu")
    C.check_gelu(got.cpu(), c)


@gpu
@requires_cuda
def test_gemm_dense_asymmetric():
    from pathway_amd import ops

    a, bt, c, want = C.dense_case()
    got = ops.gemm_bias_act_gpu(a.to(DEV), bt.to(DEV), None, act="none").cpu()
    assert torch.equal(got, want), (
        f"{int((got != want).sum())} of {want.numel()} elements wrong"
    )


@gpu
@requires_cuda
@pytest.mark.parametrize("shape", C.GEMM_EMPTY_SHAPES, ids=str)
def test_gemm_empty_output(shape):
    from pathway_amd import ops

    M, N, K = shape
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    bt = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    bias = torch.zeros(N, device=DEV)
    for act in ("none", "gelu"):
        got = ops.gemm_bias_act_gpu(a, bt, bias, act=act)
        assert got.shape == (M, N) and got.dtype == torch.bfloat16
        assert got.device == a.device

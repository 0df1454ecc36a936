"""Inputs and oracles for the top-k, ANN and bf16 GEMM device tests
(tests/test_topk_gemm_gpu.py, tests/test_ann_gpu.py), checked on the CPU by
tests/test_topk_gemm_cpu.py.

Top-k.  The oracle is torch.topk on the CPU copy of the scores with NaN
replaced by -inf: the kernel never selects a NaN or a -inf, an unfilled slot
is (-inf, -1), and torch.topk values such a slot -inf too.  Selection copies
values, so the values compare with torch.equal.  Ties rank in no defined
order, so indices are checked through the scores they point at.

ANN.  Vectors and queries are small integers and the metric is the negated
squared distance, so every score is an integer that float32 holds exactly
on either device, whatever the order of summation.

GEMM.  A and B^T are ternary (+1 and -1 with probability 1/8 each, else 0)
and the bias is an integer in [-8, 8]: every product and partial sum is an
integer far below 2^24, float32 accumulation is exact in any order, and the
int64 matmul on the CPU is the exact result.  tests/test_topk_gemm_cpu.py
asserts max|C| <= 256 for every shape, so every result is a bf16 value and
the device result must be torch.equal to it (measured maxima, with bias:
(256,256,1536) 44, (128,256,512) 32, (128,128,576) 31, (128,128,640) 30).

GELU.  The reference is the float64 GELU of the exact integer
pre-activation and the bound is |got - ref| <= 2^-8 |ref| + GELU_ATOL.
2^-8 |ref| is half a bf16 ulp, from the final rounding.  GELU_ATOL covers
the float32 cancellation in 1 + erf(x / sqrt 2) at negative x: the kernel's
own float32 formula, evaluated with torch on the CPU against float64 over
the integers in [-64, 64] (the pre-activations of GEMM_SHAPES lie in
[-44, 44]), differs by 1.54e-7 at the most.  GELU_ATOL is four
times that, because the device erff may differ from the host's by a few ulp.
"""

from __future__ import annotations

import functools
import math

import torch

NEG_INF = float("-inf")
F32_LOWEST = torch.finfo(torch.float32).min

# ------------------------------------------------------------------ top-k --

#: (nq, m, k): one element; k = 32 with one more candidate than k; one
#: thread short of, at and over the 256-thread block with odd and full k;
#: 33 candidates per thread; many blocks; no rows
TOPK_SHAPES = [
    (1, 1, 1),
    (3, 33, 32),
    (5, 255, 7),
    (5, 256, 32),
    (5, 257, 32),
    (2, 8193, 32),
    (300, 100, 5),
    (0, 10, 3),
]

TOPK_CONTENTS = [
    "normal",
    "all_equal",
    "heavy_ties",
    "inf_and_lowest",
    "few_finite",
    "nan",
    "transposed",
]


def few_finite_counts(k: int) -> list[int]:
    """The numbers of finite entries a 'few_finite' row may have: 0, 1, k-1."""
    return sorted({0, min(1, k - 1), k - 1})


def topk_scores(content: str, nq: int, m: int, k: int) -> torch.Tensor:
    """(nq, m) float32 scores on the CPU; 'transposed' is not contiguous."""
    g = torch.Generator().manual_seed(1000 * nq + 10 * m + k)
    normal = torch.randn(nq, m, generator=g)
    if content == "normal":
        return normal
    if content == "all_equal":
        return torch.full((nq, m), 1.5)
    if content == "heavy_ties":
        return torch.randint(-2, 3, (nq, m), generator=g).to(torch.float32)
    if content == "inf_and_lowest":
        s = normal.clone()
        for q in range(nq):
            s[q, (7 * q) % m] = float("inf")
            s[q, (7 * q + 3) % m] = F32_LOWEST
            s[q, (7 * q + 5) % m] = NEG_INF
        return s
    if content == "few_finite":
        s = torch.full((nq, m), NEG_INF)
        counts = few_finite_counts(k)
        for q in range(nq):
            j = counts[q % len(counts)]
            # spread over the threads' strided slices, last element included
            pos = [(m - 1 - 37 * t) % m for t in range(j)]
            assert len(set(pos)) == j
            s[q, pos] = normal[q, pos]
        return s
    if content == "nan":
        s = normal.clone()
        s[:, ::3] = float("nan")
        return s
    if content == "transposed":
        return torch.randn(m, nq, generator=g).t()
    raise ValueError(content)


def topk_oracle(scores: torch.Tensor, k: int) -> torch.Tensor:
    """(nq, k) values torch.topk gives once NaN counts as -inf."""
    clean = torch.where(torch.isnan(scores), torch.full_like(scores, NEG_INF), scores)
    return torch.topk(clean, k, dim=1).values


def check_topk(scores: torch.Tensor, k: int, vals: torch.Tensor, idx: torch.Tensor):
    """Every assertion of the top-k tests, on CPU tensors."""
    nq, m = scores.shape
    assert vals.shape == (nq, k) and idx.shape == (nq, k)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64
    ref = topk_oracle(scores, k)
    assert torch.equal(vals, ref), "values differ from torch.topk"
    if nq == 0:
        return
    filled = idx >= 0
    assert torch.equal(filled, vals > NEG_INF), "idx < 0 exactly where unfilled"
    assert bool((idx[~filled] == -1).all())
    assert bool((idx[filled] < m).all()), "index out of range"
    picked = scores.contiguous().gather(1, idx.clamp(min=0))
    assert torch.equal(picked[filled], vals[filled]), "idx does not point at vals"
    assert bool((vals[:, 1:] <= vals[:, :-1]).all()), "values not non-increasing"
    for q in range(nq):
        row = idx[q][filled[q]].tolist()
        assert len(set(row)) == len(row), f"row {q}: repeated index"


# -------------------------------------------------------------------- ANN --

#: anything but "cos": score = -(squared distance)
ANN_METRIC = "l2"
ANN_DIM = 4


def _ann_keys(n: int) -> torch.Tensor:
    return torch.stack(
        [
            torch.arange(1, n + 1, dtype=torch.int64),
            torch.arange(1, n + 1, dtype=torch.int64) * 1000 + 7,
        ],
        dim=1,
    )


def _near_points(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (n, ANN_DIM), generator=g).to(torch.float32)


def ann_flat_case():
    """40 rows, 10 of them deleted (row 0 among them), k = 32 > 30 live."""
    keys = _ann_keys(40)
    vecs = _near_points(40, 11)
    deleted = torch.arange(0, 40, 4)
    queries = torch.tensor(
        [[0, 0, 0, 0], [1, -2, 3, 0], [4, 4, -4, 1]], dtype=torch.float32
    )
    return keys, vecs, deleted, queries, 32


#: rows of ann_ivf_case() that form the far cluster
IVF_FAR_ROWS = (5, 17)
IVF_K = 8


def ann_ivf_case():
    """38 rows around the origin and 2 far away, 3 near rows deleted (row 0
    among them).  With nlist = 2 and nprobe = 1 the first query probes the
    far list (2 rows < k) and the second the near list (35 live rows > k)."""
    keys = _ann_keys(40)
    vecs = _near_points(40, 12)
    vecs[IVF_FAR_ROWS[0]] = torch.tensor([60.0, 60.0, 60.0, 60.0])
    vecs[IVF_FAR_ROWS[1]] = torch.tensor([61.0, 60.0, 59.0, 60.0])
    deleted = torch.tensor([0, 9, 30])
    queries = torch.tensor([[60, 60, 60, 59], [0, 1, 0, -1]], dtype=torch.float32)
    return keys, vecs, deleted, queries, IVF_K


LSH_K = 8


def ann_lsh_case():
    """40 rows, 10 deleted (row 0 among them); 2 tables of 3 bits, so a
    query's buckets hold from none to a dozen rows around k = 8."""
    keys = _ann_keys(40)
    vecs = _near_points(40, 13)
    deleted = torch.arange(0, 40, 4)
    queries = _near_points(12, 14)
    return keys, vecs, deleted, queries, LSH_K


def build_ann_state(state, keys, vecs, deleted):
    """Add every row in one update, then delete `deleted` in a second."""
    dev = state.device
    n = keys.shape[0]
    state.update(keys.to(dev), vecs.to(dev), torch.ones(n, dtype=torch.int64, device=dev))
    if deleted.numel():
        state.update(
            keys[deleted].to(dev),
            vecs[deleted].to(dev),
            -torch.ones(deleted.numel(), dtype=torch.int64, device=dev),
        )
    return state


def make_ivf_state(device):
    from pathway_amd.engine.ann import IvfFlatState

    return IvfFlatState(
        device, ANN_METRIC, nlist=2, nprobe=1, min_train=8,
        rebuild_every=10**9, kmeans_iters=8,
    )


def make_lsh_state(device):
    from pathway_amd.engine.ann import LshState

    return LshState(device, ANN_METRIC, n_or=2, n_and=3, seed=5151)


def exact_scores(vecs: torch.Tensor, queries: torch.Tensor) -> list[list[int]]:
    """-(squared distance) of every query to every row, as Python ints."""
    v = vecs.to(torch.int64)
    q = queries.to(torch.int64)
    d = q.unsqueeze(1) - v.unsqueeze(0)
    return (-(d * d).sum(-1)).tolist()


def hits(ids, scores, valid) -> list[list[tuple]]:
    """Per query the valid hits as (score, key0, key1), sorted: the order
    of ties is undefined."""
    ids, scores, valid = ids.cpu(), scores.cpu(), valid.cpu()
    out = []
    for q in range(scores.shape[0]):
        row = [
            (scores[q, j].item(), ids[q, j, 0].item(), ids[q, j, 1].item())
            for j in range(scores.shape[1])
            if valid[q, j]
        ]
        out.append(sorted(row))
    return out


def check_ann_invariants(keys, vecs, deleted, queries, ids, scores, valid):
    """What any search result must satisfy, whichever rows the index chose
    to look at."""
    scores_c, valid_c = scores.cpu(), valid.cpu()
    dead = set(deleted.tolist())
    live = {tuple(keys[i].tolist()): i for i in range(keys.shape[0]) if i not in dead}
    exact = exact_scores(vecs, queries)
    assert bool((scores_c[~valid_c] == NEG_INF).all()), "invalid slot with a score"
    assert int(valid_c.sum(1).max()) <= len(live)
    for q, row in enumerate(hits(ids, scores, valid)):
        got_keys = [(k0, k1) for _, k0, k1 in row]
        assert len(set(got_keys)) == len(got_keys), f"query {q}: repeated key"
        for s, k0, k1 in row:
            assert (k0, k1) in live, f"query {q}: hit {(k0, k1)} is not a live key"
            assert s == exact[q][live[(k0, k1)]], f"query {q}: wrong score"


# ------------------------------------------------------------------- GEMM --

#: (M, N, K) -> the path it exists for
GEMM_SHAPES = {
    (128, 128, 64): "one interior tile, one K-tile, DMA staging",
    (1, 1, 8): "edge tile only",
    (127, 129, 64): "edge tiles only",
    (129, 128, 64): "interior tile plus a 1-row edge tile",
    (128, 128, 72): "K tail of one whole 8-chunk",
    (128, 128, 65): "K tail of one element, misaligned rows",
    (128, 128, 100): "K tail, misaligned rows, interior tile",
    (128, 256, 512): "single buffer at its upper limit of 8 K-tiles",
    (128, 128, 576): "double buffer, odd K-tile count",
    (128, 128, 640): "double buffer, even K-tile count",
    (256, 256, 1536): "encoder shape",
}

GEMM_EMPTY_SHAPES = [(0, 128, 64), (128, 0, 64)]

DENSE_SHAPE = (129, 130, 72)

#: worst |float32 formula - float64 GELU| over the integers in [-64, 64]
GELU_FP32_WORST = 1.54e-7
GELU_ATOL = 4 * GELU_FP32_WORST
GELU_RANGE = 64


@functools.lru_cache(maxsize=None)
def ternary_case(M: int, N: int, K: int):
    """(A (M,K) bf16, B^T (N,K) bf16, bias (N,) f32, C int64, C + bias int64)."""
    # the 3 makes the one product of (1, 1, 8) non-zero
    g = torch.Generator().manual_seed(M * 1_000_003 + N * 1009 + K + 3)

    def tern(r, c):
        u = torch.randint(0, 8, (r, c), generator=g)
        return (u == 0).to(torch.int64) - (u == 1).to(torch.int64)

    a, bt = tern(M, K), tern(N, K)
    bias = torch.randint(-8, 9, (N,), generator=g)
    c = a @ bt.T
    return (
        a.to(torch.bfloat16),
        bt.to(torch.bfloat16),
        bias.to(torch.float32),
        c,
        c + bias,
    )


def dense_case():
    """A[i,k] = ((3i + 5k) % 7) - 3, B[k,j] = ((2k + 7j) % 5) - 2: no two
    rows, columns or K positions are interchangeable.  The expected result
    is the int64 product rounded to bf16 (round to nearest even)."""
    M, N, K = DENSE_SHAPE
    i = torch.arange(M).unsqueeze(1)
    k = torch.arange(K).unsqueeze(0)
    a = (3 * i + 5 * k) % 7 - 3
    kk = torch.arange(K).unsqueeze(1)
    j = torch.arange(N).unsqueeze(0)
    b = (2 * kk + 7 * j) % 5 - 2
    c = a @ b
    assert int(c.abs().max()) < 2**24
    want = c.to(torch.float32).to(torch.bfloat16)
    return a.to(torch.bfloat16), b.T.contiguous().to(torch.bfloat16), c, want


def gelu_f64(x: torch.Tensor) -> torch.Tensor:
    x = x.to(torch.float64)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_kernel_formula_f32(x: torch.Tensor) -> torch.Tensor:
    """pw_gelu of pw_kernels.hip, operation by operation, in float32."""
    x = x.to(torch.float32)
    return 0.5 * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752, dtype=torch.float32)))


def gelu_fp32_worst(lo: int, hi: int) -> float:
    x = torch.arange(lo, hi + 1)
    return float((gelu_kernel_formula_f32(x).to(torch.float64) - gelu_f64(x)).abs().max())


def check_gelu(got: torch.Tensor, pre: torch.Tensor):
    """got (bf16, CPU) against the float64 GELU of the integer `pre`."""
    ref = gelu_f64(pre)
    err = (got.to(torch.float64) - ref).abs()
    bound = ref.abs() * 2.0**-8 + GELU_ATOL
    worst = (err - bound).max().item()
    assert bool((err <= bound).all()), f"GELU misses its bound by {worst:.3e}"

"""GPU tests of ops.seg_sum_f64_gpu (pw_seg_sum_f64): segmented
double-double sums read through a permutation, against math.fsum under the
bound derived in tests/dd_cases.py."""

import math
import random

import pytest
import torch

from tests.dd_cases import check_sum, values

gpu = pytest.mark.gpu
requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


def _chunk():
    from pathway_amd import ops

    return ops.SEG_SUM_F64_CHUNK


def _lengths():
    T = _chunk()
    return [1, 2, 63, 64, 65, 257, T - 1, T, T + 1, 2 * T + 3]


class Batch:
    """Segments of given values, laid out through a shuffled permutation:
    column[perm[i]] is the i-th value in segment order."""

    def __init__(self, segs, seed, ncol=1, shuffle=True):
        rng = random.Random(seed)
        self.segs = segs  # per column: list of per-segment value lists
        flat = [[x for seg in col for x in seg] for col in segs]
        n = len(flat[0])
        self.n = n
        perm = list(range(n))
        if shuffle:
            rng.shuffle(perm)
        self.perm = torch.tensor(perm, dtype=torch.int64)
        self.cols = []
        for f in flat:
            col = torch.empty(n, dtype=torch.float64)
            col[self.perm] = torch.tensor(f, dtype=torch.float64)
            self.cols.append(col.to(DEV))
        starts = [0]
        for seg in segs[0]:
            starts.append(starts[-1] + len(seg))
        self.seg_start = torch.tensor(starts, dtype=torch.int64, device=DEV)

    def perm_as(self, kind):
        if kind == "int64":
            return self.perm.to(DEV)
        assert kind == "int32"
        return self.perm.to(torch.int32).to(DEV)  # n < 2^31: same bits as uint32

    def run(self, kind="int32", cols=None, lo_cols=None):
        from pathway_amd import ops

        hi, lo = ops.seg_sum_f64_gpu(
            self.perm_as(kind), self.seg_start, cols or self.cols, lo_cols
        )
        return [h.cpu() for h in hi], [l.cpu() for l in lo]


@pytest.fixture(scope="module")
def mixed_lengths():
    rng = random.Random(3)
    segs = [values(rng, L) for L in _lengths()]
    rng.shuffle(segs)
    b = Batch([segs], seed=4)
    assert b.n % 64 != 0
    return b


def _check_batch(b, hi, lo, col=0):
    for s, seg in enumerate(b.segs[col]):
        h, l = float(hi[s]), float(lo[s])
        assert h == h + l, ("not normalised", s, len(seg))
        check_sum(h + l, seg, what=(s, len(seg)))


@gpu
@requires_cuda
def test_segment_lengths_around_the_chunk(mixed_lengths):
    hi, lo = mixed_lengths.run("int32")
    _check_batch(mixed_lengths, hi[0], lo[0])
    # twice the same input: the same bits
    hi2, lo2 = mixed_lengths.run("int32")
    assert torch.equal(hi[0], hi2[0]) and torch.equal(lo[0], lo2[0])


@gpu
@requires_cuda
def test_permutation_kinds(mixed_lengths):
    from pathway_amd import ops

    b = mixed_lengths
    ref = b.run("int32")
    hi, lo = b.run("int64")
    _check_batch(b, hi[0], lo[0])
    assert torch.equal(hi[0], ref[0][0]) and torch.equal(lo[0], ref[1][0])
    # identity: the column already in segment order
    ordered = b.cols[0].index_select(0, b.perm.to(DEV))
    hi, lo = ops.seg_sum_f64_gpu(None, b.seg_start, [ordered])
    _check_batch(b, hi[0].cpu(), lo[0].cpu())
    assert torch.equal(hi[0].cpu(), ref[0][0]) and torch.equal(lo[0].cpu(), ref[1][0])


@gpu
@requires_cuda
def test_position_independence():
    T = _chunk()
    rng = random.Random(21)
    probes = [values(rng, L) for L in (5, 8, 9, 257, T, 2 * T + 3)]
    for probe in probes:
        first = Batch([[probe, values(rng, 7)]], seed=5)
        hi_a, lo_a = first.run()
        filler = [values(rng, L) for L in (3, 1, T + 70, 2, 65, 1, 1)]
        middle = Batch([filler[:5] + [probe] + filler[5:]], seed=6)
        hi_b, lo_b = middle.run()
        assert hi_a[0][0].item() == hi_b[0][5].item(), len(probe)
        assert lo_a[0][0].item() == lo_b[0][5].item(), len(probe)
        assert float(hi_a[0][0]).hex() == float(hi_b[0][5]).hex()


@gpu
@requires_cuda
def test_partial_double_doubles_with_low_parts():
    """Summing k partial double-doubles: the fsum of all their parts."""
    T = _chunk()
    rng = random.Random(31)
    his, los = [], []
    for L in (1, 4, 70, T + 5):
        h = values(rng, L)
        l = [rng.uniform(-0.5, 0.5) * math.ulp(x) for x in h]
        his.append(h)
        los.append(l)
    b = Batch([his, los], seed=7)
    hi, lo = b.run(cols=[b.cols[0]], lo_cols=[b.cols[1]])
    for s, (h, l) in enumerate(zip(his, los)):
        got = float(hi[0][s]) + float(lo[0][s])
        parts = h + l
        # one add per pair, the bound's sum|x| over all the parts
        check_sum(got, parts, n_adds=len(h), what=s)


@gpu
@requires_cuda
def test_two_columns_equal_two_calls():
    T = _chunk()
    rng = random.Random(41)
    lens = (2, 9, 300, T + 1, 1)
    b = Batch([[values(rng, L) for L in lens], [values(rng, L) for L in lens]], seed=8)
    hi, lo = b.run()
    for c in range(2):
        h1, l1 = b.run(cols=[b.cols[c]])
        assert torch.equal(hi[c], h1[0]) and torch.equal(lo[c], l1[0])
        _check_batch(b, hi[c], lo[c], col=c)


@gpu
@requires_cuda
def test_non_finite_inputs():
    T = _chunk()
    rng = random.Random(51)
    inf = math.inf
    segs = []
    for L in (6, 100, T + 9):
        plain = values(rng, L)
        with_inf = values(rng, L)
        with_inf[L // 2] = inf
        both = values(rng, L)
        both[1], both[L - 2] = inf, -inf
        with_nan = values(rng, L)
        with_nan[L - 1] = math.nan
        segs += [plain, with_inf, values(rng, L), both, with_nan, values(rng, L)]
    b = Batch([segs], seed=9)
    hi, lo = b.run()
    for s, seg in enumerate(segs):
        h, l = float(hi[0][s]), float(lo[0][s])
        kind = s % 6
        if kind == 1:
            assert h == inf and l == 0.0, s
        elif kind in (3, 4):
            assert math.isnan(h) and l == 0.0, s
        else:
            check_sum(h + l, seg, what=s)


@gpu
@requires_cuda
def test_many_one_row_segments_and_one_long_segment():
    """The two shapes the grid has to spread: every row its own segment,
    and all rows one segment of many chunks."""
    from pathway_amd import ops

    T = _chunk()
    rng = random.Random(61)
    n = 8 * T + 37
    xs = values(rng, n)
    col = torch.tensor(xs, dtype=torch.float64, device=DEV)
    each = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    hi, lo = ops.seg_sum_f64_gpu(None, each, [col])
    assert torch.equal(hi[0], col) and not bool(lo[0].any())
    whole = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    hi, lo = ops.seg_sum_f64_gpu(None, whole, [col])
    check_sum(float(hi[0][0]) + float(lo[0][0]), xs)

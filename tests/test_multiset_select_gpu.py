"""GPU tests of the segmented kernels behind the multiset reducers:
seg_select_gpu (pw_seg_select: the best row of every range) and
seg_distinct_gpu (pw_seg_distinct: distinct 64-bit values per range).  Both
are checked against a plain Python model written here that loops over
range(lo, hi), skips weights <= 0 and applies the documented rules.  All
comparisons are exact."""

import functools
import random

import pytest
import torch

gpu = pytest.mark.gpu
requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
NAN = float("nan")


def _ops():
    from pathway_amd import ops

    return ops


# ------------------------------------------------------------- the model --

def _better(ka, kb, mode):
    """ka strictly beats the current best kb (an equal key keeps the
    earlier row)."""
    ops = _ops()
    an, bn = ka != ka, kb != kb
    if an or bn:
        return an and not bn
    return ka < kb if mode == ops.SEG_MIN else ka > kb


def _model_select(lo, hi, w, key, mode):
    ops = _ops()
    out = []
    for a, b in zip(lo, hi):
        best = -1
        for r in range(a, b):
            if w[r] <= 0:
                continue
            if best < 0:
                best = r
                if mode == ops.SEG_FIRST:
                    break
            elif _better(key[r], key[best], mode):
                best = r
        out.append(best)
    return out


def _model_distinct(lo, hi, w, vals):
    """(count, first, status).  A range is given up (count and first None)
    when it holds more distinct values than 64 passes of GC_BUCKET_MAX_LOAD
    * capacity slots can: then some pass is over its share whatever the
    hash.  Up to three quarters of that, a pass of the 64 expects at most
    1536 of its 2048 slots with a deviation of about 39, so none is over
    its share; the cases here keep out of the band between the two."""
    ops = _ops()
    most = ops.SEG_DISTINCT_MAX_PASSES * int(
        ops.GC_BUCKET_MAX_LOAD * ops.SEG_DISTINCT_CAPACITY
    )
    out = []
    for a, b in zip(lo, hi):
        seen, first = set(), -1
        for r in range(a, b):
            if w[r] > 0:
                seen.add(vals[r])
                if first < 0:
                    first = r
        if len(seen) > most:
            out.append((None, None, 1))
        else:
            assert len(seen) <= most * 3 // 4, "a case the model cannot call"
            out.append((len(seen), first, 0))
    return out


# -------------------------------------------------------------- the store --

def _lengths():
    long_ = _ops().SEG_SELECT_LONG
    return [0, 1, 2, 63, 64, 65, 127, 128, 129, long_ - 1, long_, long_ + 1]


@functools.lru_cache(maxsize=None)
def _store():
    """One store for both kernels.  Rows [0, 300): weights alternate between
    positive and non-positive; [300, 400): every weight <= 0; the rest:
    random weights in [-2, 3].  Then one segment per length of _lengths().
    Returns (weights, segments) with segments a list of (lo, hi)."""
    rng = random.Random(9)
    w = [(1 if r % 2 else -(r % 3)) for r in range(300)]
    w += [-(r % 2) for r in range(100)]
    segs = [(0, 300), (300, 400), (250, 400), (299, 301)]
    for n in _lengths():
        segs.append((len(w), len(w) + n))
        w += [rng.randint(-2, 3) for _ in range(n)]
    segs.append((0, len(w)))  # the whole store
    return w, segs


@functools.lru_cache(maxsize=None)
def _queries(nq):
    """nq ranges in no order, one of them twice; the named segments come
    first as far as nq allows."""
    w, segs = _store()
    m = len(w)
    rng = random.Random(nq)
    qs = list(segs)
    rng.shuffle(qs)
    qs = qs[:nq]
    while len(qs) < nq - 1:
        a = rng.randrange(m)
        qs.append((a, min(m, a + rng.randrange(0, 200))))
    if len(qs) < nq:
        qs.append(qs[0])  # the same range queried twice
    rng.shuffle(qs)
    return [a for a, _ in qs], [b for _, b in qs]


def _dev(xs, dtype=torch.int64):
    return torch.tensor(xs, dtype=dtype, device=DEV)


def _keys(kind):
    w, _ = _store()
    m = len(w)
    rng = random.Random(kind)
    if kind == "int":
        # few distinct values: ties inside every range
        return [rng.randint(-5, 5) for _ in range(m)], torch.int64
    if kind == "int_extreme":
        pool = [I64_MIN, I64_MAX, 2**53 - 1, 2**53, 2**53 + 1, -(2**53) - 1, 0, -1]
        return [rng.choice(pool) for _ in range(m)], torch.int64
    if kind == "float":
        pool = [-0.0, 0.0, float("inf"), float("-inf"), 1.5, -2.5, 1e300]
        return [rng.choice(pool) for _ in range(m)], torch.float64
    if kind == "equal":
        return [7] * m, torch.int64
    if kind == "one_nan":
        # one NaN in the middle of the longest segment, on a positive row
        ks = [float(rng.randint(-9, 9)) for _ in range(m)]
        a, b = _store()[1][-2]
        r = next(r for r in range((a + b) // 2, b) if w[r] > 0)
        ks[r] = NAN
        return ks, torch.float64
    assert kind == "all_nan"
    return [NAN] * m, torch.float64


def _select_case(nq, mode, kind):
    ops = _ops()
    w, _ = _store()
    lo, hi = _queries(nq)
    key, dtype = (None, None) if kind is None else _keys(kind)
    got = ops.seg_select_gpu(
        _dev(lo), _dev(hi), _dev(w), None if key is None else _dev(key, dtype), mode
    )
    assert got.dtype == torch.int64 and got.shape == (nq,)
    want = _model_select(lo, hi, w, key, mode)
    assert got.cpu().tolist() == want
    return lo, hi, want


@gpu
@requires_cuda
@pytest.mark.parametrize("nq", [1, 65, 1000])
def test_select_first(nq):
    _select_case(nq, _ops().SEG_FIRST, None)


@gpu
@requires_cuda
@pytest.mark.parametrize("nq", [1, 65, 1000])
@pytest.mark.parametrize("kind", ["int", "int_extreme", "float"])
@pytest.mark.parametrize("mode", ["SEG_MIN", "SEG_MAX"])
def test_select_min_max(nq, kind, mode):
    lo, hi, want = _select_case(nq, getattr(_ops(), mode), kind)
    if nq == 1000:
        # the cases that must be in: an empty result and a chosen row
        assert -1 in want and any(s >= 0 for s in want)
        assert (300, 400) in set(zip(lo, hi))


@gpu
@requires_cuda
@pytest.mark.parametrize("mode", ["SEG_MIN", "SEG_MAX"])
def test_select_equal_keys_take_the_lowest_positive_row(mode):
    ops = _ops()
    lo, hi, want = _select_case(65, getattr(ops, mode), "equal")
    w, _ = _store()
    assert want == _model_select(lo, hi, w, None, ops.SEG_FIRST)


@gpu
@requires_cuda
@pytest.mark.parametrize("mode", ["SEG_MIN", "SEG_MAX"])
@pytest.mark.parametrize("kind", ["one_nan", "all_nan"])
def test_select_nan_beats_every_number(kind, mode):
    ops = _ops()
    lo, hi, want = _select_case(65, getattr(ops, mode), kind)
    w, segs = _store()
    key, _ = _keys(kind)
    if kind == "one_nan":
        (nan_row,) = [r for r, k in enumerate(key) if k != k]
        q = list(zip(lo, hi)).index(segs[-2])  # the long segment
        assert want[q] == nan_row
        q = list(zip(lo, hi)).index(segs[-1])  # the whole store
        assert want[q] == nan_row
    else:
        assert want == _model_select(lo, hi, w, None, ops.SEG_FIRST)


@gpu
@requires_cuda
def test_select_long_threshold_only_moves_work():
    """Every range through the second launch, and none: same rows."""
    ops = _ops()
    w, _ = _store()
    lo, hi = _queries(65)
    key, dtype = _keys("int")
    args = (_dev(lo), _dev(hi), _dev(w), _dev(key, dtype), ops.SEG_MAX)
    want = _model_select(lo, hi, w, key, ops.SEG_MAX)
    assert ops.seg_select_gpu(*args, long_rows=64).cpu().tolist() == want
    assert ops.seg_select_gpu(*args, long_rows=1 << 40).cpu().tolist() == want


@gpu
@requires_cuda
def test_select_checks_its_arguments():
    ops = _ops()
    lo, hi, w = _dev([0]), _dev([1]), _dev([1, 1])
    with pytest.raises(ValueError):
        ops.seg_select_gpu(lo, hi, w, None, ops.SEG_MIN)
    with pytest.raises(ValueError):
        ops.seg_select_gpu(lo, hi, w, _dev([1, 2], torch.int32), ops.SEG_MIN)
    with pytest.raises(ValueError):
        ops.seg_select_gpu(lo, hi, w, _dev([1, 2, 3]), ops.SEG_MAX)
    with pytest.raises(ValueError):
        ops.seg_select_gpu(lo, _dev([1, 2]), w, None, ops.SEG_FIRST)
    with pytest.raises(ValueError):
        ops.seg_select_gpu(lo.cpu(), hi, w, None, ops.SEG_FIRST)
    with pytest.raises(ValueError):
        ops.seg_distinct_gpu(lo, hi, w, _dev([1.0, 2.0], torch.float64))


# --------------------------------------------------------------- distinct --

def _distinct_check(lo, hi, w, vals):
    ops = _ops()
    count, first, status = ops.seg_distinct_gpu(_dev(lo), _dev(hi), _dev(w), _dev(vals))
    assert count.dtype == torch.int64 and first.dtype == torch.int64
    assert status.dtype == torch.int32
    want = _model_distinct(lo, hi, w, vals)
    got = list(zip(count.cpu().tolist(), first.cpu().tolist(), status.cpu().tolist()))
    assert [g[2] for g in got] == [x[2] for x in want]
    for g, x in zip(got, want):
        if x[2] == 0:
            assert g == x
    return want


@gpu
@requires_cuda
@pytest.mark.parametrize("nq", [1, 65, 1000])
@pytest.mark.parametrize("spread", [3, 50, 10**6])
def test_distinct_against_model(nq, spread):
    w, _ = _store()
    lo, hi = _queries(nq)
    rng = random.Random(spread)
    vals = [rng.randint(-spread, spread) for _ in w]
    want = _distinct_check(lo, hi, w, vals)
    assert all(x[2] == 0 for x in want)  # the whole store: up to 8 passes
    if nq == 1000:
        assert (0, -1, 0) in want


@functools.lru_cache(maxsize=None)
def _big_store():
    """Segments sized by the table: all distinct / all equal just under and
    just over half the capacity, two multi-pass ranges of 5x the capacity,
    the values -1 / 0 / INT64_MIN, one range with one distinct value too
    many for 64 passes, one as long with three values, and one that takes
    all 64 passes.  Weights are 1, 2, 3 in turn but for a few rows."""
    ops = _ops()
    cap = ops.SEG_DISTINCT_CAPACITY
    half = int(ops.GC_BUCKET_MAX_LOAD * cap)
    vals, segs = [], []

    def seg(vs):
        segs.append((len(vals), len(vals) + len(vs)))
        vals.extend(vs)

    base = 10**12
    for n in (half - 1, half, half + 1):
        seg([base + 17 * i for i in range(n)])  # all distinct
        seg([-(2**40)] * n)  # all equal
    seg([base * 3 + 5 * i for i in range(5 * cap)])
    seg([(i * 7) % 3 - 1 for i in range(5 * cap)])  # -1, 0, 1
    seg([-1, 0, I64_MIN, -1, I64_MIN, 0, 0])
    most = ops.SEG_DISTINCT_MAX_PASSES * half
    seg([base * 7 + i for i in range(most + 2)])
    seg([base * 8 + i % 3 for i in range(most + 2)])
    seg([base * 9 + i for i in range(40 * half + 1)])
    w = [1 + r % 3 for r in range(len(vals))]
    for a, _ in segs:
        w[a] = 0  # a first row that does not count
    return w, vals, segs


@gpu
@requires_cuda
def test_distinct_table_sizes_passes_and_give_up():
    ops = _ops()
    cap = ops.SEG_DISTINCT_CAPACITY
    half = int(ops.GC_BUCKET_MAX_LOAD * cap)
    w, vals, segs = _big_store()
    order = list(reversed(segs))
    lo, hi = [a for a, _ in order], [b for _, b in order]
    want = dict(zip(order, _distinct_check(lo, hi, w, vals)))
    counts = [want[s][0] for s in segs]
    assert counts[:6] == [half - 2, 1, half - 1, 1, half, 1]
    assert counts[6:9] == [5 * cap - 1, 3, 3]
    # only the range with 64 * half + 1 distinct values is given up: not
    # the one as long with three values, nor the one of 40 * half values
    assert [want[s][2] for s in segs] == [0] * 9 + [1, 0, 0]
    assert counts[10:] == [3, 40 * half]
    assert all(want[s][1] == s[0] + 1 for s in segs if want[s][2] == 0)

"""reducers.dd_add, the elementwise double-double add that merges the float
sums' state of a GPU group reduce, against exact rational arithmetic."""

import math
import random
from fractions import Fraction

import torch

from tests.dd_cases import U100


def _dd_add(pairs):
    from pathway_amd.engine.reducers import dd_add

    cols = [torch.tensor(c, dtype=torch.float64) for c in zip(*pairs)]
    h, l = dd_add(*cols)
    return h.tolist(), l.tolist()


def _check(pairs):
    hs, ls = _dd_add(pairs)
    for (ah, al, bh, bl), h, l in zip(pairs, hs, ls):
        exact = Fraction(ah) + Fraction(al) + Fraction(bh) + Fraction(bl)
        mag = abs(Fraction(ah)) + abs(Fraction(al)) + abs(Fraction(bh)) + abs(Fraction(bl))
        # the pair itself, before any rounding to one float: N = 1
        assert abs(Fraction(h) + Fraction(l) - exact) <= U100 * mag, (ah, al, bh, bl)
        assert h == h + l, "not normalised"


def test_big_plus_one_keeps_the_one():
    hs, ls = _dd_add([(1e16, 0.0, 1.0, 0.0)])
    assert (hs[0], ls[0]) == (1e16, 1.0)
    hs, ls = _dd_add([(hs[0], ls[0], -1e16, 0.0)])
    assert (hs[0], ls[0]) == (1.0, 0.0)


def test_cancelling_pairs():
    pairs = [
        (1e16, 1.0, -1e16, 0.0),
        (1e16, 1.0, -1e16, -1.0),
        (3.0, 2.0**-60, -3.0, 2.0**-61),
        (1e300, 1e280, -1e300, 3.0),
        (0.0, 0.0, 0.0, 0.0),
        (5.5, 0.0, 0.0, 0.0),
        (0.0, 0.0, -7.25, 2.0**-70),
    ]
    _check(pairs)
    hs, ls = _dd_add(pairs)
    assert (hs[1], ls[1]) == (0.0, 0.0)
    assert (hs[5], ls[5]) == (5.5, 0.0)
    assert (hs[6], ls[6]) == (-7.25, 2.0**-70)


def test_random_double_doubles():
    rng = random.Random(11)

    def dd():
        h = rng.gauss(0, 1) * 10 ** rng.uniform(-8, 8)
        l = rng.uniform(-0.5, 0.5) * math.ulp(h)
        return (h, l) if h + l == h else (h, 0.0)

    pairs = [dd() + dd() for _ in range(4000)]
    # near-cancelling high parts as well
    for _ in range(1000):
        h, l = dd()
        h2 = -h * (1 + rng.choice([0, 1, -1, 3]) * 2.0**-50)
        pairs.append((h, l, h2, rng.uniform(-0.5, 0.5) * math.ulp(h2)))
    _check(pairs)


def test_non_finite_high_part_gives_zero_low_part():
    inf, nan = math.inf, math.nan
    pairs = [
        (inf, 0.0, 1.0, 0.25),
        (inf, 0.0, -inf, 0.0),
        (nan, 0.0, 1.0, 0.0),
        (1.0, 2.0**-60, -inf, 0.0),
        (1.7e308, 0.0, 1.7e308, 0.0),
    ]
    hs, ls = _dd_add(pairs)
    assert hs[0] == inf and math.isnan(hs[1]) and math.isnan(hs[2])
    assert hs[3] == -inf and hs[4] == inf
    assert ls == [0.0] * 5

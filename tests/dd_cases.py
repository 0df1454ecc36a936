"""Shared by the double-double float-sum tests: the oracle (math.fsum, the
exact sum correctly rounded), the derived error bound and the input values.

Bound.  A double-double add errs by at most a few u^2 (u = 2^-53) of the
magnitude of its operands, which never exceeds the sum of |x| over what went
in; 2^-100 is 3 * 2^-106 with a margin of about 20.  After N additions the
pair (hi, lo) is therefore within N * 2^-100 * sum|x| of the exact sum, and
the emitted float hi + lo adds one rounding.  fsum adds none beyond its own
correct rounding, so

    |got - fsum| <= 2^-52 * |fsum| + N * 2^-100 * sum|x|.
"""

import math
import random
from fractions import Fraction

U52 = Fraction(1, 2**52)
U100 = Fraction(1, 2**100)


def bound(exact: float, n_adds: int, sum_abs: float) -> Fraction:
    return U52 * abs(Fraction(exact)) + n_adds * U100 * Fraction(sum_abs)


def check_sum(got: float, xs, n_adds=None, sum_abs=None, what=""):
    """`got` against fsum(xs); n_adds / sum_abs default to xs' own."""
    exact = math.fsum(xs)
    n_adds = len(xs) if n_adds is None else n_adds
    sum_abs = math.fsum(abs(x) for x in xs) if sum_abs is None else sum_abs
    if not math.isfinite(exact):
        raise AssertionError("oracle is for finite inputs")
    assert math.isfinite(got), (what, got, exact)
    err = abs(Fraction(got) - Fraction(exact))
    assert err <= bound(exact, n_adds, sum_abs), (what, got, exact, float(err))


def avg_bound(exact_sum: float, count: int, n_adds: int, sum_abs: float) -> Fraction:
    """Bound of fl((hi + lo) / count) against fsum / count: the sum's bound
    over count, widened by 2^-50 for the second-order terms of the two
    roundings that follow it, plus the rounding of the quotient."""
    b = bound(exact_sum, n_adds, sum_abs) * (1 + Fraction(1, 2**50)) / count
    return b + Fraction(1, 2**53) * abs(Fraction(exact_sum)) / count


def values(rng: random.Random, n: int, spikes: bool = True) -> list:
    """gauss(0,1) * 10^uniform(-8,8); with `spikes` and n >= 3 also 1e16,
    1.0 and -1e16 at shuffled places."""
    xs = [rng.gauss(0, 1) * 10 ** rng.uniform(-8, 8) for _ in range(n)]
    if spikes and n >= 3:
        for at, v in zip(rng.sample(range(n), 3), (1e16, 1.0, -1e16)):
            xs[at] = v
    return xs

"""Integer min/max are exact over the whole int64 range: no value passes
through a float64, which holds integers only up to 2**53.  The CPU cases run
everywhere; the GPU twin runs the same tables through the device path
(pw_seg_select)."""

import pytest
import torch

import pathway_amd as pw
from pathway_amd.debug import table_to_dicts

B = 2**53

#: (values of one group, its min, its max)
CASES = [
    ([B + 1, B + 3], B + 1, B + 3),
    ([-B - 1, 5], -B - 1, 5),
]


def _min_max(values):
    t = pw.debug.table_from_rows(
        pw.schema_from_types(g=int, v=int), [(0, v) for v in values]
    )
    r = t.groupby(pw.this.g).reduce(
        mn=pw.reducers.min(pw.this.v), mx=pw.reducers.max(pw.this.v)
    )
    _, cols = table_to_dicts(r)
    (key,) = cols["mn"]
    return cols["mn"][key], cols["mx"][key]


@pytest.mark.parametrize("values, mn, mx", CASES)
def test_int_min_max_exact_above_2_53(values, mn, mx):
    assert _min_max(values) == (mn, mx)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
@pytest.mark.parametrize("values, mn, mx", CASES)
def test_int_min_max_exact_above_2_53_gpu(values, mn, mx, monkeypatch):
    from pathway_amd import ops

    monkeypatch.setenv("PW_DEVICE", "cuda:0")
    before = ops.multiset_path_counts["select"]
    assert _min_max(values) == (mn, mx)
    assert ops.multiset_path_counts["select"] > before

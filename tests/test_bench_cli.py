"""bench.py command line: result line, --dump-outputs, --full gating."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    # runs on the GPU when there is one, on the CPU path otherwise
    cmd = [
        sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
        "--batch", "2000", "--vocab", "100", *extra,
    ]  # fmt: skip
    out = subprocess.run(
        cmd, cwd=ROOT, check=True, capture_output=True, text=True
    ).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_plain_run_line_and_dump(tmp_path):
    d = tmp_path / "dump"
    res = _run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["unit"] == "events/s" and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same 3 timed steps
    assert np.isclose(res["value"], 2000 / (res["ms_per_step"] / 1000.0), rtol=1e-9)
    # the RAG probe belongs to --full
    assert not any(k.startswith("rag_") for k in res["config"])

    arrays = {p.stem: np.load(p) for p in d.glob("*.npy")}
    assert set(arrays) == {"keys", "diffs", "word", "count"}
    n = arrays["diffs"].shape[0]
    assert 0 < n <= 200  # at most (-old, +new) per vocab word
    for name, a in arrays.items():
        assert a.dtype == np.float64 and a.shape[0] == n, name
    assert arrays["keys"].shape == (n, 4)
    assert set(np.unique(arrays["diffs"])) <= {-1.0, 1.0}
    # the last step's deltas add exactly one batch of events to the counts
    assert (arrays["diffs"] * arrays["count"]).sum() == 2000
    # 4 steps ran in all (1 warmup + 3 timed): the counts now total 4 batches
    ins = arrays["diffs"] > 0
    assert arrays["count"][ins].sum() <= 4 * 2000

    # same arguments -> same inputs -> same outputs
    d2 = tmp_path / "dump2"
    _run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d2))
    for name, a in arrays.items():
        assert np.array_equal(a, np.load(d2 / f"{name}.npy")), name

"""Shared inputs of the device-dictionary tests (CPU and GPU files)."""

from __future__ import annotations

import numpy as np
import torch

import pathway_amd as pw
from pathway_amd.engine.column import StringPool
from pathway_amd.internals.api import hash128, serialize_value
from pathway_amd.internals.rungraph import G

#: batches that mix known and new tokens, the empty token, duplicates and
#: non-ASCII text
BATCHES = [
    ["b", "a", "b", "", "c", "a"],
    ["c", "d", "", "żółć", "d", "a", "e"],
    ["żółć", "f", "f", "b", "日本語", "g"],
]


def spans_of(tokens: list[str], device="cpu"):
    """(buf, starts, ends): the tokens as newline-terminated UTF-8 lines."""
    raw = [t.encode("utf-8") for t in tokens]
    data = b"".join(r + b"\n" for r in raw)
    lens = np.array([len(r) for r in raw], dtype=np.int64)
    starts = np.zeros(len(raw), dtype=np.int64)
    if len(raw) > 1:
        starts[1:] = np.cumsum(lens + 1)[:-1]
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return (
        buf.to(device),
        torch.from_numpy(starts).to(device),
        torch.from_numpy(starts + lens).to(device),
    )


def oracle_codes(batches: list[list[str]]):
    """The codes and the pool the host path produces for the batches."""
    pool = StringPool()
    return [pool.codes(b).tolist() for b in batches], pool


def signed_hash(s: str) -> tuple[int, int]:
    def sg(x):
        return x - (1 << 64) if x >= (1 << 63) else x

    lo, hi = hash128(serialize_value(s))
    return sg(lo), sg(hi)


def assert_pool_equal(pool: StringPool, oracle: StringPool) -> None:
    assert pool._strs == oracle._strs
    assert pool._index == oracle._index
    assert pool._hash_lo == oracle._hash_lo
    assert pool._hash_hi == oracle._hash_hi


#: plaintext inputs by case: files of one directory (name -> bytes)
PLAINTEXT_OK = {
    "empty_lines": {"a.txt": b"x\n\n\ny\n\n"},
    "no_trailing_newline": {"a.txt": b"one\ntwo\nlast"},
    "empty_file": {"a.txt": b""},
    "two_files": {"a.txt": b"alpha\nbeta", "b.txt": b"beta\ngamma\n"},
    "empty_between": {"a.txt": b"p\n", "b.txt": b"", "c.txt": b"\n"},
    "non_ascii": {"a.txt": "zażółć\ngęślą\n日本語\nzażółć".encode("utf-8")},
}
PLAINTEXT_HOST_ONLY = {
    "crlf": {"a.txt": b"one\r\ntwo\rthree\n"},
    "crlf_second_file": {"a.txt": b"ok\n", "b.txt": b"x\r\ny\r\n"},
}
INVALID_UTF8 = {"a.txt": b"fine\n\xff\xfebroken\n"}


def write_files(tmp_path, files: dict[str, bytes]) -> str:
    d = tmp_path / "in"
    d.mkdir()
    for name, data in files.items():
        (d / name).write_bytes(data)
    return str(d / "*.txt")


def read_rows(path: str, mode: str, monkeypatch) -> dict:
    """{key: line} of pw.io.plaintext.read under PW_INGEST=mode."""
    monkeypatch.setenv("PW_INGEST", mode)
    G.clear()
    t = pw.io.plaintext.read(path, mode="static")
    keys, cols = pw.debug.table_to_dicts(t)
    assert set(cols) == {"data"}
    assert set(cols["data"]) == set(keys)
    return dict(cols["data"])

"""DeviceDictionary on a CPU device (host fallback) and the PW_INGEST
plaintext path: codes, lazy host sync and rows must equal the host path's.
The oracle is StringPool().codes(list_of_str)."""

from __future__ import annotations

import pytest
import torch

from pathway_amd.engine.column import StringColumn, StringPool
from tests.device_dict_cases import (
    BATCHES,
    INVALID_UTF8,
    PLAINTEXT_HOST_ONLY,
    PLAINTEXT_OK,
    assert_pool_equal,
    oracle_codes,
    read_rows,
    signed_hash,
    spans_of,
    write_files,
)


def _intern(d, tokens):
    return d.intern_spans(*spans_of(tokens)).tolist()


def test_one_dictionary_per_device():
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    assert pool.device_dictionary(torch.device("cpu")) is d
    assert not d.native


def test_intern_spans_equals_host_codes():
    want, _ = oracle_codes(BATCHES)
    d = StringPool().device_dictionary("cpu")
    assert [_intern(d, b) for b in BATCHES] == want


def test_sync_host_equals_host_pool():
    _, oracle = oracle_codes(BATCHES)
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    for b in BATCHES:
        _intern(d, b)
    d.sync_host()
    assert_pool_equal(pool, oracle)
    d.sync_host()  # idempotent
    assert_pool_equal(pool, oracle)


def test_pool_reads_drain_lazily():
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    codes = _intern(d, BATCHES[0])
    assert pool._strs == []  # nothing reached the host pool yet
    assert pool.value(codes[4]) == "c"
    assert pool._strs == ["b", "a", "", "c"]
    _intern(d, BATCHES[1])
    assert len(pool) == 7
    assert StringColumn(torch.tensor(codes), pool).to_pylist() == BATCHES[0]


def test_host_and_device_codes_interleave():
    batches = [BATCHES[0], ["x"], ["x", "h", "a"]]
    want, oracle = oracle_codes(batches)
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    assert _intern(d, batches[0]) == want[0]
    assert pool.code("x") == want[1][0]  # first code past the device's
    assert _intern(d, batches[2]) == want[2]  # "x" is known to the device
    assert pool.codes(["h", "fresh"]).tolist() == oracle.codes(["h", "fresh"]).tolist()
    assert_pool_equal(pool, oracle)


def test_encode_is_closed_world():
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    _intern(d, ["a", "b"])
    lo, hi = zip(signed_hash("b"), signed_hash("nope"), signed_hash("a"))
    got = d.encode(torch.tensor(lo), torch.tensor(hi))
    assert got.tolist() == [1, -1, 0]
    assert len(pool) == 2


def test_hash_tensors_cover_new_codes():
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    codes = [c for b in BATCHES for c in _intern(d, b)]
    tokens = [t for b in BATCHES for t in b]
    lo, hi = pool.hash_tensors("cpu")
    assert lo.shape[0] > max(codes)
    for c, t in zip(codes, tokens):
        assert (int(lo[c]), int(hi[c])) == signed_hash(t)


def test_invalid_utf8_token_raises_on_sync():
    pool = StringPool()
    d = pool.device_dictionary("cpu")
    buf = torch.tensor([0xFF, 0xFE, 10], dtype=torch.uint8)
    d.intern_spans(buf, torch.tensor([0]), torch.tensor([2]))
    with pytest.raises(UnicodeDecodeError):
        d.sync_host()


@pytest.mark.parametrize("case", sorted(PLAINTEXT_OK))
def test_plaintext_device_equals_host(case, tmp_path, monkeypatch):
    path = write_files(tmp_path, PLAINTEXT_OK[case])
    host = read_rows(path, "host", monkeypatch)
    assert read_rows(path, "device", monkeypatch) == host
    n_lines = sum(
        len(data.decode("utf-8").splitlines())
        for data in PLAINTEXT_OK[case].values()
    )
    assert len(host) == n_lines


def test_plaintext_device_path_is_taken(tmp_path, monkeypatch):
    """PW_INGEST=device builds the table from a prepared device batch."""
    import pathway_amd as pw
    from pathway_amd.engine.ingest_device import BatchSource

    path = write_files(tmp_path, PLAINTEXT_OK["two_files"])
    monkeypatch.setenv("PW_INGEST", "device")
    assert isinstance(pw.io.plaintext.read(path)._node.source, BatchSource)
    monkeypatch.setenv("PW_INGEST", "host")
    assert not isinstance(pw.io.plaintext.read(path)._node.source, BatchSource)
    monkeypatch.setenv("PW_INGEST", "gpu")
    with pytest.raises(ValueError):
        pw.io.plaintext.read(path)


@pytest.mark.parametrize("case", sorted(PLAINTEXT_HOST_ONLY))
def test_plaintext_carriage_returns_take_host_path(case, tmp_path, monkeypatch):
    path = write_files(tmp_path, PLAINTEXT_HOST_ONLY[case])
    host = read_rows(path, "host", monkeypatch)
    assert read_rows(path, "device", monkeypatch) == host
    assert "two" in host.values() or "y" in host.values()


def test_plaintext_invalid_utf8_behaves_as_host(tmp_path, monkeypatch):
    path = write_files(tmp_path, INVALID_UTF8)

    def outcome(mode):
        try:
            return read_rows(path, mode, monkeypatch)
        except UnicodeDecodeError as e:
            return (type(e), e.start, e.end)

    assert outcome("device") == outcome("host")

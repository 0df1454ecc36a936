"""Device ingest of newline-separated text: file bytes -> StringColumn.

The public counterpart of the byte-stream pipeline: the files' bytes go to
the device once, a newline scan (pw_scan_positions) yields the [start, end)
span of every line, and DeviceDictionary.intern_spans turns the spans into
string-pool codes — unseen lines are interned on the device, no python
string is built per row.  On a CPU device the same steps run on numpy and
the dictionary's host fallback.

PW_INGEST=host|device selects the path (internals/config.py).
"""

from __future__ import annotations

import codecs
import locale
import os

import numpy as np
import torch

from pathway_amd.engine.batch import DeltaBatch
from pathway_amd.engine.column import GLOBAL_STRING_POOL, StringColumn
from pathway_amd.engine import hashing
from pathway_amd.internals import dtype as dt
from pathway_amd.internals.api import TAG_INT

_NL = 10


def use_device_ingest(device) -> bool:
    """Unset: the device path on a GPU node with the native library, the
    host path otherwise.  PW_INGEST=device on a CPU node runs the device
    path's host fallback."""
    mode = os.environ.get("PW_INGEST", "").strip().lower()
    if mode not in ("", "host", "device"):
        raise ValueError(f"PW_INGEST must be 'host' or 'device', got {mode!r}")
    if mode:
        return mode == "device"
    if torch.device(device).type != "cuda":
        return False
    from pathway_amd import ops

    return ops.lib_available()


def _text_mode_is_utf8() -> bool:
    try:
        return codecs.lookup(locale.getpreferredencoding(False)).name == "utf-8"
    except LookupError:
        return False


def load_text_files(files: list[str]) -> bytes | None:
    """The files' bytes back to back, every non-empty file ending in a
    newline (so a last line without one still yields a span and never
    runs into the next file) — or None when a file must take the host
    path to keep its results and exceptions: one that holds a carriage
    return (text mode translates universal newlines) or that text mode
    would not decode as the UTF-8 the string pool stores."""
    parts: list[bytes] = []
    utf8 = None
    for f in files:
        with open(f, "rb") as fh:
            data = fh.read()
        if not data:
            continue
        if b"\r" in data:
            return None
        if not data.isascii():
            if utf8 is None:
                utf8 = _text_mode_is_utf8()
            if not utf8:
                return None
            try:
                data.decode("utf-8")
            except UnicodeDecodeError:
                return None
        parts.append(data)
        if not data.endswith(b"\n"):
            parts.append(b"\n")
    return b"".join(parts)


def line_spans(buf: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[start, end) of every newline-terminated line of a uint8 buffer."""
    if buf.is_cuda:
        from pathway_amd import ops

        nl = ops.scan_positions_gpu(buf, _NL)
    else:
        nl = torch.from_numpy(np.flatnonzero(buf.numpy() == _NL))
    starts = torch.empty_like(nl)
    if nl.shape[0]:
        starts[0] = 0
        starts[1:] = nl[:-1] + 1
    return starts, nl


def row_keys(first: int, n: int, device) -> torch.Tensor:
    """(n, 2) keys of rows numbered first, first+1, ... — the keys
    table_from_rows gives them: hash_values([row number])."""
    seq = torch.arange(first, first + n, dtype=torch.int64, device=device)
    lo, hi = hashing.value_hash_words(seq, TAG_INT)
    klo, khi = hashing.hash128_words([lo, hi])
    return torch.stack([klo, khi], dim=1)


def lines_batch(data: bytes, device, pool=None, time: int = 0) -> DeltaBatch | None:
    """One DeltaBatch with a StringColumn `data`, a row per line."""
    if not data:
        return None
    pool = pool or GLOBAL_STRING_POOL
    device = torch.device(device)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device)
    starts, ends = line_spans(buf)
    n = int(starts.shape[0])
    codes = pool.device_dictionary(device).intern_spans(buf, starts, ends)
    diffs = torch.ones(n, dtype=torch.int64, device=device)
    cols = {"data": StringColumn(codes, pool, dt.STR)}
    return DeltaBatch(row_keys(1, n, device), cols, diffs, time)


class BatchSource:
    """A prepared batch at time 0 (what StaticSource is for python rows)."""

    def __init__(self, batch: DeltaBatch | None):
        self.batch = batch
        self._done = batch is None

    def reset(self) -> None:
        self._done = self.batch is None

    def seek(self, threshold_time: int) -> None:
        if threshold_time >= 0:
            self._done = True

    def next_time(self) -> int | None:
        return None if self._done else 0

    def pull(self, time: int, device) -> DeltaBatch | None:
        if self._done or time != 0:
            return None
        self._done = True
        return self.batch.to_device(device)


def read_plaintext(files: list[str], device):
    """Table of the files' lines, or None when they must take the host path."""
    from pathway_amd.engine.nodes import InputNode
    from pathway_amd.internals.table import Table
    from pathway_amd.internals.universe import Universe

    data = load_text_files(files)
    if data is None:
        return None
    node = InputNode(BatchSource(lines_batch(data, device)), device)
    return Table(node, {"data": dt.STR}, Universe())

"""Open-vocabulary device dictionary: token bytes -> StringPool codes.

One DeviceDictionary per (StringPool, device), obtained with
StringPool.device_dictionary(device).  On a GPU it owns

* two open-addressing hash tables (ops.DeviceHashTable) token hash -> code:
  a compact "front" table of the codes whose count the host knows exactly,
  only ever rebuilt, and the open table that new tokens are interned into.
  The kernels' probe bound makes the open table large enough for a whole
  batch of unseen tokens (far past the caches for a 4M-row batch); with
  the front table ahead of it, rows that hit a known token never touch it,
* capacity-doubling device arrays pool_lo/pool_hi (row index == code) that
  StringPool.hash_tensors(device) serves views of,
* a byte arena with per-code (offset, length) holding the bytes of tokens
  the device interned and the host pool has not seen yet,
* a queue of pinned size snapshots, so the count of new tokens is read
  back one call later (or in sync_host) instead of blocking the call that
  produced it.

intern_spans() assigns unseen tokens the codes StringPool.codes() would
have assigned — first occurrence by row index — entirely on the device;
sync_host() later appends the strings to the host pool and verifies codes
and hashes.  StringPool drains attached dictionaries before it reads or
grows its string list, so the two sides never hand out the same code.

On a CPU device the same interface runs on plain numpy/python with no
native library (tests and CPU nodes), with the same laziness.

Equal 128-bit hashes are treated as equal strings, as elsewhere.
"""

from __future__ import annotations

from collections import deque

import numpy as np
import torch

from pathway_amd.internals.api import TAG_STR

_MIN_CAP = 1024
_MIN_ARENA = 1 << 16


def device_key(device) -> str:
    """Canonical name of a device ("cuda" and "cuda:0" are one device)."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return str(d)


def _pow2_at_least(x: int, floor: int) -> int:
    return max(floor, 1 << max(0, int(x) - 1).bit_length())


class DeviceDictionary:
    def __init__(self, pool, device):
        self.pool = pool
        self.device = torch.device(device_key(device))
        #: True on a GPU (HIP kernels); False runs the host fallback
        self.native = self.device.type == "cuda"
        #: pool entries mirrored here; codes >= this were assigned on the
        #: device and wait for sync_host()
        self._mirrored = 0
        #: blocking device->host reads made so far (profiling aid)
        self.blocking_syncs = 0
        if self.native:
            from pathway_amd import ops

            ops.require_lib()
            dev = self.device
            self._cap = 0
            self._grow_arrays(_MIN_CAP)
            # [dictionary size, arena cursor, kernel error bits] — the
            # kernels read the base code and reserve arena bytes here, so
            # no call needs either number on the host
            self.state = torch.zeros(3, dtype=torch.int64, device=dev)
            self._new_open_table(0)
            self.front = ops.DeviceHashTable(*self._empty_keys())
            self._front_size = 0  # codes [0, _front_size) are in front
            self.arena = torch.empty(_MIN_ARENA, dtype=torch.uint8, device=dev)
            self._size = 0  # last size confirmed by a snapshot
            self._cursor = 0  # last arena cursor confirmed by a snapshot
            self._inflight: deque = deque()  # (event, pinned, rows, bytes)
            self._rows_in_flight = 0
            self._bytes_in_flight = 0
        else:
            self._bytes_index: dict[bytes, int] = {}
            self._pending: list[bytes] = []

    # ------------------------------------------------------------ sizes --

    def _grow_arrays(self, need: int) -> None:
        if need <= self._cap:
            return
        cap = _pow2_at_least(need, max(_MIN_CAP, 2 * self._cap))
        dev = self.device
        for name in ("pool_lo", "pool_hi", "tok_off", "tok_len"):
            new = torch.empty(cap, dtype=torch.int64, device=dev)
            if self._cap:
                new[: self._cap].copy_(getattr(self, name))
            setattr(self, name, new)
        self._cap = cap

    def _empty_keys(self):
        empty = torch.empty(0, dtype=torch.int64, device=self.device)
        return empty, empty

    def _new_open_table(self, reserve: int) -> None:
        from pathway_amd import ops

        self.table = ops.DeviceHashTable(*self._empty_keys(), reserve=reserve)
        self.table.err = self.state[2:3]

    def _refresh_front(self, clear_open: bool) -> None:
        """Rebuild the front table over every code (the size must be
        exact: nothing in flight) and empty the open table."""
        from pathway_amd import ops

        assert not self._inflight
        size = self._size
        self.front = ops.DeviceHashTable(self.pool_lo[:size], self.pool_hi[:size])
        self._front_size = size
        if clear_open:
            self.table.tab_val.fill_(-1)

    def _fold(self, snap: torch.Tensor, rows: int, nbytes: int) -> None:
        from pathway_amd import ops

        self._size = int(snap[0])
        self._cursor = int(snap[1])
        self._rows_in_flight -= rows
        self._bytes_in_flight -= nbytes
        if int(snap[2]):
            raise RuntimeError(ops.intern_error_message(int(snap[2])))

    def _poll(self) -> None:
        """Fold in the snapshots that have already arrived; never waits."""
        q = self._inflight
        while q and q[0][0].query():
            _, snap, rows, nbytes = q.popleft()
            self._fold(snap, rows, nbytes)

    def _settle(self) -> None:
        """Wait for every snapshot in flight: size and cursor are exact."""
        q = self._inflight
        if q:
            self.blocking_syncs += 1
        while q:
            ev, snap, rows, nbytes = q.popleft()
            ev.synchronize()
            self._fold(snap, rows, nbytes)

    def _snapshot(self, rows: int, nbytes: int) -> None:
        snap = torch.empty(3, dtype=torch.int64, pin_memory=True)
        snap.copy_(self.state, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._inflight.append((ev, snap, rows, nbytes))
        self._rows_in_flight += rows
        self._bytes_in_flight += nbytes

    @property
    def size_upper_bound(self) -> int:
        """No code handed out so far is >= this."""
        if self.native:
            return self._size + self._rows_in_flight
        return self._mirrored + len(self._pending)

    # --------------------------------------------------------- catch up --

    def _catch_up(self) -> None:
        """Mirror the strings the host pool gained since the last call.
        The pool drained this dictionary before it grew, so nothing
        device-assigned is pending when there is anything to mirror."""
        pool = self.pool
        m = len(pool._strs) - self._mirrored
        if m <= 0:
            return
        lo_l = pool._hash_lo[self._mirrored :]
        hi_l = pool._hash_hi[self._mirrored :]
        if not self.native:
            assert not self._pending
            for k in range(m):
                c = self._mirrored + k
                self._bytes_index.setdefault(pool._strs[c].encode("utf-8"), c)
            self._mirrored += m
            return
        self._settle()
        if self._size != self._mirrored:
            raise RuntimeError(
                "host pool grew while device-assigned codes were pending"
            )
        size, dev = self._size, self.device
        self._grow_arrays(size + m)
        lo = torch.tensor(lo_l, dtype=torch.int64, device=dev)
        hi = torch.tensor(hi_l, dtype=torch.int64, device=dev)
        self.pool_lo[size : size + m] = lo
        self.pool_hi[size : size + m] = hi
        self.state[0:1] += m
        self._size += m
        self._mirrored += m
        # every earlier code is in the front table already (the last
        # sync_host or catch-up left the open table empty)
        self._refresh_front(clear_open=False)

    # ------------------------------------------------------------ encode --

    def encode(self, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
        """Closed-world probe: the code of each hash, -1 where unknown."""
        self._catch_up()
        if self.native:
            self._poll()
            codes, found = self.front.probe(lo, hi)
            if self.size_upper_bound > self._front_size:
                codes = torch.where(found, codes, self.table.probe(lo, hi)[0])
            return codes
        self.sync_host()
        pool = self.pool
        index = {
            (pool._hash_lo[c], pool._hash_hi[c]): c
            for c in range(len(pool._strs) - 1, -1, -1)
        }
        pairs = zip(lo.tolist(), hi.tolist())
        return torch.tensor([index.get(p, -1) for p in pairs], dtype=torch.int64)

    def intern_spans(
        self, buf: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor
    ) -> torch.Tensor:
        """Codes of the tokens buf[starts[i]:ends[i]] (uint8 buffer, int64
        spans on this dictionary's device); unseen tokens are interned and
        their bytes captured before this returns, so the caller may reuse
        `buf` right away."""
        if not self.native:
            return self._intern_spans_host(buf, starts, ends)
        from pathway_amd import ops

        lo, hi = ops.varlen_hash_se_gpu(buf, starts, ends, TAG_STR)
        return self.intern_hashes(lo, hi, buf, starts, ends)

    def intern_hashes(
        self,
        lo: torch.Tensor,
        hi: torch.Tensor,
        buf: torch.Tensor,
        starts: torch.Tensor,
        ends: torch.Tensor,
    ) -> torch.Tensor:
        """intern_spans() for a caller that already hashed the spans with
        varlen_hash_se_gpu(buf, starts, ends, TAG_STR)."""
        if not self.native:
            return self._intern_spans_host(buf, starts, ends)
        from pathway_amd import ops

        self._catch_up()
        self._poll()
        n = int(lo.shape[0])
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        buf = buf.contiguous()
        starts, ends = starts.contiguous(), ends.contiguous()
        nbytes = int(buf.shape[0])
        # arena: the new tokens' bytes are spans of buf, at most nbytes
        # (bounded by the bytes of the calls still in flight until their
        # cursor snapshot arrives).  Short of room: wait for the exact
        # cursor, then drain; an arena of 3 buffers holds this call, one
        # in flight and a buffer's worth of pending tokens
        cap = int(self.arena.shape[0])
        if cap - (self._cursor + self._bytes_in_flight) < nbytes:
            self._settle()
            if cap < 3 * nbytes or cap - self._cursor < nbytes:
                self.sync_host()  # leaves the arena empty
                if cap < 3 * nbytes:
                    self.arena = torch.empty(
                        3 * nbytes, dtype=torch.uint8, device=self.device
                    )
        # dictionary arrays and open table: sized by the upper bound, so
        # the exact count of earlier calls is only waited for when the
        # table would have to grow on the strength of it.  The open table
        # is folded into the front one when the exact size is at hand and
        # it holds a good share of the codes (amortised), or when it is full
        self._grow_arrays(self.size_upper_bound + n)
        if not self._inflight:
            held = self._size - self._front_size
            if held >= max(1 << 16, self._front_size // 4):
                self._refresh_front(clear_open=True)
        if not self.table.fits(self.size_upper_bound - self._front_size + n):
            self._settle()
            if self._size > self._front_size:
                self._refresh_front(clear_open=True)
            if not self.table.fits(2 * n):
                # room for this batch and one more still in flight
                self._new_open_table(2 * n)
        base = self.state[0:1]
        codes, first_rows, n_new = self.table.intern(
            lo, hi, base, self.pool_lo, self.pool_hi, front=self.front
        )
        ops.gather_spans_gpu(
            buf, starts, ends, first_rows, n_new, base, self.arena,
            self.state[1:2], self.tok_off, self.tok_len, self.table.err,
        )
        base += n_new
        self._snapshot(n, nbytes)
        return codes

    def _intern_spans_host(self, buf, starts, ends) -> torch.Tensor:
        self._catch_up()
        data = buf.cpu().numpy().tobytes()
        index, pending = self._bytes_index, self._pending
        out = np.empty(int(starts.shape[0]), dtype=np.int64)
        for i, (s, e) in enumerate(zip(starts.tolist(), ends.tolist())):
            tok = data[s:e]
            c = index.get(tok)
            if c is None:
                c = self._mirrored + len(pending)
                index[tok] = c
                pending.append(tok)
            out[i] = c
        return torch.from_numpy(out)

    # --------------------------------------------------------- host sync --

    def hash_tensors(self) -> tuple[torch.Tensor, torch.Tensor]:
        """Views of the device hash arrays covering every code handed out
        so far (rows past the exact size are never indexed)."""
        assert self.native
        self._catch_up()
        self._poll()
        n = self.size_upper_bound
        return self.pool_lo[:n], self.pool_hi[:n]

    def sync_host(self) -> None:
        """Append the device-interned tokens to the host pool (strict
        UTF-8), checking that the host assigns the same codes and computes
        the same hashes.  Raises on any mismatch."""
        pool = self.pool
        if not self.native:
            pending, self._pending = self._pending, []
            for tok in pending:
                self._append(tok.decode("utf-8"), None, None)
            return
        self._settle()
        first, size = self._mirrored, self._size
        if size == first:
            if self._cursor:
                self.state[1:2].zero_()
                self._cursor = 0
            return
        self.blocking_syncs += 1
        meta = torch.stack(
            [
                self.tok_off[first:size],
                self.tok_len[first:size],
                self.pool_lo[first:size],
                self.pool_hi[first:size],
            ]
        ).cpu()
        data = self.arena[: self._cursor].cpu().numpy().tobytes()
        off, ln, lo, hi = (r.tolist() for r in meta)
        for k in range(size - first):
            tok = data[off[k] : off[k] + ln[k]]
            if len(tok) != ln[k]:
                raise RuntimeError("device dictionary arena is truncated")
            self._append(tok.decode("utf-8"), lo[k], hi[k])
        self.state[1:2].zero_()
        self._cursor = 0
        assert len(pool._strs) == size
        self._refresh_front(clear_open=True)

    def _append(self, s: str, lo, hi) -> None:
        pool = self.pool
        want = self._mirrored
        c = pool._intern_host(s)
        if c != want:
            raise RuntimeError(
                f"device dictionary assigned code {want} to {s!r}, the host "
                f"pool assigns {c}"
            )
        if lo is not None and (pool._hash_lo[c], pool._hash_hi[c]) != (lo, hi):
            raise RuntimeError(f"device hash of {s!r} differs from the host hash")
        self._mirrored = want + 1


"""CPU checks of tests/arrange_cases.py: the sizes match the launch
geometry they are derived from, the inputs hold the edges the GPU tests are
there for, and the oracles agree with an independent formulation."""

import re

import pytest
import torch

from tests import arrange_cases as C
from tests import state_prims_cases as S


# ---------------------------------------------------------------- geometry --


def _hip_source() -> str:
    from pathway_amd.ops import build

    with open(build.SRC) as f:
        return f.read()


def _define(src: str, name: str) -> int:
    return int(re.search(rf"^#define {name} (\d+)\s*$", src, re.M).group(1))


def _body(src: str, signature: str) -> str:
    """Source text from a function's signature to its closing brace."""
    at = src.index(signature)
    return src[at : src.index("\n}\n", at)]


def test_sizes_match_the_launch_geometry():
    from pathway_amd import ops

    src = _hip_source()
    assert C.BLOCK == _define(src, "PW_BLOCK")
    assert C.MAX_GRID == _define(src, "PW_MAX_GRID")
    assert C.GRID_TRIP == C.MAX_GRID * C.BLOCK + 257
    assert C.MC_CHUNK == _define(src, "PW_MC_CHUNK")
    assert C.PART_MAX_DEST == _define(src, "PW_PART_MAX_DEST")
    assert C.RS_LANES == _define(src, "PW_RS_THREADS")
    assert _define(src, "PW_RS_DIGITS") == 256
    # the hash kernel: a table of 20 word pointers and a case for each width
    assert f"const uint64_t* p[{C.HASH_MAX_WORDS}];" in src
    assert f"CASE({C.HASH_MAX_WORDS})" in src
    assert f"CASE({C.HASH_MAX_WORDS + 1})" not in src
    assert C.HASH_MAX_WORDS == ops.HASH_MAX_WORDS
    # the gather: 8 columns a launch, 4096 blocks at the most
    gather = _body(src, 'extern "C" int pw_gather_cols(')
    assert f"ncols > {C.GATHER_COLS}" in gather
    assert f"if (nblocks > {C.GATHER_MAX_GRID}) nblocks = {C.GATHER_MAX_GRID};" in gather
    assert f"const long long* src[{C.GATHER_COLS}];" in src
    # what the wrappers decide
    assert C.PART_MAX_BLOCKS == ops.PART_MAX_BLOCKS
    assert (C.RS_LANES, C.RS_BLOCK_ROWS, C.RS_MAX_BLOCKS) == (
        ops.RS_LANES,
        ops.RS_BLOCK_ROWS,
        ops.RS_MAX_BLOCKS,
    )
    assert C.GATHER_ALL_SWITCH == ops.GATHER_ALL_MIN_ROWS


def test_sizes_sit_on_the_edges():
    # hash, value hash: a second grid trip
    assert C.GRID_TRIP > C.MAX_GRID * C.BLOCK
    assert {C.BLOCK - 1, C.BLOCK, C.BLOCK + 1, 0, 1} <= set(C.HASH_SIZES)
    assert set(C.HASH_W_NO_TAIL) == {w for w in C.HASH_W if w >= 4 and w % 4 == 0 and w > 4}
    # merge: both sides of one thread's chunk, of two, and of one block
    per_block = C.MC_CHUNK * C.BLOCK
    for edge in (C.MC_CHUNK, 2 * C.MC_CHUNK, per_block):
        assert {edge - 1, edge, edge + 1} <= set(C.MC_TOTALS)
    assert max(C.MC_TOTALS) > 2 * per_block
    # partition: past the block cap every block's chunk is longer than a block
    n = max(C.PART_N)
    nblocks = min(C.PART_MAX_BLOCKS, -(-n // C.BLOCK))
    assert nblocks == C.PART_MAX_BLOCKS and -(-n // nblocks) > C.BLOCK
    assert {0, 1, C.BLOCK - 1, C.BLOCK, C.BLOCK + 1} <= set(C.PART_N)
    assert max(C.PART_WORLDS) == C.PART_MAX_DEST and min(C.PART_WORLDS) == 1
    # radix sort: a wave, a block, and the block cap with chunk 65
    for edge in (C.RS_LANES, C.RS_BLOCK_ROWS):
        assert {edge - 1, edge, edge + 1} <= set(C.RS_N)
    assert max(C.RS_N) > 2 * C.RS_BLOCK_ROWS
    n = C.RS_N_CAP
    nblocks = min(C.RS_MAX_BLOCKS, -(-n // C.RS_BLOCK_ROWS))
    chunk = -(-n // (nblocks * C.RS_LANES))
    assert nblocks == C.RS_MAX_BLOCKS and chunk == 65
    assert (nblocks * C.RS_LANES - 1) * chunk >= n, "the last lanes must be empty"
    # gather: a second grid trip, and two launches from 9 columns on
    assert C.GATHER_TRIP > C.GATHER_MAX_GRID * C.BLOCK
    assert {C.GATHER_COLS, C.GATHER_COLS + 1, 2 * C.GATHER_COLS, 1} <= set(C.GATHER_NCOLS)
    assert {0, 1, C.BLOCK - 1, C.BLOCK, C.BLOCK + 1} <= set(C.GATHER_M)


def test_shared_names_come_from_state_prims_cases():
    assert C.SPECIALS is S.SPECIALS and C.wrap64 is S.wrap64
    assert C.columns is S.columns and C.GRID_TRIP is S.GRID_TRIP


# -------------------------------------------------------------- row hashes --


@pytest.mark.parametrize("W", C.HASH_W)
def test_hash_rows_hold_the_edges_and_the_two_references_agree(W):
    from pathway_amd.engine import hashing
    from pathway_amd.internals import api

    rows = C.hash_rows(W)
    assert len(rows) == C.HASH_SMALL_N and all(len(r) == W for r in rows)
    for p in range(W):
        assert set(C.SPECIALS) <= {r[p] for r in rows}
    assert (0,) * W in rows and (-1,) * W in rows and (1,) * W in rows
    assert sum(1 for r in rows if max(abs(v) for v in r) > 2**40) > 100
    words = C.columns(rows, W)
    lo = hashing.xxh64_words(words, api.SEED_LO).tolist()
    hi = hashing.xxh64_words(words, api.SEED_HI).tolist()
    assert list(zip(lo, hi)) == [C.py_hash128(r) for r in rows]


def test_py_hash128_is_xxh64_of_the_packed_words():
    import struct

    from pathway_amd.internals import api

    # XXH64 of the empty input and of "a", the published test vectors
    assert api.xxh64(b"", 0) == 0xEF46DB3751D8E999
    assert api.xxh64(b"a", 0) == 0xD24EC4F1A98C6E5B
    row = (C.INT64_MIN, -1, 5)
    data = struct.pack("<qqq", *row)
    assert len(data) == 24
    lo, hi = C.py_hash128(row)
    assert lo & C.MASK64 == api.xxh64(data, api.SEED_LO)
    assert hi & C.MASK64 == api.xxh64(data, api.SEED_HI)
    assert api.SEED_LO != api.SEED_HI


def test_hash_grid_words():
    for W in C.HASH_GRID_W:
        words = C.hash_grid_words(W)
        assert len(words) == W and all(w.shape == (C.GRID_TRIP,) for w in words)
        assert all(int(w[-1]) == C.INT64_MIN for w in words)
        assert bool((words[0] < 0).any()) and bool((words[0] > 2**62).any())
    assert set(C.HASH_GRID_W) == {1, 4, C.HASH_MAX_WORDS}


def test_value_tags_and_payloads():
    import inspect

    from pathway_amd.engine import hashing
    from pathway_amd.internals import api

    # every TAG_* that column_value_hash names is in VALUE_TAGS
    named = set(re.findall(r"TAG_[A-Z_]+", inspect.getsource(hashing.column_value_hash)))
    assert named and {getattr(api, t) for t in named} == set(C.VALUE_TAGS)
    for n in C.VALUE_N:
        p = C.value_payload(n)
        assert p.shape == (n,) and p.dtype == torch.int64
        assert p[:5].tolist() == list(C.SPECIALS[: min(n, 5)])
    # the CPU formulation of the value hash against serialize_value
    p = C.value_payload(257)
    lo, hi = hashing.value_hash_words(p, api.TAG_INT)
    for i in range(0, 257, 16):
        want = api.hash128(api.serialize_value(int(p[i])))
        assert (int(lo[i]) & C.MASK64, int(hi[i]) & C.MASK64) == want


# ------------------------------------------------------- merge-consolidate --


def _first_diff(a: tuple, b: tuple) -> int:
    for p, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return p
    return len(a)


@pytest.mark.parametrize("nw", C.MC_NW)
def test_mc_sides_hold_every_edge(nw):
    a, b = C.mc_sides(nw)
    for side in (a, b):
        assert side == sorted(side) and len(set(side)) == len(side)
        for p in range(nw):
            assert set(C.SPECIALS) <= {r[p] for r in side}
        # neighbours tie in every number of leading words
        assert {_first_diff(x, y) for x, y in zip(side, side[1:])} == set(range(nw))
    both = set(a) & set(b)
    assert both and set(a) - both and set(b) - both
    # in the merged order, an A row and a B row meet with their first
    # difference at every word position, and as equals
    merged = sorted([(r, "A") for r in a] + [(r, "B") for r in b])
    meets = {
        _first_diff(x[0], y[0])
        for x, y in zip(merged, merged[1:])
        if x[1] != y[1]
    }
    assert meets == set(range(nw + 1))
    union = sorted(set(a) | set(b))
    assert sorted(union, key=C.unsigned) != union


@pytest.mark.parametrize("nacc", C.MC_NACC)
@pytest.mark.parametrize("nw", C.MC_NW)
def test_mc_accs_hold_every_edge(nw, nacc):
    a, b = C.mc_sides(nw)
    a_accs, b_accs = C.mc_accs(a, b, nacc)
    in_b = {r: j for j, r in enumerate(b)}
    seen = set()
    for i, r in enumerate(a):
        j = in_b.get(r)
        if j is None:
            if a_accs[0][i] == 0:
                seen.add("unmatched A, slot 0 zero")
                assert nacc == 1 or all(acc[i] != 0 for acc in a_accs[1:])
            continue
        sums = [a_accs[c][i] + b_accs[c][j] for c in range(nacc)]
        if sums[0] == 0 and all(s != 0 for s in sums[1:]):
            seen.add("slot 0 cancels")
        if sums[0] != 0 and nacc > 1 and all(s == 0 for s in sums[1:]):
            seen.add("others cancel")
        if abs(sums[0]) >= 2**63 and C.wrap64(sums[0]) != 0:
            seen.add("slot 0 wraps")
    in_a = set(a)
    for j, r in enumerate(b):
        if r not in in_a and b_accs[0][j] == 0:
            seen.add("unmatched B, slot 0 zero")
            assert nacc == 1 or all(acc[j] != 0 for acc in b_accs[1:])
    want = {
        "unmatched A, slot 0 zero",
        "unmatched B, slot 0 zero",
        "slot 0 cancels",
        "slot 0 wraps",
    }
    if nacc > 1:
        want.add("others cancel")
    assert seen == want
    rows, accs, rep = C.mc_oracle(a, a_accs, b, b_accs)
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    assert all(v != 0 for v in accs[0])
    kept = set(rows)
    dropped = (set(a) | set(b)) - kept
    assert dropped & set(a) & set(b) and dropped - set(b) and dropped - set(a)
    for r, src in zip(rows, rep):  # A wins on a match
        assert (a + b)[src] == r and (src < len(a)) == (r in in_a)


def _host_merge(a_rows, a_w, b_rows, b_w):
    """The engine's host path for 4-word rows and one weight: sorted merge
    selection, then the consolidation scan; rep rides along as a column."""
    from pathway_amd.engine.column import TensorColumn
    from pathway_amd.engine.state import consolidate_sorted, merge_sorted_select
    from pathway_amd.internals import dtype as dt

    aw, bw = C.columns(a_rows, 4), C.columns(b_rows, 4)
    sel = merge_sorted_select(aw, bw)
    words = [torch.cat([x, y]).index_select(0, sel) for x, y in zip(aw, bw)]
    w = torch.cat(
        [torch.tensor(a_w, dtype=torch.int64), torch.tensor(b_w, dtype=torch.int64)]
    ).index_select(0, sel)
    out_words, out_w, cols = consolidate_sorted(
        words, w, {"src": TensorColumn(sel, dt.INT)}
    )
    rows = [tuple(r) for r in torch.stack(out_words, 1).tolist()] if len(out_w) else []
    return rows, out_w.tolist(), cols["src"].tensor.tolist()


def test_mc_oracle_agrees_with_the_host_merge_path():
    a, b = C.mc_sides(4)
    a_accs, b_accs = C.mc_accs(a, b, 1)
    cases = [(a, a_accs, b, b_accs)]
    a, b = C.mc_tail_function_case()
    a_accs, b_accs = C.mc_accs(a, b, 1)
    cases.append((a, a_accs, b, b_accs))
    ta, taa, tb, tba = C.mc_tail_differs_case()
    cases.append((ta, taa[:1], tb, tba[:1]))
    for shape in ("one_matched", "interleave", "identical_1030", "total_2049"):
        cases.append(C.mc_shape_case(shape, 4, 1))
    for a_rows, a_accs, b_rows, b_accs in cases:
        rows, accs, rep = C.mc_oracle(a_rows, a_accs, b_rows, b_accs, 4)
        got_rows, got_w, got_rep = _host_merge(a_rows, a_accs[0], b_rows, b_accs[0])
        assert got_rows == rows and got_w == accs[0] and got_rep == rep


def test_mc_oracle_by_hand():
    # slot 0 decides alone; the sum wraps; A wins; order is signed
    a = [(C.INT64_MIN, 1), (-1, 0), (3, 3)]
    b = [(-1, 0), (0, 0), (3, 3)]
    a_accs = [[2, 5, 2**62], [1, 1, 1]]
    b_accs = [[-5, 0, 2**62], [7, 9, 1]]
    rows, accs, rep = C.mc_oracle(a, a_accs, b, b_accs)
    assert rows == [(C.INT64_MIN, 1), (3, 3)]
    assert accs == [[2, C.INT64_MIN], [1, 2]] and rep == [0, 2]
    rows, accs, rep = C.mc_oracle([], [[]], [(4,)], [[1]])
    assert (rows, accs, rep) == ([(4,)], [[1]], [0])
    assert C.mc_oracle([], [[]], [], [[]]) == ([], [[]], [])


def test_mc_tail_cases():
    a, b = C.mc_tail_function_case()
    assert all(len(r) == 4 for r in a + b)
    assert a == sorted(a) and b == sorted(b)
    tails = {}
    for r in a + b:
        assert tails.setdefault(r[:2], r[2:]) == r[2:]
    a_accs, b_accs = C.mc_accs(a, b, 8, nwc=2)
    assert C.mc_oracle(a, a_accs, b, b_accs, 2) == C.mc_oracle(a, a_accs, b, b_accs, 4)
    # the tail words are no sorted function of the prefix
    union = sorted(set(a) | set(b))
    assert any(x[2:] > y[2:] for x, y in zip(union, union[1:]))

    a, a_accs, b, b_accs = C.mc_tail_differs_case()
    assert a == sorted(a) and b == sorted(b)
    assert len({r[:2] for r in a}) == len(a) and len({r[:2] for r in b}) == len(b)
    rows2, accs2, rep2 = C.mc_oracle(a, a_accs, b, b_accs, 2)
    rows4, accs4, rep4 = C.mc_oracle(a, a_accs, b, b_accs, 4)
    assert len(rows2) == 7 and len(rows4) == 8
    at = rows2.index((1, 2, 10, 11))
    assert (1, 2, 99, -98) not in rows2 and rep2[at] == 1
    assert [acc[at] for acc in accs2] == [2 + 6, 20 + 60]
    assert (1, 2, 10, 11) in rows4 and (1, 2, 99, -98) in rows4


def test_mc_shapes():
    assert C.mc_key_row(0, 1) == (-2,) and C.mc_key_row(5, 1) == (3,)
    for nw in C.MC_NW:
        rows = [C.mc_key_row(k, nw) for k in range(100)]
        assert rows == sorted(rows) and len(set(rows)) == 100
        assert rows[0][0] < 0 < rows[-1][0]
    sizes = {s: tuple(len(k) for k in C.mc_shape_keys(s)) for s in C.MC_SHAPES}
    assert sizes["empty"] == (0, 0) and sizes["only_b"] == (0, 1)
    assert sizes["only_a"] == (1, 0)
    assert sizes["one_matched"] == sizes["one_unmatched"] == (1, 1)
    assert sizes["identical_1030"] == (1030, 1030)
    assert {sum(sizes[f"total_{t}"]) for t in C.MC_TOTALS} == set(C.MC_TOTALS)
    a, b = C.mc_shape_keys("one_matched")
    assert a == b
    a, b = C.mc_shape_keys("one_unmatched")
    assert a != b
    a, b = C.mc_shape_keys("a_below_b")
    assert max(a) < min(b)
    a, b = C.mc_shape_keys("a_above_b")
    assert min(a) > max(b)
    a, b = C.mc_shape_keys("interleave")
    merged = sorted([(k, 0) for k in a] + [(k, 1) for k in b])
    assert [s for _, s in merged] == [0, 1] * 20
    for s in C.MC_SHAPES:
        a, b = C.mc_shape_keys(s)
        assert a == sorted(set(a)) and b == sorted(set(b))
        if s.startswith("total_") and sum(sizes[s]) > 8:
            assert set(a) & set(b) and set(a) - set(b) and set(b) - set(a)
    # identical keys: every match either cancels or survives
    a_rows, a_accs, b_rows, b_accs = C.mc_shape_case("identical_1030", 2, 8)
    rows, accs, rep = C.mc_oracle(a_rows, a_accs, b_rows, b_accs)
    assert 0 < len(rows) < 1030 and all(r < 1030 for r in rep)


# --------------------------------------------------------------- partition --


def test_partition_patterns():
    n = 1000
    for world in C.PART_WORLDS:
        for pattern in C.PART_PATTERNS:
            for size in (0, 1, n):
                d = C.partition_dest(pattern, size, world)
                assert d.dtype == torch.int64 and d.shape == (size,)
                assert size == 0 or (0 <= int(d.min()) and int(d.max()) < world)
        used = lambda p: set(C.partition_dest(p, n, world).tolist())  # noqa: E731
        assert used("all_first") == {0} and used("all_last") == {world - 1}
        assert used("round_robin") == set(range(world))
        if world > 1:
            assert used("one_unused") == set(range(world)) - {world // 2}
        asc = C.partition_dest("ascending", n, world)
        assert bool((asc[1:] >= asc[:-1]).all()) and set(asc.tolist()) == set(range(world))
        assert torch.equal(C.partition_dest("descending", n, world), asc.flip(0))


def test_check_partition_accepts_and_rejects():
    dest = C.partition_dest("round_robin", 10, 3)
    perm = torch.argsort(dest, stable=True)
    counts = torch.bincount(dest, minlength=3)
    C.check_partition(dest, 3, perm, counts)
    # any order inside a destination will do
    swapped = perm.clone()
    swapped[0], swapped[1] = perm[1], perm[0]  # both rows go to destination 0
    C.check_partition(dest, 3, swapped, counts)
    for bad_perm, bad_counts in (
        (perm.flip(0), counts),  # grouped downwards
        (torch.arange(10), counts),  # not grouped
        (perm.clamp(max=8), counts),  # a row twice, a row missing
        (perm, counts + torch.tensor([1, -1, 0])),
        (perm, counts[:2]),
    ):
        with pytest.raises(AssertionError):
            C.check_partition(dest, 3, bad_perm, bad_counts)


# -------------------------------------------------------------- radix sort --


def test_radix_key_sets():
    n = 4097
    assert set(C.radix_keys("specials", n).tolist()) == set(C.SPECIALS)
    assert len(set(C.radix_keys("all_equal", n).tolist())) == 1
    rnd = C.radix_keys("random", n)
    assert C.INT64_MIN in rnd.tolist() and C.INT64_MAX in rnd.tolist()
    assert len(set(rnd.tolist())) == n - 1  # one key twice
    srt, rev = C.radix_keys("sorted", n), C.radix_keys("reversed", n)
    assert torch.equal(srt, torch.sort(rnd).values) and torch.equal(rev, srt.flip(0))
    for p in range(8):
        k = C.radix_keys(f"pass_{p}", n)
        vals = set(k.tolist())
        assert vals == {C.wrap64(d << (8 * p)) for d in range(256)}
        assert all(v & C.MASK64 & ~(0xFF << (8 * p)) == 0 for v in vals)
        assert not torch.equal(k, torch.sort(k).values)
    top = C.radix_keys("pass_7", n)
    assert bool((top < 0).any()) and bool((top > 0).any())
    assert int(top.min()) == C.INT64_MIN
    for name in C.RS_KEY_SETS:
        for size in C.RS_N[:4]:
            assert C.radix_keys(name, size).shape == (size,)
    # a stable and an unstable sort differ on these keys, so perm is checked
    k = C.radix_keys("specials", 65)
    stable = torch.sort(k, stable=True).indices
    assert not torch.equal(stable, torch.sort(k, descending=True).indices.flip(0))


def test_radix_cap_keys():
    k = C.radix_cap_keys()
    assert k.shape == (C.RS_N_CAP,) and k.dtype == torch.int64
    assert int(k.min()) == C.INT64_MIN and int(k.max()) == C.INT64_MAX
    uniq = torch.unique(k).shape[0]
    assert uniq < C.RS_N_CAP * 0.51  # nearly every key comes twice


# ------------------------------------------------------------------ gather --


def test_gather_columns_and_indices():
    n = C.GATHER_SRC_N
    for ncols in C.GATHER_NCOLS:
        cols = C.gather_fused_cols(ncols)
        assert len(cols) == ncols
        assert all(c.shape == (n,) and c.element_size() == 8 and c.is_contiguous() for c in cols)
        assert cols[0].dtype == torch.int64 and cols[0][:5].tolist() == list(C.SPECIALS)
        if ncols > 1:
            f = cols[1]
            assert f.dtype == torch.float64
            assert int(f[:10].isnan().sum()) == 5 and int(f[:10].isinf().sum()) == 2
            assert C.bits(f)[5].item() == C.INT64_MIN and f[5].item() == 0.0  # -0.0
            # the NaNs differ as bits, which an equality of floats cannot see
            assert len(set(C.bits(f)[:5].tolist())) == 5
    mixed = C.gather_mixed_cols()
    fused = [c.dim() == 1 and c.element_size() == 8 and c.is_contiguous() for c in mixed]
    assert fused == [True, False, True, False, False, False, True, True]
    assert [c.dtype for c in mixed[1:6]] == [
        torch.int32, torch.float64, torch.bool, torch.int64, torch.int64,
    ]
    assert mixed[4].shape == (n, 2) and mixed[5].stride() == (2,)
    assert all(c.shape[0] == n for c in mixed)
    for m in C.GATHER_M:
        idx = C.gather_index("random", m)
        assert idx.shape == (m,) and idx.dtype == torch.int64
        assert m == 0 or (0 <= int(idx.min()) and int(idx.max()) < n)
        if m >= 2:
            assert int(idx[0]) == n - 1 and int(idx[-1]) == 0
    assert set(C.gather_index("all_equal", 257).tolist()) == {n - 1}
    assert C.gather_index("identity", n).tolist() == list(range(n))
    assert C.gather_index("reversed", n).tolist() == list(range(n - 1, -1, -1))
    # the oracle against plain indexing
    idx = C.gather_index("random", 257)
    for got, c in zip(C.gather_oracle(idx, mixed), mixed):
        assert got.dtype == c.dtype
        assert torch.equal(C.bits(got), C.bits(c[idx]))

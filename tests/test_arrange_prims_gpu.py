"""GPU tests of the arrange-path primitives at their edges, each wrapper of
pathway_amd.ops called directly and compared exactly with a plain oracle:
the row hashes at every width and past one grid, the merge-consolidate walk
with signed multi-word ties and comparison prefixes, the destination
partition, the radix sort digit by digit and at its block cap, and the fused
gather.  Inputs and oracles are in tests/arrange_cases.py."""

import pytest
import torch

from tests import arrange_cases as C
from tests import state_prims_cases as S

gpu = pytest.mark.gpu

requires_cuda = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

DEV = "cuda:0"


def _dev(cols):
    return [c.to(DEV) for c in cols]


# -------------------------------------------------------------- row hashes --


@gpu
@requires_cuda
@pytest.mark.parametrize("W", C.HASH_W)
def test_hash128_words_every_width(W):
    from pathway_amd import ops

    rows = C.hash_rows(W)
    lo, hi = ops.hash128_words_gpu(C.columns(rows, W, DEV))
    assert lo.dtype == torch.int64 and hi.dtype == torch.int64
    got = list(zip(lo.cpu().tolist(), hi.cpu().tolist()))
    want = [C.py_hash128(r) for r in rows]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"W={W} row {i} {rows[i]}"
    assert len(got) == len(want)


@gpu
@requires_cuda
@pytest.mark.parametrize("W", C.HASH_GRID_W)
def test_hash128_words_second_grid_trip(W):
    from pathway_amd import ops
    from pathway_amd.engine import hashing
    from pathway_amd.internals import api

    words = C.hash_grid_words(W)
    lo, hi = ops.hash128_words_gpu(_dev(words))
    assert torch.equal(lo.cpu(), hashing.xxh64_words(words, api.SEED_LO)), f"W={W} lo"
    assert torch.equal(hi.cpu(), hashing.xxh64_words(words, api.SEED_HI)), f"W={W} hi"


@gpu
@requires_cuda
def test_hash128_words_sizes():
    from pathway_amd import ops

    rows = C.hash_rows(2)
    for n in C.HASH_SIZES:
        lo, hi = ops.hash128_words_gpu(C.columns(rows[:n], 2, DEV))
        for t in (lo, hi):
            assert t.shape == (n,) and t.dtype == torch.int64 and t.is_cuda
        got = list(zip(lo.cpu().tolist(), hi.cpu().tolist()))
        assert got == [C.py_hash128(r) for r in rows[:n]], f"n={n}"


@gpu
@requires_cuda
def test_hash128_words_strided_views():
    from pathway_amd import ops

    # words as columns of a row-major (n, 3) tensor and as every other
    # element of a longer one: the hash is of the values the views hold
    rows = C.hash_rows(3)
    n = len(rows)
    t = torch.tensor(rows, dtype=torch.int64, device=DEV)
    long = torch.full((2 * n,), 12345, dtype=torch.int64, device=DEV)
    long[::2] = t[:, 2]
    words = [t[:, 0], t[:, 1], long[::2]]
    assert not any(w.is_contiguous() for w in words)
    lo, hi = ops.hash128_words_gpu(words)
    got = list(zip(lo.cpu().tolist(), hi.cpu().tolist()))
    assert got == [C.py_hash128(r) for r in rows]


@gpu
@requires_cuda
def test_hash128_words_refusals():
    from pathway_amd import ops

    col = torch.zeros(4, dtype=torch.int64, device=DEV)
    lo, hi = ops.hash128_words_gpu([col] * C.HASH_MAX_WORDS)
    assert lo.shape == (4,)
    with pytest.raises((ValueError, RuntimeError)):
        ops.hash128_words_gpu([col] * (C.HASH_MAX_WORDS + 1))
    with pytest.raises((ValueError, RuntimeError)):
        ops.hash128_words_gpu([])
    with pytest.raises(ValueError):  # one length
        ops.hash128_words_gpu([col, col[:3]])
    with pytest.raises(ValueError):
        ops.hash128_words_gpu([col[:3], col])
    with pytest.raises(ValueError):  # one device
        ops.hash128_words_gpu([col, col.cpu()])
    with pytest.raises(ValueError):  # int64
        ops.hash128_words_gpu([col, col.to(torch.int32)])
    with pytest.raises(ValueError):
        ops.hash128_words_gpu([col.to(torch.float64)])
    with pytest.raises(ValueError):  # 1-D
        ops.hash128_words_gpu([col.reshape(2, 2), col.reshape(2, 2)])


@gpu
@requires_cuda
@pytest.mark.parametrize("tag", C.VALUE_TAGS)
def test_value_hash_every_tag(tag):
    from pathway_amd import ops
    from pathway_amd.engine import hashing
    from pathway_amd.internals import api

    for n in C.VALUE_N:
        payload = C.value_payload(n)
        lo, hi = ops.value_hash_gpu(payload.to(DEV), tag)
        assert lo.shape == (n,) and lo.dtype == torch.int64
        lo, hi = lo.cpu(), hi.cpu()
        want_lo, want_hi = hashing.hash128_words([torch.full_like(payload, tag), payload])
        assert torch.equal(lo, want_lo) and torch.equal(hi, want_hi), f"tag={tag} n={n}"
        if tag == api.TAG_INT:
            sample = sorted(set(range(0, n, max(1, n // 40))) | set(range(min(n, 5))) | {n - 1})
            for i in sample:
                want = api.hash128(api.serialize_value(int(payload[i])))
                got = (int(lo[i]) & C.MASK64, int(hi[i]) & C.MASK64)
                assert got == want, f"n={n} row {i}"


# ------------------------------------------------------- merge-consolidate --


def _merge(a_rows, a_accs, b_rows, b_accs, nw, compare_words=None):
    """merge_consolidate_gpu over Python rows; (rows, accs, rep) as lists."""
    from pathway_amd import ops

    t = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)  # noqa: E731
    out_words, out_accs, rep = ops.merge_consolidate_gpu(
        C.columns(a_rows, nw, DEV),
        [t(c) for c in a_accs],
        C.columns(b_rows, nw, DEV),
        [t(c) for c in b_accs],
        **({} if compare_words is None else {"compare_words": compare_words}),
    )
    assert len(out_words) == nw and len(out_accs) == len(a_accs)
    for x in out_words + out_accs + [rep]:
        assert x.dtype == torch.int64 and x.shape == rep.shape
    rows = list(zip(*(w.cpu().tolist() for w in out_words)))
    return rows, [a.cpu().tolist() for a in out_accs], rep.cpu().tolist()


def _check_merge(case, nw, compare_words=None, where=""):
    a_rows, a_accs, b_rows, b_accs = case
    want_rows, want_accs, want_rep = C.mc_oracle(
        a_rows, a_accs, b_rows, b_accs, compare_words
    )
    rows, accs, rep = _merge(a_rows, a_accs, b_rows, b_accs, nw, compare_words)
    assert rows == want_rows, f"{where}: rows"
    assert accs == want_accs, f"{where}: accumulators"
    assert rep == want_rep, f"{where}: rep"


@gpu
@requires_cuda
@pytest.mark.parametrize("nacc", C.MC_NACC)
@pytest.mark.parametrize("nw", C.MC_NW)
def test_merge_consolidate_signed_ties_and_accumulators(nw, nacc):
    a, b = C.mc_sides(nw)
    a_accs, b_accs = C.mc_accs(a, b, nacc)
    _check_merge((a, a_accs, b, b_accs), nw, where=f"nw={nw} nacc={nacc}")
    # and with the sides swapped: rep and the carried words follow A
    _check_merge((b, b_accs, a, a_accs), nw, where=f"swapped nw={nw} nacc={nacc}")


@gpu
@requires_cuda
@pytest.mark.parametrize("nw", C.MC_NW)
def test_merge_consolidate_shapes(nw):
    for shape in C.MC_SHAPES:
        for nacc in C.MC_NACC:
            case = C.mc_shape_case(shape, nw, nacc)
            _check_merge(case, nw, where=f"{shape} nw={nw} nacc={nacc}")


@gpu
@requires_cuda
def test_merge_consolidate_compare_words_prefix():
    a, b = C.mc_tail_function_case()
    a_accs, b_accs = C.mc_accs(a, b, 8, nwc=2)
    for nwc in (2, 4):
        _check_merge((a, a_accs, b, b_accs), 4, nwc, where=f"tail function nwc={nwc}")

    case = C.mc_tail_differs_case()
    a, a_accs, b, b_accs = case
    _check_merge(case, 4, 2, where="tail differs nwc=2")
    _check_merge(case, 4, 4, where="tail differs nwc=4")
    rows2, accs2, rep2 = _merge(a, a_accs, b, b_accs, 4, 2)
    at = rows2.index((1, 2, 10, 11))  # merged, A's tail
    assert (1, 2, 99, -98) not in rows2 and rep2[at] == 1 and accs2[0][at] == 8
    rows4, _, rep4 = _merge(a, a_accs, b, b_accs, 4, 4)
    assert (1, 2, 10, 11) in rows4 and (1, 2, 99, -98) in rows4  # both survive
    assert rep4[rows4.index((1, 2, 99, -98))] == len(a) + 1


# --------------------------------------------------------------- partition --


@gpu
@requires_cuda
@pytest.mark.parametrize("world", C.PART_WORLDS)
def test_partition_patterns_and_sizes(world):
    from pathway_amd import ops

    for pattern in C.PART_PATTERNS:
        for n in C.PART_N:
            dest = C.partition_dest(pattern, n, world)
            perm, counts = ops.partition_gpu(dest.to(DEV), world)
            assert perm.is_cuda and counts.is_cuda
            try:
                C.check_partition(dest, world, perm.cpu(), counts.cpu())
            except AssertionError as e:
                raise AssertionError(f"{pattern} world={world} n={n}: {e}") from e


@gpu
@requires_cuda
def test_partition_refusals():
    from pathway_amd import ops

    dest = torch.zeros(10, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        ops.partition_gpu(dest, C.PART_MAX_DEST + 1)
    with pytest.raises(ValueError):
        ops.partition_gpu(dest, 0)
    with pytest.raises(ValueError):
        ops.partition_gpu(dest, -1)
    with pytest.raises(ValueError):
        ops.partition_gpu(dest.to(torch.int32), 2)
    with pytest.raises(ValueError):
        ops.partition_gpu(dest.reshape(5, 2), 2)


# -------------------------------------------------------------- radix sort --


def _check_radix(keys, where):
    from pathway_amd import ops

    want = torch.sort(keys, stable=True)
    got_keys, got_perm = ops.radix_sort64_gpu(keys.to(DEV))
    assert got_keys.dtype == torch.int64 and got_perm.dtype == torch.int64
    assert torch.equal(got_keys.cpu(), want.values), f"{where}: keys"
    assert torch.equal(got_perm.cpu(), want.indices), f"{where}: perm (stability)"


@gpu
@requires_cuda
@pytest.mark.parametrize("name", C.RS_KEY_SETS)
def test_radix_sort_key_sets(name):
    for n in C.RS_N:
        _check_radix(C.radix_keys(name, n), f"{name} n={n}")


@gpu
@requires_cuda
def test_radix_sort_at_the_block_cap():
    _check_radix(C.radix_cap_keys(), f"n={C.RS_N_CAP}")


@gpu
@requires_cuda
def test_lex_sort_words_through_the_radix_sort(monkeypatch):
    from pathway_amd import ops
    from pathway_amd.engine import state

    k0, k1 = S.lex_case()
    words = [k0.to(DEV), k1.to(DEV)]
    default = state.lex_sort_words(words).cpu()
    calls = []
    real = ops.radix_sort64_gpu

    def counted(keys):
        calls.append(keys.shape[0])
        return real(keys)

    monkeypatch.setattr(ops, "radix_sort64_gpu", counted)
    monkeypatch.setattr(state, "_PW_PW_SORT", True)
    perm = state.lex_sort_words(words).cpu()
    assert calls == [S.LEX_N], "the radix sort did not run"
    assert sorted(perm.tolist()) == list(range(S.LEX_N))
    rows = torch.stack([k0, k1], 1)
    assert torch.equal(rows[perm], rows[default])
    assert rows[perm].tolist() == sorted(rows.tolist())


# ------------------------------------------------------------------ gather --


def _check_gather(idx, cols, where):
    from pathway_amd import ops

    got = ops.gather_cols_gpu(idx.to(DEV), _dev(cols))
    want = C.gather_oracle(idx, cols)
    assert len(got) == len(want), where
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{where} column {c}"
        assert torch.equal(C.bits(g.cpu()), C.bits(w)), f"{where} column {c}"


@gpu
@requires_cuda
@pytest.mark.parametrize("ncols", C.GATHER_NCOLS)
def test_gather_cols_counts_and_indices(ncols):
    cols = C.gather_fused_cols(ncols)
    for m in C.GATHER_M:
        _check_gather(C.gather_index("random", m), cols, f"ncols={ncols} m={m}")
    n = C.GATHER_SRC_N
    _check_gather(C.gather_index("all_equal", 257), cols, f"ncols={ncols} all equal")
    _check_gather(C.gather_index("identity", n), cols, f"ncols={ncols} identity")
    _check_gather(C.gather_index("reversed", n), cols, f"ncols={ncols} reversed")


@gpu
@requires_cuda
def test_gather_cols_second_grid_trip():
    cols = C.gather_fused_cols(C.GATHER_COLS + 1)
    idx = C.gather_index("random", C.GATHER_TRIP)
    _check_gather(idx, cols, f"m={C.GATHER_TRIP}")


@gpu
@requires_cuda
def test_gather_cols_mixed_columns_keep_place_and_dtype():
    from pathway_amd import ops

    cols = C.gather_mixed_cols()
    dev_cols = _dev(cols[:5]) + [C.gather_int_col(2 * C.GATHER_SRC_N, 21).to(DEV)[::2]] + _dev(cols[6:])
    assert not dev_cols[5].is_contiguous()
    assert torch.equal(dev_cols[5].cpu(), cols[5])
    for m in (0, 1, 257):
        idx = C.gather_index("random", m)
        got = ops.gather_cols_gpu(idx.to(DEV), dev_cols)
        want = C.gather_oracle(idx, cols)
        assert len(got) == len(cols)
        for c, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape, f"m={m} column {c}"
            assert torch.equal(C.bits(g.cpu()), C.bits(w)), f"m={m} column {c}"


@gpu
@requires_cuda
def test_gather_all_switches_to_the_fused_kernel(monkeypatch):
    from pathway_amd import ops

    calls = []
    real = ops.gather_cols_gpu

    def counted(idx, cols):
        calls.append(idx.shape[0])
        return real(idx, cols)

    monkeypatch.setattr(ops, "gather_cols_gpu", counted)
    cols = C.gather_mixed_cols()
    dev_cols = _dev(cols)
    for m, fused in ((C.GATHER_ALL_SWITCH, False), (C.GATHER_ALL_SWITCH + 1, True)):
        idx = C.gather_index("random", m)
        calls.clear()
        got = ops.gather_all(idx.to(DEV), dev_cols)
        assert calls == ([m] if fused else []), f"m={m}"
        for c, (g, w) in enumerate(zip(got, C.gather_oracle(idx, cols))):
            assert g.dtype == w.dtype and g.shape == w.shape, f"m={m} column {c}"
            assert torch.equal(C.bits(g.cpu()), C.bits(w)), f"m={m} column {c}"

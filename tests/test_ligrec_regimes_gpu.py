"""GPU tests of every kernel configuration `sqgr_ligrec_counts` chooses (squidpy_amd/csrc/sqgr_ligrec.hip), against the CPU oracle:

  * every cluster-count regime of the host code: 4 / 2 / 1 waves per block of the sum kernel (K <= 80, <= 160, <= 256), the score
    kernel within and beyond 64 KiB of LDS (K <= 124 / >= 125), both sides of the 8-bit | tiled switch (256 | 257), two full
    tiles (510) and a ragged third one (511);
  * thresholds planted ON the permuted sums of every permutation (tests/ligrec_cases.py, proved last-bit sensitive by
    tests/test_ligrec_cases_cpu.py): the float64 sums of every lane of the wave are checked to the last bit, not only those of
    the first permutation that the `return_first_groups` hook shows;
  * planted column lengths around the 64-entry trip and its padding to 16, the 256-pair block edge of the score kernel;
  * permutation ranges beyond one launch chunk of 16384 (both generators, narrow and tiled), and the same through the front end.

All comparisons are `assert_array_equal` on int64 counts and float64 group means.  The configuration a call really ran is read
back from the context's launch timers."""

from __future__ import annotations

import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import restate as O
from squidpy_amd import AnnDataLite
from squidpy_amd._utils import pcg64_states
from tests import ligrec_cases as C

pytestmark = pytest.mark.gpu

GENERATORS = ("numpy", "philox")
NP_SEED, DEV_SEED = 11, 1234


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def launches(ctx, fn):
    """run fn() with the launch timers on -> (result, {kernel name: number of launches})"""
    ctx.timer_enable(True)
    ctx.timer_reset()
    try:
        out = fn()
        rep = ctx.timer_report()
    finally:
        ctx.timer_enable(False)
    return out, {name: cnt for name, (cnt, _) in rep.items() if cnt > 0}


def n_tiles(k: int) -> int:
    return -(-k // 255) if k > 256 else 1


def check_launches(names: dict, k: int, chunks: int = 1):
    """the sum kernel once per cluster tile and launch chunk, the tile relabelling only beyond 256 clusters, one score launch per chunk"""
    assert names.get("ligrec_sums") == n_tiles(k) * chunks, names
    assert names.get("ligrec_score") == chunks, names
    assert names.get("ligrec_tile_labels", 0) == (n_tiles(k) * chunks if k > 256 else 0), names


def labels_of(cl: np.ndarray, generator: str, seed: int, begin: int, end: int) -> np.ndarray:
    """label vectors of the permutations [begin, end) (numpy streams: of `end` streams in all)"""
    if generator == "numpy":
        return O.ligrec_perm_labels_numpy(cl, seed, end)[begin:]
    return C.philox_labels(cl, seed, begin, end)


def device_counts(L, ctx, generator, data, cl, k, inv, inter, cp, obs, valid, seed, begin, end, n_streams=None, **kw):
    """`ligrec_counts` of the permutations [begin, end) under either generator (numpy streams: out of `n_streams` in all)"""
    if generator == "numpy":
        kw["pcg_states"] = pcg64_states(seed, end if n_streams is None else n_streams)[begin:end]
    else:
        kw["seed"] = seed
    return L.ligrec_counts(ctx, sp.csc_matrix(data), cl, k, inv, inter, cp, obs, np.asarray(valid, dtype=np.uint8), perm_begin=begin, perm_end=end, **kw)


def perm_range(generator: str) -> tuple[int, int, int]:
    """(seed, begin, end): 130 numpy streams — lanes 0..63, a second group of 64 and a partial tail —, or 70 permutations of the
    device generator that start inside a group of 16"""
    return (NP_SEED, 0, C.N_NUMPY) if generator == "numpy" else (DEV_SEED, C.DEVICE_BEGIN, C.DEVICE_BEGIN + C.N_DEVICE)


# ------------------------------------------------------------------------------------------- a. every regime, both generators
@pytest.mark.parametrize("generator", GENERATORS)
@pytest.mark.parametrize("k", [80, 81, 124, 125, 160, 161, 255, 256, 257, 510, 511])
def test_every_cluster_count_regime(L, ctx, k, generator):
    n = max(320, 4 * k)
    data, cl, inter = C.problem(n, 6, k, seed=1000 + k, n_inter=12)
    cp = C.cluster_pairs(k, 300, seed=2000 + k)
    assert {(0, k - 1), (k - 1, 0)} <= {tuple(p) for p in cp} and (np.bincount(cl, minlength=k) > 0).all()
    pre = O.ligrec_prepare(data, cl, inter, cp, threshold=0.0)
    seed, begin, end = perm_range(generator)
    labels = labels_of(cl, generator, seed, begin, end)
    want = O.ligrec_score_permutations(data, labels, pre["inv_counts"], pre["mean_obs"], inter, cp, pre["valid"])
    (got, groups), names = launches(
        ctx, lambda: device_counts(L, ctx, generator, data, cl, k, pre["inv_counts"], inter, cp, pre["obs"], pre["valid"], seed, begin, end, return_first_groups=True)
    )
    check_launches(names, k)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(groups, O.ligrec_group_means(data, labels[0], pre["inv_counts"]))
    assert want.sum() > 0 and not (want == end - begin).all()


# -------------------------------------------------------------------------------------------- b. planted ties in every lane
def check_planted(L, ctx, generator, data, cl, k, inv, inter, cp, labels, seed, begin, end, valid, perms=None, n_streams=None, chunks=1):
    obs, tie, below = C.planted_obs(data, labels, inv, inter, cp, perms)
    want = C.score_with_obs(data, labels, inv, obs, inter, cp, valid)
    (got, groups), names = launches(
        ctx, lambda: device_counts(L, ctx, generator, data, cl, k, inv, inter, cp, obs, valid, seed, begin, end, n_streams=n_streams, return_first_groups=True)
    )
    check_launches(names, k, chunks)
    # separately: a failure names the side that broke (a tie counted: a sum came out too high or `>` became `>=`; a below cell
    # not counted: a sum came out too low)
    np.testing.assert_array_equal(got[tie], want[tie], err_msg="cells whose threshold IS a permuted sum")
    np.testing.assert_array_equal(got[below], want[below], err_msg="cells whose threshold is one ulp below a permuted sum")
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(groups, O.ligrec_group_means(data, labels[0], inv))
    assert (got[~valid] == 0).all() and want.sum() > 0
    return got


@pytest.mark.parametrize("generator", GENERATORS)
@pytest.mark.parametrize("k", sorted(C.PLANTED_SHAPES))
def test_planted_ties_in_every_lane(L, ctx, k, generator):
    data, cl, inter, cp, inv = C.planted_case(k)
    seed, begin, end = perm_range(generator)
    labels = labels_of(cl, generator, seed, begin, end)
    valid = C.sparse_valid((len(inter), len(cp)), seed=k)
    check_planted(L, ctx, generator, data, cl, k, inv, inter, cp, labels, seed, begin, end, valid)


# ------------------------------------------------------------------------------------------------ c. planted column lengths
@pytest.mark.parametrize("generator", GENERATORS)
@pytest.mark.parametrize("k", [4, 200])
def test_planted_column_lengths(L, ctx, k, generator):
    """columns of 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200 stored entries: none, one lane, either side of the padding to
    16 and of the 64-entry trip; three padded columns hold a value at cell 0, where the padding adds its +0.0"""
    data, cl, inter, cp, inv = C.lengths_case(k)
    np.testing.assert_array_equal(np.diff(sp.csc_matrix(data).indptr), C.COLUMN_LENGTHS)
    seed, begin, end = perm_range(generator)
    labels = labels_of(cl, generator, seed, begin, end)
    valid = np.ones((len(inter), len(cp)), dtype=bool)
    check_planted(L, ctx, generator, data, cl, k, inv, inter, cp, labels, seed, begin, end, valid)


# --------------------------------------------------------------------------------------------------------- d. score-block edge
@pytest.mark.parametrize("n_cp", [255, 256, 257])
def test_score_block_edge(L, ctx, n_cp):
    data, cl, inter, cp, inv = C.edge_case(n_cp)
    labels = labels_of(cl, "numpy", NP_SEED, 0, C.N_EDGE)
    valid = np.ones((len(inter), n_cp), dtype=bool)
    got = check_planted(L, ctx, "numpy", data, cl, 20, inv, inter, cp, labels, NP_SEED, 0, C.N_EDGE, valid)
    assert got.shape == (len(inter), n_cp)


# ------------------------------------------------------------------------------------------ e. more than one launch chunk
N_CHUNKED = C.NPL_CAP + 64 + 37


@functools.lru_cache(maxsize=None)
def chunk_reference(wide: bool, generator: str, seed: int, begin: int, end: int):
    """(case, prepared statistics, label vectors of [begin, end)) — computed once, read-only"""
    data, cl, inter, cp, inv, k = C.chunk_case(wide)
    pre = O.ligrec_prepare(data, cl, inter, cp, threshold=0.0)
    labels = labels_of(cl, generator, seed, begin, end)
    for a in (labels, pre["obs"], pre["valid"]):
        a.setflags(write=False)
    return (data, cl, inter, cp, inv, k), pre, labels


def oracle_counts(case, pre, labels):
    data, cl, inter, cp, inv, k = case
    return C.score_with_obs(data, labels, inv, pre["obs"], inter, cp, pre["valid"])


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "tiled"])
def test_two_launch_chunks_numpy_streams(L, ctx, wide):
    """16384 + 64 + 37 numpy streams: the second chunk reads its PCG64 states, writes its labels and adds its counts at the
    right offsets; the stale label columns of the short last chunk are cleared"""
    case, pre, labels = chunk_reference(wide, "numpy", 3, 0, N_CHUNKED)
    data, cl, inter, cp, inv, k = case

    def run(a, b):
        return launches(ctx, lambda: device_counts(L, ctx, "numpy", data, cl, k, inv, inter, cp, pre["obs"], pre["valid"], 3, a, b, n_streams=N_CHUNKED))

    want = oracle_counts(case, pre, labels)
    assert want.sum() > 0 and not (want == N_CHUNKED).all()
    full, names = run(0, N_CHUNKED)
    check_launches(names, k, chunks=2)
    np.testing.assert_array_equal(full, want)
    for split in (C.NPL_CAP, C.NPL_CAP + 70):
        (head, n_head), (tail, n_tail) = run(0, split), run(split, N_CHUNKED)
        check_launches(n_head, k, chunks=1 if split == C.NPL_CAP else 2)
        check_launches(n_tail, k, chunks=1)
        np.testing.assert_array_equal(tail, oracle_counts(case, pre, labels[split:]), err_msg=f"[{split}, {N_CHUNKED})")
        np.testing.assert_array_equal(full, head + tail, err_msg=f"split at {split}")


def test_planted_ties_either_side_of_the_chunk_border(L, ctx):
    """thresholds on the sums of permutation 16383 (last of the first chunk), 16384 (first of the second) and the last one"""
    case, pre, labels = chunk_reference(False, "numpy", 3, 0, N_CHUNKED)
    data, cl, inter, cp, inv, k = case
    valid = np.ones((len(inter), len(cp)), dtype=bool)
    perms = [C.NPL_CAP - 1, C.NPL_CAP, N_CHUNKED - 1]
    check_planted(L, ctx, "numpy", data, cl, k, inv, inter, cp, labels, 3, 0, N_CHUNKED, valid, perms=perms, chunks=2)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "tiled"])
def test_two_launch_chunks_device_generator(L, ctx, wide):
    """[5, 16384 + 105): the second chunk starts at permutation 16384 of the generator, and the 5 columns in front of the range
    are left out of the first chunk only.  The generator's restatement is too slow for the whole range: the two parts are
    single-chunk calls, and the second one is compared with the oracle."""
    begin, end = C.DEVICE_BEGIN, C.NPL_CAP + 105
    case, pre, labels = chunk_reference(wide, "philox", 77, C.NPL_CAP, end)
    data, cl, inter, cp, inv, k = case

    def run(a, b):
        return launches(ctx, lambda: device_counts(L, ctx, "philox", data, cl, k, inv, inter, cp, pre["obs"], pre["valid"], 77, a, b))

    full, names = run(begin, end)
    check_launches(names, k, chunks=2)
    (head, n_head), (tail, n_tail) = run(begin, C.NPL_CAP), run(C.NPL_CAP, end)
    check_launches(n_head, k, chunks=1)
    check_launches(n_tail, k, chunks=1)
    np.testing.assert_array_equal(full, head + tail)
    want_tail = oracle_counts(case, pre, labels)
    np.testing.assert_array_equal(tail, want_tail)
    assert want_tail.sum() > 0 and not (want_tail == end - C.NPL_CAP).all()


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "tiled"])
def test_two_launch_chunks_behind_skipped_columns(L, ctx, wide):
    """a range that starts inside a group of 16 of the generator (13 skipped columns in front) and is long enough for two
    chunks: the second one starts at permutation begin - 13 + 16384 and skips nothing.  The narrow case is compared with the
    oracle over the whole range (0.2 ms per permutation at 96 cells); the tiled one with its two single-chunk parts, the second
    of them and the first group means with the oracle."""
    begin = C.NPL_CAP - 3
    border = begin - begin % 16 + C.NPL_CAP
    end = border + 13
    assert begin % 16 == 13 and end - begin + begin % 16 > C.NPL_CAP
    case, pre, labels = chunk_reference(wide, "philox", 78, border if wide else begin, end)
    data, cl, inter, cp, inv, k = case

    def run(a, b, **kw):
        return launches(ctx, lambda: device_counts(L, ctx, "philox", data, cl, k, inv, inter, cp, pre["obs"], pre["valid"], 78, a, b, **kw))

    (got, groups), names = run(begin, end, return_first_groups=True)
    check_launches(names, k, chunks=2)
    np.testing.assert_array_equal(groups, O.ligrec_group_means(data, C.philox_labels(cl, 78, begin, begin + 1)[0], inv))
    if not wide:
        want = oracle_counts(case, pre, labels)
        np.testing.assert_array_equal(got, want)
        assert want.sum() > 0 and not (want == end - begin).all()
    else:
        (head, n_head), (tail, n_tail) = run(begin, border), run(border, end)
        check_launches(n_head, k, chunks=1)
        check_launches(n_tail, k, chunks=1)
        np.testing.assert_array_equal(tail, oracle_counts(case, pre, labels))
        np.testing.assert_array_equal(got, head + tail)


# ------------------------------------------------------------------------------------------------------------- f. front end
def _adata_from(data, cl):
    var = pd.DataFrame(index=[f"G{i}" for i in range(data.shape[1])])
    obs = pd.DataFrame({"cluster": pd.Categorical([f"c{c}" for c in cl])})
    return AnnDataLite(X=sp.csr_matrix(data), obs=obs, var=var)


def test_front_end_more_permutations_than_one_chunk(ctx):
    """16500 permutations of 96 cells, 3 genes, 2 clusters through `ligrec`: the oracle's `_analysis` for the same seed, exactly"""
    import squidpy_amd as sq

    data, cl, inter, cp, inv, k = C.chunk_case(False)
    res, names = launches(
        ctx,
        lambda: sq.gr.ligrec(_adata_from(data, cl), "cluster", interactions=[(f"G{s}", f"G{t}") for s, t in inter], threshold=0.0,
                             n_perms=16500, seed=3, rng="numpy", use_raw=False, copy=True),
    )
    check_launches(names, k, chunks=2)
    _, pv = O.ligrec_analysis(data, cl, inter, cp, threshold=0.0, n_perms=16500, seed=3)
    got = res["pvalues"].to_numpy(dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(pv))
    np.testing.assert_array_equal(got, pv)  # NaN == NaN here
    assert np.nanmax(pv) > 0 and np.nanmin(pv) < 1


def test_front_end_256_clusters(ctx):
    """256 clusters through the front end: the last cluster count with 8-bit labels (label 255), no cluster tiles"""
    import squidpy_amd as sq

    k = 256
    data, cl, inter = C.problem(4 * k, 5, k, seed=8, density=0.6, n_inter=6)
    res, names = launches(
        ctx,
        lambda: sq.gr.ligrec(_adata_from(data, cl), "cluster", interactions=[(f"G{s}", f"G{t}") for s, t in inter], threshold=0.0,
                             n_perms=20, seed=4, use_raw=False, copy=True, rng="numpy"),
    )
    check_launches(names, k)
    # the front end codes the clusters in category order (strings: "c0", "c1", "c10", "c100", ...)
    code = {c: i for i, c in enumerate(sorted(f"c{c}" for c in range(k)))}
    lab = np.array([code[f"c{c}"] for c in cl], dtype=np.int32)
    cp = np.array([(a, b) for a in range(k) for b in range(k)], dtype=np.int32)
    _, pv = O.ligrec_analysis(data, lab, inter, cp, threshold=0.0, n_perms=20, seed=4)
    got = res["pvalues"].to_numpy(dtype=np.float64)
    assert got.shape == (len(inter), k * k)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(pv))
    np.testing.assert_array_equal(got, pv)

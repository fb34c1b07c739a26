"""GPU parity tests of the nhood_enrichment path: libsqgr (HIP) vs the CPU oracle.  Integer results are
compared bit for bit; z-scores at the tolerance written next to each assertion."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O
from tests.helpers import codes, hex_adata, knn_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _golden_graph(golden):
    n = len(golden["nhood_indptr"]) - 1
    return sp.csr_matrix(
        (np.ones(len(golden["nhood_indices"]), np.float32), golden["nhood_indices"], golden["nhood_indptr"]), shape=(n, n)
    )


def test_counts_match_reference_kernel_golden(L, ctx, golden):
    g = L.Graph(ctx, _golden_graph(golden))
    k = int(golden["nhood_k"])
    c = L.nhood_counts(ctx, g, golden["nhood_labels"], k)
    assert c.dtype == np.uint32
    np.testing.assert_array_equal(c, golden["nhood_count"])  # bit-exact integer counts


def test_interaction_matrix_known_answers(L, ctx, golden):
    """reference tests/graph/test_nhood.py:153-173."""
    n = 5
    adj = sp.csr_matrix((golden["intmat_data"].astype(np.float32), golden["intmat_indices"], golden["intmat_indptr"]), shape=(n, n))
    g = L.Graph(ctx, adj)
    np.testing.assert_array_equal(L.interaction_matrix(ctx, g, golden["intmat_cats"], 2, True), [[5, 1], [2, 3]])
    np.testing.assert_array_equal(L.interaction_matrix(ctx, g, golden["intmat_cats"], 2, False), [[4, 1], [2, 2]])
    np.testing.assert_array_equal(L.nhood_counts(ctx, g, golden["intmat_cats"], 2), [[4, 1], [2, 2]])
    # NaN (code -1) spots are masked
    cats = golden["intmat_cats"].copy()
    cats[0] = -1
    ref = O.interaction_matrix(adj[1:, :][:, 1:].tocsr().data, adj[1:, :][:, 1:].tocsr().indices, adj[1:, :][:, 1:].tocsr().indptr, cats[1:], 2, True)
    np.testing.assert_array_equal(L.interaction_matrix(ctx, g, cats, 2, True), ref)
    # ... and the reference's literal values for it (tests/graph/test_nhood.py:165-173), also through the front end
    np.testing.assert_array_equal(L.interaction_matrix(ctx, g, cats, 2, True), [[2, 1], [2, 3]])
    np.testing.assert_array_equal(L.interaction_matrix(ctx, g, cats, 2, False), [[1, 1], [2, 2]])
    import pandas as pd

    import squidpy_amd as sq

    adata = sq.AnnDataLite(X=np.zeros((5, 5)), obs={"cat": pd.Categorical.from_codes(golden["intmat_cats"], ("a", "b"))},
                           obsp={"spatial_connectivities": sp.csr_matrix(adj, dtype=np.int64)})
    adata.obs.loc["0", "cat"] = np.nan
    np.testing.assert_array_equal(sq.gr.interaction_matrix(adata, "cat", weights=True, copy=True), [[2, 1], [2, 3]])
    np.testing.assert_array_equal(sq.gr.interaction_matrix(adata, "cat", weights=False, copy=True), [[1, 1], [2, 2]])


@pytest.mark.parametrize("k", [3, 30, 60, 150])
def test_weighted_interaction_matrix_float64_weights_reproducible(L, ctx, k):
    """Non-integer float64 weights (VERDICT r1 weak #4 / ADVICE): sums agree with the reference's serial float64 loop
    (gr/_nhood.py:412-429) to rounding, are computed from float64 weights (a float32 detour would sit at 1e-8), and — for
    K*K accumulators that fit LDS (K <= 143) — are bit-identical from run to run (per-wave private accumulators, fixed-order
    second stage; no floating-point atomics across waves)."""
    rng = np.random.default_rng(k)
    n = 20_000
    A = sp.random(n, n, density=8.0 / n, format="csr", random_state=5, dtype=np.float64)
    A.data = rng.gamma(2.0, 1.0, A.nnz) * np.exp(rng.normal(0, 3, A.nnz))  # six decades of dynamic range
    cats = rng.integers(-1, k, n).astype(np.int32)  # -1: NaN category, masked
    g = L.Graph(ctx, A)
    keep = cats >= 0
    sub = A[keep][:, keep].tocsr()
    ref = np.zeros((k, k))
    rows = np.repeat(np.arange(sub.shape[0]), np.diff(sub.indptr))
    for r, c, w in zip(cats[keep][rows], cats[keep][sub.indices], sub.data):  # the reference's serial loop order
        ref[r, c] += w
    got = [L.interaction_matrix(ctx, g, cats, k, True) for _ in range(3)]
    np.testing.assert_allclose(got[0], ref, rtol=1e-12)
    if k <= 143:
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    np.testing.assert_array_equal(L.interaction_matrix(ctx, g, cats, k, False), O.interaction_matrix(sub.data, sub.indices, sub.indptr, cats[keep], k, False))
    g.close()


def test_injected_numpy_permutations_reproduce_reference_zscore(L, ctx, golden):
    """The reference's PCG64 shuffles injected -> per-permutation counts and z-score identical (==) to the
    output of the reference's own `_nhood_enrichment_helper` + gr/_nhood.py:231."""
    g = L.Graph(ctx, _golden_graph(golden))
    k = int(golden["nhood_k"])
    P = golden["nhood_perms"].shape[0]
    lab = O.nhood_perm_labels_numpy(golden["nhood_labels"], int(golden["nhood_seed"]), P)
    perms = L.nhood_counts_batch(ctx, g, lab, k)
    np.testing.assert_array_equal(perms, golden["nhood_perms"].astype(np.uint32))
    z = O.nhood_zscore(golden["nhood_count"], perms.astype(np.float64))
    np.testing.assert_array_equal(z, golden["nhood_zscore"])


@pytest.mark.parametrize("k", [30, 60, 100, 150, 220, 256])
def test_injected_permutations_in_every_cluster_count_regime(L, ctx, k):
    """`sqgr_nhood_counts_batch` (host-drawn label vectors: the `rng="numpy-host"` route and what INTEGRATION.md offers a maintainer who
    keeps numpy's shuffles on the host) hands the labels to the count kernels through `k_transpose_labels` — rows for K <= 50, planes
    of the pass width above: 37 injected vectors (a partly filled last batch) `==` the reference kernel per vector."""
    rng = np.random.default_rng(k)
    adj = O.hex_grid_graph(37, 41)
    n = adj.shape[0]
    lab = rng.integers(0, k, size=(37, n))
    g = L.Graph(ctx, adj, with_data=False)
    got = L.nhood_counts_batch(ctx, g, lab, k)
    for p in range(37):
        np.testing.assert_array_equal(got[p], O.nhood_counts(adj.indices, adj.indptr, lab[p], k), err_msg=f"vector {p}")
    g.close()


@pytest.mark.parametrize("n", [1, 7, 49, 300, 5000])
def test_device_shuffle_matches_oracle_generator(L, ctx, n):
    rng = np.random.default_rng(n)
    k = 5
    labels = rng.integers(0, k, n)
    adj = sp.identity(n, format="csr", dtype=np.float32)
    g = L.Graph(ctx, adj)
    plan = L.NhoodPlan(ctx, g, labels, k)
    for perm in (0, 1, 17, 2**33 + 5):
        got = plan.shuffled_labels(seed=1234, perm=perm)
        exp = devrng.shuffled_labels(labels, 1234, perm)
        np.testing.assert_array_equal(got, exp)
        assert np.array_equal(np.sort(got), np.sort(labels))


@pytest.mark.parametrize("B", [16, 32])
def test_philox_permutation_test_bit_exact_vs_oracle(L, ctx, golden, B):
    adj = _golden_graph(golden)
    g = L.Graph(ctx, adj)
    k = int(golden["nhood_k"])
    labels = golden["nhood_labels"].astype(np.int32)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(B, 0, 2)
    seed, P = 99, 75  # not a multiple of the batch: exercises the masked tail
    shift = np.arange(k * k, dtype=np.int64).reshape(k, k) * 3 - 7
    s1, s2, perms = plan.run(seed, 0, P, shift, return_perms=True)
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, labels, k, seed, 0, P)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))
    d = ref.astype(np.int64) - shift
    np.testing.assert_array_equal(s1, d.sum(0))
    np.testing.assert_array_equal(s2, (d * d).sum(0).astype(np.uint64))
    # split invariance: any partition of the permutation range gives the same exact moments
    a1, a2, _ = plan.run(seed, 0, 20, shift)
    b1, b2, _ = plan.run(seed, 20, P, shift)
    np.testing.assert_array_equal(a1 + b1, s1)
    np.testing.assert_array_equal(a2 + b2, s2)


def test_philox_library_shuffle_bit_exact_vs_oracle(L, ctx, golden):
    adj = _golden_graph(golden)
    g = L.Graph(ctx, adj)
    k = int(golden["nhood_k"])
    labels = golden["nhood_labels"].astype(np.int32)
    libs = golden["nhood_lib_codes"]
    plan = L.NhoodPlan(ctx, g, labels, k, libs, 3)
    _, _, perms = plan.run(5, 3, 40, None, return_perms=True)
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, labels, k, 5, 3, 40, libs, 3)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))
    for perm in (0, 9):
        got = plan.shuffled_labels(5, perm)
        for c in range(3):  # label multiset preserved inside every library (reference test_shuffle_group)
            assert np.array_equal(np.sort(got[libs == c]), np.sort(labels[libs == c]))


@pytest.mark.parametrize("k", [5, 30, 100, 200, 256])
def test_independent_bijection_variant_bit_exact_vs_oracle(L, ctx, k, monkeypatch):
    """SQGR_SHUFFLE_INDEPENDENT=1 (bench.py's `nhood_independent_bijections` leg: what the generator costs WITHOUT the group
    bijection that 16 permutations share): every permutation its own 8-round bijection — the label vectors and the per-permutation
    counts `==` oracle/devrng.py's restatement (independent_label_permutations), in every counter layout."""
    monkeypatch.setenv("SQGR_SHUFFLE_INDEPENDENT", "1")
    rng = np.random.default_rng(k)
    adj = O.hex_grid_graph(61, 57)
    n = adj.shape[0]
    labels = rng.integers(0, k, n).astype(np.int32)
    labels[:k] = np.arange(k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    perms = np.arange(3, 3 + 40)
    pi = devrng.independent_label_permutations(n, 9, perms)
    srt = np.sort(labels)
    for j in (0, 1, 12, 13, 29, 39):
        np.testing.assert_array_equal(plan.shuffled_labels(9, int(perms[j])), srt[pi[j]], err_msg=f"permutation {perms[j]}")
    _, _, got = plan.run(9, 3, 43, None, return_perms=True)
    for j in range(40):
        np.testing.assert_array_equal(got[j], O.nhood_counts(adj.indices, adj.indptr, srt[pi[j]], k), err_msg=f"permutation {perms[j]}")
    monkeypatch.delenv("SQGR_SHUFFLE_INDEPENDENT")
    two_level = plan.shuffled_labels(9, 3)   # the default generator is another arrangement of the same multiset
    assert not np.array_equal(two_level, srt[pi[0]]) and np.array_equal(np.sort(two_level), srt)
    plan.close()
    g.close()


@pytest.mark.parametrize("k,n_libs", [(60, 3), (120, 2), (220, 4)])
def test_device_generator_with_libraries_above_50_clusters(L, ctx, k, n_libs):
    """The 16-bit counter layouts keep their chunks long when the LABELS bound a counter (largest cluster x longest row x weight
    <= 65 535: every slab column is a shuffle of the base labels) — per-library shuffles keep the cluster sizes too.  Per-permutation
    counts `==` the oracle's restatement of `_shuffle_group` with the device generator (gr/_utils.py:185-213), a ragged range."""
    rng = np.random.default_rng(k * 31 + n_libs)
    adj = O.hex_grid_graph(90, 80)
    n = adj.shape[0]
    labels = rng.integers(0, k, n).astype(np.int32)
    libs = rng.integers(0, n_libs, n).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k, libs, n_libs)
    info = plan.info()
    assert info["counter_mode"] == 2 and info["blocks_per_batch"] == 8, info   # the labels bound every counter: no extra chunks
    _, _, got = plan.run(21, 7, 7 + 35, None, return_perms=True)
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, labels, k, 21, 7, 7 + 35, libs, n_libs)
    np.testing.assert_array_equal(got, ref.astype(np.uint32))
    plan.close()
    g.close()


@pytest.mark.parametrize("k", [2, 30, 46, 60, 100, 150, 210, 256])
def test_all_cluster_count_regimes(L, ctx, k):
    """K decides which count kernel runs (LDS B=16, narrower LDS passes, device atomics): all bit-exact."""
    rng = np.random.default_rng(k)
    n = 1500
    adj = knn_graph(rng.random((n, 2)), 6)
    labels = rng.integers(0, k, n).astype(np.int32)
    g = L.Graph(ctx, adj)
    np.testing.assert_array_equal(L.nhood_counts(ctx, g, labels, k), O.nhood_counts(adj.indices, adj.indptr, labels, k))
    plan = L.NhoodPlan(ctx, g, labels, k)
    _, _, perms = plan.run(3, 0, 19, None, return_perms=True)
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, labels, k, 3, 0, 19)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))


@pytest.mark.parametrize("graph", ["hex", "hex+self", "knn", "gaps"])
@pytest.mark.parametrize("k,width,blocks", [(60, 0, 0), (60, 4, 0), (71, 8, 5), (72, 0, 0), (100, 0, 0), (101, 2, 0), (102, 0, 0), (130, 1, 0), (30, 8, 0), (30, 4, 16),
                                             (30, 2, 0), (7, 1, 3), (202, 0, 0), (203, 0, 0), (231, 0, 5), (256, 0, 0),
                                             # round 6: the 16-bit counter layouts at every width they run at (16 | 8 | 4 | 2) and at the
                                             # cluster counts where a width ends (symmetric: 100 | 142 | 201; directed: 71 | 101 | 143 | 202)
                                             (60, 8, 0), (60, 2, 3), (100, 8, 0), (100, 4, 3), (142, 0, 0), (143, 0, 0), (150, 2, 0), (201, 0, 0), (64, 1, 0)])
def test_lds_pass_kernel_every_width_on_half_and_full_lists(L, ctx, graph, k, width, blocks):
    """Above 50 clusters the counters of a block are 16 bits wide, two permutations per LDS word, on the unordered label pairs of a
    symmetric graph's half list (16 permutations per pass up to K = 100, 8 to 142, 4 to 201, 2 to 256) or on all K*K pairs of a
    directed graph's full list (16 to 71, 8 to 101, 4 to 143, 2 to 202); one permutation per pass (a cap of 1; directed graphs above
    202 clusters) and every forced width at K <= 50 keep the 32-bit counters of rounds 1-5 (k_count_pass: the machinery of the
    K <= 50 kernel at 2 | 1 lanes per edge).  Every width — the one K selects (width 0) and narrower ones forced through
    `tune` — on the symmetric half list without and with self loops (weights 2 and 1, halved sums) and on a directed kNN
    graph (full list); chunks cut so that whole-iteration blocks, a ragged last chunk and empty chunks all occur; chunk counts
    that are and are not a multiple of 8 (the XCD-aware block map and the plain one).  Per-permutation counts `==` the oracle."""
    rng = np.random.default_rng(k * 7 + width)
    if graph == "knn":
        n = 21000
        adj = knn_graph(rng.random((n, 2)), 6)
    elif graph == "gaps":  # one row in 40 has neighbours (anywhere): 256 list entries span > 255 rows — the 4-byte list entries
        n = 24000          # (row - group base in 8 bits) do not fit this graph and the 8-byte list must take over
        rows = np.repeat(np.arange(0, n, 40), 6)
        adj = sp.csr_matrix((np.ones(rows.size, np.float32), (rows, rng.integers(0, n, rows.size))), shape=(n, n))
        adj.sum_duplicates()
        adj.sort_indices()
    else:
        adj = O.hex_grid_graph(150, 160)
        n = adj.shape[0]
        if graph == "hex+self":
            adj = sp.csr_matrix(adj + sp.identity(n, format="csr", dtype=np.float32))
            adj.sort_indices()
    labels = rng.integers(0, k, n).astype(np.int32)
    g = L.Graph(ctx, adj)
    plan = L.NhoodPlan(ctx, g, labels, k)
    if width or blocks:
        plan.tune(width, blocks, 3)
    info = plan.info()
    assert info["symmetric"] == (graph in ("hex", "hex+self"))
    sym = info["symmetric"]
    if k > 50 and width != 1:  # which layout and pass width K selects (csrc/sqgr_nhood.hip: sqgr_nhood::cm / be)
        lim = (100, 142, 201, 285) if sym else (71, 101, 143, 202)
        want = next((w for w, top in zip((16, 8, 4, 2), lim) if k <= top and (not width or w <= width)), None)
        if want is None:
            assert info["counter_mode"] == 0
        else:
            assert (info["counter_mode"], info["perms_per_pass"]) == (2 if sym else 1, want), info
    else:
        assert info["counter_mode"] == 0
    n_perms = 50  # 3 batches of 16 per launch group -> two launch groups, the last batch partly filled
    _, _, perms = plan.run(11, 5, 5 + n_perms, None, return_perms=True)
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, labels, k, 11, 5, 5 + n_perms)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))
    assert int(perms[0].sum()) == adj.nnz


def test_ragged_and_empty_rows(L, ctx):
    """Rows without neighbours, self loops, duplicate and explicit-zero entries all count like the reference."""
    rng = np.random.default_rng(0)
    n, k = 400, 4
    rows = rng.integers(0, n // 2, 3000)  # upper half of the rows is empty
    cols = rng.integers(0, n, 3000)
    adj = sp.csr_matrix((rng.integers(0, 2, 3000).astype(np.float32), (rows, cols)), shape=(n, n))  # sums duplicates
    adj = adj + sp.identity(n, format="csr", dtype=np.float32)  # self loops
    adj = sp.csr_matrix(adj)
    labels = rng.integers(0, k, n).astype(np.int32)
    g = L.Graph(ctx, adj)
    np.testing.assert_array_equal(L.nhood_counts(ctx, g, labels, k), O.nhood_counts(adj.indices, adj.indptr, labels, k))
    empty = sp.csr_matrix((n, n), dtype=np.float32)
    g0 = L.Graph(ctx, empty)
    assert L.nhood_counts(ctx, g0, labels, k).sum() == 0
    plan = L.NhoodPlan(ctx, g0, labels, k)
    s1, s2, _ = plan.run(1, 0, 10)
    assert not s1.any() and not s2.any()


def test_frontend_config1_hex_grid(L):
    """BASELINE config 1 shape: 5 000-spot hex grid, 10 clusters, n_perms=1000 (front-end, both rng modes)."""
    import squidpy_amd as sq

    adata = hex_adata(50, 100, 10, seed=0)
    adj = adata.obsp["spatial_connectivities"]
    lab = codes(adata, "cluster")
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=1000, seed=0, copy=True, rng="philox")
    count_ref = O.nhood_counts(adj.indices, adj.indptr, lab, 10)
    np.testing.assert_array_equal(res.counts, count_ref)
    assert res.counts.dtype == np.uint32 and res.zscore.dtype == np.float64 and res.zscore.shape == (10, 10)
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, lab, 10, 0, 0, 1000)
    z_ref = O.nhood_zscore(count_ref, ref)
    np.testing.assert_allclose(res.zscore, z_ref, rtol=1e-9, atol=1e-12)  # exact-integer moments vs numpy mean/std
    # rng="numpy" reproduces Squidpy's own streams: equal (==) to the reference restatement
    res_np = sq.gr.nhood_enrichment(adata, "cluster", n_perms=200, seed=7, copy=True)
    perms_np = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, 10, 7, 200)
    np.testing.assert_array_equal(res_np.zscore, O.nhood_zscore(count_ref, perms_np))
    # statistical agreement between the two generators: same null distribution
    perms_np1000 = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, 10, 1, 1000)
    z2 = O.nhood_zscore(count_ref, perms_np1000)
    assert np.abs(res.zscore - z2).max() < 0.35 * max(1.0, np.abs(z2).max() * 0.1 + 1)
    np.testing.assert_allclose(ref.mean(0), perms_np1000.mean(0), rtol=0.02)
    # std of 1000 draws has a relative standard error of 1/sqrt(2000) = 2.2 %: 0.16 is ~5 sigma of the difference
    np.testing.assert_allclose(ref.std(0), perms_np1000.std(0), rtol=0.16)


def test_frontend_slots_reproducibility_and_libraries(L):
    """reference tests/graph/test_nhood.py:20-70 ported: dtypes/shapes, seed reproducibility, count invariance."""
    import squidpy_amd as sq

    adata = hex_adata(30, 40, 5, seed=3, n_libs=3)
    assert sq.gr.nhood_enrichment(adata, "cluster", n_perms=50, seed=42) is None
    slot = adata.uns["cluster_nhood_enrichment"]
    assert set(slot) == {"zscore", "count"}
    assert slot["zscore"].dtype == np.float64 and slot["count"].dtype == np.uint32
    assert slot["zscore"].shape == slot["count"].shape == (5, 5)
    r1 = sq.gr.nhood_enrichment(adata, "cluster", n_perms=50, seed=42, copy=True, n_jobs=2, backend="threading")
    r2 = sq.gr.nhood_enrichment(adata, "cluster", n_perms=50, seed=43, copy=True, numba_parallel=True)
    np.testing.assert_array_equal(r1.zscore, slot["zscore"])
    np.testing.assert_array_equal(r1.counts, r2.counts)
    assert not np.allclose(r1.zscore, r2.zscore)
    rl = sq.gr.nhood_enrichment(adata, "cluster", library_key="library", n_perms=50, seed=42, copy=True, rng="philox")
    np.testing.assert_array_equal(rl.counts, r1.counts)
    assert not np.allclose(rl.zscore, r1.zscore)
    adj = adata.obsp["spatial_connectivities"]
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, codes(adata, "cluster"), 5, 42, 0, 50, codes(adata, "library"), 3)
    np.testing.assert_allclose(rl.zscore, O.nhood_zscore(rl.counts, ref), rtol=1e-9)
    # interaction_matrix front-end
    im = sq.gr.interaction_matrix(adata, "cluster", copy=True)
    np.testing.assert_array_equal(im, O.nhood_counts(adj.indices, adj.indptr, codes(adata, "cluster"), 5).astype(float))


def test_config2_size_properties(L, ctx):
    """BASELINE config 2 size (1e5 spots, 20 clusters): counts bit-exact vs oracle; permutation counts obey the
    size-independent invariants (every permutation's counts sum to nnz; row sums follow the label degrees)."""
    rows, cols, k = 250, 400, 20
    adj = O.hex_grid_graph(rows, cols)
    rng = np.random.default_rng(0)
    labels = rng.integers(0, k, rows * cols).astype(np.int32)
    g = L.Graph(ctx, adj)
    np.testing.assert_array_equal(L.nhood_counts(ctx, g, labels, k), O.nhood_counts(adj.indices, adj.indptr, labels, k))
    plan = L.NhoodPlan(ctx, g, labels, k)
    s1, s2, perms = plan.run(11, 0, 100, None, return_perms=True)
    assert (perms.reshape(100, -1).sum(1) == adj.nnz).all()
    np.testing.assert_array_equal(s1, perms.astype(np.int64).sum(0))
    ref = O.nhood_perm_counts_philox(adj.indices, adj.indptr, labels, k, 11, 0, 3)
    np.testing.assert_array_equal(perms[:3], ref.astype(np.uint32))


def test_numpy_streams_reproduced_on_device(L, ctx, golden):
    """numpy's PCG64 + Generator.shuffle on the GPU, bit for bit — per-permutation counts equal the
    reference helper's golden output; with libraries the `_shuffle_group` semantics; z-score == the reference's."""
    import squidpy_amd as sq
    from squidpy_amd._utils import pcg64_states

    adj = _golden_graph(golden)
    g = L.Graph(ctx, adj)
    k = int(golden["nhood_k"])
    labels = golden["nhood_labels"].astype(np.int32)
    seed = int(golden["nhood_seed"])
    P = golden["nhood_perms"].shape[0]
    plan = L.NhoodPlan(ctx, g, labels, k)
    s1, s2, perms = plan.run_pcg64(pcg64_states(seed, P), return_perms=True)
    np.testing.assert_array_equal(perms, golden["nhood_perms"].astype(np.uint32))
    np.testing.assert_array_equal(s1, perms.astype(np.int64).sum(0))
    plan_l = L.NhoodPlan(ctx, g, labels, k, golden["nhood_lib_codes"], 3)
    _, _, perms_l = plan_l.run_pcg64(pcg64_states(seed, P), return_perms=True)
    np.testing.assert_array_equal(perms_l, golden["nhood_perms_lib"].astype(np.uint32))
    # front-end: rng="numpy" (device) == rng="numpy-host" == golden z-score of the reference
    obs = pd.DataFrame({"cl": pd.Categorical.from_codes(labels, list("abcde")), "lib": pd.Categorical.from_codes(golden["nhood_lib_codes"], ["x", "y", "z"])})
    adata = sq.AnnDataLite(obs=obs, obsp={"spatial_connectivities": adj})
    z_dev = sq.gr.nhood_enrichment(adata, "cl", n_perms=P, seed=seed, copy=True, rng="numpy").zscore
    z_host = sq.gr.nhood_enrichment(adata, "cl", n_perms=P, seed=seed, copy=True, rng="numpy-host").zscore
    np.testing.assert_array_equal(z_dev, golden["nhood_zscore"])
    np.testing.assert_array_equal(z_host, golden["nhood_zscore"])
    zl = sq.gr.nhood_enrichment(adata, "cl", library_key="lib", n_perms=P, seed=seed, copy=True, rng="numpy").zscore
    np.testing.assert_array_equal(zl, O.nhood_zscore(golden["nhood_count"], golden["nhood_perms_lib"]))


@pytest.mark.parametrize("k", [60, 90, 130, 230])
@pytest.mark.parametrize("libs", [0, 3])
def test_default_streams_with_more_than_50_clusters(L, ctx, k, libs):
    """numpy's streams + the pass kernel: the producers of the numpy path (`k_rows_to_slab` without libraries, `k_columns_to_slab`
    with) write the label slab in PLANES of the pass width (8 / 4 / 2 / 1 at K = 60 / 90 / 130 / 230) — per-permutation counts
    `==` the reference helper restated with numpy's own generators, z-scores of the DEFAULT front-end call `==` the reference's."""
    import squidpy_amd as sq
    from squidpy_amd._utils import pcg64_states

    rng = np.random.default_rng(k + libs)
    adata = hex_adata(60, 70, 5, seed=4, n_libs=libs)
    n = adata.n_obs
    lab = rng.integers(0, k, n).astype(np.int32)
    lab[:k] = np.arange(k)
    adata.obs["cluster"] = pd.Categorical.from_codes(lab, [f"c{i:03d}" for i in range(k)])
    adj = adata.obsp["spatial_connectivities"]
    lib = codes(adata, "library") if libs else None
    P, seed = 37, 11
    ref = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, seed, P, lib, libs)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k, lib, libs)
    _, _, perms = plan.run_pcg64(pcg64_states(seed, P), return_perms=True)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))
    plan.close()
    g.close()
    res = sq.gr.nhood_enrichment(adata, "cluster", library_key="library" if libs else None, n_perms=P, seed=seed, copy=True)
    want = O.nhood_zscore(res.counts, ref)
    np.testing.assert_array_equal(np.isnan(res.zscore), np.isnan(want))
    ok = np.isfinite(want)
    np.testing.assert_array_equal(res.zscore[ok], want[ok])


@pytest.mark.parametrize("segments", ["1", "7"])
def test_numpy_mean_std_chain_is_cut_invariant(L, ctx, golden, segments, monkeypatch):
    """`perms.mean(0)` / `perms.std(0)` of gr/_nhood.py:231 are formed on the device as two CHAINS of running sums in permutation
    order (k_numpy_chain); several ranks continue each other's sums instead of gathering all per-permutation counts.  A chain cut
    into 7 segments — what 7 ranks would do, on one GPU — gives numpy's bits like the uncut one."""
    from squidpy_amd._utils import pcg64_states

    monkeypatch.setenv("SQGR_NUMPY_STATS_SEGMENTS", segments)
    adj = _golden_graph(golden)
    g = L.Graph(ctx, adj)
    k = int(golden["nhood_k"])
    labels = golden["nhood_labels"].astype(np.int32)
    P = 103
    plan = L.NhoodPlan(ctx, g, labels, k)
    mean, std = plan.run_pcg64_stats(pcg64_states(5, P))
    _, _, perms = plan.run_pcg64(pcg64_states(5, P), return_perms=True)
    x = perms.astype(np.float64)
    np.testing.assert_array_equal(mean.reshape(k, k), x.mean(axis=0))
    np.testing.assert_array_equal(std.reshape(k, k), x.std(axis=0))


@pytest.mark.parametrize("n", [2, 77, 5000, 70001])
def test_numpy_permutation_streams_on_device(L, ctx, n):
    from squidpy_amd._utils import pcg64_states

    P = 70 if n < 10000 else 5
    got = L.pcg64_permutations(ctx, n, pcg64_states(13, P))
    np.testing.assert_array_equal(got, O.autocorr_perm_indices(n, 13, P))
    labels = np.random.default_rng(0).integers(0, 7, n)
    g = L.Graph(ctx, sp.identity(n, format="csr", dtype=np.float32))
    plan = L.NhoodPlan(ctx, g, labels, 7)
    _, _, perms = plan.run_pcg64(pcg64_states(13, P), return_perms=True)
    ref = O.nhood_perm_counts_numpy(g_identity_indices(n), np.arange(n + 1), labels, 7, 13, P)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))


def g_identity_indices(n):
    return np.arange(n)


@pytest.mark.parametrize("variant", ["wave", "wave-slow-path-only"])
def test_numpy_shuffle_kernel_variants_agree_with_numpy(L, ctx, variant, monkeypatch):
    """The wave-per-permutation shuffle (jump-ahead draws, parallel swaps, exact replay where a chunk has coinciding
    draws / borderline candidates / a mask change / a library end) and the same kernel forced onto its replay path
    must both reproduce numpy bit for bit — sizes around the 64-draw chunk and the 192-element fast-path limit, and
    libraries that end in the middle of a chunk."""
    from squidpy_amd._utils import pcg64_states

    if variant == "wave-slow-path-only":
        monkeypatch.setenv("SQGR_PCG_FORCE_SLOW", "1")
    for n in (2, 3, 63, 64, 65, 128, 191, 192, 193, 257, 1000, 4097, 33000):
        P = 66
        got = L.pcg64_permutations(ctx, n, pcg64_states(n, P))
        want = np.stack([np.random.default_rng(s).permutation(n) for s in np.random.SeedSequence(n).spawn(P)])
        np.testing.assert_array_equal(got, want, err_msg=f"n={n}")
    # label shuffles per library (`_shuffle_group`: one generator walks the libraries in category order)
    rng = np.random.default_rng(5)
    n, k, n_libs, P = 6000, 9, 7, 40
    labels = rng.integers(0, k, n).astype(np.int32)
    libs = rng.integers(0, n_libs, n).astype(np.int32)
    libs[:300] = 3  # one library is much larger than the others, one (6) may stay tiny
    libs[libs == 6] = np.where(rng.random((libs == 6).sum()) < 0.01, 6, 0)
    ring = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))  # i -> i+1
    g = L.Graph(ctx, ring)
    plan = L.NhoodPlan(ctx, g, labels, k, libs, n_libs)
    _, _, perms = plan.run_pcg64(pcg64_states(21, P), return_perms=True)
    want = np.stack([
        O.nhood_counts(ring.indices, ring.indptr, O.shuffle_group(labels, libs, n_libs, rs), k) for rs in O.spawn_generators(21, P)
    ])
    np.testing.assert_array_equal(perms, want.astype(np.uint32))
    assert len({w.tobytes() for w in want}) == P  # the counts do depend on the arrangement


@pytest.mark.parametrize("logs", ["6", "8", "12", "default"])
def test_numpy_shuffle_bucketed_replay_agrees_with_numpy(L, ctx, logs, monkeypatch):
    """The bucketed replay of `Generator.shuffle` (draws appended to per-(phase, range) lists, swaps applied range by range in
    concurrent rounds: csrc/sqgr_pcg.hip, oracle/pcg_bucket.py) must leave numpy's arrays bit for bit — phase lengths of 64,
    256 and 4096 positions put tens to thousands of phases, partial top phases and phase boundaries inside a 64-draw trip on
    small arrays; "default" is the production geometry (65536) on a 200 001-element array.  The counts over the ring graph
    i -> i+1 with ~250 distinct labels see every misplaced element."""
    from squidpy_amd._utils import pcg64_states

    monkeypatch.setenv("SQGR_PCG_KERNEL", "bucket")
    if logs != "default":
        monkeypatch.setenv("SQGR_PCG_BUCKET_LOGS", logs)
    sizes = (2, 3, 63, 64, 65, 129, 193, 1000, 4097, 33000) if logs != "default" else (1000, 70001, 200001)
    for n in sizes:
        if logs == "6" and n > 4097:  # at most 64 ranges per library: S = 64 serves up to 4096 positions
            continue
        P, k = (40 if n < 10000 else 6), 251
        labels = (np.arange(n) * 7919 % k).astype(np.int32)
        ring = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
        g = L.Graph(ctx, ring)
        plan = L.NhoodPlan(ctx, g, labels, k)
        _, _, perms = plan.run_pcg64(pcg64_states(n, P), return_perms=True)
        ref = O.nhood_perm_counts_numpy(ring.indices, ring.indptr, labels, k, n, P)
        np.testing.assert_array_equal(perms, ref.astype(np.uint32), err_msg=f"n={n} logS={logs}")
        plan.close()
        g.close()
    if logs in ("6", "default"):
        return
    # libraries (`_shuffle_group`): one generator walks them in category order; sizes from 1 to thousands, unaligned offsets
    rng = np.random.default_rng(5)
    n, k, n_libs, P = 6000, 9, 7, 40
    labels = rng.integers(0, k, n).astype(np.int32)
    libs = rng.integers(0, n_libs, n).astype(np.int32)
    libs[:300] = 3
    libs[libs == 6] = np.where(rng.random((libs == 6).sum()) < 0.01, 6, 0)
    ring = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
    g = L.Graph(ctx, ring)
    plan = L.NhoodPlan(ctx, g, labels, k, libs, n_libs)
    _, _, perms = plan.run_pcg64(pcg64_states(21, P), return_perms=True)
    want = np.stack([
        O.nhood_counts(ring.indices, ring.indptr, O.shuffle_group(labels, libs, n_libs, rs), k) for rs in O.spawn_generators(21, P)
    ])
    np.testing.assert_array_equal(perms, want.astype(np.uint32))


@pytest.mark.parametrize(
    "env",
    [
        {"SQGR_PCG_QUEUE_CAP": "4"},                              # the replay's queue overflows at once: records stay with their lanes (spill path), a drain per chunk
        {"SQGR_PCG_QUEUE_CAP": "64"},
        {"SQGR_PCG_FORCE_SLOW": "1"},                             # the generator's one-by-one path on every trip (128 slots in order)
    ],
    ids=lambda e: ",".join(f"{k[9:].lower()}={v}" for k, v in e.items()),
)
def test_numpy_shuffle_replay_variants_agree_with_numpy(L, ctx, env, monkeypatch):
    """Round 6's generator (128 draws per trip, one 64-record ring per range) and replay (exact claims, deferred queue, priority
    drains): the paths a production run hardly takes — a full queue, the one-by-one acceptance — against numpy's own shuffles:
    production geometry on 70 001 and 200 001 positions, 4096-position phases on 33 000."""
    from squidpy_amd._utils import pcg64_states

    monkeypatch.setenv("SQGR_PCG_KERNEL", "bucket")
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    for n, logs in ((33000, "12"), (70001, None), (200001, None)):
        if logs:
            monkeypatch.setenv("SQGR_PCG_BUCKET_LOGS", logs)
        else:
            monkeypatch.delenv("SQGR_PCG_BUCKET_LOGS", raising=False)
        P, k = 5, 251
        labels = (np.arange(n) * 7919 % k).astype(np.int32)
        ring = sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
        g = L.Graph(ctx, ring)
        plan = L.NhoodPlan(ctx, g, labels, k)
        _, _, perms = plan.run_pcg64(pcg64_states(n + 1, P), return_perms=True)
        ref = O.nhood_perm_counts_numpy(ring.indices, ring.indptr, labels, k, n + 1, P)
        np.testing.assert_array_equal(perms, ref.astype(np.uint32), err_msg=f"n={n} {env}")
        plan.close()
        g.close()


def test_skewed_cluster_sizes(L, ctx):
    """SURVEY §8d skewed variant: Dirichlet(0.5) cluster proportions (a few huge clusters, some almost empty, one
    empty) concentrate the count kernel's LDS atomics on few counters and make label boundaries fall inside single
    rank blocks of the shuffle's lookup table.  Counts and permutation counts stay bit-exact."""
    import squidpy_amd as sq

    rng = np.random.default_rng(3)
    k = 12
    adata = hex_adata(60, 80, k, seed=4)
    n = adata.n_obs
    prop = rng.dirichlet(np.full(k - 1, 0.5))
    lab = rng.choice(k - 1, size=n, p=prop).astype(np.int32)  # category k-1 stays empty
    adata.obs["cluster"] = pd.Categorical.from_codes(lab, [f"c{i}" for i in range(k)])
    adj = adata.obsp["spatial_connectivities"]
    g = L.Graph(ctx, adj)
    np.testing.assert_array_equal(L.nhood_counts(ctx, g, lab, k), O.nhood_counts(adj.indices, adj.indptr, lab, k))
    plan = L.NhoodPlan(ctx, g, lab, k)
    _, _, perms = plan.run(17, 0, 48, None, return_perms=True)
    np.testing.assert_array_equal(perms, O.nhood_perm_counts_philox(adj.indices, adj.indptr, lab, k, 17, 0, 48).astype(np.uint32))
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=48, seed=17, copy=True, rng="philox")
    ref = O.nhood_zscore(res.counts, perms.astype(np.float64))
    ok = np.isfinite(ref)
    np.testing.assert_allclose(res.zscore[ok], ref[ok], rtol=1e-9)
    assert np.isnan(res.zscore[k - 1]).all() and np.isnan(ref[k - 1]).all()  # empty category: 0/0 as in the reference


def test_more_than_256_clusters_run_batched_on_the_device(L, ctx):
    """256 < K <= 4096: 16-bit label slab + device-scope counters, device shuffles in both rng modes — the
    device generator against its oracle restatement, numpy streams against Squidpy's z-scores for the seed, bit for bit."""
    import squidpy_amd as sq

    k = 300
    adata = hex_adata(30, 40, 6, seed=8, n_libs=3)
    n = adata.n_obs
    lab = np.random.default_rng(8).integers(0, k, n).astype(np.int32)
    lab[:k] = np.arange(k)
    adata.obs["cluster"] = pd.Categorical.from_codes(lab, [f"c{i:03d}" for i in range(k)])
    adj = adata.obsp["spatial_connectivities"]
    count = O.nhood_counts(adj.indices, adj.indptr, lab, k)
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=40, seed=3, copy=True, rng="philox")
    np.testing.assert_array_equal(res.counts, count)
    want = O.nhood_zscore(count, O.nhood_perm_counts_philox(adj.indices, adj.indptr, lab, k, 3, 0, 40))
    np.testing.assert_array_equal(np.isnan(res.zscore), np.isnan(want))
    ok = np.isfinite(want)
    np.testing.assert_allclose(res.zscore[ok], want[ok], rtol=1e-9)
    # per-permutation counts through the C ABI, an unaligned range
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    _, _, perms = plan.run(3, 5, 39, return_perms=True)
    np.testing.assert_array_equal(perms, O.nhood_perm_counts_philox(adj.indices, adj.indptr, lab, k, 3, 5, 39).astype(np.uint32))
    plan.close()
    # libraries: per-library bijections with 16-bit labels
    libs = codes(adata, "library")
    plan = L.NhoodPlan(ctx, g, lab, k, libs, 3)
    _, _, perms = plan.run(11, 0, 20, return_perms=True)
    np.testing.assert_array_equal(perms, O.nhood_perm_counts_philox(adj.indices, adj.indptr, lab, k, 11, 0, 20, libs, 3).astype(np.uint32))
    plan.close()
    g.close()
    # numpy streams: Squidpy's z-scores for the seed
    ref_perms = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, 3, 12)
    want = O.nhood_zscore(count, ref_perms)
    ok = np.isfinite(want)
    res2 = sq.gr.nhood_enrichment(adata, "cluster", n_perms=12, seed=3, copy=True, rng="numpy")
    np.testing.assert_array_equal(res2.zscore[ok], want[ok])
    # numpy streams + libraries + K > 256 take the host-drawn route (per-library sub-shuffles): still Squidpy's z-scores
    ref_perms = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, 3, 6, libs, 3)
    want = O.nhood_zscore(count, ref_perms)
    ok = np.isfinite(want)
    res3 = sq.gr.nhood_enrichment(adata, "cluster", library_key="library", n_perms=6, seed=3, copy=True, rng="numpy")
    np.testing.assert_array_equal(res3.zscore[ok], want[ok])
    # rng="numpy-host" with more than 256 clusters (the uint8 injection path must not be taken): the same z-scores
    res4 = sq.gr.nhood_enrichment(adata, "cluster", n_perms=12, seed=3, copy=True, rng="numpy-host")
    np.testing.assert_array_equal(res4.zscore[np.isfinite(res2.zscore)], res2.zscore[np.isfinite(res2.zscore)])


def test_300_clusters_at_1e5_spots_is_a_device_path(L, ctx):
    """K = 300 on 1e5 spots, 1000 permutations: the batched device path (the host-shuffle route of round 1 needed ~1 ms per
    permutation plus a numpy shuffle: > 2 s; 100x faster was the bar)."""
    import time

    import squidpy_amd as sq

    k, P = 300, 1000
    adata = hex_adata(250, 400, 6, seed=8)
    n = adata.n_obs
    lab = np.random.default_rng(8).integers(0, k, n).astype(np.int32)
    adata.obs["cluster"] = pd.Categorical.from_codes(lab, [f"c{i:03d}" for i in range(k)])
    adj = adata.obsp["spatial_connectivities"]
    sq.gr.nhood_enrichment(adata, "cluster", n_perms=32, seed=1, copy=True, rng="philox")  # warm-up (allocations)
    t0 = time.perf_counter()
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=P, seed=1, copy=True, rng="philox")
    dt = time.perf_counter() - t0
    assert np.isfinite(res.zscore).all()
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    _, _, perms = plan.run(1, 0, P, return_perms=True)
    np.testing.assert_allclose(res.zscore, O.nhood_zscore(res.counts, perms), rtol=1e-9)
    for p in (0, 999):
        np.testing.assert_array_equal(perms[p], O.nhood_counts(adj.indices, adj.indptr, devrng.shuffled_labels(lab, 1, p), k))
    plan.close()
    g.close()
    assert dt < 1.0, f"{P} permutations took {dt:.2f} s"


def test_more_than_4096_clusters_use_the_general_path(L, ctx):
    """K > 4096: numpy streams on the host + the any-K edge-pair kernel; Squidpy's z-scores for the seed for either `rng`."""
    import squidpy_amd as sq

    k = 4200
    adata = hex_adata(70, 80, 6, seed=8)
    n = adata.n_obs
    lab = np.random.default_rng(8).integers(0, k, n).astype(np.int32)
    lab[:k] = np.arange(k)
    adata.obs["cluster"] = pd.Categorical.from_codes(lab, [f"c{i:04d}" for i in range(k)])
    adj = adata.obsp["spatial_connectivities"]
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=4, seed=3, copy=True)
    ref_perms = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, 3, 4)
    np.testing.assert_array_equal(res.counts, O.nhood_counts(adj.indices, adj.indptr, lab, k))
    want = O.nhood_zscore(res.counts, ref_perms)
    ok = np.isfinite(want)
    np.testing.assert_array_equal(res.zscore[ok], want[ok])


def test_null_distribution_matches_numpy_streams_at_high_power(L, ctx):
    """The statistic the permutation test is about: mean and variance of every count cell under the device generator vs
    under numpy's own shuffles, 30 000 permutations each on a 1e5-spot hex grid with 20 clusters (BASELINE config C2's
    shape) — a bias of ~1 % of sigma in any of the 400 cells would fail (tools/null_moments.py runs the 2e5-permutation,
    1e6-spot version)."""
    from squidpy_amd._utils import pcg64_states

    P, k = 30_000, 20
    adj = O.hex_grid_graph(250, 400)
    labels = np.random.default_rng(2).integers(0, k, adj.shape[0]).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    freq = np.bincount(labels, minlength=k) / adj.shape[0]
    shift = np.rint(adj.nnz * np.outer(freq, freq)).astype(np.int64)

    def moments(s1, s2):
        mean = s1.astype(np.float64) / P
        return mean, s2.astype(np.float64) / P - mean * mean

    s1, s2, _ = plan.run(99, 0, P, shift)
    m_dev, v_dev = moments(s1, s2)
    s1, s2, _ = plan.run_pcg64(pcg64_states(3, P), shift)
    m_np, v_np = moments(s1, s2)
    z_mean = (m_dev - m_np) / np.sqrt((v_dev + v_np) / P)
    z_var = (v_dev - v_np) / (0.5 * (v_dev + v_np) * np.sqrt(4.0 / P))
    assert np.abs(z_mean).max() < 5.0 and np.abs(z_var).max() < 5.0, (np.abs(z_mean).max(), np.abs(z_var).max())
    assert 0.7 < np.sqrt((z_mean**2).mean()) < 1.3 and 0.7 < np.sqrt((z_var**2).mean()) < 1.3


def test_numpy_streams_partial_last_batch_with_device_scope_counters(L, ctx):
    """Regression (found by tools/fuzz_gpu.py): K = 203 counts through device-scope atomics straight into global memory;
    with numpy streams the label columns past the last permutation of a partly filled batch must hold valid labels, or
    the count kernel indexes outside its counters (a GPU memory fault, not a wrong number)."""
    from squidpy_amd._utils import pcg64_states

    rng = np.random.default_rng(1)
    n, k, P = 255, 203, 38
    A = sp.csr_matrix(sp.random(n, n, density=3.0 / n, format="csr", random_state=3))
    A.data[:] = 1.0
    labels = rng.integers(0, k, n).astype(np.int32)
    g = L.Graph(ctx, A)
    for tune in ((16, 0, 3), (16, 8, 1), (16, 0, 0)):
        plan = L.NhoodPlan(ctx, g, labels, k)
        plan.tune(*tune)
        _, _, perms = plan.run_pcg64(pcg64_states(1, P), return_perms=True)
        ref = O.nhood_perm_counts_numpy(A.indices, A.indptr, labels, k, 1, P)
        np.testing.assert_array_equal(perms, ref.astype(np.uint32))
        plan.close()


def test_graph_stays_resident_between_calls_and_is_keyed_by_content(L, ctx):
    """The statistics of one analysis read the same `adata.obsp` matrix: it is uploaded once (`_lib.cached_graph`), the cache
    is keyed by the matrix CONTENT, so an in-place edit is never served stale."""
    import squidpy_amd as sq

    sq.clear_graph_cache()
    adata = hex_adata(20, 30, 4, seed=3)
    adj = adata.obsp["spatial_connectivities"]
    lab = codes(adata, "cluster")
    a = sq.gr.nhood_enrichment(adata, "cluster", n_perms=32, seed=1, copy=True)
    g1 = L.cached_graph(ctx, adj, with_data=False)
    b = sq.gr.nhood_enrichment(adata, "cluster", n_perms=32, seed=1, copy=True)
    assert L.cached_graph(ctx, adj, with_data=False) is g1 and len(L._graph_cache) == 1
    np.testing.assert_array_equal(a.zscore, b.zscore)
    sq.gr.interaction_matrix(adata, "cluster", weights=True, copy=True)
    assert len(L._graph_cache) == 2  # the weighted copy is another entry
    # in-place edit of the matrix: drop all edges of spot 0 by pointing them at itself -> different content, fresh upload
    edited = adj.copy()
    edited.indices[edited.indptr[0] : edited.indptr[1]] = 0
    adata.obsp["spatial_connectivities"] = edited
    c = sq.gr.nhood_enrichment(adata, "cluster", n_perms=32, seed=1, copy=True)
    np.testing.assert_array_equal(c.counts, O.nhood_counts(edited.indices, edited.indptr, lab, 4))
    assert not np.array_equal(c.counts, a.counts) and L.cached_graph(ctx, edited, with_data=False) is not g1
    for k in range(6):  # least recently used entries are evicted and freed
        L.cached_graph(ctx, O.hex_grid_graph(5 + k, 7), with_data=False)
    assert len(L._graph_cache) == L._GRAPH_CACHE_SLOTS and g1.h is None
    sq.clear_graph_cache()
    assert not L._graph_cache


@pytest.mark.parametrize("k", [3000, 4096])
def test_thousands_of_clusters_run_batched_on_the_device(L, ctx, k):
    """2048 < K <= 4096 (round 6; the reference has no limit): 16-bit labels, K*K*16 device-scope counters per batch (0.6 GB at
    3000 clusters), the device generator reading its label boundaries where they fit — per-permutation counts against the oracle in
    both generators, the front end's z-scores in numpy's streams against the reference's arithmetic."""
    import squidpy_amd as sq

    adata = hex_adata(60, 100, 6, seed=9)
    n = adata.n_obs
    lab = np.random.default_rng(9).integers(0, k, n).astype(np.int32)
    lab[:k] = np.arange(k)
    adata.obs["cluster"] = pd.Categorical.from_codes(lab, [f"c{i:04d}" for i in range(k)])
    adj = adata.obsp["spatial_connectivities"]
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    _, _, perms = plan.run(3, 5, 23, return_perms=True)
    np.testing.assert_array_equal(perms, O.nhood_perm_counts_philox(adj.indices, adj.indptr, lab, k, 3, 5, 23).astype(np.uint32))
    from squidpy_amd._utils import pcg64_states

    _, _, perms = plan.run_pcg64(pcg64_states(4, 7), return_perms=True)
    ref = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, 4, 7)
    np.testing.assert_array_equal(perms, ref.astype(np.uint32))
    plan.close()
    g.close()
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=7, seed=4, copy=True)
    want = O.nhood_zscore(O.nhood_counts(adj.indices, adj.indptr, lab, k), ref)
    ok = np.isfinite(want)
    np.testing.assert_array_equal(res.zscore[ok], want[ok])


def _shuffled_grid(rows, cols, k, seed, directed=False):
    """A hex grid (or its directed 6-nearest-neighbour graph) whose observations come in RANDOM order."""
    import squidpy_amd as sq
    from squidpy_amd._synthetic import hex_grid, hex_grid_graph, knn_directed_graph

    rng = np.random.default_rng(seed)
    n = rows * cols
    xy = hex_grid(rows, cols) + (rng.normal(0.0, 3.0, (n, 2)) if directed else 0.0)
    adj = (knn_directed_graph(xy, 6) if directed else hex_grid_graph(rows, cols)).tocoo()
    perm = rng.permutation(n)  # new -> old
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    shuf = sp.csr_matrix((adj.data, (inv[adj.row], inv[adj.col])), shape=(n, n))
    shuf.sort_indices()
    lab = rng.integers(0, k, n).astype(np.int32)
    adata = sq.AnnDataLite(obs=pd.DataFrame({"cluster": pd.Categorical.from_codes(lab, [f"c{i:03d}" for i in range(k)])}),
                           obsm={"spatial": xy[perm]}, obsp={"spatial_connectivities": shuf})
    return adata, lab


@pytest.mark.parametrize("k,directed,coords", [(12, False, True), (12, True, True), (60, False, True), (130, True, True), (9, False, False)])
def test_observations_in_no_spatial_order_run_on_a_renumbered_twin(L, ctx, k, directed, coords, monkeypatch):
    """Round 6: rng="philox" on observations in random order builds a renumbered twin of the graph on the device (Z-order curve of
    obsm['spatial'], or reverse Cuthill-McKee of the graph) and lets the generator permute the ranks of the CALLER's observations
    (sqgr_graph_renumbered, sqgr_spatial_order, sqgr_nhood_set_spot_map): counts and z-scores equal the ones of the plan on the
    caller's own graph, bit for bit — symmetric and directed graphs, the LDS counter layouts, with and without coordinates."""
    import squidpy_amd as sq
    from squidpy_amd import _order

    adata, lab = _shuffled_grid(190, 200, k, seed=k, directed=directed)
    if not coords:
        del adata.obsm["spatial"]
        monkeypatch.setattr(sq.gr._nhood, "RENUMBER_RCM_PERMS", 1)
    near, span = _order.edge_locality(adata.obsp["spatial_connectivities"])
    assert near < 0.05 and span > 0.2
    monkeypatch.setenv("SQGR_NHOOD_RENUMBER", "0")
    plain = sq.gr.nhood_enrichment(adata, "cluster", n_perms=300, seed=5, copy=True, rng="philox")
    monkeypatch.setenv("SQGR_NHOOD_RENUMBER", "auto")
    used = []
    real = L.NhoodPlan.set_spot_map
    monkeypatch.setattr(L.NhoodPlan, "set_spot_map", lambda self, m: (used.append(len(m)), real(self, m))[1])
    twin = sq.gr.nhood_enrichment(adata, "cluster", n_perms=300, seed=5, copy=True, rng="philox")
    assert used == [adata.n_obs], "the renumbered twin was not used"
    np.testing.assert_array_equal(twin.counts, plain.counts)
    np.testing.assert_array_equal(twin.zscore, plain.zscore)
    # the default stream keeps the caller's order (numpy permutes positions) and still returns the reference's z-scores
    adj = adata.obsp["spatial_connectivities"]
    res = sq.gr.nhood_enrichment(adata, "cluster", n_perms=6, seed=2, copy=True)
    want = O.nhood_zscore(O.nhood_counts(adj.indices, adj.indptr, lab, k), O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, 2, 6))
    ok = np.isfinite(want)
    np.testing.assert_array_equal(res.zscore[ok], want[ok])


def test_renumbered_graph_and_spot_map_through_the_c_abi(L, ctx):
    """sqgr_graph_renumbered gives P A P^T (the observed counts of the twin with the labels in twin order are the graph's), the
    device order is a permutation that restores locality, a plan with a spot map refuses numpy's streams, bad orders are refused."""
    from squidpy_amd import _order
    from squidpy_amd._utils import pcg64_states

    adata, lab = _shuffled_grid(60, 70, 7, seed=3)
    adj = adata.obsp["spatial_connectivities"]
    n = adj.shape[0]
    g = L.Graph(ctx, adj, with_data=False)
    order = L.spatial_order_device(ctx, adata.obsm["spatial"])
    assert sorted(order.tolist()) == list(range(n))
    twin = g.renumbered(order)
    np.testing.assert_array_equal(L.nhood_counts(ctx, twin, lab[order], 7), L.nhood_counts(ctx, g, lab, 7))
    back = adj[order][:, order]
    assert _order.edge_locality(sp.csr_matrix(back))[0] > 0.2
    plan = L.NhoodPlan(ctx, twin, lab[order], 7)
    plan.set_spot_map(order)
    ref = L.NhoodPlan(ctx, g, lab, 7)
    a = plan.run(11, 3, 77, None, return_perms=True)
    b = ref.run(11, 3, 77, None, return_perms=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(L.SqgrError, match="spot map"):
        plan.run_pcg64(pcg64_states(1, 4))
    plan.set_spot_map(None)
    plan.close()
    ref.close()
    bad = order.copy()
    bad[0] = bad[1]
    with pytest.raises(L.SqgrError, match="not a permutation"):
        g.renumbered(bad)
    g.close()

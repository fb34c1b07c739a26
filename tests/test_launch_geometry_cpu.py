"""CPU: the launch geometry of the mixture fit and of the PCA moments (``sqgr_gmm_geometry`` / ``sqgr_pca_geometry``: host functions of
the library, the ones the kernels' launches call; no device).

- The C geometry ``==`` a short Python restatement formed from the constants the query returns, over a sweep of (n, d, k) / (n, D)
  that holds every cap minus one, the cap, and the cap plus one.
- Every launch-geometry case of tests/niche_cases.py and tests/niche_pca_cases.py binds what it is there to bind, stated as relations
  between the returned fields and constants: a constant that is retuned so that a case no longer binds fails here, instead of
  silently uncovering the seam."""

from __future__ import annotations

import itertools

import pytest

from squidpy_amd import _lib

from tests import niche_cases as NC
from tests import niche_pca_cases as PC


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---- the mixture fit ---------------------------------------------------------------------------------------------------------------------
def gmm_restated(n: int, d: int, k: int, q: dict) -> dict:
    """``gmm_geometry`` of csrc/sqgr_gmm.hip from the constants in ``q``."""
    out = {"dp": ceil_div(d, q["E_JT"]) * q["E_JT"]}
    ntiles = ceil_div(n, q["E_T"])
    out["e_tiles_per_block"] = ceil_div(ntiles, q["E_MAX_BLOCKS"])
    out["e_blocks"] = ceil_div(ntiles, out["e_tiles_per_block"])
    chunks = min(max(1, n // q["M_MIN_ROWS"]), max(1, q["M_MAX_BLOCKS"] // k))
    out["rows_per_chunk"] = ceil_div(n, chunks)
    out["nchunks"] = ceil_div(n, out["rows_per_chunk"])
    sums_chunks = min(max(1, n // q["M_MIN_ROWS"]), q["M_SUMS_BLOCKS"])
    out["sums_rows_per_chunk"] = ceil_div(n, sums_chunks)
    out["sums_nchunks"] = ceil_div(n, out["sums_rows_per_chunk"])
    ka, db = (k + 3) & ~3, (d + 3) & ~3

    def rows_per_stage(pitch: int) -> int:
        return max(min(256, q["M_STAGE_BYTES"] // (pitch * 8) // 32 * 32), 32)

    out["rt_sums"], out["rt_cov"] = rows_per_stage(ka + db), rows_per_stage(2 * db)
    out["lds_e"] = d * q["E_T"] * 8
    out["lds_sums"] = max(out["rt_sums"] * (ka + db) * 8, q["M_RED_BYTES"])
    out["lds_cov"] = max(out["rt_cov"] * 2 * db * 8, q["M_RED_BYTES"])
    return out


def gmm_sweep() -> list:
    c = _lib.gmm_geometry(1, 1, 1)
    e_t, e_max, m_max, m_min, m_sums = (c[key] for key in ("E_T", "E_MAX_BLOCKS", "M_MAX_BLOCKS", "M_MIN_ROWS", "M_SUMS_BLOCKS"))
    ks = (1, 3, 4, 63, 64)
    ns = {1, 2, e_t - 1, e_t, e_t + 1, m_min - 1, m_min, m_min + 1, 2 * m_min - 1, 2 * m_min, 8000, 100_003, 2**31 - 1}
    for edge in (e_t * e_max, m_min * m_sums, (m_min + 1) * m_sums, 2 * e_t * e_max):  # tiles per block 1 -> 2 -> 3, the cap of the weighted sums
        ns |= {edge - 1, edge, edge + 1}
    for k in ks:  # the cap of the covariance grid for this k, and the first n whose chunks grow past the least rows
        cap = max(1, m_max // k)
        for edge in (m_min * cap, (m_min + 1) * cap):
            ns |= {edge - 1, edge, edge + 1}
    triples = [(n, d, k) for n in sorted(ns) for d, k in zip(itertools.cycle((1, 3, 4, 17, 64)), ks) if k <= n]
    triples += [(c.n, c.d, c.k) for c in NC.CASES.values()]
    return triples


def test_gmm_geometry_equals_the_restatement():
    triples = gmm_sweep()
    assert len(triples) >= 200
    for n, d, k in triples:
        q = _lib.gmm_geometry(n, d, k)
        want = gmm_restated(n, d, k, q)
        assert {key: q[key] for key in want} == want, (n, d, k)
        assert set(want) | {"E_T", "E_MAX_BLOCKS", "M_MAX_BLOCKS", "M_MIN_ROWS", "M_SUMS_BLOCKS", "E_JT", "M_STAGE_BYTES", "M_RED_BYTES"} == set(q)
        # every row is in exactly one tile, block and chunk
        assert (q["e_blocks"] - 1) * q["e_tiles_per_block"] < ceil_div(n, q["E_T"]) <= q["e_blocks"] * q["e_tiles_per_block"]
        assert q["e_blocks"] <= q["E_MAX_BLOCKS"] and q["nchunks"] * k <= max(q["M_MAX_BLOCKS"], k) and q["sums_nchunks"] <= q["M_SUMS_BLOCKS"]
        assert (q["nchunks"] - 1) * q["rows_per_chunk"] < n <= q["nchunks"] * q["rows_per_chunk"]
        assert (q["sums_nchunks"] - 1) * q["sums_rows_per_chunk"] < n <= q["sums_nchunks"] * q["sums_rows_per_chunk"]


def test_gmm_geometry_refuses_what_the_fit_refuses():
    for n, d, k in ((0, 1, 1), (10, 65, 1), (10, 1, 65), (2**31, 1, 1), (10, 0, 1)):
        with pytest.raises(_lib.SqgrError):
            _lib.gmm_geometry(n, d, k)


def test_old_gmm_cases_bind_no_cap():
    """What the two new cases add: before them no case had a block of two tiles or a capped grid."""
    for name, c in NC.CASES.items():
        if name in NC.GEOMETRY_CASES:
            continue
        q = _lib.gmm_geometry(c.n, c.d, c.k)
        assert q["e_tiles_per_block"] == 1 and c.n // q["M_MIN_ROWS"] <= min(q["M_SUMS_BLOCKS"], q["M_MAX_BLOCKS"] // c.k), name


def test_cap_rows_binds():
    c = NC.CASES["cap_rows"]
    q = _lib.gmm_geometry(c.n, c.d, c.k)
    ntiles = ceil_div(c.n, q["E_T"])
    # the E-step: more tiles than blocks, so a block walks two; the last block has one tile, and that tile one row
    assert ntiles > q["E_MAX_BLOCKS"] and q["e_tiles_per_block"] >= 2
    assert (ntiles, q["e_tiles_per_block"], q["e_blocks"]) == (4105, 2, 2053)
    assert ntiles - (q["e_blocks"] - 1) * q["e_tiles_per_block"] == 1 and c.n - (ntiles - 1) * q["E_T"] == 1
    # the weighted sums: the chunk cap binds (uncapped: one chunk more, of the least rows), the last chunk has 3 rows
    uncapped = c.n // q["M_MIN_ROWS"]
    assert uncapped > q["M_SUMS_BLOCKS"] == q["sums_nchunks"] and q["sums_rows_per_chunk"] > q["M_MIN_ROWS"]
    assert (uncapped, q["sums_nchunks"], q["sums_rows_per_chunk"]) == (513, 512, 514)
    assert c.n - (q["sums_nchunks"] - 1) * q["sums_rows_per_chunk"] == 3
    # the covariance sums: capped at M_MAX_BLOCKS / k
    cap = q["M_MAX_BLOCKS"] // c.k
    assert uncapped > cap == q["nchunks"] and (q["nchunks"], q["rows_per_chunk"]) == (512, 514)
    assert c.n - (q["nchunks"] - 1) * q["rows_per_chunk"] == 3


def test_cap_cov_k64_binds():
    c = NC.CASES["cap_cov_k64"]
    q = _lib.gmm_geometry(c.n, c.d, c.k)
    uncapped, cap = c.n // q["M_MIN_ROWS"], q["M_MAX_BLOCKS"] // c.k
    # the covariance cap binds while the cap of the weighted sums does not: the two kernels cut the rows differently
    assert uncapped > cap == q["nchunks"] and (uncapped, cap, q["rows_per_chunk"]) == (33, 32, 529)
    assert uncapped <= q["M_SUMS_BLOCKS"] and q["sums_nchunks"] == uncapped == 33
    assert q["sums_rows_per_chunk"] != q["rows_per_chunk"]
    assert q["e_tiles_per_block"] == 1 and c.n - (ceil_div(c.n, q["E_T"]) - 1) * q["E_T"] == 1  # the last tile has one row


# ---- the PCA moments ---------------------------------------------------------------------------------------------------------------------
def pca_restated(n: int, d: int, q: dict) -> dict:
    """``pca_geometry`` of csrc/sqgr_pca.hip from the constants in ``q``."""
    out = {"nt": ceil_div(d, q["PCA_TILE"])}
    out["npairs"] = out["nt"] * (out["nt"] + 1) // 2
    base = ceil_div(n, q["PCA_CHUNK"])
    out["mean_rows"] = q["PCA_CHUNK"] * ceil_div(base, q["PCA_MAX_CHUNKS"])
    out["mean_chunks"] = ceil_div(n, out["mean_rows"])
    max_chunks = min(q["PCA_MAX_CHUNKS"], max(1, q["PCA_TARGET_BLOCKS"] // out["npairs"]))
    out["scat_rows"] = q["PCA_CHUNK"] * ceil_div(base, max_chunks)
    out["scat_chunks"] = ceil_div(n, out["scat_rows"])
    return out


def scatter_chunk_cap(d: int, q: dict) -> int:
    nt = ceil_div(d, q["PCA_TILE"])
    return min(q["PCA_MAX_CHUNKS"], max(1, q["PCA_TARGET_BLOCKS"] // (nt * (nt + 1) // 2)))


def pca_sweep() -> list:
    c = _lib.pca_geometry(2, 2)
    chunk, most, tile = c["PCA_CHUNK"], c["PCA_MAX_CHUNKS"], c["PCA_TILE"]
    max_d = _lib.pca_info()["max_features"]
    ds = (2, 3, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 1100, max_d - 1, max_d)
    pairs = set()
    for d in ds:
        cap = scatter_chunk_cap(d, c)
        ns = {2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk, 3 * chunk + 1, 5633, 100_003, 2**31 - 1}
        for edge in (chunk * cap, 2 * chunk * cap, chunk * most, 2 * chunk * most):  # the chunks grow to two and to three units
            ns |= {edge - 1, edge, edge + 1}
        pairs |= {(n, d) for n in ns}
    pairs |= {(k.n, k.d) for k in list(PC.CASES.values()) + list(PC.SEAM_CASES.values())}
    return sorted(pairs)


def test_pca_geometry_equals_the_restatement():
    pairs = pca_sweep()
    assert len(pairs) >= 200
    for n, d in pairs:
        q = _lib.pca_geometry(n, d)
        want = pca_restated(n, d, q)
        assert {key: q[key] for key in want} == want, (n, d)
        assert set(want) | {"PCA_CHUNK", "PCA_MAX_CHUNKS", "PCA_TARGET_BLOCKS", "PCA_TILE"} == set(q)
        assert q["mean_chunks"] <= q["PCA_MAX_CHUNKS"] and q["scat_chunks"] <= scatter_chunk_cap(d, q)
        for rows, chunks in ((q["mean_rows"], q["mean_chunks"]), (q["scat_rows"], q["scat_chunks"])):
            assert rows % q["PCA_CHUNK"] == 0 and (chunks - 1) * rows < n <= chunks * rows
    assert _lib.pca_info()["chunk_rows"] == _lib.pca_geometry(2, 2)["PCA_CHUNK"] and _lib.pca_info()["tile_columns"] == _lib.pca_geometry(2, 2)["PCA_TILE"]


def test_pca_geometry_refuses_what_create_refuses():
    for n, d in ((1, 10), (10, 1), (10, 4097), (2**31, 10)):
        with pytest.raises(_lib.SqgrError):
            _lib.pca_geometry(n, d)


def test_old_pca_cases_bind_no_cap():
    for name in PC.NAMES:
        c = PC.case(name)
        q = _lib.pca_geometry(c.n, c.d)
        assert q["mean_rows"] == q["scat_rows"] == q["PCA_CHUNK"] and q["scat_chunks"] <= 2 and q["nt"] <= 3, name


def test_mean_cap_binds():
    c = PC.SEAM_CASES["mean_cap"]
    q = _lib.pca_geometry(c.n, c.d)
    base = ceil_div(c.n, q["PCA_CHUNK"])
    assert base > q["PCA_MAX_CHUNKS"] and q["mean_rows"] >= 2 * q["PCA_CHUNK"]  # more units than chunks: a chunk holds two
    assert (base, q["mean_rows"], q["mean_chunks"]) == (1025, 1024, 513) and c.n - (q["mean_chunks"] - 1) * q["mean_rows"] == 1
    assert (q["npairs"], q["scat_rows"], q["scat_chunks"]) == (1, 1024, 513)


def test_limit_d4096_binds():
    c = PC.SEAM_CASES["limit_d4096"]
    q = _lib.pca_geometry(c.n, c.d)
    assert c.d == _lib.pca_info()["max_features"] and (q["nt"], q["npairs"]) == (64, 2080)
    assert q["npairs"] > q["PCA_TARGET_BLOCKS"] and scatter_chunk_cap(c.d, q) == 1  # more tile pairs than target blocks: one chunk
    assert q["scat_chunks"] == 1 and q["scat_rows"] >= c.n and c.n % 32 == 1  # whose last sub-tile of 32 staged rows has one row
    assert q["mean_chunks"] == 3


def test_capped_chunks_binds():
    c = PC.SEAM_CASES["capped_chunks"]
    q = _lib.pca_geometry(c.n, c.d)
    base, cap = ceil_div(c.n, q["PCA_CHUNK"]), scatter_chunk_cap(c.d, q)
    assert (q["nt"], q["npairs"]) == (18, 171) and c.d - (q["nt"] - 1) * q["PCA_TILE"] == 12  # the last tile has 12 columns
    assert base > cap and cap < q["PCA_MAX_CHUNKS"] and (base, cap) == (12, 11)  # the target of blocks caps the chunks, not PCA_MAX_CHUNKS
    assert (q["scat_rows"], q["scat_chunks"]) == (1024, 6) and c.n - (q["scat_chunks"] - 1) * q["scat_rows"] == 513
    assert q["mean_rows"] == q["PCA_CHUNK"]  # the column sums are not capped here: the two kernels cut the rows differently

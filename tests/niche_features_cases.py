"""Shared inputs of the niche feature tests: tests/golden/make_niche_features_golden.py pushes the small cases through the reference's
literal code, tests/test_niche_features_cpu.py pins the numpy restatement (tests/niche_features_oracle.py) to that golden, and
tests/test_niche_features_gpu.py runs the same cases and the larger generated ones on the device.  No device compute here."""

from __future__ import annotations

import numpy as np
import pandas as pd
from scipy import sparse
from scipy.spatial import cKDTree

N_VARS = 5
CATEGORIES = ["B", "T", "empty", "myeloid", "stroma"]  # "empty" has no member


def hex_lattice(n_rows: int, n_cols: int) -> sparse.csr_matrix:
    """A hexagonal patch in scan order (odd rows shifted right): up to six neighbours, symmetric, float64 ones."""
    r, c = np.divmod(np.arange(n_rows * n_cols), n_cols)
    src, dst = [], []
    for dr, dc_even, dc_odd in ((0, -1, -1), (0, 1, 1), (-1, -1, 0), (-1, 0, 1), (1, -1, 0), (1, 0, 1)):
        rr = r + dr
        cc = c + np.where(r % 2 == 0, dc_even, dc_odd)
        ok = (rr >= 0) & (rr < n_rows) & (cc >= 0) & (cc < n_cols)
        src.append(np.flatnonzero(ok))
        dst.append((rr * n_cols + cc)[ok])
    a = sparse.csr_matrix((np.ones(sum(map(len, src))), (np.concatenate(src), np.concatenate(dst))), shape=(len(r), len(r)))
    a.sum_duplicates()
    assert (a != a.T).nnz == 0 and a.data.max() == 1
    return a


def knn_graph(n: int, k: int, seed: int, set_diag: bool = False) -> sparse.csr_matrix:
    """The directed k-nearest-neighbour graph of ``n`` uniform points (not symmetrised, as ``KNNBuilder`` leaves it), float64 ones;
    ``set_diag``: with a self loop on every node."""
    xy = np.random.default_rng(seed).random((n, 2))
    _, idx = cKDTree(xy).query(xy, k=k + 1)
    rows = np.repeat(np.arange(n), k)
    a = sparse.csr_matrix((np.ones(n * k), (rows, idx[:, 1:].ravel())), shape=(n, n))
    if set_diag:
        a = (a + sparse.identity(n, format="csr")).tocsr()
    a.sum_duplicates()
    return a


def with_isolated(a: sparse.csr_matrix, seed: int, n_isolated: int, n_sinks: int) -> sparse.csr_matrix:
    """``a`` with ``n_isolated`` nodes cut off entirely and ``n_sinks`` more that keep only their incoming edges."""
    n = a.shape[0]
    pick = np.random.default_rng(seed).choice(n, n_isolated + n_sinks, replace=False)
    keep_row, keep_col = np.ones(n), np.ones(n)
    keep_row[pick] = 0
    keep_col[pick[:n_isolated]] = 0
    out = (sparse.diags(keep_row) @ a @ sparse.diags(keep_col)).tocsr()
    out.eliminate_zeros()
    out.sum_duplicates()
    return out


def spectral(a: sparse.csr_matrix) -> sparse.csr_matrix:
    """The symmetrised graph under the spectral transform ``D^-1/2 A D^-1/2``: positive float64 weights."""
    s = a.maximum(a.T).tocsr()
    d = np.asarray(s.sum(axis=1)).ravel()
    inv = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    out = (sparse.diags(inv) @ s @ sparse.diags(inv)).tocsr()
    out.sum_duplicates()
    return out


def expression(n: int, n_vars: int, seed: int, density: float = 0.4) -> sparse.csr_matrix:
    """Counts 1 .. 10 at ``density`` of the entries plus a little noise so that products round: CSR float64."""
    rng = np.random.default_rng(seed)
    x = sparse.random(n, n_vars, density=density, random_state=np.random.RandomState(seed), format="csr", dtype=np.float64)
    x.data = np.round(x.data * 9 + 1) + rng.random(x.nnz) / 3
    x.sum_duplicates()
    return x


def label_codes(n: int, seed: int) -> np.ndarray:
    """Codes into ``CATEGORIES`` in spatially random order; code 2 ("empty") never occurs."""
    return np.random.default_rng(seed).choice([0, 1, 3, 4], size=n, p=[0.4, 0.3, 0.2, 0.1]).astype(np.int32)


def categorical(codes: np.ndarray) -> pd.Categorical:
    return pd.Categorical.from_codes(codes, categories=CATEGORIES)


def plain_labels(codes: np.ndarray) -> np.ndarray:
    """The same labels as a column of plain strings (not categorical): astype("category") sorts the four names that occur."""
    return np.asarray(CATEGORIES, dtype=object)[codes]


# the golden cases
def golden_graphs() -> dict[str, sparse.csr_matrix]:
    knn = knn_graph(150, 6, 11)
    return {
        "hex": hex_lattice(12, 14),
        "knn": knn,
        "knn_loops": knn_graph(150, 6, 11, set_diag=True),
        "isolated": with_isolated(knn_graph(120, 6, 12), 13, 8, 6),
        "weighted": spectral(knn),
    }


UNIT_GRAPHS = ("hex", "knn", "knn_loops", "isolated")
AGGREGATE_GRAPHS = ("knn_loops", "isolated")  # graphs whose shells also go through the literal `_normalize` / `_aggregate` one by one
# (distance, abs_nhood, n_hop_weights) of the neighbourhood profile
PROFILE_SETTINGS = ((1, False, None), (1, True, None), (2, False, [1.0, 0.5]), (3, False, [2.0, 0.25]), (3, True, [0.5]), (3, False, None))


def setting_tag(distance: int, abs_nhood: bool, weights) -> str:
    return f"d{distance}_{'abs' if abs_nhood else 'rel'}_{'none' if weights is None else '-'.join(map(str, weights))}"


def stored_graph(ref, name: str) -> sparse.csr_matrix:
    """Graph ``name`` as the golden file holds it."""
    indptr = ref[f"in/{name}/indptr"]
    return sparse.csr_matrix((ref[f"in/{name}/data"], ref[f"in/{name}/indices"], indptr), shape=(len(indptr) - 1,) * 2)


def profile_inputs(codes: np.ndarray, labels: str) -> tuple[np.ndarray, int]:
    """``(codes, n_categories)`` of the label column ``labels``: "categorical" (five categories, one empty) or "plain" (strings, which
    ``astype("category")`` turns into the four sorted names that occur)."""
    if labels == "categorical":
        return codes, len(CATEGORIES)
    column = pd.Series(plain_labels(codes)).astype("category")
    return column.cat.codes.to_numpy().astype(np.int32), len(column.cat.categories)


def hub_graph(capacity: int, n: int = 3000, seed: int = 21) -> tuple[sparse.csr_matrix, dict[str, int]]:
    """A directed kNN-6 graph with planted rows around the shell builder's on-chip capacity (``capacity`` = the largest expansion — sum
    of the lengths of the rows a row walks — that stays on chip): ``fat`` nodes of out-degree 32; node ``at`` points at capacity / 32 of
    them (expansion == capacity), node ``above`` at one more (the global-memory path) and node ``hub`` at 700 nodes."""
    assert capacity % 32 == 0 and capacity // 32 + 1 <= 40
    rng = np.random.default_rng(seed)
    a = knn_graph(n, 6, seed).tolil()
    special = rng.choice(n, 43, replace=False)
    fat, at, above, hub = special[:40], int(special[40]), int(special[41]), int(special[42])
    others = np.setdiff1d(np.arange(n), special)
    for f in fat:
        a.rows[f] = sorted(rng.choice(others, 32, replace=False).tolist())
        a.data[f] = [1.0] * 32
    for node, count in ((at, capacity // 32), (above, capacity // 32 + 1)):
        a.rows[node] = sorted(fat[:count].tolist())
        a.data[node] = [1.0] * count
    a.rows[hub] = sorted(rng.choice(others, 700, replace=False).tolist())
    a.data[hub] = [1.0] * 700
    a = a.tocsr()
    a.sum_duplicates()
    return a, {"at": at, "above": above, "hub": hub}


def two_domains(n_rows: int, n_cols: int, n_vars: int, seed: int) -> tuple[sparse.csr_matrix, np.ndarray, np.ndarray]:
    """A hex lattice whose left and right halves express different genes: ``(graph, X dense float32, domain of every spot)``."""
    rng = np.random.default_rng(seed)
    a = hex_lattice(n_rows, n_cols)
    domain = ((np.arange(n_rows * n_cols) % n_cols) >= n_cols // 2).astype(np.int64)
    means = np.where(np.arange(n_vars)[None, :] % 2 == domain[:, None], 6.0, 1.0)
    x = (means + rng.normal(0.0, 1.0, means.shape)).astype(np.float32)
    return a, x, domain

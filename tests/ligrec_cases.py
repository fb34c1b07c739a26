"""Shared case builders of the ligrec regime tests (tests/test_ligrec_cases_cpu.py proves their properties on the oracle
alone, tests/test_ligrec_regimes_gpu.py runs them on the device).  No device compute here.

The device compares ``shuf > obs`` per permutation and the suite's only view of the float64 group sums of permutations other
than the first one is that comparison.  ``obs`` is an input of ``sqgr_ligrec_counts``, so a test can put it exactly ON a
permuted sum (the strict ``>`` must not count that permutation) or one ulp below it (it must): a sum that is wrong in its
last bit, in whichever lane of the wave that permutation ran, then changes a count."""

from __future__ import annotations

from collections.abc import Sequence

import numpy as np

from oracle import devrng
from oracle import restate as O

# planted-tie shapes shared by the CPU proof and the GPU tests: k -> (n, g, k, seed); n >= 8 k keeps every planted sum > 0
PLANTED_SHAPES = {30: (320, 6, 30, 130), 100: (800, 6, 100, 131), 200: (1600, 6, 200, 132), 257: (2056, 6, 257, 133)}
N_NUMPY, N_DEVICE, DEVICE_BEGIN = 130, 70, 5  # 130 = lanes 0..63 twice and a partial tail; 5: a range that starts inside a group of 16
N_EDGE = 100  # permutations of the score-block edge case: with 255..257 pairs, columns 254..256 then hold both kinds of cell
COLUMN_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
CELL0_GENES = (4, 7, 10)  # lengths 17, 65, 129: the last trip is padded and cell 0 holds a value
NPL_CAP = 16384  # permutations per launch chunk of sqgr_ligrec_counts (sqgr_ligrec.hip: `npl`)


def problem(n: int, g: int, k: int, seed: int, density: float = 0.5, n_inter: int | None = None):
    """(data, clustering, interactions): gamma values at ``density``, ``k`` clusters of (almost) equal size in random order —
    every cluster is populated —, all ordered gene pairs or ``n_inter`` random ones."""
    rng = np.random.default_rng(seed)
    data = ((rng.random((n, g)) < density) * rng.gamma(2.0, 1.0, (n, g))).astype(np.float64)
    cl = rng.permutation(np.arange(n) % k).astype(np.int32)
    inter = np.array([(i, j) for i in range(g) for j in range(g)], dtype=np.int32)
    if n_inter is not None:
        inter = inter[rng.choice(len(inter), n_inter, replace=False)]
    return data, cl, inter


def cluster_pairs(k: int, n_random: int, seed: int, fixed: Sequence[tuple[int, int]] = ()) -> np.ndarray:
    """``n_random`` random ordered cluster pairs followed by (0, k-1), (k-1, 0), the pairs ``fixed`` and, where those clusters
    exist, (254, 255) and (255, 256): the last 8-bit label and the first cluster of a second tile."""
    rng = np.random.default_rng(seed)
    cp = [tuple(p) for p in np.stack([rng.integers(0, k, n_random), rng.integers(0, k, n_random)], axis=1)]
    cp += [(0, k - 1), (k - 1, 0), *fixed]
    cp += [p for p in ((254, 255), (255, 256)) if max(p) < k]
    return np.array(cp, dtype=np.int32)


def philox_labels(clustering: np.ndarray, seed: int, perm_begin: int, perm_end: int, batch: int = 128) -> np.ndarray:
    """``O.ligrec_perm_labels_philox`` through batched calls of the device generator's restatement (oracle/devrng.py): about
    0.2 ms per permutation of 96 cells instead of 3 ms row by row; batches of 128 keep the temporaries in cache."""
    cl = np.asarray(clustering)
    base = np.sort(cl)
    out = np.empty((perm_end - perm_begin, len(cl)), dtype=np.int32)
    for a in range(perm_begin, perm_end, batch):
        b = min(a + batch, perm_end)
        out[a - perm_begin : b - perm_begin] = base[devrng.label_permutations(len(cl), seed, np.arange(a, b, dtype=np.int64))]
    return out


def shuffled_sums(data: np.ndarray, perm: np.ndarray, inv_counts: np.ndarray, inter: np.ndarray, cp: np.ndarray) -> np.ndarray:
    """shuf[i, j] = groups[a_j, rec_i] + groups[b_j, lig_i] of one permutation (gr/_ligrec.py:664), (n_inter, n_cp)."""
    groups = O.ligrec_group_means(data, perm, inv_counts)
    return groups[cp[:, 0]][:, inter[:, 0]].T + groups[cp[:, 1]][:, inter[:, 1]].T


def planted_obs(data, labels, inv_counts, inter, cp, perms: Sequence[int] | None = None):
    """Thresholds that sit on the permuted sums.  Cell c = i * n_cp + j belongs to permutation ``perms[c % P]`` (default: all
    rows of ``labels``, P = their number); obs[i, j] is that permutation's own sum when ``c // P`` is even — an exact tie, the
    strict `>` must not count it — and ``nextafter(sum, -inf)`` when it is odd — that permutation must count it.

    Returns (obs, tie, below): the float64 thresholds and the two boolean masks; ``cell_owners`` names the owning row of
    ``labels`` per cell."""
    inter, cp = np.asarray(inter), np.asarray(cp)
    perms = np.arange(len(labels)) if perms is None else np.asarray(perms, dtype=np.int64)
    P, n_inter, n_cp = len(perms), len(inter), len(cp)
    cell = np.arange(n_inter * n_cp)
    below = ((cell // P) % 2 == 1)
    obs = np.empty(n_inter * n_cp, dtype=np.float64)
    for slot, p in enumerate(perms):
        mine = cell[cell % P == slot]
        if len(mine):
            obs[mine] = shuffled_sums(data, labels[p], inv_counts, inter, cp).ravel()[mine]
    obs[below] = np.nextafter(obs[below], -np.inf)
    shape = (n_inter, n_cp)
    return obs.reshape(shape), ~below.reshape(shape), below.reshape(shape)


def cell_owners(shape: tuple[int, int], perms: Sequence[int] | int) -> np.ndarray:
    """row of ``labels`` that owns each cell of ``planted_obs`` (``perms``: the same list, or the number of rows)"""
    perms = np.arange(perms) if np.isscalar(perms) else np.asarray(perms, dtype=np.int64)
    return perms[np.arange(shape[0] * shape[1]) % len(perms)].reshape(shape)


def score_with_obs(data, perm_labels, inv_counts, obs, inter, cp, valid) -> np.ndarray:
    """The loop of ``O.ligrec_score_permutations`` (gr/_ligrec.py:616-673) against the given thresholds ``obs``."""
    inter, cp = np.asarray(inter), np.asarray(cp)
    valid = np.asarray(valid, dtype=bool)
    counts = np.zeros(obs.shape, dtype=np.int64)
    for perm in perm_labels:
        counts += (valid & (shuffled_sums(data, perm, inv_counts, inter, cp) > obs)).astype(np.int64)
    return counts


def sparse_valid(shape: tuple[int, int], seed: int, n_zero: int = 7) -> np.ndarray:
    """all ones apart from ``n_zero`` random cells"""
    valid = np.ones(shape, dtype=bool)
    rng = np.random.default_rng(seed)
    valid.ravel()[rng.choice(valid.size, n_zero, replace=False)] = False
    return valid


def inv_counts_of(clustering: np.ndarray, k: int) -> np.ndarray:
    return 1.0 / np.maximum(np.bincount(clustering, minlength=k).astype(np.float64), 1)


def column_lengths_problem(lengths: Sequence[int], n: int, k: int, seed: int, with_cell0: Sequence[int] = ()):
    """(data, clustering): dense float64 (n, len(lengths)) whose gene g has exactly ``lengths[g]`` non-zeros, gamma values, at
    random rows (sorted, as CSC stores them); the genes ``with_cell0`` hold one of theirs at cell 0.  ``k`` balanced clusters."""
    rng = np.random.default_rng(seed)
    data = np.zeros((n, len(lengths)), dtype=np.float64)
    for g, m in enumerate(lengths):
        if g in with_cell0:
            rows = np.concatenate([[0], 1 + rng.choice(n - 1, m - 1, replace=False)])
        else:
            rows = rng.choice(n, m, replace=False)
        rows = np.sort(rows)
        data[rows, g] = rng.gamma(2.0, 1.0, m)
    cl = rng.permutation(np.arange(n) % k).astype(np.int32)
    return data, cl


def planted_case(k: int):
    """The planted-tie problem of cluster count ``k`` (one per width of the sum kernel: 4, 2, 1 waves, and the cluster tiles)."""
    n, g, kk, seed = PLANTED_SHAPES[k]
    data, cl, inter = problem(n, g, kk, seed, n_inter=12)
    cp = cluster_pairs(kk, 300, seed + 1)
    return data, cl, inter, cp, inv_counts_of(cl, kk)


def edge_case(n_cp: int):
    """K = 20 with ``n_cp`` cluster pairs: the last block of the score kernel is full (256), one short (255) or one over (257)."""
    data, cl, inter = problem(320, 6, 20, seed=40, n_inter=12)
    allp = np.array([(a, b) for a in range(20) for b in range(20)], dtype=np.int32)
    cp = allp[np.random.default_rng(41).permutation(len(allp))[:n_cp]]
    return data, cl, inter, cp, inv_counts_of(cl, 20)


def lengths_case(k: int):
    """The planted column lengths at n = 300; the interactions hold (empty gene, fullest gene) both ways."""
    data, cl = column_lengths_problem(COLUMN_LENGTHS, 300, k, seed=50 + k, with_cell0=CELL0_GENES)
    g = len(COLUMN_LENGTHS)
    inter = np.array([(0, g - 1), (g - 1, 0)] + [(i, (5 * i + 3) % g) for i in range(g)] + [(i, i) for i in range(1, g)], dtype=np.int32)
    cp = np.array([(a, b) for a in range(k) for b in range(k)], dtype=np.int32) if k <= 16 else cluster_pairs(k, 300, 60 + k)
    return data, cl, inter, cp, inv_counts_of(cl, k)


def chunk_case(wide: bool):
    """Tiny shapes for permutation ranges beyond one launch chunk: (96 cells, 3 genes, 2 clusters) or (320, 2, 257)."""
    if not wide:
        data, cl, inter = problem(96, 3, 2, seed=70)
        cp = np.array([(0, 0), (0, 1), (1, 0), (1, 1)], dtype=np.int32)
        return data, cl, inter, cp, inv_counts_of(cl, 2), 2
    data, cl, inter = problem(320, 2, 257, seed=71)
    cp = cluster_pairs(257, 30, 72, fixed=[(128, 129), (129, 128)])  # 2 tiles of 129: 128 | 129 is the tile border
    return data, cl, inter, cp, inv_counts_of(cl, 257), 257

"""A numpy restatement of ``csrc/sqgr_leiden.hip`` (the contract of ``sqgr_leiden`` in ``include/sqgr.h``), written from that contract:
the same hash, gain expression, tie rules and caps, with numpy int64 / Python integers for every weight sum and numpy float64 for the
gain — every operation rounded on its own, in the header's order.  The device must return these labels and stats bit for bit.

Also the property checkers of the suite: canonical labelling, connected communities, node stability in exact arithmetic, and the
quality ``Q`` both this restatement and networkx's Louvain are measured with."""

from __future__ import annotations

from fractions import Fraction

import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import connected_components

WEIGHT_BITS = 24
SWEEP_CAP = 1024
ITER_CAP = 16
CAPACITY = 128  # LD_CAP: decides the kernel's path only, nothing here
STATS = ("n_communities", "iterations", "levels", "sweeps", "sum_in", "two_m", "cap_hits", "settled")


def quantise(conn: sparse.csr_matrix) -> np.ndarray:
    """``max(1, rint(w / w_max * 2**24))`` as int32 for the stored values of ``conn``."""
    w = np.asarray(conn.data, dtype=np.float64)
    return np.maximum(1, np.rint(w / w.max() * float(2**WEIGHT_BITS))).astype(np.int32)


def ld_hash(v: np.ndarray, s: int) -> np.ndarray:
    x = v.astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32((s * 0x85EBCA77) & 0xFFFFFFFF)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _group_sum(keys: np.ndarray, vals: np.ndarray, size: int) -> np.ndarray:
    out = np.zeros(size, dtype=np.int64)
    np.add.at(out, keys, vals)
    return out


class _Level:
    def __init__(self, n: int, rows: np.ndarray, cols: np.ndarray, w: np.ndarray) -> None:
        self.n, self.rows, self.cols, self.w = n, rows, cols, w
        self.k = _group_sum(rows, w, n)  # self loop included


def _pairs(v: np.ndarray, c: np.ndarray, w: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Distinct (vertex, community) pairs, ascending, with their exact weight sums."""
    uniq, inv = np.unique(v.astype(np.int64) * n + c, return_inverse=True)
    return uniq // n, uniq % n, _group_sum(inv.ravel(), w, uniq.shape[0])


def _pick(n: int, pv: np.ndarray, pc: np.ndarray, g: np.ndarray, kvc: np.ndarray, own: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(want, dk_best - own's k) per vertex from its candidate pairs: best by (gain descending, id ascending), a move needs a strictly
    larger gain than the own community's.  Vertices without a pair want nothing."""
    want = np.full(n, -1, dtype=np.int64)
    k_best = np.zeros(n, dtype=np.int64)
    k_own = np.zeros(n, dtype=np.int64)
    if pv.shape[0] == 0:
        return want, k_best, k_own
    order = np.lexsort((pc, -g, pv))
    first = order[np.r_[True, pv[order][1:] != pv[order][:-1]]]
    g_own = np.full(n, -np.inf)
    g_own[pv[own]] = g[own]
    k_own[pv[own]] = kvc[own]
    bv, bc, bg = pv[first], pc[first], g[first]
    move = ~own[first] & (bg > g_own[bv])
    want[bv[move]] = bc[move]
    k_best[bv[move]] = kvc[first][move]
    return want, k_best, k_own


def _movers(L: _Level, want: np.ndarray, sweep: int) -> np.ndarray:
    """Of the vertices that want to move, those whose (hash, vertex) is smaller than that of every neighbour that wants to move too."""
    wanting = want >= 0
    e = (L.rows != L.cols) & wanting[L.rows] & wanting[L.cols]
    r, c = L.rows[e], L.cols[e]
    hr, hc = ld_hash(r, sweep), ld_hash(c, sweep)
    loses = ~((hr < hc) | ((hr == hc) & (r < c)))
    lose = np.zeros(L.n, dtype=bool)
    lose[r[loses]] = True
    return wanting & ~lose


def _sum_sq(tot: np.ndarray) -> int:
    return sum(t * t for t in tot[tot != 0].tolist())


def quality_from_integers(sum_in: int, sum_sq: int, gamma: float, two_m: int) -> float:
    m2 = float(two_m)
    return float(sum_in) / m2 - gamma * (float(sum_sq) / (m2 * m2))


def _local_moving(L: _Level, comm: np.ndarray, gamma: float, two_m: int, stats: dict) -> np.ndarray:
    n, m2 = L.n, float(two_m)
    tot = _group_sum(comm, L.k, n)
    sum_in = int(L.w[comm[L.rows] == comm[L.cols]].sum())
    best_q, best_comm = quality_from_integers(sum_in, _sum_sq(tot), gamma, two_m), comm.copy()
    off = L.rows != L.cols
    ar = np.arange(n, dtype=np.int64)
    for s in range(SWEEP_CAP):
        pv, pc, kvc = _pairs(np.r_[L.rows[off], ar], np.r_[comm[L.cols[off]], comm], np.r_[L.w[off], np.zeros(n, dtype=np.int64)], n)
        kv = L.k[pv]
        own = pc == comm[pv]
        less = tot[pc] - np.where(own, kv, 0)
        g = kvc.astype(np.float64) - gamma * kv.astype(np.float64) * less.astype(np.float64) / m2
        want, k_best, k_own = _pick(n, pv, pc, g, kvc, own)
        mv = _movers(L, want, s)
        wv = np.flatnonzero(want >= 0)
        if wv.shape[0]:  # against overshoot: the first of those that want into a community, or a gain that survives all of them joining
            t = want[wv]
            claimed = _group_sum(t, L.k[wv], n)
            prio = (ld_hash(wv, s).astype(np.uint64) << np.uint64(32)) | wv.astype(np.uint64)
            first = np.full(n, np.iinfo(np.uint64).max, dtype=np.uint64)
            np.minimum.at(first, t, prio)
            g_own = np.full(n, -np.inf)
            g_own[pv[own]] = g[own]
            crowded = tot[t] + claimed[t] - L.k[wv]
            survives = k_best[wv].astype(np.float64) - gamma * L.k[wv].astype(np.float64) * crowded.astype(np.float64) / m2 > g_own[wv]
            allowed = np.zeros(n, dtype=bool)
            allowed[wv] = (prio == first[t]) | survives
            mv &= allowed
        stats["sweeps"] += 1
        if not mv.any():
            return comm
        old, new = comm[mv], want[mv]
        comm[mv] = new
        np.add.at(tot, new, L.k[mv])
        np.subtract.at(tot, old, L.k[mv])
        sum_in += 2 * int((k_best[mv] - k_own[mv]).sum())
        q = quality_from_integers(sum_in, _sum_sq(tot), gamma, two_m)
        if q > best_q:
            best_q, best_comm = q, comm.copy()
    stats["cap_hits"] += 1
    return best_comm


def _refine(L: _Level, comm: np.ndarray, gamma: float, two_m: int, stats: dict) -> np.ndarray:
    n, m2 = L.n, float(two_m)
    tot = _group_sum(comm, L.k, n)
    inner = (L.rows != L.cols) & (comm[L.rows] == comm[L.cols])
    vext = _group_sum(L.rows[inner], L.w[inner], n)
    rcomm = np.arange(n, dtype=np.int64)
    rtot, rext, rsize = L.k.copy(), vext.copy(), np.ones(n, dtype=np.int64)
    kf = L.k.astype(np.float64)
    tot_c = tot[comm]
    connected = vext.astype(np.float64) >= gamma * kf * (tot_c - L.k).astype(np.float64) / m2
    ir, ic, iw = L.rows[inner], L.cols[inner], L.w[inner]
    for s in range(SWEEP_CAP):
        eligible = (rsize[rcomm] == 1) & connected
        ev = np.flatnonzero(eligible)
        e = eligible[ir]
        pv, pc, kvc = _pairs(np.r_[ir[e], ev], np.r_[rcomm[ic[e]], rcomm[ev]], np.r_[iw[e], np.zeros(ev.shape[0], dtype=np.int64)], n)
        kv = L.k[pv]
        own = pc == rcomm[pv]
        ts = rtot[pc]
        valid = own | (rext[pc].astype(np.float64) >= gamma * ts.astype(np.float64) * (tot_c[pv] - ts).astype(np.float64) / m2)
        less = ts - np.where(own, kv, 0)
        g = kvc.astype(np.float64) - gamma * kv.astype(np.float64) * less.astype(np.float64) / m2
        want, k_best, _ = _pick(n, pv[valid], pc[valid], g[valid], kvc[valid], own[valid])
        mv = _movers(L, want, s)
        stats["sweeps"] += 1
        if not mv.any():
            break
        old, new = rcomm[mv], want[mv]
        rcomm[mv] = new
        np.add.at(rtot, new, L.k[mv])
        np.subtract.at(rtot, old, L.k[mv])
        np.add.at(rsize, new, 1)
        np.subtract.at(rsize, old, 1)
        np.add.at(rext, new, vext[mv] - 2 * k_best[mv])
    return rcomm


def canonical(ids: np.ndarray) -> np.ndarray:
    """Communities numbered by size descending, ties by smallest member."""
    uniq, first, inv, size = np.unique(ids, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -size))
    rank = np.empty(uniq.shape[0], dtype=np.int64)
    rank[order] = np.arange(uniq.shape[0])
    return rank[inv.ravel()].astype(np.int32)


def validate(indptr: np.ndarray, indices: np.ndarray, weights: np.ndarray) -> None:
    """The refusals of ``sqgr_leiden`` as ``ValueError``."""
    n = indptr.shape[0] - 1
    if indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != indices.shape[0]:
        raise ValueError("indptr")
    if ((indices < 0) | (indices >= n)).any():
        raise ValueError("a column index is outside [0, n)")
    if (weights < 1).any():
        raise ValueError("a weight is smaller than 1")
    rows = np.repeat(np.arange(n), np.diff(indptr))
    same_row = rows[1:] == rows[:-1]
    if (same_row & (indices[1:] <= indices[:-1])).any():
        raise ValueError("a row of the graph is not sorted or repeats an entry")
    if (rows == indices).any():
        raise ValueError("the graph has a self loop")
    a = sparse.csr_matrix((weights.astype(np.int64), indices, indptr), shape=(n, n))
    if (a != a.T).nnz:
        raise ValueError("the graph is not symmetric")


def leiden(indptr: np.ndarray, indices: np.ndarray, weights: np.ndarray, resolution: float, n_iterations: int = -1) -> tuple[np.ndarray, dict]:
    indptr, indices, weights = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(weights, dtype=np.int64)
    gamma = float(resolution)
    if not (np.isfinite(gamma) and gamma > 0) or n_iterations == 0:
        raise ValueError("resolution / n_iterations")
    n = indptr.shape[0] - 1
    stats = dict.fromkeys(STATS, 0)
    if indices.shape[0] == 0:
        stats.update(n_communities=n, settled=1)
        return np.arange(n, dtype=np.int32), stats
    validate(indptr, indices, weights)
    base = _Level(n, np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)), indices, weights)
    two_m = int(base.k.sum())
    if two_m >= 2**62:
        raise NotImplementedError("2m reaches 2**62")
    prev = np.arange(n, dtype=np.int32)
    for _ in range(ITER_CAP if n_iterations < 0 else n_iterations):
        L, comm, node_of = base, prev.astype(np.int64), np.arange(n, dtype=np.int64)
        while True:
            stats["levels"] += 1
            comm = _local_moving(L, comm, gamma, two_m, stats)
            if np.unique(comm).shape[0] == L.n:
                break
            rcomm = _refine(L, comm, gamma, two_m, stats)
            ids, nr = np.unique(rcomm, return_inverse=True)
            nr = nr.ravel()
            nc = ids.shape[0]
            if nc == L.n:
                break
            pmin = np.full(L.n, nc, dtype=np.int64)
            np.minimum.at(pmin, comm, nr)
            ccomm = np.empty(nc, dtype=np.int64)
            ccomm[nr] = pmin[comm]
            node_of = nr[node_of]
            uniq, inv = np.unique(nr[L.rows] * nc + nr[L.cols], return_inverse=True)
            L, comm = _Level(nc, uniq // nc, uniq % nc, _group_sum(inv.ravel(), L.w, uniq.shape[0])), ccomm
        labels = canonical(node_of)
        stats["iterations"] += 1
        if np.array_equal(labels, prev):
            stats["settled"] = 1
            break
        prev = labels
    stats["n_communities"] = int(prev.max()) + 1
    stats["sum_in"] = int(weights[prev[base.rows] == prev[indices]].sum())
    stats["two_m"] = two_m
    return prev, stats


# ---- property checkers --------------------------------------------------------------------------------------------------------------
def assert_canonical(labels: np.ndarray) -> None:
    labels = np.asarray(labels)
    k = int(labels.max()) + 1
    size = np.bincount(labels, minlength=k)
    assert (size > 0).all(), "an empty label"
    first = np.full(k, labels.shape[0])
    np.minimum.at(first, labels, np.arange(labels.shape[0]))
    key = list(zip((-size).tolist(), first.tolist()))
    assert key == sorted(key), "labels are not numbered by (size descending, smallest member ascending)"


def assert_connected(indptr: np.ndarray, indices: np.ndarray, labels: np.ndarray) -> None:
    """Every community's induced subgraph is connected: the components of the graph that keeps the edges inside communities — the
    disjoint union of the induced subgraphs — are exactly the communities."""
    n = labels.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = labels[rows] == labels[indices]
    a = sparse.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (rows[keep], indices[keep])), shape=(n, n))
    parts, part_of = connected_components(a, directed=False)
    per_community = np.bincount(labels[np.unique(part_of, return_index=True)[1]])
    assert parts == int(labels.max()) + 1, f"communities {np.flatnonzero(per_community > 1)[:5].tolist()} are not connected"


def unstable_vertices(indptr: np.ndarray, indices: np.ndarray, weights: np.ndarray, labels: np.ndarray, resolution: float) -> list:
    """Vertices with a strictly better neighbouring community, in exact arithmetic: ``k_vc 2m - gamma k_v tot_c`` over integers and the
    exact rational value of ``resolution``."""
    n = labels.shape[0]
    gamma = Fraction(float(resolution))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    k = _group_sum(rows, weights.astype(np.int64), n)
    tot = _group_sum(labels, k, n).tolist()
    two_m = int(k.sum())
    pv, pc, kvc = _pairs(np.r_[rows, np.arange(n)], np.r_[labels[indices], labels], np.r_[weights.astype(np.int64), np.zeros(n, dtype=np.int64)], n)
    score: dict = {}
    for v, c, kc in zip(pv.tolist(), pc.tolist(), kvc.tolist()):
        kv = int(k[v])
        less = tot[c] - (kv if c == labels[v] else 0)
        score.setdefault(v, {})[c] = kc * two_m - gamma * kv * less
    return [v for v, s in score.items() if max(s.values()) > s[int(labels[v])]]


def quality(indptr: np.ndarray, indices: np.ndarray, weights: np.ndarray, labels: np.ndarray, resolution: float) -> float:
    """``Q = sum_c (in_c / 2m - gamma (tot_c / 2m)**2)`` of any labelling, from exact integers: the one helper both sides are measured with."""
    n = labels.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    w = weights.astype(np.int64)
    k = _group_sum(rows, w, n)
    two_m = int(k.sum())
    if two_m == 0:
        return 0.0
    tot = _group_sum(np.asarray(labels, dtype=np.int64), k, int(np.max(labels)) + 1)
    sum_in = int(w[labels[rows] == labels[indices]].sum())
    return float(Fraction(sum_in, two_m) - Fraction(float(resolution)) * Fraction(_sum_sq(tot), two_m * two_m))


def louvain_qualities(indptr: np.ndarray, indices: np.ndarray, weights: np.ndarray, resolution: float, seeds: tuple = (0, 1, 2, 3, 4)) -> list:
    """``quality`` of ``networkx.community.louvain_communities`` on the same integer graph, one value per seed."""
    import networkx as nx

    n = indptr.shape[0] - 1
    g = nx.from_scipy_sparse_array(sparse.csr_matrix((weights.astype(np.int64), indices, indptr), shape=(n, n)))
    out = []
    for seed in seeds:
        labels = np.empty(n, dtype=np.int64)
        for c, members in enumerate(nx.community.louvain_communities(g, weight="weight", resolution=resolution, seed=seed)):
            labels[list(members)] = c
        out.append(quality(indptr, indices, weights, labels, resolution))
    return out

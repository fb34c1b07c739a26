"""A numpy restatement of ``csrc/sqgr_leiden_multiplex.hip`` (the contract of ``sqgr_leiden_multiplex`` in ``include/sqgr.h``), written
from that contract: the single-layer restatement (tests/niche_leiden_oracle.py) with two layers over the same vertices — per-layer
exact integers, ``gain = g_0 + layer_ratio * g_1`` with the product rounded and then the sum, candidates and the independent set over
the union of the two neighbourhoods, ``claimed`` per layer, one coarse graph per layer.  The device must return these labels and
stats bit for bit.

Also the host step in front of it (``quantise_pair``: ``W_l = A_l + A_l^T``, one common scale) and the exact-rational checkers of the
suite: the multiplex objective ``Q = sum_l a_l sum_c (in^l_c - gamma_l (tot^l_c)^2 / 2m_l)`` and node stability under it, both with
``Fraction(layer_ratio)`` and ``Fraction(gamma_l)``."""

from __future__ import annotations

from fractions import Fraction

import numpy as np
from scipy import sparse

from tests import niche_leiden_oracle as LO

N_LAYERS = 2
STATS = ("n_communities", "iterations", "levels", "sweeps", "sum_in_0", "two_m_0", "sum_in_1", "two_m_1", "cap_hits", "settled")
SHARED_STATS = ("n_communities", "iterations", "levels", "sweeps", "cap_hits", "settled")  # what a single-layer run reports too
F8 = np.float64


def quantise_pair(latent: sparse.spmatrix, spatial: sparse.spmatrix, use_weights: tuple = (True, True)) -> tuple:
    """The host step: per layer the canonical CSR, values 1 where its ``use_weights`` is false, ``W = A + A^T`` in float64; then
    ``max(1, rint(w / w_max * 2**24))`` as int32 with ``w_max`` the largest value of the two ``W``.  Returns two
    ``(indptr int64, indices int32, weights int32)`` triples."""
    ws = []
    for a, use in zip((latent, spatial), use_weights):
        a = sparse.csr_matrix(a, dtype=np.float64, copy=True)
        a.sum_duplicates()
        a.eliminate_zeros()
        if not use:
            a.data[:] = 1.0
        w = sparse.csr_matrix(a + a.T)
        w.sum_duplicates()
        w.sort_indices()
        ws.append(w)
    w_max = max([float(w.data.max()) for w in ws if w.nnz], default=1.0)
    out = []
    for w in ws:
        q = np.maximum(1, np.rint(w.data / w_max * float(2**LO.WEIGHT_BITS))).astype(np.int32)
        out.append((w.indptr.astype(np.int64), w.indices.astype(np.int32), q))
    return tuple(out)


class _Level2:
    """One level: the two layers' entries over the same ``n`` nodes, and the union of their entries for the independent set."""

    def __init__(self, n: int, layers: list) -> None:
        self.n, self.layers = n, layers
        self.rows = np.r_[layers[0].rows, layers[1].rows]
        self.cols = np.r_[layers[0].cols, layers[1].cols]


def _pairs2(v: np.ndarray, c: np.ndarray, w: list, n: int) -> tuple:
    """Distinct (vertex, community) pairs, ascending, with their exact weight sums per layer."""
    uniq, inv = np.unique(v.astype(np.int64) * n + c, return_inverse=True)
    inv = inv.ravel()
    return uniq // n, uniq % n, [LO._group_sum(inv, w[l], uniq.shape[0]) for l in range(N_LAYERS)]


def _term(l: int, x: np.ndarray, gamma: tuple, a: np.ndarray, b: np.ndarray, two_m: tuple) -> np.ndarray:
    """``(double)x - gamma_l * (double)a * (double)b / (double)two_m_l``, left to right; exactly +0.0 for a layer without weight."""
    if two_m[l] == 0:
        return np.zeros(x.shape[0], dtype=F8)
    return x.astype(F8) - gamma[l] * a.astype(F8) * b.astype(F8) / float(two_m[l])


def _mix(t: list, ratio: float) -> np.ndarray:
    return t[0] + ratio * t[1]  # the product rounded, then the sum


def quality_from_integers(sum_in: list, sum_sq: list, gamma: tuple, two_m: tuple, ratio: float) -> float:
    part = [float(two_m[l]) * LO.quality_from_integers(sum_in[l], sum_sq[l], gamma[l], two_m[l]) if two_m[l] else 0.0 for l in range(N_LAYERS)]
    return part[0] + ratio * part[1]


def _candidates(L: _Level2, of_col: np.ndarray, keep: list, extra: np.ndarray) -> tuple:
    """Pairs (vertex, of_col[neighbour]) over the kept entries of both layers, plus (v, of_col[v]) with weight 0 for v in ``extra``."""
    v, c, w = [], [], [[], []]
    for l, lay in enumerate(L.layers):
        v.append(lay.rows[keep[l]])
        c.append(of_col[lay.cols[keep[l]]])
        for m in range(N_LAYERS):
            w[m].append(lay.w[keep[l]] if m == l else np.zeros(int(keep[l].sum()), dtype=np.int64))
    zeros = np.zeros(extra.shape[0], dtype=np.int64)
    return _pairs2(np.r_[v[0], v[1], extra], np.r_[c[0], c[1], of_col[extra]], [np.r_[w[m][0], w[m][1], zeros] for m in range(N_LAYERS)], L.n)


def _local_moving(L: _Level2, comm: np.ndarray, gamma: tuple, two_m: tuple, ratio: float, stats: dict) -> np.ndarray:
    n = L.n
    k = [lay.k for lay in L.layers]
    tot = [LO._group_sum(comm, k[l], n) for l in range(N_LAYERS)]
    sum_in = [int(lay.w[comm[lay.rows] == comm[lay.cols]].sum()) for lay in L.layers]
    best_q = quality_from_integers(sum_in, [LO._sum_sq(t) for t in tot], gamma, two_m, ratio)
    best_comm = comm.copy()
    off = [lay.rows != lay.cols for lay in L.layers]
    ar = np.arange(n, dtype=np.int64)
    for s in range(LO.SWEEP_CAP):
        pv, pc, kvc = _candidates(L, comm, off, ar)
        own = pc == comm[pv]
        g = _mix([_term(l, kvc[l], gamma, k[l][pv], tot[l][pc] - np.where(own, k[l][pv], 0), two_m) for l in range(N_LAYERS)], ratio)
        want, kb0, ko0 = LO._pick(n, pv, pc, g, kvc[0], own)
        _, kb1, ko1 = LO._pick(n, pv, pc, g, kvc[1], own)
        k_best, k_own = [kb0, kb1], [ko0, ko1]
        mv = LO._movers(L, want, s)
        wv = np.flatnonzero(want >= 0)
        if wv.shape[0]:
            t = want[wv]
            claimed = [LO._group_sum(t, k[l][wv], n) for l in range(N_LAYERS)]
            prio = (LO.ld_hash(wv, s).astype(np.uint64) << np.uint64(32)) | wv.astype(np.uint64)
            first = np.full(n, np.iinfo(np.uint64).max, dtype=np.uint64)
            np.minimum.at(first, t, prio)
            g_own = np.full(n, -np.inf)
            g_own[pv[own]] = g[own]
            crowded = _mix([_term(l, k_best[l][wv], gamma, k[l][wv], tot[l][t] + claimed[l][t] - k[l][wv], two_m) for l in range(N_LAYERS)], ratio)
            allowed = np.zeros(n, dtype=bool)
            allowed[wv] = (prio == first[t]) | (crowded > g_own[wv])
            mv &= allowed
        stats["sweeps"] += 1
        if not mv.any():
            return comm
        old, new = comm[mv], want[mv]
        comm[mv] = new
        for l in range(N_LAYERS):
            np.add.at(tot[l], new, k[l][mv])
            np.subtract.at(tot[l], old, k[l][mv])
            sum_in[l] += 2 * int((k_best[l][mv] - k_own[l][mv]).sum())
        q = quality_from_integers(sum_in, [LO._sum_sq(t) for t in tot], gamma, two_m, ratio)
        if q > best_q:
            best_q, best_comm = q, comm.copy()
    stats["cap_hits"] += 1
    return best_comm


def _refine(L: _Level2, comm: np.ndarray, gamma: tuple, two_m: tuple, ratio: float, stats: dict) -> np.ndarray:
    n = L.n
    k = [lay.k for lay in L.layers]
    tot_c = [LO._group_sum(comm, k[l], n)[comm] for l in range(N_LAYERS)]
    inner = [(lay.rows != lay.cols) & (comm[lay.rows] == comm[lay.cols]) for lay in L.layers]
    vext = [LO._group_sum(lay.rows[inner[l]], lay.w[inner[l]], n) for l, lay in enumerate(L.layers)]
    rcomm = np.arange(n, dtype=np.int64)
    rtot, rext, rsize = [x.copy() for x in k], [x.copy() for x in vext], np.ones(n, dtype=np.int64)
    connected = _mix([_term(l, vext[l], gamma, k[l], tot_c[l] - k[l], two_m) for l in range(N_LAYERS)], ratio) >= 0
    for s in range(LO.SWEEP_CAP):
        eligible = (rsize[rcomm] == 1) & connected
        pv, pc, kvc = _candidates(L, rcomm, [inner[l] & eligible[lay.rows] for l, lay in enumerate(L.layers)], np.flatnonzero(eligible))
        own = pc == rcomm[pv]
        target_ok = _mix([_term(l, rext[l][pc], gamma, rtot[l][pc], tot_c[l][pv] - rtot[l][pc], two_m) for l in range(N_LAYERS)], ratio) >= 0
        valid = own | target_ok
        g = _mix([_term(l, kvc[l], gamma, k[l][pv], rtot[l][pc] - np.where(own, k[l][pv], 0), two_m) for l in range(N_LAYERS)], ratio)
        want, kb0, _ = LO._pick(n, pv[valid], pc[valid], g[valid], kvc[0][valid], own[valid])
        _, kb1, _ = LO._pick(n, pv[valid], pc[valid], g[valid], kvc[1][valid], own[valid])
        mv = LO._movers(L, want, s)
        stats["sweeps"] += 1
        if not mv.any():
            break
        old, new = rcomm[mv], want[mv]
        rcomm[mv] = new
        np.add.at(rsize, new, 1)
        np.subtract.at(rsize, old, 1)
        for l, kb in enumerate((kb0, kb1)):
            np.add.at(rtot[l], new, k[l][mv])
            np.subtract.at(rtot[l], old, k[l][mv])
            np.add.at(rext[l], new, vext[l][mv] - 2 * kb[mv])
    return rcomm


def validate(layers: tuple) -> None:
    """The refusals of ``sqgr_leiden_multiplex`` as ``ValueError`` naming the layer."""
    n = layers[0][0].shape[0] - 1
    for l, (indptr, indices, weights) in enumerate(layers):
        if indptr.shape[0] - 1 != n:
            raise ValueError(f"layer {l}: indptr has another length")
        try:
            LO.validate(indptr, indices, weights)
        except ValueError as exc:
            raise ValueError(f"layer {l}: {exc}") from None


def leiden(layer0: tuple, layer1: tuple, resolutions: tuple = (1.0, 1.0), layer_ratio: float = 1.0, n_iterations: int = -1) -> tuple:
    """``(labels int32, stats)`` of two ``(indptr, indices, weights)`` layers over the same vertices."""
    layers = tuple(tuple(np.asarray(x, dtype=np.int64) for x in lay) for lay in (layer0, layer1))
    gamma, ratio = (float(resolutions[0]), float(resolutions[1])), float(layer_ratio)
    if not all(np.isfinite(x) and x > 0 for x in gamma + (ratio,)) or n_iterations == 0:
        raise ValueError("resolutions / layer_ratio / n_iterations")
    n = layers[0][0].shape[0] - 1
    stats = dict.fromkeys(STATS, 0)
    validate(layers)
    if layers[0][1].shape[0] + layers[1][1].shape[0] == 0:
        stats.update(n_communities=n, settled=1)
        return np.arange(n, dtype=np.int32), stats
    base = _Level2(n, [LO._Level(n, np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)), indices, weights) for indptr, indices, weights in layers])
    two_m = tuple(int(lay.k.sum()) for lay in base.layers)
    if max(two_m) >= 2**62:
        raise NotImplementedError("2m reaches 2**62")
    prev = np.arange(n, dtype=np.int32)
    for _ in range(LO.ITER_CAP if n_iterations < 0 else n_iterations):
        L, comm, node_of = base, prev.astype(np.int64), np.arange(n, dtype=np.int64)
        while True:
            stats["levels"] += 1
            comm = _local_moving(L, comm, gamma, two_m, ratio, stats)
            if np.unique(comm).shape[0] == L.n:
                break
            rcomm = _refine(L, comm, gamma, two_m, ratio, stats)
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
            coarse = []
            for lay in L.layers:  # one coarse graph per layer over the same numbering; the self loop carries in^l_c
                uniq, inv = np.unique(nr[lay.rows] * nc + nr[lay.cols], return_inverse=True)
                coarse.append(LO._Level(nc, uniq // nc, uniq % nc, LO._group_sum(inv.ravel(), lay.w, uniq.shape[0])))
            L, comm = _Level2(nc, coarse), ccomm
        labels = LO.canonical(node_of)
        stats["iterations"] += 1
        if np.array_equal(labels, prev):
            stats["settled"] = 1
            break
        prev = labels
    stats["n_communities"] = int(prev.max()) + 1
    for l, lay in enumerate(base.layers):
        stats[f"sum_in_{l}"] = int(lay.w[prev[lay.rows] == prev[lay.cols]].sum())
        stats[f"two_m_{l}"] = two_m[l]
    return prev, stats


# ---- property checkers --------------------------------------------------------------------------------------------------------------
def assert_connected_in_union(layer0: tuple, layer1: tuple, labels: np.ndarray) -> None:
    """Every community is connected in the union of the layers."""
    n = labels.shape[0]
    union = sum(sparse.csr_matrix((np.ones(lay[1].shape[0], dtype=np.int64), lay[1], lay[0]), shape=(n, n)) for lay in (layer0, layer1)).tocsr()
    union.sort_indices()
    LO.assert_connected(union.indptr, union.indices, labels)


def _layer_integers(layer: tuple, labels: np.ndarray) -> tuple:
    indptr, indices, weights = layer
    n = labels.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    w = np.asarray(weights, dtype=np.int64)
    k = LO._group_sum(rows, w, n)
    return rows, w, k, int(k.sum())


def multiplex_quality(layer0: tuple, layer1: tuple, labels: np.ndarray, resolutions: tuple, layer_ratio: float) -> Fraction:
    """``Q = sum_l a_l sum_c (in^l_c - gamma_l (tot^l_c)**2 / 2m_l)`` of any labelling, exact; a layer without weight adds 0."""
    labels = np.asarray(labels, dtype=np.int64)
    q = Fraction(0)
    for layer, gamma, a in zip((layer0, layer1), resolutions, (Fraction(1), Fraction(float(layer_ratio)))):
        rows, w, k, two_m = _layer_integers(layer, labels)
        if two_m == 0:
            continue
        tot = LO._group_sum(labels, k, int(labels.max()) + 1)
        sum_in = int(w[labels[rows] == labels[np.asarray(layer[1], dtype=np.int64)]].sum())
        q += a * (sum_in - Fraction(float(gamma)) * Fraction(LO._sum_sq(tot), two_m))
    return q


def unstable_vertices(layer0: tuple, layer1: tuple, labels: np.ndarray, resolutions: tuple, layer_ratio: float) -> list:
    """Vertices with a strictly better community among those of their neighbours in either layer, under the multiplex objective in
    exact arithmetic: ``sum_l a_l (k^l_vc - gamma_l k^l_v (tot^l_c - [c = comm(v)] k^l_v) / 2m_l)`` as integers over one common
    positive denominator."""
    labels = np.asarray(labels, dtype=np.int64)
    n = labels.shape[0]
    ints = [_layer_integers(layer, labels) for layer in (layer0, layer1)]
    v = np.r_[ints[0][0], ints[1][0], np.arange(n)]
    c = np.r_[labels[np.asarray(layer0[1], dtype=np.int64)], labels[np.asarray(layer1[1], dtype=np.int64)], labels]
    z = [np.zeros(x[1].shape[0], dtype=np.int64) for x in ints]
    zn = np.zeros(n, dtype=np.int64)
    pv, pc, kvc = _pairs2(v, c, [np.r_[ints[0][1], z[1], zn], np.r_[z[0], ints[1][1], zn]], n)
    own = pc == labels[pv]
    a = (Fraction(1), Fraction(float(layer_ratio)))
    num, den = [], []  # layer l's term is num[l] / den[l]
    for l in range(N_LAYERS):
        _, _, k, two_m = ints[l]
        if two_m == 0:
            num.append(np.zeros(pv.shape[0], dtype=object))
            den.append(1)
            continue
        gamma = Fraction(float(resolutions[l]))
        tot = LO._group_sum(labels, k, n)
        less = (tot[pc] - np.where(own, k[pv], 0)).astype(object)
        d = two_m * gamma.denominator * a[l].denominator
        num.append(a[l].numerator * (kvc[l].astype(object) * (two_m * gamma.denominator) - gamma.numerator * k[pv].astype(object) * less))
        den.append(d)
    score = num[0] * den[1] + num[1] * den[0]
    best: dict = {}
    own_score: dict = {}
    for vv, s, o in zip(pv.tolist(), score.tolist(), own.tolist()):
        if o:
            own_score[vv] = s
        if vv not in best or s > best[vv]:
            best[vv] = s
    return [vv for vv, s in best.items() if s > own_score[vv]]

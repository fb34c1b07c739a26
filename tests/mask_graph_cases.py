"""Cases for the segment-within-polygon predicate of ``mask_graph`` (pure numpy): every case is ``(name, a, b, mask)``, segments
``a[k] -> b[k]`` against a polygon of ``squidpy_amd.gr._mask``.  :func:`oracle` recomputes, from the expressions of
``gr/_mask.py`` itself, what decides the path of every segment — touched, cut, the number of cut parameters — next to the host answer."""

from __future__ import annotations

import numpy as np

from squidpy_amd.gr._mask import MultiPolygon, Polygon, _classify, _cross, _polygons, segments_within

SQUARE = [(0, 0), (4, 0), (4, 4), (0, 4)]
M_SHAPE = [(0, 0), (4, 0), (4, 8), (2, 1.5), (0, 8)]  # the reference's test polygon: concave, a notch between two arms


def _segs(pairs):
    arr = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    return arr[:, :2].copy(), arr[:, 2:].copy()


def _random_segs(rng, lo, hi, n, spread):
    a = rng.uniform(lo, hi, (n, 2))
    return a, a + rng.normal(0, spread, (n, 2))


def _regular(n_edges, radius=3.0, centre=(0.0, 0.0), phase=0.1):
    t = phase + 2 * np.pi * np.arange(n_edges) / n_edges
    return np.stack([centre[0] + radius * np.cos(t), centre[1] + radius * np.sin(t)], axis=1)


def _wobbly(n_vertices, seed):
    rng = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(n_vertices) / n_vertices
    r = 5.0 + 1.2 * np.sin(5 * t) + 0.6 * np.sin(17 * t + 1.0) + rng.uniform(-0.15, 0.15, n_vertices)
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1)


def reference_fixture():
    """Points and polygon of the reference's `sdata_mask_graph` fixture (tests/test_mask_graph_cpu.py: `_fixture`)."""
    rng = np.random.default_rng(42)
    points = np.concatenate([rng.uniform((3.2, 4.2), (3.8, 5.2), (3, 2)), rng.uniform((0.2, 4.2), (0.8, 5.2), (3, 2)),
                             rng.uniform((1, 0.5), (3, 1.5), (3, 2)), rng.uniform((1, 5), (2, 6), (3, 2))])
    return points, Polygon(M_SHAPE)


def comb(cap: int):
    """A comb whose teeth a segment along y = 2 crosses 2 * teeth - 2 times: with 0 and 1 that is more than ``cap`` cut parameters."""
    teeth = cap // 2 + 8
    # the base [0, 2 teeth - 1] x [0, 1] along the bottom to the right, then tooth i = [2i, 2i + 1] x [1, 3] by tooth back to the left
    shell = [(0.0, 0.0), (2.0 * teeth - 1.0, 0.0)]
    for i in range(teeth - 1, -1, -1):
        shell += [(2.0 * i + 1.0, 1.0), (2.0 * i + 1.0, 3.0), (2.0 * i, 3.0), (2.0 * i, 1.0)]
    return Polygon(shell), teeth


def cases(cap: int) -> list:
    out = []
    # the reference's ported case: the complete graph on its fixture's points
    pts, m_poly = reference_fixture()
    i, j = np.nonzero(~np.eye(len(pts), dtype=bool))
    out.append(("reference", pts[i], pts[j], m_poly))

    holed = Polygon(SQUARE, holes=[[(1, 1), (2, 1), (2, 2), (1, 2)]])
    rng = np.random.default_rng(7)
    out.append(("one_hole", *_random_segs(rng, (-0.5, -0.5), (4.5, 4.5), 150, 0.8), holed))

    # two overlapping holes: (5, 5) lies in both — per-ring parity says "in a hole", the total parity would say "inside"
    two = Polygon([(0, 0), (10, 0), (10, 10), (0, 10)], holes=[[(2, 2), (6, 2), (6, 6), (2, 6)], [(4, 4), (8, 4), (8, 8), (4, 8)]])
    a, b = _segs([(4.5, 4.5, 5.5, 5.5), (5, 5, 5, 5), (1, 1, 1.5, 9), (3, 3, 5, 5), (7, 7, 5, 5), (0.5, 0.5, 9.5, 0.7)])
    ra, rb = _random_segs(np.random.default_rng(8), (-1, -1), (11, 11), 120, 1.5)
    out.append(("overlapping_holes", np.vstack([a, ra]), np.vstack([b, rb]), two))

    multi = MultiPolygon([Polygon(SQUARE), Polygon([(6, 0), (10, 0), (10, 4), (6, 4)])])
    out.append(("multipolygon_span", *_segs([(1, 2, 9, 2), (1, 1, 3, 3), (7, 1, 9, 3), (4, 2, 6, 2), (5, 1, 5, 3), (3.5, 2, 4, 2), (2, 2, 6, 2)]), multi))

    sq = Polygon(SQUARE)
    out.append(("end_on_vertex", *_segs([(2, 2, 4, 4), (0, 0, 2, 1), (2, 2, 0, 4), (4, 4, 6, 6), (0, 0, 4, 4), (-1, 1, 1, -1)]), sq))
    out.append(("end_on_edge", *_segs([(2, 2, 4, 2), (2, 0, 2, 3), (0, 1, 4, 3), (4, 2, 5, 2), (2, 0, 3, 0), (2, 4, 2, 5)]), sq))
    # collinear with a ring edge: overlapping it, inside it, extending past it — on the shell and on a hole's edge inside the polygon
    out.append(("collinear", *_segs([(0, 0, 4, 0), (1, 0, 3, 0), (-1, 0, 2, 0), (2, 0, 6, 0), (-1, 0, 5, 0),
                                     (0.5, 1, 3, 1), (1, 1, 2, 1), (1.25, 1, 1.75, 1), (0.5, 1, 1.5, 1), (1.5, 2, 3.5, 2), (1, 0.5, 1, 3)]), holed))
    out.append(("zero_length", *_segs([(3, 3, 3, 3), (0.5, 0.5, 0.5, 0.5), (4, 2, 4, 2), (0, 0, 0, 0), (1.5, 1, 1.5, 1), (5, 5, 5, 5),
                                       (1.5, 1.5, 1.5, 1.5), (-1, 2, -1, 2)]), holed))
    # horizontal ring edges at a query's y: steps at y = 1, 2, 3
    steps = Polygon([(0, 0), (6, 0), (6, 1), (5, 1), (5, 2), (4, 2), (4, 3), (2, 3), (2, 2), (1, 2), (1, 1), (0, 1)])
    out.append(("horizontal_edges", *_segs([(-1, 2, 7, 2), (1.5, 2, 4.5, 2), (2.5, 2, 3.5, 2), (0.5, 1, 5.5, 1), (3, 3, 3, 1), (2, 3, 4, 3),
                                            (-1, 1, 0.5, 1), (1, 1, 1, 2), (3, 2, 3, 2), (1.5, 2, 1.5, 2), (7, 3, 8, 3), (0.5, 0.5, 5.5, 0.5)]), steps))
    out.append(("through_hole", *_segs([(0.5, 1.5, 3, 1.5), (0.5, 0.5, 2.5, 2.5), (0.5, 0.5, 3.5, 0.6), (1.2, 1.2, 1.8, 1.8)]), holed))
    out.append(("concave_reenter", *_segs([(1, 5, 3, 5), (1, 1, 3, 1), (0.5, 7, 3.5, 7), (2, 1.4, 2, 1.4), (1, 1, 2, 1.5), (0.2, 0.2, 3.8, 0.3)]), m_poly))
    for n_edges in (63, 64, 65, 257):
        rng = np.random.default_rng(100 + n_edges)
        out.append((f"ring_{n_edges}", *_random_segs(rng, (-3.5, -3.5), (3.5, 3.5), 90, 1.0), Polygon(_regular(n_edges))))
    for n_seg in (1, 63, 64, 65, 1031):
        rng = np.random.default_rng(200 + n_seg)
        a, b = _random_segs(rng, (-0.5, -0.5), (4.5, 8.5), n_seg, 0.9)
        if n_seg == 1:
            a, b = _segs([(1, 1, 3, 1)])
        out.append((f"segments_{n_seg}", a, b, m_poly))
    rng = np.random.default_rng(11)
    out.append(("wobbly_300", *_random_segs(rng, (-7, -7), (7, 7), 2000, 0.7), Polygon(_wobbly(300, 12), holes=[_regular(40, 1.5)])))
    poly, teeth = comb(cap)
    far = 2.0 * (teeth - 1) + 0.5
    out.append(("comb", *_segs([(0.5, 2, far, 2), (0.25, 2.5, far + 0.25, 1.5), (far, 2.75, 0.75, 1.25),  # cross every tooth: past the cap
                                (0.5, 2, far + 2, 2),  # an end outside: touched, not cut
                                (0.5, 0.5, far, 0.5), (0.5, 1.5, 0.5, 2.5), (0.5, 2, 2.5, 2), (0.5, 2, 4.5, 2), (1.5, 2, 1.75, 2)]), poly))
    return out


COMB_CROSSING = 3  # segments of the comb case that produce more cut parameters than the cap


def oracle(a: np.ndarray, b: np.ndarray, mask) -> dict:
    """Per segment, from gr/_mask.py's own expressions (lines 117-146): the classes of a, b and the midpoint, ``touched``, ``cut``
    (touched, neither end outside), ``n_col`` collinear ring edges, ``n_param`` cut parameters before duplicates are removed
    (0, 1, every hit, every projection in [0, 1]), ``n_unique`` after; and ``within``, the answer of the host code."""
    polys = _polygons(mask)
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    edges = np.concatenate([np.stack([r[:-1], r[1:]], axis=1) for rings in polys for r in rings])
    p, q = edges[:, 0], edges[:, 1]
    ca, cb, mid = _classify(a, polys), _classify(b, polys), _classify(0.5 * (a + b), polys)
    dx, dy = (b - a)[:, 0][:, None], (b - a)[:, 1][:, None]
    ex, ey = (q - p)[:, 0][None, :], (q - p)[:, 1][None, :]
    wx, wy = p[:, 0][None, :] - a[:, 0][:, None], p[:, 1][None, :] - a[:, 1][:, None]
    den = _cross(dx, dy, ex, ey)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = _cross(wx, wy, ex, ey) / den
        u = _cross(wx, wy, dx, dy) / den
    hit = (den != 0) & (t >= 0) & (t <= 1) & (u >= 0) & (u <= 1)
    col = (den == 0) & (_cross(wx, wy, dx, dy) == 0)
    touched = hit.any(axis=1) | col.any(axis=1)
    cut = touched & (ca != 0) & (cb != 0)
    n_param = np.zeros(len(a), dtype=np.int64)
    n_unique = np.zeros(len(a), dtype=np.int64)
    for k in np.nonzero(cut)[0]:
        ts = [0.0, 1.0] + list(t[k][hit[k]])
        d2 = float(dx[k, 0] ** 2 + dy[k, 0] ** 2)
        for r in np.nonzero(col[k])[0]:
            for pt in (p[r], q[r]):
                tt = ((pt[0] - a[k, 0]) * dx[k, 0] + (pt[1] - a[k, 1]) * dy[k, 0]) / d2 if d2 > 0 else 0.0
                if 0.0 <= tt <= 1.0 and d2 > 0:  # (a zero-length segment's projections are all the parameter 0 again)
                    ts.append(tt)
        n_param[k], n_unique[k] = len(ts), len(np.unique(ts))
    return {"ca": ca, "cb": cb, "mid": mid, "touched": touched, "cut": cut, "n_col": col.sum(axis=1), "n_param": n_param,
            "n_unique": n_unique, "within": segments_within(a, b, mask)}

"""Boundary pairs for the distance kernels, proved with exact rationals (no GPU).

Every distance decision on the device is a comparison of a rounded value with a threshold: the graph builders test the
float64 ``fl(fl(dx*dx) + fl(dy*dy)) <= fl(r*r)`` (sklearn's ``rdist <= r*r``), Ripley's euclidean counts test the same
float64 ``d2 <= t`` with ``t`` from ``_lib.sqrt_thresholds`` (``sqrt(d2) <= r``), and co-occurrence tests the float32
``d2 <= thr`` of the literal source, unfused or, with ``fma=True``, ``fmaf(dx, dx, dy*dy)``.  The helpers here build
point pairs whose computed value sits exactly on such a threshold, or on the nearest representable value either side,
at decimal-micron coordinates far from the origin; ``fractions.Fraction`` of the floats decides where each pair lies.
tests/test_distance_edges_gpu.py plants them in clouds that reach the grid and tile kernels."""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest

F = Fraction
OFFSETS = (0.0, 1e4, 1e5, 1e7)


# ----------------------------------------------------------------------------------------------------- exact rounding

def round_f32(q: Fraction) -> np.float32:
    """``q`` rounded to the nearest float32, ties to even (IEEE round-to-nearest), subnormals and overflow included."""
    if q == 0:
        return np.float32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < F(2) ** e:
        e -= 1
    e = max(e, -126)                              # below 2**-126 the float32 grid is the subnormal one, 2**-149
    scale = F(2) ** (e - 23)
    m = a / scale
    n = m.numerator // m.denominator
    rem = m - n
    if rem > F(1, 2) or (rem == F(1, 2) and n % 2):
        n += 1
    v = n * scale
    if v >= F(2) ** 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * float(v))           # (v is a float32: float() and the cast are exact)


def round_f64(q: Fraction) -> float:
    """``q`` rounded to the nearest float64 (CPython's int / int true division is correctly rounded)."""
    return float(q)


def d2_f64_exact(dx: float, dy: float) -> float:
    """The graph builders' and sklearn's float64 ``fl(fl(dx*dx) + fl(dy*dy))`` (never fused), from rationals."""
    return round_f64(F(round_f64(F(float(dx)) ** 2)) + F(round_f64(F(float(dy)) ** 2)))


def d2_f32_exact(dx: np.float32, dy: np.float32, fma: bool) -> np.float32:
    """co-occurrence's float32 d2 from rationals: ``fl(fl(dx*dx) + fl(dy*dy))`` or ``fl(dx*dx + fl(dy*dy))`` (fmaf)."""
    yy = F(float(round_f32(F(float(dy)) ** 2)))
    xx = F(float(dx)) ** 2
    return round_f32(xx + yy) if fma else round_f32(F(float(round_f32(xx))) + yy)


def d2_f32_fma(dx: np.ndarray, dy: np.ndarray) -> np.ndarray:
    """``fmaf(dx, dx, fl(dy*dy))`` elementwise, exactly, with numpy: dx*dx is exact in float64 (48 bits); the float64 sum
    s of it and fl32(dy*dy) carries an error e that TwoSum recovers exactly; rounding s to float32 is the correctly rounded
    result unless s is exactly a float32 midpoint, where the sign of e decides (the double-rounding case)."""
    dx = np.asarray(dx, np.float32).astype(np.float64)
    dy = np.asarray(dy, np.float32)
    a = dx * dx
    b = (dy * dy).astype(np.float64)
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf))).astype(np.float32)
    mid = (r64 + other.astype(np.float64)) * 0.5   # (two adjacent float32 and their midpoint are float64 numbers)
    tie = (s != r64) & (s == mid) & (e != 0)
    toward_other = tie & (np.sign(e) == np.sign(other.astype(np.float64) - r64))
    return np.where(toward_other, other, r).astype(np.float32)


def occur_count_fma(x: np.ndarray, y: np.ndarray, thresholds: np.ndarray, labs: np.ndarray, k: int, chunk: int = 512) -> np.ndarray:
    """``oracle.restate.occur_count`` with the fused d2 of ``cooccur_counts(..., fma=True)``; int64 (k, k, L)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    thr = np.asarray(thresholds, np.float32)
    labs = np.asarray(labs).astype(np.int64)
    n, L = len(x), len(thr)
    out = np.zeros((k * k, L), dtype=np.int64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        d2 = d2_f32_fma(x[s:e, None] - x[None, :], y[s:e, None] - y[None, :])
        pair = labs[s:e, None] * k + labs[None, :]
        notself = np.arange(s, e)[:, None] != np.arange(n)[None, :]
        pf, d2f = pair[notself], d2[notself]
        for r in range(L):
            out[:, r] += np.bincount(pf[d2f <= thr[r]], minlength=k * k)
    return out.reshape(k, k, L)


def sqrt_thresholds(r):
    from squidpy_amd import _lib

    return _lib.sqrt_thresholds(np.atleast_1d(np.asarray(r, np.float64)))


# ----------------------------------------------------------------------------------------------- boundary constructors

def _d2(kind: str, c, p) -> float:
    if kind == "cooc32":
        return d2_f32_exact(np.float32(c[0] - p[0]), np.float32(c[1] - p[1]), False)
    return d2_f64_exact(float(c[0] - p[0]), float(c[1] - p[1]))


def _threshold(kind: str, d2):
    """(threshold the device compares with, radius the caller passes) that puts a pair of computed ``d2`` exactly on the
    boundary, or None when no radius does: radius64 fl(r*r) == d2; ripley64 sqrt_thresholds(r) == d2; cooc32 the float32
    fl(r*r) == d2 (co_occurrence squares its float32 interval)."""
    if kind == "cooc32":
        r0 = np.float32(np.sqrt(np.float64(d2)))
        for r in (r0, np.nextafter(r0, np.float32(-np.inf)), np.nextafter(r0, np.float32(np.inf))):
            if np.float32(r * r) == d2:
                return d2, r
        return None
    r0 = float(np.sqrt(d2))
    if kind == "ripley64":
        return (d2, r0) if sqrt_thresholds(r0)[0] == d2 else None
    for r in (r0, math.nextafter(r0, -math.inf), math.nextafter(r0, math.inf)):
        if round_f64(F(float(r)) ** 2) == d2:
            return d2, r
    return None


def boundary_pair(kind: str, c, radius: float, theta: float, max_steps: int = 400) -> dict:
    """A neighbour ``p`` of centre ``c`` near ``c + radius * (cos theta, sin theta)`` (a decimal rounded to 1e-4) whose
    computed d2 IS the threshold of radius ``r`` (see ``_threshold``), plus ``inside`` / ``outside``: the same point moved
    along its longer axis to the nearest representable coordinate whose d2 is below / above the threshold.
    kind: "radius64" | "ripley64" (float64 coordinates) | "cooc32" (float32 coordinates)."""
    dt = np.float32 if kind == "cooc32" else np.float64
    c = (dt(c[0]), dt(c[1]))
    p0 = [dt(round(float(c[0]) + radius * math.cos(theta), 4)), dt(round(float(c[1]) + radius * math.sin(theta), 4))]
    ax = 0 if abs(math.cos(theta)) >= abs(math.sin(theta)) else 1
    away = dt(np.inf) if p0[ax] >= c[ax] else dt(-np.inf)
    toward = -away
    p = list(p0)
    for step in range(max_steps):
        p[ax] = p0[ax]
        for _ in range((step + 1) // 2):
            p[ax] = np.nextafter(p[ax], away if step % 2 else toward)
        d2 = _d2(kind, c, p)
        tr = _threshold(kind, d2)
        if tr is None:
            continue
        thr, r = tr
        out = {"kind": kind, "c": c, "p": tuple(p), "thr": thr, "r": r}
        for name, direction, want in (("inside", toward, -1), ("outside", away, 1)):
            q = list(p)
            while True:
                q[ax] = np.nextafter(q[ax], direction)
                dq = _d2(kind, c, q)
                if dq != thr:
                    break
            assert (dq > thr) == (want > 0)
            out[name] = tuple(q)
        return out
    raise AssertionError(f"no boundary pair for {kind} at {c}, radius {radius}, theta {theta}")


def fma_split_pairs(c, radius: float, n_want: int = 4, span: int = 600) -> list[dict]:
    """float32 neighbours ``p`` of ``c`` near distance ``radius`` for which ``fmaf(dx, dx, dy*dy)`` and the unfused
    ``fl(fl(dx*dx) + fl(dy*dy))`` differ, each with a float32 threshold between them (the smaller of the two): the unfused
    count and the fused count of the pair then disagree.  Empty when the float32 grid at ``c`` rounds no such d2."""
    c = (np.float32(c[0]), np.float32(c[1]))
    out = []
    for j in range(span):
        theta = 0.3 + 1.1 * j / span
        p = (np.float32(c[0] + np.float32(radius * math.cos(theta))), np.float32(c[1] + np.float32(radius * math.sin(theta))))
        dx, dy = np.float32(c[0] - p[0]), np.float32(c[1] - p[1])
        a, b = d2_f32_exact(dx, dy, False), d2_f32_exact(dx, dy, True)
        if a != b:
            out.append({"c": c, "p": p, "thr": min(a, b), "unfused": a, "fused": b})
            if len(out) >= n_want:
                break
    return out


def decimal_point(rng: np.random.Generator, offset: float, spread: float = 500.0) -> tuple[float, float]:
    """A decimal-micron coordinate pair (4 decimals: not representable in binary) around (offset, -offset)."""
    return (round(offset + rng.random() * spread, 4), round(-offset - rng.random() * spread, 4))


# --------------------------------------------------------------------------------------------------------------- tests

def test_round_f32_is_ieee_round_to_nearest():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(2000).astype(np.float32) * np.float32(1e3)
    b = rng.standard_normal(2000).astype(np.float32)
    for u, v in zip(a, b):                     # float32 products and sums of numpy are correctly rounded
        assert round_f32(F(float(u)) * F(float(v))) == u * v
        assert round_f32(F(float(u)) + F(float(v))) == u + v
    one = F(1)
    assert round_f32(one + F(1, 2 ** 24)) == np.float32(1.0)                       # tie -> even
    assert round_f32(one + F(3, 2 ** 24)) == np.float32(1.0 + 2 ** -22)            # tie -> even, upward
    assert round_f32(one + F(1, 2 ** 24) + F(1, 2 ** 80)) == np.float32(1.0 + 2 ** -23)
    assert round_f32(F(1, 2 ** 149)) == np.float32(2.0 ** -149)                   # subnormals
    assert round_f32(F(1, 2 ** 150)) == np.float32(0.0)
    assert round_f32(F(3, 2 ** 151)) == np.float32(2.0 ** -149)
    assert round_f32(F(2) ** 128) == np.float32(np.inf)
    assert round_f32(-F(5, 3)) == np.float32(-5.0 / 3.0)


def test_unfused_emulation_is_numpy_float32_and_float64():
    rng = np.random.default_rng(1)
    for off in OFFSETS:
        x = (off + rng.random(300) * 200).astype(np.float32)
        y = (-off - rng.random(300) * 200).astype(np.float32)
        dx, dy = x[:-1] - x[1:], y[:-1] - y[1:]
        np.testing.assert_array_equal([d2_f32_exact(u, v, False) for u, v in zip(dx, dy)], dx * dx + dy * dy)
        x64, y64 = np.round(off + rng.random(300) * 200, 4), np.round(-off - rng.random(300) * 200, 4)
        dx64, dy64 = x64[:-1] - x64[1:], y64[:-1] - y64[1:]
        np.testing.assert_array_equal([d2_f64_exact(u, v) for u, v in zip(dx64, dy64)], dx64 * dx64 + dy64 * dy64)


def test_vectorised_fma_emulation_is_exact():
    """d2_f32_fma (numpy, used for whole clouds) == the rational fmaf, on random pairs at every offset, on pairs that
    straddle a float32 midpoint in float64 (the double-rounding case) and on the constructed split pairs."""
    rng = np.random.default_rng(2)
    dx, dy = [], []
    for off in OFFSETS:
        for scale in (1.0, 30.0, 700.0):
            x = (off + rng.random(400) * scale).astype(np.float32)
            y = (off + rng.random(400) * scale).astype(np.float32)
            dx.append(x[:-1] - x[1:]); dy.append(y[:-1] - y[1:])
    # 4097**2 = 2**24 + 8193 is a float32 midpoint: a tiny dy*dy is lost in the float64 sum but decides the fused rounding
    dx.append(np.array([4097.0, 4097.0, 4097.0, 1.0 + 2.0 ** -23], np.float32))
    dy.append(np.array([2.0 ** -20, 0.0, 2.0 ** -14, 2.0 ** -30], np.float32))
    dx, dy = np.concatenate(dx), np.concatenate(dy)
    want = np.array([d2_f32_exact(u, v, True) for u, v in zip(dx, dy)], np.float32)
    np.testing.assert_array_equal(d2_f32_fma(dx, dy), want)
    assert d2_f32_exact(np.float32(4097.0), np.float32(2.0 ** -20), True) == np.float32(16785410.0)  # (not the tie's 16785408)
    assert d2_f32_exact(np.float32(4097.0), np.float32(0.0), True) == np.float32(16785408.0)
    c = (np.float32(10000.1234), np.float32(-10000.5678))
    for s in fma_split_pairs(c, 37.3):
        dxs, dys = np.float32(s["c"][0] - s["p"][0]), np.float32(s["c"][1] - s["p"][1])
        assert d2_f32_fma(np.array([dxs]), np.array([dys]))[0] == s["fused"]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("kind", ["radius64", "ripley64", "cooc32"])
def test_boundary_pairs_lie_where_they_claim(kind, offset):
    """Each constructed pair's d2 IS the threshold the device compares with (counted: d2 <= thr), and its inside /
    outside twins are the nearest representable points on either side — decided with rationals, at decimal coordinates."""
    rng = np.random.default_rng(int(offset) % 9973 + len(kind))
    for j in range(6):
        c = decimal_point(rng, offset)
        radius = [0.7, 3.3, 12.3, 47.9, 150.1, 911.7][j]
        bp = boundary_pair(kind, c, radius, theta=0.4 + 0.9 * j)
        thr, (cx, cy) = bp["thr"], bp["c"]
        for name, rel in (("p", 0), ("inside", -1), ("outside", 1)):
            px, py = bp[name]
            if kind == "cooc32":
                exact = d2_f32_exact(np.float32(cx - px), np.float32(cy - py), False)
                assert exact == np.float32(px - cx) * np.float32(px - cx) + np.float32(py - cy) * np.float32(py - cy)
            else:
                exact = d2_f64_exact(float(cx - px), float(cy - py))
                assert exact == (px - cx) * (px - cx) + (py - cy) * (py - cy)
            assert np.sign(F(float(exact)) - F(float(thr))) == rel, (name, exact, thr)
        r = bp["r"]
        if kind == "radius64":
            assert round_f64(F(float(r)) ** 2) == thr                   # fl(r*r): sklearn's rdist bound and radius_self's r2
        elif kind == "ripley64":
            assert sqrt_thresholds(r)[0] == thr
            assert F(float(np.sqrt(thr))) <= F(float(r)) < F(float(np.sqrt(bp_next(float(thr)))))
        else:
            assert np.float32(r) * np.float32(r) == thr              # co_occurrence's (interval ** 2) in float32
        assert abs(float(bp["p"][0]) - float(cx)) > 0 or abs(float(bp["p"][1]) - float(cy)) > 0


def bp_next(t: float) -> float:
    return math.nextafter(t, math.inf)


@pytest.mark.parametrize("offset", [0.0, 1e4, 1e5])
def test_fma_split_pairs_straddle_their_threshold(offset):
    """Pairs where the fused and unfused float32 d2 fall on different sides of a float32 threshold exist at decimal
    coordinates (they need a rounded dx*dx: |c| / ulp large enough) and are proved with rationals."""
    rng = np.random.default_rng(7)
    c = decimal_point(rng, offset)
    found = 0
    for radius in (9.1, 37.3, 123.4):
        for s in fma_split_pairs(c, radius):
            dx = np.float32(s["c"][0] - s["p"][0])
            dy = np.float32(s["c"][1] - s["p"][1])
            a, b = F(float(d2_f32_exact(dx, dy, False))), F(float(d2_f32_exact(dx, dy, True)))
            t = F(float(s["thr"]))
            assert a != b and min(a, b) == t and max(a, b) > t                       # one counts, the other does not
            assert d2_f32_exact(dx, dy, False) == dx * dx + dy * dy                  # the unfused side is numpy's
            found += 1
    assert found >= 6


def test_fma_split_pairs_at_1e7_need_a_long_radius():
    """At |x| ~ 1e7 the float32 grid is the integers: every d2 below 2**24 is exact, fused or not; past it they split."""
    c = (np.float32(1e7 + 0.3), np.float32(-1e7 - 0.7))
    assert fma_split_pairs(c, 150.0) == []
    assert len(fma_split_pairs(c, 5000.0)) >= 2


@pytest.mark.parametrize("seed", range(3))
def test_sqrt_thresholds_are_the_largest_square_below_each_radius(seed):
    """t = sqrt_thresholds(r): sqrt(t) <= r < sqrt(nextafter(t, inf)), i.e. `sqrt(d2) <= r` <=> `d2 <= t` for every float
    d2 — on random radii, perfect squares, 0, subnormals and huge values."""
    rng = np.random.default_rng(seed)
    r = np.concatenate([
        rng.random(500) * 1000, rng.random(200) * 1e-3, np.exp(rng.uniform(-300, 300, 300)),
        np.arange(0.0, 200.0), np.sqrt(np.arange(1.0, 500.0)), np.round(rng.random(200) * 1e5, 4),
        [0.0, 5e-324, 1e-320, 2.2250738585072014e-308, 1e-160, 1.3407807929942596e154, 1e154, 1e300, np.finfo(np.float64).max],
    ])
    t = sqrt_thresholds(r)
    assert np.all(np.sqrt(t) <= r)
    with np.errstate(over="ignore"):
        up = np.nextafter(t, np.inf)
    assert np.all((np.sqrt(up) > r) | ~np.isfinite(up))
    # the same as rationals where the square is representable: t == fl(r*r) shifted by a few ulps at most
    for rr, tt in zip(r[:50], t[:50]):
        assert F(float(np.sqrt(tt))) <= F(float(rr))
    assert np.all(sqrt_thresholds(np.array([-1.0, -0.0])) == np.array([-1.0, 0.0]))

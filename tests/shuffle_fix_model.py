"""Numpy model of the label shuffle's FIX pair (squidpy_amd/csrc/sqgr_shuffle.hip: k_shuffle_tab<.., FIX = true> + k_shuffle_fix) on
the functions of oracle/devrng.py: the inverse rounds (sqgr_rng.h), the block table of the label-sorted base and its eligibility
(LabelShuffler::create), the patched entries, and one k_shuffle_fix thread per (permutation, out-of-range rank)."""

from __future__ import annotations

import numpy as np

from oracle import devrng

U = np.uint64


def bits(n: int) -> tuple[int, int, int, int, int]:
    """(A, B, Bmask, bits of the high digit's round function, bits of the low digit's)."""
    A, B, Bmask = devrng.domain_dims(n)
    return A, B, Bmask, A.bit_length() - 1, (Bmask + 1).bit_length() - 1


def unadd_b(b, a, k, n: int):
    """b <- (b - F_B(a, k)) mod B: F_B <= Bmask < 2B, reduced by one conditional subtraction first (sqgr_rng.h: feistel_unadd_b)."""
    _, B, _, _, bb = bits(n)
    f = devrng._F(a, k, bb)
    f = np.where(f >= U(B), f - U(B), f)
    return np.where(b >= f, b - f, b + U(B) - f)


def sigma_inverse(a, b, sk, n: int):
    """sigma_p backwards (sqgr_rng.h: sigma_inverse).  ``sk``: (P, 2) keys, ``a``, ``b``: (P, m) uint64."""
    A, _, _, ab, _ = bits(n)
    sk = sk.astype(U) & devrng.MASK16
    a = (a - devrng._F(b, sk[:, 1:2], ab)) & U(A - 1)
    return a, unadd_b(b, a, sk[:, 0:1], n)


def rounds_inverse(a, b, gk, n: int):
    """One pass of the eight rounds backwards (sqgr_rng.h: feistel_rounds_inverse).  ``gk``: (P, 8) keys."""
    A, _, _, ab, _ = bits(n)
    gk = gk.astype(U) & devrng.MASK16
    for r in range(devrng.N_ROUNDS - 2, -1, -2):
        b = unadd_b(b, a, gk[:, r + 1 : r + 2], n)
        a = (a - devrng._F(b, gk[:, r : r + 1], ab)) & U(A - 1)
    return a, b


def boundaries(labels: np.ndarray, K: int) -> np.ndarray:
    """cum[k] = number of labels < k for k < K, cum[K] = UINT_MAX (LabelShuffler::create)."""
    cum = np.zeros(K + 1, dtype=np.int64)
    cum[1:] = np.cumsum(np.bincount(labels, minlength=K))
    cum[K] = 0xFFFFFFFF
    return cum


def block_table(cum: np.ndarray, n: int, K: int) -> np.ndarray:
    """One word per high digit a: label of rank a*B | low digit where the next label starts << 16 (0xFFFF: none); lab0 = K marks
    blocks the two-field form cannot describe and blocks behind the last rank (LabelShuffler::create)."""
    A, B, _ = devrng.domain_dims(n)
    sent = K | (0xFFFF << 16)
    blk = np.zeros(A, dtype=np.int64)
    lab = 0
    for a in range(A):
        lo, hi = a * B, a * B + B
        if lo >= n:
            blk[a] = sent
            continue
        while lab + 1 < K and cum[lab + 1] <= lo:
            lab += 1
        end = min(hi, n)
        events, ev_label, ev_pos = 0, 0, 0
        for k2 in range(lab + 1, K):
            if cum[k2] >= end:
                break
            nxt = cum[k2 + 1] if k2 + 1 < K else n
            if cum[k2] >= nxt:
                continue
            if events == 0:
                ev_label, ev_pos = k2, int(cum[k2]) - lo
            events += 1
        if hi > n:
            if events == 0:
                ev_label, ev_pos = K, n - lo
            events += 1
        if events == 0:
            blk[a] = lab | (0xFFFF << 16)
        elif events == 1 and ev_label == lab + 1 and ev_pos > 0:
            blk[a] = lab | (ev_pos << 16)
        else:
            blk[a] = sent | (lab << 8 if K <= 255 else 0)
    return blk


def refusal(blk: np.ndarray, n: int, K: int) -> str | None:
    """Why these tables keep the sentinel test (None: eligible) — the table part of the rule; the launch adds: the table kernel
    takes it, no spot map, no libraries."""
    if K > 126:
        return "more than 126 clusters"
    A, B, _ = devrng.domain_dims(n)
    past = n // B
    for a in range(min(past, A)):
        if int(blk[a]) & 0xFF == K:  # byte 0: byte 1 of such a word holds the block's first label
            return "lab0 = K"
    tail = n - past * B
    if tail > 0 and int(blk[past]) != ((K - 1) | (tail << 16)):
        return "does not end in label K - 1"
    return None


def patched(blk: np.ndarray, n: int, K: int) -> np.ndarray:
    """The table as the FIX kernel holds it in LDS: the entries of every block that reaches past rank n read K - 1, no next label."""
    _, B, _ = devrng.domain_dims(n)
    out = blk.copy()
    out[n // B :] = (K - 1) | (0xFFFF << 16)
    return out


def table_label(blk: np.ndarray, x: np.ndarray, n: int) -> np.ndarray:
    """lab0 + (b >= next) for ranks x of the whole domain A*B (put_label)."""
    _, B, _ = devrng.domain_dims(n)
    e = blk[x // B]
    return (e & 0xFF) + ((x % B) >= (e >> 16))


def first_sigma_images(n: int, seed: int, perms: np.ndarray) -> np.ndarray:
    """(P, n) first image sigma_p(pi_g(rank)) in A*B, before sigma's cycle walk — from the oracle's forward functions."""
    A, B, Bmask = devrng.domain_dims(n)
    perms = np.asarray(perms, dtype=np.int64)
    gk = devrng.group_keys(seed, perms // devrng.FEISTEL_GROUP).astype(U) & devrng.MASK16
    sk = devrng.sigma_keys(seed, perms).astype(U) & devrng.MASK16
    key = lambda r: gk[:, r : r + 1]  # noqa: E731
    x = np.tile(np.arange(n, dtype=U), (len(perms), 1))
    a, b = devrng._rounds(x // U(B), x % U(B), A, B, Bmask, key)
    bad = a * U(B) + b >= U(n)
    while bad.any():
        a2, b2 = devrng._rounds(a, b, A, B, Bmask, key)
        a, b = np.where(bad, a2, a), np.where(bad, b2, b)
        bad = a * U(B) + b >= U(n)
    a, b = devrng._sigma(a, b, A, B, Bmask, sk)
    return (a * U(B) + b).astype(np.int64)


def fix_threads(n: int, seed: int, perms: np.ndarray, cum: np.ndarray, K: int) -> list[tuple[int, int, int]]:
    """Every k_shuffle_fix thread (permutation index p into ``perms``, e < E) that stores: [(p, spot, label)], steps 1-6."""
    A, B, Bmask = devrng.domain_dims(n)
    E = A * B - n
    if E == 0:
        return []
    perms = np.asarray(perms, dtype=np.int64)
    gk = devrng.group_keys(seed, perms // devrng.FEISTEL_GROUP)
    sk = devrng.sigma_keys(seed, perms)
    sk64 = sk.astype(U) & devrng.MASK16
    y = np.tile(np.arange(n, n + E, dtype=U), (len(perms), 1))                  # 1
    ya, yb = y // U(B), y % U(B)
    a, b = sigma_inverse(ya, yb, sk, n)                                        # 2
    keep = a * U(B) + b < U(n)                                                 # 3
    bad = keep.copy()                                                          # 4: at least one pass, then while outside [0, n)
    while bad.any():
        a2, b2 = rounds_inverse(a, b, gk, n)
        a, b = np.where(bad, a2, a), np.where(bad, b2, b)
        bad = keep & (a * U(B) + b >= U(n))
    spot = a * U(B) + b
    za, zb = ya, yb                                                            # 5
    bad = keep.copy()
    while bad.any():
        a2, b2 = devrng._sigma(za, zb, A, B, Bmask, sk64)
        za, zb = np.where(bad, a2, za), np.where(bad, b2, zb)
        bad = keep & (za * U(B) + zb >= U(n))
    z = (za * U(B) + zb).astype(np.int64)
    label = np.searchsorted(cum[1 : K + 1], z, side="right")                   # the first l with z < cum[l + 1]
    p_idx, e_idx = np.nonzero(keep)
    return [(int(p), int(spot[p, e]), int(label[p, e])) for p, e in zip(p_idx, e_idx)]  # 6


def slab_offset(n: int, i: int, pw: int, j: int) -> int:
    """Byte of label j < 16 of spot i in a batch's 16 n bytes at plane width pw (sqgr_shuffle.h: slab_label_offset)."""
    return (j // pw) * n * pw + i * pw + j % pw

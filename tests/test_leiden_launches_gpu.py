"""GPU: the launch structure of ``sqgr_leiden`` and ``sqgr_leiden_multiplex``, pinned to the stats the numpy restatements pin.

Both entry points run one host driver (``csrc/sqgr_leiden_driver.h``).  The labels can survive a driver that launches a kernel twice
or not at all (a second ``k_tot`` over a zeroed ``tot`` gives the same ``tot``), so these tests count the timed launches of one call
and compare them with ``levels``, ``sweeps`` and ``cap_hits`` of that call.  The identities are read off the driver as it stood
before the two entry points shared it; per level it launches, per layer: ``rows``, ``tot`` and ``sumsq`` once, ``sumsq`` again after
every local-moving sweep, ``tot`` again when local moving hits the sweep cap, ``refine_init`` with every renumbering, and a sort and a
reduce for every coarse CSR that has entries.  ``rows`` runs once more per call, before the input check.

Cases: ``ring_cliques`` / ``ring_pair`` (on-chip tables only), ``capacity_rows`` / ``capacity_split`` (rows on both sides of the
capacity), ``star5000`` / ``star_lattice`` (the global-memory tables), ``layer1_only`` (rows that are empty in one layer) and
``ring_empty`` (a layer without entries: its input check is not launched)."""

from __future__ import annotations

import pytest

from squidpy_amd import _lib
from squidpy_amd._lib import default_context

from tests import niche_leiden_cases as LC
from tests import niche_spatialleiden_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return default_context(None)


def _timed(ctx, call):
    """``(stats, {timer name: launches})`` of one call; only the timers that ran."""
    ctx.timer_enable(True)
    try:
        ctx.timer_reset()
        _, stats = call()
        report = ctx.timer_report()
    finally:
        ctx.timer_enable(False)
    return stats, {name: count for name, (count, _) in report.items() if count}


def _check_shared(counts, stats, p, layers):
    """The identities that hold for ``layers`` layers; ``p`` is the timer prefix."""
    L, S, H = stats["levels"], stats["sweeps"], stats["cap_hits"]

    def c(name):
        return counts.get(p + name, 0)

    print({"levels": L, "sweeps": S, "cap_hits": H}, {k: v for k, v in sorted(counts.items()) if "leiden_" in k})
    assert L >= 1 and S >= L
    assert c("move_best") + c("refine_best") == S
    assert c("move_apply") == c("move_best")
    assert c("refine_apply") == c("refine_best")
    assert c("rows") == layers * (L + 1)
    assert c("tot") == layers * (L + H)
    assert c("sumsq") == layers * (L + c("move_best"))
    assert c("refine_init") == layers * c("renumber")
    assert c("sort") == c("reduce") <= layers * c("renumber")
    assert c("move_best_long") <= c("move_best") and c("refine_best_long") <= c("refine_best")
    return c


@pytest.mark.parametrize("name", ["ring_cliques", "capacity_rows", "star5000"])
def test_one_layer_launches_follow_the_stats(ctx, name):
    graph = LC.graph(name)
    stats, counts = _timed(ctx, lambda: _lib.leiden(ctx, *graph, 1.0, -1))
    assert stats == LC.expected(name, 1.0)[1]
    c = _check_shared(counts, stats, "leiden_", 1)
    assert c("check") == 1
    if name == "ring_cliques":
        assert c("move_best_long") == c("refine_best_long") == 0
    if name == "star5000":
        assert 1 <= c("move_best_long") <= c("move_best")
    assert not [k for k in counts if k.startswith("mleiden_")]


@pytest.mark.parametrize("name", ["ring_pair", "capacity_split", "star_lattice", "layer1_only", "ring_empty"])
def test_two_layer_launches_follow_the_stats(ctx, name):
    layers = MC.layers(name)
    stats, counts = _timed(ctx, lambda: _lib.leiden_multiplex(ctx, *layers, (1.0, 1.0), 1.0, -1))
    assert stats == MC.expected(name, (1.0, 1.0), 1.0)[1]
    c = _check_shared(counts, stats, "mleiden_", 2)
    non_empty = sum(1 for layer in layers if layer[1].shape[0])
    assert non_empty == (1 if name == "ring_empty" else 2)
    assert c("check") == non_empty
    if name == "ring_pair":
        assert c("move_best_long") == c("refine_best_long") == 0
    if name == "star_lattice":
        assert c("move_best_long") >= 1
    assert not [k for k in counts if k.startswith("leiden_")]

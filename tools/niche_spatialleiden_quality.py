"""The multiplex objective of the two-layer Leiden contract against single-layer Leiden on either layer alone, on the host: for
``lattice900`` and ``knn_blobs6_spatial`` of tests/niche_spatialleiden_cases.py, every resolution pair and layer ratio 1 and 3, the
exact multiplex ``Q`` (tests/niche_spatialleiden_oracle.py: ``multiplex_quality``) of the labels of the multiplex restatement — what
the device returns bit for bit — and of the labels the single-layer restatement finds on layer 0 alone and on layer 1 alone (each on
that layer of the commonly quantised pair, at that layer's resolution).  A clusterer that ignores a layer should not beat one that sees
both: the condition is ``Q_multiplex >= max(Q_layer0_only, Q_layer1_only)`` with zero margin.
Writes profiles/niche_spatialleiden_quality.json.  Needs no device.

Usage: python tools/niche_spatialleiden_quality.py"""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import niche_leiden_oracle as LO  # noqa: E402
from tests import niche_spatialleiden_cases as MC  # noqa: E402
from tests import niche_spatialleiden_oracle as MO  # noqa: E402

RATIOS = (1.0, 3.0)


def row(name: str, resolutions: tuple, ratio: float) -> dict:
    layers = MC.layers(name)
    labels, stats = MC.expected(name, resolutions, ratio)
    q = {"multiplex": MO.multiplex_quality(*layers, labels, resolutions, ratio)}
    for l in range(2):
        alone = LO.leiden(*layers[l], resolutions[l])[0]
        q[f"layer{l}_only"] = MO.multiplex_quality(*layers, alone, resolutions, ratio)
    return {"case": name, "resolutions": list(resolutions), "layer_ratio": ratio, "q": {k: float(v) for k, v in q.items()},
            "ok": bool(q["multiplex"] >= max(q["layer0_only"], q["layer1_only"])), "n_communities": stats["n_communities"],
            "sweeps": stats["sweeps"], "cap_hits": stats["cap_hits"]}


def main() -> None:
    rows = []
    for name in MC.QUALITY_CASES:
        for resolutions in MC.RESOLUTIONS:
            for ratio in RATIOS:
                rows.append(row(name, resolutions, ratio))
                r = rows[-1]
                print(f"{name:20s} gamma={resolutions} ratio={ratio:<4} multiplex {r['q']['multiplex']:.6e}  layer 0 only {r['q']['layer0_only']:.6e}  "
                      f"layer 1 only {r['q']['layer1_only']:.6e}  {'ok' if r['ok'] else 'BELOW'}", flush=True)
    with open(os.path.join(ROOT, "profiles", "niche_spatialleiden_quality.json"), "w") as fh:
        json.dump({"condition": "q.multiplex >= max(q.layer0_only, q.layer1_only), exact rational comparison, zero margin", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

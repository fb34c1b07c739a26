"""Quality of the Leiden contract against networkx's Louvain, on the host: for every case of tests/niche_leiden_cases.py and every
resolution, Q of the numpy restatement (tests/niche_leiden_oracle.py, what the device returns bit for bit) and Q of
``networkx.community.louvain_communities`` at seeds 0-4 on the same quantised graph, both from ``niche_leiden_oracle.quality``.
Writes profiles/niche_leiden_quality.json.  Needs no device.

Usage: python tools/niche_leiden_quality.py"""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import niche_leiden_cases as LC  # noqa: E402
from tests import niche_leiden_oracle as LO  # noqa: E402

SEEDS = (0, 1, 2, 3, 4)


def main() -> None:
    rows = []
    for name in LC.NETWORKX_CASES:
        for resolution in LC.PLANTED_RESOLUTIONS if name in LC.PLANTED else LC.RESOLUTIONS:
            labels, stats = LC.expected(name, resolution)
            ours = LO.quality(*LC.graph(name), labels, resolution)
            theirs = LO.louvain_qualities(*LC.graph(name), resolution, SEEDS)
            bound = min(theirs) - (max(theirs) - min(theirs))
            rows.append({"case": name, "resolution": resolution, "q_ours": ours, "q_networkx": theirs, "bound": bound, "ok": ours >= bound,
                         "n_communities": stats["n_communities"], "sweeps": stats["sweeps"], "cap_hits": stats["cap_hits"]})
            print(f"{name:18s} gamma={resolution:<5} ours {ours:.6f}  networkx {min(theirs):.6f} .. {max(theirs):.6f}  {'ok' if ours >= bound else 'BELOW'}",
                  flush=True)
    with open(os.path.join(ROOT, "profiles", "niche_leiden_quality.json"), "w") as fh:
        json.dump({"seeds": list(SEEDS), "condition": "q_ours >= min(q_networkx) - (max(q_networkx) - min(q_networkx))", "rows": rows}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""Developer tool (GPU box): the LDS-bucketed dot at config 3's shape, 1000 permutations.
`--one`: one timing of both statistics under the environment given (tools/joint_order.sh and tools/pmc_order.sh drive it for the
list schedules)."""
import os, sys, json
if len(sys.argv) > 1 and sys.argv[1] == "--one":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    from sklearn.preprocessing import normalize
    from squidpy_amd import _lib as L
    from squidpy_amd._synthetic import hex_grid_graph
    ctx = L.default_context()
    rows, cols, G, P = int(os.environ.get("EXP_ROWS", 250)), int(os.environ.get("EXP_COLS", 400)), 2048, int(os.environ.get("EXP_PERMS", 1000))
    n = rows * cols
    g = normalize(hex_grid_graph(rows, cols), norm="l1", axis=1)
    vals = np.random.default_rng(11).gamma(2.0, 1.0, size=(G, n))
    graph = L.Graph(ctx, g, with_data=True)
    plan = L.AutocorrPlan(ctx, graph, vals)
    out = {}
    for mode in ("moran", "geary"):
        plan.perms(mode, seed=1, perm_begin=0, perm_end=P)
        ctx.sync(); ctx.timer_enable(True); ctx.timer_reset()
        for i in range(3):
            plan.perms(mode, seed=2 + i, perm_begin=0, perm_end=P)
        ctx.sync()
        rep = ctx.timer_report(); ctx.timer_enable(False)
        out[mode] = {k: round(v[1] / 3, 2) for k, v in rep.items() if v[0]}
    print(json.dumps(out))
    sys.exit(0)
sys.exit("usage: python tools/autocorr_order_exp.py --one")

"""Worker of tests/test_sepal_dist_gpu.py: TWO ranks sharing one GPU (gloo collectives).  ``sq.gr.sepal`` splits the genes across
the ranks and all-reduces the stop sweeps: both ranks must return the frame a single process returns."""
import os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch.distributed as dist

    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    import pandas as pd
    import squidpy_amd as sq
    from squidpy_amd import AnnDataLite, _dist
    from tests import sepal_oracle as SO

    assert _dist.is_distributed() and _dist.world() == (rank, 2)
    xy, g = SO.hex_grid(16, 18)
    X = SO.mixed_genes(xy, 7, seed=21)
    ad = AnnDataLite(X=X, var=pd.DataFrame(index=[f"g{j}" for j in range(7)]), obsm={"spatial": xy}, obsp={"spatial_connectivities": g})
    df = sq.gr.sepal(ad, max_neighs=6, copy=True)
    lat = SO.compute_idxs(g, xy, 6)
    for j in range(7):  # each rank scored half of the genes; every score must equal the single-process restatement's band
        stop, deltas, _, _ = SO.diffusion(X[:, j], True, 30000, lat, 0.001, 1e-8)
        lo, hi = SO.band(deltas, 1e-8)
        s = df.loc[f"g{j}", "sepal_score"]
        assert (np.isnan(s) and lo < 0) or (lo <= round(s / 0.001) <= max(hi, lo)), (j, s, lo, hi)
    # the single-process frame: every gene through one plan on this rank, without the split
    from squidpy_amd._lib import DeviceMatrix, SepalPlan, default_context
    from squidpy_amd.gr._sepal import sepal_lattice

    sat, sat_idx, unsat, nearest = sepal_lattice(g, xy, 6)
    pos = np.empty(len(xy), np.int64)
    pos[sat] = np.arange(len(sat))
    ctx = default_context()
    plan, m = SepalPlan(ctx, len(xy), 6, sat, sat_idx, unsat, pos[nearest]), DeviceMatrix(ctx, X)
    it = plan.run(m, np.arange(7, dtype=np.int32), 30000, 0.001, 1e-8)
    single = pd.DataFrame(np.where(it >= 0, 0.001 * it.astype(np.float64), np.nan), index=[f"g{j}" for j in range(7)], columns=["sepal_score"])
    pd.testing.assert_frame_equal(df, single.sort_values(by="sepal_score", ascending=False))
    frames = _dist.allgather_object([list(df.index), df["sepal_score"].to_numpy()])
    assert frames[0][0] == frames[1][0] and np.array_equal(frames[0][1], frames[1][1], equal_nan=True)
    print("SEPAL_DIST_OK", rank, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

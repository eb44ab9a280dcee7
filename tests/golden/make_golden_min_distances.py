#!/usr/bin/env python3
"""Golden vectors for ``c_min_distances`` of the REAL reference (generators/utils/calc_min_distances.h: the nearest-point
search of ADD-S, its only native code on the path).

Runs only in the build container: it calls oracle/_ref/libmindist.so, which oracle/Makefile compiles from the reference's
header where it lies (``make -C oracle``).  The tests replay the stored answers wherever that library is absent.

    python tests/golden/make_golden_min_distances.py    # writes tests/golden/min_distances.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)


def cases():
    """Seeded clouds, regenerated identically by the tests: ([(name, gt cloud, predicted cloud)], (model points, R_gt, t_gt,
    R_pred, t_pred) for add_s_metric).  Close pairs, duplicates and large offsets; 2500 model points -> step 3 -> 834 points."""
    from oracle import decode_ref as D
    rng = np.random.Generator(np.random.PCG64(5))
    clouds = []
    for n_g, n_p, scale, off in ((1, 1, 1.0, 0.0), (7, 13, 100.0, 0.0), (500, 500, 130.0, 2.5), (1000, 777, 0.05, 1000.0)):
        g = (rng.standard_normal((n_g, 3)) * scale + off).astype(np.float32)
        p = (rng.standard_normal((n_p, 3)) * scale + off).astype(np.float32)
        if n_p > 10:
            p[3] = g[min(2, n_g - 1)]                       # an exact hit
            p[5] = p[4]                                    # duplicates
        clouds.append((f"g{n_g}_p{n_p}", g, p))
    pts = (rng.standard_normal((2500, 3)) * 60).astype(np.float32)
    Rg, Rp = D.rodrigues(np.array([0.3, -1.2, 0.5])), D.rodrigues(np.array([0.31, -1.18, 0.52]))
    tg, tp = np.array([10., -20., 600.]), np.array([11., -19., 604.])
    return clouds, (pts, Rg, tg, Rp, tp)


def metric_clouds(pts, Rg, tg, Rp, tp):
    """The two clouds add_s_metric hands to c_min_distances for 2500 model points (every third point)."""
    return (pts @ Rg.T + tg)[::3], (pts @ Rp.T + tp)[::3]


def main():
    from oracle import decode_ref as D
    clouds, metric = cases()
    fx = {name: D.reference_min_distances(g, p) for name, g, p in clouds}
    fx["add_s_metric"] = D.reference_min_distances(*metric_clouds(*metric))
    assert all(a.dtype == np.float32 for a in fx.values())
    np.savez_compressed(os.path.join(HERE, "min_distances.npz"), **fx)
    print("wrote min_distances.npz:", {k: v.shape for k, v in fx.items()})


if __name__ == "__main__":
    main()

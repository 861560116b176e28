"""CPU, oracle port only: do the noisy clouds of tests/test_gpu_pair_stream.py reach what the tests assert?  A kd-tree search,
the point-to-plane system and its solve per iteration (oracle/oracle.py), no engine.  Prints, for the converged case, the
share of points whose match is unchanged over the last three of twelve iterations, and for the transient, per iteration,
how often a point changes its match after keeping it for two iterations.  Output: profiles/pair_stream_seed_check.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from oracle import oracle as orc  # noqa: E402

orc.build()


def run(tree, tgt, nrm, pts, init, iters, max_dist):
    T = np.eye(4, dtype=np.float32) if init is None else init.copy()
    hist = []
    for _ in range(iters + 1):
        q = orc.transform_points(T, pts)
        _, idx, _ = tree.search_radius(q, max_dist, 1)
        m = idx[:, 0].copy()
        hist.append(m)
        rows = np.flatnonzero(m >= 0)
        cor = np.stack([rows, m[rows]], 1).astype(np.int32)
        _, dT = orc.solve_system(orc.compute_system(orc.EST_PT2PL, q, tgt, cor, tgt_nrm=nrm), -1.0)
        T = (dT.astype(np.float64) @ T.astype(np.float64)).astype(np.float32)
    return hist


def converged(n, seed):
    src, tgt, nrm, _, max_dist = bench.synth(n)
    s = float(n) ** (-1.0 / 3.0)
    rng = np.random.default_rng(seed)
    keep = rng.random(n) < 0.6
    noisy = (src[keep] + rng.normal(0.0, 0.15 * s, (int(keep.sum()), 3))).astype(np.float32)
    h = run(orc.Tree(tgt), tgt, nrm, noisy, None, 12, max_dist)
    same = (h[12] == h[11]) & (h[11] == h[10]) & (h[10] == h[9])
    print("converged: 60 %% of synth(%d), seed %d: %d points; unchanged over the last three of twelve: %.4f %%; changes per iteration: %s"
          % (n, seed, len(noisy), 100 * same.mean(), " ".join(str(int((h[t] != h[t - 1]).sum())) for t in range(1, 13))))


def transient(n, seed):
    src, tgt, nrm, _, max_dist = bench.synth(n)
    s = float(n) ** (-1.0 / 3.0)
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = (1.5 * s / np.sqrt(3.0)) * np.array([1.0, -1.0, 1.0], np.float32)
    ang = 0.5 * s
    init[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]], np.float32)
    rng = np.random.default_rng(seed)
    noisy = (src + rng.normal(0.0, 0.15 * s, src.shape)).astype(np.float32)
    h = run(orc.Tree(tgt), tgt, nrm, noisy, init, 30, max_dist)
    per = [int(((h[t - 3] == h[t - 2]) & (h[t - 2] == h[t - 1]) & (h[t] != h[t - 1])).sum()) for t in range(3, 31)]
    print("transient: synth(%d), seed %d: changes after two still iterations, iterations 3..30: %s; after iteration 10: %d"
          % (n, seed, " ".join(map(str, per)), sum(per[8:])))


if __name__ == "__main__":
    converged(200_003, 5)   # 120,061 points: below the one-launch iteration's limit, not usable
    converged(300_007, 5)
    transient(200_003, 6)
    transient(200_003, 7)

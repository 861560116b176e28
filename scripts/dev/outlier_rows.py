"""The outlier filters' rows: one JSON line.

    python scripts/dev/outlier_rows.py                       # the timed rows
    python scripts/dev/outlier_rows.py --profile             # only the 10M statistical filter, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -o rows -- python scripts/dev/outlier_rows.py --profile
    python scripts/dev/outlier_rows.py --tail DIR/.../rows_results.db           # the post-walk tail from that trace

Rows (ms, median of the timed calls after a warm-up call, timed with events on the engine's stream):
  stat_<n>    RemoveStatisticalOutliers(20, 2.0) of n uniform points in [0, 1)^3 with normals and colours
  radius_<n>  RemoveRadiusOutliers(16, 2.5 spacings) of the same cloud
  normals30_<n>  EstimateNormals(KNN 30) of the same points, in the same process
  ref_radius / ref_stat  the reference benchmark's rows (remove_radius_outlier(10, 0.1),
              remove_statistical_outlier(20, 2.0)) on tests/golden/fragment_every3rd.npz through the pybind module
The tail (--tail): per statistical call, every kernel between the k-NN walk and the end of select_gather -- the
statistics, the keep flags, the three scan launches and the gather -- from the first one's start to the gather's end
and as the sum of their own durations, median over the calls."""
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPS = 7


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 3)


def cloud(n, seed=42):
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda()
    nrm = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    col = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda()
    return p, nrm, col


def rows():
    from cupoch_amd.engine import Engine
    from cupoch_amd import pybind as cph
    eng = Engine(0)
    out = {}
    for n in (1_000_000, 10_000_000):
        p, nrm, col = cloud(n)
        tag = "%dM" % (n // 1_000_000)
        r = 2.5 * n ** (-1.0 / 3.0)
        out["stat_" + tag] = timed(lambda: eng.remove_statistical_outliers(p, 20, 2.0, nrm, col))
        out["radius_" + tag] = timed(lambda: eng.remove_radius_outliers(p, 16, r, nrm, col))
        out["normals30_" + tag] = timed(lambda: eng.estimate_normals_knn(p, 30))
        out["kept_stat_" + tag] = len(eng.remove_statistical_outliers(p, 20, 2.0)[3])
        out["kept_radius_" + tag] = len(eng.remove_radius_outliers(p, 16, r)[3])
        del p, nrm, col
    d = np.load(os.path.join(ROOT, "tests", "golden", "fragment_every3rd.npz"))
    pcd = cph.geometry.PointCloud()
    pcd.points = cph.utility.Vector3fVector(d["points"].astype(np.float32))
    out["ref_radius"] = timed(lambda: pcd.remove_radius_outlier(10, 0.1))
    out["ref_stat"] = timed(lambda: pcd.remove_statistical_outlier(20, 2.0))
    out["ref_points"] = len(pcd.points)
    eng.close()
    return out


def profile():
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    p, nrm, col = cloud(10_000_000)
    for _ in range(4):
        eng.remove_statistical_outliers(p, 20, 2.0, nrm, col)
    torch.cuda.synchronize()
    eng.close()


def _dispatches(trace):
    """(name, start ns, end ns) of every kernel in a rocprofv3 kernel trace: its results database (rocpd, the default
    output) or its kernel_trace.csv (--output-format csv)"""
    if trace.endswith(".db"):
        import sqlite3
        with sqlite3.connect(trace) as db:
            return [(n, int(a), int(b)) for n, a, b in db.execute("select name, start, end from kernels")]
    with open(trace) as f:
        recs = list(csv.DictReader(f))
    name = next(k for k in recs[0] if k.lower() in ("kernel_name", "kernelname", "name"))
    t0 = next(k for k in recs[0] if k.lower().startswith("start_timestamp"))
    t1 = next(k for k in recs[0] if k.lower().startswith("end_timestamp"))
    return [(r[name], int(r[t0]), int(r[t1])) for r in recs]


def tail(trace):
    recs = sorted(_dispatches(trace), key=lambda r: r[1])
    span, busy = [], []
    for i, (name, _, end) in enumerate(recs):
        if "select_gather" not in name:
            continue
        j = i
        while j > 0 and "knn_normals_kernel" not in recs[j - 1][0]:
            j -= 1
        if j == 0:
            continue
        span.append((end - recs[j][1]) / 1e6)                      # first tail kernel's start -> the gather's end
        busy.append(sum(b - a for _, a, b in recs[j:i + 1]) / 1e6)  # the tail's kernels alone
        kernels = [n.split("(")[0].replace("void ", "") for n, _, _ in recs[j:i + 1]]
    return {"tail_10M_ms": round(float(np.median(span)), 3), "tail_10M_kernels_ms": round(float(np.median(busy)), 3),
            "tail_calls": len(span), "tail_kernels": kernels}


if __name__ == "__main__":
    if "--profile" in sys.argv:
        profile()
    elif "--tail" in sys.argv:
        print(json.dumps(tail(sys.argv[sys.argv.index("--tail") + 1])))
    else:
        print(json.dumps(rows()))

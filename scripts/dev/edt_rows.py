"""Times of geometry::DistanceTransform.
  compute_edt at 128^3, 256^3 and 512^3 for three site sets -- 100 random cells, a surface-like 1 % (a spherical shell),
    a random 50 % --: host wall time of the Python call (it ends with a synchronisation), the median of 5 after a warm-up
    call, beside the traffic floor of the call: the clear of the seed plane, the z pass (one plane read, one written) and
    the y and x passes (each: the transform read, the stack written, the stack read, the transform written), 11 planes
    of res^3 x 4 bytes at 6.0 TB/s; and beside scipy.ndimage.distance_transform_edt of the same input on the host CPU,
    as context only (--no-scipy leaves it out; 512^3 is run for the surface set alone);
  get_distances of 1M queries at 512^3;
  --passes: the kernel time of every launch of one compute (the clear, the seeding, the three passes), per resolution
    and site set.  The library has no timing path, so each of these rows comes from a kernel trace of a fresh child
    process of this script (rocprofv3 --kernel-trace, a run of its own) that makes one warm-up call and one more; the
    second call's launches are reported.
Prints one line per row.

    python scripts/dev/edt_rows.py [--passes] [--res R] [--set 100|surface|random] [--no-scipy]
"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PLANES = 11
SWEEP_BYTES_PER_S = 6.0e12
SETS = ("100", "surface", "random")
LABEL = {"100": "100 cells", "surface": "surface 1 %", "random": "random 50 %"}


def median_ms(fn, sync, n=5):
    fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def site_set(torch, res, name):
    gen = torch.Generator(device="cuda").manual_seed(res)
    if name == "100":
        return torch.randint(0, res, (100, 3), generator=gen, device="cuda", dtype=torch.int32)
    if name == "surface":
        d = torch.randn((res ** 3 // 100, 3), generator=gen, device="cuda")
        d = d / d.norm(dim=1, keepdim=True) * (0.35 * res) + 0.5 * res
        return d.floor().to(torch.int32).clamp_(0, res - 1)
    lin = torch.nonzero(torch.rand(res ** 3, generator=gen, device="cuda") < 0.5).reshape(-1)
    return torch.stack([lin // (res * res), (lin // res) % res, lin % res], dim=1).to(torch.int32)


def scipy_ms(cells, res):
    from scipy import ndimage
    free = np.ones((res, res, res), bool)
    c = cells.cpu().numpy()
    free[c[:, 0], c[:, 1], c[:, 2]] = False
    t0 = time.perf_counter()
    ndimage.distance_transform_edt(free, return_distances=False, return_indices=True)
    return (time.perf_counter() - t0) * 1e3


def traced_child(res, name):
    """the run a kernel trace wants: one warm-up compute, one more, nothing else"""
    import torch
    from cupoch_amd import geometry
    d = geometry.DistanceTransform(1.0, res)
    cells = site_set(torch, res, name)
    torch.cuda.synchronize()
    d.compute_edt(cells)
    d.compute_edt(cells)
    torch.cuda.synchronize()


def pass_row(res, name):
    """-> [(kernel, microseconds)] of the second compute of a traced child, in launch order"""
    tmp = tempfile.mkdtemp(prefix="edt_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "edt", "--",
                        sys.executable, os.path.abspath(__file__), "--traced-child", str(res), name],
                       check=True, capture_output=True, text=True, timeout=300)
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    k = {key.lower(): v for key, v in r.items()}
                    col = lambda part: next(v for key, v in k.items() if part in key)
                    rows.append((int(col("start")), int(col("end")), col("kernel_name")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows.sort()
    ours = [(s, e, n) for s, e, n in rows if "edt_" in n or "fill" in n.lower()]
    first = [i for i, r in enumerate(ours) if "edt_pass_z" in r[2]]
    if len(first) < 2:
        raise RuntimeError("the trace does not hold two computes: %s" % sorted({n for _, _, n in rows}))
    # the second compute: from the launches between the two z passes that follow the first compute's x pass
    last_x = max(i for i, r in enumerate(ours[:first[1]]) if "edt_pass" in r[2] and "edt_pass_z" not in r[2])
    return [(n.split("(")[0].replace("mi::", "").replace("void ", ""), (e - s) / 1e3) for s, e, n in ours[last_x + 1:]]


def main():
    if "--traced-child" in sys.argv:
        i = sys.argv.index("--traced-child")
        return traced_child(int(sys.argv[i + 1]), sys.argv[i + 2])
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    sizes = [int(arg("--res", 0))] if "--res" in sys.argv else [128, 256, 512]
    sets = [arg("--set", None)] if "--set" in sys.argv else list(SETS)
    if "--passes" in sys.argv:          # (this process never opens the GPU: every row is a child of its own)
        for res in sizes:
            for name in sets:
                row = pass_row(res, name)
                print("passes %4d^3  %-12s %s   sum %.1f us" % (res, LABEL[name], ", ".join("%s %.1f" % kv for kv in row),
                                                                 sum(v for _, v in row)), flush=True)
        return
    import torch
    from cupoch_amd import geometry
    with_scipy = "--no-scipy" not in sys.argv
    sync = torch.cuda.synchronize
    for res in sizes:
        d = geometry.DistanceTransform(1.0, res)
        floor_ms = PLANES * res ** 3 * 4 / SWEEP_BYTES_PER_S * 1e3
        for name in sets:
            cells = site_set(torch, res, name)
            ms = median_ms(lambda: d.compute_edt(cells), sync)
            host = ""
            if with_scipy and (res < 512 or name == "surface"):
                host = "; scipy on the host %.0f ms" % scipy_ms(cells, res)
            print("compute_edt %4d^3  %-12s %8.3f ms   %9d cells given; floor %.3f ms (%.1fx)%s" %
                  (res, LABEL[name], ms, int(cells.shape[0]), floor_ms, ms / floor_ms, host), flush=True)
        if res == sizes[-1]:
            q = (torch.rand((1_000_000, 3), device="cuda") - 0.5) * float(res)
            ms = median_ms(lambda: d.get_distances(q), sync)
            print("get_distances %4d^3, 1M queries    %8.3f ms" % (res, ms), flush=True)
        del d


if __name__ == "__main__":
    main()

"""GPU: geometry::Graph<3> and planning::Pos3DPlanner through the C++ surface (tests/cpp/test_graph.cpp: the
reference's unit tests, the zero-weight trap, the wall with a window), built as the other tests/cpp programs are and
held exactly to the numpy restatement of the contract (tests/graph_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import graph_exact as gx
from test_gpu_planning import GOAL, RADIUS, REACH, START, VS, wall_keys

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_graph")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_graph.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    wall_keys(True).tofile(str(tmp_path / "wall.i32"))
    wall_keys(False).tofile(str(tmp_path / "closed.i32"))
    with open(str(tmp_path / "scene.txt"), "w") as f:
        f.write(" ".join("%.9g" % F(v) for v in (VS, RADIUS, REACH) + START + GOAL))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    for flag in ("ctor", "same_node", "early", "no_path", "written"):
        assert r[flag], flag
    assert "Unsupported obstacle type." in out.stderr
    n, lines, w, start = gx.small_cases()["five"]
    dist, prev = gx.sssp(lines, w, n, start)
    assert r["five_offsets"] == [0, 2, 4, 6, 9, 10] and r["five_dist"] == dist.tolist() == [0, 1, 2, 2, 3]
    assert r["five_prev"] == prev.tolist() and r["five_path"] == [0, 1, 3, 4]
    n, lines, w, start = gx.small_cases()["zero_pair_trap"]
    assert r["trap_prev"] == gx.sssp(lines, w, n, start)[1].tolist() == [3, 3, 1, 3]
    pts, lat, _, _ = gx.lattice((-1, -1, -1), (1, 1, 1), (10, 10, 10))
    assert (r["nodes"], r["edges"]) == (len(pts), len(lat))
    side = ("voxel", wall_keys(True), VS, np.zeros(3, F))
    want, ls, ws = gx.find_path(pts, lat, START, GOAL, [side], RADIUS, REACH)
    got = np.fromfile(str(tmp_path / "path.f32"), F).reshape(-1, 3)
    assert got.tobytes() == want.tobytes() and len(got) >= 4
    assert os.path.getsize(str(tmp_path / "path_closed.f32")) == 0
    free = np.fromfile(str(tmp_path / "path_free.f32"), F).reshape(-1, 3)
    assert free.tobytes() == gx.find_path(pts, lat, (-1.0, -0.5, -0.2), (0.8, 0.9, 0.7), [], 0.1, 1.0)[0].tobytes()
    import collision_exact as cx
    pairs = cx.compute_intersection(side, ("lines", pts, lat), RADIUS)
    ww = gx.set_edge_weights(lat, gx.weights_from_distance(pts, lat), lat[pairs[:, 1]], np.inf, False)
    assert np.fromfile(str(tmp_path / "weights.f32"), F).tobytes() == ww.tobytes()

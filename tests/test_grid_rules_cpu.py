"""CPU: the rules the grid geometries share (csrc/grid_rules.h: floor_int, cell_of, the res^3 cube, the bounds box, the
searches in ascending keys) against the numpy restatement -- tests/cpp/test_grid_rules.cpp, a stand-alone program that
includes nothing of the library but that header, built with AddressSanitizer and UBSan and run directly."""
import os
import re
import subprocess

import numpy as np
import pytest

import occgrid_exact as ox
from conftest import ROOT

F = np.float32
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _bits(v):
    return "%08x" % int(np.array(v, F).view(np.uint32))


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """ask(lines) -> the program's answers, one list of ints per request"""
    exe = str(tmp_path_factory.mktemp("grid_rules") / "test_grid_rules")
    src = os.path.join(ROOT, "tests", "cpp", "test_grid_rules.cpp")
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["grid_rules.h"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cupoch_amd", "csrc"), src, "-o", exe])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
        got = [[int(t) for t in line.split()] for line in out.stdout.split("\n") if line.strip()]
        assert len(got) == len(lines)
        return got
    return ask


def test_floor_int_at_the_clamps_and_on_seeded_values(rules):
    big = F(1.0e9)
    edge = [np.nan, np.inf, -np.inf, big, -big, np.nextafter(big, F(np.inf)), np.nextafter(big, F(0)),
            np.nextafter(-big, F(-np.inf)), np.nextafter(-big, F(0)), 2.0 ** 31, -2.0 ** 31, 3e38, -3e38, -0.0, -0.5, -1.0,
            0.99999994]
    rng = np.random.default_rng(7)
    seeded = np.concatenate([rng.uniform(-50, 50, 500), rng.uniform(-3e9, 3e9, 300), rng.integers(-99, 99, 200)])
    x = np.concatenate([np.array(edge, F), seeded.astype(F)])
    got = rules(["F " + _bits(v) for v in x])
    assert [g[0] for g in got] == ox.floor_int(x).tolist()
    assert got[0] == [-10 ** 9] and got[1] == [10 ** 9] and got[2] == [-10 ** 9]      # NaN, +inf, -inf


def test_cell_of_in_the_frame_that_is_no_multiple_of_the_voxel(rules):
    g = ox.new_grid(33)
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(-2.5, 2.5, (300, 3)), g.origin + F(0.1) * rng.integers(-17, 18, (100, 3))]).astype(F)
    want = ox.voxel_of(g, pts) - g.h
    lines = ["C %s %s %s %s %s %d" % (_bits(g.voxel_size), *[_bits(o) for o in g.origin], _bits(p[k]), k)
             for p in pts for k in range(3)]
    got = np.array(rules(lines)).reshape(-1, 3)
    assert np.array_equal(got, want)
    assert len(np.unique(got)) > 30


BOXES = [((3, 9, 5), (7, 19, 27)), ((4, 4, 4), (4, 4, 4)),
         ((8, 9, 5), (7, 19, 27)), ((3, 20, 5), (7, 19, 27)), ((3, 9, 28), (7, 19, 27))]   # the last three: empty on x, y, z


def test_box_of_bounds_and_box_voxel_in_box_linear_order(rules):
    g = ox.Grid(0.1, 32, ox.ORIGINS[33])
    got = rules(["B 32 %d %d %d %d %d %d" % (lo + hi) for lo, hi in BOXES])
    for (lo, hi), row in zip(BOXES, got):
        g.min_bound, g.max_bound = np.array(lo, np.int64), np.array(hi, np.int64)
        want = ox.box_linear(g)
        ext = [h - l + 1 for l, h in zip(lo, hi)]
        if len(want) == 0:
            assert row == [0] * 7
        else:
            assert row[:7] == list(lo) + ext + [len(want)]
        assert row[7:] == want.tolist()
    assert len(got[0]) == 7 + 5 * 11 * 23 and len(got[1]) == 8


@pytest.mark.parametrize("res", [2, 33])
def test_cube_inside_and_index_on_the_faces(rules, res):
    g = ox.Grid(0.1, res)
    side = np.array([-1, 0, 1, res - 2, res - 1, res])
    ijk = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
    got = rules(["I %d %d %d %d" % (res, *v) for v in ijk])
    inside = g.inside(ijk)
    want = [[1, int(l)] if ok else [0, -1] for ok, l in zip(inside, g.linear(ijk))]
    assert got == want
    assert inside.any() and not inside.all()


def test_occupied_is_known_and_above_the_threshold(rules):
    cases = [(np.nan, 0.0), (0.0, 0.0), (1e-30, 0.0), (-0.4, 0.0), (0.85, 0.85), (3.5, 0.85), (np.inf, 3.5), (-np.inf, -1.0)]
    got = rules(["O %s %s" % (_bits(p), _bits(t)) for p, t in cases])
    assert [g[0] for g in got] == [int((not np.isnan(p)) and F(p) > F(t)) for p, t in cases] == [0, 0, 1, 0, 0, 1, 1, 0]


@pytest.mark.parametrize("m", [0, 1, 200])
def test_keys3_searches_against_numpy(rules, m):
    rng = np.random.default_rng(13 + m)
    pool = np.array([I32_MIN + 1, -7, -1, 0, 1, 2, 5, I32_MAX], np.int64)
    keys = np.unique(pool[rng.integers(0, len(pool), (4 * m, 3))], axis=0)   # (unique sorts rows lexicographically)
    keys = keys[np.sort(rng.permutation(len(keys))[:m])]
    assert len(keys) == m
    if m == 200:
        assert (keys == I32_MIN + 1).any() and (keys == I32_MAX).any()
    steps = np.concatenate([np.zeros((1, 3), np.int64), np.eye(3, dtype=np.int64), -np.eye(3, dtype=np.int64)])
    q = np.concatenate([(keys[:, None, :] + steps[None]).reshape(-1, 3), np.full((1, 3), I32_MIN), np.full((1, 3), I32_MAX)])
    q = np.clip(q, I32_MIN, I32_MAX)       # (a step past the ends of int32 stays at the end)

    def below(strict):
        k, t = keys[None], q[:, None]
        last = k[..., 2] < t[..., 2] if strict else k[..., 2] <= t[..., 2]
        return ((k[..., 0] < t[..., 0]) | ((k[..., 0] == t[..., 0]) & ((k[..., 1] < t[..., 1]) | ((k[..., 1] == t[..., 1]) & last)))).sum(1)
    want = np.stack([below(True), below(False)], 1)
    got = rules(["K %d %s" % (m, " ".join(str(v) for v in keys.ravel()))] + ["Q %d %d %d" % tuple(v) for v in q])
    assert got[0] == [m]
    assert np.array_equal(np.array(got[1:]).reshape(-1, 2), want)
    if m:
        assert (want[:, 1] - want[:, 0]).max() == 1 and (want[:, 1] == want[:, 0]).any()

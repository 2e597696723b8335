"""The C++ side of the footprint check: PathOptimizationNS::FootprintChecker (include/pqp_footprint_checker.hpp) over the C ABI.
CPU: it compiles and links against libpqp_hip.so and the HIP runtime, and fails cleanly without a GPU.
GPU: its batch-of-one methods and checkPaths give what Handle.footprint_check gives for the same states."""
import math
import os
import subprocess

import numpy as np
import pytest

import cpp_demo
from path_optimizer_2_amd import capi
from path_optimizer_2_amd.synth import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo_exe(hip_lib):
    return cpp_demo.build("footprint_demo")


def _scene(tmp_path):
    cs = [make_scene(seed=s) for s in range(2)]
    c0 = cs[0]
    geom = capi.PqpGridGeometry(c0["rows"], c0["cols"], c0["resolution"], c0["length"][0], c0["length"][1], 0.0, 0.0)
    dists = np.stack([c["dist"] for c in cs])
    rng = np.random.default_rng(4)
    paths = []
    for k, n in enumerate([7, 1, 12, 5]):
        st = np.zeros((n, 3))
        st[:, 0] = rng.uniform(-0.55, 0.55, n) * geom.length_x
        st[:, 1] = rng.uniform(-0.55, 0.55, n) * geom.length_y
        st[:, 2] = rng.uniform(-math.pi, math.pi, n)
        paths.append((st, k % 2))
    path = tmp_path / "footprint.bin"
    with open(path, "wb") as f:
        f.write(np.array([geom.rows, geom.cols, 2, len(paths)], np.int32).tobytes())
        f.write(np.array([geom.resolution, geom.length_x, geom.length_y, geom.pos_x, geom.pos_y]).tobytes())
        f.write(np.ascontiguousarray(np.transpose(dists, (0, 2, 1))).astype(np.float32).tobytes())
        for st, m in paths:
            f.write(np.array([len(st), m], np.int32).tobytes())
            f.write(np.ascontiguousarray(st).tobytes())
    return str(path), geom, dists, paths


def test_checker_builds_and_fails_cleanly_without_gpu(demo_exe, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    path, *_ = _scene(tmp_path)
    r = subprocess.run([demo_exe, path], capture_output=True, text=True)
    assert r.returncode == 1 and "no checker" in r.stderr


@pytest.mark.gpu
def test_checker_agrees_with_the_python_call(demo_exe, tmp_path):
    path, geom, dists, paths = _scene(tmp_path)
    r = subprocess.run([demo_exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    n = max(len(st) for st, _ in paths)
    states = np.zeros((len(paths), n, 3))
    for k, (st, _) in enumerate(paths):
        states[k, :len(st)] = st
    n_of = np.array([len(st) for st, _ in paths], np.int32)
    map_of = np.array([m for _, m in paths], np.int32)
    want = {mode: h.footprint_check(states, n_of, dists, geom, map_of=map_of, mode=mode) for mode in (0, 1)}
    h.close()
    i = 0
    seen = [0, 0]
    for k, (st, _) in enumerate(paths):
        assert lines[i].split() == ["path", str(want[0]["first_collision"][k]), str(want[1]["first_collision"][k])]
        i += 1
        for j in range(len(st)):
            c, b, fc = (int(v) for v in lines[i].split())
            i += 1
            assert (c, b, fc) == (want[0]["free"][k, j], want[1]["free"][k, j], want[0]["free"][k, j]), (k, j)
            seen[c] += 1
    assert i == len(lines) and min(seen) > 0          # both answers occur

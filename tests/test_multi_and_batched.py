"""The multi-GPU driver of the C ABI (pqp_multi_*: one handle + host thread per shard) and the batched C++ surface
(include/pqp_batched_solver.hpp).  CPU: the sharding rule, symbols, clean failure without a GPU.  GPU: two shards on ONE device
(two handles, two host threads) against the single-handle solve; BatchedPathSolver with ragged scenarios against the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpp_demo
from path_optimizer_2_amd import capi
from path_optimizer_2_amd.shard import shard_range
from path_optimizer_2_amd.synth import make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_optimizer_2_amd", "csrc")


def test_shard_range_is_the_contiguous_split_of_the_python_side(hip_lib):
    first, count = C.c_int32(), C.c_int32()
    for total, world in [(65536, 8), (4096, 8), (1024, 3), (7, 8), (1, 1), (1000, 7)]:
        covered = 0
        for rank in range(world):
            hip_lib.pqp_shard_range(total, world, rank, C.byref(first), C.byref(count))
            assert (first.value, count.value) == shard_range(total, world, rank)
            assert first.value == covered
            covered += count.value
        assert covered == total


def test_multi_create_fails_loudly_without_a_device(hip_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.PqpError, match="no HIP device"):
        capi.MultiHandle(devices=(0, 1))


@pytest.fixture(scope="module")
def batched_exe(hip_lib):
    return cpp_demo.build("batched_demo", hip=False)


def _scenarios_text(b, counts):
    lines = [str(len(counts))]
    for q, n in enumerate(counts):
        lines.append(str(n))
        for i in range(n):
            lines.append(" ".join(repr(float(v)) for v in list(b["ref"][q, i]) + list(b["bounds"][q, i])))
        lines.append(" ".join(repr(float(v)) for v in b["scal"][q]))
    return "\n".join(lines) + "\n"


def test_batched_solver_builds_and_fails_cleanly_without_gpu(batched_exe):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    b = make_batch(2, 20)
    r = subprocess.run([batched_exe], input=_scenarios_text(b, [20, 12]), capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr and "Solving failed" in r.stderr


@pytest.mark.gpu
def test_two_shards_on_one_device_equal_the_single_handle_solve(hip_lib):
    """pqp_multi_path_solve with two handles (two host threads) on device 0: bit for bit what one handle gives for the whole batch,
    with and without a waypoint count per QP, odd batch (shards of 129 and 128)."""
    b = make_batch(257, 80)
    prm = capi.production_params()
    one = capi.Handle(prm, max_batch=257, max_n=80)
    want = one.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    two = capi.MultiHandle(prm, devices=(0, 0), max_batch_per_shard=129, max_n=80)
    got = two.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    for k in ("out", "status", "iters"):
        np.testing.assert_array_equal(got[k], want[k])
    assert (got["status"] == 1).all()
    counts = np.full(257, 80, dtype=np.int32)
    counts[::5] = 61
    counts[3] = 1                                   # a road blocked at its first waypoint: skipped, UNSOLVED
    want_v = one.solve_var(counts, b["ref"], b["bounds"], b["scal"], passes=1)
    got_v = two.solve(b["ref"], b["bounds"], b["scal"], passes=1, n_of=counts)
    for k in ("out", "status", "iters"):
        np.testing.assert_array_equal(got_v[k], want_v[k])
    assert got_v["status"][3] == 0 and (np.delete(got_v["status"], 3) == 1).all()
    two.close(); one.close()


@pytest.mark.gpu
def test_multi_driver_overlaps_its_shards_and_keeps_its_threads(hip_lib):
    """The host loop an 8-GPU node runs every tick: persistent worker threads (none created per call), pinned staging, asynchronous copies.
    Two shards on ONE device must overlap - the copies of one beside the solve of the other, the two solves sharing the chip: twice the
    QPs in well under twice the time of one shard through the same driver.  (How far under is bounded by the solve kernel itself: its
    persistent workgroups own every SIMD's register file, a second launch only gets the slots the first one's tail frees - 0.66 ms per
    launch with two in flight against 0.54 ms alone, i.e. at most 1.64x - and by ~0.3 ms of host staging per call: 1.38-1.41x measured,
    profiles/r03h_multi.txt.  On two GPUs nothing is shared.)"""
    import threading
    import time
    b1 = make_batch(1024, 80)
    b2 = make_batch(2048, 80)
    prm = capi.production_params()
    one = capi.MultiHandle(prm, devices=(0,), max_batch_per_shard=1024, max_n=80)
    two = capi.MultiHandle(prm, devices=(0, 0), max_batch_per_shard=1024, max_n=80)
    base_threads = threading.active_count()            # (python threads; the driver's std::threads are counted through /proc below)

    def os_threads():
        return len(os.listdir("/proc/self/task"))

    def rate(m, b, reps=30):
        for _ in range(3):
            m.solve(b["ref"], b["bounds"], b["scal"], passes=1)
        t0 = time.perf_counter()
        for _ in range(reps):
            r = m.solve(b["ref"], b["bounds"], b["scal"], passes=1)
        dt = (time.perf_counter() - t0) / reps
        assert (r["status"] == 1).all()
        return b["ref"].shape[0] / dt, r

    before = os_threads()
    # measured 1.38-1.49x; a serialised driver gives 1.0x.  Host-staging bound, i.e. sensitive to whatever else the box's host does: the ratio of the
    # best of up to three rounds is what is asserted (one round in ~10 of the GPU suite dipped below 1.2 on an otherwise green run)
    ratios = []
    for _ in range(3):
        r1, _ = rate(one, b1)
        r2, got = rate(two, b2)
        ratios.append(r2 / r1)
        if ratios[-1] >= 1.2:
            break
    assert os_threads() == before                       # the calls created no thread
    assert threading.active_count() == base_threads
    assert max(ratios) >= 1.2, ratios
    h = capi.Handle(prm, max_batch=2048, max_n=80)
    want = h.solve(b2["ref"], b2["bounds"], b2["scal"], passes=1)
    np.testing.assert_array_equal(got["out"], want["out"])
    # an inverted collision box is refused as by the single-handle host entry point
    bad = {k: v.copy() for k, v in b1.items()}
    bad["bounds"][7, 11, 0] = 9.0                       # (lower bound above the upper one)
    r = two.solve(bad["ref"][:64], bad["bounds"][:64], bad["scal"][:64], passes=1)
    assert r["status"][7] == 4 and (r["out"][7] == 0).all() and (np.delete(r["status"], 7) == 1).all()
    print(f"multi driver: one shard {r1 / 1e6:.2f} M paths/s, two shards on one device {r2 / 1e6:.2f} M paths/s")
    one.close(); two.close(); h.close()


@pytest.mark.gpu
def test_gather_over_rccl_in_the_c_abi(hip_lib):
    """pqp_multi_gather_paths: the result slabs the shards keep in device memory, gathered over RCCL so that every shard's GPU holds the whole
    batch (north_star: "RCCL over xGMI only to gather results").  On this one-GPU box: a single shard through the full RCCL path - dlopen,
    communicator, grouped broadcasts on the shard's stream - must hand back exactly the paths the host copy returned; two shards on ONE device
    are refused (RCCL takes one rank per device), as is a shape that is not the preceding solve's.  With one device per shard the same code
    broadcasts every shard's slab to the others (slabs of a batch that does not divide evenly differ by one QP, hence broadcasts, not one all-gather)."""
    import torch
    b = make_batch(96, 80)
    prm = capi.production_params()
    one = capi.MultiHandle(prm, devices=(0,), max_batch_per_shard=96, max_n=80)
    got = one.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    assert (got["status"] == 1).all()
    assert one.gather_ranks() == 0                                  # no communicator before the first gather
    full = one.gather_paths((0,))
    np.testing.assert_array_equal(full[0].cpu().numpy(), got["out"])
    assert one.gather_ranks() == 1                                  # ncclCommCount of the gather's communicator: one shard, one rank
    # a second call reuses the communicator; another batch through the same driver
    b2 = make_batch(64, 80, seed=77)
    got2 = one.solve(b2["ref"], b2["bounds"], b2["scal"], passes=1)
    np.testing.assert_array_equal(one.gather_paths((0,))[0].cpu().numpy(), got2["out"])
    one._last = (96, 80)
    with pytest.raises(capi.PqpError, match="not those of the preceding"):
        one.gather_paths((0,))
    one.close()
    two = capi.MultiHandle(prm, devices=(0, 0), max_batch_per_shard=48, max_n=80)
    two.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    with pytest.raises(capi.PqpError, match="one rank per device"):
        two.gather_paths((0, 0))
    two.close()


@pytest.mark.gpu
def test_gather_from_a_torch_free_process(hip_lib, tmp_path):
    """The same gather from a C++ caller that has never heard of torch (tests/cpp/gather_demo.cpp: plain HIP runtime + the C ABI): librccl.so is
    found by dlopen, every GPU's gathered copy equals the host copy.  Runs with as many shards as the box has GPUs (one here; on an 8-GPU node the
    same program checks all eight copies: `tests/cpp/gather_demo <file> 8`)."""
    import torch
    exe = os.path.join(ROOT, "tests", "cpp", "gather_demo")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "gather_demo.cpp"),
                    "-L" + CSRC, "-lpqp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    b = make_batch(70, 80, seed=5)
    path = str(tmp_path / "batch.bin")
    with open(path, "wb") as f:
        f.write(np.array([70, 80], dtype=np.int32).tobytes())
        for k in ("ref", "bounds", "scal"):
            f.write(np.ascontiguousarray(b[k], dtype=np.float64).tobytes())
    shards = torch.cuda.device_count()
    r = subprocess.run([exe, path, str(shards)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"gather ok {shards} 70 solved 70" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.gpu
def test_multi_driver_carries_a_planning_cycle(hip_lib):
    """pqp_multi_set_option(PQP_OPT_CARRY_CYCLES): a call of the shape of the previous one starts every shard's first solve from what its handle
    kept - same paths as a driver without the option, on scenarios that moved by 5 %; a call of another shape starts cold."""
    from path_optimizer_2_amd.synth import jitter_batch
    host = make_batch(600, 80, seed=3)
    prm = capi.production_params()
    a = capi.MultiHandle(prm, devices=(0, 0), max_batch_per_shard=300, max_n=80)
    b = capi.MultiHandle(prm, devices=(0, 0), max_batch_per_shard=300, max_n=80)
    assert a.lib.pqp_multi_set_option(a._m, capi.OPT_CARRY_CYCLES, 1) == 0
    for v in range(3):
        hv = jitter_batch(host, v, seed=3)
        ra = a.solve(host["ref"], hv["bounds"], hv["scal"], passes=1)
        rb = b.solve(host["ref"], hv["bounds"], hv["scal"], passes=1)
        assert (ra["status"] == 1).all()
        assert np.abs(ra["out"] - rb["out"]).max() < 1e-6
        if v > 0:
            assert ra["info"][:, 6].mean() < 0.9 * rb["info"][:, 6].mean()        # fewer factorisations: the carried start
    other = make_batch(200, 64, seed=4)
    np.testing.assert_array_equal(a.solve(other["ref"], other["bounds"], other["scal"], passes=1)["out"], b.solve(other["ref"], other["bounds"], other["scal"], passes=1)["out"])
    a.close(); b.close()


@pytest.mark.gpu
def test_batched_cpp_solver_against_the_c_abi(batched_exe, hip_lib):
    """BatchedPathSolver (production setting) on three scenarios of different length, one and two shards: the paths the C++ vectors
    carry are the C ABI's solve_var result digit for digit."""
    b = make_batch(3, 80)
    counts = [80, 57, 33]
    h = capi.Handle(capi.production_params(), max_batch=3, max_n=80)
    want = h.solve_var(np.array(counts, dtype=np.int32), b["ref"], b["bounds"], b["scal"], passes=1)
    h.close()
    for shards in ("1", "2"):
        env = dict(os.environ)
        r = subprocess.run([batched_exe, shards], input=_scenarios_text(b, counts), capture_output=True, text=True, env=env)
        if shards == "2" and r.returncode != 0 and "bad device ordinal" in r.stderr:
            continue                                 # a one-GPU box: the second shard's device does not exist (refused loudly)
        assert r.returncode == 0, r.stderr
        rows = r.stdout.strip().splitlines()
        pos = 0
        for q, n in enumerate(counts):
            ok, m = (int(v) for v in rows[pos].split())
            assert ok == 1 and m == n
            got = np.array([[float(v) for v in ln.split()] for ln in rows[pos + 1:pos + 1 + m]])
            np.testing.assert_array_equal(got, want["out"][q, :n])
            pos += 1 + m

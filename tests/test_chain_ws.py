"""The workspace of pqp_optimize_path_device is sized and carved from one list of its arrays (csrc/pqp_chain_ws.hpp): tests/cpp/chain_ws_check.cpp,
a plain C++ program on that header alone, checks sizes against the closed forms, disjointness, tiling and alignment.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_workspace_arrays_tile_their_buffers(tmp_path):
    exe = str(tmp_path / "chain_ws_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "chain_ws_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok 12", r.stdout          # 3 capacity sets x 2 batches x 2 values of second_pass

"""Building the C++ demos of tests/cpp against libpqp_hip.so (the link needs no device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_optimizer_2_amd", "csrc")
SHIM = os.path.join(CSRC, "base_solver_shim.cpp")          # the drop-in BaseSolver, compiled into the demos that use it (extra=[SHIM])
REF_INCLUDE = "/root/reference/include"                    # the reference's own headers, for the compile checks against them (skipped where absent)


def build(name, hip=True, extra=()):
    """tests/cpp/<name>.cpp (and the sources in `extra`) -> the executable tests/cpp/<name>, linked against libpqp_hip.so.
    hip: the demo includes the HIP runtime's headers and links the runtime; otherwise plain C++ against the library alone."""
    exe = os.path.join(ROOT, "tests", "cpp", name)
    src = [exe + ".cpp", *extra]
    if hip:
        cmd = ["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-o", exe,
               *src, "-L" + CSRC, "-lpqp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-o", exe, *src, "-L" + CSRC, "-lpqp_hip", "-Wl,-rpath," + CSRC]
    subprocess.run(cmd, check=True)
    return exe


def shim_scenario_text(b, q):
    """scenario q of the batch b as tests/cpp/shim_demo.cpp and shim_latency.cpp read it from standard input"""
    n = b["ref"].shape[1]
    lines = [str(n)]
    for i in range(n):
        lines.append(" ".join(repr(float(v)) for v in list(b["ref"][q, i]) + list(b["bounds"][q, i])))
    lines.append(" ".join(repr(float(v)) for v in b["scal"][q]))
    return "\n".join(lines) + "\n"

"""What the build left behind, read by more than one test file: the functions include/pqp.h declares and the compiler's resource report
of every kernel (__graft_entry__.build_hip -> csrc/libpqp_hip.resources.txt)."""
import os
import re

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    """the names of the functions include/pqp.h declares"""
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pqp_[a-z_0-9]+)\s*\(", txt)))


def kernel_report():
    """{kernel's mangled name: {resource: value}} from the compiler's remarks"""
    g.build_hip()
    if not os.path.exists(g.RESOURCES):
        g.build_hip(force=True)
    kernels, cur = {}, None
    for line in open(g.RESOURCES):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[\w/]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def find_kernel(kernels, *parts):
    """the one kernel of the report whose name holds every one of `parts`"""
    hits = [(k, v) for k, v in kernels.items() if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, [k for k, _ in hits])
    return hits[0][1]

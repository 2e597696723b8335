"""What of the reference compiles from its own std-only sources (oracle/_ref/libref_types.so: constrainAngle of include/tools/tools.hpp:24-35,
the POD types of include/data_struct/data_struct.hpp:14-32,74-93, VehicleState of src/data_struct/vehicle_state_frenet.cpp) against the
restatements: constrain_angle of both oracles and of the HIP kernels bit for bit, include/pqp_types.hpp field by field."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ref_pieces as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constrain_angle_of_both_oracles_is_the_reference_template_bit_for_bit():
    import pqp_oracle as O
    import __graft_entry__ as g
    g.build_oracle()
    oc = C.CDLL(os.path.join(ROOT, "oracle", "libpqp_oracle.so"))
    oc.pqo_constrain_angle.argtypes = [C.c_double]
    oc.pqo_constrain_angle.restype = C.c_double
    ref = RP.reference()
    for a, want in zip(ref["angle"], ref["angle_constrained"]):
        a, want = float(a), float(want)
        assert -math.pi <= want <= math.pi
        assert O.constrain_angle(float(a)) == want, a
        assert oc.pqo_constrain_angle(float(a)) == want, a


def test_pqp_types_have_the_reference_layouts_and_semantics():
    ref = RP.reference()
    want_layout = [int(v) for v in ref["layout"]]
    o8, o6 = list(ref["state"]), list(ref["vehicle"])
    exe = os.path.join(ROOT, "tests", "cpp", "types_layout")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "types_layout.cpp")], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {ln.split()[0]: ln.split()[1:] for ln in lines}
    assert [int(x) for x in got["layout"]] == want_layout                      # sizeof / offsetof of State, SlState, SingleBound, VehicleStateBound
    assert want_layout[0] == 64 and want_layout[9] == 80 and want_layout[18] == 120
    assert [float(x) for x in got["state"]] == list(o8)                         # State(x, y, heading, k, s, v, a): d_k stays 0
    assert [float(x) for x in got["vehicle"]] == list(o6)
    # SingleBound::set takes {ub, lb} in that order (data_struct.hpp:82-88): what the shim's bounds[n][6] = (lb, ub) per circle undoes
    assert RP.BOUND_ARGS == ((1.75, -2.25), (4.0, 5.0, 0.5))
    assert list(ref["single_bound"]) == [1.75, -2.25, 4.0, 5.0, 0.5]


@pytest.mark.gpu
def test_constrain_angle_of_the_hip_kernels_is_the_reference_template_bit_for_bit(hip_lib):
    from path_optimizer_2_amd import capi
    ref = RP.reference()
    a, want = ref["angle"], ref["angle_constrained"]
    h = capi.Handle(capi.default_params(), device=0, max_batch=1, max_n=8)
    got = h.constrain_angle(a)
    h.close()
    assert np.array_equal(got, want)

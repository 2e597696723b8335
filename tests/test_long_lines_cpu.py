"""PQP_OPT_LONG_LINES without a GPU: the option's value in the C header is the binding's, and the long forms of the line kernels
(pqp_corridor_kernels.inc: each the text of its LDS kernel, a pqp_*_body.inc with PQP_LINE_LONG = 1) keep everything in registers - no scratch - with the static LDS the launchers count on."""
import os
import re

import pytest

from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_value_matches_the_header():
    text = open(os.path.join(ROOT, "include", "pqp.h")).read()
    m = re.search(r"PQP_OPT_LONG_LINES\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == capi.OPT_LONG_LINES == 8


# kernel -> static LDS ("LDS Size"): the long DP keeps its cost tables in dynamic LDS (DpBlock<false, true>), the corridor forms their first-blocked
# index, reference states its count, the B-spline its count and degree
LONG_KERNELS = {"long_fit_kernel": 0, "long_ref_states_kernel": 4, "long_ref_length_kernel": 0, "long_offsets_kernel": 0,
                "long_bspline_kernel": 8, "long_dp_kernel": 0, "long_corridor_kernel": 16, "long_states_kernel": 16}


@pytest.fixture(scope="module")
def kernels():
    from build_util import kernel_report
    return kernel_report()


@pytest.mark.parametrize("name", sorted(LONG_KERNELS))
def test_long_forms_use_no_scratch(kernels, name):
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, name
    r = hits[0]
    assert r["ScratchSize"] == 0, r
    assert r["LDS Size"] == LONG_KERNELS[name], r


def test_no_existing_kernel_name_is_part_of_a_long_form_name(kernels):
    """tests/test_kernel_resources.py finds a kernel by a substring of its name"""
    for new in LONG_KERNELS:
        assert len([k for k in kernels if new in k]) == 1, new
    for old in ("spline_fit_kernel", "reference_states_kernel", "reference_length_kernel", "offsets_to_points_kernel", "bspline_resample_kernel",
                "dp_corridor_kernel", "corridor_bounds_kernel", "states_bounds_kernel"):
        assert len([k for k in kernels if old in k]) == 1, old

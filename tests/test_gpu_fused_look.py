"""The look fused into a polish solve on the device: the lane-per-waypoint kernel against the host emulation of the same source, QP by QP.
The emulation exchanges neighbours through the shared array and runs one lane after the other; the device runs rows of 16 lanes through DPP, wavefronts
side by side and the look's reduction across them.  An accept / reject decision that differed would show as another status or another count of reduced
solves (info[5]) or factorisations (info[6]).  N = 17, 64, 65, 80: a row's last lane (15 | 16), a wavefront's (63 | 64), the last real lane on and
beside them, N not a multiple of 16."""
import pytest

import emu_util as EU
from emu_util import compare_counts as _compare
from path_optimizer_2_amd.synth import make_batch

pytestmark = pytest.mark.gpu


def _both(hip_lib, batch, n, profile="uniform"):
    from path_optimizer_2_amd import capi
    b = make_batch(batch, n, profile)
    h = capi.Handle(capi.production_params(), device=0, max_batch=batch, max_n=n)
    h.set_option(capi.OPT_STORE_WARM, 0)
    dev = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    h.close()
    emu = EU.solve(EU.production(), b["ref"], b["bounds"], b["scal"], passes=1)
    return dev, emu


def test_bench_batch_counts_equal_the_emulation(hip_lib):
    """configs[1]'s batch (1024 QPs of 80 waypoints, the production setting) through the shipped library"""
    dev, emu = _both(hip_lib, 1024, 80)
    _compare(dev, emu, "configs[1] 1024 x 80")


@pytest.mark.parametrize("n", [17, 64, 65, 80])
def test_boundary_lanes_counts_equal_the_emulation(hip_lib, n):
    dev, emu = _both(hip_lib, 256, n, "varied" if n == 80 else "uniform")
    _compare(dev, emu, f"256 x {n}")

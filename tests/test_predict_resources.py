"""Register / scratch budget of the prediction kernel (pqp_predict_kernels.inc), from the compiler's own report written by the build, as
tests/test_kernel_resources.py reads it for the other families."""
from build_util import find_kernel as _find
from test_kernel_resources import kernels  # noqa: F401  (the module-scoped fixture)


def test_predict_kernel_uses_no_scratch_and_no_lds(kernels):  # noqa: F811
    """one wavefront per (scene, agent): the track, the anchor and a step's pose live in registers (189 VGPRs); the
    projection shares its scan through shuffles, so there is no LDS either"""
    r = _find(kernels, "predict_agents_kernel")
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["LDS Size"] == 0, r

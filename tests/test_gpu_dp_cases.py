"""dp_corridor_kernel and its long form long_dp_kernel (pqp_dp_body.inc) on the scenes of tests/dp_cases.py, whose bounds depend on the edge
costs, the own cost of a node, the admissible-predecessor window, the tie rule and the ring of prepared layers, and in which no decision of the
search is within round-off of going the other way (tests/test_dp_cases_cpu.py holds the margins and the mutation table).  So every lb / ub
entry is held to 1e-9 - no share of the entries may differ - and both forms, through the host and the device entry point, give the same bits.
Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import dp_cases as D
import long_line_util as LL
from device_form import SENT, d_dp, host_equals_device
from path_optimizer_2_amd import capi
from shared_util import capi_geom, same_bytes

pytestmark = pytest.mark.gpu

FORMS = (LL.OPT_LDS_ONLY, LL.OPT_LONG_ALWAYS)          # dp_corridor_kernel, long_dp_kernel


@pytest.fixture(scope="module")
def handles(hip_lib):
    """a default handle and one whose line kernels always run in their long form"""
    hs = {v: LL.with_option(capi.Handle(capi.default_params(), device=0, max_batch=64, max_n=128), v) for v in FORMS}
    yield hs
    for h in hs.values():
        h.close()


def _prm(p):
    return capi.PqpDpParams(p.lateral_range, p.longitudinal_spacing, p.lateral_spacing, p.car_width)


def _launch(h, device, tab, ext, length, start, dist, geom, prm, max_layers, map_of=None):
    """(layers_s, lb, ub, count, vehicle_l) through the device or the host entry point"""
    if device:
        rc, *out = d_dp(h, tab, ext, length, start, dist, capi_geom(geom), max_layers, map_of=map_of, prm=_prm(prm))
        assert rc == 0
        return out
    return h.dp_corridor(tab, ext, length, start, dist, capi_geom(geom), max_layers=max_layers, map_of=map_of, prm=_prm(prm))


def _scene_launch(h, device, sc, max_layers):
    return _launch(h, device, sc["tab"][None], sc["ext"][None], np.array([sc["length"]]), np.array([sc["start"]]), np.ascontiguousarray(sc["dist"]),
                   sc["geom"], sc["prm"], max_layers)


def _all_four(handles, sc, max_layers):
    """{(form, device): outputs}; all four agree bit for bit (the device form leaves the rows past count alone, the host form has zeros there)"""
    got = {(v, dev): _scene_launch(handles[v], dev, sc, max_layers) for v in FORMS for dev in (False, True)}
    base = got[(FORMS[0], False)]
    for v in FORMS:
        host, dev = got[(v, False)], got[(v, True)]
        assert np.array_equal(host[3], dev[3]) and same_bytes(host[4], dev[4]), (v, host[3], dev[3])
        for j in range(3):
            host_equals_device(host[j], dev[j], dev[3], max_layers)
        assert all(same_bytes(a, b) for a, b in zip(host, base)), ("form", v)
    return base


def _against_the_oracle(out, q, want, what):
    """every output of scenario q of a launch against the oracle's result: no entry excused"""
    ls, lb, ub, count, vl = out
    k = len(want["lb"])
    print(f"{what}: count {int(count[q])} (oracle {k}), |vehicle_l| err {abs(vl[q] - want['vehicle_l']):.2e}", end="")
    assert count[q] == k, what
    e_s = np.abs(ls[q, :k] - want["layers_s"]).max()
    e_lb, e_ub = np.abs(lb[q, :k] - want["lb"]), np.abs(ub[q, :k] - want["ub"])
    print(f", layers_s err {e_s:.2e}, lb err {e_lb.max():.2e} ({int((e_lb >= 1e-9).sum())} entries off), ub err {e_ub.max():.2e} ({int((e_ub >= 1e-9).sum())} off)")
    assert abs(vl[q] - want["vehicle_l"]) <= 1e-12, what
    assert e_s <= 1e-11, what
    assert np.all(e_lb < 1e-9) and np.all(e_ub < 1e-9), (what, np.nonzero(e_lb >= 1e-9)[0], np.nonzero(e_ub >= 1e-9)[0], lb[q, :k], want["lb"], ub[q, :k], want["ub"])


@pytest.mark.parametrize("name", D.NAMES)
def test_scene_matches_the_oracle_in_both_forms(handles, name):
    sc = D.scenes()[name]
    want = D.expected(name)
    out = _all_four(handles, sc, want["n_layers_sampled"] + 3)
    _against_the_oracle(out, 0, want, name)
    if name == "wall":                        # stopped: the layers behind the last reachable one are not reported
        assert 0 < out[3][0] < want["n_layers_sampled"] and np.all(out[0][0, out[3][0]:] == 0.0)


def test_max_layers_exactly_the_layer_count_and_one_less(handles):
    sc = D.scenes()["discs_0"]
    want = D.expected("discs_0")
    n = want["n_layers_sampled"]
    assert len(want["lb"]) == n
    out = _all_four(handles, sc, n)
    _against_the_oracle(out, 0, want, "max_layers == layers")
    for v in FORMS:
        for dev in (False, True):
            ls, lb, ub, count, vl = _scene_launch(handles[v], dev, sc, n - 1)
            assert count[0] == -1 and abs(vl[0] - want["vehicle_l"]) <= 1e-12
            if dev:                                                                    # nothing reported
                assert np.all(ls == SENT) and np.all(lb == SENT) and np.all(ub == SENT)


def test_batch_on_several_maps_is_each_scenario_alone(handles):
    """seven scenarios on four maps in one launch - among them the stopped one, one with the vehicle out of range (count 0) and one whose
    layers do not fit (count -1): the blocks do not see each other, every scenario comes out bit for bit as launched alone"""
    b = D.batch()
    B, max_layers = len(b["names"]), b["max_layers"]
    prm = D.scenes()["discs_0"]["prm"]
    want = [D.batch_expected(q) for q in range(B)]
    counts = np.array([D.batch_count(w, max_layers) for w in want])
    base = None
    for v in FORMS:
        host = _launch(handles[v], False, b["tab"], b["ext"], b["length"], b["start"], b["dist"], D.GEOM, prm, max_layers, map_of=b["map_of"])
        dev = _launch(handles[v], True, b["tab"], b["ext"], b["length"], b["start"], b["dist"], D.GEOM, prm, max_layers, map_of=b["map_of"])
        assert np.array_equal(host[3], counts), (v, host[3], counts)
        assert np.array_equal(dev[3], counts) and same_bytes(host[4], dev[4])
        for j in range(3):
            host_equals_device(host[j], dev[j], dev[3], max_layers)
        base = base or host
        assert all(same_bytes(x, y) for x, y in zip(host, base)), ("form", v)
        for q in range(B):
            alone = _launch(handles[v], False, b["tab"][q:q + 1], b["ext"][q:q + 1], b["length"][q:q + 1], b["start"][q:q + 1],
                            b["dist"][b["map_of"][q]], D.GEOM, prm, max_layers)
            assert all(same_bytes(x[q:q + 1], y) for x, y in zip(host, alone)), (v, b["names"][q])
    for q in range(B):
        if counts[q] > 0:
            _against_the_oracle(base, q, want[q], "batch " + b["names"][q])
        elif want[q] is not None:
            assert abs(base[4][q] - want[q]["vehicle_l"]) <= 1e-12
        assert np.all(base[1][q, max(counts[q], 0):] == 0.0)

"""The configurations of Handle.optimize_path that tests/test_chain_plan.py, test_gpu_chain.py and tools/chain_wrapper_digest.py share: every
combination of the steps behind the device chain in which the wrapper takes another path, at the smallest shapes that keep the sizes
apart - a batch of four in three groups (one empty, so groups != batch), two scenes of one agent, three layers, two sub-steps per layer
(five fine steps) and three samples."""
import math

import numpy as np

from path_optimizer_2_amd import capi

B, N_MAX, GROUP_START, GROUPS, SCENES, LAYERS, R, FINE, SAMPLES = 4, 128, [0, 2, 2, 4], 3, 2, 3, 2, 5, 3
CHAIN_CONFIG = dict(raw_max=64, sample_max=48, layer_max=32, n_max=N_MAX)          # Handle.chain_config(**CHAIN_CONFIG)


def configs(lib, start=None, target=None):
    """name -> (on_grid, keyword arguments), in the order (a) .. (l).  start / target [B][3]: the scenarios' poses, which put one agent
    per scene across a candidate's line and one track on its way back from the target (None: all zero, for a plan without a device)."""
    start, target = (np.zeros((B, 3)) if x is None else np.asarray(x) for x in (start, target))
    gs = np.array(GROUP_START, np.int32)
    sp = capi.speed_default_params(lib, v_max=8.0)
    se = capi.search_params_from_speed(lib, sp, 1.0, 0.5)
    se.stations, se.margin = 96, 0.2
    rf = capi.refine_default_params(lib, w_jerk=0.5, window=6)
    agents = np.zeros((SCENES, 1, LAYERS, 6))
    tracks = np.zeros((SCENES, 1, 9))
    for s in range(SCENES):                                      # scene s: the candidates 2 s and 2 s + 1
        st, tg = start[2 * s], target[2 * s]
        agents[s, 0, :] = [0.5 * (st[0] + tg[0]), 0.5 * (st[1] + tg[1]), st[2] + 1.5, 2.2, 0.9, 0.1]
        agents[s, 0, 0, 3] = -1.0                                # absent at the first layer
        tracks[s, 0] = [tg[0], tg[1], tg[2] + math.pi, 3.0, 0.5, 0.05, 2.2, 0.9, 0.1]
    fine_agents = np.ascontiguousarray(agents[:, :, np.arange(FINE) // R])
    rows = dict(v_start=np.linspace(0.0, 3.0, B), scene_of=np.array([0, 0, 1, 1], np.int32))                # one entry per candidate
    winners = dict(v_start=np.linspace(0.5, 2.5, GROUPS), scene_of=np.array([0, 1, 1], np.int32))          # one entry per group
    b = dict(check_footprint=True)
    d = dict(b, select=gs)
    e = dict(d, speed=sp, sample=capi.sample_default_params(lib), samples=SAMPLES, agents=agents, **winners)
    f = dict(b, speed=sp, agents=agents, search=se, **rows)
    stack = dict(f, refine=rf, plan_samples=R, plan_agents=fine_agents)
    j = dict(stack, rank=gs, rank_params=capi.rank_default_params(lib, w_clearance=0.5))
    return {
        "a": (False, {}),
        "b": (False, b),
        "c": (True, b),
        "d": (False, d),
        "d_winners": (False, dict(d, winners_only=True)),
        "e": (False, e),
        "e_winners": (False, dict(e, winners_only=True)),
        "f": (False, f),
        "g": (False, dict(speed=sp, sample=capi.sample_default_params(lib), samples=SAMPLES, agents=agents, search=se, **rows)),
        "h": (False, dict(select=gs, speed=sp, agents=agents, search=se, refine=rf, plan_samples=R, plan_agents=fine_agents, **winners)),
        "i": (False, dict(f, plan_samples=R)),
        "j": (False, j),
        "j_winners": (False, dict(j, winners_only=True)),
        "k": (False, dict(speed=sp, v_start=rows["v_start"], tracks=(tracks, None, None, None), layers=LAYERS, search=se, plan_samples=R,
                          predict_anchor=True, rank=gs)),
        "l": (False, dict(f, agents=np.zeros((SCENES, 0, LAYERS, 6)))),
    }

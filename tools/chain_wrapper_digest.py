"""What Handle.optimize_path / optimize_path_on_grid return for every configuration of tests/chain_plan_cases.py, as digests: a JSON of
{config: {key: [dtype, shape, sha256 of the bytes]}} in the result's own key order, a fresh pair of handles per configuration.  Run on two
commits, the two files tell whether a change of the wrapper (path_optimizer_2_amd/capi.py) changed a bit of what it returns - a change of
a kernel may, so the digests are a record (profiles/), not a test.  The first failure ends the run.

  python tools/chain_wrapper_digest.py --out digest.json [--times times.json]

--times: also the wall time of optimize_path in configuration (j) at a batch of 16, 10 calls after 2 warm-up calls, in milliseconds."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import chain_plan_cases as cases  # noqa: E402
import chain_util  # noqa: E402
from distance_util import occupancy_of  # noqa: E402
from path_optimizer_2_amd import capi  # noqa: E402


def run(sc, on_grid, kw, batch):
    h, hs = chain_util.handles(batch, max_n=(cases.N_MAX, cases.N_MAX))
    call = h.optimize_path_on_grid if on_grid else h.optimize_path
    layer = np.stack([occupancy_of(d) for d in sc["dist"]]) if on_grid else sc["dist"]
    args = (sc["pts"], sc["n_pts"], sc["start"], sc["target"], layer, sc["geom"])
    more = dict(map_of=sc["map_of"], smoother=hs, cfg=h.chain_config(**cases.CHAIN_CONFIG), **kw)
    return h, hs, lambda: call(*args, **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--times")
    a = ap.parse_args()
    lib = capi.load_library()
    sc = chain_util.scenarios(cases.B)
    digest = {}
    for name, (on_grid, kw) in cases.configs(lib, sc["start"], sc["target"]).items():
        h, hs, call = run(sc, on_grid, kw, cases.B)
        res = call()
        h.close(); hs.close()
        digest[name] = {k: [str(v.dtype), list(v.shape), hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()] for k, v in res.items()}
        print(name, len(res), "keys,", int((res["stage"] == 0).sum()), "of", cases.B, "scenarios give a path", flush=True)
    with open(a.out, "w") as f:
        json.dump(digest, f, indent=1)
    if a.times:
        batch = 16
        sc = chain_util.scenarios(batch)
        kw = dict(cases.configs(lib, sc["start"][::4], sc["target"][::4])["j"][1], v_start=np.linspace(0.0, 3.0, batch),
                  scene_of=(np.arange(batch) // 8).astype(np.int32), rank=np.array([0, 5, 5, batch], np.int32))
        h, hs, call = run(sc, False, kw, batch)
        ms = []
        for _ in range(12):
            t0 = time.perf_counter()
            call()
            ms.append(1e3 * (time.perf_counter() - t0))
        h.close(); hs.close()
        with open(a.times, "w") as f:
            json.dump(dict(config="j", batch=batch, warm_up_ms=ms[:2], call_ms=ms[2:]), f, indent=1)
        print("config j at batch", batch, "ms per call:", " ".join(f"{v:.3f}" for v in ms[2:]), flush=True)


if __name__ == "__main__":
    main()

"""What one re_logic_list (the frame's entity-logic call list, LogicFlow::update_logic on the device) costs on bench.py's 10,077,696-entity world with
every 100th entity a rotating body (configs[2]) and bench.py's camera (far 1000), after the frame's synchronous re_cull_pack.  GPU.

  case a   the 100,777 rotating bodies carry a type with entity logic (the listed rows are the non-static entities)
  case b   every entity carries it (10,077,696 listed rows; the static ones leave after their flag word)
  call_us  wall time of one re_logic_list with the records read back: median (min / max) after warm-up
Kernel time: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/logic_cost.py --reps 50` (k_logic_list in the stats)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import render_engine_amd as R  # noqa: E402
from bench import make_shard, PER_GPU_AXIS  # noqa: E402

TYPE = 0x51DE0001


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2), n=int(len(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    atomic = 64
    ents, dims, first = make_shard(0, 1, PER_GPU_AXIS, atomic, 100)
    centre = np.array([(first + d / 2.0) * atomic for d in (dims[0], dims[2], dims[1])], np.float32)
    p = R.Pipeline(16384, atomic); p.register_model_instances(ents)
    p.set_entity_logic([(TYPE, R._capi.LOGIC_ENTITY)])
    cam = R.Camera(centre, (0.0, 0.0, -1.0), 1000.0)
    spinners = np.ascontiguousarray(ents["id"][(ents["flags"] & R.F_HAS_ROTVEL) != 0], np.uint32)
    out = dict(workload="configs[2] world: %d entities, %d rotating, far 1000" % (len(ents), len(spinners)))
    for name, ids in (("a_spinners_typed", spinners), ("b_every_entity_typed", np.ascontiguousarray(ents["id"], np.uint32))):
        t0 = time.perf_counter()
        p.set_entity_types(ids, np.full(len(ids), TYPE, np.uint64))
        g = p.cull_and_pack(cam, copy=False)
        rec, n = p.logic_calls()                                     # (the first call rebuilds the listed rows)
        setup_s = time.perf_counter() - t0
        us = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); rec, n2 = p.logic_calls(capacity=n); t1 = time.perf_counter()
            assert n2 == n and len(rec) == n
            if i >= a.warmup:
                us.append((t1 - t0) * 1e6)
        st = p.stats()
        out[name] = dict(listed_rows=int(len(ids)), records=int(n), visible_instances=int(g["total"]), call_us=stats(us), set_types_cull_first_list_s=round(setup_s, 3),
                         n_seal_waits=st["n_seal_waits"], n_sync_fallbacks=st["n_sync_fallbacks"])
    print(json.dumps(out))
    p.close()


if __name__ == "__main__":
    main()

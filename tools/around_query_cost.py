"""What one re_query_boxes_around ("who is within reach of me", asked by entity id) costs against the path it replaces.  GPU.

  world lattice   bench.py's 10,077,696-entity world (configs[2]: one entity per level-0 section, every 100th rotating): no shared sections
  world mixed     synthetic.mixed_world scaled up (--mixed-n entities over a cube of +-1500 units): unique sections of several levels and shared sections
  batches         1, 64 and 4096 askers drawn among the entities, reach --reach; askers the device refuses (RE_AROUND_TOO_LARGE: re_query_boxes would
                  refuse the whole batch) are drawn again
  around_us       (i)   the new call with the hits read back: median (min / max) of --reps calls after --warmup, all in one process
  replaced_us     (ii)  the path it replaces: n x re_read_component(RE_C_STATIC_AABB), the boxes in numpy, re_query_boxes (a tenth of the repetitions for
                        the largest batch: one repetition is thousands of blocking copies)
  boxes_us        (iii) re_query_boxes alone on the boxes built beforehand: the floor the new call sits on, plus one small launch
  spheres_us      re_query_spheres_around for the same askers and reach, and sphere_floor_us: re_query_spheres on spheres built beforehand
Kernel time: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/around_query_cost.py --reps 50 --only-new`: the trace then
holds k_around_build_boxes / k_box_query_around and k_around_build_spheres / k_sphere_query alone."""
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
from segment_query_cost import stats  # noqa: E402

F32 = np.float32
OUTLINE = 16384


def timed(fn, warmup, reps):
    us = []
    for i in range(warmup + reps):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if i >= warmup:
            us.append((t1 - t0) * 1e6)
    return stats(us)


def measure(ents, atomic, a, rng):
    L = R._capi
    p = R.Pipeline(OUTLINE, atomic); p.register_model_instances(ents)
    st = p.stats()
    out = dict(entities=int(len(ents)), sections=int(st["n_sections"]), shared_sections=int(st["n_shared_sections"]))
    for n in a.batches:
        ids = ents["id"][rng.integers(0, len(ents), n)].astype(np.uint32)
        for _ in range(8):                                                 # askers the device refuses are drawn again
            _, _, status = p.find_entities_around(ids, a.reach, capacity=0)
            if not status.any():
                break
            ids[status != 0] = ents["id"][rng.integers(0, len(ents), int((status != 0).sum()))]
        assert not status.any()
        hits, total, _ = p.find_entities_around(ids, a.reach)

        def around():
            h, n2, s = p.find_entities_around(ids, a.reach, capacity=total)
            assert n2 == total and len(h) == total

        rec = dict(hits=int(total), around_us=timed(around, a.warmup, a.reps))
        sh, stotal, sstatus = p.find_entities_within_reach(ids, a.reach)
        assert not sstatus.any()
        rec["sphere_hits"] = int(stotal)
        rec["spheres_us"] = timed(lambda: p.find_entities_within_reach(ids, a.reach, capacity=stotal), a.warmup, a.reps)
        if not a.only_new:
            def build_boxes():
                boxes = np.zeros((n, 6), F32)
                for j, e in enumerate(ids):
                    ab = p.read_component(int(e), L.C_STATIC_AABB)
                    boxes[j, 0::2] = ab[0::2] - F32(a.reach); boxes[j, 1::2] = ab[1::2] + F32(a.reach)
                return boxes
            boxes = build_boxes()
            bh, btotal = p.find_entities_in_boxes(boxes)
            assert btotal == total + n                                     # the same pairs, and every asker itself
            rec["replaced_us"] = timed(lambda: p.find_entities_in_boxes(build_boxes(), capacity=btotal), 2 if n > 1000 else a.warmup, max(10, a.reps // 10) if n > 1000 else a.reps)
            rec["boxes_us"] = timed(lambda: p.find_entities_in_boxes(boxes, capacity=btotal), a.warmup, a.reps)
            sph = np.zeros((n, 4), F32)
            for j, e in enumerate(ids):
                sph[j, 0:3] = p.read_component(int(e), L.C_POSITION)
            sph[:, 3] = a.reach
            rec["sphere_floor_us"] = timed(lambda: p.find_entities_within_radius(sph, exclude=ids, capacity=stotal), a.warmup, a.reps)
        out["batch_%d" % n] = rec
    st = p.stats()
    out["n_seal_waits"], out["n_sync_fallbacks"] = st["n_seal_waits"], st["n_sync_fallbacks"]
    assert st["n_seal_waits"] == 0 and st["n_sync_fallbacks"] == 0
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096]); ap.add_argument("--reach", type=float, default=50.0)
    ap.add_argument("--mixed-n", type=int, default=200000); ap.add_argument("--worlds", nargs="+", default=["lattice", "mixed"])
    ap.add_argument("--only-new", action="store_true", help="the new calls alone (a kernel trace then holds their kernels alone)")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    out = {}
    if "lattice" in a.worlds:
        ents, dims, first = make_shard(0, 1, PER_GPU_AXIS, 64, 100)
        out["lattice"] = measure(ents, 64, a, rng)
        del ents
    if "mixed" in a.worlds:
        ents = R.synthetic.mixed_world(a.mixed_n, seed=7, spread=1500.0)
        out["mixed"] = measure(ents, 64, a, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

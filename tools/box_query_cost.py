"""What one re_query_boxes (the tree query the logic callbacks get instead of &BoundingBoxTree) costs.  GPU.

  world lattice   bench.py's 10,077,696-entity world (configs[2]: one entity per level-0 section, every 100th rotating): no shared sections
  world mixed     synthetic.mixed_world scaled up (--mixed-n entities over a cube of +-1500 units): unique sections of several levels and a shared
                  section for most of the larger entities -- the O(shared sections x queries) part of the kernel; its shared-section count is reported
  batches         1, 64 and 4096 boxes of 200 units a side around random entities
  call_us         wall time of one call with the hits read back: median (min / max) after warm-up
  cells / keys    candidate cells of the batch == keys the kernel probes (same integer arithmetic as the library)
Kernel time: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/box_query_cost.py --reps 50`; the launches of one batch
share one grid size in the kernel trace (n + ceil(shared sections / 256) * ceil(n / 256) workgroups, printed as "grid")."""
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


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2), n=int(len(xs)))


def candidate_cells(box, outline, atomic):
    """the library's count (make_box_query, re_api.hip): per level 0 .. max_level the product over the axes of the cell range of the clipped box"""
    n, max_level = 0, int(np.ceil(np.log2(np.float32(outline) / np.float32(atomic))))
    clip = np.minimum(np.maximum(np.asarray(box, np.float32), np.float32(0)), np.float32(outline))
    for level in range(max_level + 1):
        ln, p = atomic << level, 1
        for a in range(3):
            umin, umax = int(clip[2 * a]), int(clip[2 * a + 1])
            lo = umin // ln
            if np.float32(umin) == clip[2 * a] and lo > 0 and lo * ln == umin:
                lo -= 1
            p *= umax // ln - lo + 1
        n += p
    return n


def measure(name, ents, atomic, a, rng):
    p = R.Pipeline(16384, atomic); p.register_model_instances(ents)
    st = p.stats()
    out = dict(entities=int(len(ents)), sections=int(st["n_sections"]), shared_sections=int(st["n_shared_sections"]))
    for n in a.batches:
        pos = ents["pos"][rng.integers(0, len(ents), n)]
        boxes = np.zeros((n, 6), np.float32)
        for k in range(3):
            boxes[:, 2 * k] = pos[:, k] - 100.0; boxes[:, 2 * k + 1] = pos[:, k] + 100.0
        hits, total = p.find_entities_in_boxes(boxes)                 # (the first call brings the device's lookup tables up to date)
        us = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); hits, n2 = p.find_entities_in_boxes(boxes, capacity=total); t1 = time.perf_counter()
            assert n2 == total and len(hits) == total
            if i >= a.warmup:
                us.append((t1 - t0) * 1e6)
        sh_chunks = (st["n_shared_sections"] + 255) // 256
        out["batch_%d" % n] = dict(hits=int(total), keys_probed=int(sum(candidate_cells(b, 16384, atomic) for b in boxes[:min(n, 256)]) * (n / min(n, 256))),
                                   grid=int(n + sh_chunks * ((n + 255) // 256)), call_us=stats(us))
    st = p.stats()
    out["n_seal_waits"], out["n_sync_fallbacks"] = st["n_seal_waits"], st["n_sync_fallbacks"]
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096]); ap.add_argument("--mixed-n", type=int, default=200000)
    ap.add_argument("--worlds", nargs="+", default=["lattice", "mixed"])
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    out = {}
    if "lattice" in a.worlds:
        ents, dims, first = make_shard(0, 1, PER_GPU_AXIS, 64, 100)
        out["lattice"] = measure("lattice", ents, 64, a, rng)
        del ents
    if "mixed" in a.worlds:
        ents = R.synthetic.mixed_world(a.mixed_n, seed=7, spread=1500.0)
        out["mixed"] = measure("mixed", ents, 64, a, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What one re_query_spheres (who is within r of a point: an explosion, a proximity trigger, a producer looking for asteroids) costs.  GPU.

  world lattice   bench.py's 10,077,696-entity world (configs[2]: one entity per level-0 section, every 100th rotating): no shared sections
  world mixed     synthetic.mixed_world scaled up (--mixed-n entities over a cube of +-1500 units): unique sections of several levels and a shared
                  section for most of the larger entities -- the O(shared sections x spheres) part of the kernel
  batches         1, 64 and 4096 spheres of radius 50 and of radius 400, centred on random entities
  call_us         wall time of one call with the hits read back: median (min / max) after warm-up
  cells           candidate cells of the batch: those of the spheres' bounding cubes, inflated by the margin (the library's integer arithmetic)
  keys_probed     the cells the prune lets through to the key lookup (the kernel's distance test on the inflated, boundary-extended cell boxes, in numpy f32)
  box_*           what the call replaces: re_query_boxes on the spheres' raw bounding cubes -- the keys it probes (all its candidate cells), its pairs and
                  its wall time; the caller would then read back the AABBs and filter on the host
Kernel time: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/sphere_query_cost.py --reps 50 --no-boxes`; the launches
of one batch size share one grid size in the kernel trace (n + ceil(shared sections / 256) * ceil(n / 256) workgroups, printed as "grid"), the smaller
radius of a size first."""
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
from segment_query_cost import stats, level_ranges, cells_of  # noqa: E402

F32 = np.float32
OUTLINE = 16384


def dist_sq(c, boxes):
    """the squared distance of the rule from the point c to boxes [n, 6], in f32, every operation rounded once"""
    e = []
    for a in range(3):
        mn, mx = boxes[:, 2 * a], boxes[:, 2 * a + 1]
        e.append(np.where(c[a] < mn, mn - c[a], np.where(c[a] > mx, c[a] - mx, F32(0))).astype(F32))
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def sphere_cells(c, r, outline, atomic):
    """(candidate cells, cells that pass the prune, cells of the raw bounding cube) of one sphere"""
    m = F32(outline) * F32(1.0 / 4096.0)
    raw = np.zeros(6, F32); raw[0::2] = c - r; raw[1::2] = c + r
    box = raw.copy(); box[0::2] -= m; box[1::2] += m
    r2 = F32(r) * F32(r)
    total = kept = 0
    for level, axes in enumerate(level_ranges(box, outline, atomic)):
        ln = atomic << level
        grids = np.meshgrid(*[np.arange(lo, hi + 1, dtype=np.int64) for lo, hi in axes], indexing="ij")
        lc = np.stack([g.ravel() for g in grids], axis=1) * ln
        b = np.zeros((len(lc), 6), F32)
        for a in range(3):
            b[:, 2 * a] = np.where(lc[:, a] == 0, F32(-np.inf), lc[:, a].astype(F32) - m)
            b[:, 2 * a + 1] = np.where(lc[:, a] + ln >= outline, F32(np.inf), (lc[:, a] + ln).astype(F32) + m)
        total += len(lc); kept += int((dist_sq(c, b) <= r2).sum())
    return total, kept, cells_of(level_ranges(raw, outline, atomic))


def measure(ents, atomic, a, rng):
    p = R.Pipeline(OUTLINE, atomic); p.register_model_instances(ents)
    st = p.stats()
    out = dict(entities=int(len(ents)), sections=int(st["n_sections"]), shared_sections=int(st["n_shared_sections"]))
    sh_chunks = (st["n_shared_sections"] + 255) // 256
    for n in a.batches:
        for radius in a.radii:
            c = ents["pos"][rng.integers(0, len(ents), n)].astype(F32)
            sph = np.concatenate([c, np.full((n, 1), radius, F32)], axis=1)
            hits, total = p.find_entities_within_radius(sph)               # (the first call brings the device's lookup tables up to date)
            us = []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter(); hits, n2 = p.find_entities_within_radius(sph, capacity=total); t1 = time.perf_counter()
                assert n2 == total and len(hits) == total
                if i >= a.warmup:
                    us.append((t1 - t0) * 1e6)
            m = min(n, 256)
            counts = np.array([sphere_cells(c[j], F32(radius), OUTLINE, atomic) for j in range(m)], np.int64).sum(axis=0) * (n / m)
            rec = dict(hits=int(total), cells=int(counts[0]), keys_probed=int(counts[1]), box_keys_probed=int(counts[2]),
                       grid=int(n + sh_chunks * ((n + 255) // 256)), call_us=stats(us))
            if not a.no_boxes:
                boxes = np.zeros((n, 6), F32); boxes[:, 0::2] = c - F32(radius); boxes[:, 1::2] = c + F32(radius)
                bh, btotal = p.find_entities_in_boxes(boxes)
                us = []
                for i in range(3 + max(10, a.reps // 10)):                # (a tenth of the repetitions: the large batches return tens of megabytes)
                    t0 = time.perf_counter(); bh, n2 = p.find_entities_in_boxes(boxes, capacity=btotal); t1 = time.perf_counter()
                    if i >= 3:
                        us.append((t1 - t0) * 1e6)
                rec["box_hits"], rec["box_call_us"] = int(btotal), stats(us)
            out["batch_%d_radius_%d" % (n, radius)] = rec
    st = p.stats()
    out["n_seal_waits"], out["n_sync_fallbacks"] = st["n_seal_waits"], st["n_sync_fallbacks"]
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096]); ap.add_argument("--radii", type=int, nargs="+", default=[50, 400])
    ap.add_argument("--mixed-n", type=int, default=200000); ap.add_argument("--worlds", nargs="+", default=["lattice", "mixed"])
    ap.add_argument("--no-boxes", action="store_true", help="leave the re_query_boxes comparison out (a kernel trace then holds k_sphere_query alone)")
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

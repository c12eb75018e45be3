"""What one re_query_segments (what lies along a line: a shot, a line of sight, a pick ray) costs.  GPU.

  world lattice   bench.py's 10,077,696-entity world (configs[2]: one entity per level-0 section, every 100th rotating): no shared sections
  world mixed     synthetic.mixed_world scaled up (--mixed-n entities over a cube of +-1500 units): unique sections of several levels and a shared
                  section for most of the larger entities -- the O(shared sections x segments) part of the kernel
  batches         1, 64 and 4096 segments of 200 and of 1500 units in random directions, starting at random entities
  call_us         wall time of one call with the hits read back: median (min / max) after warm-up
  cells           candidate cells of the batch: those of the segments' bounding boxes, inflated by the margin (the library's integer arithmetic)
  keys_probed     the cells the prune lets through to the key lookup (the kernel's slab test on the inflated, boundary-extended cell boxes, in numpy f32)
  box_*           re_query_boxes on the segments' raw bounding boxes: the keys it probes (all its candidate cells), its hits and its wall time
Kernel time: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/segment_query_cost.py --reps 50 --no-boxes`; the launches
of one batch size share one grid size in the kernel trace (n + ceil(shared sections / 256) * ceil(n / 256) workgroups, printed as "grid"), the 200-unit
batch of a size first."""
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

F32 = np.float32
OUTLINE = 16384


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2), n=int(len(xs)))


def level_ranges(box, outline, atomic):
    """per level 0 .. max_level the cell range [(lo, hi)] * 3 of a box, as the library computes it (make_box_query, box_level_range)"""
    max_level = int(np.ceil(np.log2(F32(outline) / F32(atomic))))
    clip = np.minimum(np.maximum(np.asarray(box, F32), F32(0)), F32(outline))
    out = []
    for level in range(max_level + 1):
        ln, axes = atomic << level, []
        for a in range(3):
            umin, umax = int(clip[2 * a]), int(clip[2 * a + 1])
            lo = umin // ln
            if F32(umin) == clip[2 * a] and lo > 0 and lo * ln == umin:
                lo -= 1
            axes.append((lo, umax // ln))
        out.append(axes)
    return out


def cells_of(ranges):
    return sum(int(np.prod([hi - lo + 1 for lo, hi in axes])) for axes in ranges)


def slab(p0, d, boxes):
    lo, hi, ok = np.zeros(len(boxes), F32), np.ones(len(boxes), F32), np.ones(len(boxes), bool)
    with np.errstate(over="ignore"):
        for a in range(3):
            mn, mx = boxes[:, 2 * a], boxes[:, 2 * a + 1]
            if d[a] == 0:
                ok &= (p0[a] >= mn) & (p0[a] <= mx)
                continue
            u, v = (mn - p0[a]) / d[a], (mx - p0[a]) / d[a]
            swap = u > v
            u, v = np.where(swap, v, u), np.where(swap, u, v)
            lo = np.where(u > lo, u, lo); hi = np.where(v < hi, v, hi)
    return ok & (lo <= hi)


def segment_cells(p0, p1, outline, atomic):
    """(candidate cells, cells that pass the prune, cells of the raw bounding box) of one segment"""
    m = F32(outline) * F32(1.0 / 4096.0)
    raw = np.zeros(6, F32); raw[0::2] = np.minimum(p0, p1); raw[1::2] = np.maximum(p0, p1)
    box = raw.copy(); box[0::2] -= m; box[1::2] += m
    d = p1 - p0
    d = np.where(np.abs(d) < np.finfo(F32).tiny, F32(0), d).astype(F32)
    total = kept = 0
    for level, axes in enumerate(level_ranges(box, outline, atomic)):
        ln = atomic << level
        grids = np.meshgrid(*[np.arange(lo, hi + 1, dtype=np.int64) for lo, hi in axes], indexing="ij")
        c = np.stack([g.ravel() for g in grids], axis=1) * ln
        b = np.zeros((len(c), 6), F32)
        for a in range(3):
            b[:, 2 * a] = np.where(c[:, a] == 0, F32(-np.inf), c[:, a].astype(F32) - m)
            b[:, 2 * a + 1] = np.where(c[:, a] + ln >= outline, F32(np.inf), (c[:, a] + ln).astype(F32) + m)
        total += len(c); kept += int(slab(p0, d, b).sum())
    return total, kept, cells_of(level_ranges(raw, outline, atomic))


def measure(ents, atomic, a, rng):
    p = R.Pipeline(OUTLINE, atomic); p.register_model_instances(ents)
    st = p.stats()
    out = dict(entities=int(len(ents)), sections=int(st["n_sections"]), shared_sections=int(st["n_shared_sections"]))
    sh_chunks = (st["n_shared_sections"] + 255) // 256
    for n in a.batches:
        for length in a.lengths:
            p0 = ents["pos"][rng.integers(0, len(ents), n)].astype(F32)
            dirn = rng.normal(size=(n, 3)); dirn /= np.linalg.norm(dirn, axis=1)[:, None]
            p1 = (p0 + dirn.astype(F32) * F32(length)).astype(F32)
            seg = np.concatenate([p0, p1], axis=1)
            hits, total = p.find_entities_along_segments(seg)             # (the first call brings the device's lookup tables up to date)
            us = []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter(); hits, n2 = p.find_entities_along_segments(seg, capacity=total); t1 = time.perf_counter()
                assert n2 == total and len(hits) == total
                if i >= a.warmup:
                    us.append((t1 - t0) * 1e6)
            m = min(n, 256)
            counts = np.array([segment_cells(p0[j], p1[j], OUTLINE, atomic) for j in range(m)], np.int64).sum(axis=0) * (n / m)
            rec = dict(hits=int(total), cells=int(counts[0]), keys_probed=int(counts[1]), box_keys_probed=int(counts[2]),
                       grid=int(n + sh_chunks * ((n + 255) // 256)), call_us=stats(us))
            if not a.no_boxes:
                boxes = np.zeros((n, 6), F32); boxes[:, 0::2] = np.minimum(p0, p1); boxes[:, 1::2] = np.maximum(p0, p1)
                bh, btotal = p.find_entities_in_boxes(boxes)
                us = []
                for i in range(3 + max(10, a.reps // 10)):                # (a tenth of the repetitions: the large batches return tens of megabytes)
                    t0 = time.perf_counter(); bh, n2 = p.find_entities_in_boxes(boxes, capacity=btotal); t1 = time.perf_counter()
                    if i >= 3:
                        us.append((t1 - t0) * 1e6)
                rec["box_hits"], rec["box_call_us"] = int(btotal), stats(us)
            out["batch_%d_length_%d" % (n, length)] = rec
    st = p.stats()
    out["n_seal_waits"], out["n_sync_fallbacks"] = st["n_seal_waits"], st["n_sync_fallbacks"]
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096]); ap.add_argument("--lengths", type=int, nargs="+", default=[200, 1500])
    ap.add_argument("--mixed-n", type=int, default=200000); ap.add_argument("--worlds", nargs="+", default=["lattice", "mixed"])
    ap.add_argument("--no-boxes", action="store_true", help="leave the re_query_boxes comparison out (a kernel trace then holds k_segment_query alone)")
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

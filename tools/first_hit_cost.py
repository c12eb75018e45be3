"""What re_query_segments_first and re_query_spheres_nearest cost against the path they replace: the all-hits call plus first_hits / nearest_hits on the host.  GPU.

  worlds, batches   those of tools/segment_query_cost.py and tools/sphere_query_cost.py: the lattice (bench.py's 10,077,696-entity world) and the mixed world
                    (synthetic.mixed_world scaled up), 1 / 64 / 4096 queries, segments of length 200 and 1500, spheres of radius 50 and 400
  reduced_us        wall time of the new call: median (min / max) after warm-up; 16 bytes a query come back
  all_hits_us       wall time of the sibling with every hit read back; pick_us: first_hits / nearest_hits on those records (numpy, on the host);
                    replaced_us: the two together, call by call -- what a caller paid for the same answer.  Fewer repetitions (--old-reps) where the
                    batch returns millions of records
  found, hits       queries with a hit, records of the sibling; the two answers are compared once per row (byte for byte)
Kernel time: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/first_hit_cost.py --trace --reps 50` -- the new call, then the
sibling, nothing on the host between them -- and give the kernel trace to `--summarize FILE`: per kernel and grid size (n + ceil(shared sections / 256) *
ceil(n / 256) workgroups, printed as "grid") the median of the last two thirds of the launches of each of the two lengths / radii, the smaller one first."""
import argparse
import csv
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


def timed(fn, reps, warmup):
    us, out = [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
        if i >= warmup:
            us.append((t1 - t0) * 1e6)
    return us, out


def row(p, a, n, sh_chunks, reduced, all_hits, pick):
    """one batch: reduced() -> (records, found); all_hits(capacity) -> (hits, total); pick(hits, n) -> (records, found)"""
    _, total = all_hits(None)                                          # (the first call brings the device's lookup tables up to date)
    rec = dict(hits=int(total), grid=int(n + sh_chunks * ((n + 255) // 256)))
    if a.trace:
        timed(reduced, a.reps, a.warmup); timed(lambda: all_hits(total), a.reps, a.warmup)
        return rec
    us, got = timed(reduced, a.reps, a.warmup)
    rec["found"], rec["reduced_us"] = int(got[1].sum()), stats(us)
    old_reps = a.reps if total < 200000 else a.old_reps
    call_us, pick_us, both_us = [], [], []
    for i in range(2 + old_reps):
        t0 = time.perf_counter(); hits, n2 = all_hits(total); t1 = time.perf_counter(); want = pick(hits, n); t2 = time.perf_counter()
        assert n2 == total and len(hits) == total
        if i >= 2:
            call_us.append((t1 - t0) * 1e6); pick_us.append((t2 - t1) * 1e6); both_us.append((t2 - t0) * 1e6)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    rec["all_hits_us"], rec["pick_us"], rec["replaced_us"] = stats(call_us), stats(pick_us), stats(both_us)
    return rec


def measure(ents, atomic, a, rng):
    p = R.Pipeline(OUTLINE, atomic); p.register_model_instances(ents)
    st = p.stats()
    out = dict(entities=int(len(ents)), sections=int(st["n_sections"]), shared_sections=int(st["n_shared_sections"]))
    sh_chunks = (st["n_shared_sections"] + 255) // 256
    for n in a.batches:
        for length in a.lengths:
            p0 = ents["pos"][rng.integers(0, len(ents), n)].astype(F32)
            dirn = rng.normal(size=(n, 3)); dirn /= np.linalg.norm(dirn, axis=1)[:, None]
            seg = np.concatenate([p0, (p0 + dirn.astype(F32) * F32(length)).astype(F32)], axis=1)
            out["segments_%d_length_%d" % (n, length)] = row(p, a, n, sh_chunks, lambda: p.find_first_along_segments(seg),
                                                             lambda cap: p.find_entities_along_segments(seg, capacity=cap), R.first_hits)
        for radius in a.radii:
            c = ents["pos"][rng.integers(0, len(ents), n)].astype(F32)
            sph = np.concatenate([c, np.full((n, 1), radius, F32)], axis=1)
            out["spheres_%d_radius_%d" % (n, radius)] = row(p, a, n, sh_chunks, lambda: p.find_nearest_within_radius(sph),
                                                            lambda cap: p.find_entities_within_radius(sph, capacity=cap), R.nearest_hits)
    st = p.stats()
    out["n_seal_waits"], out["n_sync_fallbacks"] = st["n_seal_waits"], st["n_sync_fallbacks"]
    assert out["n_seal_waits"] == 0 and out["n_sync_fallbacks"] == 0, out
    p.close()
    return out


def summarize(path, parts):
    """per (kernel, grid size) of a rocprofv3 kernel trace: the launches in order, cut into `parts` equal runs (the lengths / radii of a batch size), the
    median of the last two thirds of each run, in microseconds"""
    runs = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            if "first" not in name and "nearest" not in name and name not in ("re::k_segment_query", "re::k_sphere_query", "k_segment_query", "k_sphere_query"):
                continue
            grid = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)
            runs.setdefault((name, grid), []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out = {}
    for (name, grid), xs in sorted(runs.items()):
        d = [us for _, us in sorted(xs)]
        k = len(d) // parts
        out["%s grid %d" % (name, grid)] = [dict(launches=k, median_us=round(float(np.median(d[i * k + k // 3:(i + 1) * k])), 2)) for i in range(parts) if k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--old-reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 4096]); ap.add_argument("--radii", type=int, nargs="+", default=[50, 400])
    ap.add_argument("--lengths", type=int, nargs="+", default=[200, 1500])
    ap.add_argument("--mixed-n", type=int, default=200000); ap.add_argument("--worlds", nargs="+", default=["lattice", "mixed"])
    ap.add_argument("--trace", action="store_true", help="calls only, nothing timed or picked on the host: for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--summarize", help="a rocprofv3 kernel trace (csv) of a --trace run: kernel times per kernel and grid size")
    a = ap.parse_args()
    if a.summarize:
        print(json.dumps(summarize(a.summarize, 2)))
        return
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

"""What one re_shadow_step (ShadowFlow::calculate_shadow_maps on the device) costs at configs[1] -- bench.py's 10,077,696-entity world and camera (far
1000) -- with spot lights near the camera, next to the frame's synchronous re_cull_pack.  GPU.

  step_enqueue_us   host time of one step with out == NULL (nothing waits: the call only enqueues k_shadow_select)
  step_stream_us    back-to-back steps with out == NULL, one stream synchronise at the end: wall / steps (the per-step cost in a frame loop)
  step_out_us       one step with the decision read back (waits for k_shadow_select)
  cull_pack_us      one synchronous re_cull_pack of the same world and camera
Medians (min / max) after warm-up.  Kernel times: run under `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/shadow_cost.py`."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import render_engine_amd as R  # noqa: E402
from render_engine_amd import lighting, shadow  # noqa: E402
from bench import make_shard, PER_GPU_AXIS  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2), n=int(len(xs)))


def main(reps=200, warm=20, light_radius=300.0, every=8):
    atomic = 64
    ents, dims, first = make_shard(0, 1, PER_GPU_AXIS, atomic, 0)
    centre = np.array([(first + d / 2.0) * atomic for d in (dims[0], dims[2], dims[1])], np.float32)
    near = np.nonzero(np.all(np.abs(ents["pos"] - centre) < light_radius, axis=1))[0][::every]
    ents["flags"][near] |= np.uint32(R.F_LIGHT_SPOT)
    lights = np.sort(ents["id"][near])
    p = R.Pipeline(16384, atomic); p.register_model_instances(ents)
    I = np.zeros(len(lights), R.LIGHT_INFORMATION_DT); I["radius"] = 120.0
    p.set_light_information(lights, I)
    dl = lighting.DeferredLighting(64, 64, max_spot_lights=64, max_point_lights=8)
    S = shadow.Shadow(p, n_shadow_maps=32, upload_capacity=256)
    cam = R.Camera(centre, (0.0, 0.0, -1.0), 1000.0)
    L = R._capi.load()
    sync = lambda: L.re_debug_copy_to_host(p._h, None, None, 0)   # noqa: E731  (0 bytes: a synchronise of the pipeline's stream)
    dl.set_lights_from_world(p, cam, 4); p.cull_and_pack(cam)
    enq, out_w, cull, maps = [], [], [], 0
    for i in range(warm + reps):
        sync()
        t0 = time.perf_counter(); S.step(cam, lighting=dl, wait=False); t1 = time.perf_counter()
        sync()
        t2 = time.perf_counter(); f = S.step(cam, lighting=dl); t3 = time.perf_counter()
        maps += int(f["new_map"])
        t4 = time.perf_counter(); p.cull_and_pack(cam); t5 = time.perf_counter()
        if i >= warm:
            enq.append((t1 - t0) * 1e6); out_w.append((t3 - t2) * 1e6); cull.append((t5 - t4) * 1e6)
    stream = []
    for _ in range(5):
        sync(); t0 = time.perf_counter()
        for _ in range(reps):
            S.step(cam, lighting=dl, wait=False)
        sync(); stream.append((time.perf_counter() - t0) * 1e6 / reps)
    print(json.dumps(dict(workload="configs[1]: %d static entities, far 1000, %d spot lights within %g of the camera" % (len(ents), len(lights), light_radius),
                          nearby_spot_lights=int(len(p.visible_lights(cam, R.F_LIGHT_SPOT))), step_enqueue_us=stats(enq), step_stream_us=stats(stream),
                          step_out_us=stats(out_w), cull_pack_us=stats(cull), new_maps=maps, shadow_stats=S.stats())))
    S.close(); dl.close(); p.close()


if __name__ == "__main__":
    main()

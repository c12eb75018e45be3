"""configs[4] size (4,096 spot lights, 4096x4096 G-buffer): what one frame's light upload costs by the host route it replaces -- re_visible_lights for
the three types, one re_read_component(Position) per selected light, re_lighting_set_lights -- against re_lighting_set_lights_from_world, and K5 with
its parameters from the device block against K5 host-fed.  Medians over repeated calls after warm-up, with min / max.  GPU."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import render_engine_amd as R  # noqa: E402
from render_engine_amd import lighting  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2), n=int(len(xs)))


def main(reps=30, warm=5):
    n = 4096
    L = lighting.synthetic_lights(n_spot=n, n_point=0)
    ents = np.zeros(n, R.ENTITY_DT)
    ents["id"] = np.arange(n, dtype=np.uint32); ents["flags"] = R.F_LIGHT_SPOT; ents["pos"] = L["spot_pos"]
    ents["original"] = np.array([-0.5, 0.5, -0.5, 0.5, -0.5, 0.5], np.float32); ents["scale"] = 1.0; ents["rot_axis"] = (1.0, 0.0, 0.0)
    p = R.Pipeline(16384, 64); p.register_model_instances(ents)
    I = np.zeros(n, R.LIGHT_INFORMATION_DT)
    I["radius"] = L["spot_radius"]; I["diffuse"] = L["spot_diffuse"]; I["specular"] = L["spot_specular"]; I["ambient"] = L["spot_ambient"]
    I["linear"] = L["spot_linear"]; I["quadratic"] = L["spot_quadratic"]
    p.set_light_information(ents["id"], I)
    gb = lighting.synthetic_gbuffer(4096, 4096)
    A = lighting.DeferredLighting(4096, 4096, max_spot_lights=n, max_point_lights=64); A.upload_gbuffer(*gb)
    B = lighting.DeferredLighting(4096, 4096, max_spot_lights=n, max_point_lights=64); B.upload_gbuffer(*gb)
    cam = R.Camera(L["camera_pos"], (0.0, 0.0, -1.0), 2048.0)
    pos = np.zeros(3, np.float32)

    def host_route():
        ids = [p.visible_lights(cam, t) for t in (R.F_LIGHT_DIRECTIONAL, R.F_LIGHT_POINT, R.F_LIGHT_SPOT)]
        sp = np.zeros((len(ids[2]), 3), np.float32)
        for k, e in enumerate(ids[2]):
            p._check(p._L.re_read_component(p._h, int(e), R._capi.C_POSITION, pos.ctypes.data), "re_read_component"); sp[k] = pos
        M = dict(L); M["spot_pos"] = sp
        B.set_lights(M)

    out = {}
    for name, fn in (("host_route_us", host_route), ("from_world_us", lambda: A.set_lights_from_world(p, cam, 8, wait=False)),
                     ("from_world_with_out_us", lambda: A.set_lights_from_world(p, cam, 8, wait=True))):
        ts = []
        for i in range(warm + reps):
            t0 = time.perf_counter(); fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        out[name] = stats(ts[warm:])
    # (wait=False returns with the two launches in flight: their device time shows in the next call, whose resolve() settles the stream)
    A.set_lights_from_world(p, cam, 8, wait=True); B.set_lights(L)
    ka, kb = [], []
    for i in range(warm + reps):                                              # alternating, so drift hits both alike
        ka.append(A.run()); kb.append(B.run())
    out["k5_device_params_us"] = stats(ka[warm:]); out["k5_host_fed_us"] = stats(kb[warm:])
    out["images_identical"] = bool(np.array_equal(A.read_pixels(np.arange(0, 4096 * 4096, 997, dtype=np.uint32)),
                                                  B.read_pixels(np.arange(0, 4096 * 4096, 997, dtype=np.uint32))))
    print(json.dumps(out))
    A.close(); B.close(); p.close()


if __name__ == "__main__":
    main()

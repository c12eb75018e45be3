"""ShadowFlow::calculate_shadow_maps (flows/shadow_flow.rs:111-453) on the device: re_shadow_* of include/re_hip.h.

One Shadow object is one RenderFlow's shadow flow over one Pipeline's world.  A frame calls step() before the lighting context's
set_lights_from_world(), as RenderFlow::render runs calculate_shadow_maps before RenderSystem::draw uploads the lights."""
import ctypes as C

import numpy as np

from . import _capi
from .pipeline import RenderEngineError

DIRECTIONAL, POINT, SPOT = _capi.WL_DIRECTIONAL, _capi.WL_POINT, _capi.WL_SPOT
NONE = 0xFFFFFFFF


class Shadow:
    def __init__(self, pipeline, n_shadow_maps=6, upload_capacity=64):
        self._L = _capi.load()
        self._pipeline = pipeline                       # (the world context must outlive the shadow flow)
        cfg = _capi.ShadowConfig(n_shadow_maps, upload_capacity)
        h = C.c_void_p()
        rc = self._L.re_shadow_create(pipeline._h, C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RenderEngineError(f"re_shadow_create failed ({rc}): {self._L.re_shadow_last_error(None).decode()}")
        self._h = h

    def _check(self, rc, what):
        if rc != 0:
            raise RenderEngineError(f"{what} failed ({rc}): {self._L.re_shadow_last_error(self._h).decode()}")

    def step(self, camera, window=(1280, 720), lighting=None, wait=True):
        """one calculate_shadow_maps.  wait=True returns the frame as a dict (new_map, light_type, entity_id, face, texture_index, n_uploads and
        the matrices / planes / box as float32 arrays); wait=False returns None and leaves the step in flight on the pipeline's stream"""
        cam = camera if isinstance(camera, _capi.CameraC) else camera.to_c()
        args = _capi.ShadowArgs(int(window[0]), int(window[1]))
        out = _capi.ShadowFrame() if wait else None
        self._check(self._L.re_shadow_step(self._h, lighting._h if lighting is not None else None, C.byref(cam), C.byref(args), 0,
                                           C.byref(out) if wait else None), "re_shadow_step")
        if not wait:
            return None
        f = {k: int(getattr(out, k)) for k in ("new_map", "light_type", "entity_id", "face", "texture_index", "n_uploads")}
        f["new_map"] = bool(f["new_map"])
        for k, shape in (("light_projection_view", (16,)), ("light_view", (16,)), ("culler", (16,)), ("planes", (6, 4)), ("box", (6,)), ("position", (3,))):
            f[k] = np.array(getattr(out, k), np.float32).reshape(shape)
        f["far_draw"] = np.float32(out.far_draw)
        return f

    def uploads(self, capacity=64):
        """the last entries of upload_matrices / upload_view_matrices / upload_indexes, oldest first"""
        m = np.zeros((capacity, 16), np.float32); v = np.zeros((capacity, 16), np.float32); i = np.zeros(capacity, np.uint32); n = C.c_uint32()
        self._check(self._L.re_shadow_uploads(self._h, m.ctypes.data, v.ctypes.data, i.ctypes.data, capacity, C.byref(n)), "re_shadow_uploads")
        return m[:n.value], v[:n.value], i[:n.value]

    def stats(self):
        s = _capi.ShadowStats()
        self._check(self._L.re_shadow_get_stats(self._h, C.byref(s)), "re_shadow_get_stats")
        return dict(n_steps=s.n_steps, n_host_waits=s.n_host_waits, n_column_uploads=s.n_column_uploads)

    def close(self):
        if getattr(self, "_h", None):
            self._L.re_shadow_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""CPU restatement of ShadowFlow::calculate_shadow_maps (flows/shadow_flow.rs:111-453) for the tests of re_shadow_step: the round-robin state machine,
find_next_light_to_have_shadow_map and the light cameras' parameters.  Hash order -> ascending EntityId (sets and maps), as the library does."""
from collections import deque

DIRECTIONAL, POINT, SPOT = 0, 1, 2
NONE = 0xFFFFFFFF
# handle_spot_light's tables (:300-320)
SPOT_DIRS = ((-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
SPOT_UPS = ((0.0, -1.0, 0.0), (0.0, 0.0, -1.0), (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0))


class ShadowPanic(Exception):
    """where the reference unwraps a None (the library returns RE_E_STATE naming the light)"""
    def __init__(self, entity_id):
        super().__init__(f"light {entity_id}")
        self.entity_id = entity_id


class ShadowFlowRule:
    def __init__(self, n_shadow_maps=6):
        self.type, self.cur = DIRECTIONAL, None
        self.maps = {POINT: {}, SPOT: {}}             # EntityId -> [Option<usize>; 6]; directional_lights is never filled
        self.free = deque(range(n_shadow_maps))
        self.uploads = []                             # (light id, face, texture index): upload_matrices / _view_matrices / _indexes grow together

    def _find(self, t, nearby, visible):
        if not self.free:
            return None
        m = self.maps[t]
        for e in sorted(m):                           # lights no longer nearby give their indexes back
            if e not in nearby:
                for x in m.pop(e):
                    if x is not None:
                        self.free.append(x)
        priority = None
        for x in sorted(visible):                     # the LAST visible light without a map
            if x not in m:
                priority = x
        if priority is not None:
            return priority
        for x in sorted(nearby):                      # else the first nearby light that is not visible
            if x not in visible:
                return x
        return None

    def step(self, nearby, visible, dir_candidates=(), info=None):
        """nearby[t] / visible[t]: sets of ids per type; dir_candidates: live entities with sortable index 1; info(id) -> dict of what the light
        carries (keys radius, direction, fov; missing key = None) or None.  Returns None (NoNewMapRequired) or a dict with type, id, face, index and
        the light camera (kind, direction, up, fov, aspect, near, far).  Raises ShadowPanic and leaves the state unchanged where the reference panics."""
        info = info or (lambda e: {"radius": 100.0, "direction": (0.0, -1.0, 0.0), "fov": 45.0})
        saved = (self.type, self.cur, {t: {k: list(v) for k, v in m.items()} for t, m in self.maps.items()}, deque(self.free), list(self.uploads))
        try:
            return self._step(nearby, visible, dir_candidates, info)
        except ShadowPanic:
            self.type, self.cur, self.maps, self.free, self.uploads = saved
            raise

    def _need(self, e, info, keys):
        I = info(e)
        if I is None or any(I.get(k) is None for k in keys):
            raise ShadowPanic(e)
        return I

    def _step(self, nearby, visible, dir_candidates, info):
        if self.type == DIRECTIONAL:
            cur = self.cur
            if cur is None:
                if not self.free:
                    self.type = POINT
                    return None
                for e in sorted(dir_candidates):
                    cur = e; self.cur = e
                    break
            if cur is None:
                self.type = POINT
                return None
            if not self.free:
                raise ShadowPanic(cur)
            I = self._need(cur, info, ("direction",))
            idx = self.free.popleft()
            return dict(type=DIRECTIONAL, id=cur, face=None, index=idx, kind="ortho", direction=I["direction"], up=(0.0, 1.0, 0.0), far=I["radius"])
        if self.type == POINT:
            cur = self.cur
            if cur is None:
                cur = self._find(POINT, nearby[POINT], visible[POINT]); self.cur = cur
                if cur is not None:
                    self.maps[POINT][cur] = [None] * 6
            if cur is None:
                self.type = SPOT
                return None
            if not self.free:
                return None
            I = self._need(cur, info, ("direction", "fov"))
            idx = self.free.popleft()
            return dict(type=POINT, id=cur, face=None, index=idx, kind="perspective", direction=I["direction"], up=(0.0, 1.0, 0.0), fov=I["fov"],
                        near=0.1, far=I["radius"])
        cur = self.cur
        if cur is None:
            cur = self._find(SPOT, nearby[SPOT], visible[SPOT]); self.cur = cur
            if cur is not None:
                self.maps[SPOT][cur] = [None] * 6
        if cur is None:
            self.type = DIRECTIONAL
            return None
        slots = self.maps[SPOT][cur]
        if None not in slots:
            self.type, self.cur = DIRECTIONAL, None
            return None
        face = slots.index(None)
        if not self.free:
            return None
        I = self._need(cur, info, ())
        idx = self.free.popleft()
        slots[face] = idx
        self.uploads.append((cur, face, idx))
        return dict(type=SPOT, id=cur, face=face, index=idx, kind="perspective", direction=SPOT_DIRS[face], up=SPOT_UPS[face], fov=90.0, near=0.10,
                    far=I["radius"], aspect=1.0)

"""CPU restatement of RenderSystem::upload_{directional,point,spot}_lights (render_system/render_system.rs:681-845) for the tests of
re_lighting_set_lights_from_world: the slot rule with its previous sets, and the uniform arrays it leaves, in the layout re_lighting_set_lights takes."""
import numpy as np

TYPE_FLAGS = (0x2000, 0x4000, 0x8000)        # RE_F_LIGHT_DIRECTIONAL, _POINT, _SPOT == RE_WL_* order


def upload_slots(previous, nearby, max_lights):
    """one upload_*_lights: (slots or None, next previous set).  Empty nearby: the function returns false before it touches anything"""
    nearby = [int(x) for x in nearby]
    if not nearby:
        return None, previous
    existing = sorted(previous & set(nearby))                     # previous ∩ nearby, ascending (the stand-in for hash order)
    slots = (existing + nearby)[:min(len(nearby), max_lights)]    # existing.iter().chain(nearby.iter()).take(N): a light can appear twice
    return slots, set(slots)


def empty_arrays():
    z3, z1, z4 = np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros((0, 4), np.float32)
    return dict(n_spot=0, n_point=0, spot_pos=z3, spot_diffuse=z3, spot_specular=z3, spot_ambient=z4, spot_linear=z1, spot_quadratic=z1, spot_radius=z1,
                point_pos=z3, point_dir=z3, point_diffuse=z3, point_specular=z3, point_ambient=z4, point_linear=z1, point_quadratic=z1, point_cutoff=z1,
                point_outer_cutoff=z1, camera_pos=np.zeros(3, np.float32), no_light_source_cutoff=0.2, default_diffuse_factor=0.2, any_light_source_visible=0)


def spot_arrays(slots, pos_of, info_of, max_spot):
    """numberSpotLights = max_spot_lights: slots past the selection stay zero (position, colours, radius)"""
    L = dict(n_spot=max_spot, spot_pos=np.zeros((max_spot, 3), np.float32), spot_diffuse=np.zeros((max_spot, 3), np.float32),
             spot_specular=np.zeros((max_spot, 3), np.float32), spot_ambient=np.zeros((max_spot, 4), np.float32), spot_linear=np.zeros(max_spot, np.float32),
             spot_quadratic=np.zeros(max_spot, np.float32), spot_radius=np.zeros(max_spot, np.float32))
    for s, e in enumerate(slots):
        I = info_of(e)
        L["spot_pos"][s] = pos_of(e); L["spot_diffuse"][s] = I["diffuse"]; L["spot_specular"][s] = I["specular"]; L["spot_ambient"][s] = I["ambient"]
        L["spot_linear"][s] = I["linear"]; L["spot_quadratic"][s] = I["quadratic"]; L["spot_radius"][s] = I["radius"]
    return L


def point_arrays(slots, pos_of, info_of):
    """numberPointLights = N"""
    n = len(slots)
    L = dict(n_point=n, point_pos=np.zeros((n, 3), np.float32), point_dir=np.zeros((n, 3), np.float32), point_diffuse=np.zeros((n, 3), np.float32),
             point_specular=np.zeros((n, 3), np.float32), point_ambient=np.zeros((n, 4), np.float32), point_linear=np.zeros(n, np.float32),
             point_quadratic=np.zeros(n, np.float32), point_cutoff=np.zeros(n, np.float32), point_outer_cutoff=np.zeros(n, np.float32))
    for s, e in enumerate(slots):
        I = info_of(e)
        L["point_pos"][s] = pos_of(e); L["point_dir"][s] = I["direction"]; L["point_diffuse"][s] = I["diffuse"]; L["point_specular"][s] = I["specular"]
        L["point_ambient"][s] = I["ambient"]; L["point_linear"][s] = I["linear"]; L["point_quadratic"][s] = I["quadratic"]
        L["point_cutoff"][s] = I["cutoff"]; L["point_outer_cutoff"][s] = I["outer_cutoff"]
    return L


class RenderSystemLights:
    """one render system's second-pass uniforms and its three previous sets, frame after frame"""

    def __init__(self, max_directional, max_point, max_spot):
        self.max = [max_directional, max_point, max_spot]
        self.previous = [set(), set(), set()]
        self.arrays = empty_arrays()

    def frame(self, nearby, pos_of, info_of, camera_pos, no_light_source_cutoff=0.2, default_diffuse_factor=0.2):
        """nearby: three ascending id lists (directional, point, spot).  Returns the per-type slots (None = not written) and anyLightSourceVisible;
        self.arrays is then what the shader sees"""
        slots = []
        for t in range(3):
            s, self.previous[t] = upload_slots(self.previous[t], nearby[t], self.max[t])
            slots.append(s)
        if slots[1] is not None:
            self.arrays.update(point_arrays(slots[1], pos_of, info_of))
        if slots[2] is not None:
            self.arrays.update(spot_arrays(slots[2], pos_of, info_of, self.max[2]))
        anyv = any(s is not None for s in slots)
        self.arrays.update(camera_pos=np.asarray(camera_pos, np.float32), no_light_source_cutoff=no_light_source_cutoff,
                           default_diffuse_factor=default_diffuse_factor, any_light_source_visible=int(anyv))
        return slots, anyv

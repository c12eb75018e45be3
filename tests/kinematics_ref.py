"""A float64 restatement of the reference's kinematics, written from its Rust source: registration (exports/entity_transformer.rs:55-142,
exports/movement_components.rs:108-164), one tick (flows/logic_flow.rs:366-448, movement_components.rs:210-299), the box and matrix after a
kinematic change (helper_things/entity_change_helpers.rs:217-262, world/bounding_volumes/aabb.rs:95-114) and the section decision of a box
(world/bounding_box_tree_v2.rs:451-551, 563-581, 1315-1397).  Nothing here is taken from the kernels, the oracle or their shared arithmetic: the
ECS tick, the registration transform and sin/cos of the device and of the oracle are measured against this file.

Also here, because the CPU and the GPU tests must use the same ones: the worlds and argument lists of those tests (seeded, so both see one input).

Matrices are column-major 16-vectors (m[col * 4 + row]) where they meet the project's; boxes are (xmin, xmax, ymin, ymax, zmin, zmax)."""
import numpy as np

F32 = np.float32

# one entity as EntityTransformationBuilder fills it (the project's upload record, 140 bytes) and the bits of its `flags` (include/re_hip.h)
ENTITY_DT = np.dtype([
    ("id", "u4"), ("model_index", "u4"), ("render_system", "u4"), ("sortable", "u4"), ("flags", "u4"),
    ("original", "f4", 6), ("pos", "f4", 3), ("rot_axis", "f4", 3), ("rot_angle", "f4"), ("scale", "f4", 3),
    ("vel", "f4", 3), ("acc", "f4", 3), ("rotvel_axis", "f4", 3), ("rotvel", "f4"), ("rotacc_axis", "f4", 3), ("rotacc", "f4"),
])
F_STATIC, F_HAS_VEL, F_HAS_ACC, F_HAS_ROT, F_HAS_ROTVEL, F_HAS_ROTACC, F_HAS_SCALE, F_ALWAYS_EXEC = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
F_OOB_LOGIC, F_HAS_MOVED, F_HAS_ROTATED = 0x100, 0x200, 0x400


def blank_entities(n):
    e = np.zeros(n, ENTITY_DT)
    e["rot_axis"][:, 0] = 1; e["rotvel_axis"][:, 0] = 1; e["rotacc_axis"][:, 0] = 1; e["scale"][:] = 1
    return e


def ulp32(x):
    """the spacing of f32 at the largest magnitude in x (at least the smallest subnormal), as a float64"""
    return float(np.spacing(F32(np.max(np.abs(x))))) or 1.4e-45


# ---------------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def normalize(v):
    return v / np.sqrt(v @ v)


def rotation(axis, angle):
    """right-handed rotation by `angle` about the unit vector `axis` (Rodrigues), 3x3"""
    u = axis
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * np.outer(u, u)


def trs(pos, axis=None, angle=0.0, scale=None):
    """translate(I, pos) * rotate(angle, axis) * scale(scale) as a 4x4 [row, col]; a factor is present only when its argument is"""
    M = np.eye(4); M[:3, 3] = pos
    if axis is not None:
        R = np.eye(4); R[:3, :3] = rotation(axis, angle); M = M @ R
    if scale is not None:
        M = M @ np.diag([scale[0], scale[1], scale[2], 1.0])
    return M


def two_corner_box(orig, M):
    """StaticAABB::apply_transformation: the min corner and the max corner are transformed, and the box is spanned by those two points"""
    a = M @ np.array([orig[0], orig[2], orig[4], 1.0]); b = M @ np.array([orig[1], orig[3], orig[5], 1.0])
    return np.array([min(a[0], b[0]), max(a[0], b[0]), min(a[1], b[1]), max(a[1], b[1]), min(a[2], b[2]), max(a[2], b[2])])


class Body:
    """the components of one entity in float64, starting from the f32 values of its upload record"""

    def __init__(self, rec):
        f = lambda k: np.asarray(rec[k], np.float64)
        self.id, self.flags = int(rec["id"]), int(rec["flags"])
        has = lambda bit: bool(self.flags & bit)
        self.has_vel, self.has_acc, self.has_rot, self.has_scale = has(F_HAS_VEL), has(F_HAS_ACC), has(F_HAS_ROT), has(F_HAS_SCALE)
        self.has_rotvel, self.has_rotacc = has(F_HAS_ROTVEL), has(F_HAS_ROTACC)
        assert not self.has_acc or self.has_vel                                   # check_invariants (entity_transformer.rs:77-97)
        assert not self.has_rotvel or self.has_rot
        assert not self.has_rotacc or (self.has_rotvel and self.has_rot)
        self.orig, self.pos = f("original"), f("pos")
        self.rot_axis = normalize(f("rot_axis")) if self.has_rot else np.array([1.0, 0.0, 0.0])      # Rotation::new normalises; ::default is (+x, 0)
        self.angle = float(rec["rot_angle"]) if self.has_rot else 0.0
        self.scale = f("scale") if self.has_scale else np.ones(3)
        self.vel, self.acc = f("vel"), f("acc")
        self.w_axis, self.w = normalize(f("rotvel_axis")), float(rec["rotvel"])                      # VelocityRotation::new normalises
        self.a_axis, self.aw = normalize(f("rotacc_axis")), float(rec["rotacc"])                     # AccelerationRotation::new normalises
        # apply_choices: only the supplied components enter the matrix
        self.M = trs(self.pos, self.rot_axis if self.has_rot else None, self.angle, self.scale if self.has_scale else None)
        self.box = two_corner_box(self.orig, self.M)

    def tick(self, dt):
        """apply_kinematics, then update_aabb_after_kinematic_change; returns (position written, rotation written)"""
        moved = rotated = False
        if self.has_vel:
            v_old = self.vel
            if self.has_acc and np.sqrt(self.acc @ self.acc) != 0.0:
                self.vel = v_old + self.acc * dt
            # the reference reads Velocity again after queueing the change: the ECS still holds the old one (changes apply at the end of the frame)
            if np.sqrt(v_old @ v_old) != 0.0:
                self.pos = self.pos + v_old * dt
                moved = True
        if self.has_rotvel:
            w_axis_old, w_old = self.w_axis, self.w
            if self.has_rotacc and self.aw != 0.0:
                # AccelerationRotation * dt = ::new(axis * dt, a * dt), which normalises; += adds axis and amount, then normalises the axis
                self.w_axis = normalize(w_axis_old + normalize(self.a_axis * dt))
                self.w = w_old + self.aw * dt
            if w_old != 0.0:
                self.rot_axis = normalize(self.rot_axis + normalize(w_axis_old * dt))
                self.angle = self.angle + w_old * dt
                rotated = True
        if moved and not rotated:
            # only_translation_changed_entities: column 3 overwritten, box = OriginalAABB + position; rotation and scale are NOT applied to the box
            self.M = self.M.copy(); self.M[:3, 3] = self.pos
            self.box = self.orig + np.repeat(self.pos, 2)
        elif rotated:
            self.M = trs(self.pos, self.rot_axis, self.angle, self.scale)          # all three factors, defaults where a component is absent
            self.box = two_corner_box(self.orig, self.M)
        return moved, rotated


def sections_1d(mn, mx, length):
    """the closure of calculate_number_world_sections_each_dimension (bounding_box_tree_v2.rs:1315-1346)"""
    if np.trunc(mn / length) == np.trunc(mx / length):
        return 1
    n = 0
    if np.ceil(mn / length) > mn / length:
        mn = np.ceil(mn / length) * length; n = 1
    while mn < mx:
        n += 1; mn += length
    return n


def _level(box, atomic):
    length, level = atomic, 0
    while np.prod([sections_1d(box[2 * k], box[2 * k + 1], length) for k in range(3)]) > 1:
        length *= 2; level += 1
    return level, length


def section_decision(box, outline, atomic):
    """BoundingBoxTree::add_entity up to the choice of section: (out_of_bounds, keys) with keys the sorted (level, x, z, y) of the unique section,
    or of the 2..8 sections a shared section links.  For boxes whose numbers are exact in f32 (the f32 decision is then this one)."""
    box = np.asarray(box, np.float64)
    oob = bool(np.any(box < 0.0) or np.any(box > outline))
    box = np.clip(box, 0.0, float(outline))
    level, length = _level(np.array([0.0, box[1] - box[0], 0.0, box[3] - box[2], 0.0, box[5] - box[4]]), atomic)   # find_aabb_level_from_length
    nx, ny, nz = (sections_1d(box[2 * k], box[2 * k + 1], length) for k in range(3))
    if nx * ny * nz == 1:
        level, length = _level(box, atomic)                                       # find_unique_world_section_id: the level of the box where it lies
        return oob, [(level, int(box[0]) // length, int(box[4]) // length, int(box[2]) // length)]
    keys = [(level, (int(box[0]) + length * x) // length, (int(box[4]) + length * z) // length, (int(box[2]) + length * y) // length)
            for x in range(nx) for y in range(ny) for z in range(nz)]
    return oob, sorted(keys)


def pack_key(level, x, z, y):
    return (level << 48) | (x << 32) | (z << 16) | y


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs of the tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _within_120_degrees(rng, of):
    """random unit vectors at most 120 degrees from the unit vectors `of`: a sum of the two never cancels"""
    v = _units(rng, len(of))
    return np.where((np.sum(v * of, axis=1) < -0.5)[:, None], -v, v)


def random_bodies(n, seed, first_id=10):
    """n entities inside level-0 sections around the middle of a 16384 / 64 world: all combinations of Velocity / Acceleration / VelocityRotation /
    AccelerationRotation the reference admits (index bits 0..3), every third with Scale, every fifth with Rotation; |v| <= 20 per axis, |a| <= 5,
    scale 0.5..2.5, angle +-6, rates +-3 and +-1; positions 64 c + 32 +- 8 with c in 120..135; axis pairs that get summed at most 120 degrees apart"""
    rng = np.random.default_rng(seed)
    e = blank_entities(n)
    e["id"] = np.arange(n) + first_id
    for i in range(n):
        b, fl = i % 16, 0
        if b & 1: fl |= F_HAS_VEL
        if (b & 2) and (b & 1): fl |= F_HAS_ACC
        if b & 4: fl |= F_HAS_ROTVEL | F_HAS_ROT
        if (b & 8) and (b & 4): fl |= F_HAS_ROTACC
        if i % 3 == 0: fl |= F_HAS_SCALE
        if i % 5 == 0: fl |= F_HAS_ROT
        e["flags"][i] = fl
    e["original"][:] = np.array([-1, 2, -3, 1, -0.5, 4], F32) * rng.uniform(0.3, 1.0, (n, 1))
    e["pos"] = rng.integers(120, 136, (n, 3)) * 64 + 32 + rng.uniform(-8, 8, (n, 3))
    e["rot_axis"] = _units(rng, n) * rng.uniform(0.5, 3, (n, 1)); e["rot_angle"] = rng.uniform(-6, 6, n)
    e["scale"] = np.where((e["flags"] & F_HAS_SCALE)[:, None] != 0, rng.uniform(0.5, 2.5, (n, 3)), 1.0)
    e["vel"] = rng.uniform(-20, 20, (n, 3)); e["acc"] = rng.uniform(-5, 5, (n, 3))
    ra = e["rot_axis"] / np.linalg.norm(e["rot_axis"], axis=1, keepdims=True)
    wa = _within_120_degrees(rng, ra)
    e["rotvel_axis"] = wa * 2; e["rotvel"] = rng.uniform(-3, 3, n)
    e["rotacc_axis"] = _within_120_degrees(rng, wa) * 0.7; e["rotacc"] = rng.uniform(-1, 1, n)
    return e


def world96():
    """the 96 entities of the three-tick test; entities 1, 3, 4 and 12 have zero velocity / acceleration / rotation rate / rotation acceleration"""
    e = random_bodies(96, seed=3)
    e["vel"][1] = 0; e["acc"][3] = 0; e["rotvel"][4] = 0; e["rotacc"][12] = 0
    return e


WORLD96_CAMERA = dict(position=(8192.0, 8192.0, 12192.0), direction=(0.0, 0.0, -1.0), far=8000.0)
WORLD96_DT = 0.016
WORLD96_CHANGED = (70, 70, 70)          # by the rule: entities with a non-zero velocity or rotation rate, each tick


def _near_quarter_turns(kmax):
    k = np.arange(-kmax, kmax + 1)
    near = (k * np.pi / 2).astype(F32)
    return np.concatenate([near, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf))])


def sincos_arguments(n_uniform=20000, kmax=4000, n_mid=20000, n_high=20000, n_beyond=200, seed=11):
    """(small, high, beyond) f32 arguments: small = uniform in +-50, float32(k pi / 2) and both neighbours for |k| <= kmax, log-uniform in 1e3..1e6,
    +-0 and two tiny values, the last f32 below 1e6; high = 1e6, the next f32 above and log-uniform in 1e6..2^26 (both signs); beyond = above 2^26"""
    rng = np.random.default_rng(seed)
    small = np.concatenate([rng.uniform(-50, 50, n_uniform).astype(F32), _near_quarter_turns(kmax),
                            (10.0 ** rng.uniform(3, 6, n_mid) * rng.choice([-1.0, 1.0], n_mid)).astype(F32),
                            np.array([0.0, -0.0, 1e-45, -1e-45, 1e-30, 999999.9], F32)])
    small = small[np.abs(small) < F32(1e6)]
    high = np.concatenate([np.array([1e6, np.nextafter(F32(1e6), F32(np.inf)), 2.0 ** 26, -1e6], F32),
                           (2.0 ** rng.uniform(np.log2(1e6), 26, n_high) * rng.choice([-1.0, 1.0], n_high)).astype(F32)])
    high = high[(np.abs(high) >= F32(1e6)) & (np.abs(high) <= F32(2.0 ** 26))]
    beyond = np.concatenate([np.array([np.nextafter(F32(2.0 ** 26), F32(np.inf)), 1e9, 1e10, 1e12, 1e20, 3.0e38, -3.4e38], F32),
                             (10.0 ** rng.uniform(np.log10(2.0 ** 26) + 0.001, 38, n_beyond - 7) * rng.choice([-1.0, 1.0], n_beyond - 7)).astype(F32)])
    return small, high, beyond


def sincos_bounds(x):
    """float64 sin and cos of the f32 arguments x, and the bound of each: 1 f32 ulp of the float64 value rounded to f32 for |x| < 1e6; up to 2^26 half an
    ulp of 1 plus the error of the double 2 pi, 2.449e-16 per turn = 3.9e-17 per unit of argument; beyond 2^26 nothing but [-1, 1] (bound 2)"""
    x64 = np.asarray(x, np.float64); ax = np.abs(x64)
    s, c = np.sin(x64), np.cos(x64)
    one_ulp = lambda r: np.maximum(np.spacing(np.abs(r.astype(F32))).astype(np.float64), 1.4e-45)
    mid = 2.0 ** -25 + ax * 3.9e-17
    pick = lambda r: np.where(ax < 1e6, one_ulp(r), np.where(ax <= 2.0 ** 26, mid, 2.0))
    return s, c, pick(s), pick(c)


# ---- exact section edges -----------------------------------------------------------------------------------------------------------------
# Unit boxes (-1, 1)^3 with a velocity along one axis (x or z) and one tick of 0.5.  Positions are written in units of the cell size A, so one
# table serves every world: at 16384 / 64 it reads 8224 -> 8247, 8257, 8256, 8255.5, 8225, 8352, 16352 -> 16383, 16384, 32 -> 1, 0, and at
# 12288 / 96 it holds 6192 -> 6239, 6241, 6240, 6193 and 12240 -> 12287, 12288.
# (name, start cell, start offset, end cell, end offset, extra flags, expected): the moving coordinate goes from A * cell + offset to
# A * end cell + end offset; expected = ("unique", cell) | ("shared", cell, cell + 1) | ("removed",) along the moving axis, after the tick.
def edge_cases(outline, atomic):
    A, last, mid, h = atomic, outline // atomic - 1, (outline // 2) // atomic, atomic // 2
    return [
        ("A inside, 8 short of the wall", mid, h, mid, A - 9, 0, ("unique", mid)),
        ("A1 max edge on the wall", mid, h, mid, A - 1, 0, ("unique", mid)),
        ("B min edge on the wall", mid, h, mid + 1, 1, 0, ("unique", mid + 1)),
        ("C centre on the wall", mid, h, mid + 1, 0, 0, ("shared", mid, mid + 1)),
        ("D half a unit across", mid, h, mid, A - 0.5, 0, ("shared", mid, mid + 1)),
        ("G stays", mid, h, mid, h + 1, 0, ("unique", mid)),
        ("H two cells on", mid, h, mid + 2, h, 0, ("unique", mid + 2)),
        ("E0 max edge on the world face", last, h, last, A - 1, 0, ("unique", last)),
        ("E1 max edge one beyond", last, h, last + 1, 0, 0, ("removed",)),
        ("E2 one beyond, OutOfBoundsLogic", last, h, last + 1, 0, F_OOB_LOGIC, ("unique", last)),
        ("F0 min edge on the world face", 0, h, 0, 1, 0, ("unique", 0)),
        ("F1 min edge one beyond", 0, h, 0, 0, 0, ("removed",)),
        ("F2 one beyond, OutOfBoundsLogic", 0, h, 0, 0, F_OOB_LOGIC, ("unique", 0)),
    ]


EDGE_DT = 0.5


def edge_camera(outline, atomic):
    """a camera that sees the cases in the middle of the world (every case is AlwaysExecute: the tick does not depend on it)"""
    m = float(outline // 2)
    return dict(position=(m, m + 6.0 * atomic, m + 25.0 * atomic), direction=(0.0, 0.0, -1.0), far=50.0 * atomic)


# every case moves; B, C, D and H change section; E1 and F1 leave the world.  (The table of the 16384 / 64 world in the issue has twelve rows; A1, the
# 12288 / 96 table's "max edge on the wall", is the thirteenth in every world.)
EDGE_TOTALS = dict(n_changed=13, n_rebucket=4, n_out_of_bounds=2)


def edge_world(outline, atomic, axis, moving=True):
    """(entities, end positions, cases): one entity per case, ids 1.., in its own y row so that its cell key identifies it, box (-1, 1)^3,
    AlwaysExecute.  axis: 0 or 2, the moving coordinate.  With moving=True the entities carry the velocity that takes them to the end position in
    one tick of 0.5; otherwise none, and the end position is to arrive as a Position change request."""
    assert axis in (0, 2)
    rows = edge_cases(outline, atomic)
    A, mid, h = atomic, (outline // 2) // atomic, atomic // 2
    e = blank_entities(len(rows)); e["id"] = np.arange(len(rows)) + 1
    e["original"][:] = (-1, 1, -1, 1, -1, 1)
    end = np.zeros((len(rows), 3), F32)
    for i, (name, c0, o0, c1, o1, fl, want) in enumerate(rows):
        p = np.full(3, A * mid + h, np.float64); p[1] = A * (mid + i) + h
        q = p.copy()
        p[axis] = A * c0 + o0; q[axis] = A * c1 + o1
        e["pos"][i] = p; end[i] = q
        e["flags"][i] = F_ALWAYS_EXEC | fl | (F_HAS_VEL if moving else 0)
        if moving:
            e["vel"][i] = (q - p) * 2.0
    assert not moving or np.all(e["pos"] + e["vel"] * F32(EDGE_DT) == end)      # every number is exact in f32
    return e, end, rows


def edge_expected_keys(outline, atomic, axis, i, want):
    """the sorted packed section keys of case i after the tick, written from its row of the table ([] = removed)"""
    mid = (outline // 2) // atomic
    out = []
    for c in want[1:]:
        cell = [mid, mid + i, mid]; cell[axis] = c                 # x, y, z
        out.append(pack_key(0, cell[0], cell[2], cell[1]))
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparison of an f32 implementation with the rule, and its bounds
# ---------------------------------------------------------------------------------------------------------------------------------------
# Each bound follows from the f32 roundings between the inputs and the value.  In brackets: what the CPU oracle measures on world96 after
# 1 / 2 / 3 ticks; the device measures the same figures to every digit shown.  The bounds were fixed before any device ran them.
#   position, velocity   k ulp of the largest component: per tick one product and one sum, half an ulp each      [0.50 / 0.99 / 1.49 ulp]
#   unit axes            4 * 2^-23 absolute: two normalisations and a sum per tick on components <= 1            [8.8e-8 / 8.8e-8 / 8.9e-8]
#   angle, rate          k ulp of the value: a product and a sum per tick                                        [0.48 / 0.96 / 1.45 ulp]
#   matrix 3x3 block     1e-5 * max(1, largest scale): the project's bar for emitted matrices                    [4.6e-7 / 8.4e-7 / 1.26e-6]
#   matrix column 3      the stored position, bit for bit; the bottom row is (0, 0, 0, 1) exactly
#   box edge             3 ulp of the edge's magnitude (three sums onto a coordinate ~ 8192) plus the matrix bound times the sum of
#                        |OriginalAABB|                                                                          [0.94 / 1.39 / 1.89 ulp]
# At registration (k = 0) position, velocity, angle and rate are the uploaded f32 values themselves.              [0; axes 8.8e-8, matrix 2.4e-7, box 0.5 ulp]
AXIS_BOUND = 4.0 * 2.0 ** -23
MATRIX_BAR = 1e-5


def check_body(got, body, k, measured=None, what=""):
    """got: dict(pos, vel, rot, rotvel, mat, aabb) of f32 arrays as an implementation holds entity `body.id` after k ticks (rot and rotvel as
    (axis xyz, amount); entries of components the entity lacks are ignored); asserts every bound above against the float64 `body` and records the
    largest figure of each kind in `measured`"""
    m = measured if measured is not None else {}
    tag = f"{what} entity {body.id} after {k} ticks"

    def note(key, value):
        m[key] = max(m.get(key, 0.0), float(value))
        return value

    f64 = lambda a: np.asarray(a, np.float64)
    pos = f64(got["pos"])
    assert note("pos_ulp", np.max(np.abs(pos - body.pos)) / ulp32(body.pos)) <= k, tag
    if body.has_vel:
        assert note("vel_ulp", np.max(np.abs(f64(got["vel"]) - body.vel)) / ulp32(body.vel)) <= k, tag
    if body.has_rot:
        rot = f64(got["rot"])
        assert note("axis_abs", np.max(np.abs(rot[:3] - body.rot_axis))) <= AXIS_BOUND, tag
        assert note("angle_ulp", abs(rot[3] - body.angle) / ulp32(body.angle)) <= k, tag
    if body.has_rotvel:
        rv = f64(got["rotvel"])
        assert note("axis_abs", np.max(np.abs(rv[:3] - body.w_axis))) <= AXIS_BOUND, tag
        assert note("angle_ulp", abs(rv[3] - body.w) / ulp32(body.w)) <= k, tag
    M = f64(got["mat"]).reshape(4, 4).T
    mat_bound = MATRIX_BAR * max(1.0, float(np.max(body.scale)))
    assert note("mat_abs", np.max(np.abs(M[:3, :3] - body.M[:3, :3]))) <= mat_bound, tag
    assert np.array_equal(np.asarray(got["mat"], F32)[12:15], np.asarray(got["pos"], F32)), tag
    assert np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]), tag
    box = f64(got["aabb"])
    err = np.abs(box - body.box)
    edge_ulp = np.array([ulp32(v) for v in body.box])
    note("box_ulp", np.max(err / edge_ulp))
    assert np.all(err <= 3.0 * edge_ulp + mat_bound * np.sum(np.abs(body.orig))), (tag, err, edge_ulp)
    return m


def check_sincos(x, s, c, measured=None):
    """s, c: f32 sin and cos of the f32 arguments x by an implementation; asserts sincos_bounds and that every value is finite and in [-1, 1]"""
    m = measured if measured is not None else {}
    x = np.asarray(x, F32); s = np.asarray(s, np.float64); c = np.asarray(c, np.float64)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(c)) and np.all(np.abs(s) <= 1.0) and np.all(np.abs(c) <= 1.0)
    rs, rc, bs, bc = sincos_bounds(x)
    ax = np.abs(x.astype(np.float64))
    for got, ref, bound, name in ((s, rs, bs, "sin"), (c, rc, bc, "cos")):
        # below 1e6 the comparison is with the float64 value rounded to f32, as the bound is one ulp of that
        err = np.where(ax < 1e6, np.abs(got - ref.astype(F32).astype(np.float64)), np.abs(got - ref))
        bad = np.flatnonzero(err > bound)
        assert not len(bad), (name, x[bad][:5], got[bad][:5], ref[bad][:5])
        lo, hi = ax < 1e6, (ax >= 1e6) & (ax <= 2.0 ** 26)
        if lo.any():
            m["small_ulp"] = max(m.get("small_ulp", 0.0), float(np.max(np.abs(got[lo] - ref[lo]) / bound[lo])))
        if hi.any():
            m["high_abs"] = max(m.get("high_abs", 0.0), float(np.max(err[hi]))); m["high_of_bound"] = max(m.get("high_of_bound", 0.0), float(np.max(err[hi] / bound[hi])))
    return m

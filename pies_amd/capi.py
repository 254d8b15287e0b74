"""ctypes binding of include/pies_hip.h (the C ABI of libpies_hip.so).

Used by tests/, bench.py and __graft_entry__.py.  There is no CPU path: if the library is missing or no
gfx950 device is present every entry point raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# PIES_LIB: development tools load the diagnostic build (pies_amd/build.py --exp) instead; tests and bench.py never set it
LIB_PATH = os.environ.get("PIES_LIB") or os.path.join(HERE, "lib", "libpies_hip.so")

OK, ERR_INVALID, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = range(5)
PBD, PD = 0, 1
POSITION, DISTANCE, TET, VOLUME, BEND, SHAPE, GOAL, TRIANGLES, LINES, NODES = range(10)
SCHEDULE_EXACT, SCHEDULE_COLOURED, SCHEDULE_LAYERED = 0, 1, 2
SCHEDULE_DEFAULT = SCHEDULE_LAYERED  # PIES_SCHEDULE_DEFAULT
DEVICE_NONE = -1  # PIES_DEVICE_NONE: host-only handle (scenes and schedules, no compute)
FLAG_RELEASE_HINGE, FLAG_NODE_COLLISIONS, FLAG_TRIANGLE_COLLISIONS, FLAG_REFERENCE_COLLISION_ORDER, FLAG_COLLISION_ORDER = 0, 1, 2, 3, 4
FLAG_RENUMBER_NODES = 5  # PD: pies_finalize may renumber the nodes on the device (host ids stay the host's)
FLAG_PD_NODE_CONTACTS = 6  # PD: node-node contacts detected on the device every substep
COLLISION_ORDER_REFERENCE, COLLISION_ORDER_GROUPS, COLLISION_ORDER_PAIRS = 0, 1, 2
NODE_POSITION, NODE_PREV_POSITION, NODE_VELOCITY, NODE_RADIUS, NODE_INV_MASS = range(5)
KERNEL_NAMES = ["predict", "position", "distance", "tet", "bend", "floor", "velocity", "hash", "collide",
                "pd_predict", "pd_local_distance", "pd_local_tet", "pd_local_volume", "pd_rhs", "pd_spmv", "pd_cg_update",
                "pd_velocity", "wave", "layer"]
KERNEL_PREDICT, KERNEL_POSITION, KERNEL_DISTANCE, KERNEL_TET, KERNEL_BEND, KERNEL_FLOOR, KERNEL_VELOCITY = range(7)
KERNEL_COUNT = 19
SYSTEM_NNZ = 10
REST_SETS = 11
ROW_STENCILS = 12
PD_TILES = 13
PD_TILE_RECORDS = 14
PD_CG_SINGLE = 15
PD_WINDOW_ENTRIES, PD_WINDOW_HALO = 16, 17
NODE_PAIRS = 18  # the node-node CollisionConstraint extension container (PD)
NODES_RENUMBERED = 19  # pies_count: 1 when the device holds the nodes in another numbering (FLAG_RENUMBER_NODES)
NODE_CONTACTS = 20  # pies_count: node-node contacts of the last PD substep (FLAG_PD_NODE_CONTACTS)
SKINS, SKIN_VERTICES = 21, 22  # pies_count: embedded surface meshes (pies_add_skin) and their vertices over all skins
LAYER_REST_SETS = 23  # pies_count: sets in the rest dictionary of schedule LAYERED's tetrahedral container (0: per-element arrays)
LAYER_MAX_TILES = 24  # pies_count: tiles of the phase of schedule LAYERED's plan that has most (0: not active)
LAYER_MAX_CLASS = 25  # pies_count: the largest colour class of any tile and container of schedule LAYERED's plan (0: not active)
PD_CG_BLOCKS = 26  # pies_count: workgroups of the PD CG launches that meet at a grid barrier (at most half the resident grid)
RAY_SCENE_TRIANGLES, RAY_SKIN = 0, 1  # pies_raycast targets
RAY_CULL_BACK = 1  # pies_raycast flag
RAY_MISS = 0xFFFFFFFF  # PIES_RAY_MISS
NEAR_NONE = 0xFFFFFFFF  # PIES_NEAR_NONE: pies_closest_points found no candidate
PROP_SPHERE, PROP_CAPSULE, PROP_BOX = 0, 1, 2  # pies_prop_t.shape
PROP_NONE = 0xFFFFFFFF  # PIES_PROP_NONE: no prop touched the node
PROP_MAX = 64  # PIES_PROP_MAX
FIELD_MAX = 64  # PIES_FIELD_MAX: fields per handle
FIELD_PROP_MAX = 64  # PIES_FIELD_PROP_MAX: field props per call
FORCE_DIRECTIONAL, FORCE_RADIAL, FORCE_VORTEX, FORCE_DRAG, FORCE_WIND = 0, 1, 2, 3, 4  # pies_force_t.type
FALLOFF_NONE, FALLOFF_LINEAR, FALLOFF_SMOOTH = 0, 1, 2  # pies_force_t.falloff
FORCE_IS_FORCE = 1  # pies_force_t.flags: vector / strength give a force, not an acceleration
FORCE_MAX = 64  # PIES_FORCE_MAX
LOAD_PRESSURE, LOAD_GAS, LOAD_FLUID = 0, 1, 2  # pies_surface_load_t.type
LOAD_INWARD = 1  # pies_surface_load_t.flags: the range's triangles are wound with their normals inward
LOAD_MAX = 64  # PIES_LOAD_MAX
LOAD_TO_END = 0xFFFFFFFF  # pies_surface_load_t.count: to the container's end
ANCHOR_SET_MAX, ANCHOR_FRAME_MAX = 64, 64  # PIES_ANCHOR_SET_MAX: sets per handle; PIES_ANCHOR_FRAME_MAX: frames per set
ANCHOR_PIN = 1  # pies_anchor_t.flags: the node sits on the attachment point
TIE_SET_MAX, TIE_GROUP_MAX = 64, 64  # PIES_TIE_SET_MAX: sets per handle; PIES_TIE_GROUP_MAX: groups per set
ACTUATOR_SET_MAX, ACTUATOR_CHANNEL_MAX = 64, 64  # PIES_ACTUATOR_SET_MAX: sets per handle; PIES_ACTUATOR_CHANNEL_MAX: channels per set
ACTUATOR_OFFSET = 1  # pies_actuator_t.flags: r = base + gain u instead of base (1 + gain u)
ELEMENT_INVERTED, ELEMENT_OVER, ELEMENT_UNDER, ELEMENT_NONFINITE = 1, 2, 4, 8  # pies_element_measure_t.flags
MEASURE_RANGE_MAX = 64  # PIES_MEASURE_RANGE_MAX: ranges per pies_measure_nodes call
IO_HOST_SYNC = 1  # PIES_IO_HOST_SYNC: a device-side read or write returns after its launches have finished
LAYER_REST_MAX_SETS = 64  # kLayerRestMaxSets (layer_rest.h): a scene with more distinct sets reads the per-element arrays

# every symbol include/pies_hip.h declares (checked by tests/test_capi_symbols.py against the header)
SYMBOLS = [
    "pies_create", "pies_destroy", "pies_clear", "pies_last_error", "pies_abi_version", "pies_default_options",
    "pies_get_options", "pies_add_nodes", "pies_add_nodes_ex", "pies_add_position_constraints",
    "pies_add_distance_constraints", "pies_add_tet_constraints", "pies_add_volume_constraints",
    "pies_add_bend_constraints", "pies_add_triangles", "pies_create_tet_box", "pies_create_box", "pies_create_sheet",
    "pies_create_bend_sheet", "pies_set_flag", "pies_set_schedule", "pies_finalize", "pies_tick", "pies_tick_async",
    "pies_synchronize", "pies_failed", "pies_count", "pies_read_nodes", "pies_write_nodes", "pies_get_ids",
    "pies_get_rest", "pies_get_order", "pies_get_batches", "pies_profile_substep", "pies_launch_counts",
    "pies_set_pcg", "pies_get_pcg_stats", "pies_collision_pairs", "pies_add_shape_constraint",
    "pies_add_goal_constraint", "pies_set_goal_transform", "pies_add_fixed_regions", "pies_update_fixed_regions",
    "pies_add_linked_regions", "pies_create_shape_matching_box", "pies_create_shape_matching_sheet", "pies_get_group",
    "pies_get_tri_contacts", "pies_tick_begin", "pies_export_acquire", "pies_export_release",
    "pies_read_positions_strided", "pies_set_pcg_retry", "pies_get_pcg_health", "pies_profile_in_situ",
    "pies_collision_stats", "pies_get_collision_health", "pies_set_collision_rounds", "pies_set_solver", "pies_debug_pair_state", "pies_set_tuning",
    "pies_get_pd_tile_plan", "pies_get_tri_grid_stats", "pies_set_rest", "pies_get_collision_fallbacks",
    "pies_add_node_pair_constraints", "pies_get_node_order", "pies_get_node_contacts",
    "pies_add_skin", "pies_get_skin_binding", "pies_read_skin", "pies_export_acquire_skin",
    "pies_voxelize_tri_mesh", "pies_add_tri_mesh_volume", "pies_raycast", "pies_closest_points", "pies_collide_props",
    "pies_add_field", "pies_add_field_tri_mesh", "pies_get_field", "pies_collide_field_props", "pies_apply_forces",
    "pies_apply_surface_loads", "pies_add_anchors", "pies_get_anchors", "pies_apply_anchors",
    "pies_add_ties", "pies_get_ties", "pies_apply_ties", "pies_get_tie_state", "pies_reset_ties",
    "pies_add_actuators", "pies_get_actuators", "pies_drive_actuators", "pies_drive_actuators_device",
    "pies_measure_elements", "pies_measure_nodes",
    "pies_read_nodes_device", "pies_write_nodes_device", "pies_read_skin_device",
    "pies_layer_rest_pack", "pies_layer_rest_unpack", "pies_layer_rest_usable",
    "pies_resource_counts",
]


class PiesError(RuntimeError):
    pass


def layer_rest_pack(ids, set_index):
    """pies_layer_rest_pack: the two record words of an element (13-bit tile-local ids, 12-bit set index), None when one does not fit"""
    i, w = (C.c_uint32 * 4)(*ids), (C.c_uint32 * 2)()
    return (w[0], w[1]) if load().pies_layer_rest_pack(i, set_index, w) == OK else None


def layer_rest_unpack(words):
    """pies_layer_rest_unpack: (ids, set index) of an element's two record words"""
    w, i, s = (C.c_uint32 * 2)(*words), (C.c_uint32 * 4)(), C.c_uint32()
    load().pies_layer_rest_unpack(w, i, C.byref(s))
    return list(i), s.value


def layer_rest_usable(sets, count, max_group_nodes, lds_bytes=0):
    """pies_layer_rest_usable: whether such a scene takes the rest dictionary (all or nothing); lds_bytes 0: the library's figure for
    gfx950, the one host-only handles decide with"""
    return load().pies_layer_rest_usable(sets, count, max_group_nodes, lds_bytes) == 1


# the eight kinds of pies_resource_counts, in the order of either half of its sixteen words
RESOURCE_KINDS = ("device_bytes", "device_allocations", "pinned_bytes", "pinned_allocations", "streams", "events", "graphs",
                  "graph_execs")


def resource_counts():
    """pies_resource_counts: {"live": {kind: n}, "created": {kind: n}} over RESOURCE_KINDS - the HIP resources the library holds
    now, and has created since it was loaded, over all handles of the process (destroyed ones included)"""
    out = (C.c_uint64 * 16)()
    if load().pies_resource_counts(out) != OK:
        raise PiesError("pies_resource_counts failed")
    return {"live": {k: int(out[i]) for i, k in enumerate(RESOURCE_KINDS)},
            "created": {k: int(out[8 + i]) for i, k in enumerate(RESOURCE_KINDS)}}


def set_tuning(name, value):
    """pies_set_tuning: process-wide tuning / diagnostic switch (value None unsets)"""
    rc = load().pies_set_tuning(name.encode(), None if value is None else str(value).encode())
    if rc != OK:
        raise PiesError("pies_set_tuning(%s): invalid name" % name)


class Options(C.Structure):
    """pies_options_t == Pies::SolverOptions field for field."""
    _fields_ = [
        ("fixedTimestepSize", C.c_float), ("timeSubsteps", C.c_uint32), ("iterations", C.c_uint32),
        ("collisionStabilizationIterations", C.c_uint32), ("collisionThresholdDistance", C.c_float),
        ("collisionThickness", C.c_float), ("gravity", C.c_float), ("damping", C.c_float),
        ("friction", C.c_float), ("staticFrictionThreshold", C.c_float), ("floorHeight", C.c_float),
        ("gridSpacing", C.c_float), ("threadCount", C.c_uint32), ("solver", C.c_int32),
    ]

    def __init__(self, **kw):
        super().__init__(0.012, 1, 4, 4, 0.1, 0.05, 10.0, 0.006, 0.01, 0.0, 0.0, 2.0, 8, PD)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class Prop(C.Structure):
    """pies_prop_t field for field: a kinematic sphere, capsule or rounded box of pies_collide_props."""
    _fields_ = [
        ("shape", C.c_int32), ("radius", C.c_float), ("centre", C.c_float * 3), ("end", C.c_float * 3),
        ("axes", C.c_float * 9), ("half", C.c_float * 3), ("velocity", C.c_float * 3), ("angular", C.c_float * 3),
        ("pivot", C.c_float * 3), ("friction", C.c_float),
    ]

    @classmethod
    def _make(cls, shape, radius, centre, velocity, angular, pivot, friction):
        p = cls()
        p.shape, p.radius, p.friction = shape, radius, friction
        p.centre[:] = [float(x) for x in centre]
        p.velocity[:] = [float(x) for x in velocity]
        p.angular[:] = [float(x) for x in angular]
        p.pivot[:] = [float(x) for x in (centre if pivot is None else pivot)]
        p.axes[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        return p

    @classmethod
    def sphere(cls, centre, radius, velocity=(0, 0, 0), angular=(0, 0, 0), pivot=None, friction=0.0):
        """pivot None: the centre"""
        return cls._make(PROP_SPHERE, radius, centre, velocity, angular, pivot, friction)

    @classmethod
    def capsule(cls, a, b, radius, velocity=(0, 0, 0), angular=(0, 0, 0), pivot=None, friction=0.0):
        """the segment a b with a radius; pivot None: end a"""
        p = cls._make(PROP_CAPSULE, radius, a, velocity, angular, pivot, friction)
        p.end[:] = [float(x) for x in b]
        return p

    @classmethod
    def box(cls, centre, half, axes=None, rounding=0.0, velocity=(0, 0, 0), angular=(0, 0, 0), pivot=None, friction=0.0):
        """axes: 3 x 3, row j the unit axis j (None: the world's); rounding: the rounding radius; pivot None: the centre"""
        p = cls._make(PROP_BOX, rounding, centre, velocity, angular, pivot, friction)
        p.half[:] = [float(x) for x in half]
        if axes is not None:
            p.axes[:] = [float(x) for x in np.asarray(axes, dtype=np.float32).reshape(9)]
        return p


class FieldProp(C.Structure):
    """pies_field_prop_t field for field: a rigid placement of a signed distance field (pies_collide_field_props)."""
    _fields_ = [
        ("field", C.c_uint32), ("radius", C.c_float), ("centre", C.c_float * 3), ("axes", C.c_float * 9),
        ("velocity", C.c_float * 3), ("angular", C.c_float * 3), ("pivot", C.c_float * 3), ("friction", C.c_float),
    ]

    @classmethod
    def make(cls, field, centre, axes=None, radius=0.0, velocity=(0, 0, 0), angular=(0, 0, 0), pivot=None, friction=0.0):
        """centre: the world position of the field's local origin (0, 0, 0); axes: 3 x 3, row j the unit axis j of the local frame
        (None: the world's); radius: inflation of the zero level set; pivot None: the centre"""
        p = cls()
        p.field, p.radius, p.friction = field, radius, friction
        p.centre[:] = [float(x) for x in centre]
        p.axes[:] = [float(x) for x in np.asarray(np.eye(3) if axes is None else axes, dtype=np.float32).reshape(9)]
        p.velocity[:] = [float(x) for x in velocity]
        p.angular[:] = [float(x) for x in angular]
        p.pivot[:] = [float(x) for x in (centre if pivot is None else pivot)]
        return p


class Force(C.Structure):
    """pies_force_t field for field: one force field of pies_apply_forces.  The builders give a force that acts everywhere;
    within() confines it to a sphere."""
    _fields_ = [
        ("type", C.c_int32), ("flags", C.c_uint32), ("centre", C.c_float * 3), ("radius", C.c_float), ("falloff", C.c_int32),
        ("vector", C.c_float * 3), ("strength", C.c_float), ("shear", C.c_float),
    ]

    @classmethod
    def _make(cls, type, vector=(0, 0, 0), strength=0.0, shear=0.0, centre=(0, 0, 0), is_force=False):
        f = cls()
        f.type, f.flags, f.falloff = type, FORCE_IS_FORCE if is_force else 0, FALLOFF_NONE
        f.radius, f.strength, f.shear = float("inf"), strength, shear
        f.centre[:] = [float(x) for x in centre]
        f.vector[:] = [float(x) for x in vector]
        return f

    @classmethod
    def directional(cls, vector, is_force=False):
        """an acceleration (is_force: a force) along vector"""
        return cls._make(FORCE_DIRECTIONAL, vector=vector, is_force=is_force)

    @classmethod
    def radial(cls, centre, strength, is_force=False):
        """away from centre with strength > 0 (a blast), towards it with strength < 0 (an attractor)"""
        return cls._make(FORCE_RADIAL, strength=strength, centre=centre, is_force=is_force)

    @classmethod
    def vortex(cls, centre, axis, strength=1.0, is_force=False):
        """cross(axis, p - centre) * strength; the axis need not be a unit vector"""
        return cls._make(FORCE_VORTEX, vector=axis, strength=strength, centre=centre, is_force=is_force)

    @classmethod
    def drag(cls, strength, velocity=(0, 0, 0)):
        """a medium moving with velocity that takes the share min(strength * dt, 1) of the relative velocity"""
        return cls._make(FORCE_DRAG, vector=velocity, strength=strength)

    @classmethod
    def wind(cls, velocity, strength, shear=0.0):
        """air moving with velocity against the scene's triangles: strength for the normal part, shear for the tangential part"""
        return cls._make(FORCE_WIND, vector=velocity, strength=strength, shear=shear)

    def within(self, centre, radius, falloff=FALLOFF_NONE):
        """confines the force to the sphere (centre, radius); radial forces and vortices refer to the same centre"""
        self.centre[:] = [float(x) for x in centre]
        self.radius, self.falloff = radius, falloff
        return self


class SurfaceLoad(C.Structure):
    """pies_surface_load_t field for field: one load of pies_apply_surface_loads on the triangles [first, first + count) of the
    TRIANGLES container (count None: to the container's end)."""
    _fields_ = [
        ("type", C.c_int32), ("flags", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32), ("strength", C.c_float),
        ("rest_volume", C.c_float), ("point", C.c_float * 3), ("up", C.c_float * 3), ("velocity", C.c_float * 3), ("drag", C.c_float),
    ]

    @classmethod
    def _make(cls, type, strength, first, count, about=(0, 0, 0)):
        f = cls()
        f.type, f.strength, f.first, f.count = type, strength, first, LOAD_TO_END if count is None else count
        f.point[:] = [float(x) for x in about]
        f.up[:] = [0.0, 1.0, 0.0]
        return f

    @classmethod
    def pressure(cls, p, first=0, count=None, about=(0, 0, 0)):
        """the pressure p along every triangle's normal; about: the point the returned torque refers to"""
        return cls._make(LOAD_PRESSURE, p, first, count, about)

    @classmethod
    def gas(cls, ambient, rest_volume, first=0, count=None, about=(0, 0, 0)):
        """an isothermal gas inside the closed range: ambient * (rest_volume / V - 1) along every normal"""
        f = cls._make(LOAD_GAS, ambient, first, count, about)
        f.rest_volume = rest_volume
        return f

    @classmethod
    def fluid(cls, weight, surface_point, up=(0, 1, 0), first=0, count=None):
        """a fluid of `weight` per unit volume (density x gravity) whose surface holds surface_point and faces up"""
        f = cls._make(LOAD_FLUID, weight, first, count, surface_point)
        f.up[:] = [float(x) for x in up]
        return f

    def with_drag(self, drag, velocity=(0, 0, 0)):
        """a fluid's drag per unit of relative speed and submerged area, the fluid moving with velocity"""
        self.drag = drag
        self.velocity[:] = [float(x) for x in velocity]
        return self

    def inward(self):
        """the range's triangles are wound with their normals pointing into the body"""
        self.flags |= LOAD_INWARD
        return self


class AnchorFrame(C.Structure):
    """pies_anchor_frame_t field for field: a moving frame of pies_apply_anchors - where the host's rigid body is and how it moves."""
    _fields_ = [
        ("origin", C.c_float * 3), ("axes", C.c_float * 9), ("velocity", C.c_float * 3), ("angular", C.c_float * 3),
        ("pivot", C.c_float * 3), ("strength", C.c_float),
    ]

    @classmethod
    def make(cls, origin, axes=None, velocity=(0, 0, 0), angular=(0, 0, 0), pivot=None, strength=1.0):
        """origin: the world position of local (0, 0, 0); axes: 3 x 3, row j the unit axis j (None: the world's); pivot None: the
        origin; strength scales the stiffness and damping of the frame's springs, 0 releases its springs and its pins"""
        f = cls()
        f.origin[:] = [float(x) for x in origin]
        f.axes[:] = [float(x) for x in np.asarray(np.eye(3) if axes is None else axes, dtype=np.float32).reshape(9)]
        f.velocity[:] = [float(x) for x in velocity]
        f.angular[:] = [float(x) for x in angular]
        f.pivot[:] = [float(x) for x in (origin if pivot is None else pivot)]
        f.strength = strength
        return f


class Anchor(C.Structure):
    """pies_anchor_t field for field: one node tied to the point `local` of frame `frame` by a spring-damper, or pinned to it."""
    _fields_ = [
        ("node", C.c_uint32), ("frame", C.c_uint32), ("local", C.c_float * 3), ("stiffness", C.c_float), ("damping", C.c_float),
        ("flags", C.c_uint32),
    ]

    @classmethod
    def make(cls, node, frame_index, local, stiffness=0.0, damping=0.0, pin=False):
        a = cls()
        a.node, a.frame, a.stiffness, a.damping, a.flags = node, frame_index, stiffness, damping, ANCHOR_PIN if pin else 0
        a.local[:] = [float(x) for x in local]
        return a

    @classmethod
    def at(cls, node, frame_index, frame, position, stiffness=0.0, damping=0.0, pin=False):
        """the anchor whose attachment point is the world `position` as `frame` (an AnchorFrame) stands: local_j = axis_j .
        (position - origin), in fp32, each dot product summed left to right"""
        f32 = np.float32
        d = np.array(list(position), f32) - np.array(list(frame.origin), f32)
        axes = np.array(list(frame.axes), f32).reshape(3, 3)
        local = [(axes[j, 0] * d[0] + axes[j, 1] * d[1]) + axes[j, 2] * d[2] for j in range(3)]
        return cls.make(node, frame_index, local, stiffness, damping, pin)


class Actuator(C.Structure):
    """pies_actuator_t field for field: constraint `index` of the DISTANCE or BEND container (host order) whose rest datum follows
    activation channel `channel`: base (1 + gain u), or base + gain u with offset=True, clamped to [lo, hi].  `base` is written
    by the library when the set is added."""
    _fields_ = [
        ("type", C.c_int32), ("index", C.c_uint32), ("channel", C.c_uint32), ("gain", C.c_float), ("lo", C.c_float), ("hi", C.c_float),
        ("base", C.c_float), ("flags", C.c_uint32),
    ]

    @classmethod
    def make(cls, ctype, index, channel=0, gain=1.0, lo=0.0, hi=3.0e38, offset=False):
        a = cls()
        a.type, a.index, a.channel, a.gain, a.lo, a.hi, a.base = ctype, index, channel, gain, lo, hi, 0.0
        a.flags = ACTUATOR_OFFSET if offset else 0
        return a


class Tie(C.Structure):
    """pies_tie_t field for field: node `node` bound to the point sum weight_j p_to[j] by a spring-damper of group `group`."""
    _fields_ = [
        ("node", C.c_uint32), ("to", C.c_uint32 * 3), ("weight", C.c_float * 3), ("stiffness", C.c_float), ("damping", C.c_float),
        ("group", C.c_uint32),
    ]

    @classmethod
    def make(cls, node, to, weights=(1.0, 0.0, 0.0), stiffness=0.0, damping=0.0, group=0):
        """to: one, two or three carrier node ids (missing slots repeat the first id with weight 0); weights: as many, or three"""
        to = [int(i) for i in np.atleast_1d(to)]
        weights = [float(x) for x in weights][:max(len(to), 1)] if len(to) < 3 else [float(x) for x in weights]
        t = cls()
        t.node, t.stiffness, t.damping, t.group = node, stiffness, damping, group
        t.to[:] = (to + [to[0]] * 3)[:3]
        t.weight[:] = (weights + [0.0] * 3)[:3]
        return t

    @classmethod
    def on_triangle(cls, node, corner_ids, u, v, stiffness=0.0, damping=0.0, group=0):
        """the tie to the point (u, v) of a triangle as pies_closest_points reports it: weights ((1 - u) - v, u, v) in fp32"""
        f32 = np.float32
        u, v = f32(u), f32(v)
        return cls.make(node, corner_ids, ((f32(1.0) - u) - v, u, v), stiffness, damping, group)


class TieGroup(C.Structure):
    """pies_tie_group_t field for field: what a call gives the ties of one group."""
    _fields_ = [("pivot", C.c_float * 3), ("strength", C.c_float), ("break_stretch", C.c_float)]

    @classmethod
    def make(cls, pivot=(0, 0, 0), strength=1.0, break_stretch=0.0):
        """pivot: the point the returned torque refers to; strength scales stiffness and damping, 0 releases the group;
        break_stretch > 0: a tie found longer than this breaks and stays broken until reset_ties"""
        g = cls()
        g.pivot[:] = [float(x) for x in pivot]
        g.strength, g.break_stretch = strength, break_stretch
        return g


class ElementMeasure(C.Structure):
    """pies_element_measure_t field for field: one element's record of pies_measure_elements (eight words)."""
    _fields_ = [("s", C.c_float * 3), ("j", C.c_float), ("volume", C.c_float), ("i1", C.c_float), ("green", C.c_float),
                ("flags", C.c_uint32)]


class ElementSummary(C.Structure):
    """pies_element_summary_t field for field: the summary of a range of elements."""
    _fields_ = [("max_stretch", C.c_float), ("min_stretch", C.c_float), ("min_j", C.c_float), ("max_j", C.c_float),
                ("max_green", C.c_float), ("volume", C.c_float), ("inverted", C.c_uint32), ("over", C.c_uint32),
                ("under", C.c_uint32), ("nonfinite", C.c_uint32)]


class NodeSums(C.Structure):
    """pies_node_sums_t field for field: the sums of one range of pies_measure_nodes (thirteen words)."""
    _fields_ = [("mass", C.c_float), ("momentum", C.c_float * 3), ("angular", C.c_float * 3), ("moment", C.c_float * 3),
                ("kinetic", C.c_float), ("dynamic", C.c_uint32), ("fixed", C.c_uint32)]


# numpy views of the two records: Solver.measure_elements / measure_nodes return structured arrays
class DeviceNodes(C.Structure):
    """pies_device_nodes_t: device addresses (0 / None: the array is not part of the call)"""
    _fields_ = [("position", C.c_void_p), ("prev_position", C.c_void_p), ("velocity", C.c_void_p), ("radius", C.c_void_p),
                ("inv_mass", C.c_void_p), ("stride", C.c_uint32)]


ELEMENT_MEASURE_DTYPE = np.dtype([("s", np.float32, 3), ("j", np.float32), ("volume", np.float32), ("i1", np.float32),
                                  ("green", np.float32), ("flags", np.uint32)])
NODE_SUMS_DTYPE = np.dtype([("mass", np.float32), ("momentum", np.float32, 3), ("angular", np.float32, 3),
                            ("moment", np.float32, 3), ("kinetic", np.float32), ("dynamic", np.uint32), ("fixed", np.uint32)])


_lib = None


def load():
    """Loads libpies_hip.so.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PiesError("%s is missing: build it with `python -m pies_amd.build` (needs hipcc); "
                        "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, f32, i32 = C.c_void_p, C.c_uint32, C.c_float, C.c_int
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    ppv = C.POINTER(C.c_void_p)
    sig = {
        "pies_create": [C.POINTER(Options), i32, ppv],
        "pies_destroy": [vp], "pies_clear": [vp],
        "pies_default_options": [C.POINTER(Options)],
        "pies_get_options": [vp, C.POINTER(Options)],
        "pies_add_nodes": [vp, u32, pf, pu],
        "pies_add_nodes_ex": [vp, u32, pf, pf, pf, pf, pu],
        "pies_add_position_constraints": [vp, u32, pu, f32],
        "pies_add_distance_constraints": [vp, u32, pu, f32],
        "pies_add_tet_constraints": [vp, u32, pu, f32, f32, f32],
        "pies_add_volume_constraints": [vp, u32, pu, f32, f32, f32],
        "pies_add_bend_constraints": [vp, u32, pu, f32],
        "pies_add_node_pair_constraints": [vp, u32, pu],
        "pies_add_triangles": [vp, u32, pu],
        "pies_create_tet_box": [vp, u32, u32, u32, pf, f32, pf, f32, f32, u32],
        "pies_create_box": [vp, u32, u32, u32, pf, f32, f32, i32, u32, u32],
        "pies_create_sheet": [vp, u32, u32, pf, f32, f32, f32],
        "pies_create_bend_sheet": [vp, u32, u32, pf, f32, f32],
        "pies_set_flag": [vp, i32, i32], "pies_set_schedule": [vp, i32],
        "pies_finalize": [vp], "pies_tick": [vp], "pies_tick_async": [vp], "pies_synchronize": [vp],
        "pies_failed": [vp, C.POINTER(i32)],
        "pies_count": [vp, i32, pu],
        "pies_read_nodes": [vp, i32, pf, u32], "pies_write_nodes": [vp, i32, pf, u32],
        "pies_get_ids": [vp, i32, pu, u32], "pies_get_rest": [vp, i32, pf, u32],
        "pies_set_rest": [vp, i32, u32, u32, pf],
        "pies_get_collision_fallbacks": [vp, pu],
        "pies_get_order": [vp, i32, pu, u32], "pies_get_batches": [vp, i32, pu, u32, pu],
        "pies_get_node_order": [vp, pu, u32],
        "pies_profile_substep": [vp, i32, pu, C.POINTER(C.c_double), C.POINTER(C.c_uint64)],
        "pies_launch_counts": [vp, pu],
        "pies_set_pcg": [vp, f32, u32],
        "pies_get_pcg_stats": [vp, pf, pu, pu],
        "pies_collision_pairs": [vp, C.POINTER(C.c_uint64)],
        "pies_add_shape_constraint": [vp, u32, pu, f32],
        "pies_add_goal_constraint": [vp, u32, pu, f32, pu],
        "pies_set_goal_transform": [vp, u32, pf],
        "pies_add_fixed_regions": [vp, u32, pf, f32],
        "pies_update_fixed_regions": [vp, u32, pf],
        "pies_add_linked_regions": [vp, u32, pf, f32],
        "pies_create_shape_matching_box": [vp, pf, u32, u32, u32, f32],
        "pies_create_shape_matching_sheet": [vp, u32, u32, pf, f32, f32],
        "pies_get_group": [vp, i32, u32, pu, u32, pu],
        "pies_get_tri_contacts": [vp, pu, u32, pu],
        "pies_get_node_contacts": [vp, pu, u32, pu],
        "pies_get_tri_grid_stats": [vp, pu],
        "pies_tick_begin": [vp, C.POINTER(C.c_uint64)],
        "pies_export_acquire": [vp, C.c_uint64, C.POINTER(pf), pu],
        "pies_export_release": [vp, C.c_uint64],
        "pies_read_positions_strided": [vp, vp, C.c_uint64, u32],
        "pies_set_pcg_retry": [vp, i32],
        "pies_collision_stats": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
        "pies_get_pcg_health": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), pu, pu],
        "pies_get_collision_health": [vp, pu, pu, pu, pu],
        "pies_set_collision_rounds": [vp, u32],
        "pies_set_solver": [vp, i32],
        "pies_debug_pair_state": [vp, pf, pf, pu, u32],
        "pies_profile_in_situ": [vp, i32, u32, pu, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)],
    }
    sig["pies_set_tuning"] = [C.c_char_p, C.c_char_p]
    sig["pies_add_skin"] = [vp, u32, pf, u32, pu, u32, pu, f32, pu]
    sig["pies_get_skin_binding"] = [vp, u32, pu, pu, pf, u32, pu]
    sig["pies_read_skin"] = [vp, u32, pf, pf, u32]
    sig["pies_export_acquire_skin"] = [vp, C.c_uint64, u32, C.POINTER(pf), C.POINTER(pf), pu]
    sig["pies_voxelize_tri_mesh"] = [vp, u32, pf, u32, pu, pf, f32, pu, pf, C.POINTER(C.c_uint8)]
    sig["pies_add_tri_mesh_volume"] = [vp, u32, pf, u32, pu, pf, f32, f32, f32, f32, f32, f32, f32, u32, pu, pu, pu, pu]
    sig["pies_raycast"] = [vp, i32, u32, u32, pf, pf, f32, u32, pu, pf, pf]
    sig["pies_closest_points"] = [vp, i32, u32, u32, pf, f32, pu, pf, pf, pf, pf]
    sig["pies_collide_props"] = [vp, u32, C.POINTER(Prop), pf, pf, pu, pu]
    sig["pies_add_field"] = [vp, pu, pf, f32, pf, pu]
    sig["pies_add_field_tri_mesh"] = [vp, u32, pf, u32, pu, f32, f32, pu]
    sig["pies_get_field"] = [vp, u32, pu, pf, pf, pf, C.c_uint64]
    sig["pies_collide_field_props"] = [vp, u32, C.POINTER(FieldProp), pf, pf, pu, pu]
    sig["pies_apply_forces"] = [vp, u32, C.POINTER(Force), f32, pf, pf, pu]
    sig["pies_apply_surface_loads"] = [vp, u32, C.POINTER(SurfaceLoad), f32, pf, pf, pu, pf, pf]
    sig["pies_add_anchors"] = [vp, u32, C.POINTER(Anchor), u32, pu]
    sig["pies_get_anchors"] = [vp, u32, C.POINTER(Anchor), u32, pu, pu]
    sig["pies_apply_anchors"] = [vp, u32, u32, C.POINTER(AnchorFrame), f32, pf, pf, pu, pf]
    sig["pies_add_ties"] = [vp, u32, C.POINTER(Tie), u32, pu]
    sig["pies_get_ties"] = [vp, u32, C.POINTER(Tie), u32, pu, pu]
    sig["pies_apply_ties"] = [vp, u32, u32, C.POINTER(TieGroup), f32, u32, pf, pf, pu, pf]
    sig["pies_get_tie_state"] = [vp, u32, C.POINTER(C.c_uint8), u32, pu]
    sig["pies_reset_ties"] = [vp, u32]
    sig["pies_add_actuators"] = [vp, u32, C.POINTER(Actuator), u32, pu]
    sig["pies_get_actuators"] = [vp, u32, C.POINTER(Actuator), u32, pu, pu]
    sig["pies_drive_actuators"] = [vp, u32, u32, pf, pf, pu, pf]
    sig["pies_drive_actuators_device"] = [vp, u32, u32, vp, vp, vp, vp, vp, u32]
    sig["pies_measure_elements"] =[vp, i32, u32, u32, C.POINTER(ElementMeasure), C.POINTER(ElementSummary)]
    sig["pies_measure_nodes"] = [vp, u32, pu, pf, C.POINTER(NodeSums)]
    sig["pies_read_nodes_device"] = [vp, C.POINTER(DeviceNodes), u32, vp, u32]
    sig["pies_write_nodes_device"] = [vp, C.POINTER(DeviceNodes), vp, u32, vp, u32]
    sig["pies_read_skin_device"] = [vp, u32, vp, vp, u32, vp, u32]
    sig["pies_layer_rest_pack"] = [pu, u32, pu]
    sig["pies_layer_rest_unpack"] = [pu, pu, pu]
    sig["pies_layer_rest_usable"] = [u32, u32, u32, u32]
    sig["pies_resource_counts"] = [C.POINTER(C.c_uint64)]
    sig["pies_get_pd_tile_plan"] = [vp, pu, pu, pu, pu, pu, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), u32]
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = None if name == "pies_default_options" else C.c_int
    L.pies_last_error.argtypes = [vp]
    L.pies_last_error.restype = C.c_char_p
    L.pies_abi_version.argtypes = []
    L.pies_abi_version.restype = C.c_int
    _lib = L
    return L


def _pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _pu(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


_IDS_PER = {POSITION: 1, DISTANCE: 2, TET: 4, VOLUME: 4, BEND: 4, TRIANGLES: 3, LINES: 1, NODE_PAIRS: 2}
_REST_PER = {DISTANCE: 1, TET: 9, VOLUME: 9, BEND: 1}


class Solver:
    """Object wrapper over one pies_solver_t handle (one HIP device + stream)."""

    def __init__(self, options=None, device=0, **kw):
        self._L = load()
        self.options = options if options is not None else Options(**kw)
        h = C.c_void_p()
        rc = self._L.pies_create(C.byref(self.options), device, C.byref(h))
        if rc != OK:
            raise PiesError("pies_create failed (code %d): no gfx950 HIP device %d, or runtime error" % (rc, device))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.pies_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != OK:
            raise PiesError("pies error %d: %s" % (rc, self._L.pies_last_error(self._h).decode()))

    # -- scene ---------------------------------------------------------------------------------
    def addNodes(self, pos):
        pos = _f32(pos).reshape(-1, 3)
        first = C.c_uint32()
        self._ck(self._L.pies_add_nodes(self._h, len(pos), _pf(pos), C.byref(first)))
        return first.value

    def add_nodes_raw(self, pos, vel=None, radius=None, invMass=None):
        pos = _f32(pos).reshape(-1, 3)
        n = len(pos)
        vel = None if vel is None else _f32(vel).reshape(n, 3)
        radius = None if radius is None else _f32(np.broadcast_to(radius, (n,)))
        invMass = None if invMass is None else _f32(np.broadcast_to(invMass, (n,)))
        first = C.c_uint32()
        self._ck(self._L.pies_add_nodes_ex(self._h, n, _pf(pos), None if vel is None else _pf(vel),
                                           None if radius is None else _pf(radius),
                                           None if invMass is None else _pf(invMass), C.byref(first)))
        return first.value

    def add_position(self, ids, w):
        ids = _u32(ids).reshape(-1)
        self._ck(self._L.pies_add_position_constraints(self._h, len(ids), _pu(ids), w))

    def add_distance(self, ids, w):
        ids = _u32(ids).reshape(-1, 2)
        self._ck(self._L.pies_add_distance_constraints(self._h, len(ids), _pu(ids), w))

    def add_tet(self, ids, w, minStrain=0.8, maxStrain=1.0):
        ids = _u32(ids).reshape(-1, 4)
        self._ck(self._L.pies_add_tet_constraints(self._h, len(ids), _pu(ids), w, minStrain, maxStrain))

    def add_volume(self, ids, w, compression=1.0, stretching=1.0):
        ids = _u32(ids).reshape(-1, 4)
        self._ck(self._L.pies_add_volume_constraints(self._h, len(ids), _pu(ids), w, compression, stretching))

    def add_bend(self, ids, w):
        ids = _u32(ids).reshape(-1, 4)
        self._ck(self._L.pies_add_bend_constraints(self._h, len(ids), _pu(ids), w))

    def add_node_pairs(self, ids):
        """extension: node-node CollisionConstraints (CollisionConstraint.cpp:7-65) over the listed pairs; PD only"""
        ids = _u32(ids).reshape(-1, 2)
        self._ck(self._L.pies_add_node_pair_constraints(self._h, len(ids), _pu(ids)))

    def add_triangles(self, ids):
        ids = _u32(ids).reshape(-1, 3)
        self._ck(self._L.pies_add_triangles(self._h, len(ids), _pu(ids)))

    def add_shape(self, ids, w):
        ids = _u32(ids).reshape(-1)
        self._ck(self._L.pies_add_shape_constraint(self._h, len(ids), _pu(ids), w))

    def add_goal(self, ids, w):
        ids = _u32(ids).reshape(-1)
        k = C.c_uint32()
        self._ck(self._L.pies_add_goal_constraint(self._h, len(ids), _pu(ids), w, C.byref(k)))
        return k.value

    def set_goal_transform(self, goal, m16):
        m = _f32(m16).reshape(16)
        self._ck(self._L.pies_set_goal_transform(self._h, goal, _pf(m)))

    def add_fixed_regions(self, mats, w):
        m = _f32(mats).reshape(-1, 16)
        self._ck(self._L.pies_add_fixed_regions(self._h, len(m), _pf(m), w))

    def update_fixed_regions(self, mats):
        m = _f32(mats).reshape(-1, 16)
        self._ck(self._L.pies_update_fixed_regions(self._h, len(m), _pf(m)))

    def add_linked_regions(self, mats, w):
        m = _f32(mats).reshape(-1, 16)
        self._ck(self._L.pies_add_linked_regions(self._h, len(m), _pf(m), w))

    def create_shape_matching_box(self, translation, cx, cy, cz, w):
        t = _f32(translation)
        self._ck(self._L.pies_create_shape_matching_box(self._h, _pf(t), cx, cy, cz, w))

    def create_shape_matching_sheet(self, W, H, translation=(0, 0, 0), scale=1.0, w=1.0):
        t = _f32(translation)
        self._ck(self._L.pies_create_shape_matching_sheet(self._h, W, H, _pf(t), scale, w))

    def group_ids(self, ctype, k):
        n = C.c_uint32()
        self._ck(self._L.pies_get_group(self._h, ctype, k, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        self._ck(self._L.pies_get_group(self._h, ctype, k, _pu(out), out.size, C.byref(n)))
        return out

    def create_tet_box(self, W, H, D, translation=(0, 0, 0), scale=1.0, velocity=(0, 0, 0), w=1.0, mass=1.0,
                       volume=True, triangles=True):
        t, v = _f32(translation), _f32(velocity)
        self._ck(self._L.pies_create_tet_box(self._h, W, H, D, _pf(t), scale, _pf(v), w, mass,
                                             (1 if volume else 0) | (2 if triangles else 0)))

    def create_box(self, W, H, D, translation=(0, 0, 0), scale=1.0, w=1.0, existing_offset=None, triangles=True):
        t = _f32(translation)
        self._ck(self._L.pies_create_box(self._h, W, H, D, _pf(t), scale, w, 0 if existing_offset is None else 1,
                                         0 if existing_offset is None else existing_offset, 2 if triangles else 0))

    def create_sheet(self, W, H, translation=(0, 0, 0), scale=1.0, mass=1.0, w=1.0):
        t = _f32(translation)
        self._ck(self._L.pies_create_sheet(self._h, W, H, _pf(t), scale, mass, w))

    def create_bend_sheet(self, W, H, translation=(0, 0, 0), scale=1.0, w=1.0):
        t = _f32(translation)
        self._ck(self._L.pies_create_bend_sheet(self._h, W, H, _pf(t), scale, w))

    def add_skin(self, vertices, tets, triangles=None, max_distance=0.0):
        """pies_add_skin: binds the render vertices (n x 3) to the listed tetrahedra (m x 4 global node ids), each vertex to one
        element with barycentric weights; `triangles` (k x 3 indices into the vertices, or None) serve the normals.  Returns the
        skin's id."""
        v = _f32(vertices).reshape(-1, 3)
        t = _u32(tets).reshape(-1, 4)
        tri = None if triangles is None else _u32(triangles).reshape(-1, 3)
        k = C.c_uint32()
        self._ck(self._L.pies_add_skin(self._h, len(v), _pf(v), 0 if tri is None else len(tri), None if tri is None else _pu(tri),
                                       len(t), _pu(t), max_distance, C.byref(k)))
        return k.value

    def skin_binding(self, skin):
        """pies_get_skin_binding: (tet, node_ids, weights) per vertex - the index into the tetrahedra given, its four nodes (host
        ids) and (w0, w1, w2, w3) as stored (w0 = 1 - (w1 + w2 + w3))."""
        n = C.c_uint32()
        if self._L.pies_get_skin_binding(self._h, skin, None, None, None, 0, C.byref(n)) != OK:
            raise PiesError("pies_get_skin_binding: no skin %d" % skin)
        tet, ids, w = np.empty(n.value, np.uint32), np.empty((n.value, 4), np.uint32), np.empty((n.value, 4), np.float32)
        if self._L.pies_get_skin_binding(self._h, skin, _pu(tet), _pu(ids), _pf(w), n.value, C.byref(n)) != OK:
            raise PiesError("pies_get_skin_binding failed")
        return tet, ids, w

    def read_skin(self, skin, normals=True):
        """pies_read_skin: the skin evaluated from the device's current node positions; (positions, normals) as (n, 3) arrays,
        or positions alone with normals=False (the normals are then not computed)."""
        n = C.c_uint32()
        if self._L.pies_get_skin_binding(self._h, skin, None, None, None, 0, C.byref(n)) != OK:
            raise PiesError("pies_read_skin: no skin %d" % skin)
        x = np.empty((n.value, 3), np.float32)
        nr = np.empty((n.value, 3), np.float32) if normals else None
        self._ck(self._L.pies_read_skin(self._h, skin, _pf(x), None if nr is None else _pf(nr), n.value))
        return (x, nr) if normals else x

    def export_acquire_skin(self, frame, skin):
        """pies_export_acquire_skin: (positions, normals) of `skin` in frame `frame` as (n, 3) float32 views of the frame's
        pinned buffers, valid until export_release(frame) like export_acquire's view."""
        p, q, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_uint32()
        self._ck(self._L.pies_export_acquire_skin(self._h, frame, skin, C.byref(p), C.byref(q), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value, 3)), np.ctypeslib.as_array(q, shape=(n.value, 3))

    def voxelize_tri_mesh(self, vertices, triangles, origin, cell, dims):
        """pies_voxelize_tri_mesh: (winding numbers float32, inside mask bool) of the cell centres origin + ((i, j, k) + 0.5) cell
        of the dims = (nx, ny, nz) lattice, both shaped dims (k fastest), evaluated on the device."""
        v = _f32(vertices).reshape(-1, 3)
        tri = _u32(triangles).reshape(-1, 3)
        o, d = _f32(origin).reshape(3), _u32(dims).reshape(3)
        w = np.empty(tuple(int(x) for x in d), np.float32)
        inside = np.empty(w.shape, np.uint8)
        self._ck(self._L.pies_voxelize_tri_mesh(self._h, len(v), _pf(v), len(tri), _pu(tri), _pf(o), cell, _pu(d), _pf(w),
                                                inside.ctypes.data_as(C.POINTER(C.c_uint8))))
        return w, inside.astype(bool)

    def add_tri_mesh_volume(self, vertices, triangles, resolution, velocity=(0, 0, 0), density=1.0, strain_stiffness=1.0,
                            min_strain=0.8, max_strain=1.0, volume_stiffness=1.0, compression=1.0, stretching=1.0):
        """pies_add_tri_mesh_volume: a closed triangle mesh as a lattice body (the cells inside the surface, six tetrahedra each)
        with the mesh bound to it as a skin.  Returns (first node, nodes, elements, skin id)."""
        v = _f32(vertices).reshape(-1, 3)
        tri = _u32(triangles).reshape(-1, 3)
        vel = _f32(velocity).reshape(3)
        out = [C.c_uint32() for _ in range(4)]
        self._ck(self._L.pies_add_tri_mesh_volume(self._h, len(v), _pf(v), len(tri), _pu(tri), _pf(vel), density, strain_stiffness,
                                                  min_strain, max_strain, volume_stiffness, compression, stretching, resolution,
                                                  *[C.byref(x) for x in out]))
        return tuple(x.value for x in out)

    def raycast(self, origins, directions, t_max=float("inf"), target=RAY_SCENE_TRIANGLES, skin=0, cull_back=False):
        """pies_raycast: the nearest hit of every ray (origins, directions: n x 3; t in units of |d|) on the scene's triangles or
        on skin `skin` (target=RAY_SKIN), at the positions the device holds now.  Returns (triangle uint32 (n), t float32 (n),
        uv float32 (n, 2)); a miss is (RAY_MISS, +inf, (0, 0))."""
        o, d = _f32(origins).reshape(-1, 3), _f32(directions).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("raycast: origins and directions differ in length")
        n = len(o)
        tri, t, uv = np.empty(n, np.uint32), np.empty(n, np.float32), np.empty((n, 2), np.float32)
        self._ck(self._L.pies_raycast(self._h, target, skin, n, _pf(o), _pf(d), t_max, RAY_CULL_BACK if cull_back else 0,
                                      _pu(tri), _pf(t), _pf(uv)))
        return tri, t, uv

    def closest_points(self, points, max_distance=float("inf"), target=RAY_SCENE_TRIANGLES, skin=0, winding=False):
        """pies_closest_points: for every point (n x 3) the closest point of the scene's triangles or of skin `skin`
        (target=RAY_SKIN) within max_distance, at the positions the device holds now.  Returns (triangle uint32 (n), distance
        float32 (n), uv float32 (n, 2), point float32 (n, 3)) and, with winding=True, the winding number float32 (n) as a fifth
        (inside a closed surface: |w| > 0.5); no candidate is (NEAR_NONE, +inf, (0, 0), the point itself)."""
        p = _f32(points).reshape(-1, 3)
        n = len(p)
        tri, dist = np.empty(n, np.uint32), np.empty(n, np.float32)
        uv, q = np.empty((n, 2), np.float32), np.empty((n, 3), np.float32)
        w = np.empty(n, np.float32) if winding else None
        self._ck(self._L.pies_closest_points(self._h, target, skin, n, _pf(p), max_distance, _pu(tri), _pf(dist), _pf(uv), _pf(q),
                                             _pf(w) if winding else None))
        return (tri, dist, uv, q, w) if winding else (tri, dist, uv, q)

    def collide_props(self, props, reaction=True, node_prop=False):
        """pies_collide_props: pushes the nodes out of the props (a sequence of Prop, applied in order) where the device holds
        them; the velocity response is relative to the moving prop.  Returns (impulse float32 (k, 3), torque float32 (k, 3), hits
        uint32 (k)) with reaction=True - the host applies -impulse and -torque (about the prop's pivot) to its own body -, followed by
        the last prop that touched every node (uint32 (n), PROP_NONE: none) with node_prop=True; None when neither is asked for."""
        return self._node_edit(self._L.pies_collide_props, Prop, props, (), reaction, node_prop)

    def _node_edit(self, call, ctype, records, dt, reaction, node_prop=None, extras=0):
        """One between-tick edit of node state through its entry point: the records as an array of ctype, dt as () or (dt,), the
        reaction outputs (impulse (k, 3), torque (k, 3), counts uint32 (k), then `extras` float32 (k) arrays; NULL without
        reaction) and, for a call that has the output (node_prop not None), the last record that touched every node.  Returns what
        was asked for as one tuple, None when nothing was."""
        records = list(records)
        k = len(records)
        arr = (ctype * max(k, 1))(*records)
        out, args = (), (None,) * (3 + extras)
        if reaction:
            out = (np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.uint32))
            args = (_pf(out[0]), _pf(out[1]), _pu(out[2]))
            for _ in range(extras):
                out += (np.zeros(k, np.float32),)
                args += (_pf(out[-1]),)
        if node_prop:
            out += (np.empty(self.count(NODES), np.uint32),)
            args += (_pu(out[-1]),)
        elif node_prop is not None:
            args += (None,)
        self._ck(call(self._h, k, arr if k else None, *dt, *args))
        return out or None

    def add_field(self, samples, origin, cell):
        """pies_add_field: a signed distance field from host samples shaped (nz, ny, nx) - sample [k, j, i] sits at the local
        position origin + (i, j, k) * cell -, negative inside.  Returns the field id."""
        v = np.ascontiguousarray(samples, dtype=np.float32)
        if v.ndim != 3:
            raise ValueError("add_field: samples must be shaped (nz, ny, nx)")
        dims = _u32(v.shape[::-1])
        o, out = _f32(origin).reshape(3), C.c_uint32()
        self._ck(self._L.pies_add_field(self._h, _pu(dims), _pf(o), cell, _pf(v), C.byref(out)))
        return out.value

    def add_field_tri_mesh(self, vertices, triangles, cell, margin):
        """pies_add_field_tri_mesh: the signed distance field of a closed triangle mesh, built on the device (brute force, once)
        on a lattice that covers the mesh's bounding box grown by margin.  Returns the field id."""
        v = _f32(vertices).reshape(-1, 3)
        tri = _u32(triangles).reshape(-1, 3)
        out = C.c_uint32()
        self._ck(self._L.pies_add_field_tri_mesh(self._h, len(v), _pf(v), len(tri), _pu(tri), cell, margin, C.byref(out)))
        return out.value

    def get_field(self, field):
        """pies_get_field: (samples float32 (nz, ny, nx), origin float32 (3), cell) of a field, from the library's host copy"""
        dims, o, cell = np.zeros(3, np.uint32), np.zeros(3, np.float32), C.c_float()
        self._ck(self._L.pies_get_field(self._h, field, _pu(dims), _pf(o), C.byref(cell), None, 0))
        v = np.empty(tuple(int(x) for x in dims[::-1]), np.float32)
        self._ck(self._L.pies_get_field(self._h, field, None, None, None, _pf(v), v.size))
        return v, o, cell.value

    def collide_field_props(self, props, reaction=True, node_prop=False):
        """pies_collide_field_props: pushes the nodes out of the field props (a sequence of FieldProp, applied in order) where the
        device holds them.  Returns what collide_props returns: (impulse, torque, hits) with reaction=True, followed by the last
        prop that touched every node with node_prop=True; None when neither is asked for."""
        return self._node_edit(self._L.pies_collide_field_props, FieldProp, props, (), reaction, node_prop)

    def apply_forces(self, forces, dt, reaction=True):
        """pies_apply_forces: changes the velocities by the forces (a sequence of Force) acting for dt seconds, where the device
        holds them; every force reads the state the call found.  Returns (impulse float32 (k, 3), torque float32 (k, 3) about each
        force's centre, nodes uint32 (k)) with reaction=True, else None."""
        return self._node_edit(self._L.pies_apply_forces, Force, forces, (dt,), reaction)

    def apply_surface_loads(self, loads, dt, reaction=True):
        """pies_apply_surface_loads: changes the velocities by the loads (a sequence of SurfaceLoad) acting for dt seconds, where
        the device holds them; every load reads the state the call found.  Returns (impulse float32 (k, 3), torque float32 (k, 3)
        about each load's point, nodes uint32 (k), volume float32 (k), area float32 (k)) with reaction=True, else None."""
        return self._node_edit(self._L.pies_apply_surface_loads, SurfaceLoad, loads, (dt,), reaction, extras=2)

    def add_anchors(self, anchors, n_frames):
        """pies_add_anchors: stores a set of anchors (a sequence of Anchor) that refer to n_frames frames.  Returns the set id.  A set
        is an asset: it survives finalize, scene edits and ticks, and ends with clear() or the handle."""
        anchors = list(anchors)
        arr = (Anchor * max(len(anchors), 1))(*anchors)
        out = C.c_uint32()
        self._ck(self._L.pies_add_anchors(self._h, len(anchors), arr if anchors else None, n_frames, C.byref(out)))
        return out.value

    def get_anchors(self, anchor_set):
        """pies_get_anchors: (anchors: a list of Anchor in the set's own order, n_frames), from the library's host copy"""
        n, frames = C.c_uint32(), C.c_uint32()
        self._ck(self._L.pies_get_anchors(self._h, anchor_set, None, 0, C.byref(n), C.byref(frames)))
        arr = (Anchor * max(n.value, 1))()
        self._ck(self._L.pies_get_anchors(self._h, anchor_set, arr, n.value, None, None))
        return [Anchor.from_buffer_copy(arr[i]) for i in range(n.value)], frames.value

    def apply_anchors(self, anchor_set, frames, dt, reaction=True, per_anchor=False):
        """pies_apply_anchors: ties the set's nodes to the frames (a sequence of AnchorFrame, as many as the set was added with) as
        they stand and move now, for dt seconds, where the device holds the nodes.  Returns (impulse float32 (f, 3), torque
        float32 (f, 3) about each frame's pivot, live uint32 (f)) with reaction=True - the host applies -impulse and -torque to its
        own body -, followed by the per-anchor array float32 (n, 4): the impulse the anchor gave its node and its stretch, in the
        set's own order, with per_anchor=True; None when neither is asked for."""
        frames = list(frames)
        k = len(frames)
        arr = (AnchorFrame * max(k, 1))(*frames)
        out, args = (), (None, None, None)
        if reaction:
            out = (np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.uint32))
            args = (_pf(out[0]), _pf(out[1]), _pu(out[2]))
        if per_anchor:
            n = C.c_uint32()
            self._ck(self._L.pies_get_anchors(self._h, anchor_set, None, 0, C.byref(n), None))
            out += (np.zeros((n.value, 4), np.float32),)
            args += (_pf(out[-1]),)
        else:
            args += (None,)
        self._ck(self._L.pies_apply_anchors(self._h, anchor_set, k, arr if k else None, dt, *args))
        return out or None

    def add_ties(self, ties, n_groups=1):
        """pies_add_ties: stores a set of ties (a sequence of Tie) that refer to n_groups groups.  Returns the set id.  A set is an
        asset: it survives finalize, scene edits and ticks, and ends with clear() or the handle."""
        ties = list(ties)
        arr = (Tie * max(len(ties), 1))(*ties)
        out = C.c_uint32()
        self._ck(self._L.pies_add_ties(self._h, len(ties), arr if ties else None, n_groups, C.byref(out)))
        return out.value

    def get_ties(self, tie_set):
        """pies_get_ties: (ties: a list of Tie in the set's own order, n_groups), from the library's host copy"""
        n, groups = C.c_uint32(), C.c_uint32()
        self._ck(self._L.pies_get_ties(self._h, tie_set, None, 0, C.byref(n), C.byref(groups)))
        arr = (Tie * max(n.value, 1))()
        self._ck(self._L.pies_get_ties(self._h, tie_set, arr, n.value, None, None))
        return [Tie.from_buffer_copy(arr[i]) for i in range(n.value)], groups.value

    def apply_ties(self, tie_set, groups, dt, iterations=4, reaction=True, per_tie=False):
        """pies_apply_ties: binds the set's nodes to their carriers for dt seconds in `iterations` Jacobi iterations, with the
        groups (a sequence of TieGroup, as many as the set was added with) of this call, where the device holds the nodes.
        Returns (impulse float32 (g, 3): what the group's ties gave their nodes a, torque float32 (g, 3) about each group's pivot,
        live uint32 (g)) with reaction=True, followed by the per-tie array float32 (n, 4): J and the stretch, in the set's own
        order, with per_tie=True; None when neither is asked for."""
        groups = list(groups)
        k = len(groups)
        arr = (TieGroup * max(k, 1))(*groups)
        out, args = (), (None, None, None)
        if reaction:
            out = (np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.uint32))
            args = (_pf(out[0]), _pf(out[1]), _pu(out[2]))
        if per_tie:
            n = C.c_uint32()
            self._ck(self._L.pies_get_ties(self._h, tie_set, None, 0, C.byref(n), None))
            out += (np.zeros((n.value, 4), np.float32),)
            args += (_pf(out[-1]),)
        else:
            args += (None,)
        self._ck(self._L.pies_apply_ties(self._h, tie_set, k, arr if k else None, dt, iterations, *args))
        return out or None

    def tie_state(self, tie_set):
        """pies_get_tie_state: the set's broken bytes (uint8 (n), 1: broken), from the library's host copy"""
        n = C.c_uint32()
        self._ck(self._L.pies_get_ties(self._h, tie_set, None, 0, C.byref(n), None))
        out = np.zeros(n.value, np.uint8)
        self._ck(self._L.pies_get_tie_state(self._h, tie_set, out.ctypes.data_as(C.POINTER(C.c_uint8)), n.value, None))
        return out

    def reset_ties(self, tie_set):
        """pies_reset_ties: no tie of the set is broken any more"""
        self._ck(self._L.pies_reset_ties(self._h, tie_set))

    def add_actuators(self, actuators, n_channels=1):
        """pies_add_actuators: stores a set of actuators (a sequence of Actuator) that refer to n_channels activation channels.
        Returns the set id.  A set is an asset: it survives finalize, scene edits and ticks, and ends with clear() or the handle."""
        if isinstance(actuators, C.Array):  # (a ctypes array of Actuator as it is: a large set built elsewhere)
            arr = actuators
        else:
            actuators = list(actuators)
            arr = (Actuator * max(len(actuators), 1))(*actuators)
        out = C.c_uint32()
        self._ck(self._L.pies_add_actuators(self._h, len(actuators), arr if len(actuators) else None, n_channels, C.byref(out)))
        return out.value

    def get_actuators(self, actuator_set):
        """pies_get_actuators: (actuators: a list of Actuator in the set's own order with `base` filled in, n_channels), from the
        library's host copy"""
        n, channels = C.c_uint32(), C.c_uint32()
        self._ck(self._L.pies_get_actuators(self._h, actuator_set, None, 0, C.byref(n), C.byref(channels)))
        arr = (Actuator * max(n.value, 1))()
        self._ck(self._L.pies_get_actuators(self._h, actuator_set, arr, n.value, None, None))
        return [Actuator.from_buffer_copy(arr[i]) for i in range(n.value)], channels.value

    def drive_actuators(self, actuator_set, activation, sums=True, per_actuator=False):
        """pies_drive_actuators: writes the rest lengths and angles of the set's constraints from the activations (one float per
        channel of the set) where the device holds the rest records - no rebuild.  Returns (sums float32 (c, 2): per channel the
        live actuators' measured values and written rests added, live uint32 (c)) with sums=True, followed by the per-actuator
        array float32 (n, 2): the rest the constraint holds after the call and its measured value (a length, or the cosine of
        the dihedral angle), in the set's own order, with per_actuator=True; None when neither is asked for."""
        u = np.ascontiguousarray(activation, np.float32).reshape(-1)
        k = len(u)
        out, args = (), (None, None)
        if sums:
            out = (np.zeros((k, 2), np.float32), np.zeros(k, np.uint32))
            args = (_pf(out[0]), _pu(out[1]))
        if per_actuator:
            n = C.c_uint32()
            self._ck(self._L.pies_get_actuators(self._h, actuator_set, None, 0, C.byref(n), None))
            out += (np.zeros((n.value, 2), np.float32),)
            args += (_pf(out[-1]),)
        else:
            args += (None,)
        self._ck(self._L.pies_drive_actuators(self._h, actuator_set, k, _pf(u) if k else None, *args))
        return out or None

    def drive_actuators_device(self, actuator_set, n_channels, activation, sums=0, live=0, per_actuator=0, stream=0, flags=0):
        """pies_drive_actuators_device: the same with the activations and the outputs at device addresses (integers; 0: not wanted),
        ordered against `stream` (0: the default stream) by events; no host synchronisation unless flags has IO_HOST_SYNC"""
        self._ck(self._L.pies_drive_actuators_device(self._h, actuator_set, n_channels, C.c_void_p(activation or None), C.c_void_p(sums or None),
                                                     C.c_void_p(live or None), C.c_void_p(per_actuator or None), C.c_void_p(stream or None),
                                                     flags))

    def measure_elements(self, ctype, first=0, n=None, records=True, summary=True):
        """pies_measure_elements: elements [first, first + n) of the TET or VOLUME container (n None: to the container's end) at
        the positions the device holds.  Returns (records, summary): a structured array of ELEMENT_MEASURE_DTYPE (s, j, volume,
        i1, green, flags) or None, and an ElementSummary or None."""
        if n is None:
            n = self.count(ctype) - first
        rec = np.zeros(n, ELEMENT_MEASURE_DTYPE) if records else None
        summ = ElementSummary() if summary else None
        self._ck(self._L.pies_measure_elements(self._h, ctype, first, n,
                                               rec.ctypes.data_as(C.POINTER(ElementMeasure)) if records else None,
                                               C.byref(summ) if summary else None))
        return rec, summ

    def measure_nodes(self, ranges, about=None):
        """pies_measure_nodes: mass, momentum, angular momentum about `about` (one point per range; None: the origin), first
        moment, kinetic energy and node counts of up to MEASURE_RANGE_MAX (first, count) ranges of host node ids, summed where
        the device holds the nodes.  Returns a structured array of NODE_SUMS_DTYPE, one entry per range."""
        r = np.ascontiguousarray(ranges, np.uint32).reshape(-1, 2)
        k = len(r)
        a = None if about is None else np.ascontiguousarray(about, np.float32).reshape(k, 3)
        out = np.zeros(k, NODE_SUMS_DTYPE)
        self._ck(self._L.pies_measure_nodes(self._h, k, _pu(r) if k else None, None if a is None or not k else _pf(a),
                                            out.ctypes.data_as(C.POINTER(NodeSums)) if k else None))
        return out

    def clear(self):
        self._ck(self._L.pies_clear(self._h))

    # -- configuration -------------------------------------------------------------------------
    def set_flag(self, flag, value):
        self._ck(self._L.pies_set_flag(self._h, flag, int(value)))

    def set_schedule(self, schedule):
        self._ck(self._L.pies_set_schedule(self._h, schedule))

    def set_solver(self, solver):
        self._ck(self._L.pies_set_solver(self._h, solver))

    def set_pcg(self, rel_tol, max_iters):
        self._ck(self._L.pies_set_pcg(self._h, rel_tol, max_iters))

    def pcg_stats(self):
        """(max relative residual, max CG iterations used, number of solves) over the last tick."""
        r, it, n = C.c_float(), C.c_uint32(), C.c_uint32()
        self._ck(self._L.pies_get_pcg_stats(self._h, C.byref(r), C.byref(it), C.byref(n)))
        return r.value, it.value, n.value

    def set_pcg_retry(self, enabled):
        self._ck(self._L.pies_set_pcg_retry(self._h, int(enabled)))

    def pcg_health(self):
        """dict: short_solves / solves (kept substeps, since finalize), substeps_retried, budget (CG iterations captured)."""
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._ck(self._L.pies_get_pcg_health(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(short_solves=a.value, solves=b.value, substeps_retried=c.value, budget=d.value)

    def finalize(self):
        self._ck(self._L.pies_finalize(self._h))

    # -- hot path ------------------------------------------------------------------------------
    def tick(self, n=1):
        for _ in range(n):
            self._ck(self._L.pies_tick(self._h))

    def tick_async(self, n=1):
        for _ in range(n):
            self._ck(self._L.pies_tick_async(self._h))

    def synchronize(self):
        self._ck(self._L.pies_synchronize(self._h))

    def tick_begin(self):
        """Queues one tick and the asynchronous export of its positions; returns the frame id."""
        f = C.c_uint64()
        self._ck(self._L.pies_tick_begin(self._h, C.byref(f)))
        return f.value

    def export_acquire(self, frame):
        """Blocks until `frame` has landed in pinned host memory; returns an (n, 4) float32 view (x, y, z, invMass)
        that is valid until export_release(frame)."""
        p, n = C.POINTER(C.c_float)(), C.c_uint32()
        self._ck(self._L.pies_export_acquire(self._h, frame, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros((0, 4), np.float32)
        return np.ctypeslib.as_array(p, shape=(n.value, 4))

    def export_release(self, frame):
        self._ck(self._L.pies_export_release(self._h, frame))

    def read_positions_strided(self, stride_floats):
        n = self.count(NODES)
        out = np.zeros((n, stride_floats), dtype=np.float32)
        self._ck(self._L.pies_read_positions_strided(self._h, out.ctypes.data_as(C.c_void_p), 4 * stride_floats, n))
        return out

    def last_error(self):
        return self._L.pies_last_error(self._h).decode()

    @property
    def failed(self):
        f = C.c_int()
        self._ck(self._L.pies_failed(self._h, C.byref(f)))
        return bool(f.value)

    @property
    def tri_collisions(self):
        n = C.c_uint32()
        self._ck(self._L.pies_get_tri_contacts(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 4), dtype=np.uint32)
        if n.value:
            self._ck(self._L.pies_get_tri_contacts(self._h, _pu(out), n.value, C.byref(n)))
        return out

    def node_contacts(self):
        """pies_get_node_contacts: the last PD substep's node-node contacts (FLAG_PD_NODE_CONTACTS) as an (m, 2) array of host ids,
        in the order the friction loop ran them"""
        n = C.c_uint32()
        self._ck(self._L.pies_get_node_contacts(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), dtype=np.uint32)
        if n.value:
            self._ck(self._L.pies_get_node_contacts(self._h, _pu(out), n.value, C.byref(n)))
        return out[: n.value]

    def tri_grid_stats(self):
        """pies_get_tri_grid_stats: the broad phase of the last PD substep's point-triangle detection."""
        out = np.zeros(8, dtype=np.uint32)
        self._ck(self._L.pies_get_tri_grid_stats(self._h, _pu(out)))
        return {"ccd_pairs": int(out[0]), "hit_pairs": int(out[1]), "longest": out[2:5].tolist(), "listed": out[5:8].tolist()}

    @property
    def collision_pairs(self):
        n = C.c_uint64()
        self._ck(self._L.pies_collision_pairs(self._h, C.byref(n)))
        return n.value

    def collision_stats(self):
        """(resolved pairs, candidates looked at) since the last call"""
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.pies_collision_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pair_state(self):
        n = self.count(NODES)
        sl, ex, dg = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
        self._ck(self._L.pies_debug_pair_state(self._h, sl.ctypes.data_as(C.POINTER(C.c_float)), ex.ctypes.data_as(C.POINTER(C.c_float)),
                                               dg.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return sl, ex, dg

    def set_collision_rounds(self, rounds):
        self._ck(self._L.pies_set_collision_rounds(self._h, rounds))

    def collision_health(self):
        """pair order: levels and listed pairs of the last pass; passes repeated / inexact since finalize"""
        v = [C.c_uint32() for _ in range(4)]
        self._ck(self._L.pies_get_collision_health(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("levels", "pairs_listed", "passes_repeated", "passes_inexact"), (x.value for x in v)))

    @property
    def collision_fallbacks(self):
        """node-node passes the reference's sequential loop ran in place of a parallel order (pies_get_collision_fallbacks)"""
        v = C.c_uint32()
        self._ck(self._L.pies_get_collision_fallbacks(self._h, C.byref(v)))
        return v.value

    # -- state ---------------------------------------------------------------------------------
    def count(self, what):
        out = C.c_uint32()
        self._ck(self._L.pies_count(self._h, what, C.byref(out)))
        return out.value

    def _read(self, what, cols):
        n = self.count(NODES)
        out = np.empty((n, cols) if cols > 1 else (n,), dtype=np.float32)
        self._ck(self._L.pies_read_nodes(self._h, what, _pf(out), n))
        return out

    def _write(self, what, a):
        a = _f32(a)
        self._ck(self._L.pies_write_nodes(self._h, what, _pf(a), self.count(NODES)))

    positions = property(lambda self: self._read(NODE_POSITION, 3))
    prev_positions = property(lambda self: self._read(NODE_PREV_POSITION, 3))
    velocities = property(lambda self: self._read(NODE_VELOCITY, 3))
    radii = property(lambda self: self._read(NODE_RADIUS, 1))
    inv_masses = property(lambda self: self._read(NODE_INV_MASS, 1))

    def set_positions(self, p):
        self._write(NODE_POSITION, p)

    def set_prev_positions(self, p):
        self._write(NODE_PREV_POSITION, p)

    def set_velocities(self, v):
        self._write(NODE_VELOCITY, v)

    def set_radii(self, r):
        self._write(NODE_RADIUS, r)

    def set_inv_masses(self, m):
        self._write(NODE_INV_MASS, m)

    # -- the same, to and from device memory (integer addresses; pies_amd.tensors speaks torch tensors) --
    @staticmethod
    def _device_nodes(position, prev_position, velocity, radius, inv_mass, stride):
        return DeviceNodes(position or None, prev_position or None, velocity or None, radius or None, inv_mass or None, stride)

    def read_nodes_device(self, position=0, prev_position=0, velocity=0, radius=0, inv_mass=0, stride=3, n=None, stream=0, flags=0):
        """pies_read_nodes_device: the named arrays (device addresses; `stride` floats per node, radius and inv_mass one) filled
        in host numbering on the solver's stream, ordered against `stream` (a hipStream_t as an integer, 0: the default stream)
        by events; no host synchronisation unless flags has IO_HOST_SYNC."""
        a = self._device_nodes(position, prev_position, velocity, radius, inv_mass, stride)
        self._ck(self._L.pies_read_nodes_device(self._h, C.byref(a), self.count(NODES) if n is None else n, stream or None, flags))

    def write_nodes_device(self, position=0, prev_position=0, velocity=0, stride=3, ids=0, m=None, stream=0, flags=0):
        """pies_write_nodes_device: positions, previous positions and / or velocities replaced in HBM from device arrays; ids (a
        device array of m host ids) names the nodes of the rows, 0: row k is node k and m is the node count."""
        a = self._device_nodes(position, prev_position, velocity, 0, 0, stride)
        self._ck(self._L.pies_write_nodes_device(self._h, C.byref(a), ids or None, self.count(NODES) if m is None else m,
                                                 stream or None, flags))

    def skin_vertex_count(self, skin):
        n = C.c_uint32()
        if self._L.pies_get_skin_binding(self._h, skin, None, None, None, 0, C.byref(n)) != OK:
            raise PiesError("no skin %d" % skin)
        return n.value

    def read_skin_device(self, skin, positions, normals=0, n=None, stream=0, flags=0):
        """pies_read_skin_device: pies_read_skin into device arrays (n x 3 floats each; normals 0: not computed)"""
        self._ck(self._L.pies_read_skin_device(self._h, skin, positions or None, normals or None,
                                               self.skin_vertex_count(skin) if n is None else n, stream or None, flags))

    def ids(self, ctype):
        n, k = self.count(ctype), _IDS_PER[ctype]
        out = np.empty((n, k) if k > 1 else (n,), dtype=np.uint32)
        self._ck(self._L.pies_get_ids(self._h, ctype, _pu(out), out.size))
        return out

    def rest(self, ctype):
        n, k = self.count(ctype), _REST_PER[ctype]
        out = np.empty((n, k) if k > 1 else (n,), dtype=np.float32)
        self._ck(self._L.pies_get_rest(self._h, ctype, _pf(out), out.size))
        return out

    def set_rest(self, ctype, rest, first=0):
        """pies_set_rest: rest data of constraints first .. of a container (DISTANCE target, TET / VOLUME Qinv column-major, BEND angle)"""
        r = np.ascontiguousarray(rest, dtype=np.float32)
        n = r.size // _REST_PER[ctype]
        self._ck(self._L.pies_set_rest(self._h, ctype, first, n, _pf(r)))

    def order(self, ctype):
        out = np.empty(self.count(ctype), dtype=np.uint32)
        self._ck(self._L.pies_get_order(self._h, ctype, _pu(out), out.size))
        return out

    def node_order(self):
        """pies_get_node_order: order[internal] = host id (the identity unless FLAG_RENUMBER_NODES renumbered the scene)"""
        out = np.empty(self.count(NODES), dtype=np.uint32)
        self._ck(self._L.pies_get_node_order(self._h, _pu(out), out.size))
        return out

    def pd_tile_plan(self):
        """pies_get_pd_tile_plan: None when the scene keeps per-(element, node) records, otherwise a dict of the plan's arrays
        (info: nodes | elements << 16 per tile; node, elem, local: 128 per tile; nptr: 132 per tile; inc: 512 per tile)."""
        nt = C.c_uint32()
        self._ck(self._L.pies_get_pd_tile_plan(self._h, C.byref(nt), None, None, None, None, None, None, 0))
        n = nt.value
        if n == 0:
            return None
        info, node, elem, local = (np.empty(k * n, dtype=np.uint32) for k in (1, 128, 128, 128))
        nptr, inc = np.empty(132 * n, dtype=np.uint16), np.empty(512 * n, dtype=np.uint16)
        p16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))  # noqa: E731
        self._ck(self._L.pies_get_pd_tile_plan(self._h, C.byref(nt), _pu(info), _pu(node), _pu(elem), _pu(local), p16(nptr), p16(inc), n))
        return {"info": info, "node": node.reshape(n, 128), "elem": elem.reshape(n, 128), "local": local.reshape(n, 128),
                "nptr": nptr.reshape(n, 132), "inc": inc.reshape(n, 512)}

    def batches(self, ctype):
        nb = C.c_uint32()
        self._ck(self._L.pies_get_batches(self._h, ctype, None, 0, C.byref(nb)))
        offs = np.empty(nb.value + 1, dtype=np.uint32)
        self._ck(self._L.pies_get_batches(self._h, ctype, _pu(offs), offs.size, C.byref(nb)))
        return offs

    # -- measurement ---------------------------------------------------------------------------
    def launch_counts(self):
        out = np.zeros(KERNEL_COUNT, dtype=np.uint32)
        self._ck(self._L.pies_launch_counts(self._h, _pu(out)))
        return dict(zip(KERNEL_NAMES, out.tolist()))

    def profile_in_situ(self, kernel, substeps=3):
        """Whole substeps launched eagerly with HIP events around every launch of `kernel` (all other kernels run as
        well, so caches are in the state the substep leaves them in); returns (launches, ms, units, bracket_overhead_ms):
        ms is the sum of the brackets, bracket_overhead_ms what one bracket costs around nothing (calibrated in the same
        pass with an empty kernel)."""
        n, ms, units, ov = C.c_uint32(), C.c_double(), C.c_uint64(), C.c_double()
        self._ck(self._L.pies_profile_in_situ(self._h, kernel, substeps, C.byref(n), C.byref(ms), C.byref(units), C.byref(ov)))
        return n.value, ms.value, units.value, ov.value

    def profile_substep(self, kernel):
        """One un-graphed substep with per-dispatch timing of `kernel`; returns (launches, ms, units)."""
        n, ms, units = C.c_uint32(), C.c_double(), C.c_uint64()
        self._ck(self._L.pies_profile_substep(self._h, kernel, C.byref(n), C.byref(ms), C.byref(units)))
        return n.value, ms.value, units.value

"""ctypes binding of include/pbf_hip.h (libpbf_hip.so).  Plumbing only: no numerics here."""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# PBF_HIP_LIB: A/B another build of the same sources (diagnostic; tools/ab_flags.sh)
LIB_PATH = os.environ.get("PBF_HIP_LIB") or os.path.join(PKG_DIR, "libpbf_hip.so")

ABI_VERSION = 1
FLAG_STAGE_TIMING = 1 << 0
FLAG_FAST_MATH = 1 << 1
FLAG_NO_LDS = 1 << 2

BUF_KEYS, BUF_TABLE, BUF_PSTAR = 0, 1, 2
BUF_NBR_COUNT = 3
BUF_OMEGA = 4
BUF_SURFACE = 5
BUF_DENSITY = 6
BUF_WHITEWATER = 7
BUF_COLLIDER_PUSH = 8
WW_SPRAY, WW_FOAM, WW_BUBBLE = 0, 1, 2
DIAG_DENSITY = 1 << 0
SAMPLE_VELOCITY, SAMPLE_COLOUR = 1 << 0, 1 << 1
MESH_NEGATE = 1 << 0
MESH_SIGN_WINDING = 1 << 2
MESH_RECORD = 30
MESH_SOUP_RECORD = 9


class PbfError(RuntimeError):
    pass


class Desc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("fp64", C.c_int32),
        ("device", C.c_int32),
        ("flags", C.c_uint32),
        ("h", C.c_double),
        ("stream", C.c_void_p),
    ]


class Params(C.Structure):
    _fields_ = [
        ("dt", C.c_double),
        ("scale", C.c_double),
        ("iteration", C.c_uint64),
        ("constant_force", C.c_double * 3),
        ("min_bound", C.c_double * 3),
        ("max_bound", C.c_double * 3),
        ("n_wells", C.c_int32),
        ("wells", C.POINTER(C.c_double)),
        ("xsph", C.c_int32),
        ("vorticity", C.c_int32),
    ]

    def copy(self):
        p = Params()
        C.memmove(C.byref(p), C.byref(self), C.sizeof(Params))
        if hasattr(self, "_wells_keepalive"):
            p._wells_keepalive = self._wells_keepalive
        return p

    def set_wells(self, wells):
        if wells is None or len(wells) == 0:
            self.n_wells, self.wells = 0, None
            return self
        w = np.ascontiguousarray(wells, dtype=np.float64).reshape(-1, 4)
        self._wells_keepalive = w
        self.n_wells = w.shape[0]
        self.wells = w.ctypes.data_as(C.POINTER(C.c_double))
        return self


class McParams(C.Structure):
    """sph::McParams (sph.hpp:82-95); defaults = simpleConfigWith2Cubes' (sph.hpp:179-184)."""
    _fields_ = [("resolution", C.c_double), ("isolevel", C.c_double), ("particle_size", C.c_double),
                ("particle_influence", C.c_double)]

    def __init__(self, resolution=2.0, isolevel=100.0, particle_size=25.0, particle_influence=0.5):
        super().__init__(resolution, isolevel, particle_size, particle_influence)


class SlabCut(C.Structure):
    _fields_ = [("xlo", C.c_uint32), ("xhi", C.c_uint32), ("has_left", C.c_int32), ("has_right", C.c_int32)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                          C.c_void_p, C.c_size_t)


class Source(C.Structure):
    """sph::Source (sph.hpp:62-67)"""
    _fields_ = [("tag", C.c_uint64), ("centre", C.c_double * 3), ("velocity", C.c_double * 3), ("colour", C.c_double * 4),
                ("rate", C.c_double)]


class Drain(C.Structure):
    """sph::Drain (sph.hpp:69-72)"""
    _fields_ = [("centre", C.c_double * 3), ("width", C.c_double)]


class Diag(C.Structure):
    """pbf_diag (include/pbf_hip.h): 27 eight-byte words"""
    _fields_ = [("n_fluid", C.c_uint64), ("n_obstacle", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("mass", C.c_double), ("moment", C.c_double * 3), ("momentum", C.c_double * 3), ("kinetic", C.c_double),
                ("max_speed", C.c_double), ("aabb_min", C.c_double * 3), ("aabb_max", C.c_double * 3),
                ("n_density", C.c_uint64), ("nbr_max", C.c_uint64),
                ("rho_min", C.c_double), ("rho_max", C.c_double), ("rho_mean", C.c_double), ("err_mean", C.c_double),
                ("err_max", C.c_double), ("compression_mean", C.c_double), ("nbr_mean", C.c_double)]

    def as_dict(self):
        out = {}
        for name, t in self._fields_:
            v = getattr(self, name)
            out[name] = np.array(v[:], np.float64) if hasattr(v, "__len__") else (int(v) if t is C.c_uint64 else float(v))
        return out


class SampleOut(C.Structure):
    """pbf_sample_out (include/pbf_hip.h): six caller-owned host arrays, any may be NULL"""
    _fields_ = [("rho", C.c_void_p), ("weight", C.c_void_p), ("mv", C.c_void_p), ("mc", C.c_void_p),
                ("count", C.c_void_p), ("outside", C.c_void_p)]


class Whitewater(C.Structure):
    """pbf_whitewater (include/pbf_hip.h)"""
    _fields_ = [("capacity", C.c_uint64), ("seed", C.c_uint64), ("k_ta", C.c_double), ("k_wc", C.c_double),
                ("tau_ta", C.c_double * 2), ("tau_wc", C.c_double * 2), ("tau_k", C.c_double * 2),
                ("lifetime", C.c_double * 2), ("k_b", C.c_double), ("k_d", C.c_double),
                ("spray_below", C.c_uint32), ("bubble_from", C.c_uint32)]


class WhitewaterStats(C.Structure):
    """pbf_whitewater_stats (include/pbf_hip.h): 7 eight-byte words"""
    _fields_ = [("alive", C.c_uint64), ("emitted", C.c_uint64), ("dropped", C.c_uint64), ("died", C.c_uint64),
                ("kind", C.c_uint64 * 3)]


class WhitewaterSolids(C.Structure):
    """pbf_whitewater_solids (include/pbf_hip.h): two doubles and two 32-bit words, 24 bytes"""
    _fields_ = [("restitution", C.c_double), ("friction", C.c_double), ("absorb", C.c_uint32), ("reserved", C.c_uint32)]


class WhitewaterSolidsStats(C.Structure):
    """pbf_whitewater_solids_stats (include/pbf_hip.h): 5 eight-byte words"""
    _fields_ = [("hit_collider", C.c_uint64), ("hit_scenery", C.c_uint64), ("absorbed", C.c_uint64),
                ("born_inside", C.c_uint64), ("step", C.c_uint64)]


class Anisotropy(C.Structure):
    """pbf_anisotropy (include/pbf_hip.h)"""
    _fields_ = [("smoothing", C.c_double), ("k_r", C.c_double), ("k_s", C.c_double), ("k_n", C.c_double),
                ("min_neighbours", C.c_uint32)]


class AnisotropyOut(C.Structure):
    """pbf_anisotropy_out (include/pbf_hip.h): five caller-owned host arrays, any may be NULL"""
    _fields_ = [("centre", C.c_void_p), ("G", C.c_void_p), ("axes", C.c_void_p), ("radii", C.c_void_p),
                ("neighbours", C.c_void_p)]


class AnisoSurface(C.Structure):
    """pbf_aniso_surface (include/pbf_hip.h)"""
    _fields_ = [("resolution", C.c_double), ("isolevel", C.c_double), ("kernel", Anisotropy)]


class ColliderSdf(C.Structure):
    """pbf_collider_sdf (include/pbf_hip.h)"""
    _fields_ = [("dims", C.c_uint32 * 3), ("origin", C.c_double * 3), ("spacing", C.c_double), ("margin", C.c_double),
                ("phi", C.c_void_p)]


class ColliderPose(C.Structure):
    """pbf_collider_pose (include/pbf_hip.h)"""
    _fields_ = [("rot", C.c_double * 9), ("trans", C.c_double * 3)]


class ColliderWrench(C.Structure):
    """pbf_collider_wrench (include/pbf_hip.h)"""
    _fields_ = [("impulse", C.c_double * 3), ("angular", C.c_double * 3), ("abs_impulse", C.c_double * 3),
                ("abs_angular", C.c_double * 3), ("hits", C.c_uint64), ("particles", C.c_uint64), ("step", C.c_uint64)]

    def as_dict(self):
        d = {k: np.array(getattr(self, k)) for k in ("impulse", "angular", "abs_impulse", "abs_angular")}
        d.update(hits=int(self.hits), particles=int(self.particles), step=int(self.step))
        return d


class ColliderBody(C.Structure):
    """pbf_collider_body (include/pbf_hip.h)"""
    _fields_ = [("mass", C.c_double), ("inertia", C.c_double * 3), ("gain", C.c_double), ("linear_damping", C.c_double),
                ("angular_damping", C.c_double), ("accel", C.c_double * 3), ("linear_factor", C.c_double * 3),
                ("angular_factor", C.c_double * 3), ("centre_min", C.c_double * 3), ("centre_max", C.c_double * 3),
                ("pose", ColliderPose), ("velocity", C.c_double * 3), ("angular_velocity", C.c_double * 3)]


class ColliderBodyState(C.Structure):
    """struct pbf_collider_body_state (include/pbf_hip.h)"""
    _fields_ = [("pose", ColliderPose), ("quat", C.c_double * 4), ("velocity", C.c_double * 3), ("angular_velocity", C.c_double * 3),
                ("impulse", C.c_double * 3), ("angular", C.c_double * 3), ("hits", C.c_uint64), ("steps", C.c_uint64),
                ("rejected", C.c_uint64)]

    def as_dict(self):
        d = {k: np.array(getattr(self, k)) for k in ("quat", "velocity", "angular_velocity", "impulse", "angular")}
        d.update(rot=np.array(self.pose.rot).reshape(3, 3), centre=np.array(self.pose.trans), hits=int(self.hits),
                 steps=int(self.steps), rejected=int(self.rejected))
        return d


def collider_body(mass, inertia=(1.0, 1.0, 1.0), rot=np.eye(3), centre=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0),
                  angular_velocity=(0.0, 0.0, 0.0), gain=0.49, accel=(0.0, 0.0, 0.0), linear_damping=0.0, angular_damping=0.0,
                  linear_factor=(1.0, 1.0, 1.0), angular_factor=(1.0, 1.0, 1.0), centre_min=(-np.inf,) * 3, centre_max=(np.inf,) * 3):
    """-> a filled ColliderBody (the arguments of Solver.set_collider_body)"""
    b = ColliderBody()
    b.mass, b.gain, b.linear_damping, b.angular_damping = float(mass), float(gain), float(linear_damping), float(angular_damping)
    for name, v in (("inertia", inertia), ("accel", accel), ("linear_factor", linear_factor), ("angular_factor", angular_factor),
                    ("centre_min", centre_min), ("centre_max", centre_max), ("velocity", velocity), ("angular_velocity", angular_velocity)):
        getattr(b, name)[:] = [float(x) for x in np.asarray(v, np.float64).reshape(3)]
    b.pose.rot[:] = [float(x) for x in np.asarray(rot, np.float64).reshape(9)]
    b.pose.trans[:] = [float(x) for x in np.asarray(centre, np.float64).reshape(3)]
    return b


class BodyContact(C.Structure):
    """pbf_body_contact (include/pbf_hip.h)"""
    _fields_ = [("level", C.c_double), ("stride", C.c_uint32), ("skin", C.c_double), ("restitution", C.c_double),
                ("friction", C.c_double), ("correction", C.c_double), ("slop", C.c_double), ("iterations", C.c_uint32)]


class BodyContactState(C.Structure):
    """struct pbf_body_contact_state (include/pbf_hip.h)"""
    _fields_ = [("depth_sum", C.c_double), ("push", C.c_double * 3), ("arm", C.c_double * 3), ("depth_max", C.c_double),
                ("impulse", C.c_double * 3), ("shift", C.c_double * 3), ("points", C.c_uint64), ("passes", C.c_uint64),
                ("contacts", C.c_uint64), ("rejected", C.c_uint64)]

    def as_dict(self):
        d = {k: np.array(getattr(self, k)) for k in ("push", "arm", "impulse", "shift")}
        d.update(depth_sum=float(self.depth_sum), depth_max=float(self.depth_max), points=int(self.points), passes=int(self.passes),
                 contacts=int(self.contacts), rejected=int(self.rejected))
        return d


class ColliderFriction(C.Structure):
    """pbf_collider_friction (include/pbf_hip.h)"""
    _fields_ = [("mu", C.c_double), ("velocity", C.c_double * 3), ("angular_velocity", C.c_double * 3)]


class Mesh(C.Structure):
    """pbf_mesh (include/pbf_hip.h)"""
    _fields_ = [("n_vertices", C.c_uint64), ("n_triangles", C.c_uint64), ("vertices", C.c_void_p), ("triangles", C.c_void_p)]


class MeshInfo(C.Structure):
    """pbf_mesh_info (include/pbf_hip.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("n_edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges",
                                          "degenerate_triangles")] + \
               [("volume", C.c_double), ("aabb_min", C.c_double * 3), ("aabb_max", C.c_double * 3)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_[:5]}
        d.update(volume=float(self.volume), aabb_min=tuple(self.aabb_min), aabb_max=tuple(self.aabb_max))
        return d


class MeshSdfStats(C.Structure):
    """pbf_mesh_sdf_stats (include/pbf_hip.h)"""
    _fields_ = [("pairs_total", C.c_uint64), ("pairs_tested", C.c_uint64)]


class AosLayout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("stride", "off_id", "off_type", "off_mass", "off_pos", "off_vel",
                                          "off_colour")]


def build(force=False):
    """Compile libpbf_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        r = subprocess.run(["make", "-C", PKG_DIR], capture_output=True, text=True)
        if r.returncode != 0:
            raise PbfError("building libpbf_hip.so failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


_lib = None

_SIGS = {
    "pbf_abi_version": (C.c_int, []),
    "pbf_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "pbf_set_surface_tension": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "pbf_set_collider": (C.c_int, [C.c_void_p, C.POINTER(ColliderSdf)]),
    "pbf_collider_sample": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_set_collider_pose": (C.c_int, [C.c_void_p, C.POINTER(ColliderPose)]),
    "pbf_set_collider_reaction": (C.c_int, [C.c_void_p, C.c_int]),
    "pbf_collider_reaction": (C.c_int, [C.c_void_p, C.POINTER(ColliderWrench)]),
    "pbf_set_collider_body": (C.c_int, [C.c_void_p, C.POINTER(ColliderBody)]),
    "pbf_collider_body_state": (C.c_int, [C.c_void_p, C.POINTER(ColliderBodyState)]),
    "pbf_stage_body": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_set_collider_body_contact": (C.c_int, [C.c_void_p, C.POINTER(BodyContact)]),
    "pbf_collider_body_contact_points": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "pbf_collider_body_contact_state": (C.c_int, [C.c_void_p, C.POINTER(BodyContactState)]),
    "pbf_set_collider_friction": (C.c_int, [C.c_void_p, C.POINTER(ColliderFriction)]),
    "pbf_collider_friction_reaction": (C.c_int, [C.c_void_p, C.POINTER(ColliderWrench)]),
    "pbf_mesh_records": (C.c_int, [C.POINTER(Mesh), C.c_int, C.c_void_p, C.POINTER(MeshInfo)]),
    "pbf_sdf_from_mesh": (C.c_int, [C.c_void_p, C.POINTER(Mesh), C.POINTER(ColliderSdf), C.c_uint32, C.c_void_p, C.POINTER(MeshSdfStats)]),
    "pbf_set_collider_mesh": (C.c_int, [C.c_void_p, C.POINTER(Mesh), C.POINTER(ColliderSdf), C.c_uint32, C.POINTER(MeshSdfStats)]),
    "pbf_mesh_soup_records": (C.c_int, [C.POINTER(Mesh), C.c_int, C.c_void_p, C.POINTER(MeshInfo)]),
    "pbf_mesh_winding": (C.c_int, [C.c_void_p, C.POINTER(Mesh), C.POINTER(ColliderSdf), C.c_void_p]),
    "pbf_set_scenery": (C.c_int, [C.c_void_p, C.POINTER(ColliderSdf)]),
    "pbf_set_scenery_mesh": (C.c_int, [C.c_void_p, C.POINTER(Mesh), C.POINTER(ColliderSdf), C.c_uint32, C.POINTER(MeshSdfStats)]),
    "pbf_scenery_sample": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_create": (C.c_int, [C.POINTER(Desc), C.POINTER(C.c_void_p)]),
    "pbf_destroy": (None, [C.c_void_p]),
    "pbf_last_error": (C.c_char_p, [C.c_void_p]),
    "pbf_upload": (C.c_int, [C.c_void_p, C.c_size_t] + [C.c_void_p] * 6),
    "pbf_download": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "pbf_count": (C.c_size_t, [C.c_void_p]),
    "pbf_upload_aos": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(AosLayout)]),
    "pbf_download_aos": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AosLayout)]),
    "pbf_download_aos_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AosLayout)]),
    "pbf_download_aos_end": (C.c_int, [C.c_void_p]),
    "pbf_step": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_steps": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_uint32]),
    "pbf_sync": (C.c_int, [C.c_void_p]),
    "pbf_graph_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pbf_stage_predict": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_stage_sort": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_stage_diffuse": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_stage_lambda": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_stage_delta": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_stage_finalise": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_stage_scene": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_set_sources": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pbf_set_drains": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pbf_scene_host_syncs": (C.c_uint64, [C.c_void_p]),
    "pbf_query_cells": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pbf_diagnostics": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_uint32, C.POINTER(Diag)]),
    "pbf_sample_points": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_size_t, C.c_void_p, C.c_uint32, C.POINTER(SampleOut)]),
    "pbf_sample_lattice": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.POINTER(SampleOut)]),
    "pbf_anisotropy_compute": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(Anisotropy), C.POINTER(AnisotropyOut)]),
    "pbf_whitewater_configure": (C.c_int, [C.c_void_p, C.POINTER(Whitewater)]),
    "pbf_whitewater_upload": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_whitewater_step": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(WhitewaterStats)]),
    "pbf_whitewater_count": (C.c_size_t, [C.c_void_p]),
    "pbf_whitewater_download": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "pbf_set_whitewater_solids": (C.c_int, [C.c_void_p, C.POINTER(WhitewaterSolids)]),
    "pbf_whitewater_solids_stats": (C.c_int, [C.c_void_p, C.POINTER(WhitewaterSolidsStats)]),
    "pbf_read_buffer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "pbf_table_size": (C.c_size_t, [C.c_void_p]),
    "pbf_selftest_math": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pbf_selftest_divides": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pbf_grid_extent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                  C.c_int]),
    "pbf_reset_stage_times": (C.c_int, [C.c_void_p]),
    "pbf_surface": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(C.c_uint64)]),
    "pbf_download_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_map_mesh": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "pbf_read_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_surface_indexed": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pbf_surface_anisotropic": (C.c_int, [C.c_void_p, C.POINTER(Params), C.POINTER(AnisoSurface), C.c_int, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "pbf_download_mesh_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_map_mesh_indexed": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p)]),
    "pbf_reserve": (C.c_int, [C.c_void_p, C.c_size_t]),
    "pbf_slab_configure": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "pbf_slab_record_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "pbf_slab_migrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pbf_slab_add_migrants": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "pbf_slab_ghosts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pbf_slab_add_ghosts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "pbf_slab_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_slab_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbf_slab_finish": (C.c_int, [C.c_void_p]),
    "pbf_owned_count": (C.c_size_t, [C.c_void_p]),
    "pbf_slab_column_histogram": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pbf_comm_unique_id": (C.c_int, [C.c_void_p]),
    "pbf_comm_create_rccl": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pbf_comm_create_host_callback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "pbf_comm_destroy": (None, [C.c_void_p]),
    "pbf_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "pbf_comm_rounds": (C.c_uint64, [C.c_void_p]),
    "pbf_comm_allreduce_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pbf_slab_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "pbf_slab_set_cuts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pbf_slab_step": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "pbf_slab_steps": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_uint32]),
    "pbf_slab_host_syncs": (C.c_uint64, [C.c_void_p]),
    "pbf_scene_cubes": (C.c_size_t, [C.c_int, C.c_size_t] + [C.c_void_p] * 6),
    "pbf_scene_dambreak": (C.c_size_t, [C.c_int, C.c_size_t] + [C.c_void_p] * 6 + [C.POINTER(C.c_double)]),
    "pbf_apply_motion": (None, [C.c_int, C.POINTER(Params), C.c_uint64, C.POINTER(Params)]),
    "pbf_default_params": (None, [C.c_uint64, C.c_double, C.POINTER(Params)]),
}


def exported_symbols():
    """Every entry point include/pbf_hip.h declares (checked by the CPU test-suite)."""
    return sorted(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PbfError(f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        if L.pbf_abi_version() != ABI_VERSION:
            raise PbfError("libpbf_hip.so ABI version mismatch")
        _lib = L
    return _lib


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_params(iteration=4, box_side=1000.0):
    p = Params()
    lib().pbf_default_params(iteration, box_side, C.byref(p))
    return p


def apply_motion(base, frame, fp64=False):
    out = Params()
    lib().pbf_apply_motion(int(fp64), C.byref(base), frame, C.byref(out))
    return out


def _scene(fn, fp64, *args):
    dt = np.float64 if fp64 else np.float32
    n = fn(int(fp64), *args, None, None, None, None, None, None)
    out = dict(id=np.empty(n, np.uint64), type=np.empty(n, np.uint8), mass=np.empty(n, dt), pos=np.empty((n, 3), dt),
               vel=np.empty((n, 3), dt), colour=np.empty((n, 4), dt))
    return n, out


def scene_cubes(count, fp64=False):
    """simpleConfigWith2Cubes particles (sph.hpp:160-166)."""
    L = lib()
    n, o = _scene(lambda f, c, *a: L.pbf_scene_cubes(f, c, *a), fp64, count)
    L.pbf_scene_cubes(int(fp64), count, _vp(o["id"]), _vp(o["type"]), _vp(o["mass"]), _vp(o["pos"]), _vp(o["vel"]),
                      _vp(o["colour"]))
    return o


def scene_dambreak(nominal, fp64=False):
    """Dam-break column. Returns (particles, box_side)."""
    L = lib()
    side = C.c_double()
    n, o = _scene(lambda f, c, *a: L.pbf_scene_dambreak(f, c, *a, C.byref(side)), fp64, nominal)
    L.pbf_scene_dambreak(int(fp64), nominal, _vp(o["id"]), _vp(o["type"]), _vp(o["mass"]), _vp(o["pos"]),
                         _vp(o["vel"]), _vp(o["colour"]), C.byref(side))
    return o, side.value


def whitewater_config(capacity, tau_ta, tau_wc, tau_k, k_ta=0.0, k_wc=0.0, lifetime=(2.0, 5.0), k_b=2.0, k_d=0.8,
                      spray_below=6, bubble_from=20, seed=0):
    """A pbf_whitewater from keywords.  The classification thresholds, buoyancy and drag default to the paper's; the tau
    ranges depend on the scene and have no default."""
    w = Whitewater()
    w.capacity, w.seed, w.k_ta, w.k_wc = int(capacity), int(seed), float(k_ta), float(k_wc)
    for name, pair in (("tau_ta", tau_ta), ("tau_wc", tau_wc), ("tau_k", tau_k), ("lifetime", lifetime)):
        lo, hi = pair
        getattr(w, name)[:] = [float(lo), float(hi)]
    w.k_b, w.k_d, w.spray_below, w.bubble_from = float(k_b), float(k_d), int(spray_below), int(bubble_from)
    return w


# ---- host-only helpers for pbf_set_collider: analytic signed distances (float64, NEGATIVE inside the solid) and their
# evaluation on a lattice.  Union = np.minimum, complement = negation (a bowl is the negated sphere).
def sdf_sphere(centre, radius):
    """points (..., 3) -> distance to the sphere's surface, negative inside"""
    c = np.asarray(centre, np.float64).reshape(3)

    def f(x):
        d = np.asarray(x, np.float64) - c
        return np.sqrt((d * d).sum(axis=-1)) - float(radius)
    return f


def sdf_box(lo, hi):
    """points (..., 3) -> distance to the axis-aligned box [lo, hi], negative inside"""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    centre, half = (lo + hi) / 2, (hi - lo) / 2

    def f(x):
        q = np.abs(np.asarray(x, np.float64) - centre) - half
        out = np.maximum(q, 0)
        return np.sqrt((out * out).sum(axis=-1)) + np.minimum(q.max(axis=-1), 0)
    return f


def sdf_plane(normal, d):
    """points (..., 3) -> n.x - d with n = normal / |normal|: the half space n.x < d is solid"""
    n = np.asarray(normal, np.float64).reshape(3)
    n = n / np.sqrt((n * n).sum())

    def f(x):
        return np.asarray(x, np.float64) @ n - float(d)
    return f


def sdf_lattice(fn, origin, spacing, dims):
    """fn on the nodes origin + (i, j, k) * spacing, i < dims[0] ..., in float64 -> array of shape dims (C order: node
    (i, j, k) at (i * dims[1] + j) * dims[2] + k, the layout pbf_set_collider takes)"""
    o = np.asarray(origin, np.float64).reshape(3)
    ax = [o[a] + np.arange(int(dims[a]), dtype=np.float64) * float(spacing) for a in range(3)]
    x = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)
    return np.ascontiguousarray(np.asarray(fn(x), np.float64).reshape([int(v) for v in dims]))


def mesh_struct(vertices, triangles):
    """(vertices (nv, 3) float64, triangles (nt, 3) uint32) -> (Mesh, the arrays it points into: keep them alive)"""
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    return Mesh(len(v), len(t), v.ctypes.data, t.ctypes.data), (v, t)


def mesh_records(vertices, triangles, fp64=False):
    """pbf_mesh_records (host only, no GPU): the kernel's per-triangle records -> (records (nt, 30) of N, info dict).  A mesh
    that is refused raises PbfError; its .info holds the counts."""
    m, keep = mesh_struct(vertices, triangles)
    rec = np.zeros((len(keep[1]), MESH_RECORD), np.float64 if fp64 else np.float32)
    info = MeshInfo()
    rc = lib().pbf_mesh_records(C.byref(m), int(bool(fp64)), _vp(rec), C.byref(info))
    if rc < 0:
        e = PbfError(f"pbf_mesh_records failed ({rc}): {lib().pbf_last_error(None).decode()}")
        e.info = info.as_dict()
        raise e
    return rec, info.as_dict()


def mesh_soup_records(vertices, triangles, fp64=False):
    """pbf_mesh_soup_records (host only, no GPU): the records of a triangle soup for the winding-number sign -> (records (nt, 9)
    of N: a, b, c; info dict, complete: boundary, non-manifold and misoriented edges are reports here).  A mesh that is
    refused raises PbfError; its .info holds what was measured."""
    m, keep = mesh_struct(vertices, triangles)
    rec = np.zeros((len(keep[1]), MESH_SOUP_RECORD), np.float64 if fp64 else np.float32)
    info = MeshInfo()
    rc = lib().pbf_mesh_soup_records(C.byref(m), int(bool(fp64)), _vp(rec), C.byref(info))
    if rc < 0:
        e = PbfError(f"pbf_mesh_soup_records failed ({rc}): {lib().pbf_last_error(None).decode()}")
        e.info = info.as_dict()
        raise e
    return rec, info.as_dict()


def _mesh_flags(negate, winding):
    return (MESH_NEGATE if negate else 0) | (MESH_SIGN_WINDING if winding else 0)


def _lattice_struct(origin, spacing, dims, margin=0.0):
    sdf = ColliderSdf()
    sdf.dims[:] = [int(v) for v in dims]
    sdf.origin[:] = [float(v) for v in origin]
    sdf.spacing, sdf.margin, sdf.phi = float(spacing), float(margin), None
    return sdf


class Solver:
    """Mirror of sph::hip_impl::Solver<T,N> (host/hipsph.hpp) over the C ABI: ctor takes h like
    omp_impl::Solver(N h) (ompsph.hpp:83); state is device-resident between steps."""

    def __init__(self, h=0.1, fp64=False, device=0, flags=0, stream=None):
        self.L = lib()
        self.fp64 = bool(fp64)
        self.dtype = np.float64 if fp64 else np.float32
        d = Desc(ABI_VERSION, int(self.fp64), device, flags, h, stream)
        self.ctx = C.c_void_p()
        rc = self.L.pbf_create(C.byref(d), C.byref(self.ctx))
        if rc != 0:
            msg = self.L.pbf_last_error(None)
            self.ctx = None
            raise PbfError(f"pbf_create failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "ctx", None):
            self.L.pbf_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            msg = self.L.pbf_last_error(self.ctx)
            raise PbfError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        return rc

    @property
    def n(self):
        return self.L.pbf_count(self.ctx)

    def upload(self, id, type, mass, pos, vel, colour):
        n = len(id)
        a = [np.ascontiguousarray(id, np.uint64), np.ascontiguousarray(type, np.uint8),
             np.ascontiguousarray(mass, self.dtype), np.ascontiguousarray(pos, self.dtype).reshape(n, 3),
             np.ascontiguousarray(vel, self.dtype).reshape(n, 3),
             np.ascontiguousarray(colour, self.dtype).reshape(n, 4)]
        self._chk(self.L.pbf_upload(self.ctx, n, *[_vp(x) for x in a]), "pbf_upload")
        return self

    def download(self):
        n = self.n
        o = dict(id=np.empty(n, np.uint64), type=np.empty(n, np.uint8), mass=np.empty(n, self.dtype),
                 pos=np.empty((n, 3), self.dtype), vel=np.empty((n, 3), self.dtype),
                 colour=np.empty((n, 4), self.dtype))
        self._chk(self.L.pbf_download(self.ctx, _vp(o["id"]), _vp(o["type"]), _vp(o["mass"]), _vp(o["pos"]),
                                      _vp(o["vel"]), _vp(o["colour"])), "pbf_download")
        return o

    def step(self, p):
        self._chk(self.L.pbf_step(self.ctx, C.byref(p)), "pbf_step")
        return self

    def steps(self, p, count):
        self._chk(self.L.pbf_steps(self.ctx, C.byref(p), count), "pbf_steps")
        return self

    def set_option(self, name, value):
        self._chk(self.L.pbf_set_option(self.ctx, name.encode(), int(value)), "pbf_set_option")
        return self

    def set_surface_tension(self, cohesion, adhesion=0.0):
        """Opt-in surface tension (cohesion gamma) and adhesion to obstacles (beta) after Akinci et al. 2013; 0 / 0 = off.
        Persists in the solver and applies to every later step (include/pbf_hip.h)."""
        self._chk(self.L.pbf_set_surface_tension(self.ctx, float(cohesion), float(adhesion)), "pbf_set_surface_tension")
        return self

    # the collider and the scenery are given, built from a mesh and sampled alike: `which` names the entry point
    def _set_solid(self, which, phi, origin, spacing, margin):
        entry = f"pbf_set_{which}"
        if phi is None:
            self._chk(getattr(self.L, entry)(self.ctx, None), entry)
            return self
        a = np.ascontiguousarray(phi, self.dtype)
        if a.ndim != 3:
            raise ValueError(f"set_{which}: phi must have shape (nx, ny, nz)")
        sdf = _lattice_struct(origin, spacing, a.shape, margin)
        sdf.phi = a.ctypes.data
        self._chk(getattr(self.L, entry)(self.ctx, C.byref(sdf)), entry)
        return self

    def _set_solid_mesh(self, which, vertices, triangles, origin, spacing, dims, margin, negate, winding):
        entry = f"pbf_set_{which}_mesh"
        m, keep = mesh_struct(vertices, triangles)
        sdf = _lattice_struct(origin, spacing, dims, margin)
        st = MeshSdfStats()
        self._chk(getattr(self.L, entry)(self.ctx, C.byref(m), C.byref(sdf), _mesh_flags(negate, winding), C.byref(st)), entry)
        return dict(pairs_total=int(st.pairs_total), pairs_tested=int(st.pairs_tested))

    def _solid_sample(self, which, p, points):
        entry = f"pbf_{which}_sample"
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = len(pts)
        o = dict(phi=np.zeros(n, self.dtype), moved=np.zeros((n, 3), self.dtype), hit=np.zeros(n, np.uint8))
        self._chk(getattr(self.L, entry)(self.ctx, C.byref(p), n, _vp(pts), _vp(o["phi"]), _vp(o["moved"]), _vp(o["hit"])), entry)
        return o

    def set_collider(self, phi, origin=(0.0, 0.0, 0.0), spacing=1.0, margin=0.0):
        """Opt-in static collider (pbf_set_collider, include/pbf_hip.h): phi = signed distances in world units on a lattice
        of shape (nx, ny, nz), negative inside the solid (sdf_lattice makes one); origin = world position of node (0, 0, 0);
        delta-p keeps the fluid at phi >= margin.  phi=None clears it.  Persists in the solver."""
        return self._set_solid("collider", phi, origin, spacing, margin)

    def set_collider_pose(self, rot, trans=(0.0, 0.0, 0.0)):
        """A rigid pose for the installed collider (pbf_set_collider_pose, include/pbf_hip.h): the lattice is read in a body
        frame, a world point being w = rot @ b + trans.  rot: (3, 3) rotation, body -> world; rot=None returns to the static
        collider.  No upload, no synchronisation and no recapture per call; persists until it is changed."""
        if rot is None:
            self._chk(self.L.pbf_set_collider_pose(self.ctx, None), "pbf_set_collider_pose")
            return self
        pose = ColliderPose()
        pose.rot[:] = [float(v) for v in np.asarray(rot, np.float64).reshape(9)]
        pose.trans[:] = [float(v) for v in np.asarray(trans, np.float64).reshape(3)]
        self._chk(self.L.pbf_set_collider_pose(self.ctx, C.byref(pose)), "pbf_set_collider_pose")
        return self

    def set_collider_reaction(self, on=True):
        """Opt-in records of what the collider did to the fluid (pbf_set_collider_reaction): per particle through
        collider_push(), summed through collider_reaction()."""
        self._chk(self.L.pbf_set_collider_reaction(self.ctx, 1 if on else 0), "pbf_set_collider_reaction")
        return self

    def collider_reaction(self, raw=False):
        """The impulse and angular impulse the collider gave the fluid in the last step (pbf_collider_reaction) -> dict(impulse
        (3,), angular (3,), abs_impulse, abs_angular, hits, particles, step); raw: the ColliderWrench itself.  The body
        received the negatives."""
        w = ColliderWrench()
        self._chk(self.L.pbf_collider_reaction(self.ctx, C.byref(w)), "pbf_collider_reaction")
        return w if raw else w.as_dict()

    def set_collider_body(self, mass=None, inertia=(1.0, 1.0, 1.0), rot=np.eye(3), centre=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0),
                          angular_velocity=(0.0, 0.0, 0.0), gain=0.49, accel=(0.0, 0.0, 0.0), linear_damping=0.0, angular_damping=0.0,
                          linear_factor=(1.0, 1.0, 1.0), angular_factor=(1.0, 1.0, 1.0), centre_min=(-np.inf,) * 3, centre_max=(np.inf,) * 3):
        """The installed collider as a rigid body the fluid moves (pbf_set_collider_body, include/pbf_hip.h): every later step
        sums the reaction, advances the body and writes the pose of the next step on the device, pbf_steps and graph replays
        included.  rot / centre: the start pose (the body frame's origin is the centre of mass); inertia: the principal
        moments along the lattice's axes; gain 0.49 = the momentum finalise gave the fluid.  mass=None turns the body off
        (the solid stays where it is).  Calling it again re-places the body without a recapture."""
        if mass is None:
            self._chk(self.L.pbf_set_collider_body(self.ctx, None), "pbf_set_collider_body")
            return self
        self._chk(self.L.pbf_set_collider_body(self.ctx, C.byref(collider_body(
            mass, inertia, rot, centre, velocity, angular_velocity, gain, accel, linear_damping, angular_damping, linear_factor,
            angular_factor, centre_min, centre_max))), "pbf_set_collider_body")
        return self

    def collider_body_state(self, raw=False):
        """The body's state between steps (pbf_collider_body_state; it synchronises) -> dict(rot (3, 3), centre, quat (w, x, y,
        z), velocity, angular_velocity, impulse and angular — the sums the last advance consumed —, hits, steps, rejected);
        raw: the ColliderBodyState itself."""
        st = ColliderBodyState()
        self._chk(self.L.pbf_collider_body_state(self.ctx, C.byref(st)), "pbf_collider_body_state")
        return st if raw else st.as_dict()

    def set_collider_body_contact(self, level=0.0, stride=1, skin=0.0, restitution=0.0, friction=0.0, correction=0.8, slop=0.0,
                                  iterations=1, on=True):
        """Contact of the body with the scenery (pbf_set_collider_body_contact, include/pbf_hip.h): the body's surface, phi ==
        level of the collider's lattice sampled every `stride` cells, is tested against the scenery after every advance,
        `iterations` times per step, and answered with one impulse (restitution, Coulomb friction) and a shift of the centre
        (`correction` of the depth beyond `slop`) on the device.  Needs a body and scenery.  on=False turns it off.  Calling
        it again with the same level and stride rewrites the device record without a recapture."""
        if not on:
            self._chk(self.L.pbf_set_collider_body_contact(self.ctx, None), "pbf_set_collider_body_contact")
            return self
        c = BodyContact(float(level), int(stride), float(skin), float(restitution), float(friction), float(correction), float(slop),
                        int(iterations))
        self._chk(self.L.pbf_set_collider_body_contact(self.ctx, C.byref(c)), "pbf_set_collider_body_contact")
        return self

    def collider_body_contact_state(self, raw=False):
        """The contact's state between steps (pbf_collider_body_contact_state; it synchronises) -> dict(depth_sum, push (3,),
        arm (3,), depth_max — the raw sums of the last pass —, impulse, shift — what that pass applied —, points, passes,
        contacts, rejected); raw: the BodyContactState itself."""
        st = BodyContactState()
        self._chk(self.L.pbf_collider_body_contact_state(self.ctx, C.byref(st)), "pbf_collider_body_contact_state")
        return st if raw else st.as_dict()

    def collider_body_contact_points(self):
        """The body's surface points (pbf_collider_body_contact_points) -> (n, 3) of the solver's dtype, body frame, in
        cell-index order"""
        n = C.c_uint64(0)
        self._chk(self.L.pbf_collider_body_contact_points(self.ctx, C.byref(n), None), "pbf_collider_body_contact_points")
        pts = np.empty((int(n.value), 3), self.dtype)
        self._chk(self.L.pbf_collider_body_contact_points(self.ctx, C.byref(n), _vp(pts)), "pbf_collider_body_contact_points")
        return pts

    def set_collider_friction(self, mu=None, velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0)):
        """Coulomb friction against the installed collider (pbf_set_collider_friction, include/pbf_hip.h): one pass after every
        finalise drags the tangential velocity of the particles the solid pushed towards the solid's contact velocity,
        velocity + angular_velocity x (x - the pose's t) (a body's own while a body is on).  mu = inf is no-slip; mu=None turns
        it off.  Calling it again rewrites the device record without a recapture."""
        if mu is None:
            self._chk(self.L.pbf_set_collider_friction(self.ctx, None), "pbf_set_collider_friction")
            return self
        f = ColliderFriction()
        f.mu = float(mu)
        f.velocity[:] = [float(x) for x in np.asarray(velocity, np.float64).reshape(3)]
        f.angular_velocity[:] = [float(x) for x in np.asarray(angular_velocity, np.float64).reshape(3)]
        self._chk(self.L.pbf_set_collider_friction(self.ctx, C.byref(f)), "pbf_set_collider_friction")
        return self

    def collider_friction_reaction(self, raw=False):
        """The last friction pass's raw sums (pbf_collider_friction_reaction; it synchronises) -> the dict of collider_reaction():
        impulse, angular (about the pose's t; the solid received their negatives), the sums of |term|, hits = particles that
        slid, particles = particles in contact, step = passes since friction was turned on; raw: the ColliderWrench itself."""
        w = ColliderWrench()
        self._chk(self.L.pbf_collider_friction_reaction(self.ctx, C.byref(w)), "pbf_collider_friction_reaction")
        return w if raw else w.as_dict()

    def collider_push(self):
        """(n, 8): {A.xyz, hits, B.xyz, 0} per particle, the order of pstar() (PBF_BUF_COLLIDER_PUSH)"""
        a = np.empty((self.n, 8), self.dtype)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_COLLIDER_PUSH, _vp(a), a.nbytes), "read collider push records")
        return a

    def sdf_from_mesh(self, vertices, triangles, origin, spacing, dims, negate=False, winding=False):
        """pbf_sdf_from_mesh: the signed distance to a closed triangle mesh (counter-clockwise from outside) on the lattice
        origin + (i, j, k) * spacing, computed on the device -> (phi of shape dims, negative inside the mesh; negate: outside),
        dict(pairs_total, pairs_tested)).  winding: the mesh is a triangle soup signed by the winding number
        (PBF_MESH_SIGN_WINDING): open, misoriented and non-manifold meshes are accepted."""
        m, keep = mesh_struct(vertices, triangles)
        sdf = _lattice_struct(origin, spacing, dims)
        phi = np.zeros([int(v) for v in dims], self.dtype)
        st = MeshSdfStats()
        self._chk(self.L.pbf_sdf_from_mesh(self.ctx, C.byref(m), C.byref(sdf), _mesh_flags(negate, winding), _vp(phi), C.byref(st)),
                  "pbf_sdf_from_mesh")
        return phi, dict(pairs_total=int(st.pairs_total), pairs_tested=int(st.pairs_tested))

    def set_collider_mesh(self, vertices, triangles, origin, spacing, dims, margin=0.0, negate=False, winding=False):
        """pbf_set_collider_mesh: the lattice of sdf_from_mesh computed and installed as the collider without leaving the
        device -> dict(pairs_total, pairs_tested)"""
        return self._set_solid_mesh("collider", vertices, triangles, origin, spacing, dims, margin, negate, winding)

    def mesh_winding(self, vertices, triangles, origin, spacing, dims):
        """pbf_mesh_winding: the generalised winding number of a triangle soup at the lattice's nodes, computed on the device ->
        w of shape dims: 1 inside a closed outward mesh, 0 outside, the covered share of the sphere of directions for an open
        one (the solid of sdf_from_mesh(winding=True) is where w > 1/2)"""
        m, keep = mesh_struct(vertices, triangles)
        sdf = _lattice_struct(origin, spacing, dims)
        w = np.zeros([int(v) for v in dims], self.dtype)
        self._chk(self.L.pbf_mesh_winding(self.ctx, C.byref(m), C.byref(sdf), _vp(w)), "pbf_mesh_winding")
        return w

    def collider_sample(self, p, points):
        """The collider's device function at world points (pbf_collider_sample) -> dict(phi (n,) interpolated distance, +inf
        outside the lattice; moved (n,3) the solver-frame position delta-p would store; hit (n,) uint8)"""
        return self._solid_sample("collider", p, points)

    def set_scenery(self, phi, origin=(0.0, 0.0, 0.0), spacing=1.0, margin=0.0):
        """Opt-in scenery (pbf_set_scenery, include/pbf_hip.h): a second, static lattice in the world frame beside the collider,
        given as set_collider's is; delta-p projects the fluid out of it after the collider.  It never has a pose, a body,
        friction or a reaction; with a collider installed as well the reaction records are on.  phi=None clears it."""
        return self._set_solid("scenery", phi, origin, spacing, margin)

    def set_scenery_mesh(self, vertices, triangles, origin, spacing, dims, margin=0.0, negate=False, winding=False):
        """pbf_set_scenery_mesh: set_collider_mesh's build, installed as the scenery -> dict(pairs_total, pairs_tested)"""
        return self._set_solid_mesh("scenery", vertices, triangles, origin, spacing, dims, margin, negate, winding)

    def scenery_sample(self, points, params):
        """The static device function on the scenery's lattice at world points (pbf_scenery_sample) -> the dict of
        collider_sample()"""
        return self._solid_sample("scenery", params, points)

    def surface_state(self):
        """(n,4): {n.xyz, rho} of the last surface-tension pass — surface normal and density per particle, device order
        (zero for obstacles)"""
        a = np.empty((self.n, 4), self.dtype)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_SURFACE, _vp(a), a.nbytes), "read surface state")
        return a

    def diagnostics(self, p=None, density=False, raw=False):
        """Conserved sums, extrema and — `density`, which needs the params of the last step — the density residual of the
        resident state, computed and reduced on the device (pbf_diagnostics, include/pbf_hip.h) -> dict of the fields of
        pbf_diag (3-vectors as float64 arrays); raw: the Diag structure itself."""
        d = Diag()
        what = DIAG_DENSITY if density else 0
        self._chk(self.L.pbf_diagnostics(self.ctx, None if p is None else C.byref(p), what, C.byref(d)), "pbf_diagnostics")
        return d if raw else d.as_dict()

    def density(self):
        """(n,): rho_i of the last diagnostics(p, density=True), device order (zero for obstacles)"""
        a = np.empty(self.n, self.dtype)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_DENSITY, _vp(a), a.nbytes), "read density")
        return a

    def reserve(self, capacity):
        """Particle capacity for what sources emit (and, in slab mode, migrants and copies); before upload()."""
        self._chk(self.L.pbf_reserve(self.ctx, int(capacity)), "pbf_reserve")
        return self

    def set_sources(self, sources):
        """sources: list of (tag, centre3, velocity3, colour4, rate) (sph::Source); [] clears.  Emitted on the device at
        the top of every later step (include/pbf_hip.h)."""
        arr = (Source * max(len(sources), 1))()
        for a, (tag, centre, velocity, colour, rate) in zip(arr, sources):
            a.tag, a.rate = int(tag), float(rate)
            a.centre[:], a.velocity[:], a.colour[:] = [float(v) for v in centre], [float(v) for v in velocity], [float(v) for v in colour]
        self._chk(self.L.pbf_set_sources(self.ctx, len(sources), C.byref(arr) if sources else None), "pbf_set_sources")
        return self

    def set_drains(self, drains):
        """drains: list of (centre3, width) (sph::Drain); [] clears.  Applied on the device after the sources."""
        arr = (Drain * max(len(drains), 1))()
        for a, (centre, width) in zip(arr, drains):
            a.centre[:], a.width = [float(v) for v in centre], float(width)
        self._chk(self.L.pbf_set_drains(self.ctx, len(drains), C.byref(arr) if drains else None), "pbf_set_drains")
        return self

    def scene_host_syncs(self):
        """host read-backs made for drains so far (at most one per step)"""
        return int(self.L.pbf_scene_host_syncs(self.ctx))

    def query(self, p, points, cap=4096):
        """ids of the fluid particles in the cell of each world point, on the last step's table (ompsph.hpp:167-186) ->
        list of uint64 arrays (the first `cap` ids of a cell); last_query_counts keeps the full counts"""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        counts = np.zeros(len(pts), np.uint32)
        ids = np.zeros((len(pts), max(cap, 1)), np.uint64)
        self._chk(self.L.pbf_query_cells(self.ctx, C.byref(p), len(pts), _vp(pts), _vp(counts), _vp(ids), cap),
                  "pbf_query_cells")
        self.last_query_counts = counts
        return [ids[i, :min(int(counts[i]), cap)].copy() for i in range(len(pts))]

    def _sample_arrays(self, n, velocity, colour):
        a = dict(rho=np.zeros(n, self.dtype), weight=np.zeros(n, self.dtype), count=np.zeros((n, 2), np.uint32),
                 outside=np.zeros(n, np.uint8))
        if velocity:
            a["mv"] = np.zeros((n, 3), self.dtype)
        if colour:
            a["mc"] = np.zeros((n, 4), self.dtype)
        out = SampleOut(_vp(a["rho"]), _vp(a["weight"]), _vp(a.get("mv")), _vp(a.get("mc")), _vp(a["count"]), _vp(a["outside"]))
        return a, out, (SAMPLE_VELOCITY if velocity else 0) | (SAMPLE_COLOUR if colour else 0)

    @staticmethod
    def _sample_normalised(a):
        # the caller's division (include/pbf_hip.h): mv / weight, mc / weight, 0 where weight == 0
        w = a["weight"][:, None]
        safe = np.where(w == 0, 1, w)
        for raw, name in (("mv", "velocity"), ("mc", "colour")):
            if raw in a:
                a[name] = np.where(w == 0, 0, a[raw] / safe).astype(a[raw].dtype)
        return a

    def sample(self, p, points, velocity=False, colour=False):
        """The SPH sums at world points (pbf_sample_points, include/pbf_hip.h) -> dict of numpy arrays: the raw sums rho,
        weight, mv (n,3), mc (n,4), count (n,2) {fluid, obstacle}, outside, plus velocity = mv / weight and colour =
        mc / weight (0 where weight == 0) when asked for."""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        a, out, what = self._sample_arrays(len(pts), velocity, colour)
        self._chk(self.L.pbf_sample_points(self.ctx, C.byref(p), len(pts), _vp(pts), what, C.byref(out)), "pbf_sample_points")
        return self._sample_normalised(a)

    def sample_lattice(self, p, origin, spacing, dims, velocity=False, colour=False):
        """The same sums on the lattice origin + (i, j, k) * spacing, i < dims[0] ... (pbf_sample_lattice); point (i, j, k)
        has index (i * dims[1] + j) * dims[2] + k."""
        o, sp = np.ascontiguousarray(origin, np.float64).reshape(3), np.ascontiguousarray(spacing, np.float64).reshape(3)
        d = np.ascontiguousarray(dims, np.uint64).reshape(3)
        n = int(d[0]) * int(d[1]) * int(d[2])
        a, out, what = self._sample_arrays(n if n < 2 ** 31 else 0, velocity, colour)
        self._chk(self.L.pbf_sample_lattice(self.ctx, C.byref(p), _vp(o), _vp(sp), _vp(d), what, C.byref(out)), "pbf_sample_lattice")
        return self._sample_normalised(a)

    def anisotropy(self, p, smoothing=0.9, k_r=4.0, k_s=20.0 / 3.0, k_n=0.5, min_neighbours=25, only=None):
        """Smoothed centres and anisotropy matrices after Yu & Turk 2013 on the state the last step left
        (pbf_anisotropy_compute, include/pbf_hip.h) -> dict of arrays in device order: centre (n,3) world, G (n,6)
        {xx yy zz xy xz yz} in the solver frame, axes (n,3,3) unit rows in descending order, radii (n,3), neighbours (n,).
        The library's arrays are component-major; these are transposed views of them.  only: names to ask for (the other
        pointers are NULL)."""
        n = self.n
        planes = dict(centre=3, G=6, axes=9, radii=3)
        names = list(planes) + ["neighbours"] if only is None else list(only)
        raw = {k: np.zeros((planes[k], n), self.dtype) if k in planes else np.zeros(n, np.uint32) for k in names}
        cfg = Anisotropy(float(smoothing), float(k_r), float(k_s), float(k_n), int(min_neighbours))
        out = AnisotropyOut(*[_vp(raw.get(k)) for k in ("centre", "G", "axes", "radii", "neighbours")])
        self._chk(self.L.pbf_anisotropy_compute(self.ctx, C.byref(p), C.byref(cfg), C.byref(out)), "pbf_anisotropy_compute")
        o = {k: (v.T if k in planes else v) for k, v in raw.items()}
        if "axes" in o:
            o["axes"] = o["axes"].reshape(n, 3, 3)
        return o

    def whitewater_configure(self, **cfg):
        """Configure the pool of diffuse particles (pbf_whitewater_configure, include/pbf_hip.h).  Keywords = the fields of
        pbf_whitewater; the tau ranges have no defaults (tools/whitewater_probe.py prints a scene's percentiles to pick
        them from).  capacity=0 frees the pool."""
        w = whitewater_config(**cfg)
        self._chk(self.L.pbf_whitewater_configure(self.ctx, C.byref(w)), "pbf_whitewater_configure")
        return self

    def whitewater_upload(self, pos, vel=None, life=None):
        """Replace the pool's content (restart, tests): pos (n,3) world; vel None = at rest; life None = lifetime[1]."""
        pos = np.ascontiguousarray(pos, self.dtype).reshape(-1, 3)
        n = len(pos)
        vel = None if vel is None else np.ascontiguousarray(vel, self.dtype).reshape(n, 3)
        life = None if life is None else np.ascontiguousarray(life, self.dtype).reshape(n)
        self._chk(self.L.pbf_whitewater_upload(self.ctx, n, _vp(pos), _vp(vel), _vp(life)), "pbf_whitewater_upload")
        return self

    def whitewater_step(self, p):
        """One whitewater step on the state the last step left -> dict(alive, emitted, dropped, died, kind=[spray, foam,
        bubble])"""
        st = WhitewaterStats()
        self._chk(self.L.pbf_whitewater_step(self.ctx, C.byref(p), C.byref(st)), "pbf_whitewater_step")
        return dict(alive=int(st.alive), emitted=int(st.emitted), dropped=int(st.dropped), died=int(st.died),
                    kind=[int(k) for k in st.kind])

    @property
    def whitewater_count(self):
        return self.L.pbf_whitewater_count(self.ctx)

    def whitewater_download(self):
        """The pool -> dict(pos (n,3), vel (n,3), life (n,), kind (n,) uint8, parent_id (n,) uint64)"""
        n = self.whitewater_count
        o = dict(pos=np.empty((n, 3), self.dtype), vel=np.empty((n, 3), self.dtype), life=np.empty(n, self.dtype),
                 kind=np.empty(n, np.uint8), parent_id=np.empty(n, np.uint64))
        self._chk(self.L.pbf_whitewater_download(self.ctx, _vp(o["pos"]), _vp(o["vel"]), _vp(o["life"]), _vp(o["kind"]),
                                                 _vp(o["parent_id"])), "pbf_whitewater_download")
        return o

    def set_whitewater_solids(self, restitution=0.0, friction=0.0, absorb=False, off=False, reserved=0):
        """Diffuse particles collide with the collider and the scenery from the next whitewater step on
        (pbf_set_whitewater_solids, include/pbf_hip.h).  restitution=None or off=True turns the setting off."""
        if off or restitution is None:
            self._chk(self.L.pbf_set_whitewater_solids(self.ctx, None), "pbf_set_whitewater_solids")
            return self
        cfg = WhitewaterSolids(float(restitution), float(friction), 1 if absorb else 0, int(reserved))
        self._chk(self.L.pbf_set_whitewater_solids(self.ctx, C.byref(cfg)), "pbf_set_whitewater_solids")
        return self

    def whitewater_solids_stats(self):
        """The counts of the last whitewater step -> dict(hit_collider, hit_scenery, absorbed, born_inside, step)"""
        st = WhitewaterSolidsStats()
        self._chk(self.L.pbf_whitewater_solids_stats(self.ctx, C.byref(st)), "pbf_whitewater_solids_stats")
        return {k: int(getattr(st, k)) for k, _ in WhitewaterSolidsStats._fields_}

    def whitewater_potentials(self):
        """(n,4): {I_ta, I_wc, E_k, n_d} of the last whitewater step, device order (zero for obstacles)"""
        a = np.empty((self.n, 4), self.dtype)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_WHITEWATER, _vp(a), a.nbytes), "read whitewater potentials")
        return a

    def sync(self):
        self._chk(self.L.pbf_sync(self.ctx), "pbf_sync")
        return self

    def graph_stats(self):
        """(graphs captured, graph replays, graphs still enabled) of pbf_steps' hipGraph path"""
        o = np.zeros(3, np.uint64)
        self._chk(self.L.pbf_graph_stats(self.ctx, _vp(o)), "pbf_graph_stats")
        return int(o[0]), int(o[1]), bool(o[2])

    def stage(self, name, p):
        self._chk(getattr(self.L, "pbf_stage_" + name)(self.ctx, C.byref(p)), "pbf_stage_" + name)
        return self

    def nbr_counts(self):
        """Neighbour-list length per particle of the last list build (0xFFFFFFFF: overflowed row)."""
        k = np.empty(self.n, np.uint32)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_NBR_COUNT, _vp(k), k.nbytes), "read neighbour counts")
        # raw word = length | chunk << 8 (the chunk of the list's slots beyond the 40 in the rows), or 0xFFFFFFFF
        return np.where(k == 0xFFFFFFFF, k, k & 0xFF).astype(np.uint32)

    def keys(self):
        k = np.empty(self.n, np.uint32)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_KEYS, _vp(k), k.nbytes), "read keys")
        return k

    def table(self):
        t = np.empty(self.L.pbf_table_size(self.ctx), np.uint32)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_TABLE, _vp(t), t.nbytes), "read table")
        return t

    def pstar(self):
        """(n,4): pStar.xyz, lambda"""
        a = np.empty((self.n, 4), self.dtype)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_PSTAR, _vp(a), a.nbytes), "read pstar")
        return a

    def omega(self):
        """(n,3): vorticity estimate of the last step run with p.vorticity (opt-in extra), device order"""
        a = np.empty((self.n, 4), self.dtype)
        self._chk(self.L.pbf_read_buffer(self.ctx, BUF_OMEGA, _vp(a), a.nbytes), "read omega")
        return a[:, :3].copy()

    def _read_lattice(self):
        smp = np.zeros(3, np.uint64)
        self._chk(self.L.pbf_read_lattice(self.ctx, _vp(smp), None, None), "pbf_read_lattice")
        nn = int(smp.prod())
        pn, cc = np.empty((nn, 4), self.dtype), np.empty((nn, 4), self.dtype)
        self._chk(self.L.pbf_read_lattice(self.ctx, _vp(smp), _vp(pn), _vp(cc)), "pbf_read_lattice")
        return dict(sample=smp, pn=pn, c=cc)

    def _read_soup(self, n):
        vs, ns, cs = np.empty((3 * n, 3), self.dtype), np.empty((3 * n, 3), self.dtype), np.empty((3 * n, 4), self.dtype)
        self._chk(self.L.pbf_download_mesh(self.ctx, _vp(vs), _vp(ns), _vp(cs)), "pbf_download_mesh")
        return dict(vs=vs, ns=ns, cs=cs, **self._read_lattice())

    def _read_indexed(self, v, t):
        vs, ns, cs = np.empty((v, 3), self.dtype), np.empty((v, 3), self.dtype), np.empty((v, 4), self.dtype)
        tris = np.empty((t, 3), np.uint32)
        self._chk(self.L.pbf_download_mesh_indexed(self.ctx, _vp(vs), _vp(ns), _vp(cs), _vp(tris)), "pbf_download_mesh_indexed")
        return dict(vs=vs, ns=ns, cs=cs, tris=tris, **self._read_lattice())

    def surface(self, p, mc=None):
        """Marching cubes on the state the last step left -> dict(vs, ns, cs, sample, pn, c)."""
        mc = mc or McParams()
        nt = C.c_uint64()
        self._chk(self.L.pbf_surface(self.ctx, C.byref(p), C.byref(mc), C.byref(nt)), "pbf_surface")
        return self._read_soup(nt.value)

    def surface_indexed(self, p, mc=None):
        """The same surface as an indexed mesh: one vertex per crossed lattice edge -> dict(vs (V,3), ns (V,3), cs (V,4),
        tris (T,3) uint32, sample, pn, c).  vs[tris] is surface()'s soup (include/pbf_hip.h)."""
        mc = mc or McParams()
        nv, nt = C.c_uint64(), C.c_uint64()
        self._chk(self.L.pbf_surface_indexed(self.ctx, C.byref(p), C.byref(mc), C.byref(nv), C.byref(nt)), "pbf_surface_indexed")
        return self._read_indexed(nv.value, nt.value)

    def surface_anisotropic(self, p, resolution, isolevel, indexed=False, **kernel):
        """The iso-surface of Yu & Turk's anisotropic-kernel field over the ellipsoids of anisotropy() (pbf_surface_anisotropic,
        include/pbf_hip.h) -> the dict of surface(), or with indexed=True that of surface_indexed().  kernel: anisotropy()'s
        smoothing, k_r, k_s, k_n, min_neighbours.  The isolevel has no default: the field's scale is not the stock one's."""
        k = dict(smoothing=0.9, k_r=4.0, k_s=20.0 / 3.0, k_n=0.5, min_neighbours=25)
        unknown = set(kernel) - set(k)
        if unknown:
            raise TypeError(f"surface_anisotropic: unknown kernel argument(s) {sorted(unknown)}")
        k.update(kernel)
        cfg = AnisoSurface(float(resolution), float(isolevel),
                           Anisotropy(float(k["smoothing"]), float(k["k_r"]), float(k["k_s"]), float(k["k_n"]), int(k["min_neighbours"])))
        nv, nt = C.c_uint64(), C.c_uint64()
        self._chk(self.L.pbf_surface_anisotropic(self.ctx, C.byref(p), C.byref(cfg), 1 if indexed else 0, C.byref(nv), C.byref(nt)),
                  "pbf_surface_anisotropic")
        return self._read_indexed(nv.value, nt.value) if indexed else self._read_soup(nt.value)

    def extent(self):
        e = np.zeros(3, np.uint64)
        m = np.zeros(3, np.float64)
        self._chk(self.L.pbf_grid_extent(self.ctx, _vp(e), _vp(m)), "grid_extent")
        return e, m

    def selftest_divides(self, numerators=8):
        """pbf_selftest_divides -> (mismatches[8], visited[8]) (include/pbf_hip.h names the categories)."""
        bad, seen = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
        self._chk(self.L.pbf_selftest_divides(self.ctx, int(numerators), _vp(bad), _vp(seen)), "pbf_selftest_divides")
        return bad, seen

    def stage_times(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        calls = (C.c_uint64 * 16)()
        k = self._chk(self.L.pbf_stage_times(self.ctx, names, ms, calls, 16), "pbf_stage_times")
        return {names[i].decode(): (ms[i], calls[i]) for i in range(k)}

    def reset_stage_times(self):
        self._chk(self.L.pbf_reset_stage_times(self.ctx), "pbf_reset_stage_times")

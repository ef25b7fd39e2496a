"""ctypes binding of oracle/liboracle.so (the fp64 CPU restatement in rpt_oracle.cpp) and the
lowering of an `rpt_amd.api.Scene` description onto it.  TEST INFRASTRUCTURE: see the header of
rpt_oracle.cpp for who may use it and for the parity status ("parity unpinned" apart from the
colour KAT of src/color.rs:30-38)."""
import ctypes as C
import os
import subprocess

import numpy as np

from rpt_amd._lib import vp as _vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboracle.so")


class ShapeDesc(C.Structure):
    pass


ShapeDesc._fields_ = [("kind", C.c_int32), ("has_transform", C.c_int32), ("transform", C.c_double * 16),
                      ("plane_normal", C.c_double * 3), ("plane_value", C.c_double),
                      ("tris", C.POINTER(C.c_double)), ("n_tris", C.c_uint64),
                      ("children", C.POINTER(ShapeDesc)), ("n_children", C.c_uint64)]


class MaterialDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("albedo", C.c_double * 3), ("emittance", C.c_double),
                ("shininess", C.c_double), ("ior", C.c_double)]


class CameraDesc(C.Structure):
    _fields_ = [("eye", C.c_double * 3), ("direction", C.c_double * 3), ("up", C.c_double * 3), ("fov", C.c_double),
                ("aperture", C.c_double), ("focal_distance", C.c_double)]


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("exposure_value", C.c_double),
                ("max_bounces", C.c_uint32), ("robust", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "obj_tests", "nodes", "tri_tests", "hits", "samples", "vertices",
                                           "self_hits", "shadow_tests", "shadow_pass", "shadow_near")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def build(force=False):
    src = os.path.join(_HERE, "rpt_oracle.cpp")
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-B" if force else "-s", "liboracle.so"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        P, D = C.c_void_p, C.POINTER(C.c_double)
        L.orc_scene_new.restype = P
        L.orc_scene_free.argtypes = [P]
        L.orc_add_object.argtypes = [P, C.POINTER(ShapeDesc), C.POINTER(MaterialDesc)]
        L.orc_add_light.argtypes = [P, C.c_int, D, D, C.POINTER(ShapeDesc), C.POINTER(MaterialDesc), C.c_int]
        L.orc_add_medium.argtypes = [P, C.c_int, C.c_double, C.c_double]
        L.orc_set_environment.argtypes = [P, D]
        L.orc_set_environment_hdri.argtypes = [P, C.c_uint32, C.c_uint32, D]
        L.orc_render.argtypes = [P, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint64, C.c_uint32, P,
                                 C.c_int, C.POINTER(Counters), P, C.c_uint64]
        L.orc_intersect.argtypes = [P, C.c_uint64, P, P, C.c_int, P, P, P]
        L.orc_render_paths.restype = C.c_uint64
        L.orc_render_paths.argtypes = [P, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint64, C.c_uint32, P, C.c_int, P, P, C.c_uint64]
        L.orc_shape_intersect.argtypes = [C.POINTER(ShapeDesc), D, D, C.c_double, C.c_double, D, D, C.c_int]
        L.orc_mesh_kd_vs_brute.argtypes = [C.POINTER(ShapeDesc), C.c_uint64, P, P, P]
        L.orc_mesh_kd_vs_brute.restype = C.c_int64
        L.orc_shape_sample.argtypes = [C.POINTER(ShapeDesc), D, C.c_uint64, C.c_uint32, C.c_uint32, D, D, D]
        L.orc_hex_color.argtypes = [C.c_uint32, D]
        L.orc_color_bytes.argtypes = [D, C.POINTER(C.c_uint8)]
        L.orc_rng_u32.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, P]
        L.orc_rng_uniform.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, P]
        L.orc_material_sample_f.argtypes = [C.POINTER(MaterialDesc), D, D, C.c_uint64, C.c_uint32, C.c_uint32, D, D,
                                            C.POINTER(C.c_int)]
        L.orc_material_bsdf.argtypes = [C.POINTER(MaterialDesc), D, D, D, D]
        L.orc_material_sample.argtypes = [C.POINTER(MaterialDesc), C.c_uint64, P, P, C.c_uint64, P, P, P, P, P]
        L.orc_material_bsdf_n.argtypes = [C.POINTER(MaterialDesc), C.c_uint64, P, P, P, P]
        L.orc_camera_rays.argtypes = [C.POINTER(CameraDesc), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, P, P, P]
        L.orc_bounce.argtypes = [C.POINTER(MaterialDesc), C.c_int, C.c_double, C.c_double, C.c_int, D, C.c_uint32, C.c_uint32,
                                 C.c_uint64, P, P, C.c_uint64, P, P, P, P]
        L.orc_medium_sample_d.argtypes = [C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, D, D, D]
        L.orc_medium_sample_ph.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, D, D]
        L.orc_camera_cast_ray.argtypes = [C.POINTER(CameraDesc), C.c_double, C.c_double, C.c_uint64, C.c_uint32,
                                          C.c_uint32, D, D]
        L.orc_pixel_ndc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, D, D]
        L.orc_light_illuminate.argtypes = [P, C.c_int, D, C.c_uint64, C.c_uint32, C.c_uint32, D, D, D]
        L.orc_light_sample.argtypes = [P, C.c_int, C.c_uint64, P, C.c_uint64, P, P, P, P, P, P, P]
        L.orc_env_color.argtypes = [P, C.c_uint64, P, P]
        L.orc_photon_map_build.restype = P
        L.orc_photon_map_build.argtypes = [P, C.c_uint64, C.c_int, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
        L.orc_photon_map_from_photons.restype = P
        L.orc_photon_map_from_photons.argtypes = [C.c_uint64, C.c_int, C.c_double, C.c_uint64, C.c_uint64, P, C.c_uint64, P, C.c_uint64]
        L.orc_photon_map_free.argtypes = [P]
        L.orc_photon_chains.restype = P
        L.orc_photon_chains.argtypes = [P, C.c_uint64, C.c_uint64, C.c_uint64, P, C.c_int, C.c_double, C.c_uint64, C.c_int, C.c_double,
                                        C.c_uint64, C.c_int]
        L.orc_photon_chains_free.argtypes = [P]
        L.orc_photon_chains_totals.argtypes = [P, P]
        L.orc_photon_chains_get.argtypes = [P, P, P, P, P, P, P, P]
        L.orc_photon_map_get.restype = C.c_uint64
        L.orc_photon_map_get.argtypes = [P, C.c_int, P]
        L.orc_photon_render.argtypes = [P, P, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint64,
                                        C.c_uint32, P, C.c_int, P, C.c_uint64]
        _lib = L
    return _lib


def _d3(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _mat(material):
    from rpt_amd.api import material_desc
    return material_desc(material, MaterialDesc)


def material_sample(material, normals, wos, seed=0):
    """Material::sample_f, case i on Rng(seed, i, 0), and Material::bsdf at the sampled direction -> dict of some (n, int32),
    wi (n, 3), pdf (n), f (n, 3), next_word (n, uint32: the stream's next word after sample_f)."""
    nrm = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    wo = np.ascontiguousarray(wos, dtype=np.float64).reshape(-1, 3)
    n = nrm.shape[0]
    assert wo.shape[0] == n
    out = {"some": np.empty(n, np.int32), "wi": np.empty((n, 3)), "pdf": np.empty(n), "f": np.empty((n, 3)),
           "next_word": np.empty(n, np.uint32)}
    lib().orc_material_sample(C.byref(_mat(material)), n, _vp(nrm), _vp(wo), C.c_uint64(seed),
                              *[_vp(out[k]) for k in ("some", "wi", "pdf", "f", "next_word")])
    return out


def material_bsdf(material, normals, wos, wis):
    """Material::bsdf over n cases -> (n, 3)."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in (normals, wos, wis)]
    n = arrs[0].shape[0]
    assert all(a.shape[0] == n for a in arrs)
    f = np.empty((n, 3))
    lib().orc_material_bsdf_n(C.byref(_mat(material)), n, *[_vp(a) for a in arrs], _vp(f))
    return f


def bounce(material, normals, rds, max_bounces=3, depth=0, seed=0, medium=None, medium_event=False, position=(0.0, 0.0, 0.0)):
    """The continuation of a path vertex as Renderer::trace_ray performs it, case i on Rng(seed, i, 0): at a surface of `material`
    with normal normals[i] reached along rds[i], or (medium_event) at `position` inside `medium` (an rpt_amd Medium; None: a scene
    without one) -> dict of cont (n, int32), wi, k (n, 3), next_word (n, uint32)."""
    nrm = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    rd = np.ascontiguousarray(rds, dtype=np.float64).reshape(-1, 3)
    n = nrm.shape[0]
    assert rd.shape[0] == n
    out = {"cont": np.empty(n, np.int32), "wi": np.empty((n, 3)), "k": np.empty((n, 3)), "next_word": np.empty(n, np.uint32)}
    kind, a, s = (-1, 0.0, 0.0) if medium is None else (medium.kind, medium.absorption, medium.scattering)
    rc = lib().orc_bounce(C.byref(_mat(material)), kind, a, s, int(bool(medium_event)), _d3(position), max_bounces, depth, n,
                          _vp(nrm), _vp(rd), C.c_uint64(seed), *[_vp(out[k]) for k in ("cont", "wi", "k", "next_word")])
    if rc != 0:
        raise ValueError("a medium event needs a medium")
    return out


def camera_rays(camera, width, height, sample=0, seed=0):
    """The camera sample of get_color for every pixel of a width x height frame, pixel y * width + x on Rng(seed, pixel, sample)
    -> dict of o, d (n, 3), next_word (n, uint32: the stream's next word after cast_ray)."""
    from rpt_amd.api import camera_desc
    n = width * height
    out = {"o": np.empty((n, 3)), "d": np.empty((n, 3)), "next_word": np.empty(n, np.uint32)}
    lib().orc_camera_rays(C.byref(camera_desc(camera, CameraDesc)), width, height, C.c_uint64(seed), sample,
                          *[_vp(out[k]) for k in ("o", "d", "next_word")])
    return out


def _same_shape(a, b):
    """Geometry identity, as the product's flattener defines a light's twin object."""
    from rpt_amd.api import KdTree, Mesh, Plane
    ba, bb = a.base(), b.base()
    if type(ba) is not type(bb):
        return False
    ma, mb = a.matrix(), b.matrix()
    if (ma is None) != (mb is None) or (ma is not None and not np.array_equal(ma, mb)):
        return False
    if isinstance(ba, Plane):
        return np.array_equal(ba.normal, bb.normal) and ba.value == bb.value
    if isinstance(ba, Mesh):
        return ba.tris.shape == bb.tris.shape and np.array_equal(ba.tris, bb.tris)
    if isinstance(ba, KdTree):
        return len(ba.shapes) == len(bb.shapes) and all(_same_shape(x, y) for x, y in zip(ba.shapes, bb.shapes))
    return True


class OracleScene:
    """An `rpt_amd.api.Scene` lowered onto the oracle."""

    def __init__(self, scene):
        from rpt_amd.api import Light, material_desc, shape_desc
        L = lib()
        self.h = L.orc_scene_new()
        self._keep = []
        for o in scene.objects:
            sd, keep = shape_desc(o.shape, ShapeDesc)
            self._keep.append(keep)
            assert L.orc_add_object(self.h, C.byref(sd), C.byref(material_desc(o.material_, MaterialDesc))) >= 0
        for l in scene.lights:
            if l.kind == Light.OBJECT:
                sd, keep = shape_desc(l.object.shape, ShapeDesc)
                twin = -1
                for j, o in enumerate(scene.objects):
                    if _same_shape(l.object.shape, o.shape):
                        twin = j
                        break
                rc = L.orc_add_light(self.h, l.kind, None, None, C.byref(sd),
                                     C.byref(material_desc(l.object.material_, MaterialDesc)), twin)
                if rc != 0:
                    raise ValueError("light object cannot be sampled (Plane::sample is unimplemented in rpt)")
            else:
                L.orc_add_light(self.h, l.kind, _d3(l.color), _d3(l.vec if l.vec is not None else np.zeros(3)), None,
                                None, -1)
        self.n_lights = len(scene.lights)
        for m in scene.media:
            L.orc_add_medium(self.h, m.kind, m.absorption, m.scattering)
        if getattr(scene.environment, "hdri", None) is not None:
            hd = scene.environment.hdri
            L.orc_set_environment_hdri(self.h, hd.shape[1], hd.shape[0], _d3(hd))
        else:
            L.orc_set_environment(self.h, _d3(scene.environment.color))

    def render(self, camera, width, height, iterations, max_bounces, seed=0, sample_offset=0, exposure_value=0.0,
               robust=0, threads=None, counters=False, pixels=None):
        """Renderer::sample restated: -> (h*w, 3) fp64 means [, counters dict]."""
        from rpt_amd.api import camera_desc
        L = lib()
        p = Params(width, height, exposure_value, max_bounces, robust)
        out = np.zeros((width * height, 3), dtype=np.float64)
        cnt = Counters()
        if threads is None:
            threads = os.cpu_count() or 1
        pl, npix = None, 0
        if pixels is not None:
            pl = np.ascontiguousarray(pixels, dtype=np.uint32)
            npix = pl.size
        L.orc_render(self.h, C.byref(camera_desc(camera, CameraDesc)), C.byref(p), iterations, C.c_uint64(seed),
                     sample_offset, out.ctypes.data_as(C.c_void_p), threads, C.byref(cnt) if counters else None,
                     pl.ctypes.data_as(C.c_void_p) if pl is not None else None, npix)
        return (out, cnt.as_dict()) if counters else out

    PATH_LEVELS = 16
    PATH_END = ("miss", "roulette or max_bounces", "no sample")
    PATH_MEDIUM_EVENT, PATH_FAR_MISS, PATH_OVERFLOW = 1, 2, 4
    PATH_DTYPE = np.dtype([("sig", np.uint64), ("clamp", np.uint64), ("depth", np.uint32), ("end", np.uint32), ("flags", np.uint32),
                           ("levels", np.uint32), ("d", np.float64, (16, 3)), ("k", np.float64, (16, 3))])

    def render_paths(self, camera, width, height, max_bounces, seed=0, sample_offset=0, exposure_value=0.0, robust=0, threads=None):
        """render(iterations=1) with what happened on each path (PathRecord in rpt_oracle.cpp) -> (h*w, 3) radiance of the streams
        (seed, pixel, sample_offset), a structured array of PATH_DTYPE per pixel, and per light the number of vertices at which its
        shadow test passed."""
        from rpt_amd.api import camera_desc
        p = Params(width, height, exposure_value, max_bounces, robust)
        n = width * height
        out = np.zeros((n, 3), dtype=np.float64)
        rec = np.zeros(n, dtype=self.PATH_DTYPE)
        lights = np.zeros(max(self.n_lights, 1), dtype=np.uint64)
        if threads is None:
            threads = os.cpu_count() or 1
        size = lib().orc_render_paths(self.h, C.byref(camera_desc(camera, CameraDesc)), C.byref(p), C.c_uint64(seed), sample_offset,
                                      _vp(out), threads, _vp(rec), _vp(lights), self.n_lights)
        assert size == self.PATH_DTYPE.itemsize
        return out, rec, lights[:self.n_lights]

    def intersect(self, origins, dirs, robust=0):
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        t = np.empty(n)
        obj = np.empty(n, dtype=np.int32)
        nrm = np.empty((n, 3))
        lib().orc_intersect(self.h, n, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), robust,
                            t.ctypes.data_as(C.c_void_p), obj.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p))
        return t, obj, nrm

    def light_sample(self, light_index, positions, seed=0):
        """Shape::sample and Light::illuminate of one Light::Object at n positions, case i on Rng(seed, i, 0):
        -> dict of v, nrm (n, 3), p (n), intensity, wi (n, 3), dist (n), next_word (n, uint32: the stream's next word
        after illuminate)."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        n = pos.shape[0]
        out = {"v": np.empty((n, 3)), "nrm": np.empty((n, 3)), "p": np.empty(n), "intensity": np.empty((n, 3)),
               "wi": np.empty((n, 3)), "dist": np.empty(n), "next_word": np.empty(n, dtype=np.uint32)}
        rc = lib().orc_light_sample(self.h, light_index, n, pos.ctypes.data_as(C.c_void_p), C.c_uint64(seed),
                                    *[out[k].ctypes.data_as(C.c_void_p) for k in ("v", "nrm", "p", "intensity", "wi", "dist", "next_word")])
        if rc != 0:
            raise ValueError(f"light {light_index} is not a Light::Object that can be sampled")
        return out

    def env_color(self, dirs):
        """Environment::get_color of n directions (any length) -> (n, 3)."""
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        out = np.empty_like(d)
        lib().orc_env_color(self.h, d.shape[0], d.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out

    def photon_map_from_photons(self, photon_count, kind, watts, gather_size, gather_size_volume, surface, volume, robust=0):
        """The maps of PhotonMap::new over photon lists handed in ((n, 10) arrays laid out as OraclePhotonMap.photons returns them):
        a camera pass on the very photons another implementation shot."""
        return OraclePhotonMap(self, photon_count, kind, watts, gather_size, gather_size_volume, 0, robust, photons=(surface, volume))

    def photon_map(self, photon_count, kind, watts, gather_size=50, gather_size_volume=50, seed=0, robust=0):
        """Renderer::photon_render's shooting + map build (src/photon.rs:655-704)."""
        return OraclePhotonMap(self, photon_count, kind, watts, gather_size, gather_size_volume, seed, robust)

    CHAIN_ROW = 12

    def photon_chains(self, photon_count, kind, watts, seed=0, robust=0, first=0, n=None, indices=None, amp=0.0, cloud_seed=0, verts=False):
        """orc_photon_chains: photons [first, first + n) (or `indices`) of a photon_count map, chain by chain, no map built.  -> dict:
        ns, nv (records per photon; volume after thinning), sig (u64 signature of the chain's decisions), surface, volume ((., 10) as
        OraclePhotonMap.photons lays them out), and with verts: nrows and rows ((., 12), see ChainTrace in rpt_oracle.cpp)."""
        L = lib()
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint64)
        m = int(n if idx is None else idx.size)
        h = L.orc_photon_chains(self.h, int(photon_count), int(first), m, None if idx is None else idx.ctypes.data_as(C.c_void_p), int(kind),
                                float(watts), int(seed), int(robust), float(amp), int(cloud_seed), int(bool(verts)))
        if not h:
            raise ValueError("Only found non-object lights while photon mapping")
        try:
            tot = np.zeros(3, dtype=np.uint64)
            L.orc_photon_chains_totals(h, tot.ctypes.data_as(C.c_void_p))
            out = {"ns": np.zeros(m, np.uint32), "nv": np.zeros(m, np.uint32), "nrows": np.zeros(m, np.uint32), "sig": np.zeros(m, np.uint64),
                   "surface": np.zeros((int(tot[0]), 10)), "volume": np.zeros((int(tot[1]), 10)), "rows": np.zeros((int(tot[2]), self.CHAIN_ROW))}
            L.orc_photon_chains_get(h, *[out[k].ctypes.data_as(C.c_void_p) for k in ("ns", "nv", "nrows", "sig", "surface", "volume", "rows")])
        finally:
            L.orc_photon_chains_free(h)
        return out

    def close(self):
        if self.h:
            lib().orc_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OraclePhotonMap:
    PHOTON_MAP, POINT_BEAM, BEAM_BEAM = 0, 1, 2

    def __init__(self, oscene, photon_count, kind, watts, gather_size, gather_size_volume, seed, robust, photons=None):
        self.oscene = oscene
        self.robust = robust
        if photons is not None:
            ps = np.ascontiguousarray(photons[0], dtype=np.float64).reshape(-1, 10)
            pv = np.ascontiguousarray(photons[1], dtype=np.float64).reshape(-1, 10)
            self.h = lib().orc_photon_map_from_photons(photon_count, kind, watts, gather_size, gather_size_volume,
                                                       ps.ctypes.data_as(C.c_void_p), len(ps), pv.ctypes.data_as(C.c_void_p), len(pv))
            return
        self.h = lib().orc_photon_map_build(oscene.h, photon_count, kind, watts, gather_size, gather_size_volume,
                                            C.c_uint64(seed), robust)
        if not self.h:
            raise ValueError("Only found non-object lights while photon mapping")

    def photons(self, which):
        """(n, 10) array: position, direction, power, radius (volume photons of the beam map)."""
        L = lib()
        n = L.orc_photon_map_get(self.h, which, None)
        out = np.zeros((n, 10))
        if n:
            L.orc_photon_map_get(self.h, which, out.ctypes.data_as(C.c_void_p))
        return out

    def render(self, camera, width, height, num_samples, seed=0, sample_offset=0, exposure_value=0.0, threads=None,
               pixels=None):
        from rpt_amd.api import camera_desc
        p = Params(width, height, exposure_value, 0, self.robust)
        out = np.zeros((width * height, 3))
        if threads is None:
            threads = os.cpu_count() or 1
        pl, npix = None, 0
        if pixels is not None:
            pl = np.ascontiguousarray(pixels, dtype=np.uint32)
            npix = pl.size
        lib().orc_photon_render(self.oscene.h, self.h, C.byref(camera_desc(camera, CameraDesc)), C.byref(p), num_samples,
                                C.c_uint64(seed), sample_offset, out.ctypes.data_as(C.c_void_p), threads,
                                pl.ctypes.data_as(C.c_void_p) if pl is not None else None, npix)
        return out

    def __del__(self):
        try:
            if self.h:
                lib().orc_photon_map_free(self.h)
                self.h = None
        except Exception:
            pass

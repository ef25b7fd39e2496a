"""Host-side mirror of rpt's builder API (same names, argument meaning and error behaviour),
lowered onto the C ABI of include/rpt_hip.h.  Reference: neevparikh/rpt `src/`:

    Scene / SceneAdd        scene.rs:12-81        Object            object.rs:10-31
    Light                   light.rs:7-19         Material          material.rs:8-97
    Medium                  medium.rs:78-122      Camera            camera.rs:9-62
    sphere/cube/plane/...   shape.rs:288-314      Transformed       shape.rs:102-285
    Renderer                renderer.rs:23-156    Buffer / Filter   buffer.rs:6-108
    hex_color/color_bytes   color.rs:10-24        Environment       environment.rs:56-77

Everything here is scene description and output bookkeeping in numpy fp64; the per-sample work
(`Renderer.sample`, renderer.rs:158-171) runs in the HIP library.  Additions with no
counterpart in the reference: `Renderer.seed(u64)` (the reference seeds from entropy,
renderer.rs:163), `Renderer.shard(rank, count)` (multi-GPU tiles) and `Renderer.device(i)`.
"""
import ctypes as C
import math
import weakref

import numpy as np

from . import _lib
from ._lib import RptError, vp as _vp

def shard_pixels(width, height, rank, count):
    """Pixel indices (y*width + x) owned by `rank` of `count` under the renderer's 32x32-tile
    sharding (rpt_shard_tiles), in ascending order."""
    lib = _lib.load()
    n = _lib.check(lib.rpt_shard_tiles(width, height, rank, count, None, 0))
    tiles = np.zeros(max(n, 1), dtype=np.uint32)
    _lib.check(lib.rpt_shard_tiles(width, height, rank, count, tiles.ctypes.data_as(C.c_void_p), n))
    tiles_x = (width + 31) // 32
    ys, xs = np.mgrid[0:32, 0:32]
    out = []
    for t in tiles[:n]:
        x = (int(t) % tiles_x) * 32 + xs
        y = (int(t) // tiles_x) * 32 + ys
        m = (x < width) & (y < height)
        out.append((y[m] * width + x[m]).astype(np.uint32))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, dtype=np.uint32)


_LIVE_SCENES = weakref.WeakSet()   # Scene objects that hold a device handle


def set_option(name, value):
    """Process-wide convenience over the C ABI's per-scene options: sets the default for scenes created from now on
    (rpt_set_option) and the option of every scene this process has on a device (rpt_scene_set_option), so that
    `set_option("counters", 1)` acts on the renderer at hand as it always did.  Options read by rpt_scene_commit
    ("scene_bvh_min", "instancing", "room_shell", "scan_specialise", "scan_cull", "shadow_scan", "bvh_leaf_max", "bvh_max_depth") only matter before a scene's
    first render; use Scene.set_option to give one scene its own value."""
    lib = _lib.load()
    _lib.check(lib.rpt_set_option(name.encode(), int(value)))
    for sc in list(_LIVE_SCENES):
        if sc._handle is not None:
            _lib.check(lib.rpt_scene_set_option(sc._handle, name.encode(), int(value)))


__all__ = [
    "set_option", "shard_pixels",
    "vec3", "hex_color", "color_bytes", "Sphere", "Cube", "Plane", "Triangle", "Mesh", "KdTree", "Transformed",
    "MonomialSurface", "sphere", "cube", "plane", "polygon", "monomial_surface", "Material", "Object", "Light", "Medium", "Environment",
    "Scene", "Camera", "Filter", "Buffer", "DeviceBuffer", "Renderer", "RptError", "DenoiseParams", "Denoiser", "AdaptiveParams",
    "TemporalParams", "TemporalAccumulator", "temporal_camera_record", "temporal_motion_record",
    "UpsampleParams", "upsample", "upsample_device", "image_bytes_device",
]


def vec3(x, y, z):
    """glm::vec3"""
    return np.array([x, y, z], dtype=np.float64)


def _v(a):
    a = np.asarray(a, dtype=np.float64)
    if a.shape != (3,):
        raise ValueError("expected a 3-vector")
    return a


# ------------------------------------------------------------------ color.rs
SRGB_GAMMA = 2.2


def hex_color(x):
    """color.rs:10-15: sRGB hex integer -> linear RGB (gamma 2.2)."""
    r = ((x >> 16) & 0xFF) / 255.0
    g = ((x >> 8) & 0xFF) / 255.0
    b = (x & 0xFF) / 255.0
    return vec3(r ** SRGB_GAMMA, g ** SRGB_GAMMA, b ** SRGB_GAMMA)


def color_bytes(color):
    """color.rs:18-24: clamp, gamma 1/2.2, *255, truncating `as u8`.  Accepts (...,3) arrays."""
    c = np.clip(np.asarray(color, dtype=np.float64), 0.0, 1.0) ** (1.0 / SRGB_GAMMA) * 255.0
    c = np.where(np.isnan(c), 0.0, c)
    return c.astype(np.uint8)


# ------------------------------------------------------------------ shapes (shape.rs)
def _translate(v):
    m = np.eye(4)
    m[:3, 3] = _v(v)
    return m


def _scale(v):
    return np.diag(np.append(_v(v), 1.0))


def _rotate(angle, axis):
    # glm::rotate(identity, angle, axis): axis is normalised, right-handed
    a = _v(axis)
    a = a / np.linalg.norm(a)
    c, s = math.cos(angle), math.sin(angle)
    x, y, z = a
    r = np.array([
        [c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
        [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
        [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)],
    ])
    m = np.eye(4)
    m[:3, :3] = r
    return m


class Shape:
    """trait Shape + Transformable (shape.rs:19-26, 179-230)."""
    KIND = -1

    def _wrap(self, m):
        return Transformed(self, m)

    def translate(self, v):
        return self._wrap(_translate(v))

    def scale(self, v):
        return self._wrap(_scale(v))

    def rotate(self, angle, axis):
        return self._wrap(_rotate(angle, axis))

    def rotate_x(self, angle):
        return self._wrap(_rotate(angle, (1, 0, 0)))

    def rotate_y(self, angle):
        return self._wrap(_rotate(angle, (0, 1, 0)))

    def rotate_z(self, angle):
        return self._wrap(_rotate(angle, (0, 0, 1)))

    def transform(self, m):
        return self._wrap(np.asarray(m, dtype=np.float64).reshape(4, 4))

    # -- lowering helpers (shared by the HIP binding and, in tests, the oracle binding)
    def base(self):
        return self

    def matrix(self):
        return None


class Sphere(Shape):
    """Unit sphere at the origin (shape/sphere.rs:10)."""
    KIND = 0


class Cube(Shape):
    """Unit cube centred at the origin (shape/cube.rs:10)."""
    KIND = 1


class Plane(Shape):
    """x . normal = value (shape/plane.rs:7-13)."""
    KIND = 2

    def __init__(self, normal, value):
        self.normal = _v(normal)
        self.value = float(value)


class MonomialSurface(Shape):
    """y = height * (x^2 + z^2)^2 for x^2 + z^2 <= 1, two-sided (shape/monomial_surface.rs:8-19).  `exp` is stored but, as in
    the reference, intersection hard-codes the exponent 4.  Bounded: it may sit in a KdTree.  Not a Light::Object, and scenes that
    hold one are not photon-mapped (the library refuses both)."""
    KIND = 5

    def __init__(self, height, exp):
        self.height = float(height)
        self.exp = float(exp)

    def _closest(self, point, precise):
        p = (C.c_double * 3)(*[float(x) for x in point])
        out = (C.c_double * 3)()
        _lib.check(_lib.load().rpt_monomial_closest_point(self.height, p, precise, out))
        return np.array(out[:], dtype=np.float64)

    def closest_point(self, point):
        """The closest of the 201 curve samples xf = -1, -0.99 .. 1 to `point`, rotated back about the axis
        (monomial_surface.rs:126-151; the exponent is 4, as there).  A host function: include/rpt_hip.h states its arithmetic."""
        return self._closest(point, 0)

    def closest_point_precise(self, point):
        """... of 20,001 samples (monomial_surface.rs:154-178)."""
        return self._closest(point, 1)


class Triangle:
    """shape/mesh.rs:9-39."""

    def __init__(self, v1, v2, v3, n1, n2, n3):
        self.v1, self.v2, self.v3 = _v(v1), _v(v2), _v(v3)
        self.n1, self.n2, self.n3 = _v(n1), _v(n2), _v(n3)

    @staticmethod
    def from_vertices(v1, v2, v3):
        v1, v2, v3 = _v(v1), _v(v2), _v(v3)
        n = np.cross(v2 - v1, v3 - v1)
        n = n / np.linalg.norm(n)
        return Triangle(v1, v2, v3, n, n, n)


class Mesh(Shape):
    """`Mesh = KdTree<Triangle>` (shape/mesh.rs:103).  Holds an (n, 6, 3) fp64 array:
    v1 v2 v3 n1 n2 n3 per triangle.  The acceleration structure is built in the library."""
    KIND = 3

    def __init__(self, triangles):
        if isinstance(triangles, np.ndarray):
            arr = np.ascontiguousarray(triangles, dtype=np.float64).reshape(-1, 6, 3)
        else:
            arr = np.array([[t.v1, t.v2, t.v3, t.n1, t.n2, t.n3] for t in triangles], dtype=np.float64).reshape(-1, 6, 3)
        self.tris = arr

    def clone(self):
        return Mesh(self.tris.copy())


class KdTree(Shape):
    """`KdTree<Box<dyn Bounded>>` used as one shape (kdtree.rs:103-146; examples/fractal_spheres.rs:45):
    a group of bounded shapes (spheres, cubes, meshes, nested groups, transformed or not) sharing
    one material.  Planes are not `Bounded` and are rejected."""
    KIND = 4

    def __init__(self, shapes):
        self.shapes = list(shapes)
        if not self.shapes:
            raise ValueError("KdTree needs at least one shape")
        for s in self.shapes:
            if isinstance(s.base(), Plane):
                raise TypeError("Plane is not Bounded and cannot be put in a KdTree")

    def clone(self):
        return KdTree(self.shapes)


class Transformed(Shape):
    """shape.rs:102-125.  Chained calls left-multiply and do not nest (shape.rs:232-285)."""

    def __init__(self, shape, m):
        if isinstance(shape, Transformed):
            m = np.asarray(m) @ shape.m
            shape = shape.shape
        self.shape = shape
        self.m = np.asarray(m, dtype=np.float64).reshape(4, 4)

    def _wrap(self, m):
        return Transformed(self.shape, m @ self.m)

    def base(self):
        return self.shape

    def matrix(self):
        return self.m

    def clone(self):
        return Transformed(self.shape, self.m.copy())


def sphere():
    return Sphere()


def cube():
    return Cube()


def plane(normal, value):
    return Plane(normal, value)


def monomial_surface(height, exp):
    """shape.rs:292-295."""
    return MonomialSurface(height, exp)


def polygon(verts):
    """shape.rs:308-314: fan triangulation from verts[0]."""
    verts = [_v(p) for p in verts]
    return Mesh([Triangle.from_vertices(verts[0], verts[i], verts[i + 1]) for i in range(1, len(verts) - 1)])


# ------------------------------------------------------------------ material.rs
class Material:
    LAMBERTIAN, PHONG, MIRROR, TRANSMISSIVE = 0, 1, 2, 3

    def __init__(self, kind=0, albedo=(0.5, 0.5, 0.5), emittance=0.0, shininess=0.0, ior=1.0):
        self.kind = kind
        self.albedo = _v(albedo)
        self.emittance_ = float(emittance)
        self.shininess = float(shininess)
        self.ior = float(ior)

    # constructors, material.rs:34-97
    @staticmethod
    def diffuse(color):
        return Material(Material.LAMBERTIAN, color)

    @staticmethod
    def specular(color, roughness):
        return Material(Material.PHONG, color, shininess=roughness)  # roughness IS the shininess (sic)

    @staticmethod
    def mirror():
        return Material(Material.MIRROR, (0, 0, 0))

    @staticmethod
    def transmissive(ior):
        return Material(Material.TRANSMISSIVE, (0, 0, 0), ior=ior)

    @staticmethod
    def clear(index, _roughness=0.0):
        return Material(Material.TRANSMISSIVE, (0, 0, 0), ior=index)

    @staticmethod
    def transparent(color, index, _roughness=0.0):
        return Material(Material.TRANSMISSIVE, color, ior=index)

    @staticmethod
    def metallic(color, roughness):
        return Material(Material.PHONG, color, shininess=roughness)

    @staticmethod
    def light(color, emittance):
        return Material(Material.LAMBERTIAN, color, emittance=emittance)

    def emittance(self):  # material.rs:100-106
        return self.emittance_ if self.kind in (0, 1) else 0.0

    def color(self):  # material.rs:107-113
        return self.albedo if self.kind in (0, 1) else vec3(0, 0, 0)


class Object:
    """object.rs:10-31."""

    def __init__(self, shape):
        if not isinstance(shape, Shape):
            raise TypeError("Object::new expects a shape")
        self.shape = shape
        self.material_ = Material()

    def material(self, material):
        self.material_ = material
        return self


class Light:
    """enum Light (light.rs:7-19)."""
    POINT, AMBIENT, DIRECTIONAL, OBJECT = 0, 1, 2, 3

    def __init__(self, kind, color=None, vec=None, obj=None):
        self.kind, self.color, self.vec, self.object = kind, color, vec, obj

    @staticmethod
    def Point(color, location):
        return Light(Light.POINT, _v(color), _v(location))

    @staticmethod
    def Ambient(color):
        return Light(Light.AMBIENT, _v(color))

    @staticmethod
    def Directional(color, direction):
        return Light(Light.DIRECTIONAL, _v(color), _v(direction))

    @staticmethod
    def Object(obj):
        return Light(Light.OBJECT, obj=obj)


class Medium:
    """medium.rs:78-122: the two constructors are the closed set (fields are private)."""
    HOMOGENEOUS_ISOTROPIC, COLORED_GLOWING_FOG = 0, 1

    def __init__(self, kind, absorption, scattering):
        self.kind, self.absorption, self.scattering = kind, float(absorption), float(scattering)

    @staticmethod
    def homogeneous_isotropic(absorption, scattering):
        return Medium(Medium.HOMOGENEOUS_ISOTROPIC, absorption, scattering)

    @staticmethod
    def colored_glowing_fog(absorption, scattering):
        return Medium(Medium.COLORED_GLOWING_FOG, absorption, scattering)


class Environment:
    """environment.rs:3-77: Environment::Color(c) or Environment::Hdri(Hdri::new(width, height, buf))."""

    def __init__(self, color=(0, 0, 0), hdri=None):
        self.color = _v(color)
        self.hdri = hdri          # (height, width, 3) fp64 array or None

    @staticmethod
    def Color(color):
        return Environment(color)

    @staticmethod
    def Hdri(width, height, buf):
        buf = np.ascontiguousarray(buf, dtype=np.float64).reshape(-1, 3)
        assert buf.shape[0] == width * height and width > 0 and height > 0     # Hdri::new, environment.rs:18-22
        return Environment((0, 0, 0), buf.reshape(height, width, 3))


class Scene:
    """scene.rs:12-81."""

    def __init__(self):
        self.objects, self.lights, self.media = [], [], []
        self.environment = Environment((0, 0, 0))
        self._handle = None
        self._options = {}

    @staticmethod
    def new():
        return Scene()

    def add(self, node):
        if self._handle is not None:
            raise RptError("scene is immutable once rendered (committed to the device)")
        if isinstance(node, Object):
            self.objects.append(node)
        elif isinstance(node, Light):
            self.lights.append(node)
        elif isinstance(node, Medium):
            self.media.append(node)
        elif isinstance(node, tuple) and len(node) == 2 and isinstance(node[1], Material):
            # SceneAdd<(Mesh, Material)> / SceneAdd<(Transformed<Cube>, Material)>, scene.rs:57-75:
            # the same geometry becomes an Object AND a Light::Object
            shape, material = node
            ok = isinstance(shape, Mesh) or (isinstance(shape, Transformed) and isinstance(shape.shape, Cube))
            if not ok:
                raise TypeError("SceneAdd is implemented for (Mesh, Material) and (Transformed<Cube>, Material)")
            self.add(Object(shape.clone()).material(material))
            self.add(Light.Object(Object(shape.clone()).material(material)))
        else:
            raise TypeError(f"cannot add {type(node).__name__} to a Scene")

    def set_option(self, name, value):
        """rpt_scene_set_option: this scene's own value of an option (see rpt_hip.h), whatever other scenes use."""
        self._options[name] = int(value)
        if self._handle is not None:
            _lib.check(_lib.load().rpt_scene_set_option(self._handle, name.encode(), int(value)))
        return self

    # ---- lowering onto the C ABI
    def _commit(self, device):
        if self._handle is not None:
            if self._device != device:
                raise RptError("scene already committed to another device")
            return self._handle
        lib = _lib.load()
        h = lib.rpt_scene_create()
        try:
            for o in self.objects:
                sd, keep = shape_desc(o.shape, _lib.ShapeDesc)
                _lib.check(lib.rpt_scene_add_object(h, C.byref(sd), C.byref(material_desc(o.material_, _lib.MaterialDesc))))
            for l in self.lights:
                if l.kind == Light.POINT:
                    _lib.check(lib.rpt_scene_add_light_point(h, _dp(l.color), _dp(l.vec)))
                elif l.kind == Light.AMBIENT:
                    _lib.check(lib.rpt_scene_add_light_ambient(h, _dp(l.color)))
                elif l.kind == Light.DIRECTIONAL:
                    _lib.check(lib.rpt_scene_add_light_directional(h, _dp(l.color), _dp(l.vec)))
                else:
                    sd, keep = shape_desc(l.object.shape, _lib.ShapeDesc)
                    _lib.check(lib.rpt_scene_add_light_object(
                        h, C.byref(sd), C.byref(material_desc(l.object.material_, _lib.MaterialDesc))))
            for m in self.media:
                _lib.check(lib.rpt_scene_add_medium(h, m.kind, m.absorption, m.scattering))
            env = self.environment
            if env.hdri is not None:
                _lib.check(lib.rpt_scene_set_environment_hdri(h, env.hdri.shape[1], env.hdri.shape[0], _dp(env.hdri)))
            else:
                _lib.check(lib.rpt_scene_set_environment_color(h, _dp(env.color)))
            for name, value in self._options.items():
                _lib.check(lib.rpt_scene_set_option(h, name.encode(), value))
            _lib.check(lib.rpt_scene_commit(h, device))
        except Exception:
            lib.rpt_scene_destroy(h)
            raise
        self._handle, self._device = h, device
        _LIVE_SCENES.add(self)
        return h

    # ---- moving spheres (rpt_hip.h, "moving spheres": an addition): the one change a committed scene takes
    def set_movable_spheres(self, objects, device=0):
        """rpt_scene_set_movable_spheres: `objects` are indices into self.objects of spheres under translate(c) * scale(r, r, r);
        the scene is committed to `device` if it has not been.  A second call replaces the list.  self.objects keeps describing
        the scene as it was committed."""
        h = self._commit(self._device if self._handle is not None else device)
        objects = np.ascontiguousarray(objects, dtype=np.uint32).reshape(-1)
        _lib.check(_lib.load().rpt_scene_set_movable_spheres(h, _lib.vp(objects), len(objects)))
        self._movable = objects.copy()
        return self

    def _movable_handle(self, what):
        if self._handle is None or getattr(self, "_movable", None) is None:
            raise RptError(f"{what}: set_movable_spheres must be called first")
        return self._handle

    def move_spheres(self, centres, offsets=None, motion=False):
        """rpt_scene_move_spheres: listed sphere k moves to centres[k] (+ offsets[k], one rounded add per component); synchronous.
        With motion=True returns the (len(self.objects), 24) motion table of the move: rpt_temporal_motion_record of each listed
        sphere's new and previous matrix, identity for every other object."""
        h = self._movable_handle("move_spheres")
        n = len(self._movable)
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 3)
        if len(centres) != n or (offsets is not None and len(offsets) != n):
            raise ValueError(f"move_spheres: {n} movable spheres, {len(centres)} centres")
        table = np.zeros((len(self.objects), 24)) if motion else None
        _lib.check(_lib.load().rpt_scene_move_spheres(h, _lib.vp(centres) if n else None, _lib.vp(offsets) if offsets is not None and n else None,
                                                      _lib.vp(table) if motion and len(self.objects) else None))
        return table

    def move_spheres_device(self, d_centres, d_offsets=0, d_motion=0, stream_ptr=0):
        """rpt_scene_move_spheres_device: centres (n x 3 doubles), offsets (or 0) and the motion table (len(self.objects) x 24
        doubles that hold identity records, or 0) are device addresses; asynchronous on `stream_ptr` and ordered like a render of
        the scene."""
        h = self._movable_handle("move_spheres_device")
        _lib.check(_lib.load().rpt_scene_move_spheres_device(h, C.c_void_p(d_centres or None), C.c_void_p(d_offsets or None), C.c_void_p(d_motion or None),
                                                             C.c_void_p(stream_ptr or None)))

    def movable_info(self):
        """rpt_scene_movable_info as a dict."""
        if self._handle is None:
            raise RptError("movable_info: the scene is not committed")
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().rpt_scene_movable_info(self._handle, out))
        keys = ("set", "spheres", "tree_nodes", "tree_heights", "cull32_groups", "moves", "table_bytes", "epsilon")
        return dict(zip(keys, (int(x) for x in out)))

    def debug_records(self, which, dtype=np.uint8):
        """rpt_debug_scene_records: one of the arrays an update touches (RPT_SCENE_RECORDS_*), downloaded, as a flat array of `dtype`."""
        if self._handle is None:
            raise RptError("debug_records: the scene is not committed")
        lib = _lib.load()
        n = C.c_uint64()
        _lib.check(lib.rpt_debug_scene_records(self._handle, int(which), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            _lib.check(lib.rpt_debug_scene_records(self._handle, int(which), _lib.vp(out), n.value, C.byref(n)))
        return out.view(dtype)

    def close(self):
        if self._handle is not None:
            _lib.load().rpt_scene_destroy(self._handle)
            self._handle = None
            self._movable = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dp(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def shape_desc(shape, cls):
    """Fill a rpt_shape_desc-shaped ctypes struct `cls` from a Shape.  Returns (desc, keepalive)."""
    base, m = shape.base(), shape.matrix()
    d = cls()
    d.kind = base.KIND
    d.has_transform = 0 if m is None else 1
    flat = (np.eye(4) if m is None else m).reshape(-1)
    for i in range(16):
        d.transform[i] = float(flat[i])
    keep = None
    if isinstance(base, Plane):
        for i in range(3):
            d.plane_normal[i] = float(base.normal[i])
        d.plane_value = base.value
    elif isinstance(base, MonomialSurface):
        d.plane_normal[0] = base.height
        d.plane_normal[1] = base.exp
    elif isinstance(base, Mesh):
        keep = np.ascontiguousarray(base.tris, dtype=np.float64)
        d.tris = keep.ctypes.data_as(C.POINTER(C.c_double))
        d.n_tris = keep.shape[0]
    elif isinstance(base, KdTree):
        arr = (cls * len(base.shapes))()
        keep = [arr]
        for i, child in enumerate(base.shapes):
            cd, ck = shape_desc(child, cls)
            C.memmove(C.byref(arr, i * C.sizeof(cls)), C.byref(cd), C.sizeof(cls))
            keep.append(ck)
        d.children = C.cast(arr, C.POINTER(cls))
        d.n_children = len(base.shapes)
    elif not isinstance(base, (Sphere, Cube)):
        raise TypeError(f"unsupported shape {type(base).__name__}")
    d._keep = keep
    return d, keep


def material_desc(mat, cls):
    d = cls()
    d.kind = mat.kind
    for i in range(3):
        d.albedo[i] = float(mat.albedo[i])
    d.emittance = mat.emittance_
    d.shininess = mat.shininess
    d.ior = mat.ior
    return d


# ------------------------------------------------------------------ camera.rs
class Camera:
    def __init__(self, eye=(0.0, 0.0, 10.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0),
                 fov=math.pi / 6, aperture=0.0, focal_distance=0.0):
        self.eye, self.direction, self.up = _v(eye), _v(direction), _v(up)
        self.fov, self.aperture, self.focal_distance = float(fov), float(aperture), float(focal_distance)

    @staticmethod
    def look_at(eye, center, up, fov):  # camera.rs:44-56
        eye, center, up = _v(eye), _v(center), _v(up)
        direction = center - eye
        direction = direction / np.linalg.norm(direction)
        up = up - np.dot(up, direction) * direction
        up = up / np.linalg.norm(up)
        return Camera(eye, direction, up, fov)

    def focus(self, focal_point, aperture):  # camera.rs:58-62
        self.focal_distance = float(np.dot(_v(focal_point) - self.eye, self.direction))
        self.aperture = float(aperture)
        return self


def camera_desc(cam, cls):
    d = cls()
    for i in range(3):
        d.eye[i], d.direction[i], d.up[i] = float(cam.eye[i]), float(cam.direction[i]), float(cam.up[i])
    d.fov, d.aperture, d.focal_distance = cam.fov, cam.aperture, cam.focal_distance
    return d


# ------------------------------------------------------------------ buffer.rs
class Filter:
    def __init__(self, radius=0):
        self.radius = int(radius)

    @staticmethod
    def Box(radius):
        return Filter(radius)

    @staticmethod
    def default():
        return Filter(0)


class Buffer:
    """buffer.rs:6-93: one mean colour per pixel per `sample()` call."""

    def __init__(self, width, height, filter=None):
        self.width, self.height = int(width), int(height)
        self.samples = []  # list of (h*w, 3) arrays, one per add_samples call
        self.filter = filter or Filter.default()

    def add_samples(self, samples):
        samples = np.asarray(samples, dtype=np.float64).reshape(-1, 3)
        assert samples.shape[0] == self.width * self.height, "Invalid sample dimension"
        self.samples.append(samples)

    def _filtered(self):
        assert self.samples, "Pixel found with no samples"
        total = np.sum(self.samples, axis=0).reshape(self.height, self.width, 3)
        count = float(len(self.samples))
        r = self.filter.radius
        if r == 0:
            return total / count
        # box window clipped to the image: sum of sums / sum of counts (buffer.rs:75-93)
        pad = np.zeros((self.height + 2 * r, self.width + 2 * r, 3))
        pad[r:r + self.height, r:r + self.width] = total
        cnt = np.zeros((self.height + 2 * r, self.width + 2 * r))
        cnt[r:r + self.height, r:r + self.width] = count
        acc = np.zeros_like(total)
        cacc = np.zeros((self.height, self.width))
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                acc += pad[dy:dy + self.height, dx:dx + self.width]
                cacc += cnt[dy:dy + self.height, dx:dx + self.width]
        return acc / cacc[..., None]

    def image(self):
        """(h, w, 3) uint8, the analogue of image::RgbImage (buffer.rs:43-56)."""
        return color_bytes(self._filtered())

    def variance(self):
        """buffer.rs:59-73: mean per-pixel sample variance across batches (n-1 dof)."""
        s = np.stack(self.samples)  # (n, hw, 3)
        n = s.shape[0]
        mean = s.mean(axis=0)
        ss = ((s - mean) ** 2).sum(axis=2).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.mean(ss / (n - 1.0)))


class DeviceBuffer:
    """The same Buffer kept on the GPU (rpt_buffer_*): per-pixel running sums, box filter +
    color_bytes and variance computed where the frame is.  What Renderer.render() and
    iterative_render() use; `Buffer` above is the host restatement."""

    def __init__(self, width, height, filter=None, device=0):
        self.width, self.height = int(width), int(height)
        self.filter = filter or Filter.default()
        self.device = int(device)
        self._h = _lib.load().rpt_buffer_create(self.device, self.width, self.height, int(self.filter.radius))
        if not self._h:
            _lib.check(-1)

    def add_samples(self, samples):
        samples = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 3)
        assert samples.shape[0] == self.width * self.height, "Invalid sample dimension"
        _lib.check(_lib.load().rpt_buffer_add_samples(self._h, samples.ctypes.data_as(C.c_void_p)))

    def add_samples_device(self, d_rgb_ptr, stream_ptr=0):
        _lib.check(_lib.load().rpt_buffer_add_samples_device(self._h, C.c_void_p(d_rgb_ptr), C.c_void_p(stream_ptr)))

    @property
    def batches(self):
        n = C.c_uint32()
        _lib.check(_lib.load().rpt_buffer_batches(self._h, C.byref(n)))
        return int(n.value)

    def image(self):
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        _lib.check(_lib.load().rpt_buffer_image(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def variance(self):
        v = C.c_double()
        _lib.check(_lib.load().rpt_buffer_variance(self._h, C.byref(v)))
        return float(v.value)

    def mean_device(self, d_rgb_ptr, d_var_ptr, stream_ptr=0):
        """rpt_buffer_mean_device: device pointers to width*height*3 and width*height doubles (d_var_ptr 0 / None: not computed)."""
        _lib.check(_lib.load().rpt_buffer_mean_device(self._h, C.c_void_p(d_rgb_ptr or None), C.c_void_p(d_var_ptr or None),
                                                      C.c_void_p(stream_ptr)))

    def mean(self):
        """-> (rgb, var): the per-pixel mean of the batches in push order, (h, w, 3), and the variance of that mean, (h, w): what
        Denoiser.denoise takes.  Needs at least two batches."""
        n = self.width * self.height
        d = _device_zeros(4 * n, self.device)
        _sync(self.device)                                       # batches may have been added on other streams
        self.mean_device(d.data_ptr(), d.data_ptr() + 24 * n)
        host = d.cpu().numpy()
        return host[:3 * n].reshape(self.height, self.width, 3).copy(), host[3 * n:].reshape(self.height, self.width).copy()

    # ---- adaptive sampling by tile (an addition)
    @property
    def tiles(self):
        """(tiles_x, tiles_y): the frame in 32 x 32 tiles; a tile id is ty * tiles_x + tx."""
        return (self.width + 31) // 32, (self.height + 31) // 32

    def add_samples_tiles_device(self, d_rgb_ptr, d_tiles_ptr, n_tiles, stream_ptr=0):
        """rpt_buffer_add_samples_tiles_device: one batch for the listed tiles alone (device frame, device list of n_tiles distinct
        uint32 ids); the tiles' batch counts go up by one."""
        n_tiles = int(n_tiles)
        if n_tiles < 0 or n_tiles > self.tiles[0] * self.tiles[1]:
            raise ValueError(f"add_samples_tiles_device: {n_tiles} tiles listed, the frame has {self.tiles[0] * self.tiles[1]}")
        if not d_rgb_ptr or (n_tiles and not d_tiles_ptr):
            raise ValueError("add_samples_tiles_device: null pointer")
        _lib.check(_lib.load().rpt_buffer_add_samples_tiles_device(self._h, C.c_void_p(d_rgb_ptr), C.c_void_p(d_tiles_ptr or None), n_tiles,
                                                                   C.c_void_p(stream_ptr)))

    def tile_batches(self):
        """-> (tiles_y, tiles_x) uint32: the batches every pixel of a tile holds (full-frame batches + the tile's own)."""
        tx, ty = self.tiles
        out = np.empty((ty, tx), dtype=np.uint32)
        _lib.check(_lib.load().rpt_buffer_tile_batches(self._h, _vp(out), out.size))
        return out

    def tile_errors(self, floor):
        """rpt_buffer_tile_errors_device -> (tiles_y, tiles_x) float64: per tile, the mean of v / (y^2 + floor^2) over its pixels
        (v the variance of the pixel's mean, y the sum of its mean's channels).  Needs at least two full-frame batches."""
        floor = float(floor)
        if not (floor > 0.0) or math.isinf(floor):
            raise ValueError("tile_errors: floor must be finite and > 0")
        tx, ty = self.tiles
        d = _device_zeros(tx * ty, self.device)
        _sync(self.device)                                       # batches may have been added on other streams
        _lib.check(_lib.load().rpt_buffer_tile_errors_device(self._h, floor, C.c_void_p(d.data_ptr()), None))
        _sync(self.device)
        return d.cpu().numpy().reshape(ty, tx).copy()

    def refine_tiles(self, params):
        """rpt_buffer_refine_tiles -> (ids, errors): the ascending ids of the tiles whose error is above params.threshold ** 2 and
        that hold fewer than params.max_batches batches, uint32, and every tile's error, (tiles_y, tiles_x) float64."""
        import torch
        tx, ty = self.tiles
        d_err = _device_zeros(tx * ty, self.device)
        d_ids = torch.zeros(tx * ty, dtype=torch.int32, device=f"cuda:{self.device}")
        _sync(self.device)
        n = C.c_uint32()
        _lib.check(_lib.load().rpt_buffer_refine_tiles(self._h, C.byref(params.desc()), C.c_void_p(d_ids.data_ptr()), C.byref(n),
                                                       C.c_void_p(d_err.data_ptr()), None))
        _sync(self.device)
        return d_ids.cpu().numpy().view(np.uint32)[:n.value].copy(), d_err.cpu().numpy().reshape(ty, tx).copy()

    def _plane_pointers(self, planes, what, scale=1):
        """`planes`: a dict with any of "albedo", "normal", "depth", each an (h, w, 3) array as Renderer.features_array returns it or a
        device pointer (int) as Renderer.features_device filled it -> (what keeps the uploads alive, the three pointers).  scale:
        the planes are that many times the buffer's size on each axis."""
        unknown = set(planes) - {"albedo", "normal", "depth"}
        if unknown:
            raise ValueError(f"{what}: unknown planes {sorted(unknown)}")
        keep, ptrs = [], []
        for k in ("albedo", "normal", "depth"):
            v = planes.get(k)
            if v is None or isinstance(v, int):
                ptrs.append(C.c_void_p(v or None))
                continue
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.size != scale * self.width * scale * self.height * 3:
                raise ValueError(f"{what}: plane {k} is not {scale * self.height} x {scale * self.width} x 3")
            keep.append(_device_copy(a, self.device))
            ptrs.append(C.c_void_p(keep[-1].data_ptr()))
        _sync(self.device)
        return keep, ptrs

    def denoised_image(self, denoiser, planes, params=None):
        """rpt_buffer_denoised_image: mean -> a-trous filter -> color_bytes, no box filter -> (h, w, 3) uint8.  `planes`: a dict with
        any of "albedo", "normal", "depth" (what `params` needs), each an (h, w, 3) array as Renderer.features_array returns it or
        a device pointer (int) as Renderer.features_device filled it."""
        params = params or DenoiseParams()
        keep, ptrs = self._plane_pointers(planes, "denoised_image")
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        _lib.check(_lib.load().rpt_buffer_denoised_image(self._h, denoiser._h, C.byref(params.desc()), *ptrs, _vp(out)))
        return out

    def upsampled_image(self, planes, hi_planes, params=None, denoiser=None, denoise=None):
        """rpt_buffer_upsampled_image: this buffer holds the LOW-resolution batches; mean -> (with `denoiser`, of this buffer's size:
        the a-trous filter at the low resolution, parameters `denoise`) -> guided upsampling -> color_bytes ->
        (s h, s w, 3) uint8.  `planes`: the low-resolution feature planes as for denoised_image; `hi_planes`: the same dict for the
        full-resolution ones, arrays of (s h, s w, 3) or device pointers."""
        params = params or UpsampleParams()
        if denoiser is not None:
            denoise = denoise or DenoiseParams()
        s = params.scale
        if s not in (2, 3, 4):
            raise ValueError("upsampled_image: scale must be 2, 3 or 4")
        keep, ptrs = self._plane_pointers(planes, "upsampled_image")
        hi_keep, hi_ptrs = self._plane_pointers(hi_planes, "upsampled_image", s)
        out = np.empty((s * self.height, s * self.width, 3), dtype=np.uint8)
        _lib.check(_lib.load().rpt_buffer_upsampled_image(
            self._h, denoiser._h if denoiser is not None else None, C.byref(denoise.desc()) if denoise is not None else None,
            C.byref(params.desc()), *ptrs, *hi_ptrs, _vp(out)))
        return out

    def temporal_image(self, accumulator, camera, planes, temporal=None, denoiser=None, denoise=None):
        """rpt_temporal_frame_image: mean and variance -> the accumulation -> (with `denoiser`: the a-trous filter with the
        accumulated variance, parameters `denoise`) -> color_bytes -> (h, w, 3) uint8.  `camera` is the camera the batches and the
        planes were rendered with; `planes` as for denoised_image, "depth" always, "normal" where temporal.normal_tol > 0 or the
        filter needs it."""
        temporal = temporal or TemporalParams()
        if denoiser is not None:
            denoise = denoise or DenoiseParams()
        keep, ptrs = self._plane_pointers(planes, "temporal_image")
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        _lib.check(_lib.load().rpt_temporal_frame_image(
            accumulator._h, C.byref(temporal.desc()), C.byref(camera_desc(camera, _lib.CameraDesc)), self._h,
            denoiser._h if denoiser is not None else None, C.byref(denoise.desc()) if denoise is not None else None, *ptrs, _vp(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rpt_buffer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ denoiser (rpt_denoise*, an addition)
def _device_zeros(n_doubles, device):
    """Device scratch of the wrappers that hand host arrays to a device-pointer entry point (torch is the allocator, imported lazily
    as in rpt_amd.dist: `import rpt_amd` stays numpy-only)."""
    import torch
    return torch.zeros(int(n_doubles), dtype=torch.float64, device=f"cuda:{int(device)}")


def _device_copy(a, device):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).to(f"cuda:{int(device)}")   # (a copy: the caller's array may be read-only)


def _sync(device):
    import torch
    torch.cuda.synchronize(int(device))


class DenoiseParams:
    """rpt_denoise_params.  A term is on iff its sigma > 0.  The defaults are those of the CPU prototype on the oracle's renders
    ("Denoiser"); sigma_depth is off because it is in scene units per pixel step and no default is right for
    every scene."""
    DEMODULATE, MATCH_ID = 1, 2

    def __init__(self, passes=4, demodulate=True, match_id=True, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.0):
        self.passes = int(passes)
        self.demodulate, self.match_id = bool(demodulate), bool(match_id)
        self.sigma_color, self.sigma_normal, self.sigma_depth = float(sigma_color), float(sigma_normal), float(sigma_depth)

    @property
    def flags(self):
        return (self.DEMODULATE if self.demodulate else 0) | (self.MATCH_ID if self.match_id else 0)

    def desc(self):
        return _lib.DenoiseParams(self.passes, self.flags, self.sigma_color, self.sigma_normal, self.sigma_depth)


class AdaptiveParams:
    """rpt_adaptive_params: batches of spp_per_batch samples; every tile gets min_batches (>= 2) of them, then one more per round
    while its error -- the mean over its pixels of the squared relative standard error of the pixel's mean, `floor` added to the
    squared brightness -- is above threshold ** 2 and it holds fewer than max_batches."""

    def __init__(self, spp_per_batch=4, min_batches=4, max_batches=16, threshold=0.05, floor=0.05):
        self.spp_per_batch, self.min_batches, self.max_batches = int(spp_per_batch), int(min_batches), int(max_batches)
        self.threshold, self.floor = float(threshold), float(floor)
        if self.spp_per_batch < 1:
            raise ValueError("AdaptiveParams: spp_per_batch must be at least 1")
        if self.min_batches < 2:
            raise ValueError("AdaptiveParams: min_batches must be at least 2")
        if self.max_batches < self.min_batches:
            raise ValueError("AdaptiveParams: max_batches must be at least min_batches")
        if self.max_batches * self.spp_per_batch >= 1 << 32:
            raise ValueError("AdaptiveParams: max_batches * spp_per_batch must fit 32 bits")
        if not self.threshold >= 0.0:
            raise ValueError("AdaptiveParams: threshold must be >= 0 (inf allowed)")
        if not self.floor > 0.0 or math.isinf(self.floor):
            raise ValueError("AdaptiveParams: floor must be finite and > 0")

    def desc(self):
        return _lib.AdaptiveParams(self.spp_per_batch, self.min_batches, self.max_batches, 0, self.threshold, self.floor)


class Denoiser:
    """rpt_denoiser: the variance-guided a-trous filter of include/rpt_hip.h for frames of one size on one device."""

    def __init__(self, width, height, device=0):
        self.width, self.height, self.device = int(width), int(height), int(device)
        if self.width <= 0 or self.height <= 0:
            raise ValueError("Denoiser: empty frame")
        self._h = _lib.load().rpt_denoiser_create(self.device, self.width, self.height)
        if not self._h:
            _lib.check(-1)

    def denoise(self, rgb, var, albedo, normal, depth, params=None, return_variance=False):
        """Host arrays: rgb, albedo, normal, depth of (h, w, 3), var of (h, w); any but rgb may be None where `params` does not
        need it -> the filtered (h, w, 3) frame, with return_variance the filtered (h, w) variance as well."""
        params = params or DenoiseParams()
        n = self.width * self.height
        arrays = []
        for name, a, size in (("rgb", rgb, 3 * n), ("var", var, n), ("albedo", albedo, 3 * n), ("normal", normal, 3 * n), ("depth", depth, 3 * n)):
            if a is None:
                if name == "rgb":
                    raise ValueError("denoise: rgb is required")
                arrays.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != size:
                raise ValueError(f"denoise: {name} has {a.size} values, the frame needs {size}")
            arrays.append(a)
        out = np.empty((self.height, self.width, 3), dtype=np.float64)
        out_var = np.empty((self.height, self.width), dtype=np.float64) if return_variance else None
        _lib.check(_lib.load().rpt_denoise(self._h, C.byref(params.desc()), *[_vp(a) if a is not None else None for a in arrays],
                                           _vp(out), _vp(out_var) if return_variance else None))
        return (out, out_var) if return_variance else out

    def denoise_device(self, d_rgb, d_var, d_albedo, d_normal, d_depth, d_out, d_out_var=0, params=None, stream_ptr=0):
        """Asynchronous variant: device pointers (0 / None: a null plane), enqueued on stream_ptr."""
        params = params or DenoiseParams()
        _lib.check(_lib.load().rpt_denoise_device(
            self._h, C.byref(params.desc()), *[C.c_void_p(p or None) for p in (d_rgb, d_var, d_albedo, d_normal, d_depth, d_out, d_out_var)],
            C.c_void_p(stream_ptr)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rpt_denoiser_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ guided upsampling (rpt_upsample*, an addition)
class UpsampleParams:
    """rpt_upsample_params: scale s in {2, 3, 4}, radius r in {1, 2} (2 r taps per axis); a term is on iff its sigma > 0.  The
    defaults are those of tools/upsample_quality.py on the oracle's renders ("Guided upsampling"); sigma_depth
    is off because it is in scene units per low-resolution pixel and no default is right for every scene.  On that grid
    sigma_normal = 1 gives the figures of the term switched off at radius 1: it is the loosest setting that still has the term on.
    Warning: demodulate=True can do worse than plain s x s replication on scenes whose materials have an albedo channel of 0
    (saturated colours, black backgrounds): at an edge where the channel is 0 on one side only, the pixel is remodulated with 1
    instead of 0 (cornell: RMS 26.27 levels against replication's 15.75, 14.62 with the id match alone at sigma_normal 0.5).  Pass demodulate=False there."""
    DEMODULATE, MATCH_ID = 1, 2

    def __init__(self, scale=2, radius=1, demodulate=True, match_id=True, sigma_normal=1.0, sigma_depth=0.0):
        self.scale, self.radius = int(scale), int(radius)
        self.demodulate, self.match_id = bool(demodulate), bool(match_id)
        self.sigma_normal, self.sigma_depth = float(sigma_normal), float(sigma_depth)

    @property
    def flags(self):
        return (self.DEMODULATE if self.demodulate else 0) | (self.MATCH_ID if self.match_id else 0)

    def desc(self):
        return _lib.UpsampleParams(self.scale, self.radius, self.flags, 0, self.sigma_normal, self.sigma_depth)


def upsample(lo_rgb, lo_var=None, lo_albedo=None, lo_normal=None, lo_depth=None, hi_albedo=None, hi_normal=None, hi_depth=None, params=None,
             return_variance=False, device=0):
    """rpt_upsample.  Host arrays: lo_rgb (h, w, 3), lo_var (h, w), the low-resolution planes (h, w, 3), the full-resolution ones
    (s h, s w, 3); any but lo_rgb may be None where `params` does not need it -> the (s h, s w, 3) frame, with return_variance the
    (s h, s w) variance as well."""
    params = params or UpsampleParams()
    lo_rgb = np.ascontiguousarray(lo_rgb, dtype=np.float64)
    if lo_rgb.ndim != 3 or lo_rgb.shape[2] != 3:
        raise ValueError("upsample: lo_rgb must be (h, w, 3)")
    h, w = lo_rgb.shape[:2]
    n, s = w * h, params.scale
    if s not in (2, 3, 4):
        raise ValueError("upsample: scale must be 2, 3 or 4")
    arrays = [lo_rgb]
    for name, a, size in (("lo_var", lo_var, n), ("lo_albedo", lo_albedo, 3 * n), ("lo_normal", lo_normal, 3 * n), ("lo_depth", lo_depth, 3 * n),
                          ("hi_albedo", hi_albedo, 3 * n * s * s), ("hi_normal", hi_normal, 3 * n * s * s), ("hi_depth", hi_depth, 3 * n * s * s)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != size:
                raise ValueError(f"upsample: {name} has {a.size} values, the frame needs {size}")
        arrays.append(a)
    out = np.empty((s * h, s * w, 3), dtype=np.float64)
    out_var = np.empty((s * h, s * w), dtype=np.float64) if return_variance else None
    _lib.check(_lib.load().rpt_upsample(int(device), C.byref(params.desc()), w, h, *[_vp(a) if a is not None else None for a in arrays],
                                        _vp(out), _vp(out_var) if return_variance else None))
    return (out, out_var) if return_variance else out


def upsample_device(lo_width, lo_height, d_lo_rgb, d_lo_var, d_lo_albedo, d_lo_normal, d_lo_depth, d_hi_albedo, d_hi_normal, d_hi_depth,
                    d_out, d_out_var=0, params=None, stream_ptr=0):
    """rpt_upsample_device: asynchronous and stateless, device pointers on the current device (0 / None: a null plane), enqueued on
    stream_ptr."""
    params = params or UpsampleParams()
    _lib.check(_lib.load().rpt_upsample_device(
        C.byref(params.desc()), int(lo_width), int(lo_height),
        *[C.c_void_p(p or None) for p in (d_lo_rgb, d_lo_var, d_lo_albedo, d_lo_normal, d_lo_depth, d_hi_albedo, d_hi_normal, d_hi_depth,
                                          d_out, d_out_var)], C.c_void_p(stream_ptr)))


def image_bytes_device(d_rgb, width, height, stream_ptr=0):
    """rpt_image_bytes_device: color_bytes of a device plane of width*height*3 doubles, enqueued on stream_ptr and waited for ->
    (h, w, 3) uint8.  What ends a pipeline composed from device entry points."""
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("image_bytes_device: empty image")
    out = np.empty((height, width, 3), dtype=np.uint8)
    _lib.check(_lib.load().rpt_image_bytes_device(C.c_void_p(d_rgb or None), width, height, _vp(out), C.c_void_p(stream_ptr)))
    return out


# ------------------------------------------------------------------ temporal accumulation (rpt_temporal_*, an addition)
class TemporalParams:
    """rpt_temporal_params.  max_history 1..4096 caps the history length (1: no reuse); a test is on iff its tolerance > 0:
    depth_tol relative, on squared distances, normal_tol on the distance of the normal planes.  clip=True sets RPT_TEMPORAL_CLIP:
    the history colour is clamped to the current frame's window around the pixel, with the accumulator's settings
    (TemporalAccumulator.set_clip)."""
    MATCH_ID = 1
    CLIP = 2

    def __init__(self, max_history=16, match_id=True, depth_tol=0.1, normal_tol=0.5, clip=False):
        self.max_history, self.match_id, self.clip = int(max_history), bool(match_id), bool(clip)
        self.depth_tol, self.normal_tol = float(depth_tol), float(normal_tol)
        if not 1 <= self.max_history <= 4096:
            raise ValueError("TemporalParams: max_history must be 1..4096")
        for t in (self.depth_tol, self.normal_tol):
            if not t >= 0.0 or math.isinf(t):
                raise ValueError("TemporalParams: a tolerance must be finite and >= 0")

    @property
    def flags(self):
        return (self.MATCH_ID if self.match_id else 0) | (self.CLIP if self.clip else 0)

    def desc(self):
        return _lib.TemporalParams(self.max_history, self.flags, self.depth_tol, self.normal_tol)


def temporal_camera_record(camera):
    """rpt_temporal_camera_record -> the 13 doubles eye, direction, right, up, d that the accumulation takes (a host function)."""
    out = np.empty(13, dtype=np.float64)
    _lib.check(_lib.load().rpt_temporal_camera_record(C.byref(camera_desc(camera, _lib.CameraDesc)), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


MOTION_DOUBLES = 24


def temporal_motion_record(cur, prev):
    """rpt_temporal_motion_record -> the 24 doubles A (3 x 4), G (3 x 3), three zeros of an object whose object-to-world matrices
    are `cur` in the current and `prev` in the previous frame (4 x 4, as Shape.matrix() gives them; None: the identity).  A host
    function."""
    mats = [np.ascontiguousarray(np.eye(4) if m is None else m, dtype=np.float64).reshape(16) for m in (cur, prev)]
    out = np.empty(MOTION_DOUBLES, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().rpt_temporal_motion_record(mats[0].ctypes.data_as(dp), mats[1].ctypes.data_as(dp), out.ctypes.data_as(dp)))
    return out


class TemporalAccumulator:
    """rpt_temporal: the history of a frame sequence of one size on one device, and the accumulation of include/rpt_hip.h."""

    def __init__(self, width, height, device=0):
        self.width, self.height, self.device = int(width), int(height), int(device)
        if self.width <= 0 or self.height <= 0:
            raise ValueError("TemporalAccumulator: empty frame")
        self._h = _lib.load().rpt_temporal_create(self.device, self.width, self.height)
        if not self._h:
            _lib.check(-1)

    def accumulate(self, camera, rgb, var, normal, depth, params=None, return_variance=False, return_length=False):
        """Host arrays: rgb, normal, depth of (h, w, 3), var of (h, w); var may be None, normal is None iff params.normal_tol == 0
        -> the accumulated (h, w, 3) frame, then as asked its (h, w) variance and the (h, w) history lengths."""
        params = params or TemporalParams()
        n = self.width * self.height
        arrays = []
        for name, a, size in (("rgb", rgb, 3 * n), ("var", var, n), ("normal", normal, 3 * n), ("depth", depth, 3 * n)):
            if a is None:
                if name in ("rgb", "depth"):
                    raise ValueError(f"accumulate: {name} is required")
                arrays.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != size:
                raise ValueError(f"accumulate: {name} has {a.size} values, the frame needs {size}")
            arrays.append(a)
        out = np.empty((self.height, self.width, 3), dtype=np.float64)
        out_var = np.empty((self.height, self.width), dtype=np.float64) if return_variance else None
        out_len = np.empty((self.height, self.width), dtype=np.float64) if return_length else None
        _lib.check(_lib.load().rpt_temporal_accumulate(
            self._h, C.byref(params.desc()), C.byref(camera_desc(camera, _lib.CameraDesc)), *[_vp(a) if a is not None else None for a in arrays],
            _vp(out), _vp(out_var) if return_variance else None, _vp(out_len) if return_length else None))
        res = (out,) + ((out_var,) if return_variance else ()) + ((out_len,) if return_length else ())
        return res if len(res) > 1 else out

    def accumulate_device(self, camera, d_rgb, d_var, d_normal, d_depth, d_out, d_out_var=0, d_out_len=0, params=None, stream_ptr=0):
        """Asynchronous variant: device pointers (0 / None: a null plane), enqueued on stream_ptr."""
        params = params or TemporalParams()
        _lib.check(_lib.load().rpt_temporal_accumulate_device(
            self._h, C.byref(params.desc()), C.byref(camera_desc(camera, _lib.CameraDesc)),
            *[C.c_void_p(p or None) for p in (d_rgb, d_var, d_normal, d_depth, d_out, d_out_var, d_out_len)], C.c_void_p(stream_ptr)))

    # ---- the accumulation without its side effects, over a tile list (rpt_temporal_preview_device, an addition)
    @property
    def tiles(self):
        """(tiles_x, tiles_y): the frame in 32 x 32 tiles; a tile id is ty * tiles_x + tx."""
        return (self.width + 31) // 32, (self.height + 31) // 32

    def _tile_list(self, tiles, what):
        """`tiles`: None (every tile) or a sequence of distinct ids -> (what keeps the upload alive, pointer, count)."""
        if tiles is None:
            return None, None, 0
        import torch
        ids = np.ascontiguousarray(tiles, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= 1 << 32):
            raise ValueError(f"{what}: a tile id does not fit 32 bits")
        if np.unique(ids).size != ids.size:
            raise ValueError(f"{what}: a tile id is listed twice")
        if ids.size > self.tiles[0] * self.tiles[1]:
            raise ValueError(f"{what}: {ids.size} tiles listed, the frame has {self.tiles[0] * self.tiles[1]}")
        # (one spare entry: an empty list is still a list, not "every tile")
        d = torch.from_numpy(np.concatenate([ids.astype(np.uint32), np.zeros(1, np.uint32)]).view(np.int32)).to(f"cuda:{self.device}")
        return d, d.data_ptr(), int(ids.size)

    def preview_device(self, camera, d_rgb, d_var, d_normal, d_depth, d_out, d_out_var=0, d_out_len=0, params=None, d_tiles=0, n_tiles=0,
                       stream_ptr=0):
        """rpt_temporal_preview_device: what accumulate_device would write to its outputs in the listed tiles (d_tiles: a device
        array of n_tiles distinct uint32 ids; 0 with n_tiles 0: every tile), enqueued on stream_ptr.  Nothing of the accumulator
        changes: no history is written, frames stays, a pending motion table stays set."""
        params = params or TemporalParams()
        _lib.check(_lib.load().rpt_temporal_preview_device(
            self._h, C.byref(params.desc()), C.byref(camera_desc(camera, _lib.CameraDesc)),
            *[C.c_void_p(p or None) for p in (d_rgb, d_var, d_normal, d_depth, d_tiles)], int(n_tiles),
            *[C.c_void_p(p or None) for p in (d_out, d_out_var, d_out_len)], C.c_void_p(stream_ptr)))

    def preview(self, camera, rgb, var, normal, depth, params=None, tiles=None, fill=np.nan):
        """Host arrays as for accumulate -> (out, out_var, out_len) as accumulate(..., return_variance=True, return_length=True)
        would return them in the tiles of `tiles` (None: every tile); pixels of other tiles hold `fill`.  Synchronous."""
        params = params or TemporalParams()
        n = self.width * self.height
        dev = []
        for name, a, size in (("rgb", rgb, 3 * n), ("var", var, n), ("normal", normal, 3 * n), ("depth", depth, 3 * n)):
            if a is None:
                if name in ("rgb", "depth"):
                    raise ValueError(f"preview: {name} is required")
                dev.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != size:
                raise ValueError(f"preview: {name} has {a.size} values, the frame needs {size}")
            dev.append(_device_copy(a, self.device))
        keep, d_tiles, n_tiles = self._tile_list(tiles, "preview")
        out = _device_copy(np.full(5 * n, fill, dtype=np.float64), self.device)
        _sync(self.device)
        self.preview_device(camera, *[d.data_ptr() if d is not None else 0 for d in dev], out.data_ptr(), out.data_ptr() + 24 * n,
                            out.data_ptr() + 32 * n, params, d_tiles, n_tiles)
        _sync(self.device)
        host = out.cpu().numpy()
        return (host[:3 * n].reshape(self.height, self.width, 3).copy(), host[3 * n:4 * n].reshape(self.height, self.width).copy(),
                host[4 * n:].reshape(self.height, self.width).copy())

    def tile_errors(self, rgb, var, floor, tiles=None, fill=np.nan):
        """rpt_temporal_tile_errors_device -> (tiles_y, tiles_x) float64: DeviceBuffer.tile_errors' error with the pixel's mean and the
        variance of that mean taken from the (h, w, 3) and (h, w) planes, for the tiles of `tiles` (None: every tile); the entries
        of other tiles hold `fill`."""
        floor = float(floor)
        if not (floor > 0.0) or math.isinf(floor):
            raise ValueError("tile_errors: floor must be finite and > 0")
        n = self.width * self.height
        rgb, var = np.ascontiguousarray(rgb, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
        if rgb.size != 3 * n or var.size != n:
            raise ValueError(f"tile_errors: the planes are not {self.height} x {self.width} x 3 and {self.height} x {self.width}")
        tx, ty = self.tiles
        d_rgb, d_var = _device_copy(rgb, self.device), _device_copy(var, self.device)
        d_err = _device_copy(np.full(tx * ty, fill, dtype=np.float64), self.device)
        keep, d_tiles, n_tiles = self._tile_list(tiles, "tile_errors")
        _sync(self.device)
        _lib.check(_lib.load().rpt_temporal_tile_errors_device(self._h, C.c_void_p(d_rgb.data_ptr()), C.c_void_p(d_var.data_ptr()), floor,
                                                               C.c_void_p(d_tiles), n_tiles, C.c_void_p(d_err.data_ptr()), None))
        _sync(self.device)
        return d_err.cpu().numpy().reshape(ty, tx).copy()

    def set_motion(self, records):
        """rpt_temporal_set_motion: an (n, 24) array of motion records (temporal_motion_record), record i for the object with id
        i + 1, or None to clear.  One-shot: the next accumulate, accumulate_device or temporal_image consumes the table."""
        if records is None:
            _lib.check(_lib.load().rpt_temporal_set_motion(self._h, None, 0))
            return
        records = np.ascontiguousarray(records, dtype=np.float64)
        if records.ndim != 2 or records.shape[1] != MOTION_DOUBLES:
            raise ValueError("set_motion: records must be an (n, 24) array")
        _lib.check(_lib.load().rpt_temporal_set_motion(self._h, records.ctypes.data_as(C.POINTER(C.c_double)), records.shape[0]))

    def set_motion_device(self, ptr, n):
        """rpt_temporal_set_motion_device: a device table of n records that the caller owns and leaves unchanged until the
        consuming call's work is done.  One-shot, like set_motion."""
        _lib.check(_lib.load().rpt_temporal_set_motion_device(self._h, C.c_void_p(ptr or None), int(n)))

    def set_clip(self, radius=1, gamma=0.5, history=1):
        """rpt_temporal_set_clip: the settings of TemporalParams(clip=True) -- the window's radius 1..3, the width gamma >= 0 of the
        clamp in standard deviations of the window, and the history length 0..4096 a clipped pixel keeps (0: all of it).  A host
        setting that persists over calls and over reset(); without clip=True it is ignored."""
        _lib.check(_lib.load().rpt_temporal_set_clip(self._h, int(radius), float(gamma), int(history)))

    def reset(self):
        """Forget the history (and a motion table that was not consumed): the next frame passes through."""
        _lib.check(_lib.load().rpt_temporal_reset(self._h))

    @property
    def frames(self):
        """Frames accumulated since the creation or the last reset."""
        n = C.c_uint32()
        _lib.check(_lib.load().rpt_temporal_frames(self._h, C.byref(n)))
        return int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rpt_temporal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ renderer.rs
class Renderer:
    def __init__(self, scene, camera):
        self.scene, self.camera = scene, camera
        self.width_, self.height_ = 800, 600
        self.exposure_value_ = 0.0
        self.filter_ = Filter.default()
        self.stepsize_ = 0.0
        self.max_bounces_ = 0
        self.num_samples_ = 1
        self.gather_size_, self.gather_size_volume_, self.watts_ = 50, 50, 100.0
        self.seed_ = 0
        self.shard_rank_, self.shard_count_ = 0, 1
        self.device_ = 0
        self._sample_offset = 0

    @staticmethod
    def new(scene, camera):
        return Renderer(scene, camera)

    def width(self, v):
        self.width_ = int(v); return self

    def height(self, v):
        self.height_ = int(v); return self

    def exposure_value(self, v):
        self.exposure_value_ = float(v); return self

    def stepsize(self, v):
        self.stepsize_ = float(v); return self  # stored, never read (renderer.rs:43, 96-99)

    def filter(self, f):
        self.filter_ = f; return self

    def max_bounces(self, v):
        self.max_bounces_ = int(v); return self

    def num_samples(self, v):
        self.num_samples_ = int(v); return self

    def gather_size(self, v):
        self.gather_size_ = int(v); return self

    def gather_size_volume(self, v):
        self.gather_size_volume_ = int(v); return self

    def watts(self, v):
        self.watts_ = float(v); return self

    # additions (documented deviations)
    def seed(self, v):
        self.seed_ = int(v) & 0xFFFFFFFFFFFFFFFF; return self

    def shard(self, rank, count):
        self.shard_rank_, self.shard_count_ = int(rank), int(count); return self

    def device(self, index):
        self.device_ = int(index); return self

    def _params(self):
        p = _lib.RenderParams()
        p.width, p.height = self.width_, self.height_
        p.exposure_value = self.exposure_value_
        p.max_bounces = self.max_bounces_
        p.shard_rank, p.shard_count = self.shard_rank_, self.shard_count_
        return p

    def sample_array(self, iterations):
        """Renderer::sample (renderer.rs:158-171) -> (h*w, 3) fp64 array of per-pixel means."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        out = np.empty((self.width_ * self.height_, 3), dtype=np.float64)
        _lib.check(lib.rpt_render_sample(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), int(iterations),
            C.c_uint64(self.seed_), self._sample_offset, out.ctypes.data_as(C.c_void_p)))
        self._sample_offset += int(iterations)
        return out

    def sample_device(self, iterations, d_out_ptr, stream_ptr=0):
        """Asynchronous variant: d_out_ptr is a device pointer to width*height*3 doubles."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        _lib.check(lib.rpt_render_sample_device(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), int(iterations),
            C.c_uint64(self.seed_), self._sample_offset, C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))
        self._sample_offset += int(iterations)

    # Tile-list renders (rpt_render_sample_tiles*, an addition): the listed 32 x 32 tiles alone, the bits a full render puts there.
    def _check_tiles(self, what):
        if self.shard_count_ != 1:
            raise ValueError(f"{what}: a tile-list render is not sharded")
        if self.width_ <= 0 or self.height_ <= 0:
            raise ValueError(f"{what}: empty frame")
        return ((self.width_ + 31) // 32) * ((self.height_ + 31) // 32)

    def sample_tiles_device(self, iterations, d_tiles_ptr, n_tiles, d_out_ptr, stream_ptr=0):
        """d_tiles_ptr: device array of n_tiles distinct uint32 tile ids (ty * tiles_x + tx); d_out_ptr: device frame of
        width*height*3 doubles, written in the listed tiles only.  Advances the sample offset like sample_device."""
        total, n_tiles = self._check_tiles("sample_tiles_device"), int(n_tiles)
        if n_tiles < 0 or n_tiles > total:
            raise ValueError(f"sample_tiles_device: {n_tiles} tiles listed, the frame has {total}")
        if not d_out_ptr or (n_tiles and not d_tiles_ptr):
            raise ValueError("sample_tiles_device: null pointer")
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        _lib.check(lib.rpt_render_sample_tiles_device(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), int(iterations),
            C.c_uint64(self.seed_), self._sample_offset, C.c_void_p(d_tiles_ptr or None), n_tiles, C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))
        self._sample_offset += int(iterations)

    def sample_tiles_array(self, iterations, tiles, out):
        """Host variant: `tiles` a sequence of distinct tile ids, `out` a C-contiguous float64 array of width*height*3 values that is
        updated in place in the listed tiles and keeps its values everywhere else -> out."""
        total = self._check_tiles("sample_tiles_array")
        tiles = np.ascontiguousarray(tiles, dtype=np.int64).reshape(-1)
        if tiles.size and (tiles.min() < 0 or tiles.max() >= total):
            raise ValueError(f"sample_tiles_array: tile id outside 0..{total - 1}")
        if np.unique(tiles).size != tiles.size:
            raise ValueError("sample_tiles_array: a tile id is listed twice")
        if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable
                and out.size == self.width_ * self.height_ * 3):
            raise ValueError(f"sample_tiles_array: out must be a writable C-contiguous float64 array of {self.width_ * self.height_ * 3} values")
        ids = tiles.astype(np.uint32)
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        _lib.check(lib.rpt_render_sample_tiles(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), int(iterations),
            C.c_uint64(self.seed_), self._sample_offset, _vp(ids), ids.size, _vp(out)))
        self._sample_offset += int(iterations)
        return out

    def sample_adaptive(self, params, buffer):
        """rpt_render_adaptive (an addition) into an empty DeviceBuffer: params.min_batches full frames of params.spp_per_batch
        samples, then one more batch per round for the tiles whose error is still above the threshold, at most params.max_batches.
        A pixel of a tile that ends with n batches holds the sums n full-frame sample() calls would have put there.
        -> (rounds that rendered a tile list, tile-batches rendered, tiles at max_batches, tiles)."""
        if not isinstance(params, AdaptiveParams):
            raise ValueError("sample_adaptive: params must be an AdaptiveParams")
        if not isinstance(buffer, DeviceBuffer):
            raise ValueError("sample_adaptive: the buffer must be a DeviceBuffer")
        if self.shard_count_ != 1:
            raise ValueError("sample_adaptive: an adaptive render is not sharded")
        stats = (C.c_uint64 * 4)()
        _lib.check(_lib.load().rpt_render_adaptive(
            self.scene._commit(self.device_), C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()),
            C.byref(params.desc()), C.c_uint64(self.seed_), buffer._h, stats))
        return tuple(int(v) for v in stats)

    def sample_adaptive_temporal(self, params, buffer, accumulator, camera_planes, temporal=None, sample_offset=None):
        """rpt_render_adaptive_temporal (an addition) into an empty DeviceBuffer: sample_adaptive with a tile's error taken from the
        preview of `accumulator`'s accumulation of the frame so far, so that params.threshold is the relative standard error of the
        frame that is shown and tiles that their history carries stop early.  `camera_planes`: a dict with "depth" and, where
        temporal.normal_tol > 0, "normal", as DeviceBuffer.temporal_image takes them.  Batch k uses the samples at
        sample_offset + k * spp_per_batch (sample_offset None: the renderer's, which is advanced by max_batches * spp_per_batch).
        Nothing is accumulated: DeviceBuffer.temporal_image finishes the frame.  -> sample_adaptive's four numbers."""
        if not isinstance(params, AdaptiveParams):
            raise ValueError("sample_adaptive_temporal: params must be an AdaptiveParams")
        if not isinstance(buffer, DeviceBuffer):
            raise ValueError("sample_adaptive_temporal: the buffer must be a DeviceBuffer")
        if not isinstance(accumulator, TemporalAccumulator):
            raise ValueError("sample_adaptive_temporal: the accumulator must be a TemporalAccumulator")
        if temporal is not None and not isinstance(temporal, TemporalParams):
            raise ValueError("sample_adaptive_temporal: temporal must be a TemporalParams or None")
        if self.shard_count_ != 1:
            raise ValueError("sample_adaptive_temporal: an adaptive render is not sharded")
        temporal = temporal or TemporalParams()
        offset = self._sample_offset if sample_offset is None else int(sample_offset)
        if offset < 0 or offset + params.max_batches * params.spp_per_batch >= 1 << 32:
            raise ValueError("sample_adaptive_temporal: sample_offset + max_batches * spp_per_batch must fit 32 bits")
        keep, ptrs = buffer._plane_pointers({k: v for k, v in camera_planes.items() if k != "albedo"}, "sample_adaptive_temporal")
        stats = (C.c_uint64 * 4)()
        _lib.check(_lib.load().rpt_render_adaptive_temporal(
            self.scene._commit(self.device_), C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()),
            C.byref(params.desc()), C.c_uint64(self.seed_), offset, buffer._h, accumulator._h, C.byref(temporal.desc()), ptrs[1], ptrs[2],
            stats))
        if sample_offset is None:
            self._sample_offset += params.max_batches * params.spp_per_batch
        return tuple(int(v) for v in stats)

    def render_adaptive(self, params=None, denoise=None):
        """sample_adaptive into a fresh DeviceBuffer -> (image, tile_batches): (h, w, 3) uint8 and the (tiles_y, tiles_x) batches each
        tile ended with.  The image is DeviceBuffer.image() (filter() applies), or with denoise=DenoiseParams(..)
        DeviceBuffer.denoised_image() over the feature planes of the first min_batches * spp_per_batch samples (filter() is not
        applied).  num_samples() is not read."""
        params = params or AdaptiveParams()
        if not isinstance(params, AdaptiveParams):
            raise ValueError("render_adaptive: params must be an AdaptiveParams")
        if denoise is not None and not isinstance(denoise, DenoiseParams):
            raise ValueError("render_adaptive: denoise must be a DenoiseParams or None")
        if self.shard_count_ != 1:
            raise ValueError("render_adaptive: an adaptive render is not sharded")
        buffer = DeviceBuffer(self.width_, self.height_, None if denoise is not None else self.filter_, self.device_)
        if denoise is not None:
            n = self.width_ * self.height_ * 3
            planes = _device_zeros(3 * n, self.device_)
            _sync(self.device_)
            ptrs = [planes.data_ptr() + 8 * n * k for k in range(3)]
            self.features_device(params.min_batches * params.spp_per_batch, *ptrs, sample_offset=0)
        self.sample_adaptive(params, buffer)
        counts = buffer.tile_batches()
        if denoise is not None:
            denoiser = Denoiser(self.width_, self.height_, self.device_)
            img = buffer.denoised_image(denoiser, dict(zip(("albedo", "normal", "depth"), ptrs)), denoise)
            denoiser.close()
        else:
            img = buffer.image()
        buffer.close()
        return img, counts

    # First-hit feature planes (rpt_render_features*, an addition): of the camera samples that the NEXT sample call of this renderer
    # traces -- same seed, same sample offset; the offset is not advanced (sample_offset=...: another one).
    def features_array(self, iterations, albedo=True, normal=True, depth=True, sample_offset=None):
        """-> dict of the requested planes, (h, w, 3) float64 each: "albedo" (mean Material::color of the first hit, the environment's
        colour on a miss), "normal" (mean normal, 0 on a miss, not renormalised), "depth" (mean hit distance over all samples,
        coverage, object index + 1 of the first sample or 0).  Honours seed(), shard() and device() like sample_array."""
        want = {"albedo": bool(albedo), "normal": bool(normal), "depth": bool(depth)}
        if not any(want.values()):
            raise ValueError("features_array: no plane requested")
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        out = {k: np.empty((self.height_, self.width_, 3), dtype=np.float64) for k, v in want.items() if v}
        _lib.check(lib.rpt_render_features(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), int(iterations),
            C.c_uint64(self.seed_), self._sample_offset if sample_offset is None else int(sample_offset),
            *[_vp(out[k]) if k in out else None for k in ("albedo", "normal", "depth")]))
        return out

    def features_device(self, iterations, d_albedo, d_normal, d_depth, stream_ptr=0, sample_offset=None):
        """Asynchronous variant: device pointers to width*height*3 doubles each (0 / None: the plane is not computed)."""
        if not (d_albedo or d_normal or d_depth):
            raise ValueError("features_device: no plane requested")
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        _lib.check(lib.rpt_render_features_device(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), int(iterations),
            C.c_uint64(self.seed_), self._sample_offset if sample_offset is None else int(sample_offset),
            C.c_void_p(d_albedo or None), C.c_void_p(d_normal or None), C.c_void_p(d_depth or None), C.c_void_p(stream_ptr)))

    def sample(self, iterations, buffer):
        """Renderer::sample (renderer.rs:158-171).  A DeviceBuffer receives the batch on the GPU."""
        if isinstance(buffer, DeviceBuffer) and self.shard_count_ == 1:
            _lib.check(_lib.load().rpt_render_into_buffer(
                self.scene._commit(self.device_), C.byref(camera_desc(self.camera, _lib.CameraDesc)),
                C.byref(self._params()), int(iterations), C.c_uint64(self.seed_), self._sample_offset, buffer._h))
            self._sample_offset += int(iterations)
        else:
            buffer.add_samples(self.sample_array(iterations))

    def render(self):
        """renderer.rs:137-141 -> (h, w, 3) uint8 image."""
        buffer = DeviceBuffer(self.width_, self.height_, self.filter_, self.device_)
        self._sample_offset = 0
        self.sample(self.num_samples_, buffer)
        return buffer.image()

    def render_denoised(self, batches=4, params=None):
        """An addition: num_samples in `batches` batches (at least 2; the first num_samples % batches of them one sample longer) into
        a DeviceBuffer, the feature planes of the same num_samples camera samples, then DeviceBuffer.denoised_image: the per-pixel
        mean and the variance of that mean, the a-trous filter, color_bytes -> (h, w, 3) uint8.  The frame, the planes and the
        filter stay on the device; filter() is not applied.  Not for sharded renders (rank 0 filters the assembled frame)."""
        batches = int(batches)
        if batches < 2:
            raise ValueError("render_denoised: the variance of the mean needs at least 2 batches")
        if self.num_samples_ < batches:
            raise ValueError("render_denoised: num_samples must be at least the number of batches")
        if self.shard_count_ != 1:
            raise ValueError("render_denoised: a sharded frame is assembled first; rank 0 filters it")
        buffer = DeviceBuffer(self.width_, self.height_, None, self.device_)
        denoiser = Denoiser(self.width_, self.height_, self.device_)
        n = self.width_ * self.height_ * 3
        planes = _device_zeros(3 * n, self.device_)
        _sync(self.device_)
        ptrs = [planes.data_ptr() + 8 * n * k for k in range(3)]
        self.features_device(self.num_samples_, *ptrs, sample_offset=0)
        self._sample_offset = 0
        base, extra = divmod(self.num_samples_, batches)
        for k in range(batches):
            self.sample(base + (1 if k < extra else 0), buffer)
        img = buffer.denoised_image(denoiser, dict(zip(("albedo", "normal", "depth"), ptrs)), params)
        denoiser.close()
        buffer.close()
        return img

    def _low(self, scale, what):
        """This renderer at 1 / scale of its size: the same scene, camera, seed and settings (the reference's pixel-to-ray map is
        scale-consistent: a low-resolution pixel integrates over scale x scale full-resolution ones)."""
        if scale not in (2, 3, 4):
            raise ValueError(f"{what}: scale must be 2, 3 or 4")
        if self.width_ % scale or self.height_ % scale or self.width_ < scale or self.height_ < scale:
            raise ValueError(f"{what}: width and height must be multiples of the scale {scale}")
        import copy
        lo = copy.copy(self)
        lo.width_, lo.height_ = self.width_ // scale, self.height_ // scale
        return lo

    def render_upsampled(self, params=None, batches=4, denoise=None, guide_samples=1):
        """An addition: the frame rendered at (width / s, height / s) and rebuilt at full size.  num_samples in `batches` batches
        (as render_denoised) at the low resolution with the same camera into a DeviceBuffer, the low-resolution feature planes of
        the same camera samples, the full-resolution planes of `guide_samples` samples, then DeviceBuffer.upsampled_image
        (`params`: an UpsampleParams or None for the defaults; denoise=DenoiseParams(..): the a-trous filter at the low resolution
        first) -> (h, w, 3) uint8.  width and height must be multiples of params.scale.  Everything but the bytes stays on the
        device; filter() is not applied.  Not for sharded renders."""
        params = params or UpsampleParams()
        if not isinstance(params, UpsampleParams):
            raise ValueError("render_upsampled: params must be an UpsampleParams or None")
        if denoise is not None and not isinstance(denoise, DenoiseParams):
            raise ValueError("render_upsampled: denoise must be a DenoiseParams or None")
        batches, guide_samples = int(batches), int(guide_samples)
        if batches < 2:
            raise ValueError("render_upsampled: the variance of the mean needs at least 2 batches")
        if self.num_samples_ < batches:
            raise ValueError("render_upsampled: num_samples must be at least the number of batches")
        if guide_samples < 1:
            raise ValueError("render_upsampled: guide_samples must be at least 1")
        if self.shard_count_ != 1:
            raise ValueError("render_upsampled: a sharded frame is assembled first; rank 0 upsamples it")
        lo = self._low(params.scale, "render_upsampled")
        buffer, denoiser = DeviceBuffer(lo.width_, lo.height_, None, self.device_), None
        try:
            if denoise is not None:
                denoiser = Denoiser(lo.width_, lo.height_, self.device_)
            n, big = lo.width_ * lo.height_ * 3, self.width_ * self.height_ * 3
            planes = _device_zeros(3 * n + 3 * big, self.device_)
            _sync(self.device_)
            ptrs = [planes.data_ptr() + 8 * n * k for k in range(3)]
            hi_ptrs = [planes.data_ptr() + 8 * (3 * n + big * k) for k in range(3)]
            lo.features_device(self.num_samples_, *ptrs, sample_offset=0)
            self.features_device(guide_samples, *hi_ptrs, sample_offset=0)
            lo._sample_offset = 0
            base, extra = divmod(self.num_samples_, batches)
            for k in range(batches):
                lo.sample(base + (1 if k < extra else 0), buffer)
            names = ("albedo", "normal", "depth")
            return buffer.upsampled_image(dict(zip(names, ptrs)), dict(zip(names, hi_ptrs)), params, denoiser, denoise)
        finally:
            if denoiser is not None:
                denoiser.close()
            buffer.close()

    def _upsampled_sequence(self, cameras, batches, temporal, denoise, scenes, upsample, guide_samples):
        """render_sequence with upsample=: composed from the device entry points on the default stream."""
        lo = self._low(upsample.scale, "render_sequence")
        accumulator, denoiser = TemporalAccumulator(self.width_, self.height_, self.device_), None
        own, own_scene = self.camera, self.scene
        try:
            if denoise is not None:
                denoiser = Denoiser(self.width_, self.height_, self.device_)
            n, big = lo.width_ * lo.height_, self.width_ * self.height_
            # low resolution: mean 3 n, variance n, planes 9 n; full resolution: planes 9, upsampled 3 + 1, accumulated 3 + 1, filtered 3
            mem = _device_zeros(13 * n + 20 * big, self.device_)
            _sync(self.device_)
            at = lambda k: mem.data_ptr() + 8 * k  # noqa: E731
            mean, var = at(0), at(3 * n)
            ptrs = [at(4 * n + 3 * n * k) for k in range(3)]
            hi_ptrs = [at(13 * n + 3 * big * k) for k in range(3)]
            up, up_var, acc, acc_var, out = (at(13 * n + big * k) for k in (9, 12, 13, 16, 17))
            base, extra = divmod(self.num_samples_, batches)
            for f, cam in enumerate(cameras):
                self.camera = lo.camera = cam
                if scenes is not None:
                    self.scene = lo.scene = scenes[f]
                    if f > 0:
                        accumulator.set_motion(np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix())
                                                         for c, p in zip(scenes[f].objects, scenes[f - 1].objects)])
                                               if scenes[f].objects else None)
                buffer = DeviceBuffer(lo.width_, lo.height_, None, self.device_)
                try:
                    lo.features_device(self.num_samples_, *ptrs, sample_offset=f * self.num_samples_)
                    self.features_device(guide_samples, *hi_ptrs, sample_offset=f * self.num_samples_)
                    lo._sample_offset = f * self.num_samples_
                    for k in range(batches):
                        lo.sample(base + (1 if k < extra else 0), buffer)
                    _sync(self.device_)                          # batches and planes may have been written on other streams
                    buffer.mean_device(mean, var)
                    _sync(self.device_)                          # (the buffer goes away below: its sums have been read)
                finally:
                    buffer.close()
                upsample_device(lo.width_, lo.height_, mean, var, *ptrs, *hi_ptrs, up, up_var, params=upsample)
                accumulator.accumulate_device(cam, up, up_var, hi_ptrs[1] if temporal.normal_tol > 0.0 else 0, hi_ptrs[2], acc, acc_var,
                                              params=temporal)
                last = acc
                if denoiser is not None:
                    denoiser.denoise_device(acc, acc_var, *hi_ptrs, out, params=denoise)
                    last = out
                img = image_bytes_device(last, self.width_, self.height_)
                self.camera, self.scene = own, own_scene
                yield img
        finally:
            self.camera, self.scene = own, own_scene
            accumulator.close()
            if denoiser is not None:
                denoiser.close()

    def render_sequence(self, cameras, batches=4, temporal=None, denoise=None, scenes=None, adaptive=None, return_tile_batches=False,
                        upsample=None, guide_samples=1, live=None):
        """An addition: a generator of one (h, w, 3) uint8 frame per camera of `cameras`, for a camera that moves over this scene
        or, with `scenes` (one Scene per camera, as the reference builds one per frame: the same number of objects with the same
        base shape kinds in the same order, else ValueError), over objects that move: frame f renders scenes[f], committed when its
        turn comes, and for f > 0 the accumulation gets the motion table built by temporal_motion_record from
        objects[i].shape.matrix() of scenes[f] and scenes[f - 1]; self.scene is left as it was.
        Frame f renders num_samples in `batches` batches (as render_denoised) at the sample offsets f * num_samples .. (fresh random
        streams per frame) into a DeviceBuffer, the feature planes of the same camera samples, then DeviceBuffer.temporal_image
        with one TemporalAccumulator for the sequence: mean and variance, accumulation over the previous frames (`temporal`: a
        TemporalParams or None for the defaults), with denoise=DenoiseParams(..) the a-trous filter, color_bytes.  Everything but
        the bytes stays on the device; filter() is not applied; self.camera is left as it was.  Not for sharded renders.
        With adaptive=AdaptiveParams(..) frame f is sampled by sample_adaptive_temporal against the sequence's accumulator instead:
        its batches at the sample offsets f * max_batches * spp_per_batch .., the feature planes those of the first
        min_batches * spp_per_batch samples at that offset (as render_adaptive takes them), the motion table set before the loop
        and consumed by temporal_image after it; num_samples and `batches` are not read.  With return_tile_batches=True (adaptive
        only) each frame comes as (image, tile_batches), the (tiles_y, tiles_x) batches its tiles ended with.
        With upsample=UpsampleParams(..) frame f is rendered at (width / s, height / s) (width and height multiples of s, else
        ValueError): its low-resolution mean and variance are upsampled under the low-resolution planes of the same camera samples
        and the full-resolution planes of `guide_samples` samples, then accumulate_device, the optional filter and
        image_bytes_device run at full resolution, where the depth and normal planes and the motion table are.  Not together
        with `adaptive` (ValueError).
        With live=mover (not together with `scenes` or `upsample`: ValueError) the objects of this renderer's own scene move on the
        device: mover.scene is this renderer's scene (else ValueError); before frame f > 0 the renderer calls mover.step(f), which moves the committed scene's spheres
        (Scene.move_spheres_device) and returns the device address of the move's motion table, len(scene.objects) x 24 doubles
        (or 0 for none), which goes to TemporalAccumulator.set_motion_device.  scenes.marbles_live builds such a mover; nothing is
        read back and nothing is committed again."""
        if live is not None:
            if scenes is not None or upsample is not None:
                raise ValueError("render_sequence: live is not combined with scenes or upsample")
            if not callable(getattr(live, "step", None)):
                raise ValueError("render_sequence: live must have a step(frame) method")
            if getattr(live, "scene", None) is not self.scene:
                raise ValueError("render_sequence: live.scene must be this renderer's scene (the mover moves what is rendered, and its "
                                 "motion table has one row per object of that scene)")
        if upsample is not None:
            if not isinstance(upsample, UpsampleParams):
                raise ValueError("render_sequence: upsample must be an UpsampleParams or None")
            if adaptive is not None:
                raise ValueError("render_sequence: adaptive sampling is not combined with upsampling")
            if int(guide_samples) < 1:
                raise ValueError("render_sequence: guide_samples must be at least 1")
            self._low(upsample.scale, "render_sequence")
        if adaptive is not None and not isinstance(adaptive, AdaptiveParams):
            raise ValueError("render_sequence: adaptive must be an AdaptiveParams or None")
        if return_tile_batches and adaptive is None:
            raise ValueError("render_sequence: return_tile_batches needs adaptive")
        batches = int(batches)
        if adaptive is None:
            if batches < 2:
                raise ValueError("render_sequence: the variance of the mean needs at least 2 batches")
            if self.num_samples_ < batches:
                raise ValueError("render_sequence: num_samples must be at least the number of batches")
        if self.shard_count_ != 1:
            raise ValueError("render_sequence: a sharded frame is assembled first; rank 0 accumulates it")
        if temporal is not None and not isinstance(temporal, TemporalParams):
            raise ValueError("render_sequence: temporal must be a TemporalParams or None")
        if denoise is not None and not isinstance(denoise, DenoiseParams):
            raise ValueError("render_sequence: denoise must be a DenoiseParams or None")
        cameras = list(cameras)
        if adaptive is not None:
            if len(cameras) * adaptive.max_batches * adaptive.spp_per_batch >= 1 << 32:
                raise ValueError("render_sequence: frames * max_batches * spp_per_batch must fit 32 bits")
        elif len(cameras) * self.num_samples_ >= 1 << 32:
            raise ValueError("render_sequence: frames * num_samples must fit 32 bits")
        if scenes is not None:
            scenes = list(scenes)
            if len(scenes) != len(cameras):
                raise ValueError("render_sequence: scenes must hold one Scene per camera")
            if any(not isinstance(sc, Scene) for sc in scenes):
                raise ValueError("render_sequence: scenes must hold Scene objects")
            kinds = [[o.shape.base().KIND for o in sc.objects] for sc in scenes]
            if any(k != kinds[0] for k in kinds[1:]):
                raise ValueError("render_sequence: every scene must hold the same base shape kinds in the same order")
        if upsample is not None:
            return self._upsampled_sequence(cameras, batches, temporal or TemporalParams(), denoise, scenes, upsample, int(guide_samples))
        return self._render_sequence(cameras, batches, temporal or TemporalParams(), denoise, scenes, adaptive, bool(return_tile_batches), live)

    def _render_sequence(self, cameras, batches, temporal, denoise, scenes=None, adaptive=None, return_tile_batches=False, live=None):
        accumulator = TemporalAccumulator(self.width_, self.height_, self.device_)
        denoiser = Denoiser(self.width_, self.height_, self.device_) if denoise is not None else None
        n = self.width_ * self.height_ * 3
        planes = _device_zeros(3 * n, self.device_)
        _sync(self.device_)
        ptrs = [planes.data_ptr() + 8 * n * k for k in range(3)]
        base, extra = divmod(self.num_samples_, batches)
        own, own_scene = self.camera, self.scene
        try:
            for f, cam in enumerate(cameras):
                self.camera = cam
                if scenes is not None:
                    self.scene = scenes[f]
                    if f > 0:
                        accumulator.set_motion(np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix())
                                                         for c, p in zip(scenes[f].objects, scenes[f - 1].objects)])
                                               if scenes[f].objects else None)
                elif live is not None and f > 0:
                    table = live.step(f)
                    if table:
                        accumulator.set_motion_device(table, len(self.scene.objects))
                buffer = DeviceBuffer(self.width_, self.height_, None, self.device_)
                counts = None
                if adaptive is not None:
                    offset = f * adaptive.max_batches * adaptive.spp_per_batch
                    self.features_device(adaptive.min_batches * adaptive.spp_per_batch, *ptrs, sample_offset=offset)
                    self.sample_adaptive_temporal(adaptive, buffer, accumulator, {"normal": ptrs[1], "depth": ptrs[2]}, temporal, sample_offset=offset)
                    if return_tile_batches:
                        counts = buffer.tile_batches()
                else:
                    self.features_device(self.num_samples_, *ptrs, sample_offset=f * self.num_samples_)
                    self._sample_offset = f * self.num_samples_
                    for k in range(batches):
                        self.sample(base + (1 if k < extra else 0), buffer)
                img = buffer.temporal_image(accumulator, cam, dict(zip(("albedo", "normal", "depth"), ptrs)), temporal, denoiser, denoise)
                buffer.close()
                self.camera, self.scene = own, own_scene
                yield (img, counts) if return_tile_batches else img
        finally:
            self.camera, self.scene = own, own_scene
            accumulator.close()
            if denoiser is not None:
                denoiser.close()

    def iterative_render(self, callback_interval, callback):
        """renderer.rs:144-156."""
        buffer = DeviceBuffer(self.width_, self.height_, self.filter_, self.device_)
        self._sample_offset = 0
        iteration = 0
        while iteration < self.num_samples_:
            steps = min(self.num_samples_ - iteration, callback_interval)
            self.sample(steps, buffer)
            iteration += steps
            callback(iteration, buffer)

    def timing(self):
        """(render_ms, resolve_ms, grid_blocks) of the last call, from HIP events on its stream."""
        a, b, g = C.c_double(), C.c_double(), C.c_int32()
        _lib.check(_lib.load().rpt_get_timing(self.scene._handle, C.byref(a), C.byref(b), C.byref(g)))
        return a.value, b.value, g.value

    def timing_mean(self):
        """(mean render_ms, mean resolve_ms, launches) over the timed calls since the previous timing_mean();
        the calls themselves never wait for their events."""
        a, b, n = C.c_double(), C.c_double(), C.c_int32()
        _lib.check(_lib.load().rpt_get_timing_mean(self.scene._handle, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def chunking(self, iterations):
        """(samples per work item, work items per pixel) of this renderer's sample(iterations) calls: the scene's own
        "chunk_spp" option applies (rpt_scene_render_chunking), as in its renders."""
        c, n = C.c_uint32(), C.c_uint32()
        _lib.check(_lib.load().rpt_scene_render_chunking(self.scene._commit(self.device_), int(iterations), C.byref(c), C.byref(n)))
        return int(c.value), int(n.value)

    def scene_stats(self):
        """rpt_scene_stats of the committed scene (flattened-layout record counts and bytes)."""
        out = (C.c_uint64 * 16)()
        _lib.check(_lib.load().rpt_scene_stats(self.scene._commit(self.device_), out))
        names = ["spheres", "cubes", "planes", "tris", "aabbs", "rects", "bvh_tris", "bvh_nodes", "scan_bytes_per_ray",
                 "scene_bytes", "scene_bvh", "scene_bvh_prims", "instances", "shared_meshes", "shell_faces", "tree_depth"]
        return dict(zip(names, [int(v) for v in out]))

    # ---- photon mapping (src/photon.rs:631-720)
    PHOTON_MAP, PHOTON_POINT_BEAM, PHOTON_BEAM_BEAM = 0, 1, 2   # enum PhotonRenderKind

    def photon_map_build(self, photon_count, kind=1):
        """Shooting + map build of Renderer::photon_render (photon.rs:655-704) on the device."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        _lib.check(lib.rpt_photon_map_build(h, int(photon_count), int(kind), self.watts_, C.c_uint64(self.seed_)))
        out = (C.c_uint64 * 8)()
        _lib.check(lib.rpt_photon_map_stats(h, out))
        return {"surface": int(out[0]), "volume": int(out[1]), "shot": int(out[2]), "shoot_us": int(out[3]),
                "build_us": int(out[4]), "shoot_blocks": int(out[5]), "surface64_blocks": int(out[6])}

    def _photon_stats(self):
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().rpt_photon_map_stats(self.scene._handle, out))
        return {"surface": int(out[0]), "volume": int(out[1]), "shot": int(out[2]), "shoot_us": int(out[3]),
                "build_us": int(out[4]), "shoot_blocks": int(out[5]), "surface64_blocks": int(out[6])}

    def photon_shoot(self, photon_count, kind, shard_rank=0, shard_count=1):
        """rpt_photon_shoot: this rank's contiguous block of the shooting loop (photon.rs:656-690);
        returns (surface, volume) record counts.  The records stay on the device (photon_records)."""
        n = (C.c_uint64 * 2)()
        h = self.scene._commit(self.device_)
        _lib.check(_lib.load().rpt_photon_shoot(h, int(photon_count), int(kind), self.watts_, C.c_uint64(self.seed_),
                                                int(shard_rank), int(shard_count), n))
        return int(n[0]), int(n[1])

    def photon_records(self, which):
        """(device pointer, count) of the records of the last photon_shoot; 48 bytes each."""
        ptr, n = C.c_void_p(), C.c_uint64()
        _lib.check(_lib.load().rpt_photon_records(self.scene._handle, int(which), C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    def photon_map_from_records(self, photon_count, kind, d_surface, n_surface, d_volume, n_volume):
        """rpt_photon_map_from_records: build the maps from (gathered) device record arrays of 48 bytes per record: position, 0;
        direction, 0; power, 0 -- the volume records of kind 2 (beam x beam) are end, radius; start, 0; power, 0, and the beam's
        radius is read from the record."""
        h = self.scene._commit(self.device_)
        _lib.check(_lib.load().rpt_photon_map_from_records(h, int(photon_count), int(kind), C.c_void_p(d_surface),
                                                           int(n_surface), C.c_void_p(d_volume), int(n_volume)))
        return self._photon_stats()

    def photon_map_download(self, which):
        """Test hook: (n, 10) float32 photons in shooting order (position, direction, power, radius)."""
        lib = _lib.load()
        h = self.scene._handle
        out = (C.c_uint64 * 8)()
        _lib.check(lib.rpt_photon_map_stats(h, out))
        n = int(out[which])
        arr = np.zeros((n, 10), dtype=np.float32)
        _lib.check(lib.rpt_photon_map_download(h, which, arr.ctypes.data_as(C.c_void_p), n))
        return arr

    def photon_positions64(self):
        """Reference-epsilon mode: the surface photons' fp64 positions, (n, 3), in the order of photon_map_download(0)."""
        n = self._photon_stats()["surface"]
        out = np.zeros((n, 3), dtype=np.float64)
        _lib.check(_lib.load().rpt_debug_photon_positions64(self.scene._handle, out.ctypes.data_as(C.c_void_p), n))
        return out

    def photon_chain_counts(self, n):
        """Test hook (scene option "photon_keep_counts" = 1): (surface, volume) record counts of the n photons of the last shooting
        pass, u32, in shooting order."""
        out = []
        for which in (0, 1):
            a = np.zeros(int(n), dtype=np.uint32)
            _lib.check(_lib.load().rpt_debug_photon_chain_counts(self.scene._handle, which, a.ctypes.data_as(C.c_void_p), int(n)))
            out.append(a)
        return out[0], out[1]

    def photon_selections(self):
        """Reference-epsilon mode, test hook: the last camera pass's per-sample selections, (pixel slots, gather_size + 2, samples) u32."""
        lib = _lib.load()
        dims = (C.c_uint64 * 3)()
        _lib.check(lib.rpt_debug_photon_selections(self.scene._handle, None, 0, dims))
        out = np.zeros((int(dims[0]), int(dims[1]), int(dims[2])), dtype=np.uint32)
        _lib.check(lib.rpt_debug_photon_selections(self.scene._handle, out.ctypes.data_as(C.c_void_p), out.size, dims))
        return out

    def photon_sample_array(self, num_samples):
        """get_color_with_photon_map over the frame (photon.rs:706-716): (h*w, 3) fp64 means."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        out = np.empty((self.width_ * self.height_, 3), dtype=np.float64)
        _lib.check(lib.rpt_photon_render_sample(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), self.gather_size_,
            self.gather_size_volume_, int(num_samples), C.c_uint64(self.seed_), self._sample_offset,
            out.ctypes.data_as(C.c_void_p)))
        self._sample_offset += int(num_samples)
        return out

    def photon_sample_device(self, num_samples, d_out_ptr, stream_ptr=0):
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        _lib.check(lib.rpt_photon_render_sample_device(
            h, C.byref(camera_desc(self.camera, _lib.CameraDesc)), C.byref(self._params()), self.gather_size_,
            self.gather_size_volume_, int(num_samples), C.c_uint64(self.seed_), self._sample_offset,
            C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))
        self._sample_offset += int(num_samples)

    def photon_render(self, photon_count, kind):
        """Renderer::photon_render (photon.rs:655-720) -> (h, w, 3) uint8 image."""
        self.photon_map_build(photon_count, kind)
        buffer = Buffer(self.width_, self.height_, self.filter_)
        self._sample_offset = 0
        buffer.add_samples(self.photon_sample_array(self.num_samples_))
        return buffer.image()

    def photon_point_query_beam_render(self, photon_count):   # photon.rs:642-644
        return self.photon_render(photon_count, Renderer.PHOTON_POINT_BEAM)

    def photon_beam_query_beam_render(self, photon_count):    # photon.rs:646-648
        return self.photon_render(photon_count, Renderer.PHOTON_BEAM_BEAM)

    def photon_map_render(self, photon_count):                # photon.rs:650-652
        return self.photon_render(photon_count, Renderer.PHOTON_MAP)

    def counters(self):
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().rpt_get_counters(self.scene._handle, out))
        names = ["samples", "rays", "vertices", "wave_trips", "prim_tests", "bvh_nodes", "bvh_tris", "stack_overflows"]
        return dict(zip(names, [int(v) for v in out]))

    def get_closest_hit(self, origins, dirs):
        """Renderer::get_closest_hit (renderer.rs:416-425), batched: -> (t, object index, normal)."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.empty(n, dtype=np.float32)
        obj = np.empty(n, dtype=np.int32)
        nrm = np.empty((n, 3), dtype=np.float32)
        _lib.check(lib.rpt_intersect_batch(h, n, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                           t.ctypes.data_as(C.c_void_p), obj.ctypes.data_as(C.c_void_p),
                                           nrm.ctypes.data_as(C.c_void_p)))
        return t, obj, nrm

    def get_closest_hit_f64(self, origins, dirs):
        """The same query in the reference-epsilon mode (a scene with set_option("epsilon_policy", 1)): fp64 rays, t_min = 1e-12,
        the mode's own closest hit -> (t, object index, normal), fp64; t = inf and object -1 on a miss."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        t = np.empty(n, dtype=np.float64)
        obj = np.empty(n, dtype=np.int32)
        nrm = np.empty((n, 3), dtype=np.float64)
        _lib.check(lib.rpt_intersect_batch_f64(h, n, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                               t.ctypes.data_as(C.c_void_p), obj.ctypes.data_as(C.c_void_p),
                                               nrm.ctypes.data_as(C.c_void_p)))
        return t, obj, nrm

    def f64_mesh_tree_info(self):
        """The candidate trees of the reference-epsilon mode's large meshes (scene option "f64_mesh_tree_min") -> dict of meshes,
        triangles, nodes, depth, bytes, render_uses_trees, photon_uses_trees (1: the pass walks the trees, 0: it scans every
        triangle) and tree_min.  RPT_ERR_STATE for an fp32 scene."""
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().rpt_f64_mesh_tree_info(self.scene._commit(self.device_), out))
        keys = ("meshes", "triangles", "nodes", "depth", "bytes", "render_uses_trees", "photon_uses_trees", "tree_min")
        return {k: int(v) for k, v in zip(keys, out)}

    # ---- per-call hooks on the committed scene (rpt_debug_*): one device-function call per case
    def debug_light_sample(self, light_index, positions, seed=0, f64=False):
        """Shape::sample and Light::illuminate of Light::Object `light_index` at n positions, case i on stream (seed, i, 0), by the
        scene's own mode (f64: the reference-epsilon mode's functions) -> dict of v, nrm (n, 3), p (n), intensity, wi (n, 3),
        dist (n), next_word (n, uint32)."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        ft = np.float64 if f64 else np.float32
        pos = np.ascontiguousarray(positions, dtype=ft).reshape(-1, 3)
        n = pos.shape[0]
        out = {"v": np.empty((n, 3), ft), "nrm": np.empty((n, 3), ft), "p": np.empty(n, ft), "intensity": np.empty((n, 3), ft),
               "wi": np.empty((n, 3), ft), "dist": np.empty(n, ft), "next_word": np.empty(n, np.uint32)}
        fn = lib.rpt_debug_light_sample_f64 if f64 else lib.rpt_debug_light_sample
        _lib.check(fn(h, light_index, n, pos.ctypes.data_as(C.c_void_p), seed,
                      *[out[k].ctypes.data_as(C.c_void_p) for k in ("v", "nrm", "p", "intensity", "wi", "dist", "next_word")]))
        return out

    def debug_env_color(self, dirs, f64=False):
        """Environment::get_color of n directions (any length) by the scene's own mode -> (n, 3)."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        d = np.ascontiguousarray(dirs, dtype=np.float64 if f64 else np.float32).reshape(-1, 3)
        out = np.empty_like(d)
        fn = lib.rpt_debug_env_color_f64 if f64 else lib.rpt_debug_env_color
        _lib.check(fn(h, d.shape[0], d.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_medium_distance(self, n, seed=0):
        """The distance sample of a vertex in the scene's medium, case i on stream (seed, i, 0) -> (dmed, t_limit), fp32."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        dmed, lim = np.empty(n, np.float32), np.empty(n, np.float32)
        _lib.check(lib.rpt_debug_medium_distance(h, n, seed, dmed.ctypes.data_as(C.c_void_p), lim.ctypes.data_as(C.c_void_p)))
        return dmed, lim

    def debug_shadow_test(self, light_index, origins, dirs, dist):
        """The scan kernels' shadow query and light decision for Light::Object `light_index`, one segment per case: from origins[i]
        along dirs[i] with the light's sample at dist[i] -> (flag (n, int32): the light is visible, t (n, fp32): the closest hit's
        parameter, dist (1 + 1e-3) on a miss).  Scenes without a tree (the linear scan's query)."""
        lib = _lib.load()
        h = self.scene._commit(self.device_)
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        ds = np.ascontiguousarray(dist, dtype=np.float32).reshape(-1)
        n = o.shape[0]
        if d.shape[0] != n or ds.shape[0] != n:
            raise ValueError("origins, dirs and dist differ in length")
        flag, t = np.empty(n, np.int32), np.empty(n, np.float32)
        _lib.check(lib.rpt_debug_shadow_test(h, light_index, n, _vp(o), _vp(d), _vp(ds), _vp(flag), _vp(t)))
        return flag, t

    def shadow_scan_info(self, light_index):
        """How the scan kernels test the visibility of Light::Object `light_index` -> dict of twin_lo, twin_hi (hit codes of its twin
        object's records; lo > hi: no single range), shadow_form (1: the scan's shadow form, option "shadow_scan"; 0: the closest-hit
        scan) and twin_object (-1: none)."""
        out = (C.c_uint32 * 4)()
        _lib.check(_lib.load().rpt_shadow_scan_info(self.scene._commit(self.device_), light_index, out))
        return {"twin_lo": int(out[0]), "twin_hi": int(out[1]), "shadow_form": int(out[2]), "twin_object": int(np.int32(np.uint32(out[3])))}

    def scan_jit_info(self):
        """rpt_scan_jit_info: the scan kernel compiled for this scene's record counts (option "scan_jit") -> dict of state ("off", "idle",
        "active", "fallback", "out_of_scope"), cache ("none", "memory", "disk", "miss"), compile_ms, vgprs, scratch (bytes per lane),
        launches (of the specialised kernel on this scene), compiles (in this process), aot_vgprs, shape, reason and structure
        (rpt_scan_jit_structure: the second block of constants, "groups=...;lights=...;mats=...;medium_kind=...;hdri=...;pairs=...")."""
        out = (C.c_int64 * 8)()
        text, structure = C.create_string_buffer(2048), C.create_string_buffer(512)
        _lib.check(_lib.load().rpt_scan_jit_info(self.scene._commit(self.device_), out, C.cast(text, C.c_void_p), len(text)))
        _lib.check(_lib.load().rpt_scan_jit_structure(self.scene._commit(self.device_), C.cast(structure, C.c_void_p), len(structure)))
        shape, _, reason = text.value.decode(errors="replace").partition("\n")
        return {"state": ("off", "idle", "active", "fallback", "out_of_scope")[int(out[0])], "cache": ("none", "memory", "disk", "miss")[int(out[1])],
                "compile_ms": out[2] / 1000.0, "vgprs": int(out[3]), "scratch": int(out[4]), "launches": int(out[5]), "compiles": int(out[6]),
                "aot_vgprs": int(out[7]), "shape": shape, "reason": reason, "structure": structure.value.decode(errors="replace")}


# ---- per-call hooks that need no scene (rpt_debug_bounce, rpt_debug_distance_pair, rpt_debug_material_f64, rpt_debug_material_bsdf_f64)
def debug_distance_pair(sigma_t, k0, n):
    """The medium distance -ln(xi) / sigma_t of the draws xi = (2 k + 1) 2^-24, k = k0 .. k0 + n - 1 -> (as the render kernels form
    it, by the guarded __logf), fp32 each."""
    new, guarded = np.empty(n, np.float32), np.empty(n, np.float32)
    _lib.check(_lib.load().rpt_debug_distance_pair(float(sigma_t), int(k0), int(n), _vp(new), _vp(guarded)))
    return new, guarded


DRAW_FORM_WORDS = 274


def debug_draw_forms(seed, n):
    """The draw forms the kernels changed for speed and the forms they replace, lane i on stream (seed, i, 0) -> (new, ref), uint32
    arrays of shape (274, n): rows [0, 64) range(-1, 1) as float bits, [64, 256) range(-inv, inv) for inv = 1/64, 1/1024, 1/3000,
    [256, 258) the roulette decisions of draws 0..63 as bits, [258, 274) ku, kv of the first eight accepted triangle pairs."""
    new, ref = np.empty((DRAW_FORM_WORDS, n), np.uint32), np.empty((DRAW_FORM_WORDS, n), np.uint32)
    _lib.check(_lib.load().rpt_debug_draw_forms(C.c_uint64(int(seed)), int(n), _vp(new), _vp(ref)))
    return new, ref


def debug_bounce(material, normals, rds, max_bounces=3, depth=0, seed=0, in_medium=False, medium_event=False, albedo_med=0.0,
                 medium_color=(0.0, 0.0, 0.0)):
    """The render kernels' bounce stage (fp32 mode), case i on stream (seed, i, 0), at a surface of `material` with normal
    normals[i] reached along rds[i], or at a medium point (medium_event) -> dict of flag (n, int32), wi, k (n, 3),
    next_word (n, uint32)."""
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    rd = np.ascontiguousarray(rds, dtype=np.float32).reshape(-1, 3)
    n = nrm.shape[0]
    if rd.shape[0] != n:
        raise ValueError("normals and rds differ in length")
    mcol = np.ascontiguousarray(medium_color, dtype=np.float32).reshape(3)
    out = {"flag": np.empty(n, np.int32), "wi": np.empty((n, 3), np.float32), "k": np.empty((n, 3), np.float32),
           "next_word": np.empty(n, np.uint32)}
    md = material_desc(material, _lib.MaterialDesc)
    _lib.check(_lib.load().rpt_debug_bounce(C.byref(md), max_bounces, depth, int(bool(in_medium)), int(bool(medium_event)),
                                            float(albedo_med), _vp(mcol), n, _vp(nrm), _vp(rd), seed,
                                            *[_vp(out[k]) for k in ("flag", "wi", "k", "next_word")]))
    return out


def debug_material_f64(material, normals, wos, seed=0):
    """The reference-epsilon mode's sample_f, case i on stream (seed, i, 0), and its bsdf at the sampled direction -> dict of
    some (n, int32), wi (n, 3), pdf (n), f (n, 3), next_word (n, uint32)."""
    nrm = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    wo = np.ascontiguousarray(wos, dtype=np.float64).reshape(-1, 3)
    n = nrm.shape[0]
    if wo.shape[0] != n:
        raise ValueError("normals and wos differ in length")
    out = {"some": np.empty(n, np.int32), "wi": np.empty((n, 3)), "pdf": np.empty(n), "f": np.empty((n, 3)),
           "next_word": np.empty(n, np.uint32)}
    md = material_desc(material, _lib.MaterialDesc)
    _lib.check(_lib.load().rpt_debug_material_f64(C.byref(md), n, _vp(nrm), _vp(wo), seed,
                                                  *[_vp(out[k]) for k in ("some", "wi", "pdf", "f", "next_word")]))
    return out


def debug_material_bsdf_f64(material, normals, wos, wis):
    """The reference-epsilon mode's bsdf at given directions -> (n, 3)."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in (normals, wos, wis)]
    n = arrs[0].shape[0]
    if any(a.shape[0] != n for a in arrs):
        raise ValueError("normals, wos and wis differ in length")
    f = np.empty((n, 3))
    md = material_desc(material, _lib.MaterialDesc)
    _lib.check(_lib.load().rpt_debug_material_bsdf_f64(C.byref(md), n, *[_vp(a) for a in arrs], _vp(f)))
    return f


def debug_camera_sample(camera, width, height, sample=0, seed=0, f64=False):
    """The camera sample of a render for every pixel of a width x height frame: pixel -> NDC, the two jitter draws and cast_ray
    on stream (seed, pixel, sample), by the fp32 mode's functions or (f64) the reference-epsilon mode's -> dict of o, d (n, 3),
    next_word (n, uint32), pixel y * width + x."""
    ft = np.float64 if f64 else np.float32
    n = width * height
    out = {"o": np.empty((n, 3), ft), "d": np.empty((n, 3), ft), "next_word": np.empty(n, np.uint32)}
    prm = _lib.RenderParams(width, height, 0.0, 0, 0, 1)
    lib = _lib.load()
    fn = lib.rpt_debug_camera_sample_f64 if f64 else lib.rpt_debug_camera_sample
    _lib.check(fn(C.byref(camera_desc(camera, _lib.CameraDesc)), C.byref(prm), seed, sample,
                  *[_vp(out[k]) for k in ("o", "d", "next_word")]))
    return out

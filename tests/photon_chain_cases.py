"""The scenes of the chain-by-chain tests of the photon shooting pass (tests/photon_chain_ref.py has the rule; CPU only: scene
descriptions, no device, no oracle).

Every family is the room [-1, 1]^3 with the side x = +1 open (photons can escape), five Lambertian walls of different colours (a record
credited to the wrong wall has the wrong power from the next vertex on) and one emitter, which is a Light::Object only: nothing can hit
it.  4,096 photons are 16 blocks of the fp32 shooting kernel, so a grid capped at 3 or 1 blocks strides; the per-photon power is exactly
16 (watts = 16 photon_count), a number every format holds.

  flat          the room alone, quad light at y = 0.98                                   photon_shoot_kernel<false, false, .>
  objects       + glass sphere and glass cube (ior 1.5), mirror cube under rotate_y,     mirror / glass vertices store nothing; total
                Phong sphere                                                             internal reflection (the cube: a sphere has
                                                                                         none for light from outside); wi.n <= 0
  fog           flat + homogeneous medium (sigma_a 0.35, sigma_s 3.15): about 6 volume   <true, false, .>; kinds 0, 1 and 2 -- kind 2 with
                records per chain                                                        65,536 photons (0.1 % of the vertices are kept)
  glow          flat + colored_glowing_fog, the room moved up by 250: y = 250 halves it  the colour switch; fp32 only
  glow low      the same, not moved (every vertex below y = 250)                         the reference-epsilon mode's glow
  mesh          flat + a bumpy_torus(12, 8) mesh, which gets a tree of its own           <false, true, .>
  sphere light  flat, the emitter a sphere off the room's axis                           sample_light_shape's sphere branch; emitter
  cube light    flat, the emitter an axis-aligned cube                                   normals near and at +-Y in rotate_from_y
  far index     flat; photon_count 2^33, shard 2^20 + 3 of 2^21: first = 2^32 + 12,288   the g >> 32 half of the stream key; fp32 only
  many          flat + 30 small Lambertian spheres: more than 32 objects                 reference-epsilon mode: LDSTAB = false
"""
import numpy as np

from rpt_amd import Light, Material, Medium, Mesh, Object, Scene, cube, polygon, scenes, sphere, vec3

N_PHOTONS = 4096
N_PHOTONS_BEAMS = 65536
SEED = 5
WALL_COLOURS = [(0.7, 0.7, 0.7), (0.6, 0.7, 0.8), (0.8, 0.8, 0.6), (0.75, 0.7, 0.65), (0.8, 0.4, 0.3)]   # z-, z+, y-, y+, x-
FOG = (0.35, 3.15)
GLOW_LIFT = 250.0

# name -> (modes, kinds); photon_count and the shard of "far index" are in `shoot_args`
FAMILIES = {
    "flat": (("fp32", "fp64"), (1,)),
    "objects": (("fp32", "fp64"), (1,)),
    "fog": (("fp32", "fp64"), (0, 1, 2)),
    "glow": (("fp32",), (1,)),
    "glow low": (("fp64",), (1,)),
    "mesh": (("fp32",), (1,)),
    "sphere light": (("fp32",), (1,)),
    "cube light": (("fp32",), (1,)),
    "far index": (("fp32",), (1,)),
    "many": (("fp64",), (1,)),
}
# records of each kind a family is there to store: (surface, volume) minimum
EXERCISES = {"flat": (1000, 0), "objects": (1000, 0), "fog": (1000, 1000), "glow": (1000, 1000), "glow low": (1000, 1000),
             "mesh": (1000, 0), "sphere light": (1000, 0), "cube light": (1000, 0), "far index": (1000, 0), "many": (1000, 0)}
MIN_BEAMS = 300


def cases():
    """-> [(family, mode, kind)] in a fixed order."""
    return [(f, m, k) for f, (modes, kinds) in FAMILIES.items() for m in modes for k in kinds]


def shoot_args(family, kind):
    """-> dict(photon_count, first, n, shard_rank, shard_count, watts)."""
    if family == "far index":
        pc, sc, rank = 2 ** 33, 2 ** 21, 2 ** 20 + 3
        first, last = pc * rank // sc, pc * (rank + 1) // sc
        assert first == 2 ** 32 + 12288 and last - first == N_PHOTONS and pc * rank < 2 ** 64
        return {"photon_count": pc, "first": first, "n": N_PHOTONS, "shard_rank": rank, "shard_count": sc, "watts": 16.0 * pc}
    pc = N_PHOTONS_BEAMS if kind == 2 else N_PHOTONS
    return {"photon_count": pc, "first": 0, "n": pc, "shard_rank": 0, "shard_count": 1, "watts": 16.0 * pc}


def _room(sc, lift):
    c = [[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]]
    for q, col in zip([(0, 1, 2, 3), (4, 7, 6, 5), (0, 4, 5, 1), (3, 2, 6, 7), (0, 3, 7, 4)], WALL_COLOURS):
        sc.add(Object(polygon([vec3(c[k][0], c[k][1] + lift, c[k][2]) for k in q])).material(Material.diffuse(vec3(*col))))


def _quad_light(lift, y=0.98, a=0.3):
    return polygon([vec3(a, y + lift, -a), vec3(a, y + lift, a), vec3(-a, y + lift, a), vec3(-a, y + lift, -a)])


def scene(family):
    """A fresh Scene of the family (a scene is committed to a device by its first use)."""
    lift = GLOW_LIFT if family == "glow" else 0.0
    sc = Scene()
    _room(sc, lift)
    emitter = _quad_light(lift)
    if family == "objects":
        sc.add(Object(sphere().scale(vec3(0.35, 0.35, 0.35)).translate(vec3(-0.4, -0.55, 0.3))).material(Material.transmissive(1.5)))
        sc.add(Object(cube().scale(vec3(0.25, 0.25, 0.25)).translate(vec3(-0.5, -0.7, -0.5))).material(Material.transmissive(1.5)))
        sc.add(Object(cube().scale(vec3(0.35, 0.35, 0.35)).rotate_y(0.5).translate(vec3(0.45, -0.6, 0.45))).material(Material.mirror()))
        sc.add(Object(sphere().scale(vec3(0.4, 0.4, 0.4)).translate(vec3(0.25, 0.2, -0.35))).material(Material.specular(vec3(0.8, 0.7, 0.5), 3.0)))
    elif family == "fog":
        sc.add(Medium.homogeneous_isotropic(*FOG))
    elif family in ("glow", "glow low"):
        sc.add(Medium.colored_glowing_fog(*FOG))
    elif family == "mesh":
        sc.add(Object(Mesh(scenes.bumpy_torus(12, 8)).scale(vec3(1.6, 1.6, 1.6)).rotate_x(0.5).translate(vec3(0.0, -0.3, 0.0)))
               .material(Material.diffuse(vec3(0.8, 0.6, 0.3))))
    elif family == "sphere light":
        emitter = sphere().scale(vec3(0.15, 0.15, 0.15)).translate(vec3(0.3, 0.5, -0.2))
    elif family == "cube light":
        emitter = cube().scale(vec3(0.15, 0.15, 0.15)).translate(vec3(0.0, 0.5, 0.0))
    elif family == "many":
        rng = np.random.default_rng(3)
        for k in range(30):
            at = rng.uniform(-0.8, 0.8, 3)
            sc.add(Object(sphere().scale(vec3(0.09, 0.09, 0.09)).translate(vec3(*at))).material(Material.diffuse(vec3(0.5 + 0.01 * k, 0.6, 0.7))))
    sc.add(Light.Object(Object(emitter).material(Material.light(vec3(1.0, 0.9, 0.8), 40.0))))
    return sc

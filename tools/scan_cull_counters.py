"""Primary scans by wave trip (COUNT build, scan_primary_culled in device_core.h): how many lanes of a wave have a search interval
that reaches the box around the scanned records, how often no such lane reaches a record group's box, and what a culled scan would
save per trip at the per-record VALU costs of DESIGN.md section 4 (tools/scan_slope.py: 30 per box, 48 per transformed cube; 15 per
rectangle, 60 for the shell, 40 per sphere, 25 per triangle).
The model prices two designs: groups tested only when at most 8 lanes reach the bound (the whole scan skipped when none does), and
groups tested in every trip.  Last line: how often the tail cull that is built (option "scan_cull") left the tail out.
Usage: python tools/scan_cull_counters.py [workload] [spp] [scan_cull 0|1]"""
import ctypes as C
import sys

sys.path.insert(0, ".")
import rpt_amd  # noqa: E402
from rpt_amd import Renderer, _lib, scenes  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "C3"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 16
cull = int(sys.argv[3]) if len(sys.argv) > 3 else 0
scene, cam, cfg = scenes.CONFIGS[name]()
scene.set_option("scan_cull", cull)
r = Renderer(scene, cam).width(min(cfg["width"], 1024)).height(min(cfg["height"], 1024)).max_bounces(cfg["max_bounces"]).seed(0)
rpt_amd.set_option("counters", 1)
r.sample_array(spp)
c = r.counters()
lib = _lib.load()
out = (C.c_uint64 * 16)()
_lib.check(lib.rpt_scan_cull_counters(r.scene._handle, out))
boxes, masks, ng, en = (C.c_float * 36)(), (C.c_uint64 * 5)(), C.c_uint32(), C.c_uint32()
_lib.check(lib.rpt_scan_cull_groups(r.scene._handle, boxes, masks, C.byref(ng), C.byref(en)))
st = r.scene_stats()
n_sph, n_cub, n_aabb = st["spheres"], st["cubes"], st["aabbs"]
v = [int(x) for x in out]
hist, trips = v[0:5], sum(v[0:5])
print(f"{name} {spp} spp, scan_cull {cull} (enabled {en.value}): wave trips {c['wave_trips']}, with a primary query {trips}")
print(f"  bound lo {[round(boxes[i], 3) for i in range(3)]} hi {[round(boxes[3 + i], 3) for i in range(3)]}, always tested: {int(masks[4]):#x}")
for lab, h in zip(["0", "1-2", "3-4", "5-8", ">8"], hist):
    print(f"  lanes reaching the bound {lab:>4s}: {h:12d} trips  {h / max(trips, 1):7.4f}")


def cost(mask):
    """VALU instructions of the records in a mask, by kind (scan order: spheres, cubes, boxes, rectangles, triangles)."""
    tot, bit = 0, 0
    for n, per in ((n_sph, 40), (n_cub, 48), (n_aabb, 30), (st["rects"] - st["shell_faces"], 15), (st["tris"], 25)):
        for i in range(n):
            if (mask >> (bit + i)) & 1:
                tot += per
        bit += n
    return tot


with_lane = trips - hist[0]      # the trips the group counters were taken in
full = cost((1 << 64) - 1)
saved_groups = 0.0
for g in range(ng.value):
    m, none = int(masks[g]), v[5 + g]
    print(f"  group {g}: mask {m:#06x}  lo {[round(boxes[6 + 6 * g + i], 2) for i in range(3)]} hi {[round(boxes[9 + 6 * g + i], 2) for i in range(3)]}  "
          f"~{cost(m)} VALU;  reached by no lane in {none} of {with_lane} trips = {none / max(with_lane, 1):.4f}")
    saved_groups += cost(m) * none / max(with_lane, 1)
p0 = hist[0] / max(trips, 1)
few = (hist[1] + hist[2] + hist[3]) / max(trips, 1)
tests = 12 + 12 * ng.value     # the bound's slab test and one per group (the reciprocals are the scan's own)
print(f"  records {full} + shell 60 VALU per plain scan (model); group boxes unreached, weighted by cost: {saved_groups:.1f} VALU per trip with a lane")
print(f"  groups tested when 1..8 lanes reach the bound: at most {p0:.4f} x {full + 60} (whole scan) + {few:.4f} x {full} (every group, an upper bound)"
      f" - 12 (bound test) = {p0 * (full + 60) + few * full - 12:.1f} VALU saved per trip")
print(f"  groups tested in every trip: {p0:.4f} x {full + 60} + {1 - p0:.4f} x {saved_groups:.1f} - {tests} (tests) = "
      f"{p0 * (full + 60) + (1 - p0) * saved_groups - tests:.1f} VALU saved per trip")
print(f"  tail box lo {[round(boxes[30 + i], 2) for i in range(3)]} hi {[round(boxes[33 + i], 2) for i in range(3)]}: left out in {v[9]} trips = {v[9] / max(trips, 1):.4f}")

// scene_update_lanes.h — what one lane of scene_update.hip's kernels does, as functions the CPU harness runs serially in their place
// (tests/host/scene_update_harness.cpp): the stores of a moved sphere's records, and one child entry of a scene-tree node.
// Every store is a plain store into a record that belongs to this sphere / this entry alone.
#pragma once
#include "scene_update.h"
#include "scene_update_core.h"

namespace rptg {
// Movable sphere k: new centre, records of the mode(s) the scene was committed in, item box, motion row, centre.
RPTU_HD void move_sphere_lane(const SceneUpdateArgs& a, uint32_t k) {
    MovableSphere& m = a.table[k];
    const double r = m.radius;
    double c[3], p[3];
    for (int i = 0; i < 3; i++) {
        p[i] = m.centre[i];
        c[i] = a.centres[3 * size_t(k) + i];
        if (a.offsets) c[i] = c[i] + a.offsets[3 * size_t(k) + i];
    }
    rptu::SphereRecords rec;
    rptu::sphere_records(r, c, &rec);
    // fp32 arena: XfScan, the normal rows of XfShade (r0.w, the object, stays), pbox, and the item box the refit reads
    XfScan& sc = a.sph[m.sph];
    sc.r0 = F4{rec.scan[0], rec.scan[1], rec.scan[2], rec.scan[3]};
    sc.r1 = F4{rec.scan[4], rec.scan[5], rec.scan[6], rec.scan[7]};
    sc.r2 = F4{rec.scan[8], rec.scan[9], rec.scan[10], rec.scan[11]};
    XfShade& sh = a.sph_sh[m.sph];
    sh.r0.x = rec.shade_n; sh.r0.y = 0.f; sh.r0.z = 0.f;
    sh.r1 = F4{0.f, rec.shade_n, 0.f, 1.f};
    sh.r2 = F4{0.f, 0.f, rec.shade_n, 0.f};
    AabbScan& pb = a.pbox[m.sph];
    pb.lo = F4{rec.pbox_lo[0], rec.pbox_lo[1], rec.pbox_lo[2], 0.f};
    pb.hi = F4{rec.pbox_hi[0], rec.pbox_hi[1], rec.pbox_hi[2], 0.f};
    F4* ib = reinterpret_cast<F4*>(a.item_box) + 2 * size_t(k);
    ib[0] = F4{rec.item_lo[0], rec.item_lo[1], rec.item_lo[2], 0.f};
    ib[1] = F4{rec.item_hi[0], rec.item_hi[1], rec.item_hi[2], 0.f};
    if (a.f64) {
        rpt64::ObjRec& o = a.recs[m.rec64];
        for (int i = 0; i < 12; i++) o.inv[i] = rec.inv[i];
        rpt64::ObjShade& os = a.shade[m.rec64];
        for (int i = 0; i < 9; i++) os.nrm[i] = (i == 0 || i == 4 || i == 8) ? rec.nrm : 0.0;
        rpt64::CullBox cb;
        for (int i = 0; i < 3; i++) { cb.lo[i] = rec.cull_lo[i]; cb.hi[i] = rec.cull_hi[i]; }
        cb.unbounded = rec.cull_unbounded;
        cb.slab_test = 0u;
        a.cull[m.rec64] = cb;
    }
    if (a.motion) {
        double rec24[24];
        rptu::sphere_motion_record(r, c, p, rec24);
        double* out = a.motion + size_t(m.object) * 24;
        for (int i = 0; i < 24; i++) out[i] = rec24[i];
    }
    for (int i = 0; i < 3; i++) m.centre[i] = c[i];
}

// Child entry `side` of local scene-tree node `node`: its unpadded bounds into raw[], the padded box (BvhBuilder::build's rule) into
// the node.  The entries of the nodes it reads (an inner entry: both entries of its child node) are of a lower height.
RPTU_HD void refit_entry(const SceneUpdateArgs& a, uint32_t node, uint32_t side) {
    const uint32_t e = 2u * node + side;
    const RefitEntry d = a.entries[e];
    const F4* raw = reinterpret_cast<const F4*>(a.raw);
    const F4* ib = reinterpret_cast<const F4*>(a.item_box);
    float lo[3], hi[3];
    if (d.a == kRefitInner) {
        const F4 l0 = raw[4 * size_t(d.b)], h0 = raw[4 * size_t(d.b) + 1], l1 = raw[4 * size_t(d.b) + 2], h1 = raw[4 * size_t(d.b) + 3];
        lo[0] = fminf(l0.x, l1.x); lo[1] = fminf(l0.y, l1.y); lo[2] = fminf(l0.z, l1.z);
        hi[0] = fmaxf(h0.x, h1.x); hi[1] = fmaxf(h0.y, h1.y); hi[2] = fmaxf(h0.z, h1.z);
    } else {
        for (int k = 0; k < 3; k++) { lo[k] = d.lo[k]; hi[k] = d.hi[k]; }
        for (int s = 0; s < 2; s++) {
            const uint32_t m = s == 0 ? d.a : d.b;
            if (m == kRefitNone) continue;
            const F4 l = ib[2 * size_t(m)], h = ib[2 * size_t(m) + 1];
            lo[0] = fminf(lo[0], l.x); lo[1] = fminf(lo[1], l.y); lo[2] = fminf(lo[2], l.z);
            hi[0] = fmaxf(hi[0], h.x); hi[1] = fmaxf(hi[1], h.y); hi[2] = fmaxf(hi[2], h.z);
        }
    }
    F4* out = reinterpret_cast<F4*>(a.raw) + 2 * size_t(e);
    out[0] = F4{lo[0], lo[1], lo[2], 0.f};
    out[1] = F4{hi[0], hi[1], hi[2], 0.f};
    float plo[3], phi[3];
    rptu::pad_node_box(lo, hi, plo, phi);
    BvhNode& n = a.nodes[a.top_root + node];
    float* nlo = side == 0 ? n.lo0 : n.lo1;
    float* nhi = side == 0 ? n.hi0 : n.hi1;
    for (int k = 0; k < 3; k++) { nlo[k] = plo[k]; nhi[k] = phi[k]; }   // (e0 / e1 and the pad words between the boxes stay)
}
}  // namespace rptg

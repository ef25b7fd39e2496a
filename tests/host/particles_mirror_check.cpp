// Test infrastructure for tests/test_particles_host.py: include/rpt.hpp's particle mirrors without a GPU -- a system of the caller's
// own through the header's host RK4, the built-in circle system through the library's host function (device = -1): the same bits.
#include "rpt.hpp"
#include <cstdio>
struct Mine : rpt::ParticleSystem {
    rpt::ParticleState time_derivative(const rpt::ParticleState& s) const override {
        rpt::ParticleState d = s;
        for (size_t i = 0; i < s.size(); i++) { d.pos[i] = {-s.pos[i][1], s.pos[i][0], 0.0}; d.vel[i] = {0, 0, 0}; }
        return d;
    }
};
int main() {
    rpt::ParticleState a{{{1, 0, 0}}, {{0, 0, 0}}}, b = a;
    Mine().rk4_integrate(a, 3.14159, 0.005);
    rpt::SimpleCircleSystem c; c.device = -1; c.rk4_integrate(b, 3.14159, 0.005);
    rpt::MarblesSystem m(0.15); m.device = -1;
    auto d = m.time_derivative(b);
    auto cp = rpt::monomial_surface(2, 4).closest_point_precise({0.5, 0.2, 0});
    auto disp = m.display_positions(b.pos);
    std::printf("%d %.17g %.17g %g %g %g\n", a.pos[0] == b.pos[0], a.pos[0][0], b.pos[0][0], d.vel[0][1], cp[0], disp[0][1]);
    return a.pos[0] == b.pos[0] ? 0 : 1;
}

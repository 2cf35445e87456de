// tools/sanitize/light_pick.cpp -- stand-alone (its own main, no GPU): kyhip_scene_light_pick, and with it pack_light_pick (ky_pack.cpp), on scenes of 0 .. 16 lights of every kind with
// 0 .. 6 carrier surfaces of other shapes each -- the proxy table empty, filling, full and overflowing --, black and NaN colours.  `make sanitize` compiles it with the
// host-only sources under -fsanitize=address,undefined (build/san/light_pick_asan) and runs it.  Exit status 1 when a table is not what it must be.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../include/kyhip.h"
static ky_shape sphere(float x, float y, float z, float r) { ky_shape s{}; s.kind = KY_SHAPE_SPHERE; s.p[0][0] = x; s.p[0][1] = y; s.p[0][2] = z; s.radius = r; return s; }
static ky_shape rect(float x, float y, float z, float h) { ky_shape s{}; s.kind = KY_SHAPE_RECTANGLE; const float q[4][2] = {{-h,-h},{-h,h},{h,h},{h,-h}};
  for (int i = 0; i < 4; ++i) { s.p[i][0] = x + q[i][0]; s.p[i][1] = y + q[i][1]; s.p[i][2] = z; } s.normal[2] = -1; return s; }
int main() {
  int bad = 0;
  for (int nl = 0; nl <= 16; ++nl) for (int nc = 0; nc <= 6; ++nc) for (int variant = 0; variant < 3; ++variant) {
    std::vector<ky_shape> shapes; std::vector<ky_light> lights; std::vector<ky_surface> surfaces; std::vector<ky_material> mats(1);
    mats[0].kind = KY_MATERIAL_MATTE;
    shapes.push_back(rect(0, 0, -1, 3)); surfaces.push_back({0, 0, -1});
    int env = -1;
    for (int i = 0; i < nl; ++i) {
      ky_light l{}; l.color[0] = variant == 2 ? NAN : (variant == 1 ? 0.f : 1.f + i); l.color[1] = 2; l.color[2] = variant == 1 ? -1.f : 3; l.world_radius = 5; l.direction[2] = -1;
      const int kind = (i + variant) % 5;
      if (kind == 0) { l.kind = KY_LIGHT_POINT; }
      else if (kind == 1) { l.kind = KY_LIGHT_DIRECTION; }
      else if (kind == 2 && env < 0) { l.kind = KY_LIGHT_ENVIRONMENT; env = i; }
      else { l.kind = KY_LIGHT_AREA; shapes.push_back(kind == 3 ? sphere(i, 0, 1, 0.1f) : rect(i, 1, 2, 0.1f)); l.shape = (int)shapes.size() - 1;
             for (int k = 0; k < nc; ++k) { shapes.push_back(k & 1 ? sphere(i, k, 0, 0.05f) : rect(i, k, 0.5f, 0.05f)); surfaces.push_back({(int)shapes.size() - 1, 0, i}); } }
      lights.push_back(l);
    }
    ky_scene sc{}; sc.shapes = shapes.data(); sc.shape_count = (int)shapes.size(); sc.materials = mats.data(); sc.material_count = 1; sc.lights = lights.data(); sc.light_count = nl;
    sc.surfaces = surfaces.data(); sc.surface_count = (int)surfaces.size(); sc.environment_light = env;
    sc.camera.position[2] = 5; sc.camera.front[2] = -1; sc.camera.right[0] = 1; sc.camera.up[1] = 1; sc.camera.resolution[0] = 16; sc.camera.resolution[1] = 16;
    float p16[16]; std::vector<float> prox(11 * 40);
    const int n = kyhip_scene_light_pick(&sc, 2, p16, prox.data(), 40);
    if (sc.surface_count > KYHIP_MAX_SURFACES) continue;
    if (n < 0) { std::printf("nl %d nc %d v %d: status %d %s\n", nl, nc, variant, n, kyhip_last_error()); ++bad; continue; }
    double sum = 0; for (int i = 0; i < nl; ++i) { sum += p16[i]; if (!(p16[i] >= 0.25f / nl * 0.999f)) ++bad; }
    if (n > 32 || (nl > 0 && std::fabs(sum - 1) > 1e-5) || n < nl) { std::printf("nl %d nc %d v %d: n %d sum %g\n", nl, nc, variant, n, sum); ++bad; }
    if (kyhip_scene_light_pick(&sc, 1, nullptr, prox.data(), 3) != n) ++bad;   // a short table: the count all the same
  }
  std::printf("light_pick: %d problems\n", bad);
  return bad != 0;
}

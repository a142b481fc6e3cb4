// test_aniso_surface_shim.cpp — sph::hip_impl::Solver::surfaceAnisotropic() / surfaceAnisotropicIndexed() against the C ABI
// they wrap: the shim hands the library's mesh through bit for bit, in both precisions, for the soup and the indexed mesh;
// refuses before a step; the stock surface() before and after the call is the same mesh; and a call between two steps leaves
// the next step's result alone.  Prints "ok <name>" / "FAIL <name>" lines and "ALL OK"; tests/test_aniso_surface_gpu.py runs
// it on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "hipsph.hpp"
#include "shim_check.hpp"

using T = size_t;

using shim::check;
using shim::same_bytes;

template <typename N> static void run(const std::string &tag) {
  using P = sph::Particle<T, N, sph::vec>;
  auto [mc, config, particles] = sph::simpleConfigWith2Cubes<T, N, sph::vec>(2048, 2, N(500));
  config.surface = mc;
  for (size_t i = 0; i < particles.size(); i += 9) particles[i].type = sph::Type::Obstacle;
  const sph::Scene<T, N, sph::vec> scene{};
  const sph::hip_impl::AnisoSurface cfg{2.0, 0.4, {0.9, 4.0, 20.0 / 3.0, 0.5, 8u}};

  sph::hip_impl::Solver<T, N> a(N(0.1)), b(N(0.1));
  a.upload(particles), b.upload(particles);
  bool refused = false;
  try {
    (void)a.surfaceAnisotropic(config, cfg, scene);
  } catch (const std::exception &e) {
    refused = std::strstr(e.what(), "pbf_surface_anisotropic") != nullptr;
  }
  check(tag + "aniso_surface_shim_needs_a_step", refused);

  a.step(config), b.step(config);
  const auto stock0 = a.surface(config, scene);
  const auto soup = a.surfaceAnisotropic(config, cfg, scene);

  // the same calls through the C ABI
  pbf_params p{};
  p.dt = double(config.dt), p.scale = double(config.scale), p.iteration = config.iteration;
  p.constant_force[0] = config.constantForce.x, p.constant_force[1] = config.constantForce.y, p.constant_force[2] = config.constantForce.z;
  p.min_bound[0] = config.minBound.x, p.min_bound[1] = config.minBound.y, p.min_bound[2] = config.minBound.z;
  p.max_bound[0] = config.maxBound.x, p.max_bound[1] = config.maxBound.y, p.max_bound[2] = config.maxBound.z;
  uint64_t nt = 0, nv = 0;
  check(tag + "aniso_surface_shim_capi_ok", pbf_surface_anisotropic(a.context(), &p, &cfg, 0, nullptr, &nt) == PBF_OK && nt > 0);
  std::vector<sph::vec<3, N>> vs(3 * nt), ns(3 * nt);
  std::vector<sph::vec<4, N>> cs(3 * nt);
  check(tag + "aniso_surface_shim_download", pbf_download_mesh(a.context(), vs.data(), ns.data(), cs.data()) == PBF_OK);
  check(tag + "aniso_surface_shim_soup_bits", same_bytes(soup.vs, vs) && same_bytes(soup.ns, ns) && same_bytes(soup.cs, cs));
  bool finite = true;
  for (size_t i = 0; i < vs.size(); ++i)
    finite = finite && std::isfinite(vs[i].x + vs[i].y + vs[i].z) && std::isfinite(ns[i].x + ns[i].y + ns[i].z) &&
             std::isfinite(cs[i].x + cs[i].y + cs[i].z + cs[i].w);
  check(tag + "aniso_surface_shim_finite", finite);
  // the indexed reader refuses a soup, as after pbf_surface
  check(tag + "aniso_surface_shim_kinds_exclude", pbf_download_mesh_indexed(a.context(), nullptr, nullptr, nullptr, nullptr) == PBF_ERR_STATE);

  const auto indexed = a.surfaceAnisotropicIndexed(config, cfg, scene);
  check(tag + "aniso_surface_shim_indexed_capi_ok",
        pbf_surface_anisotropic(a.context(), &p, &cfg, 1, &nv, &nt) == PBF_OK && nt * 3 == indexed.tris.size() && nv == indexed.vs.size());
  std::vector<sph::vec<3, N>> iv(nv), in(nv);
  std::vector<sph::vec<4, N>> ic(nv);
  std::vector<uint32_t> it(3 * nt);
  check(tag + "aniso_surface_shim_indexed_download",
        pbf_download_mesh_indexed(a.context(), iv.data(), in.data(), ic.data(), it.data()) == PBF_OK);
  check(tag + "aniso_surface_shim_indexed_bits",
        same_bytes(indexed.vs, iv) && same_bytes(indexed.ns, in) && same_bytes(indexed.cs, ic) && same_bytes(indexed.tris, it));
  check(tag + "aniso_surface_shim_same_triangles", indexed.tris.size() == soup.vs.size());
  check(tag + "aniso_surface_shim_indexed_needs_n_vertices",
        pbf_surface_anisotropic(a.context(), &p, &cfg, 1, nullptr, &nt) == PBF_ERR_INVALID);

  // the stock surface is what it was
  const auto stock1 = a.surface(config, scene);
  check(tag + "aniso_surface_shim_stock_unchanged",
        same_bytes(stock0.vs, stock1.vs) && same_bytes(stock0.ns, stock1.ns) && same_bytes(stock0.cs, stock1.cs));

  // the observer changes nothing: one more step on both
  a.step(config), b.step(config);
  std::vector<P> ya, yb;
  a.download(ya), b.download(yb);
  check(tag + "aniso_surface_shim_observer", shim::same_particles(ya, yb));
}

int main() {
  run<float>("fp32_");
  run<double>("fp64_");
  return shim::finish();
}

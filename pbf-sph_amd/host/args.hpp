// args.hpp — command line of the benchmark driver.  Same flags, defaults and {iter}/{impl}/{type}
// output templates as the reference's sph::driver::Args (src/args.hpp:38-56, src/args.cpp:7-75),
// parsed by a small hand-written parser instead of the vendored Taywee/args, plus additive flags
// (marked +) that the stock CLI cannot express: its particle count, solver iterations and scene are
// compiled in (src/benchmark.cpp:23-25).
#pragma once

#include <array>
#include <cstddef>
#include <iostream>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace sph::driver {

struct Args {
  std::string impl = "hip";               // -i/--impl   (reference default "omp": not part of this product)
  bool list = false;                      // -l/--list
  bool verbose = false;                   // -v/--verbose
  std::vector<std::string> devices;       // -d/--devices (index or name substring, first match)
  size_t iterations;                      // -n/--iter
  size_t warmup = 200;                    // -w/--warmup
  bool fp64 = false;                      // --fp64
  std::string output;                     // -o/--output
  // + additive
  size_t particles = 20 * 1000;           // --particles   (stock: benchmark.cpp:23)
  size_t solverIter = 6;                  // --solver-iter (stock: benchmark.cpp:24)
  std::string scene = "cubes";            // --scene cubes|dam-break
  bool resident = false;                  // --resident: keep particles on the GPU between frames
  bool surface = true;                    // --no-surface: skip marching cubes (stock: on, benchmark.cpp:29)
  bool fastMath = false;                  // --fast-math
  bool json = false;                      // --json: one machine-readable line after the summary
  bool allDevices = false;                // --all-devices: EVERY device matching -d becomes one x-slab (RCCL halo)
  size_t slabs = 0;                       // --slabs K: K slabs on the first matching device (in-process exchange: tests)
  double cohesion = 0, adhesion = 0;      // --surface-tension=gamma[,beta]: opt-in Akinci 2013 surface tension / adhesion
  // --collider=sphere:cx,cy,cz,r | bowl:cx,cy,cz,r | plane:nx,ny,nz,d [,margin[,spacing]] with --resident: opt-in static SDF collider
  // --collider=mesh:FILE.obj[,margin[,spacing[,negate[,winding]]]]: the same collider, its lattice built on the device from a
  // closed mesh, or with the fifth field `winding` (or 1) from a triangle soup signed by the winding number
  // --scenery=<the same grammar> with --resident: a second, STATIC solid beside the collider (pbf_set_scenery); combines with
  // every --collider* flag
  struct Solid {
    std::string shape;                    // "" = off
    std::string mesh;                     // shape "mesh": the OBJ file
    bool negate = false;                  // shape "mesh": the solid is outside the mesh
    bool winding = false;                 // shape "mesh": PBF_MESH_SIGN_WINDING (open and broken meshes are accepted)
    double cfg[4] = {0, 0, 0, 0};
    double margin = 13.5;                 // half the rest spacing of 27 world units
    double spacing = 0;                   // 0 = h * scale / 2
  };
  Solid solid, scenery;                   // --collider, --scenery
  // --collider-motion=vx,vy,vz[,wx,wy,wz[,px,py,pz]] with --resident and --collider: the solid moves rigidly — a linear velocity
  // and an angular velocity (rad / s) about a pivot, world units per second; --collider-reaction[=every] prints the wrench
  bool colliderMoves = false;
  double colliderMotion[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  size_t colliderReaction = 0;            // 0 = off
  // --collider-body=mass[,Ixx,Iyy,Izz[,gain]] with --resident and --collider=sphere|bowl|plane: the solid is a rigid body the
  // fluid moves (pbf_set_collider_body); --collider-body-report[=every] prints its state
  bool colliderBody = false;
  double colliderBodyCfg[5] = {0, 0, 0, 0, 0.49};   // mass, the principal moments (0 = a solid ball of the collider's radius), gain
  size_t colliderBodyReport = 0;          // 0 = off
  // --collider-body-contact[=restitution[,mu[,iterations]]] with --collider-body and --scenery: the body collides with the
  // scenery (pbf_set_collider_body_contact); the report line then carries contact_points, contact_depth and contacts
  bool colliderBodyContact = false;
  double colliderBodyContactCfg[3] = {0, 0, 1};   // restitution, mu, iterations
  // --collider-friction=mu with --resident and --collider: Coulomb friction against the solid (pbf_set_collider_friction; inf =
  // no-slip), relative to --collider-motion's velocities when given; --collider-friction-report[=every] prints the pass's sums
  double colliderFriction = 0;            // 0 = off
  size_t colliderFrictionReport = 0;      // 0 = off
  double wwTa = 0, wwWc = 0;              // --whitewater=k_ta,k_wc[,capacity]: spray / foam / bubbles (Ihmsen 2012) with --resident
  size_t wwCapacity = 0;                  // 0 = off
  // --whitewater-solids[=restitution[,friction[,absorb]]] with --whitewater: the diffuse particles collide with the collider
  // and the scenery (pbf_set_whitewater_solids); the whitewater report then carries the four counts of the last step
  bool wwSolids = false;
  double wwSolidsCfg[3] = {0, 0, 0};      // restitution, friction, absorb
  bool anisotropy = false;                // --anisotropy[=smoothing,k_r,k_s,k_n,min_neighbours]: ellipsoids.ply (Yu & Turk 2013) with --resident
  double anisoCfg[4] = {0.9, 4.0, 20.0 / 3.0, 0.5};
  unsigned anisoMinNeighbours = 25;
  bool anisoSurface = false;              // --anisotropic-surface=isolevel[,smoothing,k_r,k_s,k_n,min_neighbours] with --resident
  double anisoSurfaceIso = 0;             // (no default: the field's scale is not the stock one's)
  double anisoSurfaceCfg[4] = {0.9, 4.0, 20.0 / 3.0, 0.5};
  unsigned anisoSurfaceMinNeighbours = 25;
  bool indexedMesh = false;               // --indexed-mesh: the frames' surface as an indexed mesh (one vertex per lattice edge)
  size_t diagnostics = 0;                 // --diagnostics[=every]: with --resident, a JSON line of pbf_diagnostics every `every` frames

  std::vector<std::array<double, 3>> probes;  // --probe=x,y,z (repeatable): with --resident, the SPH sums at that world point
  size_t probeEvery = 0;                  // --probe-every=k: a report every k timed frames (0 = once, after the last one)

  struct SourceArg {
    std::array<double, 7> v;  // x, y, z, vx, vy, vz, rate
    unsigned long long tag;
  };
  std::vector<SourceArg> sources;              // --source=x,y,z,vx,vy,vz,rate[,tag] (repeatable): an inlet (sph::Source)
  std::vector<std::array<double, 4>> drains;   // --drain=x,y,z,width (repeatable): an outlet (sph::Drain)

  Args(size_t defaultIterations, std::string defaultOutput)
      : iterations(defaultIterations), output(std::move(defaultOutput)) {}

  static void usage(std::ostream &os) {
    os << "  benchmark {OPTIONS}\n\n    PBF sph benchmark\n\n  OPTIONS:\n\n"
          "      -h, --help                        Display this help menu\n"
          "      -i[impl], --impl=[impl]           Which implementation to use.\n"
          "                                        One of: hip  (omp, ocl, sycl, sycl2020 live in the reference)\n"
          "                                        Default: hip\n"
          "      -l, --list                        List devices available for [impl] and exit\n"
          "      -v, --verbose                     Show details such as per-stage timings for [impl]\n"
          "      -d[dev...], --devices=[dev...]    Allowed device list (first match only).\n"
          "                                        Entries could be a 0-based index or a substring of the device name\n"
          "                                        Default: 0\n"
          "      -n[iter], --iter=[iter]           How many iterations to run the simulation for.\n"
          "                                        Default: 200\n"
          "      -w[warmup], --warmup=[warmup]     How many iterations to skip for warmup before timing starts.\n"
          "                                        Default: 200\n"
          "      --fp64                            Use FP64 (double) instead of FP32 (float).\n"
          "      -o[out], --output=[out]           Directory to write the final state (cloud.ply, mesh.obj) to.\n"
          "                                        Templates: {iter}, {impl}, {type}; empty string disables output\n"
          "                                        Default: ./out_{impl}_{type}_{iter}\n"
          "    additive (not in the reference CLI):\n"
          "      --particles=[n]                   Nominal particle count. Default: 20000 (stock)\n"
          "      --solver-iter=[k]                 Solver iterations per frame. Default: 6 (stock)\n"
          "      --scene=[cubes|dam-break]         cubes = stock two cubes in a moving box; dam-break = static box\n"
          "      --resident                        Time the device-resident loop (no per-frame host round trip)\n"
          "      --no-surface                      Skip the marching-cubes surface (the stock driver runs with it on)\n"
          "      --fast-math                       v_rsq / fma pair kernels (the reference builds with -Ofast)\n"
          "      --json                            Print one JSON line with the results\n"
          "      --all-devices                     Use EVERY device matching -d: one x-slab per GPU, ghost-layer\n"
          "                                        exchange over RCCL (implies --resident --no-surface)\n"
          "      --slabs=[K]                       K slabs on the first matching device (in-process exchange; tests)\n"
          "      --surface-tension=[g[,b]]         Opt-in surface tension (cohesion g) and adhesion to obstacles (b) after\n"
          "                                        Akinci et al. 2013; not in the reference. Single device only\n"
          "      --collider=[shape:a,b,c,d[,margin[,spacing]]]  With --resident: an opt-in static solid the fluid is kept out of,\n"
          "                                        as a signed-distance lattice over the box plus one spacing. shape:\n"
          "                                        sphere:cx,cy,cz,r (solid ball), bowl:cx,cy,cz,r (solid outside the ball),\n"
          "                                        plane:nx,ny,nz,d (solid where n.x < d, n normalised). The fluid stays\n"
          "                                        `margin` world units off the solid (default 13.5); lattice spacing in\n"
          "                                        world units (default h * scale / 2). Single device only\n"
          "      --collider=mesh:[FILE.obj[,margin[,spacing[,negate[,winding]]]]]  The same, from a closed triangle mesh (v and\n"
          "                                        triangular f lines, counter-clockwise from outside): the lattice is computed\n"
          "                                        on the device. negate = 1: the solid is OUTSIDE the mesh (a cavity). A fifth\n"
          "                                        field `winding` signs the distance by the winding number: open, misoriented\n"
          "                                        and non-manifold meshes are accepted, their edge counts printed\n"
          "      --scenery=[shape:... | mesh:...]  With --resident: a second, STATIC solid beside the collider, in --collider's\n"
          "                                        grammar with the same defaults (the harbour, bowl, ramp or floor around a\n"
          "                                        moving or floating collider). It stays in the world frame and has no pose,\n"
          "                                        body, friction or reaction; the fluid is projected out of it after the\n"
          "                                        collider. Combines with every --collider* flag. Single device only\n"
          "      --collider-motion=[vx,vy,vz[,wx,wy,wz[,px,py,pz]]]  With --resident and --collider: the solid moves rigidly, with\n"
          "                                        a linear velocity and an angular velocity (rad / s) about the pivot p, in\n"
          "                                        world units per second: the pose of a frame is set before it is stepped\n"
          "                                        (no lattice upload, no recapture). A body that moves further per frame\n"
          "                                        than its thickness can pass through fluid\n"
          "      --collider-reaction[=every]       With --resident and --collider: one JSON line per `every` frames with the impulse\n"
          "                                        and angular impulse the collider gave the fluid in that frame\n"
          "      --collider-body=[mass[,Ixx,Iyy,Izz[,gain]]]  With --resident and --collider=sphere|bowl|plane: the solid floats — a\n"
          "                                        rigid body integrated on the device inside every step from the reaction of\n"
          "                                        the fluid, starting at rest at the collider's centre (a plane: the box's)\n"
          "                                        under the fluid's own acceleration, its centre kept inside the box. Moments\n"
          "                                        about the lattice's axes (default: a solid ball of the sphere's radius);\n"
          "                                        gain 0.49 (default) returns the momentum the fluid was given\n"
          "      --collider-body-report[=every]    One JSON line per `every` frames with the body's state\n"
          "      --collider-body-contact[=restitution[,mu[,iterations]]]  With --collider-body and --scenery: the body collides\n"
          "                                        with the scenery — its surface (the collider's zero level, one point per\n"
          "                                        crossed lattice cell) is tested against the scenery after every advance and\n"
          "                                        answered with an impulse and a shift of the centre on the device. Defaults:\n"
          "                                        restitution 0, mu 0, 1 pass per step. The report line gains contact_points,\n"
          "                                        contact_depth and contacts\n"
          "      --collider-friction=[mu]          With --resident and --collider: Coulomb friction against the solid, one pass\n"
          "                                        after every finalise; mu > 0, inf = no-slip. With --collider-motion the drag is\n"
          "                                        towards the moving solid's contact velocity, with --collider-body the body's\n"
          "      --collider-friction-report[=every]  One JSON line per `every` frames with the impulse and angular impulse the\n"
          "                                        friction pass gave the fluid in that frame\n"
          "      --whitewater=[k_ta,k_wc[,capacity]]  With --resident: spray, foam and air bubbles after Ihmsen et al. 2012,\n"
          "                                        one whitewater step after every frame at these rates; the tau ranges are\n"
          "                                        the 10 % / 90 % quantiles of the potentials at the first frame. Pool of\n"
          "                                        `capacity` particles (default 262144); whitewater.ply beside cloud.ply.\n"
          "                                        Single device only\n"
          "      --whitewater-solids[=e[,f[,absorb]]]  With --whitewater: spray, foam and bubbles collide with --collider and\n"
          "                                        --scenery: projected out after their advection, restitution e and tangential\n"
          "                                        loss f in [0, 1] (defaults 0, 0); absorb = 1: spray outside the fluid dies on\n"
          "                                        a solid. The whitewater report gains the step's four counts\n"
          "      --anisotropy[=s,k_r,k_s,k_n,N]    With --resident: smoothed centres and anisotropy (Yu & Turk 2013) of the final\n"
          "                                        state, computed on the device; ellipsoids.ply beside cloud.ply (centre, three\n"
          "                                        radii, three axes and the neighbour count per fluid particle). Defaults:\n"
          "                                        0.9,4,6.6667,0.5,25. Single device only\n"
          "      --anisotropic-surface=[iso[,s,k_r,k_s,k_n,N]]  With --resident: the frames' surface is the iso-surface of Yu &\n"
          "                                        Turk's anisotropic-kernel field over those ellipsoids at isolevel iso (no\n"
          "                                        default: its scale is not the stock field's; 0.3 ... 0.6 suits a fluid at\n"
          "                                        rest density), at the stock resolution. Combines with --indexed-mesh;\n"
          "                                        mesh.obj as before. Single device only\n"
          "      --indexed-mesh                    Extract the surface as an indexed mesh (one vertex per crossed lattice\n"
          "                                        edge, watertight by index); mesh.obj becomes an indexed OBJ.\n"
          "                                        Single device only\n"
          "      --diagnostics[=every]             With --resident: after every [every]-th timed frame (default 1) one JSON\n"
          "                                        line {\"frame\":..,\"diag\":{..}} of the device-side diagnostics (sums,\n"
          "                                        extrema, density residual); outside the timed interval. Single device only\n"
          "      --probe=[x,y,z]                   With --resident (repeatable): density, velocity and colour sampled at the\n"
          "                                        world point on the device; one JSON line {\"frame\":..,\"probes\":[..]} per\n"
          "                                        report, outside the timed interval. Single device only\n"
          "      --probe-every=[k]                 Report the probes after every k-th timed frame.\n"
          "                                        Default: once, after the last timed frame\n"
          "      --source=[x,y,z,vx,vy,vz,rate[,tag]]  An inlet (repeatable): a floor x ceil sheet of sqrt(rate) particles\n"
          "                                        per frame at the world point, with that velocity. With --resident\n"
          "                                        emitted on the GPU, otherwise by advance(). Single device only\n"
          "      --drain=[x,y,z,width]             An outlet (repeatable): fluid closer than width to the point leaves\n";
  }

  static std::vector<double> numbers(const std::string &list) {  // "a,b,c" -> {a, b, c}
    std::vector<double> out;
    for (size_t at = 0; at <= list.size();) {
      const size_t comma = std::min(list.find(',', at), list.size());
      out.push_back(std::stod(list.substr(at, comma - at)));
      at = comma + 1;
    }
    return out;
  }

  // one grammar and one parser for --collider and --scenery (`flag` names the option in the messages)
  static void parseSolid(const std::string &flag, const std::string &v, Solid &s) {
    const size_t colon = v.find(':');
    const std::string shape = v.substr(0, colon);
    if (colon != std::string::npos && shape == "mesh") {
      const size_t comma = v.find(',', colon);
      s.mesh = v.substr(colon + 1, comma == std::string::npos ? std::string::npos : comma - colon - 1);
      std::string rest = comma == std::string::npos ? std::string() : v.substr(comma + 1);
      const std::string word = ",winding";  // the fifth field, as a word
      const bool byWord = rest.size() > word.size() && rest.compare(rest.size() - word.size(), word.size(), word) == 0;
      if (byWord) rest.resize(rest.size() - word.size());
      const auto f = rest.empty() ? std::vector<double>{} : numbers(rest);
      if (s.mesh.empty() || f.size() > (byWord ? 3u : 4u) || (byWord && f.size() != 3))
        throw std::runtime_error(flag + ": expected mesh:FILE.obj[,margin[,spacing[,negate[,winding]]]]");
      s.shape = shape;
      if (f.size() > 0) s.margin = f[0];
      if (f.size() > 1) s.spacing = f[1];
      if (f.size() > 2) s.negate = f[2] != 0;
      s.winding = byWord || (f.size() > 3 && f[3] != 0);
      if (!(s.margin >= 0) || !(s.spacing >= 0)) throw std::runtime_error(flag + ": margin and spacing must be >= 0");
      return;
    }
    if (colon == std::string::npos || (shape != "sphere" && shape != "bowl" && shape != "plane"))
      throw std::runtime_error(flag + ": expected sphere:cx,cy,cz,r | bowl:cx,cy,cz,r | plane:nx,ny,nz,d [,margin[,spacing]]");
    const auto f = numbers(v.substr(colon + 1));
    if (f.size() < 4 || f.size() > 6) throw std::runtime_error(flag + ": expected four numbers and optionally margin, spacing");
    s.shape = shape;
    for (int k = 0; k < 4; ++k) s.cfg[k] = f[size_t(k)];
    if (f.size() > 4) s.margin = f[4];
    if (f.size() > 5) s.spacing = f[5];
    if (shape != "plane" && !(s.cfg[3] > 0)) throw std::runtime_error(flag + ": the radius must be > 0");
    if (shape == "plane" && !(f[0] * f[0] + f[1] * f[1] + f[2] * f[2] > 0)) throw std::runtime_error(flag + ": the normal must not be zero");
    if (!(s.margin >= 0) || !(s.spacing >= 0)) throw std::runtime_error(flag + ": margin and spacing must be >= 0");
  }

  // returns false if the program should exit (help / parse error), like the reference's parse()
  bool parse(int argc, char *argv[]) {
    auto value = [&](int &i, const std::string &arg, const std::string &shortF, const std::string &longF,
                     std::string &out) -> bool {
      if (arg == shortF || arg == longF) {
        if (i + 1 >= argc) throw std::runtime_error("Flag '" + arg + "' requires an argument");
        out = argv[++i];
        return true;
      }
      if (!shortF.empty() && arg.rfind(shortF, 0) == 0 && arg.size() > shortF.size() && arg[1] != '-') {
        out = arg.substr(shortF.size());
        return true;
      }
      if (arg.rfind(longF + "=", 0) == 0) {
        out = arg.substr(longF.size() + 1);
        return true;
      }
      return false;
    };
    try {
      for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        std::string v;
        if (a == "-h" || a == "--help") {
          usage(std::cout);
          return false;
        } else if (a == "-l" || a == "--list") list = true;
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--fp64") fp64 = true;
        else if (a == "--resident") resident = true;
        else if (a == "--no-surface") surface = false;
        else if (a == "--fast-math") fastMath = true;
        else if (a == "--json") json = true;
        else if (a == "--all-devices") allDevices = true;
        else if (a == "--indexed-mesh") indexedMesh = true;
        else if (a == "--anisotropy") anisotropy = true;
        else if (a.rfind("--anisotropy=", 0) == 0) {
          const auto f = numbers(a.substr(13));
          if (f.size() != 5 || !(f[4] >= 0)) throw std::runtime_error("--anisotropy: expected smoothing,k_r,k_s,k_n,min_neighbours");
          anisotropy = true;
          for (int k = 0; k < 4; ++k) anisoCfg[k] = f[size_t(k)];
          anisoMinNeighbours = unsigned(f[4]);
        }
        else if (a.rfind("--anisotropic-surface=", 0) == 0) {
          const auto f = numbers(a.substr(22));
          if ((f.size() != 1 && f.size() != 6) || (f.size() == 6 && !(f[5] >= 0)))
            throw std::runtime_error("--anisotropic-surface: expected isolevel[,smoothing,k_r,k_s,k_n,min_neighbours]");
          anisoSurface = true, anisoSurfaceIso = f[0];
          if (f.size() == 6) {
            for (int k = 0; k < 4; ++k) anisoSurfaceCfg[k] = f[size_t(k) + 1];
            anisoSurfaceMinNeighbours = unsigned(f[5]);
          }
        }
        else if (a == "--diagnostics") diagnostics = 1;
        else if (a.rfind("--diagnostics=", 0) == 0) {
          diagnostics = std::stoull(a.substr(14));
          if (diagnostics == 0) throw std::runtime_error("--diagnostics: every must be >= 1");
        }
        else if (value(i, a, "", "--slabs", v)) slabs = std::stoull(v);
        else if (value(i, a, "", "--probe-every", v)) {
          probeEvery = std::stoull(v);
          if (probeEvery == 0) throw std::runtime_error("--probe-every: k must be >= 1");
        }
        else if (value(i, a, "", "--probe", v)) {
          const auto f = numbers(v);
          if (f.size() != 3) throw std::runtime_error("--probe: expected x,y,z");
          probes.push_back({f[0], f[1], f[2]});
        }
        else if (a == "--whitewater-solids") wwSolids = true;
        else if (a.rfind("--whitewater-solids=", 0) == 0) {
          const auto f = numbers(a.substr(20));
          if (f.empty() || f.size() > 3) throw std::runtime_error("--whitewater-solids: expected restitution[,friction[,absorb]]");
          if (!(f[0] >= 0 && f[0] <= 1) || (f.size() >= 2 && !(f[1] >= 0 && f[1] <= 1)) || (f.size() == 3 && f[2] != 0 && f[2] != 1))
            throw std::runtime_error("--whitewater-solids: restitution and friction in [0, 1], absorb 0 or 1");
          wwSolids = true;
          for (size_t k = 0; k < f.size(); ++k) wwSolidsCfg[k] = f[k];
        }
        else if (value(i, a, "", "--whitewater", v)) {
          const auto f = numbers(v);
          if (f.size() < 2 || f.size() > 3) throw std::runtime_error("--whitewater: expected k_ta,k_wc[,capacity]");
          wwTa = f[0], wwWc = f[1];
          wwCapacity = f.size() == 3 ? size_t(f[2]) : size_t(262144);
          if (!(wwTa >= 0 && wwWc >= 0) || wwCapacity == 0) throw std::runtime_error("--whitewater: rates must be >= 0, capacity >= 1");
        }
        else if (value(i, a, "", "--collider-motion", v)) {
          const auto f = numbers(v);
          if (f.size() != 3 && f.size() != 6 && f.size() != 9) throw std::runtime_error("--collider-motion: expected vx,vy,vz[,wx,wy,wz[,px,py,pz]]");
          for (double x : f)
            if (!std::isfinite(x)) throw std::runtime_error("--collider-motion: the values must be finite");
          colliderMoves = true;
          for (size_t k = 0; k < f.size(); ++k) colliderMotion[k] = f[k];
        }
        else if (a == "--collider-friction-report") colliderFrictionReport = 1;
        else if (a.rfind("--collider-friction-report=", 0) == 0) {
          colliderFrictionReport = std::stoull(a.substr(27));
          if (colliderFrictionReport == 0) throw std::runtime_error("--collider-friction-report: every must be >= 1");
        }
        else if (value(i, a, "", "--collider-friction", v)) {
          const auto f = numbers(v);
          if (f.size() != 1) throw std::runtime_error("--collider-friction: expected mu");
          if (!(f[0] > 0)) throw std::runtime_error("--collider-friction: mu must be > 0 (inf = no-slip)");
          colliderFriction = f[0];
        }
        else if (a == "--collider-body-contact") colliderBodyContact = true;
        else if (a.rfind("--collider-body-contact=", 0) == 0) {
          const auto f = numbers(a.substr(24));
          if (f.empty() || f.size() > 3) throw std::runtime_error("--collider-body-contact: expected restitution[,mu[,iterations]]");
          for (double x : f)
            if (!std::isfinite(x)) throw std::runtime_error("--collider-body-contact: the values must be finite");
          if (f[0] < 0 || f[0] > 1 || (f.size() >= 2 && f[1] < 0) || (f.size() == 3 && (f[2] < 1 || f[2] > 8 || f[2] != std::floor(f[2]))))
            throw std::runtime_error("--collider-body-contact: restitution in [0, 1], mu >= 0, iterations 1..8");
          colliderBodyContact = true;
          for (size_t k = 0; k < f.size(); ++k) colliderBodyContactCfg[k] = f[k];
        }
        else if (a == "--collider-body-report") colliderBodyReport = 1;
        else if (a.rfind("--collider-body-report=", 0) == 0) {
          colliderBodyReport = std::stoull(a.substr(23));
          if (colliderBodyReport == 0) throw std::runtime_error("--collider-body-report: every must be >= 1");
        }
        else if (value(i, a, "", "--collider-body", v)) {
          const auto f = numbers(v);
          if (f.size() != 1 && f.size() != 4 && f.size() != 5) throw std::runtime_error("--collider-body: expected mass[,Ixx,Iyy,Izz[,gain]]");
          for (double x : f)
            if (!std::isfinite(x)) throw std::runtime_error("--collider-body: the values must be finite");
          if (!(f[0] > 0) || (f.size() >= 4 && !(f[1] > 0 && f[2] > 0 && f[3] > 0)) || (f.size() == 5 && f[4] < 0))
            throw std::runtime_error("--collider-body: mass and moments must be > 0, gain >= 0");
          colliderBody = true;
          for (size_t k = 0; k < f.size(); ++k) colliderBodyCfg[k] = f[k];
        }
        else if (a == "--collider-reaction") colliderReaction = 1;
        else if (a.rfind("--collider-reaction=", 0) == 0) {
          colliderReaction = std::stoull(a.substr(20));
          if (colliderReaction == 0) throw std::runtime_error("--collider-reaction: every must be >= 1");
        }
        else if (value(i, a, "", "--collider", v)) parseSolid("--collider", v, solid);
        else if (value(i, a, "", "--scenery", v)) parseSolid("--scenery", v, scenery);
        else if (value(i, a, "", "--surface-tension", v)) {
          const size_t comma = v.find(',');
          cohesion = std::stod(v.substr(0, comma));
          adhesion = comma == std::string::npos ? 0.0 : std::stod(v.substr(comma + 1));
          if (!(cohesion >= 0 && adhesion >= 0)) throw std::runtime_error("--surface-tension: values must be >= 0");
        }
        else if (value(i, a, "", "--source", v)) {
          // (the tag is an id: parsed as an integer of its own, not through a double)
          size_t commas = 0, last = std::string::npos;
          for (size_t k = 0; k < v.size(); ++k)
            if (v[k] == ',') ++commas, last = k;
          if (commas != 6 && commas != 7) throw std::runtime_error("--source: x,y,z,vx,vy,vz,rate[,tag]");
          unsigned long long tag = 1000000ull + sources.size();
          if (commas == 7) {
            const std::string t = v.substr(last + 1);
            size_t used = 0;
            if (t.empty() || t[0] == '-') throw std::runtime_error("--source: tag must be a non-negative integer");
            tag = std::stoull(t, &used);
            if (used != t.size()) throw std::runtime_error("--source: tag must be a non-negative integer");
            v = v.substr(0, last);
          }
          const std::vector<double> f = numbers(v);
          if (!(f[6] >= 0)) throw std::runtime_error("--source: rate must be >= 0");
          sources.push_back({{f[0], f[1], f[2], f[3], f[4], f[5], f[6]}, tag});
        }
        else if (value(i, a, "", "--drain", v)) {
          const std::vector<double> f = numbers(v);
          if (f.size() != 4) throw std::runtime_error("--drain: x,y,z,width");
          if (!(f[3] >= 0)) throw std::runtime_error("--drain: width must be >= 0");
          drains.push_back({f[0], f[1], f[2], f[3]});
        }
        else if (value(i, a, "-i", "--impl", v)) impl = v;
        else if (value(i, a, "-d", "--devices", v)) devices.push_back(v);
        else if (value(i, a, "-n", "--iter", v)) iterations = std::stoull(v);
        else if (value(i, a, "-w", "--warmup", v)) warmup = std::stoull(v);
        else if (value(i, a, "-o", "--output", v)) output = v;
        else if (value(i, a, "", "--particles", v)) particles = std::stoull(v);
        else if (value(i, a, "", "--solver-iter", v)) solverIter = std::stoull(v);
        else if (value(i, a, "", "--scene", v)) scene = v;
        else throw std::runtime_error("Flag could not be matched: " + a);
      }
      if (scene != "cubes" && scene != "dam-break") throw std::runtime_error("Unknown scene: " + scene);
    } catch (const std::exception &e) {
      std::cerr << e.what() << std::endl;
      usage(std::cerr);
      return false;
    }
    if (devices.empty()) devices.push_back("0");
    return true;
  }

  std::string renderedOutputName() const {  // src/args.cpp:69-75
    auto replace = [](std::string s, const std::string &from, const std::string &to) {
      for (size_t pos = 0; (pos = s.find(from, pos)) != std::string::npos; pos += to.size()) s.replace(pos, from.size(), to);
      return s;
    };
    std::string name = output;
    name = replace(name, "{iter}", std::to_string(iterations));
    name = replace(name, "{type}", fp64 ? "fp64" : "fp32");
    name = replace(name, "{impl}", impl);
    return name;
  }
};

}  // namespace sph::driver

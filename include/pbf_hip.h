/*
 * pbf_hip.h — C ABI of libpbf_hip.so: the MI355X (gfx950) implementation of the PBF-SPH
 * per-step hot path behind the reference's Solver::advance() surface.
 *
 * The reference has no FFI: its backends are C++ classes chosen by a switch
 * (src/benchmark.cpp:105-172) behind
 *     sph::Solver<T,N,V>::advance(const SphParams&, const Scene&, std::vector<Particle>&)
 * (src/sph.hpp:119-125).  This header is the boundary a maintainer binds a new backend to;
 * pbf-sph_amd/host/hipsph.hpp is that binding (sph::hip_impl::Solver<T,N>, a thin shim), and
 * INTEGRATION.md shows the lines to add to the reference's benchmark.cpp / args.hpp.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returns 0 on
 * success or a negative pbf_status; pbf_last_error() gives the text.  Nothing throws across
 * the ABI (reference: exceptions, src/benchmark.cpp:32-37).  One ctx = one caller thread at a
 * time (the reference's advance() has no thread-safety contract either, src/visualise.cpp:85-109).
 * Arrays are caller-owned SoA: pos/vel 3 per particle, colour 4 per particle, element type
 * float (fp64 = 0) or double (fp64 = 1) as chosen in pbf_desc (reference: template parameter N,
 * src/specialisation.cpp:13-14).  ids are uint64 (reference T = size_t).
 */
#ifndef PBF_HIP_H
#define PBF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBF_ABI_VERSION 1

typedef struct pbf_ctx pbf_ctx;

typedef enum pbf_status {
  PBF_OK = 0,
  PBF_ERR_INVALID = -1,   /* bad argument */
  PBF_ERR_HIP = -2,       /* a HIP runtime call failed (text in pbf_last_error) */
  PBF_ERR_NO_DEVICE = -3, /* no gfx950 device / HIP runtime unusable: the product path never falls back to CPU */
  PBF_ERR_STATE = -4,     /* call order violated (e.g. stage before upload) */
  PBF_ERR_COMM = -5,      /* RCCL failure */
} pbf_status;

/* sph::Type (src/sph.hpp:15) */
enum { PBF_TYPE_FLUID = 0, PBF_TYPE_OBSTACLE = 1 };

enum {
  PBF_FLAG_STAGE_TIMING = 1u << 0, /* record hipEvents around every stage (Stopwatch analogue, src/utils.hpp:15-57) */
  PBF_FLAG_FAST_MATH = 1u << 1,    /* v_rsq/v_rcp in the pair kernels (the reference itself ships -Ofast,
                                      CMakeLists.txt:136, and native_divide/fast_distance in OpenCL) */
  PBF_FLAG_NO_LDS = 1u << 2,       /* force the per-particle global-memory gather kernels (debug / A-B) */
};

/* Replaces the ctor  omp_impl::Solver<T,N>(N h)  (src/omp/ompsph.hpp:83). */
typedef struct pbf_desc {
  uint32_t abi_version; /* PBF_ABI_VERSION */
  int32_t fp64;         /* 0: N = float, 1: N = double (benchmark --fp64, src/args.cpp:34-37) */
  int32_t device;       /* HIP device ordinal (benchmark -d, src/args.cpp:20-24) */
  uint32_t flags;       /* PBF_FLAG_* */
  double h;             /* smoothing length; benchmark.cpp:160-163 passes 0.1 */
  void *stream;         /* hipStream_t to launch on; NULL = a stream owned by the ctx */
} pbf_desc;

/* Replaces sph::SphParams (src/sph.hpp:97-103) + sph::Scene::wells (src/sph.hpp:56-60,76).
 * SphParams::h is dead in the reference (src/sph.hpp:98, never read) and therefore absent. */
typedef struct pbf_params {
  double dt, scale;
  uint64_t iteration;       /* solver iterations K */
  double constant_force[3];
  double min_bound[3], max_bound[3];
  int32_t n_wells;
  const double *wells;      /* n_wells x {cx, cy, cz, force}, host */
  int32_t xsph, vorticity;  /* opt-in, NOT in the reference (only constants survive, src/sph_constants.h:13-14) */
} pbf_params;

/* ---- lifetime -------------------------------------------------------------------------- */
int pbf_create(const pbf_desc *desc, pbf_ctx **out);
void pbf_destroy(pbf_ctx *ctx);
/* ctx may be NULL: last error of a failed pbf_create on this thread */
const char *pbf_last_error(const pbf_ctx *ctx);
int pbf_abi_version(void);
/* Tuning / diagnostic knobs (no reference counterpart): "gather" (0 global walk, 1 neighbour lists = default, 3 LDS tiles
 * per brick), "list_max", "tile_cap", "reuse_lists", "split_build" (0 = lambda builds the lists while it gathers; 4 / 5 = a
 * list-build launch of its own with 2 / 4 pair loads per trip, then a list-driven lambda; 8 = DEFAULT: the quantised list
 * build with lambda riding on its flushes, one launch — the same build kernel either way, with or without a rider), "coop" (0 = one lane per particle in the list-driven lambda /
 * delta-p, bit-exact, default; 2 / 4 / 8 = that many lanes share a particle's list and reduce the kernel sums with wave
 * shuffles: rounding-level differences), "cell_diffuse" (one colour walk per occupied cell, default 1), "fuse_diffuse",
 * "overlap_diffuse", "fuse_predict", "pipeline", "graph", "pad_lds", "timing_mask" (bit i = stage i of pbf_stage_times is
 * bracketed with events), "row_major" (DEFAULT 1: the solver iterations run on a cell-ROW-major copy of {pStar, lambda,
 * quantised position, mass, type} — one contiguous run per (dy, dz) row of the 27-cell stencil, lists of row slots; 0 =
 * everything in Morton order), "nbr_chunks" (size of the pool of 120-slot overflow chunks of the two-tier neighbour lists;
 * 0 = sized from the particle count), "row_diffuse" (DEFAULT 1, with row_major: the colour diffusion walks the row-major copy, one
 * wave per segment of 64 x cells, runs staged by LDS-DMA, sums applied in place; 0 = per-cell sums on the Morton order, beside
 * the iterations), "diffuse_cap" (diagnostic: records in that kernel's LDS tile, 0 = default 640), "build_wg" / "reader_wg" / "iter_wg" (with
 * row_major: the workgroup width of the row list build — DEFAULT 64, one wave per workgroup, so that each wave's staging LDS
 * goes back to the CU when that wave ends —, of the row delta-p reader — DEFAULT 256 —, or of both; 64, 128 or 256, anything
 * else PBF_ERR_INVALID; the lists are the same at every width, so it may change between any two launches), "sdf_cull" (pbf_sdf_from_mesh / pbf_set_collider_mesh only: 1 = a wave skips the
 * triangles whose bounding sphere is out of its brick's reach; DEFAULT 1, 0 = every pair), "sdf_launch_pairs" (diagnostic, the
 * same calls and pbf_mesh_winding: the cap on lane-triangle pairs per launch of the distance fold and of the winding fold,
 * 0 = the default, 2^33 for the distance; a small cap lets a test reach the split across launches).  Every setting of these
 * is bit-identical.  Unknown names return PBF_ERR_INVALID. */
int pbf_set_option(pbf_ctx *ctx, const char *name, int64_t value);

/* Opt-in surface tension and adhesion after Akinci, Akinci & Teschner 2013, "Versatile Surface Tension and Adhesion for
 * SPH Fluids" (ACM TOG 32(6)); no reference counterpart.  A post-solve velocity correction that runs last among the extras
 * (after vorticity confinement and XSPH, whose results it does not change), in three neighbour passes over the final pStar
 * (solver frame: world / scale, h = pbf_desc.h, m = particle mass, rho0 = 6378):
 *   rho_i = sum_{j in N(i) u {i}} m_j W_poly6(r)   (obstacles included);   n_i = h sum_{fluid j != i} (m_j / rho_j) grad W_spiky
 *   v_i += -dt [ sum_fluid j  K_ij (cohesion m_j C(r) x_ij / r + cohesion (n_i - n_j))  +  sum_obstacle b  adhesion m_b A(r) x_ib / r ]
 * with K_ij = 2 rho0 / (rho_i + rho_j), C Akinci's cohesion spline and A his adhesion kernel (both zero beyond h, A also
 * below h / 2).  Akinci's boundary pseudo-mass Psi_b is replaced by the obstacle particle's mass.  Obstacle velocities are
 * unchanged.  The setting persists in the ctx (default 0 / 0 = off; on when either is > 0) and applies to every later
 * pbf_step / pbf_steps (hipGraph replays included: the coefficients are part of a captured step's key).  NaN, infinite or
 * negative values return PBF_ERR_INVALID.  Slab mode is not supported: enabling it on a slab-attached ctx, and
 * pbf_slab_step / a slab-mode finalise with it enabled, return PBF_ERR_STATE. */
int pbf_set_surface_tension(pbf_ctx *ctx, double cohesion, double adhesion);

/* Opt-in static collider: a signed-distance lattice that delta-p projects the fluid out of, so that a bowl, a ramp or a
 * pillar needs no obstacle particles (no reference counterpart).  Default off: with no collider set every launch and every
 * byte of a step is what it is without this feature.
 *
 * pbf_set_collider copies the lattice to the device, rounded to N (float / double as the ctx), together with N(origin),
 * inv = N(1) / N(spacing) and N(margin).  The setting persists in the ctx and applies to every later pbf_stage_delta,
 * pbf_step and pbf_steps (hipGraph replays included: every call, clearing too, changes a captured step's key, so a replay
 * never uses a stale lattice).  It allocates nothing inside a step.  sdf == NULL clears the collider and frees the lattice.
 * PBF_ERR_INVALID, the setting unchanged: a dim < 2; a dims product >= 2^31; a non-finite origin, spacing or margin;
 * spacing <= 0; margin < 0; phi == NULL; a NaN in phi (infinities are legal: "no solid anywhere near").
 * Slab mode is not supported (a collider across slabs is out of scope): setting one on a slab-attached or slab-configured
 * ctx, and pbf_slab_step(s) / a delta-p stage of a slab-configured ctx with one set, return PBF_ERR_STATE.
 *
 * The contract.  One device function (csrc/pbf_collider.hpp) is shared by delta-p's epilogue and pbf_collider_sample.
 * Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it.  The input is the q that
 * delta-p computes without a collider: after the world-frame box clamp and the division by scale.
 *   w_a = q_a * scale                         u_a = (w_a - origin_a) * inv
 *   inside = for every a: u_a >= 0 && u_a <= N(dims_a - 1)            (NaN compares false: outside)
 *   i_a = min(int(u_a), dims_a - 2)           f_a = u_a - N(i_a)       (the last node: i = dims - 2, f = 1)
 *   c[x][y][z] = the eight nodes (i_x + x, i_y + y, i_z + z)
 *   d[x][y]  = c[x][y][1] - c[x][y][0]        cz[x][y] = c[x][y][0] + f_z * d[x][y]
 *   e[x]     = cz[x][1] - cz[x][0]            cy[x]    = cz[x][0] + f_y * e[x]
 *   g_x = cy[1] - cy[0]                       phi = cy[0] + f_x * g_x
 *   g_y = e[0] + f_x * (e[1] - e[0])
 *   t[x] = d[x][0] + f_y * (d[x][1] - d[x][0])     g_z = t[0] + f_x * (t[1] - t[0])
 *   len = sqrt((g_x g_x + g_y g_y) + g_z g_z)       (IEEE sqrt)
 *   hit = inside && phi < margin && len > 0
 *   s = (margin - phi) / len                         (IEEE divide)
 *   q'_a = hit ? min(maxB_a / scale, max(minB_a / scale, (w_a + s * g_a) / scale)) : q_a
 * g is the gradient of the trilinear interpolant in lattice units; the spacing is isotropic, so only its direction
 * matters.  A particle that does not hit keeps its q bit for bit (a select).  The second clamp uses the images of the box
 * under the stock clamp, so the box always wins over the collider.  The stored lambda is untouched; the quantised copy of
 * pStar is formed from q'.  Obstacles and ghost copies are never moved.  One projection runs per delta-p iteration; the K
 * iterations converge it.  Every gather path ("gather" 0 / 1 / 3, "row_major", "pipeline", "graph", PBF_FLAG_NO_LDS)
 * gives the same bytes; "coop" 2 / 4 / 8 differs at rounding level as it does without a collider.
 * Limitations: there is no restitution term — finalise derives the velocity from the projected position, as it does for
 * the box — and friction is an opt-in pass of its own (pbf_set_collider_friction below).  Whitewater's diffuse particles
 * see the collider only with pbf_set_whitewater_solids on (below); the observers (surface, sampling, diagnostics,
 * anisotropy) do not see it.  One collider and one static scenery lattice (pbf_set_scenery below) per ctx.  A
 * triangle mesh becomes a lattice through pbf_sdf_from_mesh / pbf_set_collider_mesh below.
 *
 * pbf_collider_sample is the window onto that device function, for debugging an uploaded collider: its own synchronising
 * call, never part of a step.  For each point: round to N, q = point / scale in N, then exactly the function above with
 * params' scale and bounds.  phi receives the interpolated value (+inf outside the lattice), moved the q' delta-p would
 * store, hit whether the point was projected; any output pointer may be NULL.  A non-finite point is legal: it is outside,
 * hit = 0, moved = its q.  PBF_ERR_INVALID: params == NULL; points == NULL with n > 0; dt or scale <= 0; n >= 2^31.  n == 0
 * then returns PBF_OK and launches nothing.  PBF_ERR_STATE without a collider. */
typedef struct pbf_collider_sdf {
  uint32_t dims[3];   /* nodes per axis, each >= 2; dims[0]*dims[1]*dims[2] < 2^31 */
  double origin[3];   /* world position of node (0,0,0) */
  double spacing;     /* world units between nodes, the same on all three axes, > 0 */
  double margin;      /* fluid is kept at phi >= margin (world units), >= 0 */
  const void *phi;    /* host, N[dims product] (float / double as the ctx), node (i,j,k) at (i*dims[1]+j)*dims[2]+k —
                         pbf_sample_lattice's order; signed distance in world units, NEGATIVE inside the solid */
} pbf_collider_sdf;
int pbf_set_collider(pbf_ctx *ctx, const pbf_collider_sdf *sdf);   /* NULL clears and frees the lattice */
int pbf_collider_sample(pbf_ctx *ctx, const pbf_params *params, size_t n, const double *points /* 3n, world */,
                        void *phi /* N[n] */, void *moved /* N[3n], solver frame */, uint8_t *hit /* [n] */);

/* Moving colliders: a rigid pose for the installed lattice (no reference counterpart).  Opt-in: until the first call the
 * collider is the static one above, kernels and arguments included.
 *
 * With a pose the lattice is read in a body frame: a world point is w = R b + t.  The shape does not change, only its
 * placement, so a paddle, a piston or a gate moves with one call per frame instead of a lattice upload.  The pose persists
 * until it is changed and applies to every later pbf_stage_delta, pbf_step and pbf_steps (hipGraph replays included) and
 * to pbf_collider_sample, which stays the window onto the very function delta-p runs.  Within one pbf_steps(count) call
 * the pose is constant, unless a body is on (pbf_set_collider_body below): then every step ends by writing the pose of the
 * next.  pose == NULL returns to the static collider.  pbf_set_collider and pbf_set_collider_mesh,
 * clearing included, reset the pose to "none".
 *
 * The call does not synchronise and uploads no lattice: the ctx keeps one record {N(R), N(t)} on the device, and the call
 * writes it with a one-lane kernel on the ctx's stream, in stream order with the steps already queued and those to come.
 * The posed kernels read the record through a pointer, so a new pose changes no argument of a captured step: an update
 * drops no graph and causes no recapture.  Going between "none" and a pose selects other kernels, so it changes a captured
 * step's key and drops the captured graphs as pbf_set_collider does (and synchronises, once).
 *
 * Refusals, all of which leave the pose and the state unchanged.  PBF_ERR_INVALID: pose != NULL with a non-finite entry;
 * max |R^T R - I| > 1e-5 evaluated in double (a stated condition of the interface, loose enough for a matrix composed in
 * float); det R < 0 (a reflection).  PBF_ERR_STATE: no collider is installed; the slab cases pbf_set_collider refuses.  The
 * library does not re-orthonormalise: it uses N(R) and N(t) as given.  The check is plain host code
 * (csrc/pbf_collider_pose.hpp).
 *
 * The contract with a pose (csrc/pbf_collider.hpp).  Everything is in N, in the order written, not contracted;
 * PBF_FLAG_FAST_MATH does not reach it.  q is the input of the static contract above.
 *   w_a  = q_a * scale                         d_a = w_a - t_a
 *   b_a  = (R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2                 (R^T d)
 *   u_a  = (b_a - origin_a) * inv
 *   ... inside, i, f, the eight nodes, phi, g, len, hit, s: exactly the static contract, on u ...
 *   b'_a = b_a + s * g_a
 *   w'_a = ((R[a][0] b'_0 + R[a][1] b'_1) + R[a][2] b'_2) + t_a
 *   q'_a = hit ? min(maxB_a / scale, max(minB_a / scale, w'_a / scale)) : q_a
 * A particle that does not hit keeps its bits; outside the lattice, NaN included, nothing is loaded.  The margin and the
 * spacing are lengths, so a rotation leaves them alone.  The box is the world's: the second clamp is not rotated.
 * Limitations: the wall pushes through positions and is free-slip unless pbf_set_collider_friction (below) is on, which is
 * also the only place the solid's contact velocity enters; there is no restitution, and finalise derives the velocity
 * from the projected position with the reference's damping.  There is no swept collision: a body that moves further per
 * step than its own thickness can pass through fluid.  One collider per ctx; no pose across slabs; whitewater sees the
 * posed collider only with pbf_set_whitewater_solids on (below), the observers do not see it. */
typedef struct pbf_collider_pose {
  double rot[9];     /* row-major R, body -> world */
  double trans[3];   /* t, world */
} pbf_collider_pose;
int pbf_set_collider_pose(pbf_ctx *ctx, const pbf_collider_pose *pose);   /* NULL: back to the static collider */

/* The reaction: what the collider did to the fluid in the last step, per particle and summed — the other half of a coupling
 * to a rigid-body solver (no reference counterpart).  Opt-in: pbf_set_collider_reaction(ctx, 1) allocates two vec4 of N per
 * particle at the ctx's capacity (regrown by an upload that grows it; nothing is allocated inside a step) and selects the
 * delta-p kernels that keep the records; 0 returns to the kernels without them.  Either change alters a captured step's key
 * and drops the captured graphs, as pbf_set_collider does.  PBF_ERR_STATE in slab mode.
 *
 * Per particle.  With the reaction on, delta-p runs the posed contract above (the identity pose while none is set: the
 * state then compares equal to the static collider's, a zero may change its sign) and a lane that HITS updates the record
 * of its particle, in N, after q':
 *   delta_a = (q'_a - q_a) * scale                r_a = q'_a * scale - t_a
 *   A_a += delta_a                                hits += 1          (kept as N)
 *   B_x += r_y * delta_z - r_z * delta_y          (y, z cyclic; each product rounded, one subtraction, one add)
 * A lane that does not hit stores nothing.  The records are cleared once per step by the sort stage (pbf_stage_sort,
 * pbf_step, every step of pbf_steps; the clear is captured with the step), when the device order they are indexed by is
 * established; every delta-p launch until the next sort accumulates into them.  PBF_BUF_COLLIDER_PUSH reads them back
 * through pbf_read_buffer: N[8n] = {A.xyz, hits, B.xyz, 0} per particle in the device (Morton) order of PBF_BUF_PSTAR,
 * whichever gather path ran.  PBF_ERR_STATE while the records do not describe the current arrays.
 *
 * The sum.  pbf_collider_reaction is an observer call of its own between steps (it synchronises; it is not part of a step
 * or a captured graph and changes nothing a step reads): P = sum_i m_i A_i and L = sum_i m_i B_i, raw sums as the sampling
 * calls return them, with L taken about the pose's t (about the world origin without a pose).  The body received -P and
 * -L; dividing by dt^2 to get a force is the caller's business.  Finalise derives the velocity from the projected position
 * with the reference's damping, and the figure is the usual position-based estimate, not a pressure integral.  The
 * reduction has the diagnostics' fixed shape (no atomics, particles taken in the Morton order, terms formed in double):
 * the same state gives the same bytes on every gather path and in every run.  PBF_ERR_STATE: the reaction is not enabled;
 * no collider is set; no step has run since enabling (or the arrays have changed since the last one); slab mode. */
int pbf_set_collider_reaction(pbf_ctx *ctx, int on);
typedef struct pbf_collider_wrench {
  double impulse[3];      /* P = sum_i m_i A_i   (mass x world displacement the collider gave the fluid) */
  double angular[3];      /* L = sum_i m_i B_i   (about the pose's t; about the world origin without a pose) */
  double abs_impulse[3], abs_angular[3];   /* sums of |term|: what the rounding of P and L scales with */
  uint64_t hits;          /* projections, summed over particles and iterations */
  uint64_t particles;     /* particles with at least one */
  uint64_t step;          /* serial of the step the record belongs to: steps run since the reaction was enabled */
} pbf_collider_wrench;
int pbf_collider_reaction(pbf_ctx *ctx, pbf_collider_wrench *out);

/* Floating bodies: the collider's rigid body integrated on the device (no reference counterpart) — the first half of the
 * coupling whose other half is the reaction above.  Opt-in: a ctx that never calls pbf_set_collider_body launches what it
 * always did.
 *
 * With a body on, every step (pbf_step, every step of pbf_steps, hipGraph replays included) runs one more stage after its
 * delta-p iterations and before finalise: the reaction records are summed by the reduction of pbf_collider_reaction (the
 * same partial kernel and the same fold, so the sums are the bytes that call would return for the step), and one workgroup
 * advances the body and writes the pose record the posed delta-p kernels read through a pointer.  There is no host
 * read-back in a step and no new kernel argument that changes per step: the step is captured once and replayed, and
 * pbf_steps(ctx, p, 200) runs 200 two-way coupled steps.  With iteration == 0 the records are the sort's zeros and the
 * body moves under accel alone.  A step that returns early because the particles are depleted does not advance the body.
 *
 * The contract (csrc/pbf_collider_body.hpp, plain C++ shared by the kernel and a stand-alone host program).  Everything is
 * in double whatever the ctx's N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it.  State: x
 * (centre of mass, world units; the pose's t — the body frame's origin is the centre of mass), q (unit quaternion w, x, y,
 * z, body -> world), v (world units per time), w (angular velocity, world frame, rad per time).  The body's principal axes
 * are the lattice's axes.  One advance takes dt = pbf_params.dt and the step's raw sums P, L (pbf_collider_wrench.impulse
 * and .angular; L about the t the step's delta-p launches read):
 *   R      = R(q)                     (each entry written out in csrc/pbf_collider_body.hpp)
 *   J_a    = -(gain * P_a) / dt       H_a = -(gain * L_a) / dt
 *            one non-finite J or H: all six count as zero for this step and `rejected` goes up by one
 *   v'_a   = ((v_a + dt * accel_a) + J_a / mass) * linear_factor_a / (1 + dt * linear_damping)
 *   h      = R^T H ;  k_b = h_b / inertia_b ;  w'_a = ((w_a + (R k)_a) * angular_factor_a) / (1 + dt * angular_damping)
 *   x'_a   = x_a + dt * v'_a ;  x'_a < centre_min_a or > centre_max_a: x'_a = that bound, v'_a = 0
 *   q'     = (q + (dt / 2) * (0, w') (x) q) / |q + (dt / 2) * (0, w') (x) q|
 *   pose   = { N(R(q')), N(x') }      steps += 1
 * gain is the caller's: finalise gives a particle displaced by delta the velocity change 0.49 * delta / dt (the reference's
 * damping of the position-derived velocity), so with gain = 0.49 the body receives exactly the momentum the fluid was
 * given; gain = 1 is the plain position-based estimate.  The factors are 0 or 1 per world axis (a hinge, a slider, a body
 * that only heaves); the centre bounds may be +-inf.
 *
 * pbf_set_collider_body needs an installed collider (PBF_ERR_STATE otherwise, and in the slab cases pbf_set_collider
 * refuses).  It turns the reaction records on if they are off (the allocation of pbf_set_collider_reaction(ctx, 1); nothing
 * is allocated inside a step) and writes parameters, state and start pose into one small device record with a one-lane
 * kernel on the ctx's stream that receives them by value: the call itself does not synchronise.  The start pose is kept as
 * given, so the first step reads what pbf_set_collider_pose would have left.  Going off -> on or on -> off selects another
 * launch sequence and drops the captured graphs, as pbf_set_collider does; a call while a body is on re-places the body or
 * changes its parameters (the counters start again), changes no key and drops no graph.  body == NULL turns the body off:
 * the solid stays where it is, as an ordinary pose, and the reaction stays on.  While a body is on, pbf_set_collider_pose
 * and pbf_set_collider_reaction(ctx, 0) return PBF_ERR_STATE (re-place the body through this call); pbf_set_collider and
 * pbf_set_collider_mesh, clearing included, turn the body off, since they reset the pose.
 *
 * PBF_ERR_INVALID, each with its reason, leaving everything unchanged: a non-finite parameter or start velocity (the centre
 * bounds may be infinite); mass <= 0; an inertia <= 0; gain < 0; a damping < 0; a factor other than 0 or 1; centre_min >
 * centre_max; a start pose pbf_set_collider_pose would refuse.
 *
 * Limitations: one body per ctx; no contact of the body with the box or with obstacles beyond the centre bounds (contact
 * with the scenery: pbf_set_collider_body_contact, below); no swept collision (a body that moves further per step than its
 * own thickness can pass through fluid); no restitution against the fluid; no gyroscopic
 * term (a spinning asymmetric body does not precess); not in slab mode; whitewater sees the body only with
 * pbf_set_whitewater_solids on (below; diffuse particles are massless and exert nothing on it), the observers still do not
 * see the solid. */
typedef struct pbf_collider_body {
  double mass, inertia[3];                 /* principal moments about the centre of mass, along the lattice's axes */
  double gain;                             /* 0.49: the momentum finalise gave the fluid; 1: the position-based estimate */
  double linear_damping, angular_damping;  /* >= 0, per time */
  double accel[3];                         /* world units per time squared (gravity) */
  double linear_factor[3], angular_factor[3];   /* 0 or 1 per world axis */
  double centre_min[3], centre_max[3];     /* bounds of the centre of mass, world; may be -inf / +inf */
  pbf_collider_pose pose;                  /* the start pose; trans is the centre of mass */
  double velocity[3], angular_velocity[3];
} pbf_collider_body;
/* (the struct shares its name with the call that fills it, so it has no typedef: write `struct pbf_collider_body_state`) */
struct pbf_collider_body_state {
  pbf_collider_pose pose;                  /* R(q) and x in double; the kernels read it rounded to N */
  double quat[4], velocity[3], angular_velocity[3];
  double impulse[3], angular[3];           /* the sums the last advance consumed: P and L of that step */
  uint64_t hits;                           /* and its hit count */
  uint64_t steps;                          /* advances since the body was set */
  uint64_t rejected;                       /* of which ignored their sums (a non-finite impulse) */
};
int pbf_set_collider_body(pbf_ctx *ctx, const pbf_collider_body *body);   /* NULL: off */
/* an observer between steps, like pbf_collider_reaction: it synchronises (a polled mailbox), is part of no step and changes
 * nothing a step reads.  PBF_ERR_STATE without a body. */
int pbf_collider_body_state(pbf_ctx *ctx, struct pbf_collider_body_state *out);

/* Collider friction: Coulomb drag against the collider, with the solid's contact velocity (no reference counterpart;
 * Bridson's particle - level-set friction v_t' = max(0, 1 - mu dv_n / |v_t|) v_t).  Opt-in: a ctx that never calls
 * pbf_set_collider_friction, or has cleared it, launches what it always did.
 *
 * With friction on, every step (pbf_step, every step of pbf_steps, hipGraph replays, pbf_stage_finalise) runs ONE streaming
 * pass right after finalise and before vorticity, XSPH and surface tension, which therefore see the boundary-corrected
 * velocity; pbf_steps does not fuse finalise(t) with predict(t + 1) then.  The pass reads the step's reaction records: A,
 * the summed displacement the solid gave the particle over the iterations, is the contact normal and the normal impulse at
 * once, so no lattice is read.  No host read-back, and no argument that changes per step: mu, V and W live in a small device
 * record the pass reads through a pointer.
 *
 * The contract (csrc/pbf_collider_friction.hpp).  Everything per particle is in N, in the order written, not contracted;
 * PBF_FLAG_FAST_MATH does not reach it.  vel4 is in the solver frame (world / scale); A, V, W and t are world.
 *   V, W   = the call's velocity and angular_velocity, rounded to N; while a body is on: N(velocity), N(angular_velocity)
 *            of the body's state as the pass finds them (after the step's advance)
 *   t      = the pose record's trans as the pass finds it (no pose ever set: 0); mu rounded to N
 *   particle a with the record A (obstacles keep a zero record and never act):
 *   len  = sqrt((A_x A_x + A_y A_y) + A_z A_z)          act = A.w > 0 && len > 0
 *   n_a  = A_a / len
 *   r_a  = pos4[a]_a - t_a                               (the finalised world position)
 *   c_x  = W_y r_z - W_z r_y   (y, z cyclic; each product rounded, one subtraction)
 *   vb_a = (V_a + c_a) / scale
 *   u_a  = v_a - vb_a          un = (u_x n_x + u_y n_y) + u_z n_z          ut_a = u_a - un * n_a
 *   s    = sqrt((ut_x ut_x + ut_y ut_y) + ut_z ut_z)     slide = act && s > 0
 *   jn   = (VD * (len / scale)) / dt                     VD = N(0.49f): the speed finalise gave the particle from the push
 *   g    = (mu * jn) / s        f = g < 1 ? g : 1        (a NaN g counts as 1)        dv_a = -(f * ut_a)
 *   v'_a = slide ? v_a + dv_a : v_a                      (bits kept otherwise; pos4, pStar, lambda untouched)
 * A lane that does not act loads neither position nor velocity and stores nothing.
 *
 * The sum, with the reaction's fixed-shape reduction (no atomics, Morton order, terms formed in double):
 *   p_a = m * (double(dv_a) * double(scale))     P = sum p     L = sum double(r) x p     and the sums of |term|
 * pbf_collider_friction_reaction is an observer between steps like pbf_collider_reaction (it synchronises): the LAST pass's
 * raw sums, impulses in world units x mass / time; the solid received -P and -L, L about t.  hits = particles that slid,
 * particles = particles with act, step = passes run since friction was turned on.  PBF_ERR_STATE when friction is off, when
 * no step has run since it was turned on, and in slab mode.
 *
 * With a body on as well, the body stage of step t + 1 first folds the sums of step t's pass and kicks the body (in double):
 *   v_a += (-P_a / mass) * linear_factor_a
 *   h = R(q)^T (-L) ;  k_b = h_b / inertia_b ;  w_a += (R(q) k)_a * angular_factor_a
 * a non-finite P or L: no kick, `rejected` goes up by one.  Then it advances as without friction.  The body's x does not
 * change in between, so L is about the right point.  Each pass's sums are consumed exactly once (a pending word on the
 * device), whether the step is eager, batched or replayed, or pbf_stage_body runs alone.  The sums outlive an upload, also
 * one that grows the capacity: the step after it hands them to the body.  pbf_set_collider_body while friction is on drops
 * sums that are still pending: they were taken against another pose and other velocities, and the body as placed by the
 * call starts with the velocities it was given (pbf_collider_friction_reaction still returns them).
 *
 * pbf_set_collider_friction needs an installed collider (PBF_ERR_STATE otherwise, and in the slab cases pbf_set_collider
 * refuses); PBF_ERR_INVALID for mu <= 0 or NaN (+inf is no-slip) and for a non-finite velocity; a refusal changes nothing.
 * It turns the reaction records on if they are off; while friction is on pbf_set_collider_reaction(ctx, 0) returns
 * PBF_ERR_STATE.  Off <-> on selects another launch sequence and drops the captured graphs; a call while friction is on
 * rewrites the device record with a one-lane kernel on the ctx's stream that receives it by value: no key changes, no graph
 * is dropped, nothing synchronises.  pbf_set_collider and pbf_set_collider_mesh, clearing included, turn friction off.
 *
 * Limitations: one coefficient (no separate static and kinetic friction); no restitution; no friction against the box walls
 * or obstacle particles; not in slab mode. */
typedef struct pbf_collider_friction {
  double mu;                   /* > 0; +inf = no-slip */
  double velocity[3];          /* world units per time: the solid's velocity at t (ignored while a body is on) */
  double angular_velocity[3];  /* rad per time, world frame, about the pose's t (ignored while a body is on) */
} pbf_collider_friction;
int pbf_set_collider_friction(pbf_ctx *ctx, const pbf_collider_friction *f);   /* NULL: off */
int pbf_collider_friction_reaction(pbf_ctx *ctx, pbf_collider_wrench *out);    /* observer between steps */

/* Mesh colliders: the signed-distance lattice of a closed triangle mesh, built on the device (no reference counterpart).
 * Opt-in; neither call is part of a step and both synchronise.  Without a call to them every launch of a step is unchanged.
 *
 * pbf_mesh_records is plain host code (csrc/pbf_mesh_records.hpp: no ctx, no GPU).  It checks the mesh, fills `info` and
 * writes the records the kernel reads, 30 values of N (fp64 ? double : float) per triangle; records == NULL checks only.
 * It accepts a closed, consistently oriented 2-manifold only: every index < n_vertices; no triangle of zero area in double;
 * every undirected edge used by exactly two triangles, in opposite directions.  Anything else returns PBF_ERR_INVALID, the
 * message in pbf_last_error(NULL), `records` untouched, and `info` (when not NULL) holding:
 *   mesh, vertices or triangles NULL; a count zero or >= 2^31; a vertex that is not finite:   every field zero
 *   an index >= n_vertices:                                                                   aabb_min / aabb_max, the rest zero
 *   a degenerate triangle, a boundary, non-manifold or misoriented edge:                      every field
 * n_edges counts the undirected edges; an edge used once is a boundary edge, more than twice a non-manifold edge, twice
 * in the same direction a misoriented edge.  The edge table is built by sorting: O(nt log nt).  A negative volume is legal:
 * the mesh is inside out, which gives the field of the same mesh with PBF_MESH_NEGATE.
 * The record of triangle k (vertices a, b, c), formed in double in the order written and then rounded to N:
 *   [0..8]   a, b, c
 *   [9..11]  fu = n / sqrt(n . n),  n = (b - a) x (c - a)                     (u . v = (u_x v_x + u_y v_y) + u_z v_z)
 *   [12..20] the edge pseudonormals of ab, bc, ca: fu_k + fu_k' of the two triangles on that edge
 *   [21..29] the vertex pseudonormals of a, b, c: the sum, over the triangles around the vertex in ascending triangle index
 *            and starting from 0, of angle * fu, angle = atan2(|e1 x e2|, e1 . e2) of that triangle's two edges leaving the vertex
 * Pseudonormals are not normalised.  They are the angle-weighted pseudonormals of Baerentzen & Aanaes 2005 ("Signed distance
 * computation using the angle weighted pseudonormal", IEEE TVCG 11(3)): the choice for which the sign below is right at
 * edges and vertices too.
 *
 * The field.  Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it; divides and
 * the square root are IEEE.  Node (i, j, k) is at p_a = N(origin_a) + N(i_a) * N(spacing), as pbf_sample_lattice forms its
 * points.  For a node p and a triangle the closest point q follows the seven regions of Ericson, Real-Time Collision
 * Detection 5.1.5:
 *   ab = b - a   ac = c - a   ap = p - a   bp = p - b   cp = p - c   cb = c - b
 *   d1 = ab . ap   d2 = ac . ap   d3 = ab . bp   d4 = ac . bp   d5 = ab . cp   d6 = ac . cp
 *   vc = d1 d4 - d3 d2     vb = d5 d2 - d1 d6     va = d3 d6 - d5 d4     e = d4 - d3     f = d5 - d6
 *   the first region that holds, in this order, gives q and the normal n of that feature:
 *     vertex a   d1 <= 0 && d2 <= 0                q = a                                   n = [21..23]
 *     vertex b   d3 >= 0 && d4 <= d3               q = b                                   n = [24..26]
 *     edge ab    vc <= 0 && d1 >= 0 && d3 <= 0     t = d1 / (d1 - d3)     q = a + t ab     n = [12..14]
 *     vertex c   d6 >= 0 && d5 <= d6               q = c                                   n = [27..29]
 *     edge ca    vb <= 0 && d2 >= 0 && d6 <= 0     t = d2 / (d2 - d6)     q = a + t ac     n = [18..20]
 *     edge bc    va <= 0 && e >= 0 && f >= 0       t = e / (e + f)        q = b + t cb     n = [15..17]
 *     face       otherwise    den = (va + vb) + vc   v = vb / den   w = vc / den   q = (a + v ab) + w ac   n = [9..11]
 *   r = p - q     d2 = r . r     s = r . n     neg = s < 0
 * Every candidate is computed and the result selected: no lane branches, and the 0 / 0 of a region that did not hold is
 * dropped by the select.  The fold runs over the triangles in ascending index from best = +inf, neg = false; a triangle
 * replaces {best, neg} only when d2 < best, strictly, so the lowest index among ties wins and a NaN never replaces.
 *   phi = (neg != negate) ? -sqrt(best) : sqrt(best)            negate = flags & PBF_MESH_NEGATE
 * A node on the mesh has best == 0 and s == 0, so neg is false: phi is +0 without PBF_MESH_NEGATE and -0 with it (zero
 * either way: such a node is on the solid's surface).
 *
 * pbf_sdf_from_mesh fills the lattice of `lattice` (dims, origin, spacing; its phi and margin are ignored) and copies it
 * to the host array phi, N[dims product] in pbf_set_collider's order.  pbf_set_collider_mesh computes the same lattice and
 * installs it as the ctx's collider with lattice->margin, without leaving the device: it ends in pbf_set_collider's
 * install path (a captured step's key changes, captured graphs are dropped), and every later step and pbf_collider_sample
 * gives the bytes they give after pbf_set_collider with the array pbf_sdf_from_mesh returned.  The lattice arguments are
 * checked by the code that checks pbf_set_collider's (margin by the installing call only); a refused mesh is
 * PBF_ERR_INVALID with pbf_mesh_records' message in pbf_last_error(ctx); so are lattice == NULL, phi == NULL and unknown
 * flag bits.  The slab refusals are pbf_set_collider's (PBF_ERR_STATE).  A refusal leaves the ctx, its collider and phi
 * untouched.  stats (may be NULL): pairs_total = nodes x triangles, pairs_tested = the pairs the kernel evaluated — equal
 * with "sdf_cull" 0, fewer with 1 (the default); the field's bytes are the same either way.  The work is split over launches of at most
 * 2^33 lane-triangle pairs so that no single kernel runs for seconds.
 *
 * Sign by winding number (PBF_MESH_SIGN_WINDING; combines with PBF_MESH_NEGATE; bit 1 of flags stays unknown).  With the
 * flag pbf_sdf_from_mesh and pbf_set_collider_mesh take the mesh as a triangle SOUP: open, misoriented, duplicated and
 * interpenetrating triangles are accepted, and pbf_mesh_soup_records replaces pbf_mesh_records as the check.  The unsigned
 * distance is the fold above — the same expressions, the same order, the strict < — on the soup's a, b, c; the sign is the
 * generalised winding number's (Jacobson, Kavan & Sorkine-Hornung 2013, ACM TOG 32(4); solid angles by van Oosterom &
 * Strackee 1983), which needs no adjacency.  Without the flag nothing changes: every kernel, record and refusal is as above.
 * Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it; sqrt and divides are IEEE;
 * u . v as above.
 *   p as the distance fold forms it;   a = A - p   b = B - p   c = C - p          (A, B, C: record values)
 *   la = sqrt(a . a)   lb = sqrt(b . b)   lc = sqrt(c . c)
 *   x = (b_y c_z - b_z c_y, b_z c_x - b_x c_z, b_x c_y - b_y c_x)      num = a . x
 *   den = ((la lb) lc + (a . b) lc) + ((b . c) la + (c . a) lb)
 *   S += atan2(num, den)          ascending triangle index, from S = 0
 *   w = S / N(2 pi)                                   (pbf_mesh_winding's output)
 *   neg = best > 0 && S > N(pi)                       (a node on the mesh keeps the existing +0 / -0 convention)
 *   phi = (neg != negate) ? -sqrt(best) : sqrt(best)
 * atan2 is the device library's and has no bit contract, so the sign and w are held by tolerance (DESIGN 5f states the
 * bar); sqrt(best) stays bit for bit the fold's.  w is 1 inside a closed outward mesh and 0 outside; for an open mesh it is
 * the share of the sphere of directions the mesh covers, and the solid is where w > 1/2.  Within rounding of a face num
 * changes sign and w jumps by 1: the field's own discontinuity.  Every pair is evaluated (a solid angle has no exact cull);
 * stats still describe the distance fold.  Limits: the distance is to the nearest triangle, buried sheets included, so a
 * union of interpenetrating parts has small |phi| at its inner faces (phi is still negative there); an open sheet without
 * volume has w < 1/2 everywhere and is no solid; zero-area triangles are refused, not dropped; no mesh is repaired.
 *
 * pbf_mesh_soup_records is plain host code beside pbf_mesh_records (no ctx, no GPU): the records of the soup, a, b, c formed
 * in double and rounded to N once, 9 values per triangle; records == NULL checks only.  It refuses only what the kernels
 * cannot survive — mesh, vertices or triangles NULL; a count zero or >= 2^31; a vertex that is not finite; an index >=
 * n_vertices; a triangle of zero area in double — with PBF_ERR_INVALID, the message in pbf_last_error(NULL), `records`
 * untouched and `info` as pbf_mesh_records leaves it in the same case.  On success `info` is complete: boundary,
 * non-manifold and misoriented edges are reports here, not refusals.
 *
 * pbf_mesh_winding returns the winding-number field itself, w above, N[dims product] in pbf_set_collider's order: for
 * voxelising, and for checking an asset before trusting it.  The lattice checks and the slab refusals are
 * pbf_sdf_from_mesh's; a refused mesh is PBF_ERR_INVALID with pbf_mesh_soup_records' message; so are lattice == NULL and
 * w == NULL.  A refusal leaves the ctx, its collider and w untouched.  It synchronises and is never part of a step. */
typedef struct pbf_mesh {
  uint64_t n_vertices, n_triangles;
  const double *vertices;      /* 3 per vertex, world units */
  const uint32_t *triangles;   /* 3 vertex indices per triangle, counter-clockwise seen from outside */
} pbf_mesh;
typedef struct pbf_mesh_info { /* filled on success AND on a mesh that is refused (see above) */
  uint64_t n_edges, boundary_edges, nonmanifold_edges, misoriented_edges, degenerate_triangles;
  double volume;               /* signed: sum a.(b x c) / 6 over the triangles in ascending index; negative = inside out */
  double aabb_min[3], aabb_max[3];
} pbf_mesh_info;
typedef struct pbf_mesh_sdf_stats { uint64_t pairs_total /* nodes x triangles */, pairs_tested; } pbf_mesh_sdf_stats;
enum {
  PBF_MESH_NEGATE = 1u << 0,        /* solid OUTSIDE the mesh: a cavity the fluid lives in */
  PBF_MESH_SIGN_WINDING = 1u << 2   /* a triangle soup signed by the winding number (above) */
};
int pbf_mesh_records(const pbf_mesh *mesh, int fp64, void *records /* N[30 n_triangles] */, pbf_mesh_info *info);
int pbf_sdf_from_mesh(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, uint32_t flags,
                      void *phi /* N[dims product] */, pbf_mesh_sdf_stats *stats /* may be NULL */);
int pbf_set_collider_mesh(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, uint32_t flags,
                          pbf_mesh_sdf_stats *stats /* may be NULL */);
int pbf_mesh_soup_records(const pbf_mesh *mesh, int fp64, void *records /* N[9 n_triangles] */, pbf_mesh_info *info);
int pbf_mesh_winding(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, void *w /* N[dims product] */);

/* Scenery: a second, STATIC signed-distance lattice beside the collider (no reference counterpart).  Opt-in: with no
 * scenery set every launch and every byte of a step is what it is without this feature.  The collider is the one solid
 * that may carry a pose, a body and friction; the scenery is the harbour, the bowl, the ramp or the floor around it.  It
 * lives in the world frame and never has a pose, a reaction, friction or a body.
 *
 * Setting.  pbf_set_scenery takes a lattice as pbf_set_collider does: rounded to N, kept in a buffer of its own, checked
 * by the same code with the same refusals in the same order (PBF_ERR_INVALID: a dim < 2; a dims product >= 2^31; a
 * non-finite origin, spacing or margin; spacing <= 0; margin < 0; phi == NULL; a NaN in phi — infinities are legal).
 * sdf == NULL clears the scenery and frees the lattice.  pbf_set_scenery_mesh is pbf_set_collider_mesh's build, flags
 * and refusals included, installed as scenery.  The setting persists until it is replaced or cleared and allocates
 * nothing inside a step.  It needs no collider; installing, replacing or clearing the collider leaves the scenery alone,
 * and the pose, the body and friction never touch it.  Slab mode is not supported: setting scenery on a slab-attached or
 * slab-configured ctx, and pbf_slab_step(s) / a delta-p stage of a slab-configured ctx with scenery set, return
 * PBF_ERR_STATE, as with a collider.  A refusal leaves the ctx, its scenery and its collider unchanged.
 *
 * The contract of a delta-p launch.  Everything is in N, in the order written, not contracted; PBF_FLAG_FAST_MATH does not
 * reach it.  q is the input of the static contract above: after the world-frame box clamp and the division by scale.
 *   Scenery alone (no collider lattice): q' = the static contract on q with the scenery's lattice — exactly the kernels
 *   and arguments pbf_set_collider with that lattice would run.
 *   Collider and scenery together:
 *     q1 = the POSED contract on q with the collider's lattice (the pose record holds the identity while no pose is set:
 *          every value compares equal to the static function's, a zero may change its sign); the reaction record is
 *          updated from (q, q1) exactly as with pbf_set_collider_reaction alone
 *     q2 = the static contract on q1 with the scenery's lattice
 *   q2 is stored and the quantised copy is formed from it.  The scenery writes no record: A, B and hits describe the
 *   collider's push alone, with r taken at q1, so the friction pass, the body stage and pbf_collider_reaction see exactly
 *   what they would see without scenery for the same q.  The scenery comes last, so where both press on a particle the
 *   static wall wins, and the box wins over both through each projection's own second clamp; the K iterations converge the
 *   rest.  A lane that hits neither keeps its bits.  Obstacles and ghost copies are never moved.  Every gather path gives
 *   the same bytes, "coop" 2 / 4 / 8 within its usual rounding.
 *
 * The reaction is on whenever both lattices are installed, as it is with a body or with friction: the combined kernel is
 * the reaction's kernel plus one projection, and no variant without records is built.  The call that completes the pair
 * (pbf_set_scenery / pbf_set_scenery_mesh with a collider present, pbf_set_collider / pbf_set_collider_mesh with scenery
 * present) turns the records on if they are off, allocating what pbf_set_collider_reaction(ctx, 1) allocates before
 * anything is changed, so a failed allocation leaves everything as it was.  While both are installed
 * pbf_set_collider_reaction(ctx, 0) returns PBF_ERR_STATE.  Clearing either solid leaves the reaction on.
 *
 * Captured graphs.  Every pbf_set_scenery / pbf_set_scenery_mesh call, clearing included, changes a captured step's key
 * and drops the captured graphs (and synchronises, once): a replay never runs on a replaced or freed lattice.
 *
 * pbf_scenery_sample is pbf_collider_sample on the scenery's lattice (always the static function): the same arguments,
 * outputs and refusals, PBF_ERR_STATE without scenery.
 *
 * Limitations: the body collides with the scenery only with pbf_set_collider_body_contact (below) on — otherwise only its
 * centre bounds hold it.  There is no friction of the fluid against the scenery and no reaction on it.  Whitewater's diffuse particles see it only with
 * pbf_set_whitewater_solids on (below); the observers do not see it.  One
 * collider and one static scenery lattice per ctx: several static solids are composed into the scenery's lattice on the
 * host, by the min of their distances.  Not in slab mode. */
int pbf_set_scenery(pbf_ctx *ctx, const pbf_collider_sdf *sdf);   /* NULL clears and frees the lattice */
int pbf_set_scenery_mesh(pbf_ctx *ctx, const pbf_mesh *mesh, const pbf_collider_sdf *lattice, uint32_t flags,
                         pbf_mesh_sdf_stats *stats /* may be NULL */);
int pbf_scenery_sample(pbf_ctx *ctx, const pbf_params *params, size_t n, const double *points /* 3n, world */,
                       void *phi /* N[n] */, void *moved /* N[3n], solver frame */, uint8_t *hit /* [n] */);

/* Body contact: the rigid body collides with the scenery, on the device (no reference counterpart).  Opt-in: a ctx that
 * never calls pbf_set_collider_body_contact — a ctx with a body and scenery included — launches exactly what it launched
 * before and produces the same bytes.
 *
 * The body's surface.  The call takes a fixed point set from the collider's lattice, once, at configure time (two kernels
 * around the library's scan, and one synchronisation to read the count; it is not a step).  One lane per cell (i, j, k) of
 * the lattice whose three indices are multiples of `stride`; the cell gives a point iff all eight nodes are finite, some
 * node is < N(level) and some node is >= N(level), and, with b_a = N(origin_a) + (N(i_a) + N(0.5)) * N(spacing), the static
 * contract above on the collider's lattice with margin := N(level) at b returns inside with len > 0 and p_a = b_a + s * g_a
 * finite (s = (margin - phi) / len whatever `hit` says, so a centre outside the level is pulled in).  p is the point, in N,
 * in the body frame.  Points are stored in cell-index order ((i * cells_y + j) * cells_z + k), so one lattice gives one
 * array on every run.  pbf_collider_body_contact_points returns the count and, where points != NULL, the array.
 *
 * The step.  With contact on, stage_body runs `iterations` passes after the body's advance, each two launches with fixed
 * arguments: one lane per point, then one workgroup.  No read-back, nothing allocated, no atomics: the sums are a fold of a
 * fixed shape (lanes by an xor butterfly, waves in wave order, partial records 256 at a time in index order), so the same
 * state gives the same bytes eagerly, through pbf_steps and in a replayed graph.
 *
 * The contract (csrc/pbf_body_contact.hpp, plain C++ shared by the kernel and a stand-alone host program).  R and x are the
 * body record's pose in double; everything is in the order written, not contracted; PBF_FLAG_FAST_MATH does not reach it.
 * Per point b (N, body frame):
 *   r_a = (R[a][0] b_0 + R[a][1] b_1) + R[a][2] b_2        w_a = r_a + x_a
 *   the static contract on the scenery's lattice with margin := N(skin), at (N(w_0), N(w_1), N(w_2))  ->  inside, hit, s, g
 *   m_a = double(s) * double(g_a)          d = sqrt((m_0 m_0 + m_1 m_1) + m_2 m_2)
 *   in contact  =  inside && hit && d > 0 && d finite
 *   sums over the points in contact:  S = sum d,  M_a = sum m_a,  A_a = sum d * r_a,  D = max d,  count
 * The response, in double.  mass, inertia, F = linear_factor, G = angular_factor and the centre bounds are the body's; e =
 * restitution, mu = friction, beta = correction; x, v, w the body's centre, velocity and angular velocity:
 *   passes += 1;  the raw sums S, M, A, D go to the state, impulse = shift = 0
 *   count == 0: done                                                        (the sums are the zeros)
 *   ln = sqrt((M_0 M_0 + M_1 M_1) + M_2 M_2)
 *   S, an M_a, an A_a, D or ln non-finite, or !(ln > 0): rejected += 1, done                  (opposite walls cancel)
 *   n_a = M_a / ln          r_a = A_a / S          contacts += 1
 *   cross(p, q) = (p_1 q_2 - p_2 q_1,  p_2 q_0 - p_0 q_2,  p_0 q_1 - p_1 q_0)
 *   dot(p, q)   = (p_0 q_0 + p_1 q_1) + p_2 q_2
 *   W(c):  h_b = (R[0][b] c_0 + R[1][b] c_1) + R[2][b] c_2 ;  k_b = h_b / inertia_b
 *          W_a = ((R[a][0] k_0 + R[a][1] k_1) + R[a][2] k_2) * G_a
 *   Wn = W(cross(r, n))
 *   kn = ((F_0 n_0 n_0 + F_1 n_1 n_1) + F_2 n_2 n_2) / mass + dot(n, cross(Wn, r))          (F_a n_a n_a = (F_a * n_a) * n_a)
 *   u  = v + cross(w, r)          un = dot(u, n)
 *   un < 0 && kn > 0:  j = -((1 + e) * un) / kn ;  v_a = v_a + ((j * n_a) / mass) * F_a ;  w_a = w_a + j * Wn_a
 *   else:              j = 0
 *   mu > 0 && j > 0:   u' = v + cross(w, r) ;  c = dot(u', n) ;  ut_a = u'_a - c * n_a
 *                      lt = sqrt((ut_0 ut_0 + ut_1 ut_1) + ut_2 ut_2)
 *                      lt > 0:  t_a = ut_a / lt ;  Wt = W(cross(r, t))
 *                               kt = ((F_0 t_0 t_0 + F_1 t_1 t_1) + F_2 t_2 t_2) / mass + dot(t, cross(Wt, r))
 *                               kt > 0:  jt = min(mu * j, lt / kt)
 *                                        v_a = v_a - ((jt * t_a) / mass) * F_a ;  w_a = w_a - jt * Wt_a
 *                      (jt = 0 and t = 0 wherever a condition fails)
 *   impulse_a = j * n_a - jt * t_a
 *   s = beta * max(D - slop, 0) ;  shift_a = (s * n_a) * F_a ;  x_a = x_a + shift_a
 *   x_a < centre_min_a or > centre_max_a: x_a = that bound, v_a = 0           (exactly as advance() applies the bounds)
 *   pose.trans = x (rot and q unchanged); the kernel rewrites N(x) in the pose record the delta-p launches read
 * The body record's layout and struct pbf_collider_body_state do not change.
 *
 * pbf_set_collider_body_contact needs a body that is on and installed scenery (PBF_ERR_STATE otherwise, and in slab mode
 * as every collider call).  PBF_ERR_INVALID, each with its reason, leaving everything unchanged: a non-finite field; stride
 * < 1; skin < 0; restitution or correction outside [0, 1]; friction < 0; slop < 0; iterations outside 1..8; a lattice that
 * yields no point.  Off -> on and on -> off change the launch sequence and drop the captured graphs; so do another level or
 * stride (another point set) and another number of iterations while on.  Any other change of parameters while on rewrites
 * the device record by value with a one-lane kernel, like a re-placed body: no synchronisation, no graph dropped; the
 * counters start again.  NULL turns contact off and frees its buffers; so do pbf_set_collider_body(ctx, NULL),
 * pbf_set_collider / pbf_set_collider_mesh (clearing included: they turn the body off) and pbf_set_scenery(ctx, NULL) /
 * a cleared pbf_set_scenery_mesh.  A replaced scenery keeps contact on (the points belong to the body); a re-placed body
 * keeps it on and zeroes the counters.
 *
 * pbf_collider_body_contact_state is an observer between steps like pbf_collider_body_state: it synchronises (a polled
 * mailbox), is part of no step and changes nothing a step reads.  PBF_ERR_STATE while contact is off.
 *
 * Limitations: no contact with the box walls or with obstacle particles (walls are composed into the scenery's lattice);
 * the position correction translates and never rotates the body; one averaged contact per pass, not a per-point manifold;
 * no swept contact; one body; not in slab mode; the scenery receives no reaction. */
typedef struct pbf_body_contact {
  double level;        /* the body's surface is phi_collider == level (world units, finite) */
  uint32_t stride;     /* >= 1: only cells whose three indices are multiples of stride give a point */
  double skin;         /* >= 0: a point is in contact where phi_scenery < skin */
  double restitution;  /* in [0, 1] */
  double friction;     /* mu >= 0 */
  double correction;   /* in [0, 1]: the share of the depth removed per pass */
  double slop;         /* >= 0: depth left alone */
  uint32_t iterations; /* 1..8 detect + resolve passes per step */
} pbf_body_contact;
int pbf_set_collider_body_contact(pbf_ctx *ctx, const pbf_body_contact *contact);   /* NULL: off */
int pbf_collider_body_contact_points(pbf_ctx *ctx, uint64_t *n, void *points /* N[3n], body frame; may be NULL */);
struct pbf_body_contact_state {
  double depth_sum, push[3], arm[3], depth_max;   /* the raw sums of the LAST pass: S, M, A, D */
  double impulse[3], shift[3];                    /* what that pass applied */
  uint64_t points;                                /* points of the body's surface */
  uint64_t passes, contacts, rejected;            /* passes since configured; of which responded; of which were refused */
};
int pbf_collider_body_contact_state(pbf_ctx *ctx, struct pbf_body_contact_state *out);  /* observer; synchronises */

/* ---- particle state (replaces the std::vector<Particle>& in/out argument, src/sph.hpp:124) */
int pbf_upload(pbf_ctx *ctx, size_t n, const uint64_t *id, const uint8_t *type, const void *mass, const void *pos,
               const void *vel, const void *colour);
/* Device order = Z-sorted after a step, exactly like the reference's write-back
 * (src/omp/ompsph.hpp:479-481).  Any pointer may be NULL. */
int pbf_download(pbf_ctx *ctx, uint64_t *id, uint8_t *type, void *mass, void *pos, void *vel, void *colour);
size_t pbf_count(const pbf_ctx *ctx);

/* AoS path for the C++ shim: `particles` is the caller's std::vector<Particle>::data()
 * (src/sph.hpp:36-54).  Unpacked / repacked on the device; offsets in bytes.  The buffer is page-locked in place
 * (hipHostRegister, kept while the same pointer comes back: benchmark.cpp:33,47 passes one vector every frame) so both
 * copies are plain DMA.  pbf_download_aos writes the FIELDS; struct padding bytes (no part of the reference's contract:
 * its write-back copies whole structs, ompsph.hpp:479-481) receive the bytes the last uploaded image held at that slot. */
typedef struct pbf_aos_layout {
  uint32_t stride, off_id, off_type, off_mass, off_pos, off_vel, off_colour;
} pbf_aos_layout;
int pbf_upload_aos(pbf_ctx *ctx, size_t n, const void *particles, const pbf_aos_layout *layout);
int pbf_download_aos(pbf_ctx *ctx, void *particles, const pbf_aos_layout *layout);
/* The same download in two halves: _begin packs the image and starts its DMA on a copy stream of its own, _end waits for it.
 * Work enqueued in between that only READS the particle state — pbf_surface, in the shim's advance() — runs while the
 * particles travel over PCIe (1 M particles: 1.1 ms hidden behind 1.0 ms of surface kernels).  `particles` must stay valid
 * until _end; no step, upload or stage call in between. */
int pbf_download_aos_begin(pbf_ctx *ctx, void *particles, const pbf_aos_layout *layout);
int pbf_download_aos_end(pbf_ctx *ctx);

/* ---- the hot path ---------------------------------------------------------------------- */
/* One advance() on device-resident state (src/omp/ompsph.hpp:128-271 + 479-481), asynchronous
 * on the ctx stream: predict+key -> counting sort + cell table -> diffuse -> K x (lambda, delta)
 * -> finalise.  The two loops the reference updates in place (racy with >1 thread,
 * src/omp/ompsph.hpp:188-207,235-248) are double-buffered (Jacobi) here. */
int pbf_step(pbf_ctx *ctx, const pbf_params *params);
/* count x pbf_step, no host sync.  Option "graph" = 1: each distinct step (same buffer roles, same parameters) is captured
 * into a hipGraph the first time it comes by and replayed afterwards — one graph launch instead of ~25 kernel launches;
 * stage timing, wells, slab mode, a step that still allocates and scenes whose parameters change every frame (the stock
 * moving box) run eagerly; results are identical either way.  Default 0: measured 1-9 % SLOWER than eager launches on
 * MI355X / ROCm 7 at 16 K - 1 M particles (the step is never host-launch bound). */
int pbf_steps(pbf_ctx *ctx, const pbf_params *params, uint32_t count);
int pbf_graph_stats(const pbf_ctx *ctx, uint64_t out[3]); /* {graphs captured, graph replays, graphs still enabled} */
int pbf_sync(pbf_ctx *ctx);

/* Stage-level entry points: exactly the launches pbf_step makes, exposed so that each kernel
 * can be checked against the oracle stage by stage.  Order as in pbf_step. */
int pbf_stage_predict(pbf_ctx *ctx, const pbf_params *params);  /* ompsph.hpp:132-154 */
int pbf_stage_sort(pbf_ctx *ctx, const pbf_params *params);     /* ompsph.hpp:157-165, sph.hpp:238-250 */
int pbf_stage_diffuse(pbf_ctx *ctx, const pbf_params *params);  /* ompsph.hpp:188-207 */
int pbf_stage_lambda(pbf_ctx *ctx, const pbf_params *params);   /* ompsph.hpp:217-232 */
int pbf_stage_delta(pbf_ctx *ctx, const pbf_params *params);    /* ompsph.hpp:235-248 */
int pbf_stage_finalise(pbf_ctx *ctx, const pbf_params *params); /* ompsph.hpp:256-264 */
/* with a body on (pbf_set_collider_body): the body's advance alone, which pbf_step runs after its delta-p iterations and
 * before finalise.  PBF_ERR_STATE without a body, or without a sort since the reaction records were enabled. */
int pbf_stage_body(pbf_ctx *ctx, const pbf_params *params);

/* ---- sources, drains and cell queries on resident state (the rest of sph::Scene, src/sph.hpp:56-79) -----------
 * What the reference does on the host at the top of advance() (src/omp/ompsph.hpp:93-118) runs here on the device,
 * before predict, inside every pbf_step / each step of pbf_steps while a source or a drain is set:
 *   emit   for each source in the order given: size = sqrt(N(rate)), a floor(size) x ceil(size) sheet in x / z at spacing
 *          h * scale / 2 around `centre` (ompsph.hpp:93-105), id = tag, type fluid, mass 1, the source's colour and
 *          velocity; appended behind the particles present (i.e. behind the last step's Z-order);
 *   drain  a fluid particle (freshly emitted ones included, obstacles never) leaves when
 *          sqrt(dx*dx + dy*dy + dz*dz) < width for any drain (ompsph.hpp:107-118), in N on the stored world position;
 *          the survivors keep their order (std::remove_if).
 * The doubles below are rounded to N first.  The settings are copied and persist in the ctx (n = 0 clears); with both
 * cleared pbf_step makes exactly the launches it makes without them.  While either is set the steps run eagerly (no
 * hipGraph replay: the particle count changes) and pbf_steps does not fuse finalise(t) with predict(t + 1).
 * NaN, infinite or negative rate / width, non-finite coordinates and a NULL array with n > 0 return PBF_ERR_INVALID and
 * leave the setting unchanged.  Growth is bounded by the capacity: the count of the last upload, or — with pbf_reserve
 * before pbf_upload — the larger of that and the reserve, exactly (the slack the arrays carry beyond a reserve for slab
 * mode is not counted).  A step whose emission would exceed it returns PBF_ERR_INVALID before anything is launched, the
 * state untouched.  The emitted count is host
 * arithmetic; the drained count is data: one host read-back per step while a drain is set and there are particles (a
 * kernel writes the count and a sequence number to pinned memory, the host polls: no hipStreamSynchronize), none
 * otherwise.  Slab mode is not supported: setting either on a slab-attached ctx, and pbf_slab_step(s) with either
 * set, return PBF_ERR_STATE. */
typedef struct pbf_source { /* sph::Source, src/sph.hpp:62-67 */
  uint64_t tag;
  double centre[3], velocity[3], colour[4], rate;
} pbf_source;
typedef struct pbf_drain { /* sph::Drain, src/sph.hpp:69-72 */
  double centre[3], width;
} pbf_drain;
int pbf_set_sources(pbf_ctx *ctx, size_t n, const pbf_source *sources);
int pbf_set_drains(pbf_ctx *ctx, size_t n, const pbf_drain *drains);
/* emit + drain alone (ompsph.hpp:93-118), like the other pbf_stage_*: exactly what pbf_step does first */
int pbf_stage_scene(pbf_ctx *ctx, const pbf_params *params);
/* host read-backs made for drains so far (at most one per step) */
uint64_t pbf_scene_host_syncs(const pbf_ctx *ctx);
/* ompsph.hpp:167-186 on the keys and table of the last step: for each world point (3 doubles) the cell code of
 * point / scale - minExtent; if code + 1 < pbf_table_size, the ids of the FLUID particles of that cell in sorted order,
 * otherwise none.  counts[i] = the full count of point i, ids[i * cap_per_point ..] its first min(count, cap_per_point)
 * ids (the rest of the row is not written).  Synchronises: meant for a handful of points per frame.  PBF_ERR_STATE before
 * any step, after anything that invalidated the table (upload, pbf_stage_scene), with params whose bounds or scale
 * describe another grid than the last step's (nothing is launched, pbf_table_size unchanged) and in slab mode. */
int pbf_query_cells(pbf_ctx *ctx, const pbf_params *params, size_t n_points, const double *points, uint32_t *counts,
                    uint64_t *ids, size_t cap_per_point);

/* ---- introspection (parity tests, Stopwatch analogue) ------------------------------------ */
enum pbf_buffer {
  PBF_BUF_KEYS = 0,   /* uint32[n]  Morton cell key per particle, current device order */
  PBF_BUF_TABLE = 1,  /* uint32[table_size] = the reference's gridTable (sph.hpp:238-250) */
  PBF_BUF_PSTAR = 2,  /* N[4n]: pStar.xyz, lambda */
  PBF_BUF_NBR_COUNT = 3, /* uint32[n]: neighbour list of each particle after the last list build: low 8 bits = length (<= 160),
                            upper 24 bits = the 120-slot pool chunk holding its slots 40..159 when the length exceeds 40 (two-tier
                            lists, csrc/pbf_kernels.hpp NbrLists); 0xFFFFFFFF = more than 160 survivors (or the chunk pool ran
                            dry): the particle walks its cells; diagnostic, list gather only */
  PBF_BUF_OMEGA = 4,  /* N[4n]: {omega.xyz, 0}, the vorticity estimate of the last step run with pbf_params.vorticity
                         (opt-in extra, absent from the reference), device order; PBF_ERR_STATE when there is none */
  PBF_BUF_SURFACE = 5, /* N[4n]: {n.xyz, rho} of the last surface-tension pass (pbf_set_surface_tension), device order; zero
                          for obstacles; PBF_ERR_STATE when there is none */
  PBF_BUF_DENSITY = 6, /* N[n]: rho_i of the last density pass (pbf_diagnostics with PBF_DIAG_DENSITY), device order; zero for
                          obstacles; PBF_ERR_STATE when there is none, or once the arrays have changed since */
  PBF_BUF_COUNT_ = 7, /* the values ABOVE it, not a bound for `which`: PBF_BUF_WHITEWATER below is 7 as well */
};
/* read through pbf_read_buffer like the values above (enum pbf_buffer itself is closed: its PBF_BUF_COUNT_ stays 7) */
enum {
  PBF_BUF_COLLIDER_PUSH = 8, /* N[8n]: {A.xyz, hits, B.xyz, 0} of pbf_set_collider_reaction, the order of PBF_BUF_PSTAR */
  PBF_BUF_WHITEWATER = 7, /* N[4n]: {I_ta, I_wc, E_k, n_d} of the last pbf_whitewater_step, device order; zero for obstacles;
                             PBF_ERR_STATE when there is none, or once the arrays have changed since */
};
int pbf_read_buffer(pbf_ctx *ctx, int which, void *host, size_t bytes);
size_t pbf_table_size(const pbf_ctx *ctx);                /* Morton(extent), sph.hpp:240 */
int pbf_grid_extent(const pbf_ctx *ctx, uint64_t extent[3], double min_extent[3]); /* ompsph.hpp:132-135 */

/* ---- diagnostics of the resident state (no reference counterpart) ----------------------------------------------
 * What a caller otherwise downloads every array for: did the run blow up, how fast is the fastest particle (the number a
 * CFL time step needs), energy and momentum, how far the fluid is from rest density after K iterations, how many
 * neighbours a particle has (the number h, "list_max" and "nbr_chunks" are tuned by).  Computed on the device and
 * reduced there in a fixed order without atomics: the same state gives the same bytes, call after call.  Its own call on
 * the ctx stream, synchronising (one polled read-back of the 216-byte record, no hipStreamSynchronize); never part of a
 * step or of a captured hipGraph, and a step after it runs exactly as it would have without.
 *
 * Stream part (always): over exactly the arrays pbf_download would return now — valid whenever pbf_download is, straight
 * after pbf_upload included.  `params` may be NULL when what == 0.  A fluid particle with a non-finite component of position
 * or velocity counts in n_nonfinite and in nothing else; obstacles count in n_obstacle and in nothing else; n_fluid counts
 * the remaining, finite fluid particles (the three add up to pbf_count).  Over those, every term formed in double from the
 * stored values widened to double (on fp32 contexts too):
 *   mass = sum m;  moment = sum m x (x the world position: the centre of mass is moment / mass);  momentum = sum m v;
 *   kinetic = 1/2 sum m (vx^2 + vy^2 + vz^2);  max_speed = sqrt(max (vx^2 + vy^2 + vz^2));  aabb_min / aabb_max = the
 *   per-axis extrema of the position.
 * With no finite fluid particle every floating field is 0.
 *
 * Density part (what & PBF_DIAG_DENSITY): the preconditions of pbf_surface — a step has run and its table is still valid,
 * PBF_ERR_STATE otherwise; so are params whose bounds or scale describe another grid than the last step's (as in
 * pbf_query_cells).  On the final pStar with the candidates of the predict-time 27 cells, exactly as the extras passes
 * run: for each fluid particle  rho_i = m_i sum_j W_poly6(r_ij)  over the candidates j with r <= h, i itself and obstacles
 * included — lambda's own expressions (ompsph.hpp:215-232), i.e. the residual iteration K + 1 would see;
 * C_i = rho_i / rho0 - 1 (rho0 = 6378);  nbr_i = the candidates j != i with r <= h.  n_density = fluid particles evaluated;
 * rho_min / rho_max / rho_mean over rho_i;  err_mean = mean |C|, err_max = max |C|, compression_mean = mean max(C, 0);
 * nbr_max / nbr_mean over nbr_i.  The means are double sums of the per-particle values (computed in N), divided once.
 * Without the flag the density fields are 0.  PBF_BUF_DENSITY reads rho_i back.
 *
 * PBF_ERR_INVALID: out == NULL, unknown bits in `what`, params == NULL with the density flag.  Slab mode is not supported
 * (global sums need an all-reduce and the ghost copies would have to be left out): PBF_ERR_STATE for both parts.  On every
 * error *out is untouched. */
enum { PBF_DIAG_DENSITY = 1u << 0 };
typedef struct pbf_diag {
  uint64_t n_fluid, n_obstacle, n_nonfinite;
  double mass, moment[3], momentum[3], kinetic, max_speed;
  double aabb_min[3], aabb_max[3];
  uint64_t n_density, nbr_max;
  double rho_min, rho_max, rho_mean, err_mean, err_max, compression_mean, nbr_mean;
} pbf_diag;
int pbf_diagnostics(pbf_ctx *ctx, const pbf_params *params, uint32_t what, pbf_diag *out);

/* ---- sampling the SPH fields at arbitrary points and on a regular lattice (no reference counterpart) -----------
 * "What is the fluid doing HERE": density, velocity and colour at a point that is not a particle — a gauge or probe at a
 * fixed position, a density or velocity volume for rendering, slices or a grid code — without downloading the particles.
 * One kernel, one lane per point, on the keys and table of the last step.  Its own call on the ctx stream, synchronising
 * (plain copies and one hipStreamSynchronize, like pbf_query_cells); never part of a step or of a captured hipGraph, and
 * a step after it runs exactly as it would have without.
 *
 * The outputs are RAW SUMS, not Shepard-normalised values: sums are what can be bounded, and what adds across slabs.
 * v(x) = mv / weight and c(x) = mc / weight are the caller's division (the C++ shim and the Python binding offer it, with 0
 * where weight == 0).
 *
 * Preconditions, those of the density part of pbf_diagnostics: a step has run and its table is still valid; params
 * describe the last step's grid (bounds and scale, as in pbf_query_cells); not slab mode (a point near a cut needs both
 * ranks' candidates) — PBF_ERR_STATE otherwise.
 * PBF_ERR_INVALID: points, out or params NULL when n > 0; a non-finite point, origin or spacing; unknown bits in `what`;
 * mv or mc non-NULL without its flag; n, or the product of dims, >= 2^31; a zero in dims.  On every error the output arrays
 * are untouched.  n = 0 returns PBF_OK and launches nothing.
 *
 * The point: rounded to N (the ctx's float or double), then x_s = point / scale in N (solver frame).  Its cell is
 * cell_coord((x_s - minExtent) / h) per axis — pbf_query_cells' expressions (truncation towards zero: a quotient in
 * (-1, 0) is cell 0).  Unlike pbf_query_cells, which keeps the low 10 bits of whatever comes out, a quotient of 2^31 or
 * more in magnitude is outside without being converted, and the coordinates are tested against the extent (below).  A lattice
 * point is origin[a] + N(i_a) * spacing[a], origin and spacing rounded to N first, formed in N on the device as one multiply
 * and one add (not contracted): pbf_sample_lattice returns bit for bit what pbf_sample_points returns on the same points
 * formed that way by the caller.
 * The grid test: the point is IN THE GRID iff every cell coordinate lies in [0, extent_a) of pbf_grid_extent and the cell's
 * code + 1 < pbf_table_size.  Otherwise outside = 1 and every other field of its record is 0.
 * The candidates: the particles of the 27 cells around that cell, by their PREDICT-TIME keys, evaluated at their FINAL pStar
 * (the one PBF_BUF_PSTAR reads), with mass, velocity and colour as pbf_download would return them now — the frame the
 * extras passes and PBF_DIAG_DENSITY use.  It follows that a particle which delta-p carried more than a cell away from its
 * predict-time cell can be missed although it lies within h of the point, exactly as those passes miss it.
 * The pair term is the density sum's, with the candidate's own mass:  r = |x_s - p_j| (IEEE sqrt; with
 * PBF_FLAG_FAST_MATH the pair kernels' v_rsq form),  in = r <= h,  w = m_j * (poly6Factor * (d * d * d)),  d = h * h - r * r.
 * An excluded candidate's term is SELECTED to +0, never multiplied by 0.  Obstacles count in rho and count[1] only.
 * Summation: one accumulator set per point, in N, in the walk's order (27 cells x fastest, then y, then z; within a cell
 * the sorted order).  The record of a point therefore does not depend on which other points are in the call, on their order
 * or on n. */
enum { PBF_SAMPLE_VELOCITY = 1u << 0, PBF_SAMPLE_COLOUR = 1u << 1 };
typedef struct pbf_sample_out {   /* caller-owned host arrays of N (float / double as the ctx); any may be NULL */
  void *rho;       /* N[n]   sum over ALL candidates j with r <= h of  m_j W_poly6(r)   (solver frame; compare with rho0 = 6378) */
  void *weight;    /* N[n]   the same sum over FLUID candidates only */
  void *mv;        /* N[3n]  sum over fluid candidates of (m_j W) v_j   — needs PBF_SAMPLE_VELOCITY */
  void *mc;        /* N[4n]  sum over fluid candidates of (m_j W) c_j   — needs PBF_SAMPLE_COLOUR */
  uint32_t *count; /* uint32[2n]  {fluid, obstacle} candidates with r <= h */
  uint8_t *outside;/* uint8[n]    1 = the point's cell is not a cell of the last step's grid: its record is all zeros */
} pbf_sample_out;
int pbf_sample_points(pbf_ctx *ctx, const pbf_params *params, size_t n, const double *points /* 3n, world */, uint32_t what,
                      const pbf_sample_out *out);
/* point (i, j, k) of the lattice has index (i * dims[1] + j) * dims[2] + k */
int pbf_sample_lattice(pbf_ctx *ctx, const pbf_params *params, const double origin[3], const double spacing[3],
                       const uint64_t dims[3], uint32_t what, const pbf_sample_out *out);

/* ---- whitewater: spray, foam and air bubbles on the resident state (no reference counterpart) ----------------------
 * Diffuse particles after Ihmsen, Akinci, Akinci & Teschner 2012, "Unified spray, foam and air bubbles for particle-based
 * fluids" (The Visual Computer 28): a pool owned by the ctx, advected and refilled by pbf_whitewater_step from the state the
 * last pbf_step left.  Its own call on the ctx stream, synchronising (one polled read-back of the 56-byte record, no
 * hipStreamSynchronize); never part of a step or of a captured hipGraph, and a step after it runs exactly as it would have
 * without.  The same resident state, configuration, pool and frame give the same bytes under every setting of pbf_set_option.
 *
 * One step, everything in N, selects and never multiplies by 0 (csrc/pbf_whitewater.hpp restates every expression in its
 * order; DESIGN.md has the reasoning):
 *  1 advect   each diffuse particle, with nF = count[0], v_f = mv / weight of pbf_sample_points at its position (nF = 0 and
 *             v_f = 0 outside the grid or where weight == 0), g = params->constant_force:
 *               spray   nF <  spray_below:  v = g dt + v
 *               bubble  nF >= bubble_from:  v = (v + (dt * -k_b) g) + k_d (v_f - v)
 *               foam    otherwise:          v = v_f;  life = life - dt
 *             then x += dt v in the relation the fluid's stored position and velocity have (positions in world units,
 *             velocities in world / scale per time: x = (v dt + x / scale) * scale), x clamped to min_bound / max_bound.  It
 *             dies when life <= 0, when a component is not finite, or when nF == 0 and the clamp moved it (it left the fluid
 *             and hit a wall: a deviation from the paper).
 *  2 normals  the surface-tension pass's density and normal (pbf_set_surface_tension's n_i), into fields of its own:
 *             PBF_BUF_SURFACE and a later surface-tension pass do not notice.
 *  3 potentials of each fluid particle i over the fluid candidates j != i of its 27 predict-time cells with 0 < r <= h, on
 *             the final pStar (solver frame) and the stored velocities, W = 1 - r / h, x_ij = x_i - x_j, v_ij = v_i - v_j:
 *               I_ta  = sum |v_ij| (1 - vhat_ij . xhat_ij) W                         (a term is 0 when |v_ij| == 0)
 *               kappa = sum over j with xhat_ji . nhat_i < 0 of (1 - nhat_i . nhat_j) W     (0 when n_i or n_j is zero)
 *               I_wc  = kappa if vhat_i . nhat_i >= 0.6, else 0;      E_k = m_i |v_i|^2 / 2
 *             Phi(I, tau) = (min(I, tau[1]) - min(I, tau[0])) / (tau[1] - tau[0]);
 *             n_d = Phi_k (k_ta Phi_ta + k_wc Phi_wc) dt (0 when v_i == 0);  count_i = min(floor(n_d + u(i, 0)), 1024);
 *             the counts are scanned in 32 bits: their sum over one step must stay below 2^32 (always so below 4 M particles).
 *  4 emit     child k of parent i goes to slot survivors + (sum of count_j over j < i in device order) + k; children past
 *             the capacity are dropped and counted.  With vhat = v_i / |v_i|, e1, e2 orthonormal to it, r_V = h scale / 2:
 *               r = r_V sqrt(u1), theta = 2 pi u2, hh = u3 dt |v_i|
 *               x_d = x_i + r cos(theta) e1 + r sin(theta) e2 + hh vhat;   v_d = r cos(theta) e1 + r sin(theta) e2 + v_i
 *               life = lifetime[0] + Phi_k (lifetime[1] - lifetime[0]);    parent_id = id_i
 *             Its kind until its first advection: the class of the parent's count of fluid candidates within h, itself included.
 *  5 compact  the survivors of 1 keep their order, the children follow in slot order.
 * u for parent id, frame (whitewater steps since pbf_whitewater_configure), child k, stream s (0: the count, with k = 0;
 * 1, 2, 3: u1, u2, u3):  u = (mix(seed ^ mix(id) ^ mix(frame * 2^32 + k * 4 + s)) >> 40) * 2^-24,  mix = splitmix64:
 * x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31.
 *
 * pbf_whitewater_configure copies the configuration, resets the frame counter and keeps the pool when the capacity is
 * unchanged (capacity 0 frees it and turns the feature off).  PBF_ERR_INVALID, the ctx unchanged: config == NULL; k_ta or
 * k_wc negative or not finite; a tau pair with max <= min, lifetime with max < min, or either not finite; k_b not finite;
 * k_d outside [0, 1]; spray_below > bubble_from; capacity >= 2^31.
 * pbf_whitewater_upload replaces the pool's content (restart, tests): vel == NULL = at rest, life == NULL = lifetime[1];
 * kind = spray, parent_id = 2^64 - 1.  PBF_ERR_STATE without a pool; PBF_ERR_INVALID for n > capacity or pos == NULL with n > 0.
 * pbf_whitewater_step: the preconditions of pbf_sample_points — a step has run, its table is valid, params describe that
 * grid — and a configured pool, PBF_ERR_STATE otherwise; also in slab mode (a diffuse particle near a cut needs both ranks'
 * candidates and the pool would have to migrate).  PBF_ERR_INVALID: params == NULL, dt or scale <= 0.  On every error nothing
 * is launched and the pool is untouched.  `out` may be NULL.  kind[] counts the pool after the step. */
enum { PBF_WW_SPRAY = 0, PBF_WW_FOAM = 1, PBF_WW_BUBBLE = 2 };
typedef struct pbf_whitewater {
  uint64_t capacity;           /* diffuse particles the pool holds; 0 = off, frees the pool */
  uint64_t seed;
  double k_ta, k_wc;           /* particles per unit time at potential 1: trapped air, wave crest */
  double tau_ta[2], tau_wc[2], tau_k[2];   /* clamp ranges {min, max}, min < max */
  double lifetime[2];          /* {min, max}: life = min + Phi_k * (max - min) */
  double k_b, k_d;             /* bubbles: buoyancy, drag in [0, 1] */
  uint32_t spray_below, bubble_from; /* fluid candidates within h: < spray_below spray, >= bubble_from bubble, else foam
                                        (Ihmsen: 6, 20) */
} pbf_whitewater;
typedef struct pbf_whitewater_stats {
  uint64_t alive, emitted, dropped, died, kind[3];
} pbf_whitewater_stats;
int pbf_whitewater_configure(pbf_ctx *ctx, const pbf_whitewater *config);
int pbf_whitewater_upload(pbf_ctx *ctx, size_t n, const void *pos, const void *vel, const void *life);
int pbf_whitewater_step(pbf_ctx *ctx, const pbf_params *params, pbf_whitewater_stats *out);
size_t pbf_whitewater_count(const pbf_ctx *ctx);
/* pos / vel = 3 values of N per diffuse particle, life = 1; any pointer may be NULL */
int pbf_whitewater_download(pbf_ctx *ctx, void *pos, void *vel, void *life, uint8_t *kind, uint64_t *parent_id);

/* ---- whitewater against the solids: diffuse particles collide with the collider and the scenery (opt-in) -------------
 * A ctx that never calls pbf_set_whitewater_solids runs pbf_whitewater_step launch for launch and byte for byte as without
 * this block.  With the setting on, every diffuse particle is projected out of the collider and then out of the scenery
 * after its advection, its velocity gets a contact response, and no particle is left inside a solid at the end of the call.
 * The setting is a wish: it needs no installed lattice and outlives pbf_set_collider, pbf_set_scenery, their _mesh forms,
 * clearing, poses, bodies and friction.  Each pbf_whitewater_step collides with whichever of the two lattices is installed
 * when it runs; with neither installed the pass is not launched.  The setting touches no collider mode and drops no captured
 * graph (the whitewater step is never captured), and a fluid step never notices it.
 *
 * The contract (csrc/pbf_whitewater_solids.hpp restates it).  Everything is in N, in the order written, not contracted;
 * PBF_FLAG_FAST_MATH does not reach it; sqrt and divide are IEEE.  Per diffuse particle after step 1 (advect) above: x its
 * world position (clamped to the box), v its velocity in the solver frame, its alive flag, and nF exactly as the advection
 * forms it (weight == 0 ? 0 : count[0]).  A particle that is dead on entry is skipped: nothing of it is moved or counted.
 * e = N(restitution), f = N(friction).
 *
 *   q_a = x_a / scale
 *   collider installed:  (q1, hit1) = what pbf_collider_sample computes for this q: the posed contract through the pose record
 *                        when one is set, else the static contract;      else q1 = q, hit1 = false
 *   scenery installed:   (q2, hit2) = the static contract on q1 with the scenery's lattice;    else q2 = q1, hit2 = false
 *   x'_a = (hit1 || hit2) ? min(maxB_a, max(minB_a, q2_a * scale)) : x_a                       (bits kept without a hit)
 *
 *   response(d, vb) for a solid that moved the point by d (solver frame) and has the velocity vb there:
 *     len = sqrt((d_x d_x + d_y d_y) + d_z d_z)      act = hit && len > 0        n_a = d_a / len
 *     u_a = v_a - vb_a      un = (u_x n_x + u_y n_y) + u_z n_z      ut_a = u_a - un * n_a
 *     v_a <- (act && un < 0) ? (vb_a + (1 - f) * ut_a) - (e * un) * n_a : v_a                  (bits kept otherwise)
 *   collider first:  d = q1 - q;   r_a = q1_a * scale - t_a;   c_x = W_y r_z - W_z r_y  (y, z cyclic; each product rounded,
 *                    one subtraction, as the friction contract forms it);   vb_a = (V_a + c_a) / scale
 *                    V, W = N(velocity), N(angular_velocity) of the body's state as the kernel finds it while a body is on;
 *                    else the friction record's while friction is on;  else vb = 0.
 *                    t = the pose record's trans as the kernel finds it (no pose ever set: 0)
 *   then scenery:    d = q2 - q1;  vb = 0, on the velocity the collider's response left
 *   alive <- alive && !(absorb && nF == 0 && (hit1 || hit2))
 *
 * Life, kind and parent are untouched.  Obstacle particles play no part.  Outside a lattice nothing is loaded, NaN included.
 * The box wins over both solids and the scenery over the collider, as in delta-p.  A receding particle (un >= 0) keeps its
 * velocity, so spray a moving collider has just pushed is not slowed; a push the box undoes entirely (len == 0) still
 * counts as a hit.  A child that step 4 (emit) places is projected by the same two position contracts before the call
 * returns: its velocity and life are kept, it never dies at birth, and it counts in born_inside when either lattice hit.
 * pbf_whitewater_stats.died includes the absorbed particles; alive + died keeps its meaning.  The call still makes exactly
 * one read-back.  The same resident state, solids, configuration, pool and frame give the same bytes under every setting of
 * pbf_set_option.
 *
 * pbf_set_whitewater_solids(ctx, NULL) turns the setting off.  PBF_ERR_INVALID, the ctx unchanged: restitution or friction
 * outside [0, 1] or NaN, reserved != 0.  pbf_whitewater_solids_stats (an observer, synchronises): the counts of the last
 * whitewater step — hit_collider / hit_scenery: particles alive on entry with hit1 / hit2 — and `step`, the whitewater steps
 * run since the setting was turned on; PBF_ERR_STATE while the setting is off or no whitewater step has run since it was
 * turned on, PBF_ERR_INVALID for out == NULL.
 *
 * Limitations: the observers (pbf_sample_*, the surface, the diagnostics, anisotropy) still do not see the solids; whitewater
 * is still not available in slab mode; no swept collision (spray that crosses a solid thinner than its own step in one step
 * passes through); the potentials ignore the solids (trapped air against a wall and obstacle particles stay as they are);
 * diffuse particles are massless, so they exert no force or friction on a body. */
typedef struct pbf_whitewater_solids {
  double restitution;   /* e in [0, 1] */
  double friction;      /* f in [0, 1]: the share of the tangential relative velocity a hit removes */
  uint32_t absorb;      /* != 0: a diffuse particle with nF == 0 that hits a solid dies (what the box walls already do) */
  uint32_t reserved;    /* 0 */
} pbf_whitewater_solids;
/* (the struct shares its name with the call that fills it, so it has no typedef: write `struct pbf_whitewater_solids_stats`) */
struct pbf_whitewater_solids_stats {
  uint64_t hit_collider, hit_scenery, absorbed, born_inside, step;
};
int pbf_set_whitewater_solids(pbf_ctx *ctx, const pbf_whitewater_solids *cfg);               /* NULL: off */
int pbf_whitewater_solids_stats(pbf_ctx *ctx, struct pbf_whitewater_solids_stats *out);      /* observer, synchronises */

/* ---- per-particle anisotropy after Yu & Turk 2013 on the resident state (no reference counterpart) --------------------
 * Yu & Turk, "Reconstructing surfaces of particle-based fluids using anisotropic kernels" (ACM TOG 32(1)): for each particle
 * a smoothed centre and an anisotropy matrix G_i from the weighted covariance of its neighbourhood — what a renderer needs
 * to splat ellipsoids (flat discs on sheets, needles on jets) instead of equal spheres, as Macklin & Mueller draw their
 * fluid.  One gather (AnisotropyOp, csrc/pbf_anisotropy.hpp) through whichever gather kernel the ctx is set to.  Its own call
 * on the ctx stream, synchronising (plain async copies of the arrays asked for and one hipStreamSynchronize); never part of a
 * step or of a captured hipGraph, and a step after it runs exactly as it would have without.  The same resident state and
 * configuration give the same bytes under every setting of pbf_set_option.
 *
 * Frame: that of the extras passes, PBF_DIAG_DENSITY and pbf_sample_points — the final pStar (solver frame: world / scale,
 * h = pbf_desc.h), the candidates of the 27 predict-time cells in walk order.  Candidates are FLUID particles only.
 * Everything in N, not contracted.  DEVIATION from the paper: the support radius is h, not 2 h (the cells are h wide and the
 * walk sees 27 of them).
 * For a fluid particle i, over the fluid candidates j with r = |p_j - p_i| <= h (pair_geom's r; with PBF_FLAG_FAST_MATH its
 * v_rsq form), i itself included, d = p_j - p_i; an excluded candidate's terms are SELECTED to +0, never multiplied by 0;
 * one accumulator set per lane, in walk order:
 *   q = r / h;   w = 1 - q * q * q
 *   S += w;   M_a += w * d_a;   Q_ab += (w * d_a) * d_b   for ab = xx yy zz xy xz yz        (ten sums)
 *   n_i = the candidates j != i (told apart by index, as PBF_DIAG_DENSITY does) with r <= h
 * then
 *   mu_a = M_a / S
 *   centre_a = (p_a + smoothing * mu_a) * scale                  (world units: the one product finalise uses)
 *   C_ab = (Q_ab / S - mu_a * mu_b) / (h * h)                    (the covariance in units of h^2)
 *   C = R diag(sigma) R^T, sigma_1 >= sigma_2 >= sigma_3, negative round-off clamped to 0: cyclic Jacobi on the symmetric
 *       3 x 3, pivots in the order (0,1), (0,2), (1,2), Rutishauser's rotation t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),
 *       theta = (a_qq - a_pp) / (2 a_pq), t selected to 0 where a_pq == 0, a fixed number of sweeps per precision (4 and 4:
 *       no data-dependent exit), then a compare-select sorting network
 *   if n_i > min_neighbours:  st_k = k_s * max(sigma_k, sigma_1 / k_r)          otherwise  st_k = k_n  and  R = I
 *   G_ab = (((R_a1 * R_b1) * (1 / st_1) + (R_a2 * R_b2) * (1 / st_2)) + (R_a3 * R_b3) * (1 / st_3)) / h
 *        i.e. G = (1 / h) R diag(1 / st) R^T, in the SOLVER frame: the ellipsoid |G x| <= 1 has semi-axes h st_k
 *   axes = the three unit eigenvectors as rows, in descending order; the third is negated when their determinant is negative
 *   radii = st (dimensionless)
 * k_s: a uniformly filled ball has sigma = 0.15 under this weight (int r^4 (1 - r^3) / (3 int r^2 (1 - r^3)) = (3/40) / (1/2)),
 * so k_s = 20 / 3 gives st ~ 1 in the bulk.  A particle with n_i > min_neighbours whose candidates all coincide with it
 * (sigma_1 == 0) gets st = 0 and a G that is not finite.
 * An obstacle's record: centre = its stored position, every other field 0.
 *
 * The arrays come back in device order (the order pbf_download returns now), COMPONENT-MAJOR: value k of particle i is at
 * [k * n + i], n = pbf_count — centre 3 planes (x y z), G 6 (xx yy zz xy xz yz), axes 9 (row-major: axis 1 x y z, axis 2 ...),
 * radii 3; neighbours[i] = n_i.  Any pointer may be NULL.
 * Preconditions, those of pbf_sample_points: a step has run and its table is still valid; params describe the last step's
 * grid; not slab mode (a particle near a cut needs both ranks' candidates) — PBF_ERR_STATE otherwise.
 * PBF_ERR_INVALID: config, out or params NULL; dt or scale <= 0; smoothing outside [0, 1]; k_r < 1 or not finite; k_s or k_n
 * not finite or <= 0.  On every error nothing is launched and the outputs are untouched.  pbf_count == 0 returns PBF_OK
 * (after the argument and slab checks) and writes nothing. */
typedef struct pbf_anisotropy { double smoothing, k_r, k_s, k_n; uint32_t min_neighbours; } pbf_anisotropy;
typedef struct pbf_anisotropy_out { void *centre /*N[3n] world*/, *G /*N[6n]*/, *axes /*N[9n]*/, *radii /*N[3n]*/;
                                    uint32_t *neighbours /*[n]*/; } pbf_anisotropy_out;   /* any pointer may be NULL */
int pbf_anisotropy_compute(pbf_ctx *ctx, const pbf_params *params, const pbf_anisotropy *config, const pbf_anisotropy_out *out);

/* Device self-test of the trimmed exact sqrt / divides the precise pair terms use (csrc/pbf_kernels.hpp sqrt_rsq /
 * div_seeded / div_ranged) against the compiler's full IEEE forms, exhaustively: mismatches[0] sqrt over EVERY fp32 value
 * >= 2^-75; mismatches[1] (h - r)^2 / r over every fp32 d2 whose root lies in [1e-8, h], for the context's own h and
 * three more; mismatches[2] x / poly6(0.3 h) over every fp32 x with 1e-30 <= |x| <= 1e30 or x == 0 (one mismatch is the
 * sign of a zero quotient, which is only ever squared); mismatches[3] delta-p's x / RHO — trimmed where the numerator is
 * in range, the compiler's divide otherwise — over EVERY fp32 x.  [0], [1], [3] must be 0, [2] <= 1.
 * On an fp64 context the same four categories are swept for the fp64 forms (v_rsq_f64-seeded sqrt = the compiler's own
 * sequence without its rescale wrappers; Newton divides with one exact-residual correction) over 1.07e10 pseudo-random
 * operands EACH (an exhaustive fp64 sweep is impossible): every exponent of the stated ranges equally often plus the pair
 * terms' own operand ranges densely (csrc/pbf_kernels.hpp k_selftest_math64); all four must be 0. */
int pbf_selftest_math(pbf_ctx *ctx, uint64_t mismatches[4]);

/* The same sweep with a count of what it visited, and the trimmed divides at the operands their later callers hand them
 * (csrc/pbf_kernels.hpp k_selftest_divides / k_selftest_divides64).  mismatches[k] / visited[k]:
 *   [0 .. 3]  pbf_selftest_math's four categories; visited = operands compared (quotients, for [1]);
 *   [4]  div_ranged(a, d) as the marching-cubes field uses it: every fp32 d with 1e-18 < d <= 64; a = 25, 1 and
 *        `numerators` (<= 64) signed pseudo-random 2^e m, e uniform over [-100, 5], per divisor;
 *   [5]  the same divisors with the numerators the field can also meet — +-0, denormals, |a| < 2^-100 (6 fixed +
 *        `numerators` drawn per divisor) — in the field's form: the trimmed divide where every numerator of the hit is at
 *        least 2^-100 in magnitude, the compiler's divide otherwise;
 *   [6]  div_seeded(a, r, y) as surface tension uses it: r, y from the trimmed sqrt of every fp32 d2 whose root lies in
 *        [1e-8, 0.2]; a = 0 and `numerators` signed pseudo-random 2^e m, e uniform over [-100, 20], per divisor;
 *   [7]  the operands of [5] through div_ranged alone, without the fall-back (what the guard is for: reported only).
 * Every fp32 category is exhaustive in the divisor, so visited[k] is a number the caller can compute.  On an fp64 context
 * the categories are drawn pseudo-randomly (divisors log-uniform over the range and uniform over [0.03, 8]; numerators
 * below 2^-100 for [5] and [7], as in fp32), 1.07e10 each — visited[k] = rounds x threads — and `numerators` is ignored. */
int pbf_selftest_divides(pbf_ctx *ctx, uint32_t numerators, uint64_t mismatches[8], uint64_t visited[8]);

/* Mean milliseconds per call of each stage since the last pbf_reset_stage_times (needs
 * PBF_FLAG_STAGE_TIMING).  names[i] points at static strings that follow the reference's Stopwatch
 * entries (ompsph.hpp:130,157,161,188,209,252); an entry named "stage/part" is a sub-interval of "stage"
 * (e.g. "sph-lambda/list-build": the neighbour-list kernel inside the lambda stage) and must not be added
 * to it.  Returns the number of entries (<= cap). */
int pbf_stage_times(pbf_ctx *ctx, const char **names, double *mean_ms, uint64_t *calls, int cap);
int pbf_reset_stage_times(pbf_ctx *ctx);

/* ---- marching-cubes surface (reference: config.surface, src/sph.hpp:82-95,102; src/omp/ompsph.hpp:277-477) ---
 * Runs on the state the last pbf_step left (its grid table is still valid): scalar field on a lattice of
 * floor(extent * resolution) + 1 nodes per axis, triangles per cube, emission in cube order.
 * pbf_surface returns the triangle count; pbf_download_mesh copies 3 vertices per triangle:
 * vs / ns = 9 values of N per triangle, cs = 12 (the reference's ColouredMesh, src/sph.hpp:105-112).
 *
 * Slab mode (a ctx attached with pbf_slab_attach, more than one rank):
 *   - pbf_surface is COLLECTIVE: every rank calls it with the same params and mc (three exchange rounds: the copies'
 *     colours, then the {v, normal} and the colour halves of one node plane).
 *   - It must follow pbf_slab_step(s) directly, while the copies of the neighbours' boundary columns are still in the
 *     arrays: after pbf_download / pbf_upload (they drop the copies) it returns PBF_ERR_STATE and exchanges nothing.  It may
 *     be repeated, with other mc, until then.
 *   - Rank r owns the node planes x of the global lattice with cuts[r] <= floor(N(x) / N(resolution)) < cuts[r + 1] and
 *     returns the triangles of the cubes whose lower plane is one of them.  Concatenated in rank order, the ranks' meshes
 *     are the global mesh in the global cube order (x-major).  A rank without particles returns its planes like far nodes
 *     of a single device (v = 0, NaN normals and colours) and no triangle.
 *   - pbf_read_lattice returns sample[0] = the rank's own planes, plus one where node planes remain to its right: the
 *     first plane of the right-hand neighbour, received from it, byte for byte.  sample[1], sample[2] are the global ones.
 *   - The indexed mesh is refused (pbf_surface_indexed below).
 *   - PBF_ERR_INVALID, on every rank alike and before anything is exchanged (pbf_comm_rounds unchanged, the state intact, a
 *     following pbf_surface at a workable resolution succeeds), when a rank with a left neighbour owns no node plane while
 *     planes remain to its right — a slab narrower than one lattice step, e.g. one column at resolution 0.7: the plane its
 *     left neighbour needs belongs to a rank the one-hop exchange does not reach.  A rightmost rank without planes is legal. */
typedef struct pbf_mc_params {
  double resolution, isolevel, particle_size, particle_influence; /* sph::McParams */
} pbf_mc_params;
int pbf_surface(pbf_ctx *ctx, const pbf_params *params, const pbf_mc_params *mc, uint64_t *n_triangles);
int pbf_download_mesh(pbf_ctx *ctx, void *vs, void *ns, void *cs);
/* The same mesh in PAGE-LOCKED host memory owned by the ctx (one DMA at PCIe speed instead of three pageable copies into
 * freshly allocated vectors: 54 MB at 1 M particles); the pointers stay valid until the next pbf_surface / pbf_destroy.
 * The C++ shim builds Result::mesh's vectors from them (range construction: no zero fill, the three copies in parallel). */
int pbf_map_mesh(pbf_ctx *ctx, const void **vs, const void **ns, const void **cs);
/* the lattice of the last pbf_surface / pbf_surface_indexed: sample[3] nodes per axis, 4 + 4 values of N per node
 * {v, normal} {colour} */
int pbf_read_lattice(pbf_ctx *ctx, uint64_t sample[3], void *pn, void *c);
/* The same surface as an INDEXED mesh (no reference counterpart): one vertex per crossed lattice edge, triangles as index
 * triples.  Same preconditions, same field and same triangles in the same order as pbf_surface; de-indexed, it is that
 * soup, except that every vertex is interpolated from the edge's lower node towards its +axis node — the soup interpolates
 * cube edges 2, 3, 6 and 7 from the other end, a few units in the last place away.  Node (x, y, z), index
 * (x * sample[1] + y) * sample[2] + z, owns the edges to its +x, +y and +z neighbours; an edge is crossed iff exactly one end
 * value is < isolevel; vertices are numbered by ascending owner index, x < y < z within a node.  Two triangles that share an
 * edge share two indices: the mesh is watertight by construction.  40 V + 12 T bytes in fp32 instead of 120 T.
 * PBF_ERR_INVALID at 2^29 vertices or more.
 * vs / ns = 3 values of N per vertex, cs = 4, tris = 3 uint32 per triangle; any pointer of pbf_download_mesh_indexed may be
 * NULL.  pbf_map_mesh_indexed: page-locked staging owned by the ctx, valid until the next surface call / pbf_destroy.
 * The two kinds exclude each other: after pbf_surface_indexed there is no soup (pbf_download_mesh / pbf_map_mesh return
 * PBF_ERR_STATE), after pbf_surface no indexed mesh (the _indexed readers return PBF_ERR_STATE).
 * Slab mode is not supported: an edge on a cut plane is owned by a node of another rank, so the vertex numbering would
 * need a scan across ranks — PBF_ERR_STATE on a ctx configured with pbf_slab_configure. */
int pbf_surface_indexed(pbf_ctx *ctx, const pbf_params *params, const pbf_mc_params *mc, uint64_t *n_vertices,
                        uint64_t *n_triangles);
int pbf_download_mesh_indexed(pbf_ctx *ctx, void *vs, void *ns, void *cs, uint32_t *tris);
int pbf_map_mesh_indexed(pbf_ctx *ctx, const void **vs, const void **ns, const void **cs, const uint32_t **tris);

/* ---- anisotropic-kernel surface: the iso-surface of Yu & Turk's field (no reference counterpart) -----------------------
 * pbf_surface / pbf_surface_indexed with another scalar field: phi(a) = sum_j W(a - centre_j, G_j) over the ellipsoids of
 * pbf_anisotropy_compute — flat where the fluid is a sheet, thin along a jet, smooth in the bulk — instead of the reference's
 * sum size / |l|^infl over equal spheres, which stays what pbf_surface computes.  Only the field stage differs: the lattice
 * geometry, the count, the scans, the emission (indexed != 0: one vertex per crossed edge, n_vertices required) and the rule
 * that the two mesh kinds exclude each other are pbf_surface's, and pbf_download_mesh / pbf_map_mesh / their _indexed forms /
 * pbf_read_lattice return this surface exactly as they return the stock one.
 * The call discipline is pbf_anisotropy_compute's: its own call on the ctx stream, never part of a step or a captured
 * hipGraph, no stage timer; a step after it, and a pbf_surface after it, produce the bytes they would have produced without.
 * The same state and configuration give the same bytes under every setting of pbf_set_option.
 *
 * CONTRACT.  The field is a function of exactly these bytes: the arrays pbf_anisotropy_compute returns for the same state and
 * `kernel` (centre, G, radii), the particles' positions, colours and types, and the predict-time cell table.  Everything in
 * N, in the order written, not contracted (csrc/pbf_aniso_field.hpp holds the same text beside the code).
 * Two DEVIATIONS from the paper: the support of pbf_anisotropy_compute is h, not 2 h; and each ellipsoid is shrunk uniformly
 * by a factor f >= 1 (below) so that it stays inside the 27 cells a lattice node looks at.  The paper's m_j / rho_j is a
 * constant here (the constraint holds the density at rho_0) and is absorbed into the isolevel — which therefore has no
 * default: phi is 1 / (radii_1 radii_2 radii_3) at the centre of an isolated ellipsoid with f = 1.
 *
 * Record of fluid particle j, H = h * scale:
 *   e = centre_j - pos_j (world);   disp = sqrt((e_x e_x + e_y e_y) + e_z e_z) / H;   f = max(1, radii_1 / (0.99 - disp))
 *   G''_ab = G_ab * (f / scale)                      (world frame; largest semi-axis of |G''(a - centre_j)| < 1: H radii_1 / f,
 *                                                    so the ellipsoid reaches at most disp + radii_1 / f <= 0.99 H from pos_j)
 *   D = 1 / (((f f) f) ((radii_1 radii_2) radii_3))  (det(h f G): Yu & Turk's ||G|| normalisation)
 *   rho2 = (((H radii_1) / f) ((H radii_1) / f)) * 1.5
 *   An obstacle, a particle whose D or G'' is not finite (sigma_1 == 0 above) or one with disp >= 0.99 contributes nothing.
 * Node a (coordinates and cell z as pbf_surface computes them): the candidates are the particles of the cells z - 1, z, z + 1
 * per axis, a cell outside [0, extent - 1] SKIPPED (pbf_surface clamps it and visits face cells more than once; this field
 * visits every cell once), slots in ascending order (x fastest), candidates in table order.  Per candidate:
 *   d = a - centre;   no hit unless (d_x d_x + d_y d_y) + d_z d_z < rho2   (a conservative pre-test that never decides:
 *                                                                          q2 < 1 implies |d| < H radii_1 / f)
 *   y_a = (G''_ax d_x + G''_ay d_y) + G''_az d_z;   q2 = (y_x y_x + y_y y_y) + y_z y_z;   a hit iff q2 < 1
 *   s = 1 - q2;   t = D ((s s) s);   phi += t
 *   z_a = (G''_ax y_x + G''_ay y_y) + G''_az y_z;   g_a += ((-6 D) (s s)) z_a        (grad phi: points into the fluid)
 *   C += t colour_j
 * Stored: phi > 0: {phi, n}, n_a = (-g_a) / len with len = sqrt((g_x g_x + g_y g_y) + g_z g_z) (0 where len == 0): outwards,
 * the stock convention — a value < isolevel is outside in both fields; colour C / phi.  Otherwise phi = 0, normal 0, colour 0:
 * never NaN (pbf_surface stores NaN at a node without hits).
 * Then every node with phi == 0 that has a 6-neighbour with phi > 0 takes as colour the sum of those neighbours' colours in
 * the order -x +x -y +y -z +z divided by their number (its normal stays 0): the far end of a crossed edge has no hit when
 * the support is compact, and the vertex colours would otherwise be mixed with zero.
 *
 * PBF_ERR_INVALID: a NULL argument; indexed without n_vertices; dt or scale <= 0; resolution or isolevel not finite or <= 0;
 * what pbf_anisotropy_compute rejects in `kernel`; the lattice-size limits of pbf_surface / pbf_surface_indexed.
 * PBF_ERR_STATE: no step has run or its table is stale; params describe another grid than the last step's; the ctx is
 * slab-configured, attached or holds ghost copies.  On every error nothing is launched and the previous mesh and lattice stay
 * readable.  pbf_count == 0 returns PBF_OK with zero triangles (after the argument and slab checks). */
typedef struct pbf_aniso_surface { double resolution, isolevel; pbf_anisotropy kernel; } pbf_aniso_surface;
int pbf_surface_anisotropic(pbf_ctx *ctx, const pbf_params *params, const pbf_aniso_surface *cfg,
                            int indexed, uint64_t *n_vertices /* may be NULL unless indexed */, uint64_t *n_triangles);

/* ---- multi-GPU: slab decomposition along x (no reference counterpart: it is single-device) ------
 * One process per GPU.  Every rank uses the GLOBAL grid (same pbf_params bounds), owns the cell columns
 * [xlo, xhi) and keeps a one-cell layer of COPIES ("ghosts", type bit PBF_TYPE_GHOST) of its x-neighbours'
 * boundary columns.  The product path is pbf_slab_attach + pbf_slab_step further down: the whole step including the
 * RCCL exchanges runs inside the library.  The calls of THIS section are the same step cut into its stages (select /
 * pack / append / unpack on the device, the caller moves the wire buffers, which are device pointers) — kept so that
 * tests can check every stage against the oracle and drive several ranks on one GPU; see pbf-sph_amd/slab.py:
 *   predict -> migrate -> add_migrants -> ghosts -> add_ghosts -> sort -> diffuse ->
 *   K x { lambda -> pack/exchange/unpack -> delta -> pack/exchange/unpack } -> finalise -> finish */
enum { PBF_TYPE_GHOST = 2 };
enum { PBF_REC_MIGRANT = 0, PBF_REC_GHOST = 1, PBF_REC_FIELD = 2 };
typedef struct pbf_slab_cut {
  uint32_t xlo, xhi;           /* owned cell columns [xlo, xhi), grid coordinates of pbf_grid_extent */
  int32_t has_left, has_right; /* is there a rank on that side */
} pbf_slab_cut;
int pbf_reserve(pbf_ctx *ctx, size_t capacity); /* room for migrants + copies / for what sources emit; call before pbf_upload */
/* Optional, before the first step: key the particles in a rank-LOCAL x frame (origin = PBF_SLAB_FRAME_MARGIN columns left of this slab's first column), so the grid table covers only the slab + ghost columns instead of Morton(global extent) — on an
 * elongated N-slab box that is 2 M entries per rank instead of 138 M at N = 8.  left_xlo / right_xlo = the
 * xlo of the neighbouring slabs (0 for rank 0 / unused without that neighbour); records are re-keyed on arrival.
 * cut = NULL returns to global keys. */
#define PBF_SLAB_FRAME_MARGIN 6u /* columns between the local frame's origin and the first owned column */
int pbf_slab_configure(pbf_ctx *ctx, const pbf_slab_cut *cut, uint32_t left_xlo, uint32_t right_xlo);
size_t pbf_slab_record_bytes(const pbf_ctx *ctx, int kind);
/* after pbf_stage_predict: compact the particles that stay, pack the leavers; counts[2] = records for left / right */
int pbf_slab_migrate(pbf_ctx *ctx, const pbf_slab_cut *cut, void *send_left, void *send_right, uint32_t cap_records,
                     uint32_t counts[2]);
int pbf_slab_add_migrants(pbf_ctx *ctx, const void *recv_left, uint32_t n_left, const void *recv_right, uint32_t n_right);
/* pack copies of the first / last owned column; remembers the sources for pbf_slab_pack */
int pbf_slab_ghosts(pbf_ctx *ctx, const pbf_slab_cut *cut, void *send_left, void *send_right, uint32_t cap_records,
                    uint32_t counts[2]);
/* append the neighbours' copies and rebuild the cell histogram; pbf_stage_sort comes next */
int pbf_slab_add_ghosts(pbf_ctx *ctx, const void *recv_left, uint32_t n_left, const void *recv_right, uint32_t n_right);
/* after each lambda / delta launch: owners' {pStar, lambda} -> wire, wire -> copies (PBF_REC_FIELD records) */
int pbf_slab_pack(pbf_ctx *ctx, void *send_left, void *send_right);
int pbf_slab_unpack(pbf_ctx *ctx, const void *recv_left, const void *recv_right);
int pbf_slab_finish(pbf_ctx *ctx); /* after finalise: drop the copies */
size_t pbf_owned_count(const pbf_ctx *ctx);
/* load balance: owned particles per GLOBAL grid column (keys of the last pbf_stage_predict), 1024 bins; synchronises.
 * The driver all-reduces the histograms and moves the cuts (pbf-sph_amd/slab.py recut()). */
int pbf_slab_column_histogram(pbf_ctx *ctx, uint32_t out[1024]);

/* ---- communicator + whole slab step behind the C ABI ------------------------------------------------------
 * (no reference counterpart).  A pbf_comm links this rank with its left (rank - 1) and right (rank + 1) slab:
 *   RCCL over xGMI  pbf_comm_unique_id on rank 0, the 128 bytes are broadcast by the caller over any channel, then
 *                   pbf_comm_create_rccl on every rank = ncclCommInitRank; the exchanges are
 *                   ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the solver's stream (no host sync);
 *   host callback   bring-up and tests (several ranks sharing ONE GPU under gloo): the library stages the wire
 *                   buffers through pinned host memory and calls `fn` to move the bytes (return 0 = ok).
 * pbf_slab_attach hands the communicator, the cuts (nranks + 1 column boundaries, identical on every rank) and the
 * wire capacities to the ctx; pbf_slab_step then runs ONE step including every exchange:
 *   predict -> [migrants] -> [ghost copies] -> sort -> diffuse -> K x { lambda -> [field] -> delta -> [field] }
 *   -> finalise [-> xsph / vorticity extras with 3 more field rounds when requested]
 *                              ([..] = one exchange round: 2 + 2K rounds per step)
 * The two assembly rounds carry their record counts in the header of a fixed-size first message {header | first
 * cap_* records} (no count round trip); the host reads those counts once per assembly round (2 small synchronising
 * read-backs per step), the 2K field rounds need none.  Only when a side holds more records than the first message
 * takes (a re-cut hands whole columns over) a second, exactly sized exchange follows.  Running out of wire buffer
 * (half the particle capacity per neighbour) is an error (PBF_ERR_COMM), never silent loss. */
typedef struct pbf_comm pbf_comm;
#define PBF_COMM_ID_BYTES 128
typedef int (*pbf_exchange_fn)(void *user, const void *send_left, size_t send_left_bytes, const void *send_right,
                               size_t send_right_bytes, void *recv_left, size_t recv_left_bytes, void *recv_right,
                               size_t recv_right_bytes); /* host pointers */
int pbf_comm_unique_id(void *id128);
int pbf_comm_create_rccl(const void *id128, int nranks, int rank, int device, pbf_comm **out);
int pbf_comm_create_host_callback(pbf_exchange_fn fn, void *user, int nranks, int rank, pbf_comm **out);
void pbf_comm_destroy(pbf_comm *comm);
const char *pbf_comm_last_error(const pbf_comm *comm); /* comm may be NULL: last failed create on this thread */
uint64_t pbf_comm_rounds(const pbf_comm *comm);        /* exchange rounds so far */
/* in-place sum over all ranks of `count` uint32 in DEVICE memory (load balance: column histograms); RCCL
 * communicators only (a host-callback communicator returns PBF_ERR_COMM: its caller reduces on the host) */
int pbf_comm_allreduce_u32(pbf_comm *comm, void *device_u32, size_t count, void *stream);
/* cuts[nranks + 1]; cap_migrants / cap_ghosts = records per neighbour in the FIRST message of the two assembly rounds
 * (size them for an ordinary step: a fraction of / one boundary column).  The ctx keeps the pointer
 * to comm (not owned).  Switches the ctx to the rank-local key frame (pbf_slab_configure). */
int pbf_slab_attach(pbf_ctx *ctx, pbf_comm *comm, const uint32_t *cuts, uint32_t cap_migrants, uint32_t cap_ghosts);
int pbf_slab_set_cuts(pbf_ctx *ctx, const uint32_t *cuts); /* load balance: new cuts (same on every rank) */
int pbf_slab_step(pbf_ctx *ctx, const pbf_params *params);
int pbf_slab_steps(pbf_ctx *ctx, const pbf_params *params, uint32_t count);
/* host read-backs pbf_slab_step has made so far: exactly 2 per step — the counts of the two assembly rounds, which size the
 * append launches and the new particle count (the 2K field rounds need none).  No hipStreamSynchronize: a one-wave kernel
 * writes the six words and then a sequence number into pinned host memory, the host polls that word. */
uint64_t pbf_slab_host_syncs(const pbf_ctx *ctx);

/* ---- scene factory (sph.hpp:127-186; dam-break: SURVEY.md §8d) — host only, no GPU needed -- */
size_t pbf_scene_cubes(int fp64, size_t count, uint64_t *id, uint8_t *type, void *mass, void *pos, void *vel,
                       void *colour);
size_t pbf_scene_dambreak(int fp64, size_t nominal, uint64_t *id, uint8_t *type, void *mass, void *pos, void *vel,
                          void *colour, double *box_side);
/* applyMotionSinXCosZ (sph.hpp:147-158): writes min/max bound of `base` shifted for `frame` into `out` */
void pbf_apply_motion(int fp64, const pbf_params *base, uint64_t frame, pbf_params *out);
/* simpleConfigWith2Cubes' SphParams (sph.hpp:168-175) with K = iteration */
void pbf_default_params(uint64_t iteration, double box_side, pbf_params *out);

#ifdef __cplusplus
}
#endif
#endif

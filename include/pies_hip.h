/* pies_hip.h -- C ABI of the MI355X (gfx950) implementation of the Pies solver loop.
 *
 * The reference (nithinp7/Pies) has no FFI: hosts include <Pies/Solver.h> and call the C++ class
 * (Include/Pies/Solver.h:40-116 in the reference tree).  This header is the boundary a binding for that
 * class would use: plain pointers and sizes, no C++ or torch types.  `include/Pies/Solver.h` in this
 * repository is the C++ drop-in class written on top of it.  Each entry point cites the reference
 * interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - every call returns 0 (PIES_OK) or a PIES_ERR_* code; pies_last_error() gives the text;
 *  - one handle = one HIP device + one stream; calls on one handle are serialised by the caller
 *    (the reference solver is single-caller as well);
 *  - inputs are copied, no caller buffer is retained;
 *  - node ids returned/accepted are global (offset by the node count at the time of the add*),
 *    exactly like the reference's add and create functions (Src/PrimitiveUtilities.cpp:53-57,358);
 *  - there is no CPU fallback: without a gfx950 device pies_create fails.
 */
#ifndef PIES_HIP_H
#define PIES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: PIES_SCHEDULE_LAYERED, PIES_KERNEL_LAYER (pies_launch_counts now fills PIES_KERNEL_COUNT = 19 entries)
 * 3: pies_tick_begin / pies_export_acquire / pies_export_release, pies_read_positions_strided, pies_get_pcg_health,
 *    pies_set_pcg_retry, PIES_FLAG_REFERENCE_COLLISION_ORDER, pies_profile_in_situ; PIES_SCHEDULE_DEFAULT */
#define PIES_ABI_VERSION 4

typedef struct pies_solver pies_solver_t;

/* Pies::SolverOptions, field for field (Include/Pies/Solver.h:23-38). solver: 0 = PBD, 1 = PD. */
typedef struct pies_options {
  float fixedTimestepSize;                   /* 0.012f */
  uint32_t timeSubsteps;                     /* 1 */
  uint32_t iterations;                       /* 4 */
  uint32_t collisionStabilizationIterations; /* 4 */
  float collisionThresholdDistance;          /* 0.1f */
  float collisionThickness;                  /* 0.05f */
  float gravity;                             /* 10.0f */
  float damping;                             /* 0.006f */
  float friction;                            /* 0.01f */
  float staticFrictionThreshold;             /* 0.f */
  float floorHeight;                         /* 0.0f */
  float gridSpacing;                         /* 2.0f */
  uint32_t threadCount;                      /* 8 (accepted; only orders PD floor contacts) */
  int32_t solver;                            /* 1 (PD) */
} pies_options_t;

enum {
  PIES_OK = 0,
  PIES_ERR_INVALID = 1,     /* bad argument (null, out-of-range node id, size mismatch) */
  PIES_ERR_HIP = 2,         /* HIP runtime error, or no gfx950 device */
  PIES_ERR_STATE = 3,       /* call not valid in the handle's current state */
  PIES_ERR_UNSUPPORTED = 4  /* feature not available in this build */
};

enum { PIES_SOLVER_PBD = 0, PIES_SOLVER_PD = 1 }; /* Pies::SolverName, Solver.h:21 */

/* constraint containers, in the order Solver::tickPBD / tickPD visit them */
enum {
  PIES_POSITION = 0, /* PositionConstraint      Constraints.cpp:58-74  */
  PIES_DISTANCE = 1, /* DistanceConstraint      Constraints.cpp:11-56  */
  PIES_TET = 2,      /* TetrahedralConstraint   Constraints.cpp:76-184 */
  PIES_VOLUME = 3,   /* VolumeConstraint        Constraints.cpp:186-310 (PD only) */
  PIES_BEND = 4,     /* BendConstraint          Constraints.cpp:312-394 */
  PIES_SHAPE = 5,    /* ShapeMatchingConstraint ShapeMatchingConstraint.cpp:6-122 (PD only) */
  PIES_GOAL = 6,     /* GoalMatchingConstraint  ShapeMatchingConstraint.cpp:124-177 (PD only) */
  PIES_TRIANGLES = 7,
  PIES_LINES = 8,
  PIES_NODES = 9,
  PIES_SYSTEM_NNZ = 10, /* pies_count only: stored entries of the PD system matrix (after pies_finalize) */
  PIES_REST_SETS = 11,  /* pies_count only: distinct sets of element constants in the PD local step's rest dictionary (0: the
                         * per-element arrays are read; after pies_finalize) */
  PIES_ROW_STENCILS = 12, /* pies_count only: distinct rows in the row dictionary of the PD system matrix (0: SELL arrays only) */
  PIES_PD_TILES = 13,     /* pies_count only: tiles of the PD strain + volume local step (0: one record per (element, node)) */
  PIES_PD_TILE_RECORDS = 14, /* pies_count only: (tile, node) sums the right-hand side gathers */
  PIES_PD_CG_SINGLE = 15, /* pies_count only: 1 when the captured global step runs one launch per CG iteration */
  PIES_PD_WINDOW_ENTRIES = 16, /* pies_count only: stored entries (padding included) of the windowed system matrix the CG iterations
                                  stream - value + 16-bit window slot each -, 0: not built (row dictionary, or the SELL arrays) */
  PIES_PD_WINDOW_HALO = 17,    /* pies_count only: its halo entries over all chunks (columns staged in LDS besides a chunk's own rows) */
  PIES_NODE_PAIRS = 18,        /* CollisionConstraint (node-node, PD)  CollisionConstraint.cpp:7-65: an EXTENSION container, see
                                  pies_add_node_pair_constraints */
  PIES_NODES_RENUMBERED = 19,  /* pies_count only: 1 when the device holds the nodes in another numbering than the host's
                                  (PIES_FLAG_RENUMBER_NODES, decided by pies_finalize), else 0 */
  PIES_NODE_CONTACTS = 20,     /* pies_count only: node-node contacts of the last PD substep (PIES_FLAG_PD_NODE_CONTACTS; synchronises),
                                  0 before the first tick and without the flag */
  PIES_SKINS = 21,             /* pies_count only: embedded surface meshes (pies_add_skin), an EXTENSION */
  PIES_SKIN_VERTICES = 22,     /* pies_count only: their vertices, over all skins */
  PIES_LAYER_REST_SETS = 23,   /* pies_count only: distinct sets of rest constants (Qinv, strain limits, w) in the rest dictionary of
                                  schedule LAYERED's tetrahedral container (PBD), 0: the per-element arrays are read (after
                                  pies_finalize; tuning switch PIES_LAYER_REST_DICT=0 forces 0) */
  PIES_LAYER_MAX_TILES = 24,   /* pies_count only: tiles (= workgroups of a launch) of the phase of schedule LAYERED's plan that has
                                  most, 0 when the plan is not active (after pies_finalize); more than the device's 256 compute
                                  units select the four-wavefronts-per-SIMD kernel variants */
  PIES_LAYER_MAX_CLASS = 25,   /* pies_count only: constraints of the largest colour class of any tile and container of schedule
                                  LAYERED's plan, 0 when the plan is not active (after pies_finalize); with at most 256 tiles it
                                  selects the workgroup of the layer kernel: 256 threads up to 256, 512 up to 512, else 1 024 */
  PIES_PD_CG_BLOCKS = 26       /* pies_count only: workgroups of the PD global step's CG launches that synchronise through a grid
                                  barrier (after pies_finalize; 0 for PBD): one per 256 rows, at most half of what the device holds
                                  resident at once, so that a second solver on the card leaves room */
};

/* How the sequential Gauss-Seidel sweeps of tickPBD (Solver.cpp:58-75) are mapped to the device.
 *  EXACT    : dependency levels of the container order; bit-identical to processing the containers
 *             sequentially in the order the host added the constraints (the reference's semantics).
 *  COLOURED : greedy graph colouring; identical to a sequential sweep over the containers re-ordered
 *             colour by colour (pies_get_order returns that order).  Fewer, larger launches.
 *  LAYERED  : breadth-first levels of the constraint graph; the constraints between two adjacent levels are
 *             swept colour by colour by one workgroup with the nodes resident in LDS (two launches per
 *             iteration; wide bodies are cut into strips by a second levelling: four phases per container).
 *             Identical to a sequential sweep in the order pies_get_order returns.  Falls back to COLOURED
 *             for scenes without distance / tetrahedral / bend constraints and for squat bodies of fewer than
 *             300k nodes whose cross-sections do not fit one workgroup (measured slower there). */
enum { PIES_SCHEDULE_EXACT = 0, PIES_SCHEDULE_COLOURED = 1, PIES_SCHEDULE_LAYERED = 2 };
/* What pies_create and Pies::Solver start with: the schedule bench.py's headline figure is measured on.  Every schedule
 * is a Gauss-Seidel sweep over the same constraints with the same per-constraint arithmetic; LAYERED and COLOURED
 * visit them in another order than the host added them, EXACT in exactly that order (and then also runs the node-node
 * pass in the reference's order, see PIES_FLAG_REFERENCE_COLLISION_ORDER).  bench.py reports how far the orders are
 * apart (`order_deviation`) and the EXACT throughput beside the headline.  The environment variable
 * PIES_SCHEDULE=exact|coloured|layered overrides the default at pies_create (not an explicit pies_set_schedule). */
#define PIES_SCHEDULE_DEFAULT PIES_SCHEDULE_LAYERED

enum {
  PIES_FLAG_RELEASE_HINGE = 0,  /* Solver::releaseHinge (Solver.h:52, Solver.cpp:59) */
  PIES_FLAG_NODE_COLLISIONS = 1,    /* extension, default 1: 0 skips the PBD node-node pass (Solver.cpp:81-130) */
  PIES_FLAG_TRIANGLE_COLLISIONS = 2, /* extension, default 1: 0 skips the PD point-triangle contacts (Solver.cpp:693-797) */
  /* PBD node-node pass (Solver.cpp:85-130).  1: the reference's loop -- nodes in ascending index, each querying the cell
   * range of its *current* position, every overlapping pair resolved at once -- executed as one sequential chain on
   * the device (bit-identical to the loop, slow).  0: the parallel visiting rule of DESIGN.md section 6 (same contact
   * set and per-pair arithmetic, different order).  Default: 1 under PIES_SCHEDULE_EXACT, 0 otherwise; setting the
   * flag overrides that until the schedule changes. */
  PIES_FLAG_REFERENCE_COLLISION_ORDER = 3,
  /* The order of the PBD node-node pass, by name (value: PIES_COLLISION_ORDER_*).  Every order uses the reference's per-pair
   * arithmetic; the loop is order dependent (Solver.cpp:85-130 moves both nodes at once).
   *  REFERENCE : the reference's loop (see above): node i meets every node of every bucket of the cell range recomputed from
   *              i's LIVE position when its turn comes (SpatialHash.h:101-106), in each direction, itself included.
   *  PAIRS and GROUPS are a documented deviation: the same per-pair arithmetic, but node i meets node j once per grid cell
   *  both were INSERTED into at the start of the iteration - the same meetings unless a node crosses a cell boundary
   *  inside the pass, and a different order.
   *  PAIRS     : default under COLOURED / LAYERED.  A node's meetings with itself first, then the pairs {i < j} in
   *              ascending order of a 64-bit mix of (i, j), each as its m visits of i to j and m visits of j to i; executed
   *              by dependency levels, one lane per pair.
   *  GROUPS    : rounds 1-2's order (nodes grouped by minimum cell, 27 residue classes, ascending index inside a group);
   *              needs cell ranges of at most two cells per axis: a scene with gridSpacing < 2 (r_max + 0.5) runs REFERENCE instead.
   * PIES_FLAG_REFERENCE_COLLISION_ORDER = 0 selects PAIRS. */
  PIES_FLAG_COLLISION_ORDER = 4,
  /* Extension, default 0.  1: pies_finalize may renumber the nodes of a PD scene on the device, for meshes whose ids do not
   * follow space (a tetrahedraliser's output).  It sorts the nodes along a Hilbert curve of their positions and keeps that order
   * when (a) the scene's own order would not give the system matrix a row dictionary (a createTetBox lattice keeps its order) and
   * (b) the curve cuts the halo per row of the windowed matrix to 0.8 of the scene's own order or less.  Every id and every
   * array the host sees stays in host numbering (node state, export frames, container ids, contacts, the tile plan); the
   * results are the same solve in another summation order (within the PD tolerance).  PBD keeps the
   * identity.  Takes effect at the next pies_finalize (the scene is rebuilt); pies_count(PIES_NODES_RENUMBERED) and
   * pies_get_node_order report the outcome. */
  PIES_FLAG_RENUMBER_NODES = 5,
  /* Extension, default 0.  1: a PD scene detects node-node contacts on the device once per substep, after the prediction
   * (where tickPD would, Solver.cpp:240), with the rule of Solver::_parallelComputeCollisions (Solver.cpp:509-637, never called by
   * the reference) made explicit: nodes i, j are in contact when they share a cell of the node grid (gridSpacing, each node's range
   * from its radius - the grid of the PBD pass), |p_i - p_j|^2 < (r_i + r_j)^2 in fp32 (the test of CollisionConstraint.cpp:20-24),
   * invMass_i + invMass_j > 0 (:36 divides by it), and no element joins them (distance, tetrahedral, volume or bend constraint,
   * triangle, listed node pair: a non-overlapping CollisionConstraint anchors its nodes with w = 1e5).
   * Every contact is a CollisionConstraint (CollisionConstraint.cpp:7-65, w = 1e5): w on the node's diagonal, w * projected in
   * the right-hand side of every local step, and the friction loop of Solver.cpp:398-428 after the velocity update, in ascending
   * order of a 64-bit mix of the pair's device ids (run in parallel rounds, the same result bit for bit); the contacts' nodes get
   * their floor friction (:473-484) after it.  Nothing is summed with atomics: runs are reproducible.  A node holds at most
   * PIES_PD_NODE_CONTACT_PARTNERS partners (pies_set_tuning, read at pies_finalize, default 32); more latch the failure
   * (pies_failed, pies_last_error names the list).  Memory: nodes x partners x 4 bytes (1M nodes x 32 = 128 MB) plus the node
   * grid.  With the flag the PD CG ceiling defaults to 256 iterations (pies_set_pcg overrides).  PBD ignores the flag (its own
   * node-node pass: PIES_FLAG_NODE_COLLISIONS).  Takes effect at the next pies_finalize.  See pies_get_node_contacts. */
  PIES_FLAG_PD_NODE_CONTACTS = 6
};
enum { PIES_COLLISION_ORDER_REFERENCE = 0, PIES_COLLISION_ORDER_GROUPS = 1, PIES_COLLISION_ORDER_PAIRS = 2 };

/* node state selectors for pies_read_nodes / pies_write_nodes */
enum { PIES_NODE_POSITION = 0, PIES_NODE_PREV_POSITION = 1, PIES_NODE_VELOCITY = 2, PIES_NODE_RADIUS = 3, PIES_NODE_INV_MASS = 4 };

/* ---- lifetime ------------------------------------------------------------------------------ */
/* device == PIES_DEVICE_NONE creates a host-only handle: scenes can be built and schedules inspected
 * (pies_get_ids/_rest/_order/_batches), every call that would compute returns PIES_ERR_HIP. */
#define PIES_DEVICE_NONE (-1)
/* Solver::Solver(const SolverOptions&) (Solver.cpp:11-17).  options == NULL -> reference defaults. */
int pies_create(const pies_options_t* options, int device, pies_solver_t** out);
/* Solver::~Solver (Solver.cpp:19-23) */
int pies_destroy(pies_solver_t* s);
/* Solver::clear (Solver.cpp:488-507); also resets the PD system. */
int pies_clear(pies_solver_t* s);
const char* pies_last_error(const pies_solver_t* s);
int pies_abi_version(void);
void pies_default_options(pies_options_t* out);
/* Solver::getOptions (Solver.h:71) */
int pies_get_options(const pies_solver_t* s, pies_options_t* out);

/* ---- scene construction (setup time; host side) --------------------------------------------- */
/* Solver::addNodes (PrimitiveUtilities.cpp:42-75): mass 1, radius 0.5, velocity 0.  pos: n x 3. */
int pies_add_nodes(pies_solver_t* s, uint32_t n, const float* pos, uint32_t* first_id);
/* Bulk node append with explicit state; vel/radius/inv_mass may be NULL (0 / 0.5 / 1). */
int pies_add_nodes_ex(pies_solver_t* s, uint32_t n, const float* pos, const float* vel, const float* radius,
                      const float* inv_mass, uint32_t* first_id);
/* create*Constraint factories (Constraints.cpp:39-56, 65-74, 130-184, 257-310, 368-394): rest state is
 * taken from the nodes' current positions, like the reference factories do. ids: n x {1,2,4,4,4}. */
int pies_add_position_constraints(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w);
int pies_add_distance_constraints(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w);
int pies_add_tet_constraints(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w, float min_strain, float max_strain);
int pies_add_volume_constraints(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w, float compression, float stretching);
int pies_add_bend_constraints(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w);
/* EXTENSION (not reachable in the reference): n node-node CollisionConstraints over the node pairs ids[2 i], ids[2 i + 1]
 * (Src/CollisionConstraint.cpp:7-65, w = 1e5 of Include/Pies/CollisionConstraint.h:14).  The reference's only source of these
 * constraints, Solver::_parallelComputeCollisions (Solver.cpp:509-637), is never called, and tickPD calls none of the type's three
 * methods - only its friction loop (Solver.cpp:398-428) walks the always-empty list.  Here a host may list pairs itself; PD then
 * treats them the way it treats the live collision constraints: projection in every local step (:10-41), w on both diagonal entries
 * of the system (:43-47), w * projected in the right-hand side (:49-65), the friction loop after the velocity update.  PBD scenes
 * ignore the list (the PBD tick has its own node-node pass, Solver.cpp:85-130).  Default: none. */
int pies_add_node_pair_constraints(pies_solver_t* s, uint32_t n, const uint32_t* ids);
/* ShapeMatchingConstraint over the listed nodes (ShapeMatchingConstraint.cpp:6-48); material coordinates
 * are the nodes' current positions, as createShapeMatching* / addLinkedRegions pass them.  PD only. */
int pies_add_shape_constraint(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w);
/* GoalMatchingConstraint over the listed nodes (ShapeMatchingConstraint.cpp:124-137).  PD only. */
int pies_add_goal_constraint(pies_solver_t* s, uint32_t n, const uint32_t* ids, float w, uint32_t* goal_index);
/* GoalMatchingConstraint::setTransform (:175-177); m16 column-major like glm::mat4 */
int pies_set_goal_transform(pies_solver_t* s, uint32_t goal, const float m16[16]);
/* Solver::addFixedRegions / updateFixedRegions / addLinkedRegions (PrimitiveUtilities.cpp:77-162);
 * mats16: n column-major 4x4 region-to-world matrices (the region is the unit box [-1,1]^3) */
int pies_add_fixed_regions(pies_solver_t* s, uint32_t n, const float* mats16, float w);
int pies_update_fixed_regions(pies_solver_t* s, uint32_t n, const float* mats16);
int pies_add_linked_regions(pies_solver_t* s, uint32_t n, const float* mats16, float w);
/* Solver::createShapeMatchingBox (:985-1048; spacing fixed to 0.5 and mass 10 like the reference) and
 * Solver::createShapeMatchingSheet (:1050-1125; reference 50 x 50, 3x3 patches) */
int pies_create_shape_matching_box(pies_solver_t* s, const float translation[3], uint32_t count_x, uint32_t count_y, uint32_t count_z, float w);
int pies_create_shape_matching_sheet(pies_solver_t* s, uint32_t W, uint32_t H, const float translation[3], float scale, float w);
/* Solver::_triangles entries (Solver.h:194); ids: n x 3 */
int pies_add_triangles(pies_solver_t* s, uint32_t n, const uint32_t* ids);
/* Solver::createTetBox (PrimitiveUtilities.cpp:330-618) on a W x H x D lattice (reference: 3x3x3, hinged
 * 10x2x10).  flags bit0: push VolumeConstraints too (the reference always does); bit1: surface triangles. */
int pies_create_tet_box(pies_solver_t* s, uint32_t W, uint32_t H, uint32_t D, const float translation[3], float scale,
                        const float velocity[3], float w, float mass, uint32_t flags);
/* Solver::createBox (PrimitiveUtilities.cpp:620-847) on a W x H x D lattice (reference: 5x5x5).
 * existing != 0: only add the distance constraints, over an existing lattice starting at node existing_first. */
int pies_create_box(pies_solver_t* s, uint32_t W, uint32_t H, uint32_t D, const float translation[3], float scale,
                    float w, int existing, uint32_t existing_first, uint32_t flags);
/* Solver::createSheet (:849-976, reference 20x20) and Solver::createBendSheet (:1127-1289, reference 10x10) */
int pies_create_sheet(pies_solver_t* s, uint32_t W, uint32_t H, const float translation[3], float scale, float mass, float w);
int pies_create_bend_sheet(pies_solver_t* s, uint32_t W, uint32_t H, const float translation[3], float scale, float w);

/* EXTENSION (the reference draws the simulation nodes themselves; Include/Pies/Tetrahedron.h and Solver.h's _spatialHashTets /
 * TetCompRange are the unfinished element grid this stands in for): an embedded surface mesh, a SKIN.  Each of the n_vertices
 * render vertices (positions: n x 3) is bound once, here, to one of the n_tets listed tetrahedra (tet_node_ids: n x 4 global node
 * ids; they need not be constraints of the scene) with barycentric weights; after any tick pies_read_skin /
 * pies_export_acquire_skin deliver the deformed vertices and their normals, evaluated on the device.  tri_ids (n_triangles x 3
 * indices into THIS skin's vertices; NULL with 0) only serve the normals.
 * The binding rule, in fp32 on the node positions at the time of the call: the candidates of vertex v are the listed tetrahedra
 * whose axis-aligned box, grown by max_distance on every side, contains v (bounds included); a tetrahedron whose
 * det [p1 - p0, p2 - p0, p3 - p0] is below FLT_MIN in magnitude, or whose inverse is not finite, is never a candidate.  The
 * barycentric coordinates are w_k = det(with column k replaced by v - p0) / det for k = 1, 2, 3 and w0 = 1 - (w1 + w2 + w3);
 * the candidate with the largest min(w0, w1, w2, w3) wins, the lowest index on a tie.  A vertex without a candidate fails the
 * call with PIES_ERR_INVALID (pies_last_error names the vertex) and nothing is added; so do a node id out of range, a triangle
 * index >= n_vertices, n_vertices == 0 and a negative or non-finite max_distance.  Candidates are found through a uniform grid
 * over the element boxes (host side, like all scene construction).
 * The binding is kept in host numbering and survives pies_finalize, later add* / create* calls (node ids never shift),
 * pies_set_solver and PIES_FLAG_RENUMBER_NODES; pies_clear drops every skin.  skin_id (may be NULL) receives 0, 1, ... */
int pies_add_skin(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles, const uint32_t* tri_ids,
                  uint32_t n_tets, const uint32_t* tet_node_ids, float max_distance, uint32_t* skin_id);
/* The stored binding of a skin, per vertex: tet = index into the tetrahedra given, node_ids = its four nodes (host ids), weights =
 * (w0, w1, w2, w3) with w0 = 1 - (w1 + w2 + w3) exactly as the device evaluates it.  Any array may be NULL; n receives the
 * vertex count, capacity is in vertices.  Works on PIES_DEVICE_NONE handles. */
int pies_get_skin_binding(const pies_solver_t* s, uint32_t skin, uint32_t* tet, uint32_t* node_ids, float* weights, uint32_t capacity,
                          uint32_t* n);

/* EXTENSION: the generalised winding number of a triangle mesh at the CELL CENTRES of a lattice, evaluated on the device; the
 * diagnostics and the test surface of the kernel pies_add_tri_mesh_volume classifies cells with.  Sample (i, j, k) of the
 * dims = (nx, ny, nz) lattice is c = origin + ((i, j, k) + 0.5) * cell and has index (i * ny + j) * nz + k (k fastest, the node
 * order of pies_create_tet_box).  For a triangle (a, b, d), in fp32 without fused multiply-adds: A = a - c, B = b - c, D = d - c
 * with lengths la, lb, ld; num = det [A, B, D] = A.x (B.y D.z - D.y B.z) - B.x (A.y D.z - D.y A.z) + D.x (A.y B.z - B.y A.z);
 * den = la lb ld + (A.B) ld + (B.D) la + (D.A) lb, summed left to right; Omega = 2 atan2f(num, den), and 0 when num and den are
 * both 0 or Omega is not finite.  w(c) = (sum of Omega over the triangles in ascending index, left to right) / (4 pi).  One lane
 * owns one sample and walks every triangle itself: no atomics, two calls agree bit for bit.  winding (n samples floats) and
 * inside (n samples bytes: |w| > 0.5) may each be NULL.  Launched on the handle's stream, outside the captured substep; the scene
 * is neither read nor changed.  PIES_ERR_INVALID: a NULL array, no vertices or triangles, a triangle index >= n_vertices, a
 * non-finite vertex or origin, cell not finite or <= 0, a zero in dims.  PIES_ERR_UNSUPPORTED: more than 2^26 samples or more
 * than 2^24 triangles.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first). */
int pies_voxelize_tri_mesh(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles,
                           const uint32_t* tri_ids, const float origin[3], float cell, const uint32_t dims[3],
                           float* winding, uint8_t* inside);
/* Solver::addTriMeshVolume (PrimitiveUtilities.cpp:164-328) without tetgen: a closed triangle mesh becomes a LATTICE body - the
 * cells of a uniform lattice that lie inside the surface, six tetrahedra each - with a staircase collision surface, and the input
 * mesh rides on it as a skin (pies_add_skin).  It is not tetgen's conforming mesh: the input vertices are not nodes.  The rules,
 * all in fp32:
 *  lattice   lo, hi = bounds of the vertices, extent = hi - lo; cell = (largest extent) / resolution;
 *            n_a = max(1, ceil(extent_a / cell)) cells per axis; origin_a = lo_a - 0.5 (n_a cell - extent_a).
 *  cells     cell (i, j, k), index (i ny + j) nz + k, is kept when |w(centre)| > 0.5 (pies_voxelize_tri_mesh on this lattice:
 *            the winding direction of the input does not matter) OR when it contains an input vertex, the cell of vertex v being
 *            floor((v_a - origin_a) / cell) clamped to [0, n_a - 1] per axis - so every input vertex lies in an element and a
 *            feature thinner than a cell becomes cells, not a binding failure.
 *  nodes     the lattice points origin + (i, j, k) cell that are a corner of a kept cell, numbered in ascending (i, j, k), k
 *            fastest; velocity = the argument, invMass = 1 / density (the reference's "mass = density", :176),
 *            radius = min(0.5, 0.95 * 0.5 * cell) (the reference's 0.5, :177, would overlap every neighbour on a fine lattice;
 *            pies_create_tet_box uses the second expression).
 *  elements  kept cells in ascending index, each as the six tetrahedra of pies_create_tet_box in its node order and its order of
 *            the six; one strain (strain_stiffness, min_strain, max_strain) and one volume (volume_stiffness, compression,
 *            stretching) constraint per element, each kind only when its stiffness is not 0 (:293-315).  No colour hints: the
 *            schedulers colour the body like any unstructured mesh.
 *  triangles every element face that belongs to exactly one element, wound so that its normal points away from the element's
 *            fourth vertex (outward), in the order: elements ascending, faces opposite vertex 0, 1, 2, 3.
 *  skin      the input vertices and triangles, bound to the new elements by pies_add_skin's rule with
 *            max_distance = 8 FLT_EPSILON max(cell, largest |coordinate| of the lattice's corners); skin_id receives its id.
 * first_node, n_nodes, n_tets, skin_id may each be NULL.  PIES_ERR_INVALID: a NULL array, resolution == 0, no vertices or
 * triangles, a non-finite vertex, a triangle index >= n_vertices, a largest extent of 0, density <= 0, no kept cell.
 * PIES_ERR_UNSUPPORTED: the limits of pies_voxelize_tri_mesh.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are
 * checked first).  All or nothing: on any failure the scene holds exactly the nodes, constraints, triangles and skins it held
 * before.  pies_clear drops the body and its skin like any other scene content. */
int pies_add_tri_mesh_volume(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles,
                             const uint32_t* tri_ids, const float velocity[3], float density, float strain_stiffness,
                             float min_strain, float max_strain, float volume_stiffness, float compression, float stretching,
                             uint32_t resolution, uint32_t* first_node, uint32_t* n_nodes, uint32_t* n_tets, uint32_t* skin_id);

/* ---- configuration -------------------------------------------------------------------------- */
int pies_set_flag(pies_solver_t* s, int flag, int value);
/* Solver::tickPBD / Solver::tickPD (Solver.h:62-63) run the named solver whatever SolverOptions::solver says: this switches
 * which loop pies_tick runs (PIES_SOLVER_PBD / PIES_SOLVER_PD).  The device buffers of the other loop are built at the next tick
 * (a full pies_finalize), so alternating every tick is correct but slow.  Node state carries over. */
int pies_set_solver(pies_solver_t* s, int solver);
int pies_set_schedule(pies_solver_t* s, int schedule);
/* PD global step: the reference solves (K + C) x = rhs with a sparse Cholesky factorisation rebuilt every
 * substep (Solver.cpp:258-262,356); here it is a Jacobi-preconditioned CG.  rel_tol bounds ||r||/||rhs|| per
 * coordinate column, max_iters the upper bound of CG iterations per solve (defaults 3e-7, 128; the captured graph
 * holds as many as the recent solves needed plus one or two). */
int pies_set_pcg(pies_solver_t* s, float rel_tol, uint32_t max_iters);
/* Over the last pies_tick, or over the pies_tick_async calls since the last synchronisation: largest ||r||/||rhs|| left by
 * any solve, most CG iterations any solve used, solves run. */
int pies_get_pcg_stats(pies_solver_t* s, float* max_rel_residual, uint32_t* max_iters_used, uint32_t* solves);
/* The reference's global step is exact (Solver.cpp:356).  pies_tick therefore does not keep a substep in which a solve
 * ended above rel_tol: the substep's input is restored and it runs again with four times the captured CG budget, up to
 * max_iters (default on; 0 switches the re-run off).  pies_tick_async cannot look at a substep before the next one is
 * queued; both paths count what was left above the tolerance:
 *   short_solves      solves of kept substeps that ended above rel_tol since pies_finalize (0 = every solve met it),
 *   solves_total      solves of kept substeps,
 *   substeps_retried  substeps pies_tick ran again,
 *   budget            CG iterations per solve in the captured graph right now. */
int pies_set_pcg_retry(pies_solver_t* s, int enabled);
int pies_get_pcg_health(pies_solver_t* s, uint64_t* short_solves, uint64_t* solves_total, uint32_t* substeps_retried, uint32_t* budget);
/* Builds schedules, uploads to HBM and captures the substep graph.  Called implicitly by pies_tick
 * when the scene changed. */
int pies_finalize(pies_solver_t* s);

/* ---- the hot path --------------------------------------------------------------------------- */
/* Solver::tick (Solver.cpp:25-38): timeSubsteps substeps of tickPBD / tickPD, then positions are copied
 * back so that pies_read_nodes / Solver::getVertices are current (Solver.cpp:157,393).  No-op once failed. */
int pies_tick(pies_solver_t* s);
/* Same work, but neither the host copy-back nor a stream synchronisation: state stays in HBM.  (Projective Dynamics: the
 * captured CG budget can only follow the solves at a host synchronisation, so every 16th call without one in between
 * synchronises first.) */
int pies_tick_async(pies_solver_t* s);
/* Waits for the queued ticks, then latches a device-side failure (pies_failed) and adapts the CG budget. */
int pies_synchronize(pies_solver_t* s);
/* Render-state export without a stall (Solver::getVertices, Solver.h:42-71; Solver.cpp:157,393 write _vertices every
 * substep): pies_tick_begin queues one tick plus the copy of its final positions into one of two pinned host buffers
 * (a copy stream moves frame k while the compute stream already runs frame k+1) and returns at once with the frame's
 * id (1, 2, ...).  pies_export_acquire blocks until that frame's copy has landed and returns n x 4 floats
 * (x, y, z, invMass); the pointer stays valid until pies_export_release or until two more frames have begun.  A
 * third pies_tick_begin while the oldest frame is still acquired fails with PIES_ERR_STATE. */
int pies_tick_begin(pies_solver_t* s, uint64_t* frame);
int pies_export_acquire(pies_solver_t* s, uint64_t frame, const float** pos4, uint32_t* n);
int pies_export_release(pies_solver_t* s, uint64_t frame);
/* Skins (pies_add_skin).  Vertex i of a skin is x_i = p0 + w1 (p1 - p0) + w2 (p2 - p0) + w3 (p3 - p0), summed left to right in
 * fp32 without fused multiply-adds; its normal is normalize(sum over the triangles that name i, in ascending triangle index, of
 * cross(x_b - x_a, x_c - x_a)) = sum / sqrt(|sum|^2), and (0, 0, 0) when |sum|^2 is 0 or not finite (a vertex no triangle names,
 * a skin without triangles).  Nothing is summed with atomics: two runs agree bit for bit.  The two kernels are launched outside
 * the captured substep; a scene without skins launches, allocates and copies nothing for them.
 * pies_read_skin evaluates skin `skin` from the device's current node positions on the solver's stream, synchronises and copies
 * out (positions: n x 3; normals: n x 3, may be NULL; n must be the skin's vertex count).
 * pies_export_acquire_skin: pies_tick_begin evaluates every skin behind the frame's position copy and the frame's copy stream
 * carries the result into per-frame pinned buffers; this waits for frame `frame` like pies_export_acquire and returns pointers
 * into them (n x 3 each; normals may be NULL), valid exactly as long as that frame's pos4 pointer.  A skin added after the frame
 * was begun is not part of it (PIES_ERR_STATE). */
int pies_read_skin(pies_solver_t* s, uint32_t skin, float* positions, float* normals, uint32_t n);
int pies_export_acquire_skin(pies_solver_t* s, uint64_t frame, uint32_t skin, const float** positions, const float** normals, uint32_t* n);
/* EXTENSION (the reference draws nodes and has no ray query; its element grid _spatialHashTets was never finished): n_rays rays
 * against the surface as the device holds it now - picking, grabbing, line-of-sight probes without a read-back.  origins and
 * directions: n_rays x 3 floats each; directions are not normalised, t is measured in units of |d|.  The outputs may each be NULL:
 * hit_triangle (n_rays), hit_t (n_rays), hit_uv (n_rays x 2: the weights of corners b and c at the hit).
 * Targets.  PIES_RAY_SCENE_TRIANGLES: the PIES_TRIANGLES container, indexed in the order the host added the triangles, at the node
 * positions the device holds (PBD and PD; under PIES_FLAG_RENUMBER_NODES the indices stay the host's).  PIES_RAY_SKIN: the
 * triangles of skin `skin` (index local to that skin) at its current deformed vertices, evaluated on the same stream first; `skin`
 * is ignored for the other target.
 * The rule for one (ray, triangle) pair, ray (o, d), corners a, b, c, in fp32 without fused multiply-adds, every dot product
 * summed left to right as x x + y y + z z, cross(p, q) = (p.y q.z - p.z q.y, p.z q.x - p.x q.z, p.x q.y - p.y q.x):
 *   e1 = b - a, e2 = c - a, p = cross(d, e2), det = e1 . p;    miss unless |det| >= FLT_MIN (PIES_RAY_CULL_BACK: det >= FLT_MIN);
 *   inv = 1 / det;                                             miss unless inv is finite;
 *   s = o - a, u = (s . p) inv;                                miss unless u >= 0 && u <= 1;
 *   q = cross(s, e1), v = (d . q) inv;                         miss unless v >= 0 && u + v <= 1;
 *   t = (e2 . q) inv + 0.0f (a -0 becomes +0);                 miss unless t >= 0 && t <= t_max.
 * Every test is the positive form written, so a NaN anywhere is a miss.  The hit of a ray is the pair with the smallest t, the
 * lowest triangle index on equal t; without one hit_triangle = PIES_RAY_MISS, hit_t = +inf, hit_uv = (0, 0).  The winner is a
 * minimum of 64-bit keys (bits of t, triangle) without atomics: every kernel variant and every split of the triangles gives the
 * same bits, and two calls agree bit for bit.
 * Runs on the handle's stream behind whatever ticks are queued and synchronises before it returns; node state, export frames,
 * captured graphs and pies_launch_counts are left as they were; its buffers are allocated at the first call and freed by the
 * next pies_finalize, pies_clear or pies_destroy.  Brute force over all triangles.
 * PIES_ERR_INVALID: a NULL input array with n_rays > 0, an unknown target, a skin id out of range, a negative or NaN t_max (+inf
 * is allowed).  PIES_ERR_UNSUPPORTED: more than 2^26 rays.  n_rays == 0 returns PIES_OK.  PIES_ERR_HIP: a PIES_DEVICE_NONE
 * handle (the arguments are checked first).  A target without triangles gives all misses. */
enum { PIES_RAY_SCENE_TRIANGLES = 0, PIES_RAY_SKIN = 1 };
enum { PIES_RAY_CULL_BACK = 1 }; /* flags */
#define PIES_RAY_MISS 0xFFFFFFFFu
int pies_raycast(pies_solver_t* s, int target, uint32_t skin, uint32_t n_rays, const float* origins, const float* directions,
                 float t_max, uint32_t flags, uint32_t* hit_triangle, float* hit_t, float* hit_uv);
/* EXTENSION (the reference has no distance query): for n_points points the closest point of the surface as the device holds it
 * now, and optionally the winding number of the surface there - penetration depth and direction of a prop the host moves, anchors
 * that follow a (triangle, u, v), proximity probes, "is this point inside the body", all without a read-back.  points: n_points x 3
 * floats.  target and skin mean what they mean for pies_raycast (PIES_RAY_SCENE_TRIANGLES: the PIES_TRIANGLES container in the
 * host's order, also under PIES_FLAG_RENUMBER_NODES; PIES_RAY_SKIN: the triangles of skin `skin`, index local to that skin, its
 * vertices evaluated on the same stream first).  The outputs may each be NULL: out_triangle (n_points), out_distance (n_points),
 * out_uv (n_points x 2: the weights of corners b and c at the closest point), out_point (n_points x 3), out_winding (n_points).
 * The rule for one (point p, triangle a b c) pair, in fp32 without fused multiply-adds, every dot product summed left to right as
 * x x + y y + z z (the region walk of Ericson's closest point on a triangle; e11, e12, e22 are computed once per triangle):
 *   e1 = b - a, e2 = c - a;  e11 = e1.e1, e12 = e1.e2, e22 = e2.e2;
 *   ap = p - a;  d1 = e1.ap, d2 = e2.ap;  d3 = d1 - e11, d4 = d2 - e12, d5 = d1 - e12, d6 = d2 - e22;
 *   vc = d1 d4 - d3 d2;  vb = d5 d2 - d1 d6;  va = d3 d6 - d5 d4;
 *   the first that holds:  d1 <= 0 && d2 <= 0                        (u, v) = (0, 0)
 *                          d3 >= 0 && d4 <= d3                       (1, 0)
 *                          vc <= 0 && d1 >= 0 && d3 <= 0             (d1 / (d1 - d3), 0)
 *                          d6 >= 0 && d5 <= d6                       (0, 1)
 *                          vb <= 0 && d2 >= 0 && d6 <= 0             (0, d2 / (d2 - d6))
 *                          va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); (1 - w, w)
 *                          otherwise                                 inv = 1 / ((va + vb) + vc); (vb inv, vc inv)
 *   q = (a + e1 u) + e2 v;  r = p - q;  dd = r.r;
 *   a candidate iff dd <= FLT_MAX && dd <= max_distance * max_distance (the product rounded to fp32).
 * Every test is the positive form written, so a NaN anywhere is no candidate.  The answer for a point is the candidate with the
 * smallest dd, the lowest triangle index on equal dd (the normal case for a point nearest to a shared edge or corner): the minimum
 * of the 64-bit key float_as_uint(dd) << 32 | triangle - dd is a sum of squares, +0 or larger, so the bit patterns order like the
 * values - taken without atomics, so every kernel variant and every split of the triangles gives the same bits and two calls agree
 * bit for bit.  out_triangle = that triangle, out_distance = sqrtf(dd), out_uv = (u, v), out_point = q, all from the winning pair
 * evaluated once more; without a candidate PIES_NEAR_NONE, +inf, (0, 0) and p itself.
 * out_winding: the generalised winding number of the target's triangle set at the point, the solid angle of a pair exactly as
 * pies_voxelize_tri_mesh states it, summed in a fixed two-level order: per tile of 256 consecutive triangles in ascending index
 * from 0.0f, then the tile sums in ascending tile index from 0.0f, then divided by 4 pi (12.566370614359172f).  The order is a
 * function of the triangle count alone - not of the point count, the kernel variant or a chunking -, so two calls agree bit for
 * bit.  "Inside" is |w| > 0.5 and means something for closed surfaces: on a scene with several closed bodies it is "inside any
 * of them"; open sheets contribute fractions, and a target that is not closed has no inside.
 * Runs on the handle's stream behind whatever ticks are queued and synchronises before it returns; node state, export frames,
 * captured graphs and pies_launch_counts are left as they were; its buffers are allocated at the first call and freed by the
 * next pies_finalize, pies_clear or pies_destroy.  Brute force over all triangles.
 * PIES_ERR_INVALID: NULL points with n_points > 0, an unknown target, a skin id out of range, a negative or NaN max_distance (+inf
 * is allowed; 0 finds only dd == 0).  PIES_ERR_UNSUPPORTED: more than 2^26 points.  n_points == 0 returns PIES_OK.  PIES_ERR_HIP:
 * a PIES_DEVICE_NONE handle (the arguments are checked first).  A target without triangles gives no candidate and winding 0. */
#define PIES_NEAR_NONE 0xFFFFFFFFu
int pies_closest_points(pies_solver_t* s, int target, uint32_t skin, uint32_t n_points, const float* points, float max_distance,
                        uint32_t* out_triangle, float* out_distance, float* out_uv, float* out_point, float* out_winding);
/* EXTENSION (the reference's only obstacle is the floor, Src/Solver.cpp): kinematic props - spheres, capsules and rounded oriented
 * boxes the host moves.  The nodes are pushed out of them where HBM holds them, the velocity response is relative to the moving
 * prop, and the reaction impulse and torque per prop come back so that the host can drive a rigid body of its own: the first
 * device-side edit of node state (the other one, pies_write_nodes, downloads, overwrites a whole host array and uploads four).
 * props: n_props records, applied in ascending index.  The outputs may each be NULL: out_impulse, out_torque (n_props x 3),
 * out_hits (n_props), out_node_prop (pies_count(PIES_NODES) entries in host numbering: the index of the last prop that touched the
 * node, or PIES_PROP_NONE).
 * The rule, in fp32 without fused multiply-adds.  Dot products are summed left to right as x x + y y + z z, cross is pies_raycast's,
 * a vector times (or divided by) a scalar is taken componentwise, a + b * t is the product rounded, then the sum.  fmaxf and fminf
 * return the other operand when one is a NaN.  Every test is the positive form written, so a NaN anywhere is "not touched".
 * A node has position p (invMass in .w), velocity v and radius r.  A node with invMass == 0 is never touched.  Otherwise the props
 * are applied in ascending index, each to the state the previous one left.  R = prop.radius + r: the node's own radius counts, as
 * it does for the floor.
 *   The sphere rule, centre c:  d = p - c, dd = d.d;  touched iff dd < R * R (the product rounded);
 *                               n = d / sqrtf(dd) if dd > 0, else (0, 1, 0);  q = c + n * R.
 *   PIES_PROP_SPHERE   the sphere rule with c = centre.
 *   PIES_PROP_CAPSULE  a = centre, b = end;  ab = b - a, ap = p - a, den = ab.ab;
 *                      t = den > 0 ? fminf(fmaxf((ap.ab) / den, 0), 1) : 0;  the sphere rule with c = a + ab * t.
 *   PIES_PROP_BOX      l_j = axis_j . (p - centre);  inside iff fabsf(l_j) <= half_j for j = 0, 1, 2.
 *                      inside:   e_j = half_j - fabsf(l_j), j* the smallest e_j (the lowest j on a tie);
 *                                n = axis_j* if l_j* >= 0, else -axis_j*;  q = p + n * (e_j* + R);  always touched.
 *                      outside:  k_j = fminf(fmaxf(l_j, -half_j), half_j);
 *                                the sphere rule with c = ((centre + axis_0 * k_0) + axis_1 * k_1) + axis_2 * k_2.
 *   A touch:  p = q, and the previous position becomes q as well - PD's velocity update reads position - prevPosition
 *             (Src/Solver.cpp:389-392), so the push does not turn into velocity there; PBD overwrites the previous position (:48).
 *             u = velocity + cross(angular, q - pivot);  rel = v - u, vn = rel.n;  tang = rel - n * vn;
 *             v' = u + (tang * (1 - friction) + n * fmaxf(vn, 0));
 *             the touch's impulse j = (v - v') * (1 / invMass), its torque cross(q - pivot, j);  then v = v'.
 *             The position correction itself carries no impulse: j is the change of momentum of the velocity response alone.
 * out_hits[k] counts the nodes prop k touched.  out_impulse[k] and out_torque[k] are the touches' j and torque summed in a fixed
 * two-level order: per tile of 256 consecutive HOST node ids in ascending id from 0.0f (an untouched node adds 0), then the tile
 * sums in ascending tile index from 0.0f.  The order is a function of the node count alone - not of a kernel variant, not of
 * PIES_FLAG_RENUMBER_NODES - and nothing is summed with atomics, so two calls agree bit for bit.  The host applies -impulse and
 * -torque (about pivot) to its own body.
 * Runs on the handle's stream behind whatever ticks are queued, finalizes a changed scene first and synchronises before it
 * returns; export frames begun earlier, captured graphs and pies_launch_counts are left as they were.  The edit is in HBM only:
 * the host mirror is marked stale for positions, previous positions and velocities, so pies_read_nodes, pies_tick and a scene edit
 * see it; nothing is uploaded.  Its buffers are allocated at the first call and freed by the next pies_finalize, pies_clear or
 * pies_destroy.
 * PIES_ERR_INVALID: NULL props with n_props > 0, an unknown shape, a negative or non-finite radius or half extent, friction
 * outside [0, 1], a non-finite field the shape uses (velocity, angular and pivot always; centre; a capsule's end; a box's axes and
 * half extents).  PIES_ERR_UNSUPPORTED: n_props > PIES_PROP_MAX.  n_props == 0 returns PIES_OK and touches nothing (out_node_prop
 * is all PIES_PROP_NONE).  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first). */
enum { PIES_PROP_SPHERE = 0, PIES_PROP_CAPSULE = 1, PIES_PROP_BOX = 2 };
#define PIES_PROP_NONE 0xFFFFFFFFu
#define PIES_PROP_MAX 64
typedef struct pies_prop {
  int32_t shape;
  float radius;      /* sphere, capsule: radius; box: rounding radius; >= 0 */
  float centre[3];   /* sphere: centre; capsule: end a; box: centre */
  float end[3];      /* capsule: end b; otherwise ignored */
  float axes[9];     /* box: axis j = axes[3 j .. 3 j + 2], unit and orthogonal (the host's duty); otherwise ignored */
  float half[3];     /* box: half extents >= 0 */
  float velocity[3]; /* velocity of the pivot */
  float angular[3];  /* angular velocity about the pivot */
  float pivot[3];    /* point the angular velocity and the returned torque refer to */
  float friction;    /* 0 .. 1: share of the tangential relative velocity a touch removes */
} pies_prop_t;
int pies_collide_props(pies_solver_t* s, uint32_t n_props, const pies_prop_t* props, float* out_impulse, float* out_torque,
                       uint32_t* out_hits, uint32_t* out_node_prop);
/* EXTENSION: signed distance FIELDS and FIELD PROPS - rigid colliders of any shape.  A field is a signed distance function sampled
 * on a regular lattice in a local frame: negative inside, positive outside.  It is either built once on the device from a closed
 * triangle mesh (pies_add_field_tri_mesh) or supplied by the host (pies_add_field: an analytic shape, a height field).  A field
 * prop is a rigid placement of a field that the host moves every frame; pies_collide_field_props pushes the nodes out of it and
 * returns impulse and torque exactly as pies_collide_props does for the primitive shapes.
 * The lattice: sample (i, j, k) of the dims lattice sits at local origin + (float)index * cell per axis (the product rounded, then
 * the sum) and is stored at (k * dims[1] + j) * dims[0] + i.  Every dim is at least 2; a lattice has at most 2^24 samples.
 * pies_add_field takes the host's samples as they are (a NaN sample is allowed: a node in a cell with one is not touched) and
 * works on PIES_DEVICE_NONE handles too - only colliding needs the device.  PIES_ERR_INVALID: a NULL argument, a dim below 2, a
 * non-finite origin, cell not finite or <= 0.  PIES_ERR_UNSUPPORTED: more than 2^24 samples, more than PIES_FIELD_MAX fields.
 * pies_add_field_tri_mesh builds the samples on the device, everything in fp32:
 *   lo, hi = the exact minimum and maximum of the vertices;  origin_j = lo_j - margin;
 *   dims_j = max(2, (uint32_t)ceilf(((hi_j + margin) - origin_j) / cell) + 1);
 *   dd = the smallest dd of the pair rule of pies_closest_points over the mesh's triangles at the sample's position (its rule, its
 *        key and its tie-breaking, max_distance = +inf), w = the winding number there in pies_closest_points' two-level order (tiles
 *        of 256 triangles);  sample = -sqrtf(dd) if |w| > 0.5, else sqrtf(dd).
 * The launches are pies_closest_points' own, so the bits are its bits and two builds agree bit for bit.  The build is BRUTE FORCE
 * over samples x triangles, once per field (DESIGN.md section 8f has timings); the mesh should be closed.  The scene is neither
 * read nor changed.  A push ends where the lattice ends: give the build a margin of at least the largest prop radius + the
 * largest node radius + cell.  PIES_ERR_INVALID: a NULL array, no vertices or triangles, a non-finite vertex, an index out of
 * range, cell not finite or <= 0, margin negative or not finite.  PIES_ERR_UNSUPPORTED: more than 2^24 samples or 2^24 triangles,
 * more than PIES_FIELD_MAX fields.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first).
 * pies_get_field returns dims, origin, cell and - when samples is given - the samples (capacity in floats; too small:
 * PIES_ERR_INVALID); every output may be NULL.  The library keeps a host copy of every field, so this needs no device.
 * Lifetime: `field` (may be NULL) receives 0, 1, ...  Fields are assets, not scene state: they survive pies_finalize, scene edits
 * and ticks (a device copy dropped by pies_finalize is staged again from the host copy at the next use) and end with pies_clear or
 * pies_destroy; after pies_clear the ids are invalid and count from 0 again.
 * The rule for one (node, field prop) pair, in fp32 without fused multiply-adds, with pies_collide_props' conventions: dot products
 * summed left to right, a + b * t the product rounded then the sum, every test the positive form written (a NaN anywhere is "not
 * touched"), a node with invMass == 0 never touched, the props applied in ascending index, each to the state the previous one
 * left.  R = prop.radius + r.  sample(i, j, k) is the prop's field.
 *   d = p - centre;  l_j = axis_j . d;  g_j = (l_j - origin_j) / cell;
 *   in the lattice iff g_j >= 0 && g_j < (float)(dims_j - 1) for j = 0, 1, 2;  otherwise not touched;
 *   i_j = (uint32_t)g_j;  f_j = g_j - (float)i_j;  s_abc = sample(i_0 + a, i_1 + b, i_2 + c);
 *   m_bc = s_0bc + (s_1bc - s_0bc) * f_0;  m_c = m_0c + (m_1c - m_0c) * f_1;  phi = m_0 + (m_1 - m_0) * f_2;
 *   touched iff phi < R;
 *   G_0: the four differences s_1bc - s_0bc, interpolated over b by f_1, then over c by f_2 (the same x + (y - x) * f form);
 *   G_1: s_a1c - s_a0c over a by f_0, then over c by f_2;  G_2: s_ab1 - s_ab0 over a by f_0, then over b by f_1;
 *   GG = G.G;  nl = G / sqrtf(GG) if GG > 0, else (0, 1, 0);
 *   n = (axis_0 * nl_0 + axis_1 * nl_1) + axis_2 * nl_2;  q = p + n * (R - phi).
 * A touch is word for word pies_collide_props' touch (p = q, the previous position = q, then u, rel, vn, tang, v', the impulse j
 * and its torque about pivot).  The push is ONE STEP along the gradient of the trilinear interpolant, not an exact projection: for a
 * true distance field it lands on the R level set to first order (DESIGN.md section 8f has the measured error).  The outputs and
 * their fixed two-level order of summation (tiles of 256 consecutive HOST node ids from 0.0f, then the tiles in ascending index,
 * also under PIES_FLAG_RENUMBER_NODES; no atomics) are pies_collide_props'; so is everything else: the call runs on the handle's
 * stream behind queued ticks, finalizes a changed scene first, synchronises before it returns, marks the host mirror stale and
 * uploads no node state; captured graphs and pies_launch_counts are left as they were.
 * PIES_ERR_INVALID: NULL props with n_props > 0, an unknown field id, a negative or non-finite radius, friction outside [0, 1], any
 * non-finite member of the record.  PIES_ERR_UNSUPPORTED: n_props > PIES_FIELD_PROP_MAX.  n_props == 0 returns PIES_OK and touches
 * nothing (out_node_prop is all PIES_PROP_NONE).  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first). */
#define PIES_FIELD_MAX 64      /* fields per handle */
#define PIES_FIELD_PROP_MAX 64 /* field props per call (one 64-bit word per tile, as for props) */
int pies_add_field(pies_solver_t* s, const uint32_t dims[3], const float origin[3], float cell, const float* samples, uint32_t* field);
int pies_add_field_tri_mesh(pies_solver_t* s, uint32_t n_vertices, const float* positions, uint32_t n_triangles,
                            const uint32_t* tri_ids, float cell, float margin, uint32_t* field);
int pies_get_field(pies_solver_t* s, uint32_t field, uint32_t dims[3], float origin[3], float* cell, float* samples, uint64_t capacity);
typedef struct pies_field_prop {
  uint32_t field;    /* id of pies_add_field / pies_add_field_tri_mesh */
  float radius;      /* inflation of the zero level set, >= 0 */
  float centre[3];   /* world position of the field's local (0, 0, 0) */
  float axes[9];     /* local frame: axis j = axes[3 j .. 3 j + 2], unit and orthogonal (the host's duty) */
  float velocity[3]; /* velocity of the pivot */
  float angular[3];  /* angular velocity about the pivot */
  float pivot[3];    /* point the angular velocity and the returned torque refer to */
  float friction;    /* 0 .. 1: share of the tangential relative velocity a touch removes */
} pies_field_prop_t;
int pies_collide_field_props(pies_solver_t* s, uint32_t n_props, const pies_field_prop_t* props, float* out_impulse,
                             float* out_torque, uint32_t* out_hits, uint32_t* out_node_prop);
/* EXTENSION (the reference's only external acceleration is options.gravity): FORCE FIELDS - wind on the scene's triangles, blasts
 * and attractors, vortices, a braking medium, a plain push - applied to the velocities where HBM holds them: the second
 * device-side edit of node state after pies_collide_props.  forces: n_forces records.  dt: the time the forces act for, in
 * seconds (the host's choice: a frame, a substep).  The outputs may each be NULL: out_impulse, out_torque (n_forces x 3),
 * out_nodes (n_forces).
 * The rule, in fp32 without fused multiply-adds, with pies_collide_props' conventions: dot products summed left to right as
 * x x + y y + z z, cross is pies_raycast's, a vector times (or divided by) a scalar is taken componentwise, fminf returns the
 * other operand when one is a NaN, every test is the positive form written, so a NaN anywhere is "not affected".  Only + - * /
 * sqrtf, fminf and comparisons occur.
 * THE STATE READ IS THE STATE THE CALL FOUND: every force, whatever its index, reads the positions p and the velocities v the
 * call found (the wind reads the velocities of a triangle's three corners).  Positions and previous positions are never written.
 * A node with invMass w == 0 is never moved and never counted.  Per node i and force k the rule yields a velocity change
 * dv_k(i), or "not affected".  A node affected by at least one force ends with v' = v + ((dv_k0 + dv_k1) + ...): the changes of
 * the forces that affect it, added per component in ascending k to a sum that starts at 0.0f, and that sum added to v.  A node
 * no force affects is not written.
 *   The region of force k at a point x:  d = x - centre, dd = d.d;  inside iff dd < radius * radius (the product rounded;
 *     radius = +inf: everywhere dd is finite);  fall = 1                                        PIES_FALLOFF_NONE
 *                                                      1 - sqrtf(dd) / radius                   PIES_FALLOFF_LINEAR
 *                                                      u * u with u = 1 - dd / (radius * radius) PIES_FALLOFF_SMOOTH
 *   The point forces take the region at x = p; outside it the node is not affected.  g = fall * dt.
 *   PIES_FORCE_DIRECTIONAL  a = vector.
 *   PIES_FORCE_RADIAL       not affected unless dd > 0;  a = (d / sqrtf(dd)) * strength: a blast when strength > 0, an attractor
 *                           when strength < 0.
 *   PIES_FORCE_VORTEX       a = cross(vector, d) * strength: vector is the axis through centre, not normalised.
 *   for these three:        a is an acceleration; with PIES_FORCE_IS_FORCE in flags it is a force, a = a * w.  dv = a * g.
 *   PIES_FORCE_DRAG         a medium that moves with vector:  k = fminf(strength * dt, 1);  dv = (vector - v) * (k * fall).
 *                           Independent of the mass; the cap keeps the explicit step from overshooting.
 *   PIES_FORCE_WIND         acts on the triangles of the PIES_TRIANGLES container, both sides alike.  For triangle t with corners
 *                           a, b, c (positions) and va, vb, vc (velocities):
 *                             N = cross(b - a, c - a), nn = N.N;  no contribution unless nn > 0;
 *                             len = sqrtf(nn), n = N / len, area = 0.5f * len;
 *                             the region at x = ((a + b) + c) / 3.0f;  no contribution outside it;
 *                             rel = vector - ((va + vb) + vc) / 3.0f;  vn = rel.n;
 *                             F = (n * (strength * vn) + (rel - n * vn) * shear) * (area * fall);
 *                           and every corner with w != 0 receives (F / 3.0f) * (dt * w) with its own w.  dv_k(i) is the sum of
 *                           what node i receives over the (triangle, corner) entries that name it, in ascending triangle index
 *                           from 0.0f; the node is affected by k iff at least one of them contributed.  strength: pressure
 *                           per unit of normal relative speed and area; shear: the same for the tangential part.
 * out_nodes[k] counts the nodes force k affected.  out_impulse[k] is the sum of j = dv_k(i) * (1 / w_i), out_torque[k] the sum
 * of cross(p_i - centre_k, j), both in pies_collide_props' fixed two-level order: per tile of 256 consecutive HOST node ids in
 * ascending id from 0.0f (a node not affected adds 0), then the tile sums in ascending tile index from 0.0f.  The order is a
 * function of the node count alone - not of a kernel variant, not of PIES_FLAG_RENUMBER_NODES - and nothing is summed with
 * atomics, so two calls agree bit for bit.  With all three outputs NULL nothing is summed and the second launch is not paid.
 * Runs on the handle's stream behind whatever ticks and begun frames are queued, finalizes a changed scene first and
 * synchronises once before it returns; export frames begun earlier, captured graphs and pies_launch_counts are left as they were.
 * The edit is in HBM only: the host mirror is marked stale for the velocities alone, nothing is uploaded.  Its buffers (and the
 * node -> triangle incidence of the wind, built at the first call with a wind after a pies_finalize) are freed by the next
 * pies_finalize, pies_clear or pies_destroy.
 * PIES_ERR_INVALID: NULL forces with n_forces > 0, an unknown type or falloff, a non-finite member of a record other than
 * radius = +inf, a negative or NaN radius, a negative or non-finite dt.  PIES_ERR_UNSUPPORTED: n_forces > PIES_FORCE_MAX.
 * n_forces == 0 returns PIES_OK and does nothing.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first).  A
 * scene without nodes synchronises and returns zeros; a wind in a scene without triangles affects nothing. */
enum { PIES_FORCE_DIRECTIONAL = 0, PIES_FORCE_RADIAL = 1, PIES_FORCE_VORTEX = 2, PIES_FORCE_DRAG = 3, PIES_FORCE_WIND = 4 };
enum { PIES_FALLOFF_NONE = 0, PIES_FALLOFF_LINEAR = 1, PIES_FALLOFF_SMOOTH = 2 };
enum { PIES_FORCE_IS_FORCE = 1 }; /* flags */
#define PIES_FORCE_MAX 64
typedef struct pies_force {
  int32_t type;
  uint32_t flags;
  float centre[3];  /* of the region; the point radial forces and vortices refer to, and the returned torque */
  float radius;     /* of the region, >= 0; +inf: everywhere */
  int32_t falloff;
  float vector[3];  /* directional: the acceleration (force); vortex: the axis; drag, wind: the medium's velocity */
  float strength;   /* radial, vortex: the factor; drag: 1 / s; wind: the normal coefficient */
  float shear;      /* wind: the tangential coefficient */
} pies_force_t;
int pies_apply_forces(pies_solver_t* s, uint32_t n_forces, const pies_force_t* forces, float dt, float* out_impulse,
                      float* out_torque, uint32_t* out_nodes);
/* EXTENSION (the reference has no such loads): SURFACE LOADS - a constant pressure, the pressure of an enclosed gas, the hydrostatic
 * pressure and the drag of a fluid - on ranges of the PIES_TRIANGLES container, applied to the velocities where HBM holds them:
 * the third device-side edit of node state after pies_collide_props and pies_apply_forces.  These are the loads that need a
 * triangle's ORIENTATION (the wind of pies_apply_forces is quadratic in the normal and treats both sides alike) or a GLOBAL
 * quantity of a body (the volume its surface encloses).  loads: n_loads records.  dt: the time the loads act for, in seconds.  The
 * outputs may each be NULL: out_impulse, out_torque (n_loads x 3), out_nodes, out_volume, out_area (n_loads).
 * The rule, in fp32 without fused multiply-adds, with pies_apply_forces' conventions: dot products summed left to right as
 * x x + y y + z z, cross is pies_raycast's, a vector times (or divided by) a scalar is taken componentwise, every test is the
 * positive form written, so a NaN anywhere is "not affected".  Only + - * / sqrtf and comparisons occur.
 * THE STATE READ IS THE STATE THE CALL FOUND: every load, whatever its index, reads the positions and the velocities the call
 * found.  Positions and previous positions are never written.  A node with invMass w == 0 is never moved and never counted.
 * A load's range is the triangles [first, first + count) of the container in the order the host added them (count == UINT32_MAX:
 * to the container's end).  A triangle's corners are a, b, c as the container names them - with PIES_LOAD_INWARD (the range's
 * triangles are wound with their normals pointing into the body) a, c, b - and va, vb, vc their velocities.  Per load k:
 *   VOLUME AND AREA of the range, evaluated whatever the type:  o = corner a of triangle `first`;  per triangle
 *     six_t = (a - o) . cross(b - o, c - o);   N = cross(b - a, c - a), nn = N.N, area_t = 0.5f * sqrtf(nn);
 *     V_k = (sum of six_t) / 6.0f,  A_k = sum of area_t;  both sums in a fixed two-level order: per tile of 256 consecutive
 *     container indices of the global tiling (tile u = indices 256 u .. 256 u + 255, restricted to the range) in ascending index
 *     from 0.0f, then the tile sums in ascending tile index from 0.0f.  The shift by o keeps a body far from the world's origin
 *     from cancelling its volume away.  An empty range gives zeros.  V_k > 0 for a closed surface wound outward (after the flag).
 *   THE PRESSURE p on triangle t:
 *     PIES_LOAD_PRESSURE  p = strength.
 *     PIES_LOAD_GAS       an isothermal gas that is at the ambient pressure `strength` when it fills rest_volume: the load acts iff
 *                         V_k > 0.0f, and then p = strength * (rest_volume / V_k - 1.0f) on every triangle of the range.
 *     PIES_LOAD_FLUID     x = ((a + b) + c) / 3.0f, depth = (point - x) . up; the triangle contributes nothing unless
 *                         depth > 0.0f;  p = -(strength * depth).  A triangle the fluid's surface cuts is in or out by its
 *                         centroid: triangles are not clipped.  On a flat triangle a pressure linear in space integrates to its
 *                         value at the centroid times the area, so a closed submerged surface receives strength * V * up in sum:
 *                         Archimedes.
 *   THE TRIANGLE'S FORCE:  no contribution unless nn > 0.0f;  F = N * (0.5f * p);  PIES_LOAD_FLUID with drag != 0.0f on a
 *     contributing triangle adds  rel = velocity - ((va + vb) + vc) / 3.0f,  F = F + rel * (drag * area_t).  Every corner with
 *     w != 0 receives (F / 3.0f) * (dt * w) with its own w.
 *   THE CHANGE FOR A NODE:  dv_k(i) is the sum of what node i receives over the (triangle, corner) entries of the range that name
 *     it, in ascending triangle index from 0.0f; the node is affected by k iff at least one of them contributed.  A node affected
 *     by at least one load ends with v' = v + ((dv_k0 + dv_k1) + ...): the changes of the loads that affect it, added per
 *     component in ascending k to a sum that starts at 0.0f, and that sum added to v.  A node no load affects is not written.
 * out_nodes[k] counts the nodes load k affected.  out_impulse[k] is the sum of j = dv_k(i) * (1 / w_i), out_torque[k] the sum of
 * cross(p_i - point_k, j), both in pies_collide_props' fixed two-level order: per tile of 256 consecutive HOST node ids in
 * ascending id from 0.0f, then the tile sums in ascending tile index from 0.0f.  Nothing is summed with atomics, so two calls
 * agree bit for bit; neither a kernel variant nor PIES_FLAG_RENUMBER_NODES changes a bit.  out_volume[k] = V_k and out_area[k] =
 * A_k, also for a load whose strength is 0: that is how a host learns a surface's volume before it chooses rest_volume.
 * Runs on the handle's stream behind whatever ticks and begun frames are queued, finalizes a changed scene first and
 * synchronises ONCE, before it returns: volume, gas pressure and the edit are chained on the device.  Export frames begun earlier,
 * captured graphs and pies_launch_counts are left as they were.  The edit is in HBM only: the host mirror is marked stale for
 * the velocities alone, nothing is uploaded.  Its buffers (and the node -> triangle incidence, shared with the wind) are freed
 * by the next pies_finalize, pies_clear or pies_destroy.
 * PIES_ERR_INVALID: NULL loads with n_loads > 0, an unknown type or flag bit, a range that leaves the container, a non-finite
 * member, PIES_LOAD_GAS with rest_volume not > 0, drag < 0, a negative or non-finite dt.  PIES_ERR_UNSUPPORTED: n_loads >
 * PIES_LOAD_MAX.  n_loads == 0 returns PIES_OK and does nothing.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are
 * checked first).  A scene without nodes or without triangles synchronises and returns zeros. */
enum { PIES_LOAD_PRESSURE = 0, PIES_LOAD_GAS = 1, PIES_LOAD_FLUID = 2 };
enum { PIES_LOAD_INWARD = 1 }; /* flags: the range's triangles are wound with their normals inward; each is read as (a, c, b) */
#define PIES_LOAD_MAX 64
typedef struct pies_surface_load { /* 16 words, no padding */
  int32_t type;
  uint32_t flags;
  uint32_t first, count; /* triangles [first, first + count) of the PIES_TRIANGLES container; count == UINT32_MAX: to its end */
  float strength;        /* PRESSURE: the pressure p.  GAS: the ambient pressure p0.  FLUID: weight per unit volume (density x gravity) */
  float rest_volume;     /* GAS: the volume at which the inside is at p0 (> 0) */
  float point[3];        /* FLUID: a point of the fluid's surface.  All types: the point the returned torque refers to */
  float up[3];           /* FLUID: the direction out of the fluid, used as given (a unit vector is the host's business) */
  float velocity[3];     /* FLUID: the fluid's velocity */
  float drag;            /* FLUID: drag per unit of relative speed and submerged area, >= 0; 0: none */
} pies_surface_load_t;
int pies_apply_surface_loads(pies_solver_t* s, uint32_t n_loads, const pies_surface_load_t* loads, float dt, float* out_impulse,
                             float* out_torque, uint32_t* out_nodes, float* out_volume, float* out_area);
/* EXTENSION (the reference pins a node to where it stood at creation; goal constraints and fixed regions are PD only): ANCHORS - nodes
 * tied to moving frames by implicit spring-dampers or by pins, applied where HBM holds the nodes, under both solvers: a tyre's rim on a
 * rigid hub, a cloth corner on a joint, a mouse drag.  A device-side edit of node state like pies_collide_props, pies_apply_forces
 * and pies_apply_surface_loads; it hands back what the attachment pulls with, per frame.
 * SETS ARE ASSETS, like fields: pies_add_anchors stores n anchors that refer to n_frames frames and returns the set's id (0, 1, ...
 * per handle); a set survives pies_finalize, scene edits and ticks and ends with pies_clear (ids start from 0 again) or
 * pies_destroy.  The library keeps a host copy of every set - pies_get_anchors reads it and needs no device - and stages the device
 * copy at the first use and again after a pies_finalize dropped it; pies_add_anchors works on PIES_DEVICE_NONE handles.  Node ids
 * are HOST ids of nodes that exist when the set is added; nodes appended later do not disturb a set.  pies_get_anchors: anchors may
 * be NULL (then capacity is not read), else capacity >= the set's count; n and n_frames may each be NULL.
 * pies_apply_anchors applies one set with the frames of this call (n_frames records, the set's count) acting for dt seconds.  The
 * outputs may each be NULL: out_impulse, out_torque (n_frames x 3), out_live (n_frames), out_anchor (n x 4, the set's own order).
 * The rule, in fp32 without fused multiply-adds, with pies_collide_props' conventions: dot products summed left to right as
 * x x + y y + z z, cross is pies_raycast's, a + b * t is the product rounded, then the sum, a vector times a scalar is taken
 * componentwise, every test is the positive form written.  Only + - * / sqrtf and comparisons occur.
 * A node has position p (invMass w in .w) and velocity v: the state the call found.  With h = dt, for anchor i with frame f:
 *   t_i = ((origin + axis_0 * l_0) + axis_1 * l_1) + axis_2 * l_2        l = local
 *   u_i = velocity + cross(angular, t_i - pivot)
 *   x_i = p - t_i;   stretch_i = sqrtf(x_i . x_i)
 * An anchor is LIVE iff w > 0 and strength_f > 0 (the positive form: a NaN is not live).  A node without a live anchor is not
 * written.
 *   SPRINGS.  For a node's live spring anchors, in ascending anchor index:
 *     k_i = stiffness_i * strength_f;  c_i = damping_i * strength_f;  a_i = c_i + k_i * h
 *     g_i = x_i * k_i + (v - u_i) * a_i
 *     A = sum a_i,  G = sum g_i              (from 0.0f, ascending anchor index, componentwise)
 *     hw = h * w;   e = -((G * hw) / (1 + hw * A));   v' = v + e
 *     j_i = (g_i + e * a_i) * (-h)           the impulse anchor i gave the node
 *   This is implicit Euler for a node held by several isotropic spring-dampers at once:
 *   m e = -h sum (k_i (x_i + h (v' - u_i)) + c_i (v' - u_i)).  It is stable for every k dt; as k -> inf it gives p + h v' = t + h u:
 *   the node reaches the moving target in one step.  Positions and previous positions are not written.
 *   A LIVE PIN (PIES_ANCHOR_PIN; a node that carries a pin carries no other anchor of the set).  p = t_i, the previous position
 *     = t_i, v' = u_i, and j_i = (u_i - v) * (1 / w): pies_collide_props' touch - the position correction itself carries no impulse.
 * out_anchor[4 i .. 4 i + 3] = j_i and stretch_i; j is 0 for an anchor that is not live, the stretch is always given (of a pin:
 * before the pin moved the node).  out_impulse[f] sums j_i of frame f's anchors in a fixed two-level order: per tile of 256
 * consecutive anchor indices in ascending index from 0.0f (another frame's anchor adds 0), then the tiles in ascending index from
 * 0.0f.  out_torque[f] sums cross(t_i - pivot_f, j_i) in the same order; out_live[f] counts the live anchors of frame f.  Nothing is
 * summed with atomics and the order is a function of the set alone - not of a kernel variant, not of PIES_FLAG_RENUMBER_NODES -, so
 * two calls agree bit for bit.  The host applies -impulse and -torque (about the frame's pivot) to its own body.  A call is ONE
 * implicit solve per node over the set's anchors: two sets applied one after the other are not one combined set.
 * Runs on the handle's stream behind whatever ticks and begun frames are queued, finalizes a changed scene first and synchronises
 * once before it returns; export frames begun earlier, captured graphs and pies_launch_counts are left as they were.  The edit is in
 * HBM only: the host mirror is marked stale for the velocities, and for positions and previous positions when the set has pins;
 * nothing is uploaded.  With dt == 0 the springs do nothing and the pins still hold.  strength scales k and c of the frame's
 * springs; 0 releases its springs AND its pins.
 * pies_add_anchors: PIES_ERR_INVALID for NULL anchors or n == 0, a node id >= the node count, n_frames == 0 or > PIES_ANCHOR_FRAME_MAX,
 * frame >= n_frames, a non-finite local, stiffness or damping negative or non-finite, an unknown flag, a node that carries a pin
 * and any other anchor of the same set; PIES_ERR_UNSUPPORTED for more than 2^24 anchors or more than PIES_ANCHOR_SET_MAX sets.
 * pies_apply_anchors: PIES_ERR_INVALID for an unknown set, n_frames different from the set's, NULL frames, a non-finite member of a
 * frame, a negative strength, a negative or non-finite dt; PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked
 * first). */
#define PIES_ANCHOR_SET_MAX 64   /* sets per handle */
#define PIES_ANCHOR_FRAME_MAX 64 /* frames per set */
enum { PIES_ANCHOR_PIN = 1 }; /* flags */
typedef struct pies_anchor { /* 32 bytes */
  uint32_t node;   /* host node id */
  uint32_t frame;  /* index into the frames of pies_apply_anchors */
  float local[3];  /* the attachment point in the frame's coordinates */
  float stiffness; /* k >= 0, finite */
  float damping;   /* c >= 0, finite */
  uint32_t flags;  /* 0 or PIES_ANCHOR_PIN */
} pies_anchor_t;
typedef struct pies_anchor_frame { /* 22 words, no padding */
  float origin[3];   /* world position of local (0, 0, 0) */
  float axes[9];     /* axis j = axes[3 j .. 3 j + 2], unit and orthogonal (the host's duty) */
  float velocity[3]; /* velocity of the pivot */
  float angular[3];  /* angular velocity about the pivot */
  float pivot[3];    /* point the angular velocity and the returned torque refer to */
  float strength;    /* >= 0, finite: scales k and c of the frame's springs; 0 releases its springs AND its pins */
} pies_anchor_frame_t;
int pies_add_anchors(pies_solver_t* s, uint32_t n, const pies_anchor_t* anchors, uint32_t n_frames, uint32_t* set);
int pies_get_anchors(const pies_solver_t* s, uint32_t set, pies_anchor_t* anchors, uint32_t capacity, uint32_t* n, uint32_t* n_frames);
int pies_apply_anchors(pies_solver_t* s, uint32_t set, uint32_t n_frames, const pies_anchor_frame_t* frames, float dt,
                       float* out_impulse, float* out_torque, uint32_t* out_live, float* out_anchor);
/* EXTENSION (the reference joins bodies by distance constraints between nodes only): TIES - nodes bound to points on other bodies by
 * implicit spring-dampers, solved where HBM holds the nodes, under both solvers: a cloth sewn to a body, skin glued to flesh, two
 * soft bodies welded at a seam, a tendon ending on a surface, a seam that rips.  Where an anchor lets the host act on a body, a tie
 * lets two parts of the scene act on each other: the carrier feels the pull.  A device-side edit of node state like
 * pies_apply_anchors; it hands back what the seam pulls with, per group.
 * A tie binds node a to the point q = sum weight_j p_bj carried by the nodes b0 b1 b2: a triangle's corners with barycentric
 * weights, an edge (weight[2] == 0), one node (weights 1, 0, 0).  A slot with weight exactly 0 is read but never written.
 * SETS ARE ASSETS exactly as anchor sets are: pies_add_ties stores n ties that refer to n_groups groups and returns the set's id (0,
 * 1, ... per handle); a set survives pies_finalize, scene edits and ticks and ends with pies_clear or pies_destroy.  The library
 * keeps a host copy - pies_get_ties and pies_get_tie_state read it and need no device - and stages the device copy at the first use
 * and again after a pies_finalize dropped it; pies_add_ties works on PIES_DEVICE_NONE handles.  Ids are HOST ids of nodes that exist
 * at the call.  pies_get_ties: ties may be NULL (then capacity is not read), else capacity >= the set's count; n and n_groups may
 * each be NULL.  pies_get_tie_state: broken (one byte per tie, 1: broken) may be NULL, else capacity >= the set's count; n_broken may
 * be NULL.  pies_reset_ties: no tie of the set is broken any more.
 * pies_apply_ties applies one set with the groups of this call (n_groups records, the set's count) acting for dt seconds, in
 * `iterations` Jacobi iterations.  The outputs may each be NULL: out_impulse, out_torque (n_groups x 3), out_live (n_groups),
 * out_tie (n x 4, the set's own order).
 * The rule, in fp32 without fused multiply-adds, with pies_apply_anchors' conventions: dot is x x + y y + z z summed left to right,
 * cross is pies_raycast's, a vector times a scalar is taken componentwise, every test is the positive form written, so a NaN is
 * "not live" and "not broken".  Only + - * / sqrtf and comparisons occur.
 *   COUNTS.  cnt_v is the number of (tie, slot) entries of the SET in which node v takes part: slot a always counts, a `to` slot
 *   counts iff its weight is not 0.  cnt_v is a function of the set alone - not of liveness, not of the call.  An entry's
 *   coefficient c is +1 for slot a and -weight_j for `to` slot j.
 *   PER TIE, ONCE PER CALL.  Tie i has group g, node a and carrier nodes 0 1 2 with weights b0 b1 b2; p is a position with the
 *   invMass w in .w, from the state the call found; h = dt; counts are converted to float.
 *     q = (p0 * b0 + p1 * b1) + p2 * b2;   x = p_a - q;   stretch_i = sqrtf(x . x)
 *     W = w_a * cnt_a + (((b0*b0) * (w0*cnt0) + (b1*b1) * (w1*cnt1)) + (b2*b2) * (w2*cnt2))
 *     k = stiffness * strength_g;  c = damping * strength_g;  a = c + k * h;  den = 1.0f + (h * a) * W
 *   A tie becomes BROKEN iff break_stretch_g > 0 and stretch_i > break_stretch_g; it stays broken until pies_reset_ties.  A tie is
 *   LIVE iff it is not broken (this call's breaks included), strength_g > 0 and W > 0.
 *   ITERATIONS.  J_i starts at 0.  Iteration t = 1 .. iterations:
 *     step 1, every live tie, from the velocities iteration t - 1 left (the first: the state the call found):
 *       uq = (v0 * b0 + v1 * b1) + v2 * b2;   r = v_a - uq
 *       rho = (x * k + r * a) * h + J_i;   dJ_i = -(rho / den);   J_i = J_i + dJ_i
 *     step 2, every node v with a live entry and w_v != 0:  v = v + S * w_v, where S sums dJ_i * c over the node's LIVE entries
 *       from 0.0f in ascending tie index (a node is in a tie's counted slots once).  No other node is written.
 *   Positions and previous positions are never written.
 *   This is Jacobi with mass splitting (Tonge et al. 2012) on the implicit Euler system of zero-length spring-dampers between a and
 *   the carried point: every node's inverse mass is shared out among its cnt_v entries, so the ties of one iteration cannot
 *   overshoot together and velocities stay bounded for every k dt.  With fewer ties than nodes the iteration converges to the
 *   coupled solve (1 + h a C M^-1 C^T) J = -h (k x + a r); very stiff seams take hundreds of iterations.
 *   Equal and opposite impulses through weights that sum to 1 conserve momentum when no tied node is fixed, and angular momentum
 *   where the tied node sits on its carried point (a sewn seam); a stretched tie pulls along k x + a r, not along x, and turns the
 *   pair by cross(x_i, J_i).
 * out_tie[4 i .. 4 i + 3] = J_i and stretch_i; J is 0 for a tie that is not live, the stretch is always given.  out_impulse[g] sums
 * J_i of group g's ties, out_torque[g] sums cross(q_i - pivot_g, J_i) and out_live[g] counts the live ties, in the anchors' fixed
 * two-level order over tie indices: tiles of 256 in ascending index from 0.0f (another group's tie adds 0), then the tiles in
 * ascending index from 0.0f.  J_i is what the seam gave node a; the carrier got -J_i.  The order is a function of the set alone - not
 * of PIES_FLAG_RENUMBER_NODES -, so two calls agree bit for bit.
 * With dt == 0 the iterations do not run: nothing is written, every J is 0, and ties still break and are counted live.
 * Runs on the handle's stream behind whatever ticks and begun frames are queued, finalizes a changed scene first and synchronises
 * once before it returns; export frames begun earlier, captured graphs and pies_launch_counts are left as they were.  The edit is in
 * HBM only: the host mirror is marked stale for the velocities; nothing is uploaded.  When some group has break_stretch > 0 the
 * call reads the broken bytes back into the host copy before it returns, so a later re-staging keeps them.
 * pies_add_ties: PIES_ERR_INVALID for NULL ties or n == 0, an id >= the node count (in any slot), a non-finite weight, all three
 * weights 0, stiffness or damping negative or non-finite, group >= n_groups, n_groups == 0 or > PIES_TIE_GROUP_MAX, a tie whose node
 * and nonzero-weight `to` ids are not pairwise distinct; PIES_ERR_UNSUPPORTED for more than 2^24 ties or more than PIES_TIE_SET_MAX
 * sets.  pies_apply_ties: PIES_ERR_INVALID for an unknown set, n_groups different from the set's, NULL groups, a non-finite or
 * negative member of a group (the pivot: non-finite), a negative or non-finite dt, iterations outside 1 .. 64; PIES_ERR_HIP: a
 * PIES_DEVICE_NONE handle (the arguments are checked first). */
#define PIES_TIE_SET_MAX 64    /* sets per handle */
#define PIES_TIE_GROUP_MAX 64  /* groups per set */
typedef struct pies_tie {      /* 40 bytes */
  uint32_t node;       /* host id of the tied node a */
  uint32_t to[3];      /* host ids b0 b1 b2 of the carrier: a triangle's corners, an edge (weight[2] == 0), one node (1, 0, 0) */
  float weight[3];     /* finite; q = sum weight_j p_bj.  A slot with weight exactly 0 is read but never written */
  float stiffness, damping; /* k, c: finite, >= 0 */
  uint32_t group;      /* < n_groups */
} pies_tie_t;
typedef struct pies_tie_group { /* 5 words */
  float pivot[3];      /* point the returned torque refers to */
  float strength;      /* >= 0, finite: scales k and c; 0 releases the group */
  float break_stretch; /* >= 0, finite; > 0: a tie of the group found longer than this breaks and stays broken */
} pies_tie_group_t;
int pies_add_ties(pies_solver_t* s, uint32_t n, const pies_tie_t* ties, uint32_t n_groups, uint32_t* set);
int pies_get_ties(const pies_solver_t* s, uint32_t set, pies_tie_t* ties, uint32_t capacity, uint32_t* n, uint32_t* n_groups);
int pies_apply_ties(pies_solver_t* s, uint32_t set, uint32_t n_groups, const pies_tie_group_t* groups, float dt, uint32_t iterations,
                    float* out_impulse, float* out_torque, uint32_t* out_live, float* out_tie);
int pies_get_tie_state(const pies_solver_t* s, uint32_t set, uint8_t* broken, uint32_t capacity, uint32_t* n_broken);
int pies_reset_ties(pies_solver_t* s, uint32_t set);
/* EXTENSION (the reference fixes a constraint's rest datum at creation): ACTUATORS - distance and bend constraints whose rest length
 * or rest angle the host drives every tick, written where HBM holds the rest records, under every schedule and both solvers: a
 * muscle, a tendon, a pneumatic bellows, a winch cable, a hinge that folds.  pies_set_rest does the same edit through a full
 * rebuild; a drive call rebuilds nothing: the rest datum of a distance or bend constraint lives in one word of one record that
 * every kernel reads through a pointer, and enters no plan, colouring, dictionary or system matrix.
 * Tetrahedral and volume rest data do and stay with pies_set_rest.
 * SETS ARE ASSETS exactly as anchor sets are: pies_add_actuators stores n actuators that refer to n_channels activation channels
 * and returns the set's id (0, 1, ... per handle); a set survives pies_finalize, scene edits and ticks and ends with pies_clear or
 * pies_destroy.  The library keeps a host copy - pies_get_actuators reads it and needs no device - and stages the device copy at the
 * first drive and again after a pies_finalize dropped it, with every index translated to the constraint's slot in the order the
 * device holds (the inverse of what pies_get_order returns); pies_add_actuators works on PIES_DEVICE_NONE handles.  index is the
 * constraint's index in its container in HOST order (pies_get_ids / pies_get_rest order), of a constraint that exists at the call;
 * constraints appended later do not disturb a set.  pies_add_actuators writes `base` of the stored copy: the constraint's rest datum
 * at that moment (what pies_get_rest returns then; the caller's value is ignored).  No two actuators of one set name the same
 * constraint; when two sets drive one constraint the later call wins.  pies_get_actuators: actuators may be NULL (then capacity is
 * not read), else capacity >= the set's count; n and n_channels may each be NULL.
 * pies_drive_actuators drives one set with the activations of this call (n_channels floats, the set's count).  The outputs may each
 * be NULL: out_sums (n_channels x 2), out_live (n_channels), out_actuator (n x 2, the set's own order).
 * The rule, in fp32 without fused multiply-adds, with pies_apply_anchors' conventions: dot products summed left to right as
 * x x + y y + z z, cross(a, b) = (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y) as in pies_raycast, a + b * t is the
 * product rounded, then the sum, a vector divided by a scalar is taken componentwise, every test is the positive form written.  Only
 * + - * / sqrtf fminf fmaxf and comparisons occur.  For actuator i with u = activation[channel_i]:
 *   r_i = base_i * (1.0f + gain_i * u)          with PIES_ACTUATOR_OFFSET:  r_i = base_i + gain_i * u
 *   r_i = fminf(fmaxf(r_i, lo_i), hi_i)
 * The actuator is LIVE iff u - u == 0.0f (u is finite: inf - inf and NaN - NaN are NaN, which equals nothing).  A live actuator
 * replaces the rest datum of its constraint by r_i in every device array that holds it; an actuator that is not live writes nothing
 * and its constraint keeps the rest it has.
 *   value_i, measured on the state the call found, from the constraint's own node ids a b (c d); p is a position:
 *     DISTANCE: d = p_a - p_b;  value_i = sqrtf(d . d)
 *     BEND:     p2 = p_b - p_a, p3 = p_c - p_a, p4 = p_d - p_a;  e = cross(p2, p3), f = cross(p2, p4);
 *               n1 = e / sqrtf(e . e), n2 = f / sqrtf(f . f);  value_i = n1 . n2
 *               - the cosine of the dihedral angle exactly as the bend projection forms it before its acos (Constraints.cpp:321-339).
 * out_actuator[2 i] = r_i (of an actuator that is not live: the rest its constraint keeps), out_actuator[2 i + 1] = value_i.
 * out_sums[2 c] sums value_i over the LIVE actuators of channel c and out_sums[2 c + 1] sums r_i over the same actuators, in a fixed
 * two-level order: per tile of 256 consecutive actuator indices in ascending index from 0.0f (another channel's actuator, and one
 * that is not live, adds 0), then the tiles in ascending index from 0.0f.  out_live[c] counts the live actuators of channel c.
 * Nothing is summed with atomics and the order is a function of the set alone - not of a kernel variant, a schedule or
 * PIES_FLAG_RENUMBER_NODES -, so two calls agree bit for bit.  Node state is not written.
 * A drive runs on the handle's stream behind whatever ticks and begun frames are queued, finalizes a changed scene first, and is one
 * launch plus the fold of the tile sums; captured graphs, pies_launch_counts and export frames begun earlier are left as they were
 * and nothing enters the captured substep.  pies_drive_actuators synchronises once before it returns.
 * pies_drive_actuators_device takes activation and the outputs as DEVICE pointers (floats and uint32 words, 4-byte aligned, device
 * memory of the handle's device) and follows pies_write_nodes_device's stream rule word for word: the solver's stream waits for what
 * `stream` has queued, `stream` waits for the call's launches, no host synchronisation unless flags has PIES_IO_HOST_SYNC, and
 * PIES_ERR_STATE when `stream` is capturing.  It cannot check the activations: the LIVE rule covers them.
 * THE HOST MIRROR STAYS TRUTHFUL.  The edit is in HBM only: the mirror's rest lengths and angles are marked stale and copied back
 * through the slot map when someone needs them - pies_get_rest, any scene edit, any rebuild -, so pies_get_rest returns the driven
 * values, a later full rebuild (pies_set_schedule, pies_set_solver, an appended body, a flag that rebuilds) keeps them, and a
 * pies_set_rest made after a drive overrides it for its range.
 * pies_add_actuators: PIES_ERR_INVALID for NULL actuators or n == 0, a type other than PIES_DISTANCE / PIES_BEND, an index beyond its
 * container, n_channels == 0 or > PIES_ACTUATOR_CHANNEL_MAX, channel >= n_channels, a non-finite gain, lo or hi, lo > hi, a
 * negative lo on DISTANCE, an unknown flag, a constraint listed twice; PIES_ERR_UNSUPPORTED for more than 2^24 actuators or more
 * than PIES_ACTUATOR_SET_MAX sets.  The drive calls: PIES_ERR_INVALID for an unknown set, n_channels different from the set's, a
 * NULL activation, (host-pointer form) a non-finite activation, (device form) a pointer that fails pies_write_nodes_device's
 * checks; PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first). */
#define PIES_ACTUATOR_SET_MAX 64     /* sets per handle */
#define PIES_ACTUATOR_CHANNEL_MAX 64 /* activation channels per set */
enum { PIES_ACTUATOR_OFFSET = 1 };   /* flags: r = base + gain u instead of base (1 + gain u) */
typedef struct pies_actuator {       /* 32 bytes */
  int32_t type;      /* PIES_DISTANCE or PIES_BEND */
  uint32_t index;    /* the constraint's index in its container, host order (pies_get_ids / pies_get_rest order) */
  uint32_t channel;  /* index into the activations of a drive call */
  float gain;        /* finite */
  float lo, hi;      /* the written rest is clamped to [lo, hi]; lo <= hi, finite; DISTANCE: lo >= 0 */
  float base;        /* written by the library at pies_add_actuators: the constraint's rest datum at that moment */
  uint32_t flags;    /* 0 or PIES_ACTUATOR_OFFSET */
} pies_actuator_t;
int pies_add_actuators(pies_solver_t* s, uint32_t n, const pies_actuator_t* actuators, uint32_t n_channels, uint32_t* set);
int pies_get_actuators(const pies_solver_t* s, uint32_t set, pies_actuator_t* actuators, uint32_t capacity, uint32_t* n, uint32_t* n_channels);
int pies_drive_actuators(pies_solver_t* s, uint32_t set, uint32_t n_channels, const float* activation, float* out_sums,
                         uint32_t* out_live, float* out_actuator);
int pies_drive_actuators_device(pies_solver_t* s, uint32_t set, uint32_t n_channels, const void* activation, void* out_sums,
                                void* out_live, void* out_actuator, void* stream, uint32_t flags);
/* EXTENSION (the reference has no such query): STRAIN, VOLUME AND MOMENTUM MEASURES evaluated where HBM holds the body - how the
 * body is doing, without a read-back.  Both calls are READ-ONLY: node state, the host mirror's stale marks, export frames begun
 * earlier, captured graphs and pies_launch_counts are left exactly as they were.  They run on the handle's stream behind whatever
 * ticks and begun frames are queued, finalize a changed scene first (so a pies_set_rest or an appended body between two calls is
 * seen by the second) and synchronise once before they return.  Their buffers (the staged element records among them) are built
 * at the first call after a pies_finalize and freed by the next pies_finalize, pies_clear or pies_destroy.
 * Both rules are fp32 without fused multiply-adds except where svd3 writes one, with pies_collide_props' conventions: dot
 * products summed left to right as x x + y y + z z, cross is pies_raycast's, a vector times a scalar is taken componentwise,
 * every test is the positive form written, so a NaN fails it.
 *
 * pies_measure_elements: elements [first, first + n) of the PIES_TET or the PIES_VOLUME container (both hold 4 node ids, Qinv and
 * two limits), numbered in the order the host added them - under PIES_FLAG_RENUMBER_NODES, in every schedule and under both
 * solvers the answer is a function of host order alone.  out: n records or NULL; summary: or NULL.  For element e with nodes
 * x1..x4 at the positions the device holds and the rest data (Qinv, lo, hi) of the call's moment:
 *   P[i] = x(i+2) - x1 (i = 0, 1, 2: the columns);  F = P Qinv in the reference's column-major arrays, as the tetrahedral
 *     projection forms it:  F[c][r] = (P[0][r] * Qinv[c][0] + P[1][r] * Qinv[c][1]) + P[2][r] * Qinv[c][2]   (Qinv[c][r] is
 *     word 3 c + r of pies_get_rest);
 *   det(M) = (M[0][0] * (M[1][1] * M[2][2] - M[2][1] * M[1][2]) - M[1][0] * (M[0][1] * M[2][2] - M[2][1] * M[0][2]))
 *            + M[2][0] * (M[0][1] * M[1][2] - M[1][1] * M[0][2]);      j = det(F);  volume = det(P) / 6.0f, signed by the
 *     element's node order (volume / j is the rest volume with the same sign; the lattice factories do not wind all their
 *     elements alike, so a host that wants a body's volume adds the records' magnitudes, not the summary's signed sum);
 *   i1 = the nine squares F[c][r] * F[c][r] added in the array's order, c outer and r inner, starting from F[0][0] * F[0][0];
 *   (a0, a1, a2) = the singular values the projection's SVD (svd3, pies_amd/csrc/dev_math.h) returns for the array F handed over
 *     as the projection hands it over (no transposition), sorted descending by the compare-exchanges (0, 1), (1, 2), (0, 1), each
 *     swapping iff a < b;  s = (a0, a1, a2), and iff j < 0.0f the last is negated: s[2] = -a2 (the projection's flip,
 *     Constraints.cpp:106-108);
 *   g_i = s[i] * s[i] - 1.0f;  green = 0.5f * sqrtf((g0 * g0 + g1 * g1) + g2 * g2): the Frobenius norm of the Green strain, zero
 *     at rest and invariant under rotation;
 *   flags: PIES_ELEMENT_NONFINITE iff not every entry of F has fabsf(F[c][r]) < +inf - the record's flags are then that bit alone,
 *     its other words are stored as computed and are unspecified, and the summary passes the element by (the call still returns:
 *     the SVD's sweeps are bounded).  Otherwise PIES_ELEMENT_INVERTED iff j < 0.0f, and with the limits as
 *     pies_add_tet_constraints / pies_add_volume_constraints took them
 *       PIES_TET:     PIES_ELEMENT_OVER iff s[0] > max_strain,  PIES_ELEMENT_UNDER iff fabsf(s[2]) < min_strain;
 *       PIES_VOLUME:  prod = (a0 * a1) * a2;  PIES_ELEMENT_OVER iff prod > stretching,  PIES_ELEMENT_UNDER iff prod < compression.
 * The summary covers the elements of the range that are not NONFINITE (nonfinite counts the others): the counts inverted, over,
 * under; volume: the elements' volumes in a fixed two-level order - per tile of 256 consecutive indices of the container (tile
 * t = indices 256 t .. 256 t + 255, restricted to the range) in ascending index from 0.0f, then the tile sums in ascending tile
 * index from 0.0f; max_stretch (of s[0]), min_stretch (of fabsf(s[2])), min_j, max_j, max_green: minima and maxima are
 * order-free but for +-0 and a NaN from an overflow, and so that those have one answer too they walk the same two levels - the
 * held value starts as the first one met and is replaced by x iff x < it (a maximum: x > it), over a tile's elements and then
 * over the values of the tiles that hold one; all five are 0.0f when the range holds no element that counts.  No atomics: two
 * calls agree bit for bit.  With out == NULL no record is
 * written; with summary == NULL nothing is reduced; with both NULL the call validates and synchronises.
 * PIES_ERR_INVALID: a type other than PIES_TET / PIES_VOLUME, a range that leaves the container.  n == 0: PIES_OK and a zero
 * summary.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are checked first).
 *
 * pies_measure_nodes: mass, momentum, angular momentum, first moment and kinetic energy of up to PIES_MEASURE_RANGE_MAX ranges of
 * HOST node ids: ranges holds n_ranges (first, count) pairs - a body is the id range its create* / pies_add_nodes call returned -
 * which may overlap and may be empty; about: 3 floats per range, the point the angular momentum refers to, or NULL: the origin.
 * Per range over its nodes with invMass w != 0 (a node with w == 0 is counted in `fixed` and adds nothing else), with position
 * p, velocity v and m = 1.0f / w:
 *   mass = sum m;  momentum = sum v * m;  angular = sum cross(p - about, v * m);  moment = sum p * m (divide by mass for the
 *   centre of mass);  kinetic = sum 0.5f * (m * (v.v));  dynamic, fixed: the node counts.
 * Every float sum is taken in pies_collide_props' fixed two-level order: per tile of 256 consecutive HOST ids of the global
 * tiling (tile t = ids 256 t .. 256 t + 255) the range's nodes in ascending id from 0.0f, then the tiles in ascending index from
 * 0.0f.  The order is a function of the range alone - not of PIES_FLAG_RENUMBER_NODES, not of the other ranges of the call - so
 * a range gives the same bits alone and in a list of 64.  THESE ARE fp32 SUMS: at 100 000 nodes the last digits of mass are
 * rounding (a sum of n terms carries an error of the order of n 2^-24 of its magnitude at worst, sqrt(n) 2^-24 typically); a
 * host that needs more digits sums fewer nodes per range and adds the ranges in double precision.
 * PIES_ERR_UNSUPPORTED: n_ranges > PIES_MEASURE_RANGE_MAX.  PIES_ERR_INVALID: NULL ranges or out with n_ranges > 0, a range that
 * leaves [0, nodes), a non-finite about.  n_ranges == 0: PIES_OK.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle (the arguments are
 * checked first). */
enum { PIES_ELEMENT_INVERTED = 1, PIES_ELEMENT_OVER = 2, PIES_ELEMENT_UNDER = 4, PIES_ELEMENT_NONFINITE = 8 };
#define PIES_MEASURE_RANGE_MAX 64
typedef struct pies_element_measure {
  float s[3];      /* the stretches, descending; s[2] < 0 on an inverted element */
  float j;         /* det F */
  float volume;    /* current; signed by the node order: det [x2 - x1, x3 - x1, x4 - x1] / 6 */
  float i1;        /* |F|_F^2 */
  float green;     /* |E|_F, E = (F^T F - 1) / 2 */
  uint32_t flags;  /* PIES_ELEMENT_* */
} pies_element_measure_t;
typedef struct pies_element_summary {
  float max_stretch, min_stretch, min_j, max_j, max_green, volume;
  uint32_t inverted, over, under, nonfinite;
} pies_element_summary_t;
typedef struct pies_node_sums {
  float mass;
  float momentum[3];
  float angular[3];
  float moment[3];
  float kinetic;
  uint32_t dynamic, fixed;
} pies_node_sums_t;
int pies_measure_elements(pies_solver_t* s, int type, uint32_t first, uint32_t n, pies_element_measure_t* out,
                          pies_element_summary_t* summary);
int pies_measure_nodes(pies_solver_t* s, uint32_t n_ranges, const uint32_t* ranges, const float* about, pies_node_sums_t* out);
/* _simFailed latch (Solver.cpp:26-28,853-856) */
int pies_failed(pies_solver_t* s, int* failed);
/* Point-triangle contacts of the last PD substep (Solver::_triCollisions, Solver.h:187), in list order:
 * 4 node ids each (point a, triangle b c d).  ids may be NULL to query the count. */
int pies_get_tri_contacts(pies_solver_t* s, uint32_t* ids, uint32_t capacity, uint32_t* count);
/* Broad phase of the last PD substep's point-triangle detection (diagnostics; synchronises).  The device lists every surface
 * triangle once, in the cell of the minimum corner of its swept range, in one of three size classes (cells of 1, 4 and 16 world
 * cells; pies_amd/csrc/tri_kernels.h) - the reference lists it in every cell of the range (Solver.cpp:692, SpatialHash.h:141-176);
 * the pairs and the contact list are the same.  out[0] = pairs handed to the CCD (Solver.cpp:775-797 runs it for every pair
 * without a common node in a shared cell), out[1] = pairs with at least one hit, out[2..4] = longest range listed per class (in
 * cells of the class), out[5..7] = triangles listed per class. */
int pies_get_tri_grid_stats(pies_solver_t* s, uint32_t out[8]);
/* PIES_FLAG_PD_NODE_CONTACTS: the node-node contacts of the last PD substep as (i, j) pairs of host ids (ids: 2 x count), in the
 * order the friction loop ran them (ascending pair key, taken over host ids).  ids may be NULL to query the count; synchronises.
 * The reference keeps them in Solver::_collisions (Solver.h), filled by _parallelComputeCollisions (Solver.cpp:509-637). */
int pies_get_node_contacts(pies_solver_t* s, uint32_t* ids, uint32_t capacity, uint32_t* count);
/* Node-node pairs resolved by the PBD collision pass since the last call (statistics). */
int pies_collision_pairs(pies_solver_t* s, uint64_t* pairs);
/* The same plus the candidates the pass looked at (bucket entries visited, the unit of SURVEY 8d's "16 B per candidate
 * neighbour"); both counters restart. */
int pies_collision_stats(pies_solver_t* s, uint64_t* pairs, uint64_t* candidates);
/* Pair order: level launches captured per pass.  By default the library follows what the passes need at host synchronisations
 * (it starts at 96; BASELINE config 4 settles at 48 in the pair order, at ~1 100 in the reference's order by turns); a call pins the count.  A single-workgroup kernel finishes deeper
 * orders than captured: slow, never wrong. */
int pies_set_collision_rounds(pies_solver_t* s, uint32_t rounds);
/* Tuning and diagnostic switches, process wide, by name (value NULL or "" unsets): graph variants and sizes that tests and
 * profiling scripts pin - PIES_PCG_BUDGET, PIES_PCG_OVERFLOW, PIES_TRI_FAST_ROWS, PIES_TRI_LDS, PIES_ROW_MAX_UNIQUE, PIES_TRI_SIDE, PIES_TRI_TEAM,
 * PIES_NO_GRAPH, PIES_NO_WAVEFRONT, PIES_NO_TET_PAIRS, PIES_PD_LOCAL_PACKED (0: one element per lane in the PD strain + volume step),
 * PIES_PD_REST_DICT (0: per-element constants instead of the rest dictionary), PIES_LAYER_REST_DICT (0: the same for the tetrahedral
 * container of schedule LAYERED, PBD), PIES_PD_ROW_DICT (0: the PD system matrix as SELL
 * arrays only, no row dictionary), PIES_LAYER_PLAN (0: schedule LAYERED's original plan only, 1: + single-level constraints dealt to either group, 2: + slabs by position; default 2) / _PLAN_FORCE (candidate index) / _SLAB / _SLAB_OFFSET, PIES_LAYER_ONE_STRIP_MAX / _TILE_NODES / _STRIPS_MIN_NODES / PIES_LAYER_BLOCK,
 * PIES_PD_TILE_ELEMS (0: per-(element, node) records instead of the tile-resident local step), PIES_PD_CG_SINGLE / _SINGLE_ROWS (0: the
 * two-launch CG everywhere / in the contact-heavy variant), PIES_PD_FUSE_RHS (0: k_pd_rhs), PIES_PD_RHS_LANES,
 * PIES_PD_NODE_CONTACT_PARTNERS (partners per node of PIES_FLAG_PD_NODE_CONTACTS, default 32) / _ROUNDS (pins the friction rounds captured),
 * PIES_COLOUR_ROUNDS, PIES_COLOUR_DSATUR, PIES_NO_COLOUR_HINT, PIES_SELL_LANES, PIES_CG_BLOCKS, PIES_COLLIDE_GLOBAL / _PASSES /
 * _SPIN_LIMIT; round 5: PIES_PD_WINDOW (0: no windowed matrix, 2: also beside a row dictionary) / _WINDOW_KERNELS (1 iterations, 2 first
 * product, 4 residual; default 3) / _WINDOW_SORT / _WINDOW_HALO32 (tests: 32-bit halo list), PIES_CG_CHUNK_ROWS, PIES_PCG_NEVER_EXIT (profiling: every captured CG launch works),
 * PIES_REFERENCE_TURNS (0: the reference's node-node order as one sequential chain, 1: by turns whatever the size; default: by turns from
 * 1 024 nodes on), PIES_FALLBACK_VISITS (candidate tests a pass left to the sequential loop may cost before it latches: 1e9),
 * PIES_PAIR_QUADS (0: one lane per pair in the pair order's levels) / _QUAD_BLOCKS / _QUAD_THREADS / PIES_PAIR_LOOK_WAVES (wavefronts of a level workgroup that look at frontier nodes, at most);
 * pies_raycast, read at every call: PIES_RAY_VARIANT (wide: one ray per lane, narrow: one triangle per lane; unset: narrow up to
 * PIES_RAY_NARROW_MAX rays, default 512: the measured crossover), PIES_RAY_CHUNKS (pins the triangle chunks of the wide variant, 1 .. 1 024);
 * pies_closest_points, read at every call: PIES_NEAR_VARIANT (wide: one point per lane, narrow: one triangle per lane; unset: narrow
 * up to PIES_NEAR_NARROW_MAX points, default 4 096: the end of the measured sweep), PIES_NEAR_CHUNKS
 * (pins the triangle chunks of the wide variant, 1 .. 1 024); the winding pass has one form;
 * pies_apply_forces, read at every call: PIES_FORCE_VARIANT (inplace: one launch writes the velocities where they are, scratch:
 * new velocities to a scratch array, a second launch commits them; unset: inplace; a list with a wind always takes scratch: its
 * lanes read their neighbours' velocities);
 * pies_apply_surface_loads, read at every call: PIES_LOAD_VARIANT (inplace / scratch as above; unset: inplace; a list with a
 * fluid drag always takes scratch);
 * pies_read_nodes_device / pies_write_nodes_device, read at every call: PIES_NODE_IO_VARIANT (plain: a packed stride-3 row moves as
 * its lane's three floats, staged: a tile's rows pass through LDS and cross as 16-byte accesses; unset: plain).
 * They take effect where the library reads them (pies_create, pies_finalize or the next graph capture).  pies_set_tuning must not
 * race with other API calls of the process (a handle reads the switches at different times of its life).  None of
 * them is read from the environment: the only environment variables the library looks at are PIES_SCHEDULE (default schedule
 * of new handles), PIES_PROFILER_SAFE (profiling runs) and the print-only PIES_PCG_DEBUG / PIES_LAYER_DEBUG. */
int pies_set_tuning(const char* name, const char* value);
/* Diagnostics of the pair order: per node the slack for the next pass, the excursion and the listed partners of the last pass. */
int pies_debug_pair_state(pies_solver_t* s, float* slack, float* excursion, uint32_t* partners, uint32_t n);
/* Pair order (PIES_COLLISION_ORDER_PAIRS): the last pass's dependency levels and listed pairs; since pies_finalize, the passes
 * that were repeated with the widest slack because a node had moved further than the pair filter allows for, and the passes in
 * which a node moved further than even that (more than 0.5 in one pass: the result may then miss visits the documented order
 * makes).  Any pointer may be NULL. */
int pies_get_collision_health(pies_solver_t* s, uint32_t* levels, uint32_t* pairs_listed, uint32_t* passes_repeated, uint32_t* passes_inexact);
/* Node-node passes (since the handle's buffers were built) that the SEQUENTIAL loop of the reference ran in place of a parallel order:
 * a pile the partner lists do not hold (more than 1 024 nodes within reach of one node, more listed pairs than reserved, more than
 * 65 535 nodes in a cell), or - reference order by turns - a pass that could not be proved exact.  Such a pass has the reference's
 * own order and result (Src/Solver.cpp:85-130 has no limit and no latch); it is slow, not wrong. */
int pies_get_collision_fallbacks(pies_solver_t* s, uint32_t* passes);

/* ---- state access --------------------------------------------------------------------------- */
int pies_count(const pies_solver_t* s, int what, uint32_t* out);
/* out: n x 3 floats for POSITION/PREV_POSITION/VELOCITY, n floats for RADIUS/INV_MASS */
int pies_read_nodes(pies_solver_t* s, int what, float* out, uint32_t n);
/* Positions into a caller array with a byte stride (Solver::Vertex::position of a std::vector<Vertex>:
 * `_vertices[i].position = node.position`, Solver.cpp:157,393).  After pies_tick this is a host-side copy. */
int pies_read_positions_strided(pies_solver_t* s, void* dst, uint64_t stride_bytes, uint32_t n);
int pies_write_nodes(pies_solver_t* s, int what, const float* in, uint32_t n);
/* EXTENSION: node state and skins to and from DEVICE memory of the caller - a renderer with HIP interop, a controller or a force
 * model that lives on the GPU (a torch tensor's data_ptr) - without a copy across the bus and without a host synchronisation.
 * Every pointer of pies_device_nodes_t is a device pointer of the handle's device, or NULL (that array is not wanted): position,
 * prev_position, velocity hold `stride` (3 or 4) floats per node, radius and inv_mass one.  Row i is HOST node i, also under
 * PIES_FLAG_RENUMBER_NODES.
 * pies_read_nodes_device fills the non-NULL arrays with exactly the words pies_read_nodes returns; with stride == 4 the fourth float
 * is written as 0.0f.  n must be pies_count(PIES_NODES).  A changed scene or a pending pies_write_nodes is brought to the device
 * first.  Read-only: no stale mark, nothing a tick can observe.
 * pies_write_nodes_device replaces position, prev_position and / or velocity in HBM.  radius and inv_mass must be NULL
 * (PIES_ERR_UNSUPPORTED: they size the node grid and the PD system; pies_write_nodes remains their path).  ids == NULL: m must be
 * the node count and row k goes to host node k.  Otherwise ids is a DEVICE array of m host ids and row k goes to node ids[k]; the
 * ids must be distinct (with duplicates, which row wins is unspecified); a row whose id is not below the node count is ignored.  A
 * position write keeps pos.w (the inverse mass); with stride == 4 the source's fourth float is not used.  The host mirror is marked
 * stale for the written arrays like after pies_collide_props: nothing is uploaded, and pies_read_nodes, pies_tick and a scene edit
 * see the result.  A pies_write_nodes made before the call is uploaded before it.
 * pies_read_skin_device: pies_read_skin's rule and launches, the vertices (n x 3 floats) and normals (n x 3, may be NULL) of skin
 * `skin` written to caller memory; n must be the skin's vertex count.
 * Streams.  `stream` is the caller's hipStream_t, by value; NULL is the legacy default stream.  The library records an event on
 * the caller's stream and lets the solver's stream wait for it (the caller's earlier work on the buffers is finished first),
 * launches on the solver's stream - one launch per node call, however many arrays -, records a second event there and lets the
 * caller's stream wait for it: work the caller queues on `stream` afterwards sees the result.  The host is never synchronised
 * unless flags has PIES_IO_HOST_SYNC (the call then returns after its launches have finished).  Frames begun before the call
 * (pies_tick_begin) hold the state before it.  A caller stream that is capturing returns PIES_ERR_STATE.  The store of the packed
 * stride-3 form has two variants, pies_set_tuning("PIES_NODE_IO_VARIANT", "plain" | "staged"); the words are
 * the same.  No atomics: two calls agree bit for bit.
 * PIES_ERR_INVALID: a NULL handle or struct, every pointer NULL, a stride other than 3 or 4, a wrong n or m, an unknown skin, a
 * pointer that is not 4-byte aligned, a pointer that is not device memory of the handle's device (or whose allocation ends before
 * the array does), an unknown PIES_NODE_IO_VARIANT.  n == 0 (m == 0) returns PIES_OK.  PIES_ERR_HIP: a PIES_DEVICE_NONE handle
 * (the arguments are checked first; what needs a device to be checked - the pointers' memory - comes after). */
typedef struct pies_device_nodes {
  void *position, *prev_position, *velocity; /* device pointers or NULL; `stride` floats per node */
  void *radius, *inv_mass;                   /* device pointers or NULL; 1 float per node; read only */
  uint32_t stride;                           /* 3 or 4 */
} pies_device_nodes_t;
enum { PIES_IO_HOST_SYNC = 1 };
int pies_read_nodes_device(pies_solver_t* s, const pies_device_nodes_t* dst, uint32_t n, void* stream, uint32_t flags);
int pies_write_nodes_device(pies_solver_t* s, const pies_device_nodes_t* src, const uint32_t* ids, uint32_t m, void* stream, uint32_t flags);
int pies_read_skin_device(pies_solver_t* s, uint32_t skin, void* positions, void* normals, uint32_t n, void* stream, uint32_t flags);
/* node ids of a container, flattened, in the order the host added them */
int pies_get_ids(const pies_solver_t* s, int type, uint32_t* out, uint32_t capacity);
/* node ids of shape (PIES_SHAPE) or goal (PIES_GOAL) constraint `index`; ids may be NULL to query count */
int pies_get_group(const pies_solver_t* s, int type, uint32_t index, uint32_t* ids, uint32_t capacity, uint32_t* count);
/* rest data in host order: DISTANCE target (1), TET/VOLUME Qinv column-major (9), BEND angle (1) */
int pies_get_rest(const pies_solver_t* s, int type, float* out, uint32_t capacity);
/* replaces the rest data of constraints [first, first + n) of a container (same layout as pies_get_rest; TET / VOLUME: A and AtA follow
 * from the new Qinv).  The reference's factories take the rest pose from the node positions at creation (Src/Constraints.cpp:39-56,
 * 130-184, 257-310, 368-394); this is the bulk raw ingestion of SURVEY 8b ("distance (ids, rest, w) ... tet/volume (ids, Qinv,
 * params, w)") for hosts that restore a saved scene. */
int pies_set_rest(pies_solver_t* s, int type, uint32_t first, uint32_t n, const float* rest);
/* Execution order of a container under the current schedule: order[slot] = index in host order.
 * batch_offsets (may be NULL) receives n_batches+1 slot offsets; batches run one after another. */
int pies_get_order(pies_solver_t* s, int type, uint32_t* order, uint32_t capacity);
int pies_get_batches(pies_solver_t* s, int type, uint32_t* batch_offsets, uint32_t capacity, uint32_t* n_batches);
/* The node numbering of the device (PIES_FLAG_RENUMBER_NODES): order[internal] = host id, n = pies_count(PIES_NODES) entries; the
 * identity when no renumbering is in effect.  Finalizes a changed scene first, like pies_get_order (also on PIES_DEVICE_NONE). */
int pies_get_node_order(pies_solver_t* s, uint32_t* order, uint32_t capacity);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Times one kernel class in isolation: a graph holding only that class's launches of one substep is
 * replayed a few times back to back between two HIP events recorded on the solver's stream (the launches form
 * one dependent chain, so time / launches is the per-launch device time including the kernel boundary).  Returns the launches
 * timed, the total milliseconds and the units (constraints or nodes) processed.  One class's working set is usually cache
 * resident in such a replay: these are launch-latency figures, not bandwidth figures.  The node state is put back. */
enum { PIES_KERNEL_PREDICT = 0, PIES_KERNEL_POSITION = 1, PIES_KERNEL_DISTANCE = 2, PIES_KERNEL_TET = 3,
       PIES_KERNEL_BEND = 4, PIES_KERNEL_FLOOR = 5, PIES_KERNEL_VELOCITY = 6, PIES_KERNEL_HASH = 7,
       PIES_KERNEL_COLLIDE = 8,
       /* projective dynamics (Solver.cpp:228-485) */
       PIES_KERNEL_PD_PREDICT = 9, PIES_KERNEL_PD_LOCAL_DISTANCE = 10, PIES_KERNEL_PD_LOCAL_TET = 11,
       PIES_KERNEL_PD_LOCAL_VOLUME = 12, PIES_KERNEL_PD_RHS = 13, PIES_KERNEL_PD_SPMV = 14,
       PIES_KERNEL_PD_CG_UPDATE = 15, PIES_KERNEL_PD_VELOCITY = 16,
       /* (round 4, graph variants with one launch per CG iteration - pies_count(PIES_PD_CG_SINGLE): PD_SPMV is k_cg1_iter, a whole
        * PCG iteration; PD_CG_UPDATE has no launches; PD_RHS is k_cg1_init when that kernel evaluates the right-hand side
        * itself - tile-resident local step, pies_count(PIES_PD_TILES) -, otherwise k_pd_rhs) */
       /* schedule EXACT: one dependency level of the whole-substep DAG (all projection kinds + floor clamps) */
       PIES_KERNEL_WAVE = 17,
       /* schedule LAYERED: the groups of one parity, LDS resident (units = algorithmic bytes of the projections and
        * per-node steps the launches execute, SURVEY 8d figures) */
       PIES_KERNEL_LAYER = 18, PIES_KERNEL_COUNT = 19 };
int pies_profile_substep(pies_solver_t* s, int kernel, uint32_t* launches, double* total_ms, uint64_t* units);
/* Times one kernel class where it runs: `substeps` whole substeps are launched eagerly (every kernel of the substep
 * runs, so the caches hold what the substep leaves in them) and each launch of the class is bracketed by two HIP events
 * on the solver's stream.  launches = bracketed launches (for PIES_KERNEL_HASH / _COLLIDE one bracket is the whole grid
 * build / resolve pass), total_ms = the sum of their event times, units as in pies_profile_substep.  For the CG classes
 * (PD_SPMV, PD_CG_UPDATE) the solves of this pass do not take the converged early exit, so every bracketed launch does
 * the full work.  bracket_overhead_ms (may be NULL): what one bracket costs by itself, measured in the same pass around one
 * and around two launches of an empty kernel (the event packets and the wait for the end-of-kernel cache write-back: several
 * microseconds, i.e. most of a bracket around a short kernel) - subtract it per launch to compare with rocprofv3's
 * kernel durations.  The node state is put back afterwards. */
int pies_profile_in_situ(pies_solver_t* s, int kernel, uint32_t substeps, uint32_t* launches, double* total_ms, uint64_t* units,
                         double* bracket_overhead_ms);
/* The tile plan of the PD strain + volume local step, computed from the host-side scene (also on PIES_DEVICE_NONE handles): tiles of
 * up to 128 element pairs on up to 128 nodes (one wavefront each).  n_tiles = 0 when the scene keeps per-(element, node) records
 * (no strain + volume pairs).  With info != NULL the plan is copied out at fixed strides per tile: info[t] = nodes | elements << 16,
 * node[128 t + k] = node of tile node k (host id, also when the nodes are renumbered), elem[128 t + e] = host index of element slot e, local[128 t + e] = its four tile-local
 * node indices (8 bits each), nptr[132 t + k] .. nptr[132 t + k + 1] = tile node k's entries in inc[512 t + ..] (element << 2 |
 * corner).  Any array pointer but info may be NULL. */
int pies_get_pd_tile_plan(pies_solver_t* s, uint32_t* n_tiles, uint32_t* info, uint32_t* node, uint32_t* elem, uint32_t* local, uint16_t* nptr,
                          uint16_t* inc, uint32_t tile_capacity);
/* The tetrahedral rest dictionary of schedule LAYERED (PIES_LAYER_REST_SETS), for inspection and tests; no handle is needed.
 * pack: four tile-local node ids (13 bits each, <= 8191) and a set index (12 bits) into the element's two record words;
 * PIES_ERR_INVALID when one does not fit.  unpack: the inverse.  usable: 1 when a scene of `count` elements with `sets` distinct sets
 * of rest constants and tiles of up to max_group_nodes nodes takes the dictionary on a device whose workgroups have lds_bytes of
 * LDS (0: gfx950's 160 KB, what a PIES_DEVICE_NONE handle decides with), else 0 (the rule is all or nothing per scene). */
int pies_layer_rest_pack(const uint32_t* ids, uint32_t set, uint32_t* words);
int pies_layer_rest_unpack(const uint32_t* words, uint32_t* ids, uint32_t* set);
int pies_layer_rest_usable(uint32_t sets, uint32_t count, uint32_t max_group_nodes, uint32_t lds_bytes);
/* launches per substep of the captured graph, per kernel class (PIES_KERNEL_COUNT entries) */
int pies_launch_counts(pies_solver_t* s, uint32_t* out);
/* The library's resource ledger: every HIP resource it creates or destroys is counted, process-wide, over all handles.  No handle
 * is taken, so what a destroyed handle left behind stays visible: after the last pies_destroy every live figure is 0.
 *   out[0..7]  live now:           device bytes, device allocations, pinned host bytes, pinned host allocations, streams, events,
 *                                  graphs, executable graphs
 *   out[8..15] created since load: the same eight kinds, in the same order (never decreasing)
 * Device and pinned bytes are the sizes requested, not what the allocator rounds them to.  pies_clear returns a handle to what
 * pies_create gave it (two streams, two events) plus what two call families create once per handle and pies_destroy releases:
 * pies_tick_begin a stream, four events and the frame buffers on the device and in pinned memory (they keep the size of the
 * largest scene exported), the device-side node and skin access (pies_read_nodes_device and kin) two events.  A graph whose
 * destruction is skipped under PIES_PROFILER_SAFE=1 stays counted as live.  Nothing inside pies_tick / pies_tick_async creates a
 * resource once the scene is finalized; pies_finalize, the first call of a query or edit entry point, and a call with more rays,
 * points or nodes than any before it, may.  Safe to call from any thread at any time; the sixteen words are read one by one, not
 * as a snapshot.  PIES_ERR_INVALID when out is NULL. */
int pies_resource_counts(uint64_t out[16]);

#ifdef __cplusplus
}
#endif
#endif /* PIES_HIP_H */

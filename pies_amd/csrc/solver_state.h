// Internal state of one pies_solver handle: host mirror of the scene (authoritative until the first
// tick / after a read-back), schedules, HBM buffers, the captured substep graph.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pies_hip.h"
#include "resource_ledger.h"
#include "kernels.h"
#include "pd_kernels.h"
#include "hash_kernels.h"
#include "pd_contact_kernels.h"
#include "pair_kernels.h"
#include "skin_kernels.h"
#include "ray_kernels.h"
#include "field_kernels.h"
#include "measure_kernels.h"
#include "anchor_kernels.h"
#include "tie_kernels.h"
#include "actuator_kernels.h"

namespace pies {

struct VelocityScratch;  // force_kernels.h

struct HostPosition {
  uint32_t id;
  float target[3];
  float w;
};
constexpr uint16_t kNoColourHint = 0xFFFFu;
struct HostDistance {
  uint32_t ids[2];
  float target;
  float w;
  uint16_t hint;  // colour proposed by a lattice factory (schedule.cpp verifies it), kNoColourHint otherwise
};
struct HostTet {  // TetrahedralConstraint and VolumeConstraint share the rest data
  uint32_t ids[4];
  float qinv[9];  // column-major (glm layout): qinv[3*col + row]
  float lo, hi;   // minStrain/maxStrain or minOmega/maxOmega
  float w;
  float AtA[16];  // row-major 4x4, A^T A (B = I so AtB = A^T)
  float A[16];    // row-major 4x4
  uint16_t hint;  // see HostDistance
  // colours proposed for schedule LAYERED when the breadth-first levels are lattice layers perpendicular to x, y or z
  // (layer_plan.cpp verifies a proposal group by group)
  uint16_t layerHint[3] = {kNoColourHint, kNoColourHint, kNoColourHint};
};
struct HostBend {
  uint32_t ids[4];
  float angle;
  float w;
};
struct HostNodePair {  // CollisionConstraint (Src/CollisionConstraint.cpp:7-65): an extension container, pies_add_node_pair_constraints
  uint32_t ids[2];
};

struct HostShape {  // ShapeMatchingConstraint (Src/ShapeMatchingConstraint.cpp:6-48)
  std::vector<uint32_t> ids;
  std::vector<double> mat;  // 3 x n material coordinates, centred (column i at mat[3i..])
  double Qinv[9];           // row-major
  float w;
};
struct HostGoal {  // GoalMatchingConstraint (Src/ShapeMatchingConstraint.cpp:124-137)
  std::vector<uint32_t> ids;
  std::vector<float> mat;  // 3 x n world positions at creation
  float transform[16];     // column-major mat4
  float w;
};
// An embedded surface mesh (pies_add_skin, skin.cpp): every vertex bound to one tetrahedron.  Node ids are HOST ids, always (the
// InternalNumbering scope of pies_finalize leaves skins alone; skin_upload translates through nodeOrder.inv).
struct HostSkin {
  std::vector<uint32_t> tet;     // per vertex: index into the tetrahedra the host listed
  std::vector<uint32_t> ids;     // 4 per vertex
  std::vector<float> w;          // 4 per vertex: w0 = 1 - (w1 + w2 + w3), w1, w2, w3
  std::vector<uint32_t> tris;    // 3 per triangle, indices into this skin's vertices
  std::vector<uint32_t> incPtr;  // vertex -> triangles that name it, CSR, ascending triangle index per vertex
  std::vector<uint32_t> inc;
  uint32_t vertexCount() const { return static_cast<uint32_t>(tet.size()); }
};
struct HostFixedRegion {  // Solver::FixedRegion (Include/Pies/Solver.h:147-151)
  float invInitialTransform[16];
  uint32_t goal;
};

struct Batch {
  uint32_t start, count;
};

// Execution plan of one constraint container: slot -> host index, and conflict-free batches of slots.
struct Plan {
  std::vector<uint32_t> order;
  std::vector<Batch> batches;
};

// Whole-substep dependency levels of schedule EXACT (wavefront.cpp)
constexpr uint64_t kWaveMaxOps = 1ull << 27;  // 512 MB of level indices: beyond this the per-sweep levels are used
struct WavePlan {
  bool active = false;
  std::vector<WaveLevel> levels;
  std::vector<uint32_t> index;         // items of every level, kind after kind
  std::vector<uint32_t> barrierAfter;  // with node-node collisions: the collision pass of iteration i runs after this many levels
};

// Schedule LAYERED (layer_plan.cpp): breadth-first levels of the constraint graph.  A constraint's nodes lie in
// two adjacent levels, so the constraints whose lowest level is l ("group l") touch levels l and l+1 only and
// groups of equal parity are independent: one workgroup sweeps one group with its nodes resident in LDS, colour
// after colour (a colouring inside the group), and a container's sweep is two launches (even groups, odd groups).
struct LayerTile {  // the nodes a workgroup keeps in LDS: two runs of the level-ordered node list (one per level)
  uint32_t first0, count0, first1, count1;
};
struct LayerKind {
  uint32_t ncol[4] = {0, 0, 0, 0};   // colours per tile in each phase (padded to the phase's maximum; 0 = phase unused)
  std::vector<uint32_t> colOff[4];   // per tile of the phase: ncol+1 absolute slot offsets
  std::vector<uint32_t> local;       // stride x count tile-local node indices (16 bit each), slot order
  uint32_t maxClass = 0;             // largest colour class of any tile
};
// A tile's phase = 2 * (parity of its lowest level) + (parity of its strip).  Order in which a container runs its phases:
// the distance container ends where the tetrahedral one starts and vice versa, so those phases share a launch.
constexpr int kLayerPhaseOrder[5][4] = {{0, 1, 2, 3}, {0, 1, 2, 3}, {3, 2, 1, 0}, {0, 1, 2, 3}, {0, 1, 2, 3}};
constexpr uint32_t kLayerMaxGroupNodes = 7936;  // 20 B per node (record + radius) + the colour offsets in the 160 KB LDS
struct LayerPlan {
  bool active = false;
  uint32_t levels = 0;         // breadth-first levels along the longest axis
  uint32_t strips = 1;         // strips of `width` levels of the second levelling (1: a pair of levels is one tile)
  uint32_t width = 1;
  uint32_t maxGroupNodes = 0;  // nodes of the largest tile
  std::vector<uint32_t> nodeList;     // node ids sorted by (level, second level, id)
  std::vector<LayerTile> tiles[4];    // per phase
  LayerKind kind[5];                  // indexed by PIES_POSITION .. PIES_BEND (PIES_VOLUME unused)
  uint32_t restSets = 0;              // sets of the tetrahedral rest dictionary (layer_rest_dictionary), 0: per-element arrays
};
struct LayerDevice {
  uint32_t* nodeList = nullptr;
  float4* lpos = nullptr;
  float* lrad = nullptr;
  pies::LayerTile* tiles[4] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t* colOff[5][4] = {};
  uint32_t* pc_lid = nullptr;  // 1 x 16 bit in a word
  uint32_t* dc_lid = nullptr;  // a | b << 16
  uint2* tc_lid = nullptr;     // (n1 | n2 << 16, n3 | n4 << 16); with a rest dictionary 13-bit ids + the set index (layer_rest.h)
  float4* restTable = nullptr;  // the rest dictionary: 3 float4 per set (Qinv, min strain, max strain, w), twice (plain, pair order: layer_rest.h), nullptr without
  uint2* bc_lid = nullptr;
};

// In-situ timing of one kernel class (pies_profile_in_situ): whole substeps are launched eagerly and every launch of the
// class is bracketed by two events on the solver's stream.
struct Probe {
  int kernel = -1;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> events;  // begin, end, begin, end, ...
  size_t used = 0;
  bool failed = false;
  void mark() {
    if (used == events.size()) {
      hipEvent_t e = nullptr;
      if (ledger::event_create(&e) != hipSuccess) { failed = true; return; }
      events.push_back(e);
    }
    if (hipEventRecord(events[used++], stream) != hipSuccess) failed = true;
  }
};

// Tiles of the PD strain + volume local step (pd_tiles.cpp; device form: PdTileArrays), fixed strides per tile
struct PdTilePlan {
  std::vector<uint32_t> info;    // per tile: nodes | elements << 16
  std::vector<uint32_t> node;    // kTileNodes per tile: global node index (unused slots repeat the last node)
  std::vector<uint32_t> elem;    // kTileElems per tile: host element index (unused slots repeat the last element)
  std::vector<uint32_t> local;   // kTileElems per tile
  std::vector<uint16_t> nptr;    // kTileNptr per tile
  std::vector<uint16_t> inc;     // 4 * kTileElems per tile
  uint64_t tileNodes = 0;        // sum of the tiles' node counts
};

// Node renumbering of PD scenes (PIES_FLAG_RENUMBER_NODES, node_order.cpp).  Empty: the device holds node h at index h.
// Otherwise the device holds the nodes in the internal numbering: order[k] is the host id of internal node k, inv its inverse.
// The host mirror and every id the host sees stay in host numbering.
struct NodeOrder {
  std::vector<uint32_t> order, inv;
  bool active() const { return !order.empty(); }
};

// A signed distance field (pies_add_field, pies_add_field_tri_mesh): the host copy pies_get_field reads and the device copy is
// staged from.  Sample (i, j, k) at (k * dims[1] + j) * dims[0] + i.
struct HostField {
  uint32_t dims[3];
  float origin[3];
  float cell;
  std::vector<float> samples;
};

// A set of anchors (pies_add_anchors, anchors.cpp): the host copy pies_get_anchors reads, and what the device copy is staged from -
// the anchors sorted by (node, anchor index) as a compact list of the anchored HOST node ids in ascending id, offsets into the
// sorted records and, in every record, its index in the set's own order.
struct HostAnchorSet {
  std::vector<pies_anchor_t> anchors;  // the set's own order
  uint32_t nFrames = 0;
  bool pins = false;                   // some anchor is a pin: a call edits positions and previous positions too
  std::vector<uint32_t> nodes;         // anchored host node ids, ascending, once each
  std::vector<uint32_t> offsets;       // nodes + 1: the node's records are [offsets[a], offsets[a + 1])
  std::vector<AnchorRecord> records;   // sorted (anchor_kernels.h)
};
struct AnchorSetDevice {  // nullptr: not staged
  uint32_t* nodes = nullptr;
  uint32_t* offsets = nullptr;
  AnchorRecord* records = nullptr;
};

// A set of ties (pies_add_ties, ties.cpp): the host copy pies_get_ties and pies_get_tie_state read, and what the device copy is
// staged from - one record per tie in the set's own order with the set's counts, and a CSR from the tied HOST node ids (ascending,
// once each) to their (tie, coefficient) entries in ascending tie index.  `broken` is the truth between calls: a call that may
// break ties reads the device's bytes back into it, and a staging (the first use, after free_device, after pies_reset_ties)
// uploads it.
struct HostTieSet {
  std::vector<pies_tie_t> ties;        // the set's own order
  uint32_t nGroups = 0;
  std::vector<uint8_t> broken;         // per tie
  bool brokenChanged = false;          // pies_reset_ties since the device copy's bytes were written
  std::vector<TieRecord> records;      // (tie_kernels.h)
  std::vector<uint32_t> nodes;         // tied host node ids, ascending, once each
  std::vector<uint32_t> offsets;       // nodes + 1
  std::vector<TieEntry> entries;
};
struct TieSetDevice {  // nullptr: not staged
  TieRecord* records = nullptr;
  uint8_t* broken = nullptr;
  uint32_t* nodes = nullptr;
  uint32_t* offsets = nullptr;
  TieEntry* entries = nullptr;
};

// A set of actuators (pies_add_actuators, actuators.cpp): the host copy pies_get_actuators reads - `base` filled in -, and what the
// device copy is staged from: the records with every host index replaced by its slot in the plan the device holds (built at the
// staging, alive until the next one: the copy is asynchronous).
struct HostActuatorSet {
  std::vector<pies_actuator_t> actuators;  // the set's own order
  uint32_t nChannels = 0;
  uint32_t restBits = 0;                   // bit 0: some actuator drives a distance constraint, bit 1: a bend constraint
  std::vector<ActuatorRecord> staged;
};

// Device buffers of pies_raycast.  free_device drops them, so the triangle list never outlives the scene or the node numbering
// it was built from; every buffer grows on demand and a handle that never casts a ray holds none.
struct RayBuffers {
  std::vector<void*> allocations;
  uint32_t* tri = nullptr;      // the scene's triangles, host order, node ids in DEVICE numbering
  uint32_t nTris = 0;
  bool triBuilt = false;
  float4* records = nullptr;    // wide variant: (a, e1, e2) per triangle of the target last staged
  size_t recordCap = 0;         // triangles
  uint64_t* partial = nullptr;  // one key per (part, ray) of a batch
  size_t partialCap = 0;        // keys
  float* rays = nullptr;        // origins (3 n) then directions (3 n)
  uint32_t* outTri = nullptr;   // results, n rays each
  float *outT = nullptr, *outUv = nullptr;
  size_t rayCap = 0;            // rays
  // pies_closest_points (nearest.cpp) shares tri, records and partial - the winding pass keeps its tile sums in partial - and
  // has the points and results to itself
  float* nearPoints = nullptr;    // 3 n
  uint32_t* nearTri = nullptr;    // results: n, n, 2 n, 3 n, n
  float *nearDistance = nullptr, *nearUv = nullptr, *nearPoint = nullptr, *nearWinding = nullptr;
  size_t nearCap = 0;             // points
  // pies_collide_props (props.cpp) has its buffers to itself; they live here so that free_device drops them with the others
  pies_prop_t* propRecords = nullptr;  // PIES_PROP_MAX records
  float* propOut = nullptr;            // PIES_PROP_MAX x kPropSumWords: the folded sums
  uint64_t* propTileMask = nullptr;    // per tile of 256 host ids: the props that touched it
  size_t propTileCap = 0;              // tiles
  float* propTileSums = nullptr;       // per (tile, prop): kPropSumWords words
  size_t propSumCap = 0;               // (tile, prop) records
  uint32_t* propNodeProp = nullptr;    // per host id: the last prop that touched the node
  size_t propNodeCap = 0;              // nodes
  // pies_collide_field_props (fields.cpp) shares the reaction's buffers above; its records and the device copies of the fields
  // it has met (nullptr: not staged - the host copy in pies_solver::h_fields is staged again at the next use)
  FieldPropRecord* fieldRecords = nullptr;    // PIES_FIELD_PROP_MAX records
  float* fieldSamples[PIES_FIELD_MAX] = {};
  // pies_apply_forces (forces.cpp) shares the reaction's buffers above (propOut, propTileMask, propTileSums); its records, the
  // scratch variant's new velocities and affected lanes, and the wind's node -> triangle incidence over `tri` (ray_build_incidence)
  pies_force_t* forceRecords = nullptr;  // PIES_FORCE_MAX records
  float4* forceVel = nullptr;            // per host id
  uint64_t* forceAffected = nullptr;     // kForceWaves words per tile of 256 host ids
  size_t forceVelCap = 0;                // nodes both hold
  uint32_t* incPtr = nullptr;            // nodes + 1, by host id
  uint32_t* inc = nullptr;               // 3 x nTris triangle indices
  bool incBuilt = false;
  // pies_apply_surface_loads (loads.cpp) shares the reaction's buffers, forceVel / forceAffected and the incidence above; its
  // records, what the fold leaves per load, the tiles of 256 triangles the call's ranges meet and their sums per (slot, load)
  pies_surface_load_t* loadRecords = nullptr;  // PIES_LOAD_MAX records
  void* loadState = nullptr;                   // PIES_LOAD_MAX LoadState records (load_kernels.h)
  uint32_t* loadTiles = nullptr;               // tile indices, ascending
  size_t loadTileCap = 0;                      // slots
  float2* loadTileSums = nullptr;
  size_t loadSumCap = 0;                       // (slot, load) records
  std::vector<uint32_t> loadTilesHost;         // the staging copy of loadTiles: alive until the call has synchronised
  // pies_apply_anchors (anchors.cpp) shares propOut, propTileMask and propTileSums above - its tiles are of 256 ANCHOR indices -;
  // the device copies of the sets it has met (not staged: the host copy in pies_solver::h_anchors is staged again at the next
  // use), the frames of a call and what the second walk leaves per anchor in the set's own order
  AnchorSetDevice anchorSets[PIES_ANCHOR_SET_MAX] = {};
  pies_anchor_frame_t* anchorFrames = nullptr;  // PIES_ANCHOR_FRAME_MAX records
  float4* anchorImpulse = nullptr;              // per anchor: j, stretch
  float4* anchorTorque = nullptr;               // per anchor: cross(t - pivot, j), the frame's index | the live bit
  size_t anchorOutCap = 0;                      // anchors both hold
  // pies_apply_ties (ties.cpp) shares propOut, propTileMask and propTileSums too - tiles of 256 TIE indices -; the device copies
  // of its sets, the groups of a call and, per tie, what the iterations pass on (tie_kernels.h: TiePass)
  TieSetDevice tieSets[PIES_TIE_SET_MAX] = {};
  pies_tie_group_t* tieGroups = nullptr;        // PIES_TIE_GROUP_MAX records
  float4* tieDelta = nullptr;
  float4* tieImpulse = nullptr;
  float4* tieTorque = nullptr;
  float4* tieScratch = nullptr;                 // 2 per tie
  size_t tieCap = 0;                            // ties all four hold
  // pies_drive_actuators (actuators.cpp) has its buffers to itself: the device copies of its sets (nullptr: not staged - the slots
  // are those of the plan this scene was built with), the activations and the folded outputs of a host-pointer call, one entry per
  // actuator and the tile records
  ActuatorRecord* actuatorSets[PIES_ACTUATOR_SET_MAX] = {};
  float* actuatorActivation = nullptr;          // PIES_ACTUATOR_CHANNEL_MAX words
  float* actuatorSums = nullptr;                // PIES_ACTUATOR_CHANNEL_MAX x 2
  uint32_t* actuatorLive = nullptr;             // PIES_ACTUATOR_CHANNEL_MAX
  float2* actuatorOut = nullptr;                // per actuator: (rest, value)
  size_t actuatorOutCap = 0;                    // actuators
  uint32_t* actuatorTileRecords = nullptr;      // per (tile, channel): kActuatorTileWords words
  size_t actuatorTileCap = 0;                   // (tile, channel) records
  // pies_measure_elements / pies_measure_nodes (measure.cpp) have their buffers to themselves.  Per container (0: PIES_TET, 1:
  // PIES_VOLUME) the elements staged in HOST order with node ids in DEVICE numbering, upload_tets' layout - the scene's own
  // tetrahedral records are in plan order and PBD stages no volume records
  uint4* measureIds[2] = {nullptr, nullptr};
  float4* measureQ[2][3] = {};
  bool measureStaged[2] = {false, false};
  pies_element_measure_t* measureOut = nullptr;  // the records of a call
  size_t measureOutCap = 0;                      // elements
  uint32_t* measureTileRecords = nullptr;        // per tile of 256 element indices: kMeasureTileWords words
  size_t measureTileCap = 0;                     // tiles
  uint32_t* measureSummary = nullptr;            // kMeasureTileWords words: the folded summary
  MeasureRange* measureRanges = nullptr;         // PIES_MEASURE_RANGE_MAX records
  float* measureNodeOut = nullptr;               // PIES_MEASURE_RANGE_MAX x kNodeSumWords: the folded sums
  float* measureNodeTileSums = nullptr;          // per (tile of 256 host ids, range): kNodeSumWords words
  size_t measureNodeTileCap = 0;                 // (tile, range) records
};

// What one pies_finalize builds in HBM for the scene as it stands.  free_device frees `allocations` and puts a fresh DeviceScene in
// its place, so a field added here needs no line of its own there.  Buffers that outlive a finalize (the pinned stages, the export
// buffers, the skins' records) and the adapted counts (pcgBudget, pairRounds, sortPasses, ncRounds) are members of pies_solver.
struct DeviceScene {
  std::vector<void*> allocations;  // every buffer below, in the order it was allocated
  NodeArrays nd{nullptr, nullptr, nullptr, nullptr, 0};
  float* d_pack = nullptr;         // n x 3: a node array's x, y, z packed for the read-back
  uint32_t* d_nodeInv = nullptr;   // HBM copy of nodeOrder.inv (nullptr: identity)
  // constraint records, in plan order
  uint32_t* d_pc_id = nullptr;
  float4* d_pc_tw = nullptr;
  uint2* d_dc_ids = nullptr;
  float2* d_dc_rw = nullptr;
  uint4* d_tc_ids = nullptr;
  float4 *d_tc_q0 = nullptr, *d_tc_q1 = nullptr, *d_tc_q2 = nullptr;
  uint4* d_bc_ids = nullptr;
  float2* d_bc_aw = nullptr;
  uint2* d_np_ids = nullptr;       // node-pair extension (PD)
  uint32_t* d_np_bits = nullptr;   // bitmap over the nodes (device numbering): in a listed pair (floor friction after the pairs' friction)
  uint32_t* d_np_nodes = nullptr;  // those nodes, ascending, once each
  uint32_t npNodes = 0;
  uint4* d_vc_ids = nullptr;       // volume constraints (PD only), host order
  float4 *d_vc_q0 = nullptr, *d_vc_q1 = nullptr, *d_vc_q2 = nullptr;
  uint32_t* d_waveIndex = nullptr;  // schedule EXACT, PBD: the items of WavePlan's levels
  LayerDevice d_layer{};            // schedule LAYERED, PBD
  HashArrays hash{};                // node grid: node-node collisions (PBD), node-node contacts (PD)
  PairArrays pairs{};               // pair-ordered resolve (PBD)
  NodeContactArrays nc{};           // node-node contacts of PD (PIES_FLAG_PD_NODE_CONTACTS)
  bool ncActive = false;            // ... built by the last pies_finalize (a PD scene with nodes)
  PdArrays pd{};                    // Projective Dynamics
  uint16_t* d_pairDictIndex = nullptr;  // PD, paired elements: index of the element's set of constants (rest dictionary), or nullptr
  float4* d_pairDictTable = nullptr;
  uint32_t pairDictSets = 0;
  uint32_t pdRowStencils = 0;       // PD: distinct rows of the system matrix in its row dictionary (0: none)
  // PD: input of a substep, kept until its solves are known to have met the tolerance (pies_tick runs it again otherwise)
  float4 *snapPos = nullptr, *snapPrev = nullptr, *snapVel = nullptr;
  double* snapQuat = nullptr;
};

}  // namespace pies

struct pies_solver {
  pies_options_t opt;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t sideStream = nullptr;  // second branch of the PD substep: the dependency levels of the contact list (needed only by the
                                     // sequential passes at the end of the substep) are computed beside the local/global iterations
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  bool triLevelsForked = true;
  bool pdLocalPacked = true;    // strain + volume local step two elements per lane in packed fp32 (PIES_PD_LOCAL_PACKED=0: one per lane)
  bool pdSingleCg = true;       // the global step's CG with one launch per iteration where it applies (PIES_PD_CG_SINGLE=0: the two-launch form everywhere)
  bool pdSingleCgRows = true;   // ... also in the contact-heavy graph variant (merged contact rows gathered inline)
  bool pdFuseRhs = true;        // its residual kernel evaluates the right-hand side when a node's records are tile sums (PIES_PD_FUSE_RHS=0: k_pd_rhs)
  bool pcgOverflow = true;      // a solve above the tolerance after its captured iterations goes on inside the last launch (PIES_PCG_OVERFLOW=0: off)
  bool pcgPinned = false;       // PIES_PCG_BUDGET
  uint32_t pcgPinnedBudget = 32;
  uint32_t asyncSinceSync = 0;  // PD ticks queued by pies_tick_async since the last host synchronisation
  std::string error;

  bool releaseHinge = false;
  bool nodeCollisions = true;
  bool collideFast = true;         // every node's cell range spans at most 2 cells per axis: the parallel visiting order may run
  std::vector<uint16_t> h_pairDictIndex;  // host copy (the tile plan stores it in tile order)
  uint32_t pdTileRecords = 0;            // sum of the tiles' node counts
  uint32_t pdTiles = 0;                  // PD: tiles of the strain + volume local step (0: per-(element, node) records)
  float pdWindowPadding = 0.0f;         // PD: stored / real entries of the windowed matrix (0: not built)
  uint32_t pdWindowEntries = 0;         // its stored entries
  uint32_t pdWindowHalo = 0;            // its halo entries over all chunks
  bool tetVolumePaired = false;    // PD: h_volume[k] and h_tet[k] are the same element for every k (fused local step)
  bool triangleCollisions = true;  // PD point-triangle CCD contacts (Solver.cpp:693-797); extension flag to switch off
  bool renumberNodes = false;      // PIES_FLAG_RENUMBER_NODES: pies_finalize may renumber the nodes of a PD scene (node_order.cpp)
  bool pdNodeContacts = false;     // PIES_FLAG_PD_NODE_CONTACTS: PD detects node-node contacts on the device every substep
  pies::NodeOrder nodeOrder;       // the numbering the device holds (decided by the last pies_finalize)
  bool internalIds = false;        // the host containers hold the internal numbering (inside an InternalNumbering scope)
  bool simFailed = false;
  int schedule = PIES_SCHEDULE_DEFAULT;
  int collisionOrderFlag = -1;     // PIES_FLAG_COLLISION_ORDER: -1 follows the schedule (EXACT: reference order, otherwise pair order)
  uint32_t sortPasses = 3;         // radix passes captured per node-grid build (up to 11 key bits each); follows the scene's cell box
  uint32_t sortCalm = 0;
  bool pairRoundsPinned = false;   // pies_set_collision_rounds: the count is the host's
  uint32_t pairCalm = 0;           // synchronisations in a row at which fewer level launches would have done
  uint32_t pairRounds = 96;        // level launches captured per pair-ordered pass (a tail kernel finishes deeper orders)

  // ---- host mirror ----
  std::vector<float> h_pos, h_prev, h_vel;  // n x 3
  std::vector<float> h_radius, h_invMass;   // n
  std::vector<pies::HostPosition> h_position;
  std::vector<pies::HostDistance> h_distance;
  std::vector<pies::HostTet> h_tet, h_volume;
  std::vector<pies::HostBend> h_bend;
  std::vector<pies::HostNodePair> h_nodePair;  // extension container (PD): pies_add_node_pair_constraints
  std::vector<pies::HostShape> h_shape;
  std::vector<pies::HostGoal> h_goal;
  std::vector<pies::HostFixedRegion> h_fixedRegions;
  bool goalDirty = false;  // a goal transform changed: refresh its projected positions in HBM
  std::vector<uint32_t> h_triangles;  // 3 per triangle
  std::vector<uint32_t> h_lines;
  std::vector<pies::HostSkin> h_skins;  // extension: embedded surface meshes (pies_add_skin)
  std::vector<pies::HostField> h_fields;  // extension: signed distance fields (pies_add_field*); assets: only pies_clear drops them
  std::vector<pies::HostAnchorSet> h_anchors;  // extension: anchor sets (pies_add_anchors); assets like the fields
  std::vector<pies::HostTieSet> h_ties;        // extension: tie sets (pies_add_ties); assets like the anchor sets
  std::vector<pies::HostActuatorSet> h_actuators;  // extension: actuator sets (pies_add_actuators); assets like the anchor sets
  uint32_t constraintId = 0;

  bool sceneDirty = true;    // topology/rest data changed: rebuild plans + upload everything
  // which host mirror arrays are older than the device's (bit 0 positions, 1 previous positions, 2 velocities):
  // a read of one array copies that array only, through the pinned staging buffer
  uint32_t stale = 0;
  // which rest data of the host mirror is older than the device's (bit 0: h_distance[].target, bit 1: h_bend[].angle) - a
  // pies_drive_actuators wrote HBM; download_rest copies the records back through the plan's order before anyone reads them
  uint32_t restStale = 0;
  bool graphDirty = false;   // only the launch sequence changed (releaseHinge, CG budget): re-capture, no re-upload
  bool hostNodesDirty = false;  // host node state edited (pies_write_nodes): upload nodes only

  // ---- plans ----
  pies::Plan plan[5];  // PIES_POSITION .. PIES_BEND
  pies::WavePlan wave;  // schedule EXACT, PBD: levels of the whole-substep DAG
  pies::LayerPlan layer;  // schedule LAYERED, PBD

  // ---- HBM: everything the last pies_finalize built (device_scene.cpp) ----
  pies::DeviceScene dev;
  uint32_t ncRounds = 8;     // PD node-node contacts: friction round launches captured per substep (adapt_nc_rounds follows the passes)
  uint32_t ncCalm = 0;       // synchronisations in a row at which fewer would have done

  // ---- Projective Dynamics ----
  uint32_t slotBase[6] = {0, 0, 0, 0, 0, 0};  // first contribution slot of each container (5: the node-pair extension)
  uint32_t pd_nnz = 0;
  uint32_t goalSlotBase = 0;  // first fp64 contribution slot of the goal constraints
  float pcgTol = 3.0e-7f;     // relative residual ||r|| / ||b|| per coordinate column
  uint32_t pcgMaxIters = 128; // upper bound of CG iterations per global step (thousands of w = 1e4 contacts need 40+)
  bool pcgCeilingSet = false; // pies_set_pcg was called: pies_finalize leaves pcgMaxIters alone (else 256 with PD node-node contacts)
  uint32_t pcgBudget = 32;    // iterations currently captured in the graph (adapted to what the solves use)
  uint32_t pcgCalm = 0;       // synchronisations in the current observation window (all solves converged)
  uint32_t pcgWindowMax = 0;  // most CG iterations any solve used in that window
  uint32_t pcgRecent[3] = {0, 0, 0};  // ... and at the last three synchronisations
  bool triFastRows = false;     // PD graph variant: contact rows of the SpMV summed by k_contact_rows (many contacts)
  uint32_t triQuiet = 0;        // synchronisations without a contact while that variant is active
  uint32_t pcgCooldown = 0;   // synchronisations left before the budget may shrink again after a solve ran out
  float4* h_stage = nullptr;  // pinned staging for the per-tick position read-back
  size_t h_stage_n = 0;
  // ---- render-state export (Solver.h:42-71): frame k is copied out while frame k+1 computes ----
  hipStream_t copyStream = nullptr;
  hipEvent_t evTick[2] = {nullptr, nullptr};    // frame's positions are in d_export
  hipEvent_t evCopied[2] = {nullptr, nullptr};  // frame's positions are in h_export[frame & 1]
  float4* h_export[2] = {nullptr, nullptr};     // pinned
  size_t h_export_n = 0;
  float4* d_export = nullptr;
  uint64_t frameBegun = 0;      // frames begun so far (frame ids start at 1)
  uint64_t frameAcquired = 0;   // frame the host currently holds (0: none)
  // ---- device-side node and skin access (node_io.cpp): the caller's stream and the solver's wait for each other ----
  hipEvent_t evIoIn = nullptr, evIoOut = nullptr;  // created at the first call: caller's work so far; the call's launches
  // ---- skins: device records of h_skins (built by skin_upload at pies_finalize / before the next use), outputs, export ----
  pies::SkinArrays skin{};
  bool skinDirty = false;            // h_skins and the device records differ
  std::vector<void*> skinAllocations;
  std::vector<uint32_t> skinFirst;   // first vertex of every skin in the concatenated arrays, + the total
  float* d_skinOut = nullptr;        // pies_read_skin: positions (3 x nVerts) then normals (3 x nVerts)
  float* h_skinStage = nullptr;      // pinned, same layout
  size_t h_skinStage_n = 0;          // vertices it holds
  float* d_skinExport = nullptr;     // pies_tick_begin: same layout, one frame
  float* h_skinExport[2] = {nullptr, nullptr};  // pinned, per frame parity
  size_t skinExport_n = 0;           // vertices the three export buffers hold
  uint32_t frameSkinVerts[2] = {0, 0};  // skin vertices frame (parity) carries
  // ---- ray casts (pies_raycast, raycast.cpp): built at the first call, freed with the scene's buffers (free_device) ----
  pies::RayBuffers ray{};
  // ---- PD: a substep whose solve ends above the tolerance is run again with a larger CG budget (pies_tick) ----
  bool pcgRetry = true;
  uint32_t pcgRetries = 0;         // substeps run again since the handle was created
  uint64_t pcgShortSolves = 0;     // solves left above the tolerance (budget at its ceiling, or asynchronous ticks)

  hipGraph_t graph = nullptr;
  hipGraphExec_t graphExec = nullptr;
  // PD: the substep graph exists once per (captured CG iterations, contact-row variant) - a ladder of budgets 2, 4, 8, ... up
  // to the ceiling of pies_set_pcg, instantiated together - so that following the solves means launching another executable
  // graph, not capturing and instantiating one in the middle of a frame (~11 ms).  graph / graphExec then alias an entry.
  struct PdGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; uint32_t counts[32] = {0}; };
  std::map<uint64_t, PdGraph> pdLadder;
  bool graphFromLadder = false;
  uint32_t launchCounts[PIES_KERNEL_COUNT] = {};
  pies::Probe* probe = nullptr;  // set for the duration of pies_profile_in_situ
  float lastWindingMs = -1.0f;   // diagnostic build only (tools/probe_trimesh.py): this handle's last k_winding launch between two events

  uint32_t nodeCount() const { return static_cast<uint32_t>(h_radius.size()); }
};

namespace pies {
// scene.cpp
int fail(pies_solver* s, int code, const std::string& msg);
// schedule.cpp : op = up to 4 node ids; bit i of writeMask set if node i is written.
struct OpView {
  const uint32_t* ids;  // count * stride entries
  uint32_t stride;      // node ids per op
  uint32_t count;
  uint8_t writeMask;    // same for every op of a container
  const uint16_t* hint = nullptr;  // optional proposed colouring (count entries)
};
void build_plan(const OpView& ops, uint32_t nodeCount, int schedule, Plan& out);
bool build_wave_plan(const pies_solver* s, WavePlan& out);
// layer_plan.cpp : fills s->layer and the four PBD plans; false (nothing changed) when the scene does not suit it
bool build_layer_plan(pies_solver* s);

// skin.cpp : device records of the skins (no-ops without skins); skin_free_device forgets them (free_device, pies_clear)
int skin_upload(pies_solver* s);
void skin_free_device(pies_solver* s);
// raycast.cpp : forgets the buffers of pies_raycast, pies_closest_points, pies_collide_props and pies_collide_field_props, the
// fields' device copies included (free_device)
void ray_free_device(pies_solver* s);
// raycast.cpp, shared with nearest.cpp : replaces a buffer of s->ray (ray_free_device frees it); the triangles of a checked
// (target, skin) of pies_raycast at the positions the device holds, a skin's vertices evaluated on the stream first
int ray_grow_bytes(pies_solver* s, size_t bytes, void** d);
template <class T> int ray_grow(pies_solver* s, size_t count, T** d) {
  void* p = *d;
  const int rc = ray_grow_bytes(s, count * sizeof(T), &p);
  *d = static_cast<T*>(p);
  return rc;
}
// ... when its capacity *cap (in items of `each` elements) is below count; the capacity is 0 while the buffer is being replaced
template <class T> int ray_reserve(pies_solver* s, size_t count, T** d, size_t* cap, size_t each = 1) {
  if (*cap >= count) return PIES_OK;
  *cap = 0;
  if (int rc = ray_grow(s, count * each, d)) return rc;
  *cap = count;
  return PIES_OK;
}
int ray_open_target(pies_solver* s, int target, uint32_t skin, pies::RayTarget* out);
// raycast.cpp, for forces.cpp : the node -> triangle incidence of the scene's triangles in s->ray (built once per pies_finalize)
int ray_build_incidence(pies_solver* s);
// nearest.cpp, shared with fields.cpp : the distance and winding launches of pies_closest_points for n points in HBM (each output
// may be nullptr); no synchronisation
int near_launch(pies_solver* s, const pies::RayTarget& T, const float* dPoints, uint32_t n, float maxDistance, uint32_t* dTri,
                float* dDistance, float* dUv, float* dPoint, float* dWinding);
// props.cpp, shared with fields.cpp and forces.cpp : the reaction's buffers of s->ray for n nodes and nProps props, filled into P;
// then, after the collide launch, the fold, the stale marks (staleBits: what the launch edited), the copies out, the synchronisation
int prop_open_pass(pies_solver* s, uint32_t nProps, bool reaction, bool nodeProp, pies::PropPass* P);
int prop_close_pass(pies_solver* s, const pies::PropPass& P, float* outImpulse, float* outTorque, uint32_t* outHits, uint32_t* outNodeProp,
                    uint32_t staleBits = 7u);
// props.cpp : what every between-tick edit of node state (props.cpp, fields.cpp, forces.cpp, loads.cpp) does before its own work,
// in this order: the list is not NULL and has at most max (maxName) records, no record has a fault (fault(k): nullptr, or what is
// wrong with record k), dt (when given) is finite and >= 0; an empty list returns - nodeProp, when given, filled with
// PIES_PROP_NONE -; the handle has a device and HBM holds the scene; in a scene without nodes, or `idle` (it lacks what else the
// records act on), the call waits for the queued work and zeroes its outputs.  Returns kEditGo when the caller has work to do,
// else what the entry point returns.  Nothing is formatted or allocated on the way to kEditGo.
struct EditNames {
  const char *call, *noun, *subject;  // the entry point; a record in messages ("prop"); what meets the nodes ("field props")
  uint32_t max;
  const char* maxName;
};
struct EditOutputs {  // each may be nullptr
  float *impulse, *torque;  // 3 per record
  uint32_t* counts;         // 1 per record
  uint32_t* nodeProp = nullptr;                // 1 per node
  float *volume = nullptr, *area = nullptr;    // 1 per record
};
constexpr int kEditGo = -1;
// (the part after the records' own checks: record `bad` has the fault `what`, or what == nullptr)
int edit_prelude_checked(pies_solver* s, const EditNames& names, uint32_t count, const void* records, uint32_t bad, const char* what,
                         const float* dt, bool idle, const EditOutputs& out);
template <class Fault>
int edit_prelude(pies_solver* s, const EditNames& names, uint32_t count, const void* records, Fault&& fault, const float* dt, bool idle,
                 const EditOutputs& out) {
  uint32_t bad = 0;
  const char* what = nullptr;
  if (records && count <= names.max)  // (else the list itself is refused first)
    for (; bad < count && !(what = fault(bad)); ++bad) {}
  return edit_prelude_checked(s, names, count, records, bad, what, dt, idle, out);
}
// ... `*scratch = true` when the tuning variable says "scratch"; "inplace" leaves the choice to the list, anything else is an error
int edit_variant(pies_solver* s, const char* variable, const char* call, bool* scratch);
// ... the scratch variant's arrays of s->ray for the scene's nodes (forces and loads share them: one call runs at a time)
int edit_velocity_scratch(pies_solver* s, pies::VelocityScratch* out);
// node_order.cpp : decides s->nodeOrder for the scene as it stands (host logic of pies_finalize, device handles and host-only ones)
void decide_node_order(pies_solver* s);
// For its lifetime the host containers of `s` (node arrays, constraint ids, groups, triangles) hold the internal numbering of
// s->nodeOrder; the host numbering is put back on destruction.  Does nothing when the identity is in effect.
class InternalNumbering {
 public:
  explicit InternalNumbering(pies_solver* s);
  ~InternalNumbering();
  InternalNumbering(const InternalNumbering&) = delete;
  InternalNumbering& operator=(const InternalNumbering&) = delete;

 private:
  pies_solver* s_ = nullptr;
  std::vector<float> pos_, prev_, vel_, radius_, invMass_;
  std::vector<HostPosition> position_;
  std::vector<HostDistance> distance_;
  std::vector<HostTet> tet_, volume_;
  std::vector<HostBend> bend_;
  std::vector<HostNodePair> nodePair_;
  std::vector<HostShape> shape_;
  std::vector<HostGoal> goal_;
  std::vector<uint32_t> triangles_, lines_;
};
}  // namespace pies

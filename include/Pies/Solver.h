// Pies::Solver -- drop-in for the reference's public class (Include/Pies/Solver.h:21-116), implemented on
// the MI355X through the C ABI in pies_hip.h (link libpies_hip.so).  Same names, signatures, defaults and
// ownership rules; hosts (PiesForAlthea / PiesForMaya) recompile against this header.
//
//   Pies::SolverOptions opt; opt.solver = Pies::SolverName::PBD;
//   Pies::Solver solver(opt);
//   solver.createTetBox({0, 5, 0}, 1.0f, {0, 0, 0}, 0.05f, 1.0f, false);
//   solver.tick(dt);                       // positions are current in getVertices() when this returns
//
// Differences from the reference, all documented in DESIGN.md: tick() runs on the GPU; getters return
// host mirrors refreshed once per tick (Solver.cpp:157,393 refresh per substep, which nothing can observe);
// addTriMeshVolume works without tetgen (not part of this build): the cells of a lattice that lie inside the surface become
// tetrahedra - a lattice body with a staircase collision surface - and the input mesh is carried along as a skin
// (lastTriMeshSkin), not as the first nodes of a conforming mesh; addTetMeshVolume takes tetgen's output arrays, or just
// elements, for hosts that mesh offline; errors surface as std::runtime_error carrying pies_last_error().
// Shape/goal matching (regions, createShapeMatching*) are Projective-Dynamics constraints, as in the reference.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../pies_hip.h"
#include "Node.h"
#include "Tetrahedron.h"
#include "Triangle.h"
#include "glm_compat.h"

namespace Pies {
enum class SolverName { PBD, PD };  // Solver.h:21

struct SolverOptions {  // Solver.h:23-38, field for field
  float fixedTimestepSize = 0.012f;
  uint32_t timeSubsteps = 1;
  uint32_t iterations = 4;
  uint32_t collisionStabilizationIterations = 4;
  float collisionThresholdDistance = 0.1f;
  float collisionThickness = 0.05f;
  float gravity = 10.0f;
  float damping = 0.006f;
  float friction = 0.01f;
  float staticFrictionThreshold = 0.f;
  float floorHeight = 0.0f;
  float gridSpacing = 2.0f;
  uint32_t threadCount = 8;
  SolverName solver = SolverName::PD;
};
static_assert(sizeof(SolverOptions) == sizeof(pies_options_t), "SolverOptions must mirror pies_options_t");

class Solver {
public:
  struct Vertex {  // Solver.h:42-49: consumed directly as a vertex/instance stream by the renderers
    glm::vec3 position{};
    float radius{};
    glm::vec3 baseColor{};
    float roughness{};
    float metallic{};
  };

  bool renderStateDirty = true;
  bool releaseHinge = false;
  // extensions (not in the reference): which device schedule maps the Gauss-Seidel sweeps, and whether the
  // PBD node-node pass runs (the reference always runs it).  PIES_SCHEDULE_EXACT sweeps the containers in the order
  // the constraints were added and the colliding nodes in ascending index - the reference's order, bit for bit the
  // sequential loop; the default (PIES_SCHEDULE_DEFAULT = LAYERED) is the fast one bench.py reports, a sweep over the
  // same constraints in another order (pies_hip.h; DESIGN.md section 3 states how far apart the results are).
  // -1 (default) leaves the handle's own choice alone: PIES_SCHEDULE_DEFAULT, or what PIES_SCHEDULE=exact|coloured|layered
  // in the environment selected when the handle was opened.
  int schedule = -1;
  bool nodeCollisions = true;       // PBD node-node pass (Solver.cpp:81-130)
  bool triangleCollisions = true;   // PD point-triangle contacts (Solver.cpp:693-797)
  bool renumberNodes = false;       // extension: PD may keep the nodes in a space-filling-curve order on the device
                                    // (PIES_FLAG_RENUMBER_NODES); getVertices() and every id stay the host's
  bool pdNodeContacts = false;      // extension: PD detects node-node contacts every substep (PIES_FLAG_PD_NODE_CONTACTS)
  uint32_t triMeshResolution = 16;  // extension: lattice cells along the longest axis of an addTriMeshVolume body
  uint32_t lastTriMeshSkin = 0;     // extension: the skin id of the last addTriMeshVolume body (getSkinVertices / getSkinNormals)

  // Like the reference's (Solver.h:54-55: `Solver() = default`, a converting constructor from the options): constructing a
  // Solver touches no device.  The device handle is opened by the first call that needs it (add*/create*/tick), which is
  // where a missing gfx950 device surfaces (std::runtime_error; there is no CPU fallback).
  Solver() = default;
  Solver(const SolverOptions& options, int device = 0) : _options(options), _device(device) {}
  Solver(Solver&& rhs) noexcept { *this = std::move(rhs); }
  Solver& operator=(Solver&& rhs) noexcept {
    if (this != &rhs) {
      if (_h) pies_destroy(_h);
      _h = rhs._h;
      rhs._h = nullptr;
      _options = rhs._options;
      _device = rhs._device;
      for (int k = 0; k < 7; ++k) _pushed[k] = rhs._pushed[k];
      _vertices = std::move(rhs._vertices);
      _lines = std::move(rhs._lines);
      _triangles = std::move(rhs._triangles);
      _skinVertices = std::move(rhs._skinVertices);
      _skinNormals = std::move(rhs._skinNormals);
      _frames[0] = rhs._frames[0];
      _frames[1] = rhs._frames[1];
      renderStateDirty = rhs.renderStateDirty;
      releaseHinge = rhs.releaseHinge;
      schedule = rhs.schedule;
      nodeCollisions = rhs.nodeCollisions;
      triangleCollisions = rhs.triangleCollisions;
      renumberNodes = rhs.renumberNodes;
      pdNodeContacts = rhs.pdNodeContacts;
      triMeshResolution = rhs.triMeshResolution;
      lastTriMeshSkin = rhs.lastTriMeshSkin;
    }
    return *this;
  }
  Solver(const Solver&) = delete;
  Solver& operator=(const Solver&) = delete;
  ~Solver() {
    if (_h) pies_destroy(_h);
  }

  // Solver.cpp:25-38.  The argument is ignored like in the reference (the step is fixedTimestepSize).
  void tick(float /*deltaTime*/) { _tickAs(_options.solver); }
  // Solver.cpp:40, :162: the reference's tickPBD / tickPD run the NAMED solver whatever SolverOptions::solver says.  So do
  // these: the handle is switched to that solver (pies_set_solver: the device buffers are rebuilt on the next tick if it
  // differs from the one the last tick ran) and stays there until another tick* asks for the other one.
  void tickPBD(float /*deltaTime*/) { _tickAs(SolverName::PBD); }
  void tickPD(float /*deltaTime*/) { _tickAs(SolverName::PD); }
  // tick() in two halves, so that a host can do its own work (or begin the next tick) while this one's positions travel:
  // beginTick queues the substeps and the asynchronous copy of their result, endTick waits for that copy and refreshes
  // getVertices().  At most two ticks may be begun before the first is ended (pies_tick_begin in pies_hip.h).
  void beginTick() {
    _pushState(_options.solver);
    uint64_t f = 0;
    _ck(pies_tick_begin(_handle(), &f));
    if (_frames[0] == 0) _frames[0] = f; else _frames[1] = f;
  }
  void endTick() {
    if (_frames[0] == 0) return;
    const uint64_t f = _frames[0];
    _frames[0] = _frames[1];
    _frames[1] = 0;
    const float* p = nullptr;
    uint32_t n = 0;
    _ck(pies_export_acquire(_handle(), f, &p, &n));
    const size_t m = n < _vertices.size() ? n : _vertices.size();
    for (size_t i = 0; i < m; ++i) _vertices[i].position = glm::vec3(p[4 * i], p[4 * i + 1], p[4 * i + 2]);
    for (uint32_t k = 0; k < _skinVertices.size(); ++k) {  // the frame's skins, from its pinned buffers
      const float *x = nullptr, *nr = nullptr;
      uint32_t nv = 0;
      _ck(pies_export_acquire_skin(_handle(), f, k, &x, &nr, &nv));
      _copySkin(k, x, nr, nv);
    }
    _ck(pies_export_release(_handle(), f));
  }

  const std::vector<Vertex>& getVertices() const { return _vertices; }
  const std::vector<uint32_t>& getLines() const { return _lines; }
  const std::vector<Triangle>& getTriangles() const { return _triangles; }
  const SolverOptions& getOptions() const { return _options; }
  // extension (see addSkin): deformed vertices and vertex normals of skin `skin`, refreshed by tick* / endTick like getVertices()
  const std::vector<glm::vec3>& getSkinVertices(uint32_t skin) const { return _skinVertices.at(skin); }
  const std::vector<glm::vec3>& getSkinNormals(uint32_t skin) const { return _skinNormals.at(skin); }

  void clear() {
    if (_h) _ck(pies_clear(_h));
    _skinVertices.clear();
    _skinNormals.clear();
    _vertices.clear();
    _lines.clear();
    _triangles.clear();
    renderStateDirty = true;
  }

  // ---- importing meshes (PrimitiveUtilities.cpp:42-328) ----
  void addNodes(const std::vector<glm::vec3>& vertices) {
    std::vector<float> p = _flatten(vertices);
    _ck(pies_add_nodes(_handle(), static_cast<uint32_t>(vertices.size()), p.data(), nullptr));
    _syncRenderState();
  }
  // PrimitiveUtilities.cpp:164-328 without tetgen (pies_add_tri_mesh_volume in pies_hip.h states the rules): the closed surface
  // `vertices` / `indices` (three per triangle) is laid over a lattice of `triMeshResolution` cells along its longest axis; the
  // cells whose centre lies inside (winding numbers, evaluated on the device) or that hold an input vertex become six tetrahedra
  // each, with mass = density per node and one strain and one volume constraint per element when the respective stiffness is not
  // 0.  The result is a LATTICE body: getTriangles() gains its staircase boundary, and the input mesh itself is bound to the
  // elements as a skin - getSkinVertices(lastTriMeshSkin) / getSkinNormals(lastTriMeshSkin) follow the body every tick.  It is
  // not tetgen's conforming mesh, where the input vertices are the first nodes.
  void addTriMeshVolume(const std::vector<glm::vec3>& vertices, const std::vector<uint32_t>& indices, const glm::vec3& initialVelocity,
                        float density, float strainStiffness, float minStrain, float maxStrain, float volumeStiffness, float compression,
                        float stretching) {
    std::vector<float> p = _flatten(vertices);
    const float v[3] = {initialVelocity[0], initialVelocity[1], initialVelocity[2]};
    uint32_t id = 0;
    _ck(pies_add_tri_mesh_volume(_handle(), static_cast<uint32_t>(vertices.size()), p.data(), static_cast<uint32_t>(indices.size() / 3),
                                 indices.data(), v, density, strainStiffness, minStrain, maxStrain, volumeStiffness, compression,
                                 stretching, triMeshResolution, nullptr, nullptr, nullptr, &id));
    lastTriMeshSkin = id;
    _skinVertices.resize(id + 1);
    _skinNormals.resize(id + 1);
    _skinVertices[id].resize(vertices.size());
    _skinNormals[id].resize(vertices.size());
    _refreshSkin(id);
    _syncRenderState();
  }
  // addTriMeshVolume after its tetrahedralize() call (PrimitiveUtilities.cpp:243-328), for hosts that mesh offline:
  // `vertices`, `tetIndices` (4 per element), `triFaceIndices` (3 per face) and `face2tet` (2 per face, -1 = no element on
  // that side) are tetgen's pointlist, tetrahedronlist, trifacelist and face2tetlist.  Like the reference: a face with an
  // element on both sides is skipped, boundary faces become triangles with the winding SWITCHED to (v0, v2, v1) so that
  // normals point outward (:255-266); mass = density, radius 0.5 (:176-177, :281-282); one strain and one volume
  // constraint per element when the respective stiffness is not 0 (:293-315).  An empty `face2tet` treats every face as a
  // boundary face.
  void addTetMeshVolume(const std::vector<glm::vec3>& vertices, const std::vector<uint32_t>& tetIndices,
                        const std::vector<uint32_t>& triFaceIndices, const std::vector<int>& face2tet, const glm::vec3& initialVelocity,
                        float density, float strainStiffness, float minStrain, float maxStrain, float volumeStiffness, float compression,
                        float stretching) {
    std::vector<uint32_t> surface;
    const size_t nf = triFaceIndices.size() / 3;
    for (size_t i = 0; i < nf; ++i) {
      if (!face2tet.empty() && face2tet[2 * i] >= 0 && face2tet[2 * i + 1] >= 0) continue;
      surface.push_back(triFaceIndices[3 * i]);
      surface.push_back(triFaceIndices[3 * i + 2]);  // switched winding
      surface.push_back(triFaceIndices[3 * i + 1]);
    }
    _addTetMesh(vertices, tetIndices, surface, initialVelocity, density, strainStiffness, minStrain, maxStrain, volumeStiffness,
                compression, stretching);
  }
  // The same without a face list: the boundary is derived from the elements (a face that belongs to exactly one element,
  // elements in order, faces opposite vertex 0, 1, 2, 3) and every triangle is wound so that its normal points away from the
  // element's fourth vertex, i.e. outward.
  void addTetMeshVolume(const std::vector<glm::vec3>& vertices, const std::vector<uint32_t>& tetIndices, const glm::vec3& initialVelocity,
                        float density, float strainStiffness, float minStrain, float maxStrain, float volumeStiffness, float compression,
                        float stretching) {
    struct Face { uint32_t key[3]; uint32_t tet, opposite; };
    static const int kFace[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
    std::vector<Face> faces;
    const size_t nt = tetIndices.size() / 4;
    for (size_t t = 0; t < nt; ++t)
      for (uint32_t f = 0; f < 4; ++f) {
        Face fc{{tetIndices[4 * t + kFace[f][0]], tetIndices[4 * t + kFace[f][1]], tetIndices[4 * t + kFace[f][2]]}, static_cast<uint32_t>(t), f};
        if (fc.key[0] > fc.key[1]) std::swap(fc.key[0], fc.key[1]);
        if (fc.key[1] > fc.key[2]) std::swap(fc.key[1], fc.key[2]);
        if (fc.key[0] > fc.key[1]) std::swap(fc.key[0], fc.key[1]);
        faces.push_back(fc);
      }
    std::vector<size_t> order(faces.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    auto less = [&](size_t a, size_t b) {
      for (int k = 0; k < 3; ++k)
        if (faces[a].key[k] != faces[b].key[k]) return faces[a].key[k] < faces[b].key[k];
      return a < b;
    };
    std::sort(order.begin(), order.end(), less);
    std::vector<char> boundary(faces.size(), 0);
    for (size_t i = 0; i < order.size();) {
      size_t j = i + 1;
      while (j < order.size() && faces[order[i]].key[0] == faces[order[j]].key[0] && faces[order[i]].key[1] == faces[order[j]].key[1] &&
             faces[order[i]].key[2] == faces[order[j]].key[2])
        ++j;
      if (j == i + 1) boundary[order[i]] = 1;
      i = j;
    }
    std::vector<uint32_t> surface;
    for (size_t i = 0; i < faces.size(); ++i) {
      if (!boundary[i]) continue;
      const uint32_t t = faces[i].tet, f = faces[i].opposite;
      uint32_t a = tetIndices[4 * t + kFace[f][0]], b = tetIndices[4 * t + kFace[f][1]], c = tetIndices[4 * t + kFace[f][2]];
      const glm::vec3 &pa = vertices[a], &pb = vertices[b], &pc = vertices[c], &pd = vertices[tetIndices[4 * t + f]];
      const float ux = pb[0] - pa[0], uy = pb[1] - pa[1], uz = pb[2] - pa[2], vx = pc[0] - pa[0], vy = pc[1] - pa[1], vz = pc[2] - pa[2];
      const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
      if (nx * (pd[0] - pa[0]) + ny * (pd[1] - pa[1]) + nz * (pd[2] - pa[2]) > 0.0f) std::swap(b, c);  // normal towards the inside: flip
      surface.push_back(a); surface.push_back(b); surface.push_back(c);
    }
    _addTetMesh(vertices, tetIndices, surface, initialVelocity, density, strainStiffness, minStrain, maxStrain, volumeStiffness,
                compression, stretching);
  }
  // Extension (pies_add_skin in pies_hip.h): an embedded surface mesh for hosts that tetrahedralise offline and draw a finer
  // surface than the simulation's own boundary - what addTriMeshVolume's "input vertices are the first nodes" gives a reference
  // host.  Every vertex is bound once to one of the listed elements (`tetIndices`: GLOBAL node ids, four per element, e.g. the
  // ids an addTetMeshVolume call produced) with barycentric weights; a vertex may lie up to `maxDistance` outside the elements'
  // boxes.  `triIndices` (three per triangle, into `vertices`; may be empty) serve the normals.  The deformed vertices and
  // normals are evaluated on the device every tick.  Returns the skin's id; throws when a vertex cannot be bound.  getSkin*
  // hold the bound rest state afterwards (evaluated on the device: the scene is finalized by this call).
  uint32_t addSkin(const std::vector<glm::vec3>& vertices, const std::vector<uint32_t>& triIndices, const std::vector<uint32_t>& tetIndices,
                   float maxDistance = 0.0f) {
    std::vector<float> p = _flatten(vertices);
    uint32_t id = 0;
    _ck(pies_add_skin(_handle(), static_cast<uint32_t>(vertices.size()), p.data(), static_cast<uint32_t>(triIndices.size() / 3),
                      triIndices.empty() ? nullptr : triIndices.data(), static_cast<uint32_t>(tetIndices.size() / 4), tetIndices.data(),
                      maxDistance, &id));
    _skinVertices.resize(id + 1);
    _skinNormals.resize(id + 1);
    _skinVertices[id].resize(vertices.size());
    _skinNormals[id].resize(vertices.size());
    _refreshSkin(id);
    return id;
  }
  // Extension (pies_raycast in pies_hip.h states the rule): the nearest hit of every ray on the scene's triangles (raycast; the
  // triangle index counts the triangles in the order they were added) or on a skin's (raycastSkin; index local to the skin), at
  // the positions the device holds now.  Directions are not normalised: t counts in units of |d|, position = o + t d; u and v
  // are the weights of the triangle's second and third corner.  A ray without a hit within tMax has hit == false, t = +inf.
  struct RayHit {
    bool hit;
    uint32_t triangle;
    float t, u, v;
    glm::vec3 position;
  };
  std::vector<RayHit> raycast(const std::vector<glm::vec3>& origins, const std::vector<glm::vec3>& directions, float tMax,
                              bool cullBack = false) {
    return _raycast(PIES_RAY_SCENE_TRIANGLES, 0, origins, directions, tMax, cullBack);
  }
  std::vector<RayHit> raycastSkin(uint32_t skin, const std::vector<glm::vec3>& origins, const std::vector<glm::vec3>& directions,
                                  float tMax, bool cullBack = false) {
    return _raycast(PIES_RAY_SKIN, skin, origins, directions, tMax, cullBack);
  }
  // Extension (pies_closest_points in pies_hip.h states the rule): for every point the closest point of the scene's triangles
  // (closestPoints; the triangle index counts the triangles in the order they were added) or of a skin's (closestPointsSkin; index
  // local to the skin) within maxDistance, at the positions the device holds now.  u and v are the weights of the triangle's
  // second and third corner at `position`.  A point without a triangle within maxDistance has found == false, distance = +inf and
  // position = the point itself.  With winding == true, `winding` is the winding number of the target's triangles at the point
  // and inside == |winding| > 0.5 (meaningful for closed surfaces; several bodies: inside any of them); otherwise both are 0.
  struct SurfacePoint {
    bool found;
    uint32_t triangle;
    float distance, u, v;
    glm::vec3 position;
    float winding;
    bool inside;
  };
  std::vector<SurfacePoint> closestPoints(const std::vector<glm::vec3>& points, float maxDistance = INFINITY, bool winding = false) {
    return _closestPoints(PIES_RAY_SCENE_TRIANGLES, 0, points, maxDistance, winding);
  }
  std::vector<SurfacePoint> closestPointsSkin(uint32_t skin, const std::vector<glm::vec3>& points, float maxDistance = INFINITY,
                                              bool winding = false) {
    return _closestPoints(PIES_RAY_SKIN, skin, points, maxDistance, winding);
  }
  // Extension (pies_collide_props in pies_hip.h states the rule): kinematic props - spheres, capsules and rounded oriented boxes
  // the host moves.  collideProps pushes the nodes out of them on the device, in the order given; a touched node takes the prop's
  // velocity at the contact along the normal (it keeps an outward normal velocity of its own) and loses the share `friction` of
  // its tangential velocity relative to the prop.  Per prop it returns the touches' impulse and torque about the prop's pivot -
  // the host applies -impulse and -torque to its own rigid body - and the number of nodes touched.  Call it once per frame
  // before tick; getVertices() is refreshed the way tick refreshes it.
  struct Prop : pies_prop_t {
    // pivot = the centre (capsule: end a) until setMotion names another
    static Prop sphere(const glm::vec3& centre, float radius) { return _shape(PIES_PROP_SPHERE, centre, radius); }
    static Prop capsule(const glm::vec3& a, const glm::vec3& b, float radius) {
      Prop p = _shape(PIES_PROP_CAPSULE, a, radius);
      for (int k = 0; k < 3; ++k) p.end[k] = b[k];
      return p;
    }
    // axes: unit and orthogonal; rounding: the radius the box's corners and edges are rounded with (it grows the box)
    static Prop box(const glm::vec3& centre, const glm::vec3& halfExtents, const glm::vec3& axis0 = glm::vec3(1.0f, 0.0f, 0.0f),
                    const glm::vec3& axis1 = glm::vec3(0.0f, 1.0f, 0.0f), const glm::vec3& axis2 = glm::vec3(0.0f, 0.0f, 1.0f),
                    float rounding = 0.0f) {
      Prop p = _shape(PIES_PROP_BOX, centre, rounding);
      for (int k = 0; k < 3; ++k) {
        p.half[k] = halfExtents[k];
        p.axes[k] = axis0[k];
        p.axes[3 + k] = axis1[k];
        p.axes[6 + k] = axis2[k];
      }
      return p;
    }
    Prop& setMotion(const glm::vec3& linear, const glm::vec3& angularVelocity, const glm::vec3& about) {
      for (int k = 0; k < 3; ++k) {
        velocity[k] = linear[k];
        angular[k] = angularVelocity[k];
        pivot[k] = about[k];
      }
      return *this;
    }
    Prop& setVelocity(const glm::vec3& linear) {
      for (int k = 0; k < 3; ++k) velocity[k] = linear[k];
      return *this;
    }
    Prop& setFriction(float f) {
      friction = f;
      return *this;
    }

   private:
    static Prop _shape(int shape, const glm::vec3& centre, float radius) {
      Prop p;
      std::memset(static_cast<pies_prop_t*>(&p), 0, sizeof(pies_prop_t));
      p.shape = shape;
      p.radius = radius;
      for (int k = 0; k < 3; ++k) p.centre[k] = p.pivot[k] = centre[k];
      p.axes[0] = p.axes[4] = p.axes[8] = 1.0f;
      return p;
    }
  };
  struct PropReaction {
    glm::vec3 impulse, torque;
    uint32_t hits;
  };
  std::vector<PropReaction> collideProps(const std::vector<Prop>& props) {
    const uint32_t n = static_cast<uint32_t>(props.size());
    std::vector<pies_prop_t> records(props.begin(), props.end());
    std::vector<float> impulse(3 * size_t(n)), torque(3 * size_t(n));
    std::vector<uint32_t> hits(n);
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_collide_props(_handle(), n, records.data(), impulse.data(), torque.data(), hits.data(), nullptr));
    _refreshPositions();
    for (uint32_t k = 0; k < _skinVertices.size(); ++k) _refreshSkin(k);
    return _reactions(impulse, torque, hits);
  }
  // Extension (pies_apply_forces in pies_hip.h states the rule): force fields.  applyForces changes the velocities on the device
  // by the forces acting for dt seconds - every force reads the state the call found, whatever its place in the list - and returns
  // per force the impulse it gave, the torque of that impulse about the force's centre and the number of nodes it affected.  A
  // force acts everywhere until within() confines it to a sphere.  Call it before tick; positions do not change.
  struct Force : pies_force_t {
    // an acceleration along `a` (asForce(): a force)
    static Force directional(const glm::vec3& a) { return _type(PIES_FORCE_DIRECTIONAL, a, 0.0f, 0.0f); }
    // away from the centre with strength > 0 (a blast), towards it with strength < 0 (an attractor)
    static Force radial(const glm::vec3& centre, float strength) { return _type(PIES_FORCE_RADIAL, glm::vec3(0.0f, 0.0f, 0.0f), strength, 0.0f).at(centre); }
    // cross(axis, p - centre) * strength; the axis need not be a unit vector
    static Force vortex(const glm::vec3& centre, const glm::vec3& axis, float strength) { return _type(PIES_FORCE_VORTEX, axis, strength, 0.0f).at(centre); }
    // a medium moving with `velocity` that takes the share min(strength * dt, 1) of the relative velocity
    static Force drag(float strength, const glm::vec3& velocity = glm::vec3(0.0f, 0.0f, 0.0f)) { return _type(PIES_FORCE_DRAG, velocity, strength, 0.0f); }
    // air moving with `velocity` against getTriangles(), both sides: strength for the normal part, shear for the tangential part
    static Force wind(const glm::vec3& velocity, float strength, float shear = 0.0f) { return _type(PIES_FORCE_WIND, velocity, strength, shear); }
    Force& within(const glm::vec3& c, float r, int fall = PIES_FALLOFF_NONE) {
      radius = r;
      falloff = fall;
      return at(c);
    }
    Force& at(const glm::vec3& c) {
      for (int k = 0; k < 3; ++k) centre[k] = c[k];
      return *this;
    }
    Force& asForce() {
      flags |= PIES_FORCE_IS_FORCE;
      return *this;
    }

   private:
    static Force _type(int type, const glm::vec3& v, float strength, float shear) {
      Force f;
      std::memset(static_cast<pies_force_t*>(&f), 0, sizeof(pies_force_t));
      f.type = type;
      f.radius = INFINITY;
      f.falloff = PIES_FALLOFF_NONE;
      f.strength = strength;
      f.shear = shear;
      for (int k = 0; k < 3; ++k) f.vector[k] = v[k];
      return f;
    }
  };
  struct ForceReaction {
    glm::vec3 impulse, torque;
    uint32_t nodes;
  };
  std::vector<ForceReaction> applyForces(const std::vector<Force>& forces, float dt) {
    const uint32_t n = static_cast<uint32_t>(forces.size());
    std::vector<pies_force_t> records(forces.begin(), forces.end());
    std::vector<float> impulse(3 * size_t(n)), torque(3 * size_t(n));
    std::vector<uint32_t> nodes(n);
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_apply_forces(_handle(), n, records.data(), dt, impulse.data(), torque.data(), nodes.data()));
    std::vector<ForceReaction> out(n);
    for (size_t k = 0; k < n; ++k) {
      out[k].impulse = glm::vec3(impulse[3 * k], impulse[3 * k + 1], impulse[3 * k + 2]);
      out[k].torque = glm::vec3(torque[3 * k], torque[3 * k + 1], torque[3 * k + 2]);
      out[k].nodes = nodes[k];
    }
    return out;
  }
  // Extension (pies_apply_surface_loads in pies_hip.h states the rule): loads that know a triangle's side and a surface's volume.
  // applySurfaceLoads changes the velocities on the device by the loads acting for dt seconds on ranges of getTriangles() - every
  // load reads the state the call found - and returns per load the impulse it gave, its torque about the load's point, the nodes
  // it affected and the volume and area of its range (also for a load of strength 0: that is how to learn a balloon's volume
  // before choosing gas()'s restVolume).  A range covers every triangle until on() confines it.  Call it before tick.
  struct SurfaceLoad : pies_surface_load_t {
    // the pressure p along every triangle's normal
    static SurfaceLoad pressure(float p) { return _type(PIES_LOAD_PRESSURE, p); }
    // an isothermal gas inside the closed range: ambient * (restVolume / V - 1) along every normal
    static SurfaceLoad gas(float ambient, float restVolume) {
      SurfaceLoad l = _type(PIES_LOAD_GAS, ambient);
      l.rest_volume = restVolume;
      return l;
    }
    // a fluid of `weight` per unit volume (density x gravity) whose surface holds surfacePoint and faces `up`
    static SurfaceLoad fluid(float weight, const glm::vec3& surfacePoint, const glm::vec3& up = glm::vec3(0.0f, 1.0f, 0.0f)) {
      SurfaceLoad l = _type(PIES_LOAD_FLUID, weight).about(surfacePoint);
      for (int k = 0; k < 3; ++k) l.up[k] = up[k];
      return l;
    }
    // a fluid's drag per unit of relative speed and submerged area, the fluid moving with `v`
    SurfaceLoad& withDrag(float d, const glm::vec3& v = glm::vec3(0.0f, 0.0f, 0.0f)) {
      drag = d;
      for (int k = 0; k < 3; ++k) velocity[k] = v[k];
      return *this;
    }
    // the range's triangles are wound with their normals pointing into the body
    SurfaceLoad& inward() {
      flags |= PIES_LOAD_INWARD;
      return *this;
    }
    // triangles [firstTriangle, firstTriangle + triangleCount) of getTriangles()
    SurfaceLoad& on(uint32_t firstTriangle, uint32_t triangleCount = UINT32_MAX) {
      first = firstTriangle;
      count = triangleCount;
      return *this;
    }
    // the point the returned torque refers to (a fluid: a point of its surface)
    SurfaceLoad& about(const glm::vec3& c) {
      for (int k = 0; k < 3; ++k) point[k] = c[k];
      return *this;
    }

   private:
    static SurfaceLoad _type(int type, float strength) {
      SurfaceLoad l;
      std::memset(static_cast<pies_surface_load_t*>(&l), 0, sizeof(pies_surface_load_t));
      l.type = type;
      l.count = UINT32_MAX;
      l.strength = strength;
      l.up[1] = 1.0f;
      return l;
    }
  };
  struct SurfaceReaction {
    glm::vec3 impulse, torque;
    uint32_t nodes;
    float volume, area;
  };
  std::vector<SurfaceReaction> applySurfaceLoads(const std::vector<SurfaceLoad>& loads, float dt) {
    const uint32_t n = static_cast<uint32_t>(loads.size());
    std::vector<pies_surface_load_t> records(loads.begin(), loads.end());
    std::vector<float> impulse(3 * size_t(n)), torque(3 * size_t(n)), volume(n), area(n);
    std::vector<uint32_t> nodes(n);
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_apply_surface_loads(_handle(), n, records.data(), dt, impulse.data(), torque.data(), nodes.data(), volume.data(), area.data()));
    std::vector<SurfaceReaction> out(n);
    for (size_t k = 0; k < n; ++k) {
      out[k].impulse = glm::vec3(impulse[3 * k], impulse[3 * k + 1], impulse[3 * k + 2]);
      out[k].torque = glm::vec3(torque[3 * k], torque[3 * k + 1], torque[3 * k + 2]);
      out[k].nodes = nodes[k];
      out[k].volume = volume[k];
      out[k].area = area[k];
    }
    return out;
  }
  // Extension (pies_apply_anchors in pies_hip.h states the rule): anchors tie nodes to frames that move - a tyre's rim to its hub, a
  // cloth corner to a joint, a picked node to the mouse - under both solvers.  addAnchors stores a set (an asset like a field: it
  // survives every scene edit and ends with clear()); applyAnchors ties the set's nodes for dt seconds to the frames as they stand
  // and move now - a node's springs are solved together and implicitly, so any stiffness is stable; a pin puts the node on its
  // point - and returns per frame the impulse the anchors gave the nodes, its torque about the frame's pivot and the number of live
  // anchors: the host applies -impulse and -torque to its rigid body.  strength 0 releases a frame.  Call it before tick;
  // getVertices() is refreshed the way tick refreshes it.
  struct AnchorFrame : pies_anchor_frame_t {
    // origin: the world position of local (0, 0, 0); the axes are the world's and pivot = origin until set otherwise
    explicit AnchorFrame(const glm::vec3& originInWorld = glm::vec3(0.0f, 0.0f, 0.0f)) {
      std::memset(static_cast<pies_anchor_frame_t*>(this), 0, sizeof(pies_anchor_frame_t));
      for (int k = 0; k < 3; ++k) origin[k] = pivot[k] = originInWorld[k];
      axes[0] = axes[4] = axes[8] = 1.0f;
      strength = 1.0f;
    }
    // unit and orthogonal
    AnchorFrame& setAxes(const glm::vec3& axis0, const glm::vec3& axis1, const glm::vec3& axis2) {
      for (int k = 0; k < 3; ++k) {
        axes[k] = axis0[k];
        axes[3 + k] = axis1[k];
        axes[6 + k] = axis2[k];
      }
      return *this;
    }
    AnchorFrame& setMotion(const glm::vec3& linear, const glm::vec3& angularVelocity, const glm::vec3& about) {
      for (int k = 0; k < 3; ++k) {
        velocity[k] = linear[k];
        angular[k] = angularVelocity[k];
        pivot[k] = about[k];
      }
      return *this;
    }
    AnchorFrame& setStrength(float s) {
      strength = s;
      return *this;
    }
    // a world position in the frame's coordinates: axis_j . (p - origin), each dot product summed left to right in fp32
    glm::vec3 toLocal(const glm::vec3& p) const {
      const float d[3] = {p[0] - origin[0], p[1] - origin[1], p[2] - origin[2]};
      glm::vec3 l;
      for (int j = 0; j < 3; ++j) l[j] = (axes[3 * j] * d[0] + axes[3 * j + 1] * d[1]) + axes[3 * j + 2] * d[2];
      return l;
    }
  };
  struct Anchor : pies_anchor_t {
    static Anchor spring(uint32_t nodeId, uint32_t frameIndex, const glm::vec3& localPoint, float k, float c = 0.0f) {
      return _make(nodeId, frameIndex, localPoint, k, c, 0u);
    }
    static Anchor pin(uint32_t nodeId, uint32_t frameIndex, const glm::vec3& localPoint) {
      return _make(nodeId, frameIndex, localPoint, 0.0f, 0.0f, PIES_ANCHOR_PIN);
    }

   private:
    static Anchor _make(uint32_t nodeId, uint32_t frameIndex, const glm::vec3& l, float k, float c, uint32_t f) {
      Anchor a;
      a.node = nodeId;
      a.frame = frameIndex;
      for (int j = 0; j < 3; ++j) a.local[j] = l[j];
      a.stiffness = k;
      a.damping = c;
      a.flags = f;
      return a;
    }
  };
  struct AnchorReaction {
    glm::vec3 impulse, torque;
    uint32_t live;
  };
  // the set's id; frameCount: how many frames applyAnchors will be given for it
  uint32_t addAnchors(const std::vector<Anchor>& anchors, uint32_t frameCount) {
    std::vector<pies_anchor_t> records(anchors.begin(), anchors.end());
    uint32_t id = 0;
    _ck(pies_add_anchors(_handle(), static_cast<uint32_t>(records.size()), records.data(), frameCount, &id));
    return id;
  }
  // the nodes `ids` tied by springs (k, c) to frame frameIndex where they are now, `frame` being where that frame stands now: the
  // attachment points are the nodes' present positions.  frameCount 0: frameIndex + 1.
  uint32_t addAnchorsHere(const std::vector<uint32_t>& ids, uint32_t frameIndex, const AnchorFrame& frame, float k, float c = 0.0f,
                          uint32_t frameCount = 0) {
    uint32_t n = 0;
    _ck(pies_count(_handle(), PIES_NODES, &n));
    std::vector<float> pos(3 * size_t(n));
    if (n) _ck(pies_read_nodes(_handle(), PIES_NODE_POSITION, pos.data(), n));
    std::vector<Anchor> anchors;
    for (uint32_t id : ids) {
      if (id >= n) throw std::runtime_error("Pies::Solver::addAnchorsHere: node id out of range");
      anchors.push_back(Anchor::spring(id, frameIndex, frame.toLocal(glm::vec3(pos[3 * size_t(id)], pos[3 * size_t(id) + 1], pos[3 * size_t(id) + 2])), k, c));
    }
    return addAnchors(anchors, frameCount ? frameCount : frameIndex + 1);
  }
  // perAnchor, when given: per anchor of the set the impulse it gave its node (x, y, z) and its stretch (w)
  std::vector<AnchorReaction> applyAnchors(uint32_t set, const std::vector<AnchorFrame>& frames, float dt,
                                           std::vector<glm::vec4>* perAnchor = nullptr) {
    const uint32_t n = static_cast<uint32_t>(frames.size());
    std::vector<pies_anchor_frame_t> records(frames.begin(), frames.end());
    std::vector<float> impulse(3 * size_t(n)), torque(3 * size_t(n)), entries;
    std::vector<uint32_t> live(n);
    if (perAnchor) {
      uint32_t count = 0;
      _ck(pies_get_anchors(_handle(), set, nullptr, 0, &count, nullptr));
      entries.resize(4 * size_t(count));
    }
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_apply_anchors(_handle(), set, n, records.data(), dt, impulse.data(), torque.data(), live.data(),
                           perAnchor ? entries.data() : nullptr));
    _refreshPositions();
    for (uint32_t k = 0; k < _skinVertices.size(); ++k) _refreshSkin(k);
    if (perAnchor) {
      perAnchor->resize(entries.size() / 4);
      for (size_t i = 0; i < perAnchor->size(); ++i)
        for (int c = 0; c < 4; ++c) (*perAnchor)[i][c] = entries[4 * i + c];
    }
    std::vector<AnchorReaction> out(n);
    for (size_t k = 0; k < n; ++k) {
      out[k].impulse = glm::vec3(impulse[3 * k], impulse[3 * k + 1], impulse[3 * k + 2]);
      out[k].torque = glm::vec3(torque[3 * k], torque[3 * k + 1], torque[3 * k + 2]);
      out[k].live = live[k];
    }
    return out;
  }
  // Extension (pies_apply_ties in pies_hip.h states the rule): ties bind nodes to points on other bodies - a cloth sewn to a body,
  // skin glued to flesh, two bodies welded at a seam, a seam that rips - under both solvers.  Where an anchor lets the host pull a
  // body, a tie lets two parts of the scene pull each other: the carrier feels it.  addTies stores a set (an asset like an anchor
  // set: it survives every scene edit and ends with clear()); applyTies binds the set's nodes for dt seconds in `iterations`
  // Jacobi iterations - implicit, so any stiffness is stable; stiff seams want more iterations - and returns per group the impulse
  // the ties gave their tied nodes, its torque about the group's pivot and the number of live ties.  strength 0 releases a group;
  // breakStretch > 0 breaks the ties found longer, for good (tieState, resetTies).  Call it after tick; getVertices() is
  // refreshed the way tick refreshes it.
  struct Tie : pies_tie_t {
    // the point (u, v) of the triangle (c0, c1, c2) as pies_closest_points reports it: weights ((1 - u) - v, u, v)
    static Tie onTriangle(uint32_t nodeId, uint32_t c0, uint32_t c1, uint32_t c2, float u, float v, float k, float c = 0.0f,
                          uint32_t groupIndex = 0) {
      return _make(nodeId, c0, c1, c2, (1.0f - u) - v, u, v, k, c, groupIndex);
    }
    // the point e0 + t (e1 - e0) of an edge
    static Tie onEdge(uint32_t nodeId, uint32_t e0, uint32_t e1, float t, float k, float c = 0.0f, uint32_t groupIndex = 0) {
      return _make(nodeId, e0, e1, e0, 1.0f - t, t, 0.0f, k, c, groupIndex);
    }
    static Tie toNode(uint32_t nodeId, uint32_t other, float k, float c = 0.0f, uint32_t groupIndex = 0) {
      return _make(nodeId, other, other, other, 1.0f, 0.0f, 0.0f, k, c, groupIndex);
    }

   private:
    static Tie _make(uint32_t a, uint32_t b0, uint32_t b1, uint32_t b2, float w0, float w1, float w2, float k, float c, uint32_t g) {
      Tie t;
      t.node = a;
      t.to[0] = b0; t.to[1] = b1; t.to[2] = b2;
      t.weight[0] = w0; t.weight[1] = w1; t.weight[2] = w2;
      t.stiffness = k;
      t.damping = c;
      t.group = g;
      return t;
    }
  };
  struct TieGroup : pies_tie_group_t {
    explicit TieGroup(const glm::vec3& torquePivot = glm::vec3(0.0f, 0.0f, 0.0f), float s = 1.0f, float breakAt = 0.0f) {
      for (int k = 0; k < 3; ++k) pivot[k] = torquePivot[k];
      strength = s;
      break_stretch = breakAt;
    }
    TieGroup& setStrength(float s) {
      strength = s;
      return *this;
    }
    TieGroup& setBreakStretch(float length) {
      break_stretch = length;
      return *this;
    }
  };
  struct TieReaction {
    glm::vec3 impulse, torque;
    uint32_t live;
  };
  // the set's id; groupCount: how many groups applyTies will be given for it
  uint32_t addTies(const std::vector<Tie>& ties, uint32_t groupCount = 1) {
    std::vector<pies_tie_t> records(ties.begin(), ties.end());
    uint32_t id = 0;
    _ck(pies_add_ties(_handle(), static_cast<uint32_t>(records.size()), records.data(), groupCount, &id));
    return id;
  }
  // perTie, when given: per tie of the set the impulse it gave its tied node (x, y, z) and its stretch (w)
  std::vector<TieReaction> applyTies(uint32_t set, const std::vector<TieGroup>& groups, float dt, uint32_t iterations = 4,
                                     std::vector<glm::vec4>* perTie = nullptr) {
    const uint32_t n = static_cast<uint32_t>(groups.size());
    std::vector<pies_tie_group_t> records(groups.begin(), groups.end());
    std::vector<float> impulse(3 * size_t(n)), torque(3 * size_t(n)), entries;
    std::vector<uint32_t> live(n);
    if (perTie) {
      uint32_t count = 0;
      _ck(pies_get_ties(_handle(), set, nullptr, 0, &count, nullptr));
      entries.resize(4 * size_t(count));
    }
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_apply_ties(_handle(), set, n, records.data(), dt, iterations, impulse.data(), torque.data(), live.data(),
                        perTie ? entries.data() : nullptr));
    _refreshPositions();
    for (uint32_t k = 0; k < _skinVertices.size(); ++k) _refreshSkin(k);
    if (perTie) {
      perTie->resize(entries.size() / 4);
      for (size_t i = 0; i < perTie->size(); ++i)
        for (int c = 0; c < 4; ++c) (*perTie)[i][c] = entries[4 * i + c];
    }
    std::vector<TieReaction> out(n);
    for (size_t k = 0; k < n; ++k) {
      out[k].impulse = glm::vec3(impulse[3 * k], impulse[3 * k + 1], impulse[3 * k + 2]);
      out[k].torque = glm::vec3(torque[3 * k], torque[3 * k + 1], torque[3 * k + 2]);
      out[k].live = live[k];
    }
    return out;
  }
  // per tie of the set: 1 once it broke
  std::vector<uint8_t> tieState(uint32_t set) {
    uint32_t count = 0;
    _ck(pies_get_ties(_handle(), set, nullptr, 0, &count, nullptr));
    std::vector<uint8_t> broken(count);
    _ck(pies_get_tie_state(_handle(), set, broken.data(), count, nullptr));
    return broken;
  }
  // no tie of the set is broken any more
  void resetTies(uint32_t set) { _ck(pies_reset_ties(_handle(), set)); }
  // Extension (pies_drive_actuators in pies_hip.h states the rule): actuators let the body move itself - a muscle, a tendon, a
  // bellows, a hinge that folds: distance and bend constraints whose rest length or rest angle follows an activation, written where
  // the device holds the rest records, without the rebuild a rest edit costs otherwise.  addActuators stores a set (an asset like
  // an anchor set: it survives every scene edit and ends with clear()); driveActuators writes the rests from one activation per
  // channel and returns per channel the measured values and the written rests of its live actuators added, and their count.  Call
  // it before tick; node state is not touched.
  struct Actuator : pies_actuator_t {
    // the rest becomes base (1 + gain u), clamped to [lo, hi]; base is the constraint's rest when the set is added
    static Actuator scaled(int containerType, uint32_t constraintIndex, uint32_t channelIndex, float g, float lowest, float highest) {
      return _make(containerType, constraintIndex, channelIndex, g, lowest, highest, 0u);
    }
    // the rest becomes base + gain u, clamped to [lo, hi]
    static Actuator offset(int containerType, uint32_t constraintIndex, uint32_t channelIndex, float g, float lowest, float highest) {
      return _make(containerType, constraintIndex, channelIndex, g, lowest, highest, PIES_ACTUATOR_OFFSET);
    }

   private:
    static Actuator _make(int t, uint32_t i, uint32_t c, float g, float l, float h, uint32_t f) {
      Actuator a;
      a.type = t;
      a.index = i;
      a.channel = c;
      a.gain = g;
      a.lo = l;
      a.hi = h;
      a.base = 0.0f;
      a.flags = f;
      return a;
    }
  };
  struct ActuatorChannel {
    float value, rest;  // sums over the channel's live actuators: measured lengths / dihedral cosines, written rests
    uint32_t live;
  };
  // the set's id; channelCount: how many activations driveActuators will be given for it
  uint32_t addActuators(const std::vector<Actuator>& actuators, uint32_t channelCount = 1) {
    std::vector<pies_actuator_t> records(actuators.begin(), actuators.end());
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);  // (the constraints the records name)
    uint32_t id = 0;
    _ck(pies_add_actuators(_handle(), static_cast<uint32_t>(records.size()), records.data(), channelCount, &id));
    return id;
  }
  // the set as the library holds it, `base` filled in
  std::vector<pies_actuator_t> actuators(uint32_t set, uint32_t* channelCount = nullptr) {
    uint32_t count = 0;
    _ck(pies_get_actuators(_handle(), set, nullptr, 0, &count, channelCount));
    std::vector<pies_actuator_t> out(count);
    if (count) _ck(pies_get_actuators(_handle(), set, out.data(), count, nullptr, nullptr));
    return out;
  }
  struct ActuatorEntry {
    float rest, value;  // the rest the actuator's constraint holds after the call; its measured length / dihedral cosine
  };
  // perActuator, when given: one entry per actuator of the set, in the set's own order
  std::vector<ActuatorChannel> driveActuators(uint32_t set, const std::vector<float>& activation,
                                              std::vector<ActuatorEntry>* perActuator = nullptr) {
    const uint32_t n = static_cast<uint32_t>(activation.size());
    std::vector<float> sums(2 * size_t(n)), entries;
    std::vector<uint32_t> live(n);
    if (perActuator) {
      uint32_t count = 0;
      _ck(pies_get_actuators(_handle(), set, nullptr, 0, &count, nullptr));
      entries.resize(2 * size_t(count));
    }
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_drive_actuators(_handle(), set, n, activation.data(), sums.data(), live.data(), perActuator ? entries.data() : nullptr));
    if (perActuator) {
      perActuator->resize(entries.size() / 2);
      for (size_t i = 0; i < perActuator->size(); ++i) (*perActuator)[i] = ActuatorEntry{entries[2 * i], entries[2 * i + 1]};
    }
    std::vector<ActuatorChannel> out(n);
    for (size_t k = 0; k < n; ++k) out[k] = ActuatorChannel{sums[2 * k], sums[2 * k + 1], live[k]};
    return out;
  }
  // Extension (pies_measure_elements / pies_measure_nodes in pies_hip.h state the rules): how the body is doing, evaluated on the
  // device without a read-back.  measureElements answers for elements [first, first + count) of the tetrahedral (PIES_TET) or the
  // volume (PIES_VOLUME) constraints in the order they were added - stretches, det F, volume, |F|^2, the norm of the Green strain
  // and the PIES_ELEMENT_* flags per element when `records` is given, and the range's summary; count == UINT32_MAX: to the
  // container's end.  measureNodes sums mass, momentum, angular momentum about `about`, first moment and kinetic energy over
  // ranges of node ids (a body is the range its create* call appended); fp32 sums in a fixed order.  Both are read-only.
  pies_element_summary_t measureElements(int type, uint32_t first = 0, uint32_t count = UINT32_MAX,
                                         std::vector<pies_element_measure_t>* records = nullptr) {
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    if (count == UINT32_MAX) {
      uint32_t size = 0;
      _ck(pies_count(_handle(), type, &size));
      count = size >= first ? size - first : 0;
    }
    if (records) records->assign(count, pies_element_measure_t{});
    pies_element_summary_t summary;
    _ck(pies_measure_elements(_handle(), type, first, count, records && count ? records->data() : nullptr, &summary));
    return summary;
  }
  struct NodeRange {
    uint32_t first, count;
    glm::vec3 about;
  };
  std::vector<pies_node_sums_t> measureNodes(const std::vector<NodeRange>& ranges) {
    const uint32_t n = static_cast<uint32_t>(ranges.size());
    std::vector<uint32_t> pairs(2 * size_t(n));
    std::vector<float> about(3 * size_t(n));
    for (size_t k = 0; k < n; ++k) {
      pairs[2 * k] = ranges[k].first;
      pairs[2 * k + 1] = ranges[k].count;
      for (int c = 0; c < 3; ++c) about[3 * k + c] = ranges[k].about[c];
    }
    std::vector<pies_node_sums_t> out(n);
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_measure_nodes(_handle(), n, pairs.data(), about.data(), out.data()));
    return out;
  }
  // Extension (pies_read_nodes_device / pies_write_nodes_device / pies_read_skin_device in pies_hip.h state the rules): node state
  // and skins to and from DEVICE memory of the host program - a vertex buffer shared with HIP, a controller that lives on the GPU -
  // ordered against `stream` (the host's hipStream_t; nullptr: the default stream) by events, without a host synchronisation
  // unless flags has PIES_IO_HOST_SYNC.  Arrays are in the order of getVertices(); a NULL pointer leaves that array out.
  // writeNodesDevice does not refresh getVertices(): the next tick does.
  void readNodesDevice(const pies_device_nodes_t& dst, void* stream = nullptr, uint32_t flags = 0) {
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    uint32_t n = 0;
    _ck(pies_count(_handle(), PIES_NODES, &n));
    _ck(pies_read_nodes_device(_handle(), &dst, n, stream, flags));
  }
  // ids == nullptr: row k is node k; otherwise a device array of `count` node ids
  void writeNodesDevice(const pies_device_nodes_t& src, const uint32_t* ids = nullptr, uint32_t count = 0, void* stream = nullptr,
                        uint32_t flags = 0) {
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    if (!ids) _ck(pies_count(_handle(), PIES_NODES, &count));
    _ck(pies_write_nodes_device(_handle(), &src, ids, count, stream, flags));
  }
  void readSkinDevice(uint32_t skin, void* positions, void* normals = nullptr, void* stream = nullptr, uint32_t flags = 0) {
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    uint32_t n = 0;
    _ck(pies_get_skin_binding(_handle(), skin, nullptr, nullptr, nullptr, 0, &n));
    _ck(pies_read_skin_device(_handle(), skin, positions, normals, n, stream, flags));
  }
  // Extension (pies_collide_field_props in pies_hip.h states the rule): rigid colliders of any shape.  A field is a signed distance
  // function on a lattice in a local frame, negative inside: addField takes the host's samples (sample (i, j, k) at local
  // origin + (i, j, k) * cell, stored at (k * ny + j) * nx + i: an analytic shape, a height field), addFieldFromTriMesh builds
  // them on the device from a closed triangle mesh (brute force, once; margin >= the largest prop radius + the largest node
  // radius + cell).  Both return the field's id; fields survive everything but clear().  A FieldProp places a field rigidly in
  // the world; collideFieldProps pushes the nodes out of the props in the order given and returns what collideProps returns.
  uint32_t addField(uint32_t nx, uint32_t ny, uint32_t nz, const glm::vec3& origin, float cell, const std::vector<float>& samples) {
    if (samples.size() != size_t(nx) * ny * nz) throw std::runtime_error("Pies::Solver::addField: samples.size() != nx * ny * nz");
    const uint32_t dims[3] = {nx, ny, nz};
    const float o[3] = {origin[0], origin[1], origin[2]};
    uint32_t id = 0;
    _ck(pies_add_field(_handle(), dims, o, cell, samples.data(), &id));
    return id;
  }
  uint32_t addFieldFromTriMesh(const std::vector<glm::vec3>& vertices, const std::vector<uint32_t>& triangleIndices, float cell,
                               float margin) {
    std::vector<float> p = _flatten(vertices);
    uint32_t id = 0;
    _ck(pies_add_field_tri_mesh(_handle(), static_cast<uint32_t>(vertices.size()), p.data(),
                                static_cast<uint32_t>(triangleIndices.size() / 3), triangleIndices.data(), cell, margin, &id));
    return id;
  }
  struct FieldProp : pies_field_prop_t {
    // centre: the world position of the field's local (0, 0, 0); the frame is the world's and pivot = centre until set otherwise
    FieldProp(uint32_t fieldId, const glm::vec3& centreInWorld, float inflation = 0.0f) {
      std::memset(static_cast<pies_field_prop_t*>(this), 0, sizeof(pies_field_prop_t));
      field = fieldId;
      radius = inflation;
      for (int k = 0; k < 3; ++k) centre[k] = pivot[k] = centreInWorld[k];
      axes[0] = axes[4] = axes[8] = 1.0f;
    }
    // unit and orthogonal: local axis j in world coordinates
    FieldProp& setAxes(const glm::vec3& axis0, const glm::vec3& axis1, const glm::vec3& axis2) {
      for (int k = 0; k < 3; ++k) {
        axes[k] = axis0[k];
        axes[3 + k] = axis1[k];
        axes[6 + k] = axis2[k];
      }
      return *this;
    }
    FieldProp& setMotion(const glm::vec3& linear, const glm::vec3& angularVelocity, const glm::vec3& about) {
      for (int k = 0; k < 3; ++k) {
        velocity[k] = linear[k];
        angular[k] = angularVelocity[k];
        pivot[k] = about[k];
      }
      return *this;
    }
    FieldProp& setVelocity(const glm::vec3& linear) {
      for (int k = 0; k < 3; ++k) velocity[k] = linear[k];
      return *this;
    }
    FieldProp& setFriction(float f) {
      friction = f;
      return *this;
    }
  };
  std::vector<PropReaction> collideFieldProps(const std::vector<FieldProp>& props) {
    const uint32_t n = static_cast<uint32_t>(props.size());
    std::vector<pies_field_prop_t> records(props.begin(), props.end());
    std::vector<float> impulse(3 * size_t(n)), torque(3 * size_t(n));
    std::vector<uint32_t> hits(n);
    _pushState(_pushed[4] >= 0 ? static_cast<SolverName>(_pushed[4]) : _options.solver);
    _ck(pies_collide_field_props(_handle(), n, records.data(), impulse.data(), torque.data(), hits.data(), nullptr));
    _refreshPositions();
    for (uint32_t k = 0; k < _skinVertices.size(); ++k) _refreshSkin(k);
    return _reactions(impulse, torque, hits);
  }
  void addFixedRegions(const std::vector<glm::mat4>& regionMatrices, float w) {
    std::vector<float> m = _flattenMats(regionMatrices);
    _ck(pies_add_fixed_regions(_handle(), static_cast<uint32_t>(regionMatrices.size()), m.data(), w));
  }
  void updateFixedRegions(const std::vector<glm::mat4>& regionMatrices) {
    std::vector<float> m = _flattenMats(regionMatrices);
    // the reference asserts and returns on a size mismatch (PrimitiveUtilities.cpp:115-118); here it throws
    _ck(pies_update_fixed_regions(_handle(), static_cast<uint32_t>(regionMatrices.size()), m.data()));
  }
  void addLinkedRegions(const std::vector<glm::mat4>& regionMatrices, float w) {
    std::vector<float> m = _flattenMats(regionMatrices);
    _ck(pies_add_linked_regions(_handle(), static_cast<uint32_t>(regionMatrices.size()), m.data(), w));
  }

  // ---- primitives (PrimitiveUtilities.cpp:330-1289), reference grid sizes ----
  void createBox(const glm::vec3& translation, float scale, float w) {
    const float t[3] = {translation[0], translation[1], translation[2]};
    _ck(pies_create_box(_handle(), 5, 5, 5, t, scale, w, 0, 0, 2u));
    _syncRenderState();
  }
  void createTetBox(const glm::vec3& translation, float scale, const glm::vec3& initialVelocity, float w, float mass, bool hinged) {
    const float t[3] = {translation[0], translation[1], translation[2]}, v[3] = {initialVelocity[0], initialVelocity[1], initialVelocity[2]};
    if (hinged) _ck(pies_create_tet_box(_handle(), 10, 2, 10, t, scale, v, w, mass, 3u));
    else _ck(pies_create_tet_box(_handle(), 3, 3, 3, t, scale, v, w, mass, 3u));
    _syncRenderState();
  }
  void createSheet(const glm::vec3& translation, float scale, float mass, float k) {
    const float t[3] = {translation[0], translation[1], translation[2]};
    _ck(pies_create_sheet(_handle(), 20, 20, t, scale, mass, k));
    _syncRenderState();
  }
  // like the reference, `scale` and `initialVelocity` are accepted and ignored (PrimitiveUtilities.cpp:995,1015)
  void createShapeMatchingBox(const glm::vec3& translation, uint32_t countX, uint32_t countY, uint32_t countZ, float /*scale*/,
                              const glm::vec3& /*initialVelocity*/, float w) {
    const float t[3] = {translation[0], translation[1], translation[2]};
    _ck(pies_create_shape_matching_box(_handle(), t, countX, countY, countZ, w));
    _syncRenderState();
  }
  void createShapeMatchingSheet(const glm::vec3& translation, float scale, const glm::vec3& /*initialVelocity*/, float w) {
    const float t[3] = {translation[0], translation[1], translation[2]};
    _ck(pies_create_shape_matching_sheet(_handle(), 50, 50, t, scale, w));
    _syncRenderState();
  }
  void createBendSheet(const glm::vec3& translation, float scale, float w) {
    const float t[3] = {translation[0], translation[1], translation[2]};
    _ck(pies_create_bend_sheet(_handle(), 10, 10, t, scale, w));
    _syncRenderState();
  }

  pies_solver_t* handle() { return _handle(); }  // escape hatch to the C ABI (schedules, PCG settings, statistics)

private:
  static float _randf() { return static_cast<float>(double(std::rand()) / RAND_MAX); }  // cosmetics only (PrimitiveUtilities.cpp:10-12)
  static std::vector<float> _flatten(const std::vector<glm::vec3>& v) {
    std::vector<float> p(3 * v.size());
    for (size_t i = 0; i < v.size(); ++i) { p[3 * i] = v[i][0]; p[3 * i + 1] = v[i][1]; p[3 * i + 2] = v[i][2]; }
    return p;
  }
  static std::vector<float> _flattenMats(const std::vector<glm::mat4>& v) {
    std::vector<float> m(16 * v.size());
    for (size_t k = 0; k < v.size(); ++k)
      for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) m[16 * k + 4 * c + r] = v[k][c][r];
    return m;
  }
  // nodes, constraints and (already outward-wound) surface triangles of a tetrahedral mesh (PrimitiveUtilities.cpp:268-326)
  void _addTetMesh(const std::vector<glm::vec3>& vertices, const std::vector<uint32_t>& tetIndices, const std::vector<uint32_t>& surface,
                   const glm::vec3& initialVelocity, float density, float strainStiffness, float minStrain, float maxStrain,
                   float volumeStiffness, float compression, float stretching) {
    const uint32_t n = static_cast<uint32_t>(vertices.size());
    std::vector<float> p = _flatten(vertices), v(3 * size_t(n)), r(n, 0.5f), im(n, 1.0f / density);
    for (uint32_t i = 0; i < n; ++i) { v[3 * i] = initialVelocity[0]; v[3 * i + 1] = initialVelocity[1]; v[3 * i + 2] = initialVelocity[2]; }
    uint32_t first = 0;
    _ck(pies_add_nodes_ex(_handle(), n, p.data(), v.data(), r.data(), im.data(), &first));
    std::vector<uint32_t> t(tetIndices), f(surface);
    for (uint32_t& id : t) id += first;
    for (uint32_t& id : f) id += first;
    const uint32_t nt = static_cast<uint32_t>(t.size() / 4);
    if (strainStiffness != 0.0f) _ck(pies_add_tet_constraints(_handle(), nt, t.data(), strainStiffness, minStrain, maxStrain));
    if (volumeStiffness != 0.0f) _ck(pies_add_volume_constraints(_handle(), nt, t.data(), volumeStiffness, compression, stretching));
    _ck(pies_add_triangles(_handle(), static_cast<uint32_t>(f.size() / 3), f.data()));
    _syncRenderState();
  }
  void _ck(int rc) const {
    if (rc != PIES_OK) throw std::runtime_error(std::string("Pies::Solver: ") + pies_last_error(_h));
  }
  // after an add*/create*: new vertices get one colour per primitive, lines/triangles are re-read
  void _syncRenderState() {
    uint32_t n = 0, nl = 0, nt = 0;
    _ck(pies_count(_handle(), PIES_NODES, &n));
    _ck(pies_count(_handle(), PIES_LINES, &nl));
    _ck(pies_count(_handle(), PIES_TRIANGLES, &nt));
    const size_t old = _vertices.size();
    _vertices.resize(n);
    std::vector<float> pos(3 * size_t(n)), rad(n);
    if (n) {
      _ck(pies_read_nodes(_handle(), PIES_NODE_POSITION, pos.data(), n));
      _ck(pies_read_nodes(_handle(), PIES_NODE_RADIUS, rad.data(), n));
    }
    const glm::vec3 colour(_randf(), _randf(), _randf());
    const float roughness = _randf(), metallic = static_cast<float>(std::rand() % 2);
    for (size_t i = 0; i < n; ++i) {
      _vertices[i].position = glm::vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
      _vertices[i].radius = rad[i];
      if (i >= old) { _vertices[i].baseColor = colour; _vertices[i].roughness = roughness; _vertices[i].metallic = metallic; }
    }
    _lines.resize(nl);
    if (nl) _ck(pies_get_ids(_handle(), PIES_LINES, _lines.data(), nl));
    _triangles.resize(nt);
    if (nt) _ck(pies_get_ids(_handle(), PIES_TRIANGLES, &_triangles[0].nodeIds[0], 3 * nt));
    renderStateDirty = true;
  }
  // Solver.cpp:157,393: _vertices[i].position = node.position.  pies_tick has already brought the positions to the
  // host (one pinned D2H copy per tick); this writes them straight into the vertex stream.
  void _refreshPositions() {
    const uint32_t n = static_cast<uint32_t>(_vertices.size());
    if (!n) return;
    _ck(pies_read_positions_strided(_handle(), &_vertices[0].position, sizeof(Vertex), n));
  }

  void _copySkin(uint32_t k, const float* x, const float* nr, uint32_t nv) {
    const size_t m = nv < _skinVertices[k].size() ? nv : _skinVertices[k].size();
    for (size_t i = 0; i < m; ++i) {
      _skinVertices[k][i] = glm::vec3(x[3 * i], x[3 * i + 1], x[3 * i + 2]);
      _skinNormals[k][i] = glm::vec3(nr[3 * i], nr[3 * i + 1], nr[3 * i + 2]);
    }
  }
  void _refreshSkin(uint32_t k) {
    const uint32_t nv = static_cast<uint32_t>(_skinVertices[k].size());
    _skinScratch.resize(6 * size_t(nv));
    _ck(pies_read_skin(_handle(), k, _skinScratch.data(), _skinScratch.data() + 3 * size_t(nv), nv));
    _copySkin(k, _skinScratch.data(), _skinScratch.data() + 3 * size_t(nv), nv);
  }

  std::vector<RayHit> _raycast(int target, uint32_t skin, const std::vector<glm::vec3>& origins, const std::vector<glm::vec3>& directions,
                               float tMax, bool cullBack) {
    if (origins.size() != directions.size()) throw std::runtime_error("Pies::Solver: raycast needs one direction per origin");
    const uint32_t n = static_cast<uint32_t>(origins.size());
    std::vector<float> o = _flatten(origins), d = _flatten(directions), t(n), uv(2 * size_t(n));
    std::vector<uint32_t> tri(n);
    _ck(pies_raycast(_handle(), target, skin, n, o.data(), d.data(), tMax, cullBack ? PIES_RAY_CULL_BACK : 0u, tri.data(), t.data(),
                     uv.data()));
    std::vector<RayHit> hits(n);
    for (size_t i = 0; i < n; ++i) {
      RayHit& h = hits[i];
      h.hit = tri[i] != PIES_RAY_MISS;
      h.triangle = tri[i];
      h.t = t[i];
      h.u = uv[2 * i];
      h.v = uv[2 * i + 1];
      const glm::vec3 &p = origins[i], &q = directions[i];
      h.position = h.hit ? glm::vec3(p[0] + t[i] * q[0], p[1] + t[i] * q[1], p[2] + t[i] * q[2]) : p;
    }
    return hits;
  }

  static std::vector<PropReaction> _reactions(const std::vector<float>& impulse, const std::vector<float>& torque,
                                              const std::vector<uint32_t>& hits) {
    std::vector<PropReaction> out(hits.size());
    for (size_t k = 0; k < hits.size(); ++k) {
      out[k].impulse = glm::vec3(impulse[3 * k], impulse[3 * k + 1], impulse[3 * k + 2]);
      out[k].torque = glm::vec3(torque[3 * k], torque[3 * k + 1], torque[3 * k + 2]);
      out[k].hits = hits[k];
    }
    return out;
  }

  std::vector<SurfacePoint> _closestPoints(int target, uint32_t skin, const std::vector<glm::vec3>& points, float maxDistance, bool winding) {
    const uint32_t n = static_cast<uint32_t>(points.size());
    std::vector<float> p = _flatten(points), d(n), uv(2 * size_t(n)), q(3 * size_t(n)), w(winding ? n : 0);
    std::vector<uint32_t> tri(n);
    _ck(pies_closest_points(_handle(), target, skin, n, p.data(), maxDistance, tri.data(), d.data(), uv.data(), q.data(),
                            winding ? w.data() : nullptr));
    std::vector<SurfacePoint> out(n);
    for (size_t i = 0; i < n; ++i) {
      SurfacePoint& o = out[i];
      o.found = tri[i] != PIES_NEAR_NONE;
      o.triangle = tri[i];
      o.distance = d[i];
      o.u = uv[2 * i];
      o.v = uv[2 * i + 1];
      o.position = glm::vec3(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
      o.winding = winding ? w[i] : 0.0f;
      o.inside = std::fabs(o.winding) > 0.5f;
    }
    return out;
  }

  // opens the device handle on first use
  pies_solver_t* _handle() {
    if (!_h) {
      pies_options_t o;
      static_assert(sizeof(o) == sizeof(_options), "layout");
      std::memcpy(&o, &_options, sizeof(o));
      if (pies_create(&o, _device, &_h) != PIES_OK) throw std::runtime_error("Pies::Solver: no gfx950 HIP device (there is no CPU fallback)");
    }
    return _h;
  }
  // the public flags, the schedule and the solver to run reach the handle when they differ from what it was last given
  void _pushState(SolverName solver) {
    pies_solver_t* h = _handle();
    const int now[7] = {releaseHinge ? 1 : 0, nodeCollisions ? 1 : 0, triangleCollisions ? 1 : 0, schedule, static_cast<int>(solver),
                        renumberNodes ? 1 : 0, pdNodeContacts ? 1 : 0};
    if (now[0] != _pushed[0]) _ck(pies_set_flag(h, PIES_FLAG_RELEASE_HINGE, now[0]));
    if (now[1] != _pushed[1]) _ck(pies_set_flag(h, PIES_FLAG_NODE_COLLISIONS, now[1]));
    if (now[2] != _pushed[2]) _ck(pies_set_flag(h, PIES_FLAG_TRIANGLE_COLLISIONS, now[2]));
    if (now[3] != _pushed[3] && now[3] >= 0) _ck(pies_set_schedule(h, now[3]));
    if (now[4] != _pushed[4]) _ck(pies_set_solver(h, now[4]));
    if (now[5] != _pushed[5]) _ck(pies_set_flag(h, PIES_FLAG_RENUMBER_NODES, now[5]));
    if (now[6] != _pushed[6]) _ck(pies_set_flag(h, PIES_FLAG_PD_NODE_CONTACTS, now[6]));
    for (int k = 0; k < 7; ++k) _pushed[k] = now[k];
  }
  void _tickAs(SolverName solver) {
    _pushState(solver);
    _ck(pies_tick(_handle()));
    _refreshPositions();
    for (uint32_t k = 0; k < _skinVertices.size(); ++k) _refreshSkin(k);
  }

  pies_solver_t* _h = nullptr;
  SolverOptions _options;
  int _device = 0;
  int _pushed[7] = {-2, -2, -2, -2, -2, -2, -2};  // releaseHinge, nodeCollisions, triangleCollisions, schedule, solver, renumberNodes,
                                                  // pdNodeContacts as last given to the handle
  std::vector<Vertex> _vertices;
  std::vector<uint32_t> _lines;
  std::vector<Triangle> _triangles;
  std::vector<std::vector<glm::vec3>> _skinVertices, _skinNormals;  // per skin (addSkin)
  std::vector<float> _skinScratch;
  uint64_t _frames[2] = {0, 0};  // ticks begun and not yet ended (beginTick / endTick)
};
}  // namespace Pies

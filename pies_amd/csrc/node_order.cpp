// Node renumbering of PD scenes (PIES_FLAG_RENUMBER_NODES): the one place that owns the permutation.
//
// The windowed system matrix stages, per chunk of 256 rows, the columns outside the chunk (its halo) in LDS.  A mesh whose ids
// follow space has a halo of about one column per row; a mesh numbered any other way (a tetrahedraliser's output, ids shuffled)
// has many more, and the CG iteration slows down about threefold.  pies_finalize therefore sorts the nodes
// of such a scene along a Hilbert curve of their positions and builds the device scene in that numbering.  The host keeps its
// own: the host mirror and the containers stay in host numbering, the device scene is built from translated copies
// (InternalNumbering), and node state crosses the bus through the permutation (device_scene.cpp: upload_nodes, download_nodes; capi.cpp: export).
//
// The decision, made on the host and deterministic:
//   1. the flag is set and the solver is PD (PBD keeps the identity: its orders are the reference's);
//   2. the identity would not be given a row dictionary (a createTetBox lattice: the dictionary streams no matrix at all);
//   3. the Hilbert order cuts the halo per row of the windowed matrix to at most kHaloRatio of the identity's.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <utility>
#include <vector>

#include "device_util.h"

namespace pies {

namespace {
// measured on the 100k-node Delaunay beam: Hilbert order 1.21 halo columns per row, lattice order 6.42,
// random order 14.6; a candidate has to beat the identity clearly for the renumbering to pay its gathers at the host boundary
constexpr double kHaloRatio = 0.8;
constexpr int kCurveBits = 21;  // per axis: 63-bit keys

// Hilbert index of a point of the 2^kCurveBits cube (J. Skilling, "Programming the Hilbert curve", AIP Conf. Proc. 707, 2004:
// the axes are converted to the transposed Hilbert index in place, whose bits, interleaved, are the index)
uint64_t hilbert_key(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t X[3] = {x, y, z};
  const uint32_t M = 1u << (kCurveBits - 1);
  for (uint32_t Q = M; Q > 1; Q >>= 1) {  // inverse undo
    const uint32_t P = Q - 1;
    for (int i = 0; i < 3; ++i) {
      if (X[i] & Q) {
        X[0] ^= P;
      } else {
        const uint32_t t = (X[0] ^ X[i]) & P;
        X[0] ^= t;
        X[i] ^= t;
      }
    }
  }
  for (int i = 1; i < 3; ++i) X[i] ^= X[i - 1];  // Gray encode
  uint32_t t = 0;
  for (uint32_t Q = M; Q > 1; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1;
  for (int i = 0; i < 3; ++i) X[i] ^= t;
  uint64_t key = 0;
  for (int b = kCurveBits - 1; b >= 0; --b)
    for (int i = 0; i < 3; ++i) key = (key << 1) | ((X[i] >> b) & 1u);
  return key;
}

// internal -> host: the nodes sorted by the Hilbert index of their position in the scene's bounding cube, ties by host id
std::vector<uint32_t> hilbert_order(const pies_solver* s) {
  const uint32_t n = s->nodeCount();
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const double v = s->h_pos[3ull * i + a];
      if (std::isfinite(v)) { lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v); }
    }
  double ext = 0.0;
  for (int a = 0; a < 3; ++a)
    if (hi[a] > lo[a]) ext = std::max(ext, hi[a] - lo[a]);
  const double cells = static_cast<double>((1u << kCurveBits) - 1u);
  std::vector<std::pair<uint64_t, uint32_t>> key(n);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) {
      const double v = s->h_pos[3ull * i + a];
      const double c = std::isfinite(v) && ext > 0.0 ? (v - lo[a]) / ext * cells : 0.0;
      q[a] = static_cast<uint32_t>(std::min(std::max(c, 0.0), cells));
    }
    key[i] = {hilbert_key(q[0], q[1], q[2]), i};
  }
  std::sort(key.begin(), key.end());
  std::vector<uint32_t> order(n);
  for (uint32_t k = 0; k < n; ++k) order[k] = key[k].second;
  return order;
}

// Halo entries of the windowed matrix over all chunks of R rows (what PIES_PD_WINDOW_HALO counts), with row k of the matrix being
// host row order[k] (order empty: the identity)
uint64_t window_halo(const PdSystem& K, uint32_t R, const std::vector<uint32_t>& order, const std::vector<uint32_t>& inv) {
  const uint32_t n = static_cast<uint32_t>(K.kdiag.size());
  const bool perm = !order.empty();
  uint64_t halo = 0;
  std::vector<uint32_t> cols;
  for (uint32_t r0 = 0; r0 < n; r0 += R) {
    const uint32_t r1 = std::min(n, r0 + R);
    cols.clear();
    for (uint32_t r = r0; r < r1; ++r) {
      const uint32_t row = perm ? order[r] : r;
      for (uint32_t k = K.rowptr[row]; k < K.rowptr[row + 1]; ++k) {
        const uint32_t j = perm ? inv[K.col[k]] : K.col[k];
        if (j < r0 || j >= r1) cols.push_back(j);
      }
    }
    std::sort(cols.begin(), cols.end());
    halo += static_cast<uint64_t>(std::unique(cols.begin(), cols.end()) - cols.begin());
  }
  return halo;
}

template <class T> void translate_ids(std::vector<T>& list, const std::vector<uint32_t>& inv) {
  for (T& c : list)
    for (uint32_t& id : c.ids) id = inv[id];
}

template <class T> void gather_nodes(std::vector<T>& a, const std::vector<uint32_t>& order, size_t stride) {
  std::vector<T> out(a.size());
  for (size_t k = 0; k < order.size(); ++k)
    for (size_t c = 0; c < stride; ++c) out[stride * k + c] = a[stride * order[k] + c];
  a.swap(out);
}
}  // namespace

void decide_node_order(pies_solver* s) {
  s->nodeOrder = NodeOrder{};
  const uint32_t n = s->nodeCount();
  if (!s->renumberNodes || s->opt.solver != PIES_SOLVER_PD || n < 2 || s->h_pos.size() != 3ull * n) return;
  PdSystem K;
  pd_assemble(s, K);
  if (pd_row_dictionary_applies(K)) return;  // a lattice: its order is the one the row dictionary needs
  NodeOrder cand;
  cand.order = hilbert_order(s);
  cand.inv.resize(n);
  for (uint32_t k = 0; k < n; ++k) cand.inv[cand.order[k]] = k;
  const uint32_t R = pd_window_chunk_rows();
  const uint64_t before = window_halo(K, R, {}, {});
  const uint64_t after = window_halo(K, R, cand.order, cand.inv);
  if (after < before && static_cast<double>(after) <= kHaloRatio * static_cast<double>(before)) s->nodeOrder = std::move(cand);
}

InternalNumbering::InternalNumbering(pies_solver* s) {
  if (!s->nodeOrder.active() || s->internalIds || s->nodeOrder.order.size() != s->nodeCount()) return;
  s_ = s;
  const std::vector<uint32_t>& order = s->nodeOrder.order;
  const std::vector<uint32_t>& inv = s->nodeOrder.inv;
  // the host numbering is kept here; the solver gets translated copies
  pos_ = s->h_pos; prev_ = s->h_prev; vel_ = s->h_vel; radius_ = s->h_radius; invMass_ = s->h_invMass;
  position_ = s->h_position; distance_ = s->h_distance; tet_ = s->h_tet; volume_ = s->h_volume; bend_ = s->h_bend;
  nodePair_ = s->h_nodePair; shape_ = s->h_shape; goal_ = s->h_goal; triangles_ = s->h_triangles; lines_ = s->h_lines;
  gather_nodes(s->h_pos, order, 3);
  gather_nodes(s->h_prev, order, 3);
  gather_nodes(s->h_vel, order, 3);
  gather_nodes(s->h_radius, order, 1);
  gather_nodes(s->h_invMass, order, 1);
  for (HostPosition& c : s->h_position) c.id = inv[c.id];
  translate_ids(s->h_distance, inv);
  translate_ids(s->h_tet, inv);
  translate_ids(s->h_volume, inv);
  translate_ids(s->h_bend, inv);
  translate_ids(s->h_nodePair, inv);
  // shape and goal groups: element by element, in their order; the material coordinates are the host's, untouched
  for (HostShape& c : s->h_shape) for (uint32_t& id : c.ids) id = inv[id];
  for (HostGoal& c : s->h_goal) for (uint32_t& id : c.ids) id = inv[id];
  for (uint32_t& id : s->h_triangles) id = inv[id];
  for (uint32_t& id : s->h_lines) id = inv[id];
  s->internalIds = true;
}

InternalNumbering::~InternalNumbering() {
  if (!s_) return;
  pies_solver* s = s_;
  s->h_pos.swap(pos_); s->h_prev.swap(prev_); s->h_vel.swap(vel_); s->h_radius.swap(radius_); s->h_invMass.swap(invMass_);
  s->h_position.swap(position_); s->h_distance.swap(distance_); s->h_tet.swap(tet_); s->h_volume.swap(volume_);
  s->h_bend.swap(bend_); s->h_nodePair.swap(nodePair_); s->h_shape.swap(shape_); s->h_goal.swap(goal_);
  s->h_triangles.swap(triangles_); s->h_lines.swap(lines_);
  s->internalIds = false;
}

}  // namespace pies

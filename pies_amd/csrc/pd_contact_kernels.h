// Launch wrappers of the PD node-node contact pipeline (pd_contact_kernels.hip; PIES_FLAG_PD_NODE_CONTACTS).
//
// Once per substep, after k_pd_predict: the node grid of the PBD pass is built from the predicted positions (launch_hash_build)
// and every node's lane lists its contact partners - nodes that share a cell, overlap, are not both pinned and are not joined by
// an element - in ascending order of the pair key (pair_mix below, over the host's ids).  The list feeds the diagonal of the system (w once per
// contact), the right-hand side of every local step (w * projected, summed in list order) and the friction loop of
// Solver.cpp:398-428, executed in ascending pair-key order by rounds: a pair runs when it is the next unprocessed pair of both its
// nodes.  No float atomics anywhere: the results are the same bit for bit from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hash_kernels.h"
#include "pd_kernels.h"

namespace pies {

constexpr uint32_t kNcDefaultPartners = 32;  // PIES_PD_NODE_CONTACT_PARTNERS
constexpr uint32_t kNcMaxRounds = 256;       // friction rounds captured at most (a tail kernel finishes deeper orders)
constexpr uint32_t kNcDeepest = kNcMaxRounds + 1;  // ctl word: most rounds a friction pass needed since the host last looked
constexpr uint32_t kNcCtlWords = kNcMaxRounds + 2;
constexpr uint32_t kNcOverflowFlag = 1024u;  // failure word bit (the node grid's word, hash_kernels.h): a partner list overflowed

struct NodeContactArrays {
  uint32_t n;
  uint32_t cap;               // partners per node
  uint32_t rounds;            // friction round launches captured (>= 1)
  const uint32_t* adjPtr;     // n + 1: nodes joined to node i by an element, ascending, in adj[adjPtr[i] .. adjPtr[i + 1])
  const uint32_t* adj;
  uint32_t* part;             // n x cap: node i's partners, ascending pair key
  uint32_t* cnt;              // n: partners listed (<= cap)
  uint32_t* cur[2];           // n: the friction pass's cursors into the lists (ping-pong between rounds)
  uint32_t* ctl;              // [r]: round r - 1 left a pair unprocessed; [kNcDeepest]
  const uint32_t* flags;      // the node grid's failure word (kNcOverflowFlag: a list was cut short, the friction pass is skipped)
  const uint32_t* hostId;     // n: the host's id of device node i (nullptr: the device holds the host's numbering)
};

// 64-bit mix of the pair {i < j} (murmur3's finaliser over i << 32 | j, the mix of the PBD pair order's key): a bijection, so no
// two pairs tie.  Always taken over the HOST's ids (NodeContactArrays::hostId): the friction order, and with it the velocities, do
// not depend on whether pies_finalize renumbered the nodes
__host__ __device__ inline uint64_t pair_mix(uint32_t i, uint32_t j) {
  uint64_t k = (static_cast<uint64_t>(i < j ? i : j) << 32) | (i < j ? j : i);
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// detection + the diagonal (w = kNodePairW once per contact into cdiag, then dinv); after launch_hash_build and after the
// point-triangle detection, which adds to cdiag as well.  1 launch.
uint32_t launch_nc_detect(hipStream_t st, const HashArrays& H, const NodeContactArrays& C, const NodeArrays& nd, const float* kdiag,
                          float* cdiag, float* dinv);
// local step: rhs[i] += sum over i's contacts of w * projected_i (CollisionConstraint.cpp:10-41, 49-65).  After the right-hand
// side is formed (launch_pd_rhs).  1 launch.
uint32_t launch_nc_rhs(hipStream_t st, const NodeContactArrays& C, const NodeArrays& nd, float4* rhs);
// friction (Solver.cpp:398-428) in ascending pair-key order, then the floor friction (Solver.cpp:473-484) of the contacts' nodes
// that are in no point-triangle contact (usedBits; nullptr: none).  C.rounds + 2 launches.
uint32_t launch_nc_friction(hipStream_t st, const NodeContactArrays& C, const HashArrays& H, const NodeArrays& nd, const uint32_t* nstatic,
                            const uint32_t* usedBits, float friction, float staticThreshold);

}  // namespace pies

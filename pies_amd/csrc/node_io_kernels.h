// pies_read_nodes_device / pies_write_nodes_device (extensions, pies_hip.h): node state between HBM and caller arrays in device
// memory, in HOST numbering.  Launch wrappers like kernels.h: no allocation, no synchronisation, everything on the given stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

namespace pies {

constexpr uint32_t kNodeIoTile = 256;  // host ids per workgroup (= its lanes)

// One call's arrays.  user[0..2]: position, previous position, velocity in caller memory, `stride` floats per node, nullptr: not
// part of the call; 4-byte aligned, nothing more is assumed (the kernels look at the base themselves).
struct NodeIoPass {
  NodeArrays nd;
  const uint32_t* inv;  // d_nodeInv: host id -> device index (nullptr: identity)
  float* user[3];
  float *radius, *invMass;  // reads only: one float per node, nullptr: not wanted
  const uint32_t* ids;      // indexed writes only: m host ids in device memory
  uint32_t m;               // ... and their number
  uint32_t stride;          // 3 or 4
  bool staged;              // stride 3: a tile's 768 floats pass through LDS and cross as 16-byte accesses where the base allows
};

// user[a][i] = x, y, z (, 0) of node i's record in array a; radius[i], invMass[i] = its radius and pos.w.  One launch.
void launch_node_io_read(hipStream_t st, const NodeIoPass& P);
// The mirror image: the x, y, z of node i's record in array a = user[a][i]; pos.w stays, prev.w and vel.w become 0.  One launch.
// With P.ids row k goes to node ids[k] (one lane per row; an id >= nd.n is skipped), else row k to node k.
void launch_node_io_write(hipStream_t st, const NodeIoPass& P);

}  // namespace pies

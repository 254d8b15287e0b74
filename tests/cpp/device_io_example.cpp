// Solver::readNodesDevice / writeNodesDevice through the drop-in class, from a host program that owns device memory and a stream
// of its own (HIP interop): the positions arrive in a hipMalloc'ed array on the program's stream and equal getVertices(); the
// velocities are replaced from device memory and the next tick starts from them.  Needs the HIP runtime for hipMalloc, so
// tests/test_device_io_cpp.py builds it with hipcc.  Exit code 0 on success.
#include <Pies/Solver.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define HIP_OK(expr)                                                       \
  do {                                                                     \
    if ((expr) != hipSuccess) {                                            \
      std::printf("device io FAILED: %s\n", #expr);                        \
      return 2;                                                            \
    }                                                                      \
  } while (0)

int main() {
  Pies::SolverOptions options;
  options.solver = Pies::SolverName::PBD;
  options.iterations = 4;
  Pies::Solver s(options);
  s.createTetBox(glm::vec3(0.25f, 1.5f, 0.5f), 1.0f, glm::vec3(0.0f, 0.0f, 0.0f), 1.0f, 1.0f, false);
  s.tick(0.0f);
  const uint32_t n = static_cast<uint32_t>(s.getVertices().size());
  if (n == 0) return 3;

  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  float *dPos = nullptr, *dVel = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dPos), 4ull * n * sizeof(float)));
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dVel), 3ull * n * sizeof(float)));

  // read: stride 4, ordered on the program's stream behind its own memset and before its own copy; one synchronisation
  std::vector<float> pos(4ull * n, -1.0f);
  HIP_OK(hipMemsetAsync(dPos, 0xFF, 4ull * n * sizeof(float), stream));
  pies_device_nodes_t io;
  std::memset(&io, 0, sizeof(io));
  io.position = dPos;
  io.stride = 4;
  s.readNodesDevice(io, stream);
  HIP_OK(hipMemcpyAsync(pos.data(), dPos, 4ull * n * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  for (uint32_t i = 0; i < n; ++i) {
    const glm::vec3 p = s.getVertices()[i].position;
    if (pos[4 * i] != p[0] || pos[4 * i + 1] != p[1] || pos[4 * i + 2] != p[2] || pos[4 * i + 3] != 0.0f) {
      std::printf("device io FAILED: node %u differs from getVertices()\n", i);
      return 4;
    }
  }

  // write: every node gets the velocity (0, 0, 2) from device memory; one tick without gravity moves the body along z by 2 dt
  std::vector<float> vel(3ull * n, 0.0f);
  for (uint32_t i = 0; i < n; ++i) vel[3 * i + 2] = 2.0f;
  HIP_OK(hipMemcpyAsync(dVel, vel.data(), 3ull * n * sizeof(float), hipMemcpyHostToDevice, stream));
  std::memset(&io, 0, sizeof(io));
  io.velocity = dVel;
  io.stride = 3;
  s.writeNodesDevice(io, nullptr, 0, stream);
  std::vector<float> back(3ull * n, -1.0f);
  if (pies_read_nodes(s.handle(), PIES_NODE_VELOCITY, back.data(), n) != PIES_OK) return 5;
  if (back != vel) {
    std::printf("device io FAILED: pies_read_nodes does not see the device write\n");
    return 5;
  }
  // a radius cannot be written on the device
  io.radius = dVel;
  bool threw = false;
  try { s.writeNodesDevice(io, nullptr, 0, stream); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) return 6;

  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipFree(dPos));
  HIP_OK(hipFree(dVel));
  HIP_OK(hipStreamDestroy(stream));
  std::printf("device io ok: %u nodes read into and written from device memory\n", n);
  return 0;
}

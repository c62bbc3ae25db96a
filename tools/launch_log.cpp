// launch_log.cpp — what the subgroup, wave and generic launchers would enqueue, without a GPU.
// The program defines the few HIP entry points a launcher calls (the <<<>>> call configuration,
// hipLaunchKernel, hipFuncSetAttribute, hipGetDevice, hipGetLastError), so the library's calls bind
// to them, and prints for every call of a family's launch entry over a grid of (n, m, mode, batch,
// layout, flags) the answer and each launch: the kernel's symbol, grid, workgroup size, dynamic LDS
// bytes and the LDS grants.  Two builds of the library launch the same kernels with the same LDS
// sizes exactly when their outputs are equal (a kernel trace reports a kernel's static LDS only).
//   usage: launch_log path/to/libqpgpu.so > log.txt     (profiles/wave_launch/README.md)
// Host code only, and no device is touched (built and run where there is no GPU):
//   hipcc --cuda-host-only -std=c++17 -rdynamic -o tools/launch_log tools/launch_log.cpp -ldl
// A diagnostic of its day, not a product tool: __hipPushCallConfiguration and
// __hipPopCallConfiguration are how this hipcc lowers <<<>>>, not a documented interface.  If a
// later compiler lowers a launch another way, the library's launches no longer arrive here; the
// program then ends with an error instead of an empty log (see the end of main).
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../motion-generation-using-quadratic-programs_amd/csrc/qp_common.h"

static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;

static long g_launches = 0;

static std::string symbol_of(const void* f) {
  Dl_info info;
  return dladdr(f, &info) && info.dli_sname ? info.dli_sname : "?";
}

extern "C" {
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
  g_grid = grid, g_block = block, g_shmem = shmem, g_stream = stream;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
  *grid = g_grid, *block = g_block, *shmem = g_shmem, *stream = g_stream;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t shmem, hipStream_t) {
  g_launches++;
  std::printf("  launch %s grid %u,%u,%u wg %u,%u,%u lds %zu\n", symbol_of(f).c_str(), grid.x, grid.y, grid.z,
              block.x, block.y, block.z, shmem);
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute attr, int value) {
  std::printf("  attribute %d of %s = %d\n", (int)attr, symbol_of(f).c_str(), value);
  return hipSuccess;
}
hipError_t hipGetDevice(int* dev) {
  *dev = 0;
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return std::fprintf(stderr, "%s\n", dlerror()), 2;
  using Launch2 = hipError_t (*)(const qpk::QpArgs*, hipStream_t);
  using Launch3 = hipError_t (*)(const qpk::QpArgs*, hipStream_t, double*);
  static double buf[16];  // what every non-NULL pointer points at; never read through
  const struct {
    const char* name;
    bool ws;
  } entries[] = {{"qpk_launch_small", false},       {"qpk_launch_small_unit", false},
                 {"qpk_launch_medium", true},       {"qpk_launch_medium_fast", false},
                 {"qpk_launch_medium_unit", false}, {"qpk_launch_generic", true}};
  const int ms[] = {0, 4, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1024, 1025, -2 /* 2n */};
  const uint32_t flag_sets[] = {0, QPGPU_FLAG_EXACT, QPGPU_FLAG_WRITE_FACTOR};
  for (const auto& e : entries) {
    void* fn = dlsym(lib, e.name);
    if (!fn) return std::fprintf(stderr, "%s: not exported\n", e.name), 2;
    for (int n = 1; n <= 257; n = n < 66 ? n + 1 : (n < 256 ? 256 : n + 1))
      for (const int mm : ms)
        for (int mode = 0; mode < 4; mode++)
          for (const int64_t batch : {(int64_t)1, (int64_t)5, (int64_t)130})
            for (const int tile : {1, 64})
              for (const uint32_t flags : flag_sets) {
                const int m = mm == -2 ? 2 * n : mm;
                if (flags && (std::strcmp(e.name, "qpk_launch_medium") != 0 || n <= 64)) continue;  // read there only
                qpk::QpArgs a = {};
                a.n = n, a.p = 2, a.m = m, a.max_steps = 100, a.tile = tile, a.batch = batch, a.flags = flags;
                a.G = buf, a.g0 = a.CE = a.ce0 = a.CI = a.ci0 = buf, a.x = a.f = buf;
                a.status = reinterpret_cast<int32_t*>(buf);
                if (mode & qpk::kDual) a.u = buf;
                if (mode & qpk::kBox) a.hi = a.lo = buf;
                std::printf("%s n=%d m=%d mode=%d batch=%lld tile=%d flags=%#x\n", e.name, n, m, mode,
                            (long long)batch, tile, flags);
                const hipError_t rc = e.ws ? reinterpret_cast<Launch3>(fn)(&a, nullptr, buf)
                                           : reinterpret_cast<Launch2>(fn)(&a, nullptr);
                std::printf("  -> %d\n", (int)rc);
              }
  }
  if (g_launches == 0) return std::fprintf(stderr, "no launch of the library arrived here: see the header\n"), 3;
  return 0;
}

// stream_hold.hip -- test-only helper of tests/test_gpu_ordering.py: hold a stream back for a bounded time, so that work
// which is NOT ordered behind the held stream is certain to overtake it.  Built by the test module
// (hipcc --offload-arch=gfx950 -O2 -fPIC -shared) and loaded with ctypes; not part of libspecan_hip.so.
//
//   stream_hold(ms, stream)   one 64-lane wave on `stream` waits until `ms` milliseconds have passed on the constant
//                             100 MHz counter (as sa_spin_kernel of sa_streams.cpp does).  The wait ends on the counter or
//                             on an iteration cap proportional to `ms`, whichever comes first, so it cannot hang.  It reads
//                             and writes no memory.  ms > 100 is refused before any launch.
// Returns 0, or the hipError_t of the refusal / the launch.
#include <hip/hip_runtime.h>

namespace {

constexpr unsigned kMaxMs = 100;
constexpr unsigned kTicksPerMs = 100000;          // the counter runs at 100 MHz whatever the shader clock does
// One iteration sleeps 127 * 64 = 8128 shader clocks: 3.4 us at 2.4 GHz, longer at any lower clock.  600 iterations per
// millisecond therefore always reach the counter's limit first (600 * 3.4 us = 2.0 ms), and if the counter stood still
// the cap would end the wait after 600 * ms iterations: 2.3 ms per ms at 2.1 GHz, and 1 s for the longest hold at 0.5 GHz.
constexpr unsigned kItersPerMs = 600;

__global__ __launch_bounds__(64) void stream_hold_kernel(unsigned ticks, unsigned cap)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (unsigned i = 0; i < cap && __builtin_amdgcn_s_memrealtime() - t0 < ticks; ++i) __builtin_amdgcn_s_sleep(127);
}

}  // namespace

extern "C" int stream_hold(unsigned ms, void *stream)
{
    if (ms > kMaxMs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_hold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ms * kTicksPerMs, ms * kItersPerMs);
    return hipGetLastError();
}

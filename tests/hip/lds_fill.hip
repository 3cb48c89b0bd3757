// lds_fill.hip -- test-only helper of tests/test_gpu_isolation.py: poison the LDS of every CU, and probe what a later
// dispatch finds there.  Built by the test module (hipcc --offload-arch=gfx950 -O2 -fPIC -shared) and loaded with ctypes;
// not part of libspecan_hip.so.
//
//   lds_fill(word, grid, stream)           grid workgroups, each holding all 160 KiB of the CU's LDS, write `word` to
//                                          every 32-bit word (ordinary 16-byte LDS writes).
//   lds_probe(word, grid, counts, stream)  grid such workgroups READ all 160 KiB without writing it and count the words
//                                          that differ from `word`: counts[4 * workgroup + wave], one count per wave.
// Both return the hipError_t of the launch (0 = hipSuccess).  The accesses are volatile so that the compiler keeps the
// writes nobody in the kernel reads, and does not fold the reads of LDS the kernel never wrote.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;                 // all of a CU's LDS on gfx950
constexpr int kVec = kLdsBytes / 16;                  // 16-byte words per workgroup
static_assert(kVec % kThreads == 0, "every thread covers the same number of 16-byte words");

// 16 bytes of LDS, addressed as LDS (ds_write_b128 / ds_read_b128, not flat accesses)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef volatile __attribute__((address_space(3))) u32x4 lds_u32x4;

__global__ __launch_bounds__(kThreads) void lds_fill_kernel(uint32_t word)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 lds[];
    lds_u32x4 *v = (lds_u32x4 *)lds;
    const u32x4 w = {word, word, word, word};
    for (int i = threadIdx.x; i < kVec; i += kThreads) v[i] = w;
}

__global__ __launch_bounds__(kThreads) void lds_probe_kernel(uint32_t word, uint32_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 lds[];
    const lds_u32x4 *v = (const lds_u32x4 *)lds;
    uint32_t bad = 0;
    for (int i = threadIdx.x; i < kVec; i += kThreads) {
        const u32x4 x = v[i];
        bad += (x.x != word) + (x.y != word) + (x.z != word) + (x.w != word);
    }
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);    // wave reduction, in registers
    if ((threadIdx.x & 63) == 0) counts[blockIdx.x * kWaves + (threadIdx.x >> 6)] = bad;
}

hipError_t allow_full_lds(const void *kern, bool *done)
{
    if (*done) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e == hipSuccess) *done = true;
    return e;
}

}  // namespace

extern "C" int lds_fill(uint32_t word, int grid, void *stream)
{
    static bool attr = false;
    hipError_t e = allow_full_lds(reinterpret_cast<const void *>(lds_fill_kernel), &attr);
    if (e != hipSuccess) return e;
    if (grid <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lds_fill_kernel, dim3(grid), dim3(kThreads), kLdsBytes, (hipStream_t)stream, word);
    return hipGetLastError();
}

extern "C" int lds_probe(uint32_t word, int grid, uint32_t *counts, void *stream)
{
    static bool attr = false;
    hipError_t e = allow_full_lds(reinterpret_cast<const void *>(lds_probe_kernel), &attr);
    if (e != hipSuccess) return e;
    if (grid <= 0 || !counts) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lds_probe_kernel, dim3(grid), dim3(kThreads), kLdsBytes, (hipStream_t)stream, word, counts);
    return hipGetLastError();
}

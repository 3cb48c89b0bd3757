// chain_f32.hip -- the float chain on float32 frames (sa_process_f32); the kernels are in chain_f32.hpp.
#include "chain_f32.hpp"

hipError_t sa_launch_chain_f32(const float *in, void *out, int batch, int out_kind, const SaF32Tables &tb,
                               hipStream_t stream, SaLaunchEv ev)
{
    return launch_chain(out, batch, out_kind, tb, stream, ev, in);
}

// phase stamps of the float32 kernels (make stamps); chain_f32_i16.hip's kernels have a stamp table of their own that
// nothing sets, so they record none
#ifdef SA_STAMPS
extern "C" int sa_debug_set_stamps(void *p)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_sa_stamps), &p, sizeof(p));
}
#endif

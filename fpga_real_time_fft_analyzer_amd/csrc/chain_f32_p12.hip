// chain_f32_p12.hip -- the float chain on packed 12-bit samples (sa_process_f32_p12, 24576 bytes per frame): unpacked,
// converted and scaled (x = float(sample) * in_scale) in the stage-in, then exactly the float32 path (chain_f32.hpp).
// A translation unit of its own, compiled beside chain_f32.hip and chain_f32_i16.hip.
#include "chain_f32.hpp"

hipError_t sa_launch_chain_f32_p12(const uint8_t *in, float in_scale, void *out, int batch, int out_kind,
                                   const SaF32Tables &tb, hipStream_t stream, SaLaunchEv ev)
{
    return launch_chain(out, batch, out_kind, tb, stream, ev, reinterpret_cast<const SaP12 *>(in), in_scale);
}

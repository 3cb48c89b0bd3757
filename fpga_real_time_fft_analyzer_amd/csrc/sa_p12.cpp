// sa_p12.cpp -- host helpers of the packed 12-bit sample format (include/specan.h, "p12"): pure functions, no handle, no
// GPU.  Sample n occupies bits [12n, 12n+12) of the packed bytes read as a little-endian bit stream, so a pair of
// samples is three bytes; the arithmetic is explicit byte arithmetic, independent of the host's byte order.
#include "../../include/specan.h"

extern "C" {

int sa_pack_samples_p12(const int16_t *samples, size_t n, uint8_t *packed)
{
    if ((n & 1) != 0 || (n != 0 && (!samples || !packed))) return SA_EINVAL;
    for (size_t i = 0; i < n; ++i)                             // checked before anything is written
        if (samples[i] < -2048 || samples[i] > 2047) return SA_EINVAL;
    for (size_t i = 0; i < n / 2; ++i) {
        const unsigned u0 = (unsigned)samples[2 * i] & 0xFFFu, u1 = (unsigned)samples[2 * i + 1] & 0xFFFu;
        packed[3 * i] = (uint8_t)(u0 & 0xFFu);
        packed[3 * i + 1] = (uint8_t)((u0 >> 8) | ((u1 & 0xFu) << 4));
        packed[3 * i + 2] = (uint8_t)(u1 >> 4);
    }
    return SA_OK;
}

int sa_unpack_samples_p12(const uint8_t *packed, size_t n, int16_t *samples)
{
    if ((n & 1) != 0 || (n != 0 && (!samples || !packed))) return SA_EINVAL;
    for (size_t i = 0; i < n / 2; ++i) {
        const unsigned b0 = packed[3 * i], b1 = packed[3 * i + 1], b2 = packed[3 * i + 2];
        const unsigned u0 = b0 | ((b1 & 0xFu) << 8), u1 = (b1 >> 4) | (b2 << 4);
        samples[2 * i] = (int16_t)((int)(u0 ^ 0x800u) - 0x800);         // sign extension of 12 bits
        samples[2 * i + 1] = (int16_t)((int)(u1 ^ 0x800u) - 0x800);
    }
    return SA_OK;
}

}  // extern "C"

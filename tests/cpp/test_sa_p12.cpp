// Stand-alone host test of the packed 12-bit sample helpers (csrc/sa_p12.cpp; the format is defined in include/specan.h).
// No GPU, no library: compiled together with sa_p12.cpp by tests/test_p12_host.py, under the address and
// undefined-behaviour sanitizers where they link.  Every output buffer is allocated at its exact size, so a write past
// 3n/2 bytes (or n samples) is an error the sanitizer reports.  Prints "ok <checks>" and returns 0, or names the first
// failed check and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/specan.h"

static int g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// the format's definition, sample by sample: bits [12n, 12n+12) of the little-endian bit stream
static int16_t sample_at(const std::vector<uint8_t> &b, size_t n)
{
    unsigned v = 0;
    for (int k = 0; k < 12; ++k) {
        const size_t bit = 12 * n + (size_t)k;
        v |= (unsigned)((b[bit >> 3] >> (bit & 7)) & 1u) << k;
    }
    return (int16_t)((int)(v ^ 0x800u) - 0x800);
}

static int round_trip(const std::vector<int16_t> &s)
{
    std::vector<uint8_t> p(3 * s.size() / 2);
    CHECK(sa_pack_samples_p12(s.data(), s.size(), p.data()) == SA_OK);
    for (size_t n = 0; n < s.size(); ++n) CHECK(sample_at(p, n) == s[n]);
    std::vector<int16_t> r(s.size());
    CHECK(sa_unpack_samples_p12(p.data(), s.size(), r.data()) == SA_OK);
    CHECK(r == s);
    return 0;
}

int main()
{
    // known answers
    {
        const int16_t a[2] = {0x123, 0x456}, b[2] = {-1, -2048};
        uint8_t p[3];
        CHECK(sa_pack_samples_p12(a, 2, p) == SA_OK && p[0] == 0x23 && p[1] == 0x61 && p[2] == 0x45);
        CHECK(sa_pack_samples_p12(b, 2, p) == SA_OK && p[0] == 0xFF && p[1] == 0x0F && p[2] == 0x80);
        int16_t r[2];
        CHECK(sa_unpack_samples_p12(p, 2, r) == SA_OK && r[0] == -1 && r[1] == -2048);
    }
    // random samples (a fixed linear congruential sequence), the alternating extremes and the ramp
    {
        std::vector<int16_t> s(4096);
        uint32_t x = 12345u;
        for (auto &v : s) {
            x = x * 1664525u + 1013904223u;
            v = (int16_t)((int)(x >> 20) - 2048);
        }
        if (round_trip(s)) return 1;
        for (size_t n = 0; n < s.size(); ++n) s[n] = (n & 1) ? 2047 : -2048;
        if (round_trip(s)) return 1;
        for (size_t n = 0; n < s.size(); ++n) s[n] = (int16_t)((int)((37 * n) % 4096) - 2048);
        if (round_trip(s)) return 1;
        if (round_trip(std::vector<int16_t>())) return 1;           // n = 0
    }
    // every three-byte pattern unpacks to the two samples the bit stream defines, and packs back to itself
    {
        std::vector<uint8_t> p(3);
        for (unsigned v = 0; v < (1u << 24); ++v) {
            p[0] = (uint8_t)v;
            p[1] = (uint8_t)(v >> 8);
            p[2] = (uint8_t)(v >> 16);
            int16_t r[2];
            uint8_t q[3];
            if (sa_unpack_samples_p12(p.data(), 2, r) != SA_OK || r[0] != sample_at(p, 0) || r[1] != sample_at(p, 1) ||
                sa_pack_samples_p12(r, 2, q) != SA_OK || std::memcmp(q, p.data(), 3) != 0) {
                std::printf("FAILED pattern %06x\n", v);
                return 1;
            }
        }
        ++g_checks;
    }
    // errors: odd n, 2048, -2049; the packer checks before it writes
    {
        std::vector<int16_t> s(8, 5);
        std::vector<uint8_t> p(12, 0xEE);
        const std::vector<uint8_t> untouched(12, 0xEE);
        CHECK(sa_pack_samples_p12(s.data(), 7, p.data()) == SA_EINVAL && p == untouched);
        s[7] = 2048;
        CHECK(sa_pack_samples_p12(s.data(), 8, p.data()) == SA_EINVAL && p == untouched);
        s[7] = -2049;
        CHECK(sa_pack_samples_p12(s.data(), 8, p.data()) == SA_EINVAL && p == untouched);
        s[7] = 2047;
        CHECK(sa_pack_samples_p12(s.data(), 8, p.data()) == SA_OK && p != untouched);
        std::vector<int16_t> r(8, 77);
        CHECK(sa_unpack_samples_p12(p.data(), 7, r.data()) == SA_EINVAL && r == std::vector<int16_t>(8, 77));
        CHECK(sa_pack_samples_p12(nullptr, 2, p.data()) == SA_EINVAL);
        CHECK(sa_unpack_samples_p12(p.data(), 2, nullptr) == SA_EINVAL);
    }
    std::printf("ok %d\n", g_checks);
    return 0;
}

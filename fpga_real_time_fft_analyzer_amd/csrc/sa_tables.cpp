// sa_tables.cpp -- fills the constant tables the kernels index (layouts: sa_tables.hpp, SaF32Tables, SaQ15Tables).
#include "sa_tables.hpp"

#include <cmath>

void default_window_f64(std::vector<double> &w)
{
    w.resize(SA_NPTS);
    for (int i = 0; i < SA_NPTS; ++i)   // scripts/hann_coeff.py:3-4
        w[i] = 0.5 * (1.0 - std::cos(2.0 * M_PI * (double)i / (double)(SA_NPTS - 1)));
}

void default_rom(std::vector<int16_t> &rom)
{
    std::vector<double> w;
    default_window_f64(w);
    rom.resize(SA_NPTS);
    for (int i = 0; i < SA_NPTS; ++i) {   // scripts/hann_coeff.py:5 (rint, int16 wrap: quirk Q1)
        const double r = std::rint((w[i] - 0.5) * 65536.0);
        rom[i] = (int16_t)(uint16_t)((int32_t)r & 0xFFFF);
    }
}

void half_window(const std::vector<double> &w, std::vector<float> &half)
{
    half.resize(SA_NPTS);
    for (int i = 0; i < SA_NPTS; ++i) half[i] = (float)(0.5 * w[i]);
}

void pass_a_window(const std::vector<float> &half, std::vector<float> &pa)
{
    pa.resize(SA_NPTS);
    for (int p = 0; p < 16; ++p)
        for (int t = 0; t < 256; ++t) {
            float *o = &pa[(p * 256 + t) * 4];
            o[0] = half[512 * (2 * p) + 2 * t];
            o[1] = half[512 * (2 * p) + 2 * t + 1];
            o[2] = half[512 * (2 * p + 1) + 2 * t];
            o[3] = half[512 * (2 * p + 1) + 2 * t + 1];
        }
}

// Least-squares fit of (a0, a1) in double, then the residual against 1.5e-7 of the window's peak: Hann, Hamming and
// every other two-term cosine window pass, anything else (Blackman, Kaiser, rectangular with a taper, ...) keeps the
// table.
bool fit_cosine_window(const float *w, double out[2])
{
    const double theta = 2.0 * M_PI / (double)(SA_NPTS - 1);
    double s1 = 0, sc = 0, scc = 0, sw = 0, swc = 0, peak = 0;
    for (int n = 0; n < SA_NPTS; ++n) {
        const double c = -std::cos(theta * n), v = (double)w[n];
        s1 += 1.0; sc += c; scc += c * c; sw += v; swc += v * c;
        peak = std::fmax(peak, std::fabs(v));
    }
    const double det = s1 * scc - sc * sc;
    // (fmax skips a NaN entry, here and in the residual below; the sum `sw` does not)
    if (!(det > 0.0) || !(peak > 0.0) || !std::isfinite(peak) || !std::isfinite(sw)) return false;
    const double a0 = (sw * scc - swc * sc) / det, a1 = (s1 * swc - sc * sw) / det;
    double worst = 0;
    for (int n = 0; n < SA_NPTS; ++n) worst = std::fmax(worst, std::fabs((double)w[n] - (a0 - a1 * std::cos(theta * n))));
    if (!(worst <= 1.5e-7 * peak)) return false;
    out[0] = a0;
    out[1] = a1;
    return true;
}

void float_twiddles(std::vector<float4> &ta, std::vector<float4> &tb, std::vector<float2> &tc)
{
    ta = std::vector<float4>(6 * 256);
    tb = std::vector<float4>(8 * 16);
    tc = std::vector<float2>(25);
    auto w8192 = [](long e) {                          // exp(-2 pi i e / 8192), e reduced first (exact)
        const double a = -2.0 * M_PI * (double)(e % 8192) / 8192.0;
        return make_float2((float)std::cos(a), (float)std::sin(a));
    };
    for (int t = 0; t < 256; ++t) {                    // per-thread anchors (SaF32Tables::twT)
        const int k[10] = {1, 2, 3, 4, 5, 6, 7, 8, 16, 24};
        for (int i = 0; i < 5; ++i) {
            const float2 u = w8192((long)k[2 * i] * t), v = w8192((long)k[2 * i + 1] * t);
            ta[i * 256 + t] = make_float4(u.x, u.y, v.x, v.y);
        }
        const double ap = -2.0 * M_PI * (double)(4 * t) / 16384.0;
        const double an = -2.0 * M_PI * (double)(4 * ((t + 1) & 255)) / 16384.0;      // (1, 0) for t = 255
        ta[5 * 256 + t] = make_float4((float)std::cos(ap), (float)std::sin(ap), (float)std::cos(an), (float)std::sin(an));
    }
    for (int pp = 0; pp < 8; ++pp)
        for (int b = 0; b < 16; ++b) {
            const double a0 = -2.0 * M_PI * (double)(2 * pp * b) / 256.0;
            const double a1 = -2.0 * M_PI * (double)((2 * pp + 1) * b) / 256.0;
            tb[pp * 16 + b] = make_float4((float)std::cos(a0), (float)std::sin(a0), (float)std::cos(a1), (float)std::sin(a1));
        }
    for (int blk = 0; blk < 5; ++blk)                   // block 4 = bin 4096 only (the seam of the last group)
        for (int e = 0; e < 5; ++e) {
            const double ang = -2.0 * M_PI * (double)(1024 * blk + e) / 16384.0;
            tc[blk * 5 + e] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        }
}

bool q15_twiddles(std::vector<uint2> &tq, std::vector<uint4> &rec)
{
    tq = std::vector<uint2>(SA_NPTS);
    auto clamp16 = [](long v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); };
    for (int m = 0; m < SA_NPTS; ++m) {   // SA-FXFFT-1 twiddles: clamp16(rint(32768 cos)), clamp16(rint(-32768 sin))
        const double a = 2.0 * M_PI * (double)m / (double)SA_NPTS;
        const long wr = clamp16(std::lrint(32768.0 * std::cos(a))), wi = clamp16(std::lrint(-32768.0 * std::sin(a)));
        // second word (-wi, wr): the operand of the two-term dot product for the real part.  -wi does not fit
        // for wi = -32768 (exponents 4082..4110); the kernel never takes the second word of those entries
        // (fx_butterfly: `wide1`, `wide2`, `wide3`)
        const long nwi = -wi > 32767 ? 32767 : -wi;
        // (margins: 32768 sin = 32767.528 at 4082 and 4110, 32767.458 at 4081 and 4111; the threshold is .5)
        if (wi == -32768 && (m < 4082 || m > 4110)) return false;
        tq[m].x = ((uint32_t)wr & 0xFFFFu) | ((uint32_t)wi << 16);
        tq[m].y = ((uint32_t)nwi & 0xFFFFu) | ((uint32_t)wr << 16);
    }
    // One 32-byte record {w(e), w(2e), w(3e), pad} per butterfly of the stages whose exponents differ from lane to
    // lane: a lane's three twiddles are one contiguous read instead of three gathers at strides 8, 16 and 24 bytes.
    rec = std::vector<uint4>(2 * kSaTwRecs);
    for (int r = 0; r < kSaTwRecs; ++r) {
        const int e = r < 4096 ? r : (r < 5120 ? 4 * (r - 4096) : 16 * (r - 5120));
        rec[2 * r] = make_uint4(tq[e].x, tq[e].y, tq[2 * e].x, tq[2 * e].y);
        rec[2 * r + 1] = make_uint4(tq[3 * e].x, tq[3 * e].y, 0u, 0u);
    }
    return true;
}

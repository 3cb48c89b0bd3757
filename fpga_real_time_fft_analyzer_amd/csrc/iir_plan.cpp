// iir_plan.cpp -- the plan algebra of the IIR cascades (iir_plan.hpp): SOS in, plan tables out; pure host code.
#include "iir_plan.hpp"

#include <cmath>
#include <cstring>
#include <vector>

// imp/filter_pkg.vhd:54-68, wire order B0,B1,B2,A0,A1,A2 per set (ALPHA then BETA)
const int8_t kDefaultQ7[12] = {-14, 0, 14, 107, 21, 127, -15, 0, 15, 107, -21, 127};

namespace {

struct Mat2 {
    double a, b, c, d;
};
inline Mat2 mul(const Mat2 &x, const Mat2 &y)
{
    return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

inline Mat2 mpow(Mat2 m, int e)
{
    Mat2 r = {1, 0, 0, 1};
    while (e > 0) {
        if (e & 1) r = mul(r, m);
        m = mul(m, m);
        e >>= 1;
    }
    return r;
}

// Pole coordinates of one section (sa_common.hpp): M = T^-1 has the eigen-directions (1, a1 + lambda) as unit columns
// -- real and imaginary part for a complex pair -- and A = T A0 M is what predictor and scan work with.
// Two real poles whose eigen-directions lie closer than 0.1 rad (a double pole included) would make that basis
// ill-conditioned (cond ~ 1/angle: the float32 scan lost 1e3-1e4x against a sequential sosfilt at a pole gap of 1e-5,
// tests/test_plan_conditioning.py); they take the real Schur basis instead -- the first eigen-direction and its
// orthogonal complement, M orthonormal, A upper triangular.
void pole_coordinates(double a1, double a2, Mat2 *Mo, Mat2 *To, Mat2 *Ao)
{
    const Mat2 A0 = {-a1, 1.0, -a2, 0.0};
    Mat2 M = {1, 0, 0, 1};
    const double disc = a1 * a1 - 4.0 * a2;
    if (a2 != 0.0) {
        double c0[2], c1[2];
        if (disc < 0.0) {
            c0[0] = 1.0; c0[1] = 0.5 * a1;                 // Re (1, a1 + lambda), lambda = -a1/2 + i sqrt(-disc)/2
            c1[0] = 0.0; c1[1] = 0.5 * std::sqrt(-disc);   // Im
        } else {
            const double sq = std::sqrt(disc);
            c0[0] = 1.0; c0[1] = a1 + 0.5 * (-a1 + sq);
            c1[0] = 1.0; c1[1] = a1 + 0.5 * (-a1 - sq);
        }
        const double n0 = std::hypot(c0[0], c0[1]), n1 = std::hypot(c1[0], c1[1]);
        const Mat2 cand = {c0[0] / n0, c1[0] / n1, c0[1] / n0, c1[1] / n1};
        const double det = cand.a * cand.d - cand.b * cand.c;
        // unit columns: |det| = sine of the angle between them
        if (std::isfinite(det) && std::fabs(det) > (disc < 0.0 ? 1e-6 : 0.1))
            M = cand;
        else if (disc >= 0.0 && std::isfinite(cand.a) && std::isfinite(cand.c))
            M = {cand.a, -cand.c, cand.c, cand.a};
    }
    const double detM = M.a * M.d - M.b * M.c;
    const Mat2 T = {M.d / detM, -M.b / detM, -M.c / detM, M.a / detM};
    *Mo = M;
    *To = T;
    *Ao = mul(T, mul(A0, M));
}

// The section count the kernels are compiled for: 0, 2, 4 or 6 (shorter cascades are padded with identity sections)
int padded_sections(int nsec_in)
{
    return nsec_in == 0 ? 0 : (nsec_in <= 2 ? 2 : (nsec_in <= 4 ? 4 : 6));
}

// Padded section count, unit-numerator rewrite and folded gain shared by both plan layouts; returns the padded count.
int normalise_cascade(const double *sos_in, int nsec_in, double *sos /*[36]*/, bool *unit_out, double *gain_out)
{
    const int nsec = padded_sections(nsec_in);
    for (int s = 0; s < nsec; ++s)
        for (int i = 0; i < 6; ++i)
            sos[6 * s + i] = s < nsec_in ? sos_in[6 * s + i] : ((i == 0 || i == 3) ? 1.0 : 0.0);
    bool unit = nsec > 0 && nsec == nsec_in;
    double gain = 1.0;
    for (int s = 0; s < nsec && unit; ++s) {
        const double b0 = sos[6 * s], b2 = sos[6 * s + 2];
        if (b0 == 0.0 || b2 != b0 || !std::isfinite(1.0 / b0)) unit = false;
        gain *= b0;
    }
    if (unit && (!std::isfinite(gain) || std::fabs(gain) < 1e-30 || std::fabs(gain) > 1e30)) unit = false;
    if (unit) {
        for (int s = 0; s < nsec; ++s) {
            const double b0 = sos[6 * s];
            sos[6 * s + 1] /= b0;
            sos[6 * s] = 1.0;
            sos[6 * s + 2] = 1.0;
        }
    } else {
        gain = 1.0;
    }
    *unit_out = unit;
    *gain_out = gain;
    return nsec;
}

inline void put_cm(float *dst, const Mat2 &m)      // column-major
{
    dst[0] = (float)m.a; dst[1] = (float)m.c; dst[2] = (float)m.b; dst[3] = (float)m.d;
}

inline void put_rm(double *dst, const Mat2 &m)      // row-major
{
    dst[0] = m.a; dst[1] = m.b; dst[2] = m.c; dst[3] = m.d;
}

}  // namespace

// Build the predict/scan/recurse plan for an a0-normalised SOS (rows b0,b1,b2,1,a1,a2), double in.
// The kernels are compiled for 2, 4 and 6 sections; shorter cascades are padded with identity
// sections (b0 = 1, rest 0: y = x exactly, all scan matrices and predictor taps come out zero).
//
// Unit-numerator form: when no padding is needed and every section has b2 == b0 != 0 (all-pole-pair
// zeros on the unit circle: Butterworth / Chebyshev / elliptic low-, high-pass and band-stop), the
// sections are rewritten as b = [1, b1/b0, 1] and the product of the b0's is folded into this plan's
// copy of the window: one multiply less per sample and section in the recursion.
// half_win: 0.5 * window in natural order (size SA_NPTS).
// cosw: {a0, a1} when the window is a0 - a1 cos(2 pi n / (N-1)) (then the IIR kernels evaluate it in place,
// see SaIirLaneTab::wgen), null for any other window.
void build_plan(const double *sos_in, int nsec_in, SaIirK *plan, SaIirLaneTab *lt, const float *half_win,
                const double *cosw)
{
    std::memset(plan, 0, sizeof(*plan));
    std::memset(lt, 0, sizeof(*lt));
    double sos[36];
    bool unit;
    double gain;
    const int nsec = normalise_cascade(sos_in, nsec_in, sos, &unit, &gain);
    plan->nsec = nsec;
    plan->unit = unit ? 1 : 0;
    plan->gain = (float)gain;
    if (half_win)
        for (int t = 0; t < 256; ++t)
            for (int g = 0; g < 16; ++g)
                for (int e = 0; e < 4; ++e)
                    lt->win_t[(g * 256 + t) * 4 + e] = (float)((double)half_win[64 * t + 4 * g + e] * gain);
    plan->wingen = 0;
    if (half_win && cosw) {
        const double theta = 2.0 * M_PI / (double)(SA_NPTS - 1), S = 0.5 * gain;
        plan->wingen = 1;
        lt->wg0 = (float)(S * cosw[0]);
        for (int t = 0; t < SA_NTHREADS; ++t)
            for (int h = 0; h < 2; ++h) {
                const double a = theta * (double)(64 * t + 32 * h);
                lt->wgen[t][2 * h] = (float)(-S * cosw[1] * std::cos(a));
                lt->wgen[t][2 * h + 1] = (float)(S * cosw[1] * std::sin(a));
            }
        for (int j = 0; j < SA_CHUNK; ++j) {
            lt->wcs[j][0] = (float)std::cos(theta * j);
            lt->wcs[j][1] = (float)std::sin(theta * j);
        }
    }
    for (int s = 0; s < nsec; ++s) {
        const double *r = sos + 6 * s;
        const double b0 = r[0], b1 = r[1], b2 = r[2], a1 = r[4], a2 = r[5];
        SaIirSecK &sp = plan->sec[s];
        sp.c[0] = (float)b0; sp.c[1] = (float)b1; sp.c[2] = (float)b2; sp.c[3] = (float)a1; sp.c[4] = (float)a2;
        Mat2 M, T, A;
        pole_coordinates(a1, a2, &M, &T, &A);
        put_cm(sp.mback, M);
        double v0 = T.a * (b1 - a1 * b0) + T.b * (b2 - a2 * b0);      // T Bv
        double v1 = T.c * (b1 - a1 * b0) + T.d * (b2 - a2 * b0);
        float (*mdst)[2] = s == 0 ? plan->m0 : plan->sec[s - 1].mnext;       // taps of section s ride with section s-1
        for (int j = SA_PRED_TAPS - 1; j >= 0; --j) {     // m[j] = A^(15-j) Bv: the taps of a HALF chunk (block Horner)
            mdst[j][0] = (float)v0;
            mdst[j][1] = (float)v1;
            const double n0 = A.a * v0 + A.b * v1, n1 = A.c * v0 + A.d * v1;
            v0 = n0; v1 = n1;
        }
        put_cm(s == 0 ? plan->p16_0 : plan->sec[s - 1].p16next, mpow(A, SA_PRED_TAPS));
        const Mat2 Pc = mpow(A, SA_CHUNK);                  // one chunk
        const Mat2 P2 = mul(Pc, Pc);                        // one thread (two chunks)
        const Mat2 Prow = mpow(P2, 16);                     // one 16-lane row
        put_cm(sp.pc, Pc);
        Mat2 q = P2, qr = Prow;
        auto tiny = [](const Mat2 &m) {
            const double mx = std::fmax(std::fmax(std::fabs(m.a), std::fabs(m.b)), std::fmax(std::fabs(m.c), std::fabs(m.d)));
            return mx < 1e-10;
        };
        sp.flags = tiny(Prow) ? SA_IIR_SKIP_ROWSCAN : 0;
        for (int i = 0; i < 4; ++i) {                       // powers 1,2,4,8
            put_cm(sp.plev[i], q);
            put_cm(sp.prow[i], qr);
            if (tiny(q)) sp.flags |= 1 << i;
            q = mul(q, q);
            qr = mul(qr, qr);
        }
        Mat2 pw = {1, 0, 0, 1};
        for (int i = 0; i < 16; ++i) {                      // lanetab[s][i] = P2^i
            put_cm(lt->p[s][i], pw);
            pw = mul(pw, P2);
        }
    }
}

// The RTL taps as real numbers: y = (B2 x + B1 x1 + B0 x2 - A0 y2 - A1 y1)/128
// => scipy row [B2,B1,B0, 128, A1, A0] / 128; stages alternate set 0 / set 1 (filter_iir12_cust.vhd:68-240).
void sos_from_q7(const int8_t *c12, double *sos /*[6][6]*/)
{
    for (int k = 0; k < 6; ++k) {
        const int8_t *c = c12 + ((k & 1) ? 6 : 0);
        double *r = sos + 6 * k;
        r[0] = c[2] / 128.0; r[1] = c[1] / 128.0; r[2] = c[0] / 128.0;
        r[3] = 1.0; r[4] = c[4] / 128.0; r[5] = c[3] / 128.0;
    }
}


// The float64-state plan (SaIirF64, iir_f64.hip) of an a0-normalised SOS: DF2T coordinates, no unit-numerator rewrite,
// shorter cascades padded with identity sections (b0 = 1, rest 0: y = x exactly, every tap and power >= 2 is zero).
void build_plan_f64(const double *sos_in, int nsec_in, SaIirF64 *p)
{
    std::memset(p, 0, sizeof(*p));
    const int nsec = padded_sections(nsec_in);
    p->hdr[0] = (double)nsec;
    for (int s = 0; s < nsec; ++s) {
        const double ident[6] = {1, 0, 0, 1, 0, 0};
        const double *r = s < nsec_in ? sos_in + 6 * s : ident;
        const double b0 = r[0], b1 = r[1], b2 = r[2], a1 = r[4], a2 = r[5];
        SaIirSecF64 &k = p->sec[s];
        k.c[0] = b0; k.c[1] = b1; k.c[2] = b2; k.c[3] = a1; k.c[4] = a2;
        const Mat2 A = {-a1, 1.0, -a2, 0.0};
        double v0 = b1 - a1 * b0, v1 = b2 - a2 * b0;          // Bv
        for (int j = 15; j >= 0; --j) {                       // m[j] = A^(15-j) Bv
            k.m[j][0] = v0;
            k.m[j][1] = v1;
            const double n0 = A.a * v0 + A.b * v1, n1 = A.c * v0 + A.d * v1;
            v0 = n0; v1 = n1;
        }
        put_rm(k.p16, mpow(A, 16));
        const Mat2 Pc = mpow(A, SA_CHUNK);
        put_rm(k.pc, Pc);
        const Mat2 P2 = mul(Pc, Pc);
        Mat2 q = P2, qr = mpow(P2, 16);
        for (int i = 0; i < 4; ++i) {
            put_rm(k.plev[i], q);
            put_rm(k.prow[i], qr);
            q = mul(q, q);
            qr = mul(qr, qr);
        }
        Mat2 pw = {1, 0, 0, 1};
        for (int i = 0; i < 16; ++i) {
            put_rm(k.lane[i], pw);
            pw = mul(pw, P2);
        }
    }
}

// a0-normalised copy of a caller's SOS; false on a bad a0 (the checks of sa_load_sos_f64 / sa_iir_plan_from_sos)
bool normalise_a0(const double *sos, int n_sections, double *norm /*[36]*/)
{
    for (int s = 0; s < n_sections; ++s) {
        const double a0 = sos[6 * s + 3];
        if (a0 == 0.0 || !std::isfinite(a0)) return false;
        for (int i = 0; i < 6; ++i) norm[6 * s + i] = sos[6 * s + i] / a0;
    }
    return true;
}

// flat float view for tests (layout documented in include/specan.h, sa_iir_plan_from_sos): header, the six
// sections' constants, then the predictor taps m[6][16][2], their half-chunk matrices p16[6][4] and the per-lane
// matrices p[6][16][4] (every matrix row-major here)
int export_plan(const SaIirK &p, const SaIirLaneTab &lt, float *out, int cap)
{
    std::vector<float> v;
    auto put_i = [&](int x) { float f; std::memcpy(&f, &x, 4); v.push_back(f); };
    put_i(p.nsec); put_i(p.unit); v.push_back(p.gain); put_i(p.wingen);
    for (int s = 0; s < SA_MAXSEC; ++s) {
        const SaIirSecK &k = p.sec[s];
        for (int i = 0; i < 5; ++i) v.push_back(k.c[i]);
        put_i(k.flags); v.push_back(k.pad[0]); v.push_back(k.pad[1]);
        auto rm = [&](const float *m) { v.push_back(m[0]); v.push_back(m[2]); v.push_back(m[1]); v.push_back(m[3]); };   // stored column-major
        rm(k.pc);
        rm(k.mback);
        for (int i = 0; i < 4; ++i) rm(k.plev[i]);
        for (int i = 0; i < 4; ++i) rm(k.prow[i]);
    }
    for (int s = 0; s < SA_MAXSEC; ++s) {
        const float (*m)[2] = s == 0 ? p.m0 : p.sec[s - 1].mnext;
        v.insert(v.end(), &m[0][0], &m[0][0] + 2 * SA_PRED_TAPS);
    }
    for (int s = 0; s < SA_MAXSEC; ++s) {
        const float *m = s == 0 ? p.p16_0 : p.sec[s - 1].p16next;
        v.push_back(m[0]); v.push_back(m[2]); v.push_back(m[1]); v.push_back(m[3]);
    }
    for (int sct = 0; sct < SA_MAXSEC; ++sct)
        for (int i = 0; i < 16; ++i) {
            const float *m = lt.p[sct][i];
            v.push_back(m[0]); v.push_back(m[2]); v.push_back(m[1]); v.push_back(m[3]);
        }
    const int n = (int)v.size();
    if (out && cap > 0) std::memcpy(out, v.data(), sizeof(float) * (size_t)(cap < n ? cap : n));
    return n;
}

// the float64-state plan of an a0-normalised SOS as flat doubles (sa_debug_iir_plan_f64, sa_iir_plan_from_sos_f64)
int export_plan_f64(const double *sos_norm, int nsec, double *out, int cap)
{
    SaIirF64 p;
    build_plan_f64(sos_norm, nsec, &p);
    if (out && cap > 0) std::memcpy(out, &p, sizeof(double) * (size_t)(cap < kSaIirF64Doubles ? cap : kSaIirF64Doubles));
    return kSaIirF64Doubles;
}

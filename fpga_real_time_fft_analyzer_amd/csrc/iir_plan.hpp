// iir_plan.hpp -- the plan algebra of the IIR cascades (iir_plan.cpp): pure host functions of the SOS and the window,
// no handle and no stream, so nothing in the handle's bookkeeping can change a plan.  Not exported by the library.
#pragma once
#include "sa_common.hpp"

#pragma GCC visibility push(hidden)

extern const int8_t kDefaultQ7[12];        // the fixed coefficient sets of filter mode 0xA1

void build_plan(const double *sos_in, int nsec_in, SaIirK *plan, SaIirLaneTab *lt, const float *half_win,
                const double *cosw = nullptr);
void build_plan_f64(const double *sos_in, int nsec_in, SaIirF64 *p);
void sos_from_q7(const int8_t *c12, double *sos /*[6][6]*/);
bool normalise_a0(const double *sos, int n_sections, double *norm /*[36]*/);
int export_plan(const SaIirK &p, const SaIirLaneTab &lt, float *out, int cap);
int export_plan_f64(const double *sos_norm, int nsec, double *out, int cap);

#pragma GCC visibility pop

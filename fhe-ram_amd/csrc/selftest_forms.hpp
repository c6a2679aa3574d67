// k_selftest_forms_fwd / k_selftest_forms_inv (selftest_forms.hip): the device side of fheram_selftest_forms — what fheram.hip sees of it.
// The kernels live in a translation unit of their own, as k_cmux_chain does (cmux_chain.hpp): compiled apart they leave the device code of
// every kernel of fheram.hip exactly as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

// the inverse forms the library instantiates, each under the buffer discipline of its call sites (kernels.hpp, cmux_step.inc, trace_tail.inc)
enum SelftestForm : int {
    SF_SKEW1_BARRIER = 0,   // fft_inv_skew<1, 1>, accumulator b in buffer b                   (the form tests/test_gpu_fft.py pins: the reference of the others)
    SF_SKEW2_BARRIER = 1,   // fft_inv_skew<2, 1>
    SF_SKEW1_ALT = 2,       // fft_inv_skew<1, 0> on alternating buffers                        (ntt_inv<1, false>(.., data + (it++ & 1) * LDS_DATA, ..))
    SF_SKEW1_FWD = 3,       // fft_inv_skew<1, 0> in ONE buffer, directly behind an ntt_fwd<1> in that buffer (k_trace_step and its kin)
    SF_SKEW1_LOOP = 4,      // fft_inv_skew<1, 2>, the same buffer every time                   (ntt_inv1_loop)
    SF_SKEW2_LOOP = 5,      // fft_inv_skew<2, 2>, the same two buffers every time              (ntt_inv2_loop)
    SF_HOOKED1 = 6,         // fft_inv1_hooked<2>, one buffer, two calls per batch              (the streamed key-switch)
    SF_HOOKED2 = 7,         // fft_inv2_hooked<2>                                               (k_read_chain)
    SF_UNITS5 = 8,          // pair, pair, two singles, pair: both hooked forms in the same buffers under one free counter (k_read_chain's five-limb units)
    SF_FORMS = 9
};

// in: [2 * n_a] int32 polynomials (a, then g);  sp: [2 * n_a] prepared polynomials out (a as it is, g scaled by gscale);  one workgroup per fwd_polys of them
hipError_t selftest_forms_fwd_launch(hipStream_t stream, int fwd_polys, const int32_t* in, double* sp, const double* tw_g, double gscale, int n_a);
// sa, sg: [K][R] prepared polynomials;  a_raw: [K][R] int32;  out: [K][2][N];  ONE workgroup
hipError_t selftest_forms_inv_launch(hipStream_t stream, int form, bool rounded, const double* sa, const double* sg, const int32_t* a_raw, double* out,
                                     const double* tw_g, int K, int R);

}  // namespace fk

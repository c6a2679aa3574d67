// One coefficient of one limb form, evaluated by calling only the functions of limb_forms.hpp — the text the kernels call.
// Shared by the device self-test (selftest.hpp: fheram_selftest_limb_forms, one thread per coefficient) and by the host
// build of the CPU suite (tests/limb_forms_host.cpp).  Integers travel as exact doubles: LF_IN doubles in, LF_OUT doubles
// out per coefficient; what a form does not use is ignored / left untouched.
//
//   form                 in                                             out
//   LF_NORM3 / LF_NORM4  S limbs (most significant first)               S digits                         normalize_coeff<S, S>
//   LF_RSH1_3            3 int limbs                                    3 digits                         rsh1_coeff<3>
//   LF_Y_OF              3 limbs, sign (0 / 1)                          Y                                y_of3
//   LF_DIGITS3           a                                              d0 (the quotient), d1, d2, and digit3_r(a, 0 / 1 / 2)
//   LF_DIGITS3_WRAPPED   a                                              d0 (wrapped), d1, d2
//   LF_CLOSED4           start value, 4 big limbs                       A = window51(V), d0, d1, d2 of A, ceil_half(A)     fold_limb4_1
//   LF_CLOSED5           start value, 5 big limbs                       the same                                           fold_limb_1<5>, ec carried between limbs
//   LF_WRITE_POST        h (3 limbs), t (3 limbs), a                    window51(whole(h) - whole(t) + a)
//   LF_PAIR_SUM          a' (3 limbs), sign, b (3 limbs)                window51(ceil_half(A(a') + A(b)))
//   LF_PAIR_DIFF         the same                                       window51(ceil_half(A(a') - A(b))), ceil_half(A(a') - A(b))
//   LF_PAIR_OUT          u, W                                           r = window51(u - window51(W)), d0, d1, d2 of r
//   LF_CMUX_4_4 / _5_4   SG product limbs, 4 row limbs                  4 digits of normalize(row + normalize(product))
#pragma once
#include "limb_forms.hpp"

namespace fk {

enum LimbForm {
    LF_NORM3 = 0, LF_NORM4 = 1, LF_RSH1_3 = 2, LF_Y_OF = 3, LF_DIGITS3 = 4, LF_DIGITS3_WRAPPED = 5, LF_CLOSED4 = 6, LF_CLOSED5 = 7,
    LF_WRITE_POST = 8, LF_PAIR_SUM = 9, LF_PAIR_DIFF = 10, LF_PAIR_OUT = 11, LF_CMUX_4_4 = 12, LF_CMUX_5_4 = 13, LF_FORMS = 14
};
constexpr int LF_IN = 10;    // doubles per coefficient, input
constexpr int LF_OUT = 6;    // doubles per coefficient, output

template <int S>
FK_HD void lf_norm(const double* in, double* out) {
    double in_l[S], out_l[S];
    for (int j = 0; j < S; j++) in_l[j] = in[j];
    normalize_coeff<S, S>(in_l, out_l);
    for (int j = 0; j < S; j++) out[j] = out_l[j];
}
template <int SK>
FK_HD void lf_closed(const double* in, double* out) {
    double od = in[0], ec = 0.0;
    for (int j = SK - 1; j >= 0; j--) {
        if constexpr (SK == 4) fold_limb4_1<SK>(od, in[1 + j], j);
        else fold_limb_1<SK>(od, ec, in[1 + j], j);
    }
    const double a = window51(od);
    out[0] = a;
    digits3(a, out[1], out[2], out[3]);
    out[4] = ceil_half(a);
}
template <int SG, int SA>
FK_HD void lf_cmux(const double* in, double* out) {
    int carry = 0, carry2 = 0;
    for (int j = SG - 1; j >= 0; j--) {
        const double ed = cmux_product_digit(in[j], carry);
        if (j < SA) out[j] = (double)cmux_row_digit((int)in[SG + j], (int)ed, carry2);
    }
}

// returns 0, or -1 for an unknown form
FK_HD int limb_form_eval(int form, const double* in, double* out) {
    switch (form) {
    case LF_NORM3: lf_norm<3>(in, out); return 0;
    case LF_NORM4: lf_norm<4>(in, out); return 0;
    case LF_RSH1_3: {
        int x[3], y[3];
        for (int j = 0; j < 3; j++) x[j] = (int)in[j];
        rsh1_coeff<3>(x, y);
        for (int j = 0; j < 3; j++) out[j] = (double)y[j];
        return 0;
    }
    case LF_Y_OF: out[0] = y_of3(in[0], in[1], in[2], in[3] != 0.0); return 0;
    case LF_DIGITS3:
        digits3(in[0], out[0], out[1], out[2]);
        for (int r = 0; r < 3; r++) out[3 + r] = digit3_r(in[0], r);
        return 0;
    case LF_DIGITS3_WRAPPED: digits3_wrapped(in[0], out[0], out[1], out[2]); return 0;
    case LF_CLOSED4: lf_closed<4>(in, out); return 0;
    case LF_CLOSED5: lf_closed<5>(in, out); return 0;
    case LF_WRITE_POST: out[0] = write_post(whole3(in[0], in[1], in[2]), whole3(in[3], in[4], in[5]), in[6]); return 0;
    case LF_PAIR_SUM:
    case LF_PAIR_DIFF: {
        const double va = whole3(in[0], in[1], in[2]);
        const double aa = in[3] != 0.0 ? -va : va;
        const double ab = whole3(in[4], in[5], in[6]);
        if (form == LF_PAIR_SUM) out[0] = pair_sum(aa, ab);
        else { out[0] = pair_diff(aa, ab); out[1] = ceil_half(aa - ab); }
        return 0;
    }
    case LF_PAIR_OUT: out[0] = pair_out(in[0], in[1]); digits3(out[0], out[1], out[2], out[3]); return 0;
    case LF_CMUX_4_4: lf_cmux<4, 4>(in, out); return 0;
    case LF_CMUX_5_4: lf_cmux<5, 4>(in, out); return 0;
    default: return -1;
    }
}

}  // namespace fk

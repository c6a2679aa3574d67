// The scalar forms of the base-2^17 limb arithmetic, one coefficient at a time: the limb walk, vec_znx_rsh(1), and the
// closed-form normalisation of the chain kernels (kernels.hpp "ks_trace_z" says why the closed form equals the walk).
// ONE text for host and device: the kernels call these functions, and so do the device self-test (selftest.hpp,
// fheram_selftest_limb_forms) and the host build of the CPU suite (tests/limb_forms_host.cpp), through limb_forms_eval.hpp.
// Depends on nothing but <cstdint>.  Every value is an exact integer held in a double (or an int), every operation
// (scaling by a power of two, + 0.5, floor, an fma whose result is representable) is exact; the fmas are placed by hand:
// compile with -ffp-contract=off.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FK_HD inline
#endif

namespace fk {

// ---- base-2^17 limb arithmetic on exact-integer doubles ------------------
constexpr int BASE2K = 17;
constexpr double TWO_B = 131072.0;         // 2^17
constexpr double INV_TWO_B = 1.0 / 131072.0;

// carry(x) = floor((x + 2^16) / 2^17);  digit(x) = x - carry*2^17 in [-2^16, 2^16)
FK_HD double carry_of(double x) { return __builtin_floor(__builtin_fma(x, INV_TWO_B, 0.5)); }
FK_HD double digit_of(double x, double c) { return __builtin_fma(-c, TWO_B, x); }

// vec_znx_big_normalize for one coefficient: in[0..SI) -> out[0..SO), SI >= SO.
template <int SI, int SO>
FK_HD void normalize_coeff(const double (&in)[SI], double (&out)[SO]) {
    double c = 0.0;
#pragma unroll
    for (int j = SI - 1; j >= 0; j--) {
        const double v = in[j] + c;
        c = carry_of(v);
        if (j < SO) out[j] = digit_of(v, c);
    }
}

// integer digit helpers (int32 is enough: all operands are sums of a few 17-bit digits)
FK_HD int digit17(int v) { return (int)((unsigned)v << 15) >> 15; }

// vec_znx_rsh_inplace(k = 1) on one coefficient of S limbs (see oracle/znx.hpp rsh_inplace):
// shift by one limb, then normalise with lsh = 16.
template <int S>
FK_HD void rsh1_coeff(const int (&x)[S], int (&y)[S]) {
    int d = -(x[S - 1] & 1);
    int c = (x[S - 1] - d) >> 1;
#pragma unroll
    for (int j = S - 1; j >= 1; j--) {
        const int src = x[j - 1];
        d = -(src & 1);
        const int cr = (src - d) >> 1;
        const int dpc = d * 65536 + c;
        y[j] = digit17(dpc);
        c = cr + ((dpc - y[j]) >> 17);
    }
    y[0] = digit17(c);
}

// ---- the one-double form (kernels.hpp "One fused trace step") -----------------------------
constexpr double TWO_2B = 17179869184.0;   // 2^34
// c = q * 2^17 + d with d in [-2^16, 2^16): returns d, leaves q in c
FK_HD double take_digit(double& c) {
    const double q = carry_of(c);
    const double d = digit_of(c, q);
    c = q;
    return d;
}
// A = l0 * 2^34 + l1 * 2^17 + l2: the integer three limbs of a coefficient stand for (the limbs need not be normalised)
// (L: int or double limbs; the conversions stand where the kernels had them)
template <typename L>
FK_HD double whole3(L l0, L l1, L l2) { return __builtin_fma(__builtin_fma((double)l0, TWO_B, (double)l1), TWO_B, (double)l2); }
// Y = ceil(A / 2) = floor(A/2 + 1/2): rsh1 of the limbs of A, as one double
FK_HD double ceil_half(double a) { return __builtin_floor(__builtin_fma(a, 0.5, 0.5)); }
// Y of three stored limbs read through a rotation: the rotation's sign comes before the shift
template <typename L>
FK_HD double y_of3(L l0, L l1, L l2, bool neg) {
    double a_ = whole3(l0, l1, l2);
    a_ = neg ? -a_ : a_;
    return ceil_half(a_);
}
// the three digits of a: d2, d1 balanced, d0 the second quotient (a in the digit window: the quotient IS the top digit)
FK_HD void digits3(double a, double& d0, double& d1, double& d2) {
    double c = a;
    d2 = take_digit(c);
    d1 = take_digit(c);
    d0 = c;
}
// digit r of c (c = the one-double form): digits leave from the least significant end
FK_HD double digit3_r(double c, int r) {
    double d = take_digit(c);
    if (r < 2) d = take_digit(c);
    if (r < 1) d = c;
    return d;
}

// ---- closed-form normalisation (kernels.hpp "ks_trace_z") ---------------------------------
constexpr double TWO_51 = 2251799813685248.0;          // 2^51
constexpr double INV_TWO_51 = 1.0 / 2251799813685248.0;
constexpr double INV_TWO_2B = 1.0 / 17179869184.0;      // 2^-34
constexpr double WIN_C = 65536.0 + 8589934592.0 + 1125899906842624.0;   // 2^16 + 2^33 + 2^50
// centred remainder of x modulo 2^17 / 2^34 (x an exact integer)
FK_HD double cmod17(double x) { return __builtin_fma(-__builtin_floor(__builtin_fma(x, INV_TWO_B, 0.5)), TWO_B, x); }
FK_HD double cmod34(double x) { return __builtin_fma(-__builtin_floor(__builtin_fma(x, INV_TWO_2B, 0.5)), TWO_2B, x); }
// V -> the integer whose balanced base-2^17 digits are the three output limbs (top carry dropped)
FK_HD double window51(double v) { return __builtin_fma(-__builtin_floor(__builtin_fma(v, INV_TWO_51, WIN_C * INV_TWO_51)), TWO_51, v); }
// the three digits of a, the top one wrapped (|Y| reaches 2^50: the quotient can be +-2^16)
FK_HD void digits3_wrapped(double a, double& d0, double& d1, double& d2) {
    double c = a;
    d2 = take_digit(c);
    d1 = take_digit(c);
    d0 = cmod17(c);
}
// adds output limb j's contribution to V, one coefficient (SO = 3 output limbs; limbs j >= 3 go through the extra-carry e first)
// (the four pieces are what the kernels' E-wide fold_limb loops over, branch by branch: kernels.hpp)
FK_HD double fold_extra_carry(double acc, double ec) { return carry_of(acc + ec); }                  // limbs 3 <= j < SK - 1: the inner carry
FK_HD double fold_limb1(double od, double acc) { return __builtin_fma(cmod34(acc), TWO_B, od); }    // limb 1
FK_HD double fold_limb0(double od, double acc) { return __builtin_fma(cmod17(acc), TWO_2B, od); }   // limb 0
template <int SK>
FK_HD void fold_limb_1(double& od, double& ec, const double acc, int j) {
    if (j >= 3) {
        if (SK >= 5 && j < SK - 1) ec = fold_extra_carry(acc, ec);
        else ec = carry_of(acc);
        if (j == 3) od += ec;
    } else if (j == 2) {
        od += acc;
    } else if (j == 1) {
        od = fold_limb1(od, acc);
    } else {
        od = fold_limb0(od, acc);
    }
}
// for 4 limbs the extra carry lives inside the call for limb 3: no state between limbs
template <int SK>
FK_HD void fold_limb4_1(double& od, const double acc, int j) {
    static_assert(SK == 4, "four limbs");
    double ec = 0.0;
    fold_limb_1<SK>(od, ec, acc, j);
}
// the write chain's last trace step: normalize(ct_hi - trace(ct_hi) + a), h and t as the integers their limbs stand for
FK_HD double write_post(double h, double t, double a) { return window51(h - t + a); }
// the pair step (k_pair_z): normalize(rsh1(a' + b)), normalize(rsh1(a' - b)) and normalize(u - tmp), A(a') and A(b) as whole3
FK_HD double pair_sum(double aa, double ab) { return window51(ceil_half(aa + ab)); }
FK_HD double pair_diff(double aa, double ab) { return window51(ceil_half(aa - ab)); }
FK_HD double pair_out(double u, double w) { return window51(u - window51(w)); }

// ---- the CMux step's two int carries (cmux_step.inc) --------------------------------------
// limb j of the product: a + carry -> its digit (returned), the new carry (exact small integers: |a| < 2^47, its carry < 2^31)
FK_HD double cmux_product_digit(double a, int& carry) {
    const double v = a + (double)carry;
    const double cy = carry_of(v);
    carry = (int)cy;
    return digit_of(v, cy);
}
// limb j of row <- normalize(row + product)
FK_HD int cmux_row_digit(int row, int ev, int& carry2) {
    const double v2 = (double)(row + ev) + (double)carry2;
    const double c2 = carry_of(v2);
    carry2 = (int)c2;
    return (int)digit_of(v2, c2);
}

}  // namespace fk

// The device side of fheram_selftest_forms (selftest.hpp, include/fheram.h): every inverse form the kernels call, under the call sites'
// own buffer discipline, on operands the host chooses; tests/test_gpu_fft_forms.py compares the raw sums with exact integers and
// across forms.  Nothing on the RAM path launches these kernels.  Plain vector loads and stores only.
// A translation unit of its own (selftest_forms.hpp says why).
#undef FK_STAMP   // (the stamp buffer of the diagnostic build belongs to fheram.hip)
#define FK_NO_PLAIN_KERNELS
#include "kernels.hpp"
#include "selftest_forms.hpp"

namespace fk {

// ---- every inverse form the chain kernels call, under the call sites' own buffer discipline (fheram_selftest_forms) ------------------
// Two launches.  k_selftest_forms_fwd transforms every operand polynomial with ntt_fwd<FP> and leaves it in a global scratch buffer in
// the prepared-operand layout (what load_ops reads): a as it is, g scaled by ninv * operand_scale.  k_selftest_forms_inv, ONE workgroup,
// then produces K batches of two accumulators (acc0 = sum_r a_r g_r, acc1 = sum_r a_r g_{r ^ 1}: 2R products per batch, ascending r in
// each accumulator, as k_selftest_convolve takes them) and runs inverse form FORM on each batch — batch i + 1's products are taken
// while batch i is transformed: inside the hooks of the hooked forms (spread over all their places: every place takes at least one at
// R = 6), between the transforms of the others.  Operands are requested one product ahead with load_ops, behind a pin_regs, as the
// chain kernels' hooks do (kernels.hpp, k_read_chain).  All forms run i_pass4(t2), i_pass4(t1), i_pass3(t0) on each polynomial, and
// -ffp-contract=off: their raw outputs are the same doubles (tests/test_gpu_fft_forms.py).

template <int FP>
__global__ __launch_bounds__(T) void k_selftest_forms_fwd(const int32_t* __restrict__ in, double* __restrict__ sp, const double* __restrict__ tw_g,
                                                          double gscale, int n_a, int n_all) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tw = lds;
    double* data = lds + LDS_TW;
    const int tid = vt((int)threadIdx.x);
    load_twiddles(tw, tw_g, tid);
    const int p0 = FP * (int)blockIdx.x;
    double x[FP][E];
#pragma unroll
    for (int b = 0; b < FP; b++) {
        const int src = (p0 + b < n_all) ? p0 + b : n_all - 1;   // (the last workgroup's spare places repeat the last polynomial: every wave runs every transform)
#pragma unroll
        for (int k = 0; k < E; k++) x[b][k] = (double)in[(long)src * N + tid + T * k];
    }
    ntt_fwd<FP>(x, tw, data, tid);
#pragma unroll
    for (int b = 0; b < FP; b++) {
        if (p0 + b >= n_all) break;
        const double sc = (p0 + b >= n_a) ? gscale : 1.0;
        double2* o = reinterpret_cast<double2*>(sp + (long)(p0 + b) * N);
#pragma unroll
        for (int kk = 0; kk < E / 2; kk++) {
            double2 w;
            w.x = x[b][2 * kk] * sc;
            w.y = x[b][2 * kk + 1] * sc;
            o[kk * T + tid] = w;
        }
    }
}

// sa, sg: [K][R] prepared polynomials (the forward launch's scratch);  a_raw: the int32 operands a (SF_SKEW1_FWD transforms them again);  out: [K][2][N]
// K and R are kernel arguments: every transform, barrier and sb_wait_free below is reached by all eight waves from uniform control flow.
template <int FORM, bool ROUNDED>
__global__ __launch_bounds__(T) void k_selftest_forms_inv(const double* __restrict__ sa, const double* __restrict__ sg, const int32_t* __restrict__ a_raw,
                                                          double* __restrict__ out, const double* __restrict__ tw_g, int K, int R) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    RoMonitor ro_mon(lds, tw_g, ROUNDED);
    double* tw = lds;
    double* data = lds + LDS_TW;
    const int tid = vt((int)threadIdx.x);
    load_twiddles(tw, tw_g, tid);      // zeroes the free counter of the FENCE == 2 forms
    const int P2 = 2 * R, NPROD = K * P2;
    double accn[2][E];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int k = 0; k < E; k++) accn[b][k] = 0.0;
    // product q of the stream: batch q / 2R, p = q % 2R: accumulator b = p / R takes a_r * g_{r ^ b}, r = p % R
    OpRegs oa, og;
    auto request = [&](int q) {
        const int i = q / P2, p = q - i * P2, b = p >= R ? 1 : 0, r = p - b * R;
        load_ops(oa, sa + (long)(i * R + r) * N, tid);
        load_ops(og, sg + (long)(i * R + (r ^ b)) * N, tid);
    };
    auto take = [&](int q) {           // its operands are in oa / og; the next product's are requested behind it
        double x[E];
#pragma unroll
        for (int kk = 0; kk < E / 2; kk++) { x[2 * kk] = oa.v[kk].x; x[2 * kk + 1] = oa.v[kk].y; }
        if (q % P2 < R) { mac_regs(accn[0], x, og); pin_regs(accn[0]); }
        else { mac_regs(accn[1], x, og); pin_regs(accn[1]); }
        __builtin_amdgcn_sched_barrier(0);
        if (q + 1 < NPROD) request(q + 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto take_range = [&](int i, int lo, int hi) {   // products [lo, hi) of batch i (none behind the last batch)
        if (i < K) {
#pragma unroll 1
            for (int p = lo; p < hi; p++) take(i * P2 + p);
        }
    };
    request(0);
    take_range(0, 0, P2);
    int it = 0;
#pragma unroll 1
    for (int i = 0; i < K; i++) {
        double acc[2][E];
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int k = 0; k < E; k++) { acc[b][k] = accn[b][k]; accn[b][k] = 0.0; }
        double (&acc0)[1][E] = *reinterpret_cast<double(*)[1][E]>(&acc[0]);
        double (&acc1)[1][E] = *reinterpret_cast<double(*)[1][E]>(&acc[1]);
        // place s of n: its share of the next batch's 2R products
        auto place = [&](auto s_tag, auto n_tag) {
            constexpr int s = decltype(s_tag)::value, n = decltype(n_tag)::value;
            take_range(i + 1, s * P2 / n, (s + 1) * P2 / n);
        };
        using std::integral_constant;
        auto hook6 = [&](auto st) { place(st, integral_constant<int, 6>{}); };
        auto hook8a = [&](auto st) { place(st, integral_constant<int, 8>{}); };
        auto hook8b = [&](auto st) { place(integral_constant<int, decltype(st)::value + 4>{}, integral_constant<int, 8>{}); };
        if constexpr (FORM == SF_SKEW1_BARRIER) {
            double* const d0[1] = {data};
            double* const d1[1] = {data + LDS_DATA};
            fft_inv_skew<1, 1, ROUNDED>(acc0, tw, d0, tid);
            take_range(i + 1, 0, R);
            fft_inv_skew<1, 1, ROUNDED>(acc1, tw, d1, tid);
            take_range(i + 1, R, P2);
        } else if constexpr (FORM == SF_SKEW2_BARRIER) {
            double* const d[2] = {data, data + LDS_DATA};
            fft_inv_skew<2, 1, ROUNDED>(acc, tw, d, tid);
            take_range(i + 1, 0, P2);
        } else if constexpr (FORM == SF_SKEW1_ALT) {
            double* const d0[1] = {data + (it++ & 1) * LDS_DATA};
            fft_inv_skew<1, 0, ROUNDED>(acc0, tw, d0, tid);
            take_range(i + 1, 0, R);
            double* const d1[1] = {data + (it++ & 1) * LDS_DATA};
            fft_inv_skew<1, 0, ROUNDED>(acc1, tw, d1, tid);
            take_range(i + 1, R, P2);
        } else if constexpr (FORM == SF_SKEW1_FWD) {
            double* const d0[1] = {data};
#pragma unroll
            for (int b = 0; b < 2; b++) {
                double xf[1][E];
#pragma unroll
                for (int k = 0; k < E; k++) xf[0][k] = (double)a_raw[(long)(i * R + b) * N + tid + T * k];
                ntt_fwd<1>(xf, tw, data, tid);          // starts with a barrier and ends in the wave's own region: what fences the inverse behind it
                pin_regs(xf[0]);
                fft_inv_skew<1, 0, ROUNDED>(b == 0 ? acc0 : acc1, tw, d0, tid);
                take_range(i + 1, b * R, (b + 1) * R);
            }
        } else if constexpr (FORM == SF_SKEW1_LOOP) {
            double* const d0[1] = {data};
            fft_inv_skew<1, 2, ROUNDED>(acc0, tw, d0, tid);
            take_range(i + 1, 0, R);
            fft_inv_skew<1, 2, ROUNDED>(acc1, tw, d0, tid);
            take_range(i + 1, R, P2);
        } else if constexpr (FORM == SF_SKEW2_LOOP) {
            double* const d[2] = {data, data + LDS_DATA};
            fft_inv_skew<2, 2, ROUNDED>(acc, tw, d, tid);
            take_range(i + 1, 0, P2);
        } else if constexpr (FORM == SF_HOOKED1) {
            fft_inv1_hooked<2, ROUNDED>(acc0, tw, data, tid, hook8a);
            fft_inv1_hooked<2, ROUNDED>(acc1, tw, data, tid, hook8b);
        } else if constexpr (FORM == SF_HOOKED2) {
            fft_inv2_hooked<2, ROUNDED>(acc, tw, data, data + LDS_DATA, tid, hook6);
        } else {
            static_assert(FORM == SF_UNITS5, "inverse form");
            if (i % 3 == 2) {      // (workgroup uniform)
                fft_inv1_hooked<2, ROUNDED>(acc0, tw, data, tid, hook8a);
                fft_inv1_hooked<2, ROUNDED>(acc1, tw, data, tid, hook8b);
            } else {
                fft_inv2_hooked<2, ROUNDED>(acc, tw, data, data + LDS_DATA, tid, hook6);
            }
        }
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int k = 0; k < E; k++) out[((long)i * 2 + b) * N + tid + T * k] = acc[b][k];
    }
}

template <int FORM, bool ROUNDED>
static hipError_t forms_inv_launch_t(hipStream_t st, const double* sa, const double* sg, const int32_t* a_raw, double* out, const double* tw_g, int K, int R) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_selftest_forms_inv<FORM, ROUNDED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_selftest_forms_inv<FORM, ROUNDED>), dim3(1), dim3(T), LDS_BYTES, st, sa, sg, a_raw, out, tw_g, K, R);
    return hipGetLastError();
}
template <int FP>
static hipError_t forms_fwd_launch_t(hipStream_t st, const int32_t* in, double* sp, const double* tw_g, double gscale, int n_a, int n_all) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_selftest_forms_fwd<FP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_selftest_forms_fwd<FP>, dim3((n_all + FP - 1) / FP), dim3(T), LDS_BYTES, st, in, sp, tw_g, gscale, n_a, n_all);
    return hipGetLastError();
}
template <int FORM = 0>
static hipError_t forms_inv_dispatch(int form, bool rounded, hipStream_t st, const double* sa, const double* sg, const int32_t* a_raw, double* out, const double* tw_g, int K, int R) {
    if constexpr (FORM < SF_FORMS) {
        if (form == FORM) return rounded ? forms_inv_launch_t<FORM, true>(st, sa, sg, a_raw, out, tw_g, K, R) : forms_inv_launch_t<FORM, false>(st, sa, sg, a_raw, out, tw_g, K, R);
        return forms_inv_dispatch<FORM + 1>(form, rounded, st, sa, sg, a_raw, out, tw_g, K, R);
    } else {
        return hipErrorInvalidValue;
    }
}

hipError_t selftest_forms_fwd_launch(hipStream_t stream, int fwd_polys, const int32_t* in, double* sp, const double* tw_g, double gscale, int n_a) {
    if (fwd_polys == 1) return forms_fwd_launch_t<1>(stream, in, sp, tw_g, gscale, n_a, 2 * n_a);
    if (fwd_polys == 2) return forms_fwd_launch_t<2>(stream, in, sp, tw_g, gscale, n_a, 2 * n_a);
    if (fwd_polys == 3) return forms_fwd_launch_t<3>(stream, in, sp, tw_g, gscale, n_a, 2 * n_a);
    return hipErrorInvalidValue;
}
hipError_t selftest_forms_inv_launch(hipStream_t stream, int form, bool rounded, const double* sa, const double* sg, const int32_t* a_raw, double* out,
                                     const double* tw_g, int K, int R) {
    return forms_inv_dispatch(form, rounded, stream, sa, sg, a_raw, out, tw_g, K, R);
}

}  // namespace fk

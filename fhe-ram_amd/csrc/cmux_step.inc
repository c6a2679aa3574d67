// cmux_step: one CMux step of Address::set_from_fheuint (conversion.rs:51-59) on one GGSW row, row <- normalize(row + normalize(X^rho row - row) (x) GGSW(b)).
// Included inside namespace fk, after kernels.hpp, by the units whose kernels run it: cmux_chain.hip (k_cmux_chain, which says what the arithmetic is)
// and cmux_jobs.hip (k_cmux_jobs).  One text, so the digits of the two kernels are the same integers.
template <int SA, int SG>
__device__ __forceinline__ void cmux_step(int32_t* acc, const double* __restrict__ gg, int rho, const double* tw, double* data, int tid) {
    double x0[SA][E], x1[SA][E];   // normalize(X^rho row - row), transformed: column 0 / column 1
    auto pre = [&](int col, double (&x)[SA][E]) {
#pragma unroll
        for (int k = 0; k < E; k++) {
            const int i = tid + T * k;
            int src; bool sgn;
            rot_src(i, rho, src, sgn);
            double in_l[SA], out_l[SA];
#pragma unroll
            for (int j = 0; j < SA; j++) in_l[j] = (double)(cneg(acc[glwe_off(j, col) + src], sgn) - acc[glwe_off(j, col) + i]);
            normalize_coeff<SA, SA>(in_l, out_l);
#pragma unroll
            for (int j = 0; j < SA; j++) x[j][k] = out_l[j];
        }
    };
    pre(0, x0);
    fwd_all<SA>(x0, tw, data, tid);
    pre(1, x1);
    fwd_all<SA>(x1, tw, data, tid);
    lds_barrier();   // every wave is done with the forward transforms' buffers — and with its reads of the row, which the loop below overwrites
    int it = 0;      // consecutive inverse transforms alternate between two exchange buffers (see ep_run)
#pragma unroll 1
    for (int co = 0; co < 2; co++) {
        int carry[E], carry2[E];   // exact small integers (|product limb| < 2^47: its carry < 2^31)
#pragma unroll
        for (int k = 0; k < E; k++) carry[k] = carry2[k] = 0;
#pragma unroll 1
        for (int j = SG - 1; j >= 0; j--) {
            double a[1][E];
#pragma unroll
            for (int k = 0; k < E; k++) a[0][k] = 0.0;
#pragma unroll
            for (int r = 0; r < SA; r++) {
                OpRegs g0, g1;
                load_ops(g0, gg + (long)(((2 * r) * SG + j) * 2 + co) * N, tid);
                load_ops(g1, gg + (long)(((2 * r + 1) * SG + j) * 2 + co) * N, tid);
                mac_regs(a[0], x0[r], g0);
                mac_regs(a[0], x1[r], g1);
            }
            ntt_inv<1, false>(a, tw, data + (it++ & 1) * LDS_DATA, tid);
            int32_t* op = acc + glwe_off(j < SA ? j : 0, co);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const double ed = cmux_product_digit(a[0][k], carry[k]);
                if (j < SA) op[tid + T * k] = cmux_row_digit(op[tid + T * k], (int)ed, carry2[k]);   // (workgroup uniform) row <- normalize(row + product), limb j
            }
        }
    }
}

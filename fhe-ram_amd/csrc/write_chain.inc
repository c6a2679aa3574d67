// Included by kernels.hpp (no include guard): a row's write chain (ram.rs:612-646, see RowChainArgs in kernels.hpp), instantiated twice.
//   FK_WRITE_CHAIN_NAME : kernel name;  FK_WRITE_CHAIN_ARGS / FK_WRITE_CHAIN_TABLE : RowChainArgs / 0, or RowChainTableArgs / 1 for the
//   write chain of a bank range (fheram_bank_write): ciphertext y = k * ws + w takes the inverse digits of entry y / ws, / 2 for that of
//   a write list (fheram_bank_write_list): and the rows (ct_hi, the last product's store) of member map(y / ws); ct_lo, trace(ct_hi) and
//   the tree's copy are per y in every form
#if FK_WRITE_CHAIN_TABLE
// recomputed where they are used rather than kept live across the steps (see FK_RC_OPND in chain_kernels.inc)
#define FK_WC_OPND(i) (ra.ep.ggsw[i] + table_opnd_offset(ra))
#else
#define FK_WC_OPND(i) ra.ep.ggsw[i]
#endif
#if FK_WRITE_CHAIN_TABLE == 2
#define FK_WC_ROW(a) table_member_row(a, ra)
#else
#define FK_WC_ROW(a) a
#endif
template <int SK, int SG>   // (only ever launched by Ram::write: never beside the gate wave)
__global__ __launch_bounds__(T, T / 256) __attribute__((amdgpu_num_vgpr(FK_WIDE_VGPRS))) void FK_WRITE_CHAIN_NAME(FK_WRITE_CHAIN_ARGS ra) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    RoMonitor ro_mon(lds, ra.ep.tw);
    double vc[E];   // (written by the first step before anything reads it)
    if (ra.tree.p != nullptr && blockIdx.x == 0) {   // k_rotate's per-coefficient code on T threads: out = a * X^rho, out does not alias a
        const int32_t* ap = at(ra.ks.base.a);
        int32_t* op = at(ra.tree);
        for (int idx = (int)threadIdx.x; idx < 2 * N; idx += T) {
            const int col = idx >> LOGN, i = idx & (N - 1);
            int src; bool sgn;
            rot_src(i, ra.tree_rho, src, sgn);
#pragma unroll
            for (int j = 0; j < 3; j++) op[glwe_off(j, col) + i] = cneg(ap[glwe_off(j, col) + src], sgn);
        }
    }
    KsArgs ka = ra.ks.base;
#pragma unroll 1
    for (int i = 0; i < ra.ks.n; i++) {          // n >= 2
        ka.out = ra.ks.buf[i & 1];
        ka.key = ra.ks.key[i];
        ka.ginv = ra.ks.ginv[i];
        int tid = vt((int)threadIdx.x);
        asm volatile("" : "+v"(tid));
        __builtin_assume(tid >= 0 && tid < T);
        if (i == 0) ks_trace_l<SK, false, 1>(ka, lds, true, tid, vc);
        else if (i + 1 < ra.ks.n) ks_trace_l<SK, true, 1>(ka, lds, false, tid, vc);
        else { ka.b = FK_WC_ROW(ra.hi); ka.out = ra.trhi; ks_trace_l<SK, true, 2>(ka, lds, false, tid, vc); }
        ka.rot_mul = 0;
        ka.rot_base = 0;
    }
    GlweRef in = ra.ep.src;
#pragma unroll 1
    for (int i = 0; i < ra.ep.n; i++) {          // n >= 2
        const GlweRef out = ra.ep.buf[i & 1];
        int tid = vt((int)threadIdx.x);
        asm volatile("" : "+v"(tid));
        __builtin_assume(tid >= 0 && tid < T);
        if (i == 0) ep_step_r<SG, 2, 1>(in, out, FK_WC_OPND(i), ra.ep.tw, lds, false, tid, vc);
        else if (i + 1 < ra.ep.n) ep_step_r<SG, 1, 1>(in, out, FK_WC_OPND(i), ra.ep.tw, lds, false, tid, vc);
        else ep_step_r<SG, 1, 0>(in, FK_WC_ROW(out), FK_WC_OPND(i), ra.ep.tw, lds, false, tid, vc);   // (the only store of the products: in place on the member's rows)
        in = out;
    }
}
#undef FK_WC_OPND
#undef FK_WC_ROW

// Included by kernels.hpp (no include guard): the chain kernels that exist in two register budgets.
//   FK_KS_CHAIN_NAME / FK_READ_CHAIN_NAME : kernel names;  FK_VG : the literal for amdgpu_num_vgpr (units of two registers)
//   FK_READ_CHAIN_ARGS / FK_READ_CHAIN_TABLE : RowChainArgs / 0, or RowChainTableArgs / 1 for the read chain over several addresses (the
//   source row through the member map), / 2 for that of a read_prepare_write list (the store_ep row through it as well), or RowChainMixArgs / 3
//   for the fallback of fheram_bank_read_mix's tail (mix.hip: per-ciphertext source pointer, digits and product count)
//   (that inclusion defines no FK_KS_CHAIN_NAME: the trace chain has no table form)
#ifdef FK_KS_CHAIN_NAME
// GLWE::trace(start, start + n) as ONE launch (see KsChainArgs in kernels.hpp)
template <int SX, int SK, int SO, int YF = 0>   // YF: 0 int32 limbs between the steps (ks_run); 3 the intermediates as Y = ceil(A/2) with the closed-form normalisation, handed over through LDS and registers (ks_trace_l)
__global__ __launch_bounds__(T, T / 256) __attribute__((amdgpu_num_vgpr(FK_VG))) void FK_KS_CHAIN_NAME(KsChainArgs ca) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    RoMonitor ro_mon(lds, ca.base.tw);
    if (ca.pred) {
        if (__hip_atomic_load(ca.pred, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ca.pred_seq) return;
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            const unsigned taken = atomicAdd(const_cast<unsigned*>(ca.pred) + 1, 1u) + 1u;   // fallbacks taken (fheram_tail_stats)
            if (ca.host_count) __hip_atomic_store(ca.host_count, taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (ca.done) {
        if (__hip_atomic_load(ca.done + (blockIdx.y * gridDim.x + blockIdx.x) * 32 + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ca.done_seq) return;
        if (threadIdx.x == 0) {
            const unsigned taken = atomicAdd(ca.done + MID_GROUPS_MAX * 32 + 1, 1u) + 1u;   // ciphertexts redone (fheram_mid_stats)
            if (ca.host_count) __hip_atomic_store(ca.host_count, taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    KsArgs ka = ca.base;
    double vcarry[E];   // YF = 3: the body column's Y on its way from one step to the next
#pragma unroll
    for (int k = 0; k < E; k++) vcarry[k] = 0.0;
#pragma unroll 1
    for (int i = 0; i < ca.n; i++) {
        ka.out = ca.buf[i & 1];
        ka.b = ka.a;
        ka.key = ca.key[i];
        ka.ginv = ca.ginv[i];
        int tid = vt((int)threadIdx.x);
        asm volatile("" : "+v"(tid));   // see k_ext_product_chain
        __builtin_assume(tid >= 0 && tid < T);
        if constexpr (YF == 3) {
            static_assert(SX == 3 && SO == 3, "the Y form is written for 3-limb ciphertexts");
            if (i == 0) ks_trace_l<SK, false, 1>(ka, lds, true, tid, vcarry);
            else if (i + 1 < ca.n) ks_trace_l<SK, true, 1>(ka, lds, false, tid, vcarry, YSTAMP_STEP(i));
            else ks_trace_l<SK, true, 0>(ka, lds, false, tid, vcarry);
        } else {
            ks_run<KS_TRACE, SX, SK, SO, 2, 0>(ka, lds, i == 0, tid);
        }
        if constexpr (YF != 3) __syncthreads();   // the step's stores have completed (vmcnt 0) and its LDS traffic is over (YF = 3: nothing passes through global memory)
        ka.a = ka.out;
        ka.rot_mul = 0;
        ka.rot_base = 0;
    }
}
#endif
// read / read_prepare_write: a row's products of coordinate 0 + its alone packer levels as ONE launch (see RowChainArgs in kernels.hpp)
template <int SK, int SG>
__global__ __launch_bounds__(T, T / 256) __attribute__((amdgpu_num_vgpr(FK_VG))) void FK_READ_CHAIN_NAME(FK_READ_CHAIN_ARGS ra) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (ra.ks.pred) {   // the fallback launch behind k_trace_tail's products + trace chain: runs only if that launch gave up
        if (__hip_atomic_load(ra.ks.pred, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ra.ks.pred_seq) return;
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            const unsigned taken = atomicAdd(const_cast<unsigned*>(ra.ks.pred) + 1, 1u) + 1u;   // fallbacks taken (fheram_tail_stats)
            if (ra.ks.host_count) __hip_atomic_store(ra.ks.host_count, taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
#if FK_READ_CHAIN_TABLE == 3
    if (ra.x.n_ep[mix_row_y()] == 0) return;   // a ciphertext without products: the trace-only fallback behind this launch redoes it (mix.hpp)
#endif
    RoMonitor ro_mon(lds, ra.ep.tw);
    double vc[E];
#pragma unroll
    for (int k = 0; k < E; k++) vc[k] = 0.0;
    {
        GlweRef in = ra.ep.src;
#if FK_READ_CHAIN_TABLE == 3
        // fheram_bank_read_mix's fallback: ciphertext y has its own source pointer, its own prepared digits and its own product count
        // (mix.hpp MixGroupArgs), recomputed where they are used as the table forms' are
#define FK_RC_OPND(i) (ra.x.ggsw[mix_row_y()] + (long)(i) * ra.x.ggsw_stride)
#define FK_RC_ROW(a) GlweRef{const_cast<int32_t*>(ra.x.src[mix_row_y()]), 0, 0}
#define FK_RC_N ra.x.n_ep[mix_row_y()]
#elif FK_READ_CHAIN_TABLE
        // the member's row map(y / ws) * ws + y mod ws (the source, and where store_ep puts the products' result) and the prepared digits of
        // address y / ws: recomputed where they are used (a few scalar instructions) rather than kept live across the steps, at this
        // kernel's scalar register pressure
#define FK_RC_OPND(i) (ra.ep.ggsw[i] + table_opnd_offset(ra))
#define FK_RC_ROW(a) table_member_row(a, ra)
#define FK_RC_N ra.ep.n
#else
#define FK_RC_OPND(i) ra.ep.ggsw[i]
#define FK_RC_ROW(a) a
#define FK_RC_N ra.ep.n
#endif
#if FK_READ_CHAIN_TABLE == 2
#define FK_RC_STORE_ROW(a) table_member_row(a, ra)
#else
#define FK_RC_STORE_ROW(a) a
#endif
#pragma unroll 1
        for (int i = 0; i < FK_RC_N; i++) {      // n >= 2
            const GlweRef out = ra.ep.buf[i & 1];
            int tid = vt((int)threadIdx.x);
            asm volatile("" : "+v"(tid));   // see k_ext_product_chain
            __builtin_assume(tid >= 0 && tid < T);
            if (i == 0) ep_step_r<SG, 0, 1>(FK_RC_ROW(in), out, FK_RC_OPND(i), ra.ep.tw, lds, true, tid, vc);
            else if (i + 1 < FK_RC_N) ep_step_r<SG, 1, 1>(in, out, FK_RC_OPND(i), ra.ep.tw, lds, false, tid, vc);
            else ep_step_r<SG, 1, 3>(in, FK_RC_STORE_ROW(out), FK_RC_OPND(i), ra.ep.tw, lds, false, tid, vc, false, ra.store_ep != 0);   // (the only store of the products, and only under store_ep)
            in = out;
        }
#undef FK_RC_OPND
#undef FK_RC_ROW
#undef FK_RC_N
#undef FK_RC_STORE_ROW
    }
    KsArgs ka = ra.ks.base;
#pragma unroll 1
    for (int i = 0; i < ra.ks.n; i++) {          // n >= 1: every step takes its input from LDS and registers
        ka.out = ra.ks.buf[i & 1];
        ka.key = ra.ks.key[i];
        ka.ginv = ra.ks.ginv[i];
        int tid = vt((int)threadIdx.x);
        asm volatile("" : "+v"(tid));
        __builtin_assume(tid >= 0 && tid < T);
        if (i + 1 < ra.ks.n) ks_trace_l<SK, true, 1>(ka, lds, false, tid, vc);
        else ks_trace_l<SK, true, 0>(ka, lds, false, tid, vc);
    }
}

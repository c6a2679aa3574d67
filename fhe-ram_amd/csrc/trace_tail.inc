// Included TWICE by kernels.hpp (no include guard): k_trace_tail (one read) and k_trace_tail_t (several addresses: a batch, a bank range, a read list),
// and a third time by mix.hip: k_trace_tail_x (fheram_bank_read_mix: every ciphertext its own source, digits and product count).
//   FK_TAIL_NAME : kernel name;  FK_TAIL_ARGS : TailArgs, TailTableArgs or TailMixArgs;  FK_TAIL_TABLE : 1 = the products' operands of ciphertext
//   y are those of address y / ws (TailTableArgs), 0 = one address, 2 = group g reads its source pointer, the pointer to its prepared
//   digits and its own product count from ta.x (mix.hpp MixGroupArgs; one ciphertext per group, gx = 1): n_ep is uniform within a group and
//   groups never wait for each other, so nothing else changes
template <int SX, int SK, int SO>
__global__ __launch_bounds__(T, T / 256) void FK_TAIL_NAME(FK_TAIL_ARGS ta) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int G = 2 * SK * SX;
    constexpr int SG = 4, GE = 2 * SG * SX;        // a product: 4 output limbs per column, 24 active members
    static_assert(GE <= G && SX == 3 && SO == 3, "the products' members are a subset of the trace steps'");
    const int g = ((int)blockIdx.x + TAIL_GROUPS - ta.xoff) % TAIL_GROUPS, m = (int)blockIdx.x / TAIL_GROUPS;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)   // the last block: every block of the launch has been placed (k_tail_gate)
        __hip_atomic_store(ta.sync + TAIL_GROUPS * 32 + 2, ta.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g >= ta.n_ct) return;
    const int tid = vt((int)threadIdx.x);
    double* tw = lds;
    double* data = lds + LDS_TW;
    int* mstage = reinterpret_cast<int*>(data);
    int* flag = reinterpret_cast<int*>(data + 2 * LDS_DATA);   // the third exchange buffer is not used here
    unsigned* ctr = ta.sync + g * 32;
    unsigned* abortp = ta.sync + TAIL_GROUPS * 32;
#if FK_TAIL_TABLE == 2
    const int n_ep = ta.x.n_ep[g], n_all = n_ep + ta.n;
#else
    const int n_ep = ta.n_ep, n_all = ta.n_ep + ta.n;
#endif
    int s = 0;   // (lives past the step loop: s < n_all there = this workgroup left early, its group gave up)
    {   // the monitor's scope (not indented): its flush comes BEFORE the workgroup counts itself as gone, so the host words below are the launch's last stores
    RoMonitor ro_mon(lds, ta.tw);
    const int r = m % SX, zz = m / SX;
    const int j = SK - 1 - zz % SK, co = zz / SK;                 // this member in a trace step
    const int je = SG - 1 - zz % SG, coe = zz / SG;               // ... and in a product (m < GE)
    const bool ep_member = m < GE;
    const long ct = (long)(g / ta.gx);
    const long cx = (long)(g % ta.gx);
#if FK_TAIL_TABLE == 2
#define FK_TAIL_OPND(i) (ta.x.ggsw[g] + (long)(i) * ta.x.ggsw_stride)
#define FK_TAIL_SRC GlweRef{const_cast<int32_t*>(ta.x.src[g]), 0, 0}   // the ciphertext itself: a packed row in an arena, a table's row, a register file's
#elif FK_TAIL_TABLE
    const long oset = (ct / ta.ws) * ta.opnd_stride;   // this ciphertext's address: its prepared digits
#define FK_TAIL_OPND(i) (ta.ggsw[i] + oset)
#define FK_TAIL_SRC ta.src
#else
#define FK_TAIL_OPND(i) ta.ggsw[i]
#define FK_TAIL_SRC ta.src
#endif
    double* const big0 = ta.big + (long)g * BIG_STRIDE * SX;   // + step parity * TAIL_GROUPS * BIG_STRIDE * SX (see the normalisation phase)
    OpRegs kop, kop1;                 // the operand(s) of the coming step: a trace key polynomial, or the two GGSW polynomials of a product
    if (n_ep > 0) {
        if (ep_member) {
            load_ops(kop, FK_TAIL_OPND(0) + (long)(((2 * r) * SG + je) * 2 + coe) * N, tid);
            load_ops(kop1, FK_TAIL_OPND(0) + (long)(((2 * r + 1) * SG + je) * 2 + coe) * N, tid);
        }
    } else {
        load_ops(kop, ta.key[0] + (long)((r * SK + j) * 2 + co) * N, tid);
    }
    if (tid == 0) {
        __hip_atomic_fetch_or(ctr + 2, 1u << xcc_id(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // performed before this workgroup's first arrival is counted
    }
    load_twiddles(tw, ta.tw, tid);
    unsigned epoch = 0;
    // step s_ writes: a product the ping-pong buffers (the last one ep_out), trace step t = s_ - n_ep buf[t & 1]
    auto out_of = [&](int s_) -> GlweRef { return s_ < n_ep ? (s_ == n_ep - 1 ? ta.ep_out : ta.buf[s_ & 1]) : ta.buf[(s_ - n_ep) & 1]; };
#pragma unroll 1
    for (; s < n_all; s++) {
        const GlweRef rin = (s == 0) ? FK_TAIL_SRC : out_of(s - 1);
        const GlweRef rout = out_of(s);
        const int32_t* ap = rin.p + ct * rin.sy + cx * rin.sx;
        int32_t* op = rout.p + ct * rout.sy + cx * rout.sx;
        const bool is_ep = s < n_ep;
        const int t = s - n_ep;                // trace step index (is_ep: negative)
        const int ginv = is_ep ? 1 : ta.ginv[t];
        const bool stepped = (t > 0);          // the input already is rsh1(a): written by the previous TRACE step of this launch
        const bool fresh = (s == 0);           // the input was written by an earlier launch: ordinary loads
        const bool last = (s + 1 == n_all);
        double* const bigg = big0 + (long)(s & 1) * TAIL_GROUPS * BIG_STRIDE * SX;
        TSTAMP(0);
        if (is_ep) {
            // ---- fine phase of a product: partial[co][j][r] = INTT(NTT(a.col0 limb r) . G[2r][j][co] + NTT(a.col1 limb r) . G[2r+1][j][co])
            if (ep_member) {
                double x[2][E];
                if (fresh) {
#pragma unroll
                    for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
                        for (int k = 0; k < E; k++) x[c2][k] = (double)gload_i32(ap + glwe_off(r, c2), (unsigned)(tid + T * k) * 4u);
                } else {
#pragma unroll
                    for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
                        for (int k = 0; k < E; k++) x[c2][k] = (double)ld_l2(ap + glwe_off(r, c2) + tid + T * k);
                }
                ntt_fwd<2>(x, tw, data, tid);
                double acc[1][E];
#pragma unroll
                for (int k = 0; k < E; k++) acc[0][k] = 0.0;
                mac_regs(acc[0], x[0], kop);
                mac_regs(acc[0], x[1], kop1);
                if (s + 1 < n_ep) {
                    load_ops(kop, FK_TAIL_OPND(s + 1) + (long)(((2 * r) * SG + je) * 2 + coe) * N, tid);
                    load_ops(kop1, FK_TAIL_OPND(s + 1) + (long)(((2 * r + 1) * SG + je) * 2 + coe) * N, tid);
                }
                ntt_inv<1, false>(acc, tw, data, tid);
                double* bgp = bigg + (long)((coe * SG + je) * SX + r) * N;
#pragma unroll
                for (int k = 0; k < E; k++) bgp[tid + T * k] = acc[0][k];
            }
            if (s + 1 == n_ep && !last) load_ops(kop, ta.key[0] + (long)((r * SK + j) * 2 + co) * N, tid);   // the first trace step's operand (every member)
        } else {
        // ---- fine phase: x = rsh1(a); partial[co][j][r] = INTT(NTT(phi_g(x.mask limb r)) . K[r][j][co]) (+ phi_g(x.body limb j))
        // staging: thread t brings coefficients 8t .. 8t+7 (natural order) of the limb polynomials it needs
        if (stepped) {
            int v[E];
#pragma unroll
            for (int q = 0; q < E / 2; q++) ld_l2_pair(ap + glwe_off(r, 1) + E * tid + 2 * q, v[2 * q], v[2 * q + 1]);
#pragma unroll
            for (int k = 0; k < E; k++) mstage[E * tid + k] = v[k];
        } else {
            // the source: written by an earlier launch (ordinary 16-byte loads) or by the last product of this one (past the L1)
            int rm[SX][E];
            if (fresh) {
#pragma unroll
                for (int q = 0; q < SX; q++)
#pragma unroll
                    for (int h = 0; h < E / 4; h++) {
                        const int4 v4 = *reinterpret_cast<const int4*>(ap + glwe_off(q, 1) + E * tid + 4 * h);
                        rm[q][4 * h] = v4.x; rm[q][4 * h + 1] = v4.y; rm[q][4 * h + 2] = v4.z; rm[q][4 * h + 3] = v4.w;
                    }
            } else {
#pragma unroll
                for (int q = 0; q < SX; q++)
#pragma unroll
                    for (int h = 0; h < E / 2; h++) ld_l2_pair(ap + glwe_off(q, 1) + E * tid + 2 * h, rm[q][2 * h], rm[q][2 * h + 1]);
            }
#pragma unroll
            for (int k = 0; k < E; k++) {
                int xi[SX], xm[SX];
#pragma unroll
                for (int q = 0; q < SX; q++) xi[q] = rm[q][k];
                rsh1_coeff<SX>(xi, xm);
                mstage[E * tid + k] = sel_limb(xm, r);
            }
        }
        __syncthreads();
        TSTAMP(1);
        double x[1][E];
        {
            int sidx = (tid * ginv) & (2 * N - 1);
            const int sstep = (T * ginv) & (2 * N - 1);
#pragma unroll
            for (int k = 0; k < E; k++) {
                x[0][k] = (double)cneg(mstage[sidx & (N - 1)], sidx >= N);
                sidx = (sidx + sstep) & (2 * N - 1);
            }
        }
        ntt_fwd<1>(x, tw, data, tid);        // starts with a barrier: every gather of the staged limbs is done
        TSTAMP(2);
        double acc[1][E];
#pragma unroll
        for (int k = 0; k < E; k++) acc[0][k] = 0.0;
        mac_regs(acc[0], x[0], kop);
        if (!last) load_ops(kop, ta.key[t + 1] + (long)((r * SK + j) * 2 + co) * N, tid);   // arrives during the rest of the step
        ntt_inv<1, false>(acc, tw, data, tid);
        TSTAMP(3);
        {
            double* bgp = bigg + (long)((co * SK + j) * SX + r) * N;
#pragma unroll
            for (int k = 0; k < E; k++) bgp[tid + T * k] = acc[0][k];
        }
        }
        if (ta.give_up_at == s && g == 0 && m == 5) {
            if (tid == 0) __hip_atomic_store(abortp, ta.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        TSTAMP(4);
        if (!tail_barrier(ctr, abortp, ta.seq, (++epoch) * G, flag, s == 0, tid)) break;
        TSTAMP(5);
        // ---- normalisation phase: one thread per (column, coefficient); same arithmetic as k_keyswitch_norm<KS_TRACE> / k_ext_product_fine_norm.
        // Every member takes an equal share of each column (CH consecutive coefficients: the phase is as long as its busiest
        // member's L2 reads; with T per member a third of the members had none).  The next fine phase of a TRACE step needs the mask
        // column only: the members announce themselves when their share of it is stored and do the body column under the hand-off's
        // latency (nobody reads it before the next normalisation phase; the partials are double buffered by step parity for
        // that, see k_chain_mid).  A product's next fine phase reads both columns.
        constexpr int CH = (N + G - 1) / G;
        static_assert(CH <= T, "one coefficient per thread and column");
        auto norm_share = [&](const int nco) {
            const int i = m * CH + tid;
            if (tid < CH && i < N) {
                const double* bgp = bigg + (long)nco * SK * SX * N + i;
                double v_[SK];
#pragma unroll
                for (int q = 0; q < SK; q++) {
                    v_[q] = ld_l2(bgp + (long)(q * SX) * N);
#pragma unroll
                    for (int w = 1; w < SX; w++) v_[q] += ld_l2(bgp + (long)(q * SX + w) * N);   // exact: integers below 2^47
                }
                int raw[SX], xa[SX];
#pragma unroll
                for (int q = 0; q < SX; q++) raw[q] = ld_l2(ap + glwe_off(q, nco) + i);
                // vec_znx_big_add_small_inplace of the body column seen through phi_g (column 0 only): it joins the sums here,
                // where every member has the same share of it, instead of lengthening the fine phase of the three members that owned it
                const int si = (i * ginv) & (2 * N - 1);
                int braw[SX], xb[SX];
#pragma unroll
                for (int q = 0; q < SX; q++) braw[q] = (nco == 0) ? ld_l2(ap + glwe_off(q, 0) + (si & (N - 1))) : 0;
                if (stepped) {
#pragma unroll
                    for (int q = 0; q < SX; q++) { xa[q] = raw[q]; xb[q] = braw[q]; }
                } else {
                    rsh1_coeff<SX>(raw, xa);
                    rsh1_coeff<SX>(braw, xb);
                }
                double carry = 0.0;
                int d[SO], y[SO];
#pragma unroll
                for (int q = SK - 1; q >= 0; q--) {
                    double v = v_[q];
                    if (q < SX) v += (double)xa[q < SX ? q : 0] + (double)cneg(xb[q < SX ? q : 0], si >= N);
                    v += carry;
                    const double cy = carry_of(v);
                    carry = cy;
                    if (q < SO) d[q < SO ? q : 0] = (int)digit_of(v, cy);
                }
                if (last) {
#pragma unroll
                    for (int q = 0; q < SO; q++) y[q] = d[q];
                } else {
                    rsh1_coeff<SO>(d, y);
                }
#pragma unroll
                for (int q = 0; q < SO; q++) op[glwe_off(q, nco) + i] = y[q];
            }
        };
        // a product's: the sums over the three digits' partials, the limb walk, the normalised limbs as they are (they ARE the next product's digits)
        auto norm_share_ep = [&](const int nco) {
            const int i = m * CH + tid;
            if (tid < CH && i < N) {
                const double* bgp = bigg + (long)nco * SG * SX * N + i;
                double v_[SG];
#pragma unroll
                for (int q = 0; q < SG; q++) {
                    v_[q] = ld_l2(bgp + (long)(q * SX) * N);
#pragma unroll
                    for (int w = 1; w < SX; w++) v_[q] += ld_l2(bgp + (long)(q * SX + w) * N);   // exact: integers below 2^47
                }
                double carry = 0.0;
#pragma unroll
                for (int q = SG - 1; q >= 0; q--) {
                    const double v = v_[q] + carry;
                    const double cy = carry_of(v);
                    carry = cy;
                    if (q < SO) op[glwe_off(q, nco) + i] = (int)digit_of(v, cy);
                }
            }
        };
        if (is_ep) {
            norm_share_ep(1);
            norm_share_ep(0);
            TSTAMP(6);
            if (!last) { if (!tail_barrier(ctr, abortp, ta.seq, (++epoch) * G, flag, false, tid)) break; }
        } else {
        norm_share(1);
        if (last) {
            norm_share(0);
            TSTAMP(6);
        } else {
            tail_arrive(ctr, tid);
            norm_share(0);
            TSTAMP(6);
            ++epoch;
            if (!tail_wait(ctr, abortp, ta.seq, epoch * G, flag, tid)) break;
        }
        }
        TSTAMP(7);
    }
    }   // (ro_mon: every wave has flushed its maximum)
    // the last workgroup of the group to leave (every one passes here exactly once, given up or not) rewinds the
    // group's words for the next launch: nobody can still be waiting on them
    // The two host words (ta.host_done: [0] done, [16] gave up; host/tail_wait.hpp reads them): a workgroup that leaves early says so
    // before it is counted as gone; the last group to be gone — one more counter, across the launch's n_ct active groups, sync[8*32 + 3] —
    // publishes the launch's generation behind a system-scope fence.  The host then knows, without waiting for the end of this kernel and of
    // the predicated launch behind it, that every store of the launch is done and that the fallback will not run.
    if (ta.host_done) {
        if (s < n_all && tid == 0) __hip_atomic_store(ta.host_done + 16, ta.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its last step's stores, its monitor flush and that word have been performed
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (unsigned)(G - 1)) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ta.host_done) {
                const unsigned gone = __hip_atomic_fetch_add(abortp + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (gone == (unsigned)(ta.n_ct - 1)) {
                    __hip_atomic_store(abortp + 3, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __threadfence_system();
                    __hip_atomic_store(ta.host_done, ta.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
    }
}
#undef FK_TAIL_OPND
#undef FK_TAIL_SRC

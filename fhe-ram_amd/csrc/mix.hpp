// fheram_bank_read_mix: a read list, a table read and a register read of one bank as ONE operation.
//
// The three reads of a VM step — the fetch (fheram_bank_table_read), rs1 / rs2 (fheram_bank_regs_read) and the data read
// (fheram_bank_read_list) — take their addresses and selectors from one derive list launch and are independent of each other, yet each
// ends in its own pass through the latency-bound end of a read: the prepared digits, the products, trace(0, log N) on a handful of
// ciphertexts.  Here the groups go their own ways until every ciphertext is a packed row — the list through read_local (path.hpp), a
// table's or a register file's row is one already — and share ONE top over the Y = (n_list + n_table + n_regs) * ws ciphertexts, laid
// out [list | table | regs]:
//   TAIL form      Y <= 8, cfg.tail_ep, chain_form answers Tail and every ciphertext has 0 or 2 .. TAIL_EP_MAX digits: ONE launch of
//                  k_trace_tail_x (mix.hip), whose groups read their source pointer, digits and product count from the argument struct — no
//                  gather launch — and behind it the predicated fallback: k_read_chain_x for the ciphertexts with products, k_keyswitch_chain
//                  for those without (a list entry of a one-coordinate bank).  They share the tail's predicate word and generation.
//   UNFUSED form   otherwise (Y > 8, a 1- or 5-digit selector, tail_ep = 0, tail = 0, safe): the products entry by entry with ep_chain,
//                  straight from the rows into the mix's buffers (ep_chain is out of place from any source, so the one-row groups need no
//                  gather; a list entry without products is copied there), then ONE trace_steps over all Y ciphertexts in the form
//                  chain_form gives it (Tail without products, Mid, Chain, Steps).
// CONTRACT-COMPATIBLE ONLY, as its parts are: entry k of a group is int64-identical to output k of that group's single
// call, and the bank is left where the sequence read_list, table_read, regs_read leaves it.  The outputs live in the mix's own buffers;
// where the last operation of a kind left its outputs is the bank's ResHome of that kind (path.hpp), which select_source and the three
// _result downloads follow.  An empty group leaves its kind's last outputs readable: the mix has three result buffers and writes the one
// no empty kind's home is in.  Buffers are allocated whole by the first call; no operation allocates (the list group grows the read
// list's dense set as fheram_bank_read_list does).
//
// This file has two parts: what mix.hip (the kernels' translation unit) and fheram.hip share — the argument structs and the launchers —
// and, for fheram.hip only, the host logic.
#pragma once
#include "kernels.hpp"

namespace fk {

constexpr int MIX_GROUPS = 8;       // ciphertexts of the tail form: one per group of k_trace_tail_x (TAIL_GROUPS)
struct MixGroupArgs {               // by value: no table in device memory, nothing to stage
    const int32_t* src[MIX_GROUPS];     // ciphertext y itself, ONE GLWE (3 limbs): a packed row in an arena, row w of a table, of a register file
    const double* ggsw[MIX_GROUPS];     // its prepared digits, ggsw_stride elements apart (nullptr: none)
    int n_ep[MIX_GROUPS];               // its product count: 0, or 2 .. TAIL_EP_MAX
    long ggsw_stride;                   // elements of one prepared GGSW
};
struct TailMixArgs : TailArgs { MixGroupArgs x; };          // (src, n_ep and ggsw of TailArgs are not read)
struct RowChainMixArgs : RowChainArgs { MixGroupArgs x; };  // (ep.src, ep.n and ep.ggsw of RowChainArgs are not read)
// the kernels' dynamic LDS (what LDSATTR does for the kernels of fheram.hip)
hipError_t mix_register();
// sk: the limb count of the context's trace keys (4 or 5).  grid: TAIL_GROUPS * 2 * sk * 3 / (1, n_ct)
void trace_tail_x_launch(int sk, hipStream_t stream, const TailMixArgs& ta);
void read_chain_x_launch(int sk, int n_ct, hipStream_t stream, const RowChainMixArgs& ra);

}  // namespace fk

#ifndef FK_MIX_KERNELS_ONLY
#include "table.hpp"

namespace {

static_assert(FHERAM_MIX_MAX == MIX_GROUPS && MIX_GROUPS == TAIL_GROUPS, "a mix of FHERAM_MIX_MAX entries of one ciphertext is one tail launch");
static_assert(FHERAM_MIX_MAX <= FHERAM_READ_LIST_MAX && FHERAM_MIX_MAX <= FHERAM_SELECT_MAX, "every group of a mix is a call its single operation takes");

// the mix's buffers, whole (path.hpp MixBufs), and the two kernels' LDS attribute
int mix_reserve(fheram_bank* b) {
    fheram_ctx* c = b->c;
    if (b->mix.cap) return FHERAM_OK;
    MixBufs nw;
    nw.cap = std::min(FHERAM_MIX_MAX * b->mws, 64);
    const size_t ct = (size_t)nw.cap * fheram_ctx::GLWE * sizeof(int32_t);
    hipError_t e = mix_register();
    for (int32_t** p : {&nw.ep, &nw.tmp, &nw.res[0], &nw.res[1], &nw.res[2]}) if (e == hipSuccess) e = hipMalloc((void**)p, ct);
    if (e == hipSuccess) e = hipHostMalloc((void**)&nw.h_res, ct * 2 + sizeof(int64_t), hipHostMallocMapped);   // int64, + the monitor's maximum
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&nw.d_h_res, nw.h_res, 0);
    if (e != hipSuccess) {
        mix_bufs_free(nw);
        (void)hipGetLastError();   // the next op's error check must not see this allocation's failure
        return fail(c, FHERAM_ERR_DEVICE, std::string("buffers of the bank's mixed reads: ") + hipGetErrorString(e));
    }
    b->mix = nw;
    return FHERAM_OK;
}

// one entry of the top: its ws ciphertexts sit sy elements apart from src on; d products with the prepared digits at prep (d == 0: none)
struct MixEntry { const int32_t* src; long sy; const double* prep; int d; };

// The TAIL form: the products of every entry and trace(0, log N) of all n_ent * ws ciphertexts as ONE launch, and its fallback.
// ep: where a ciphertext's last product lands (the trace chain's source); b: the trace chain's buffers (launch.hpp chain_bufs);
// n0: the first n0 ciphertexts have no products and sit pk.sy apart from pk.p on (the list group of a one-coordinate bank).
void mix_tail_launch(fheram_ctx* c, const MixEntry* ent, int n_ent, int ws, GlweRef pk, int n0, GlweRef ep, const GlweRef (&b)[2]) {
    const int n = LOGN, Y = n_ent * ws;
    ProfScope ps(c, "keyswitch", (uint64_t)Y, n);
    ProfScope pt(c, "keyswitch_tail_launch", (uint64_t)Y * n, 1);
    TailMixArgs ta;
    ta.src = ep;   // (not read: every group has its own)
    ta.buf[0] = b[0]; ta.buf[1] = b[1]; ta.tw = c->d_tw; ta.big = big_of(c); ta.sync = c->d_tail_sync;
    ta.n_ep = 0; ta.ep_out = ep;
    ta.host_done = c->d_h_tail_done;
    for (int i = 0; i < TAIL_EP_MAX; i++) ta.ggsw[i] = nullptr;
    ta.x = MixGroupArgs{};
    ta.x.ggsw_stride = (long)fheram_ctx::GGSW;
    bool any_ep = false;
    for (int e = 0; e < n_ent; e++)
        for (int w = 0; w < ws; w++) {
            const int y = e * ws + w;
            ta.x.src[y] = ent[e].src + (long)w * ent[e].sy; ta.x.ggsw[y] = ent[e].d ? ent[e].prep : nullptr; ta.x.n_ep[y] = ent[e].d;
            any_ep = any_ep || ent[e].d > 0;
        }
    if (++c->tail_seq == 0) ++c->tail_seq;
    c->tail_launches++;
    if (c->cfg.tail_test != 1 && c->tail_launches - c->tail_launch_mark >= 64) {   // the watch of launch_trace_tail
        const unsigned fb = *(volatile unsigned*)c->h_tail_fb;
        if (fb - c->tail_fb_mark > 16) c->cfg.tail = 0;      // takes effect from the next chain on
        c->tail_fb_mark = fb;
        c->tail_launch_mark = c->tail_launches;
    }
    // the give-up step of the test hook is counted on group 0's own steps: late, every buffer but the sources has been overwritten by then
    ta.seq = c->tail_seq; ta.n = n; ta.n_ct = Y; ta.gx = 1; ta.xoff = c->tail_xoff; ta.give_up_at = c->cfg.tail_test ? ent[0].d + n - 2 : -1;
    for (int i = 0; i < n; i++) { ta.key[i] = trace_key(c, i); ta.ginv[i] = galois_inv_mod(galois_mod(c->gal[i])); }
    trace_tail_x_launch(c->s_evk, c->cur, ta);
    // the fallback, predicated on the tail's abort word and generation: the ciphertexts with products as ONE launch of the fused row chain
    // with the same per-ciphertext arguments, those without as the trace chain
    const GlweRef last = b[(n - 1) & 1];
    const unsigned* pred = c->d_tail_sync + TAIL_GROUPS * 32;
    if (any_ep) {
        RowChainMixArgs ra;
        fill_row_chain(c, ra, nullptr, 0, 0, n);
        ra.ep.src = ep; ra.ep.buf[0] = ra.ep.buf[1] = ep; ra.store_ep = 0;
        ra.ks.base = ks_args(c, last, last, last, trace_key(c, 0), c->gal[0]);
        ra.ks.buf[0] = ra.ks.buf[1] = last;      // only the last step stores
        ra.hi = ra.trhi = last;
        ra.ks.pred = pred; ra.ks.pred_seq = ta.seq; ra.ks.host_count = c->h_tail_fb;
        ra.x = ta.x;
        c->wide_unsynced = true;                 // (the whole register file, as every k_read_chain_t launch)
        read_chain_x_launch(c->s_evk, Y, c->cur, ra);
    }
    if (n0) {
        KsChainArgs ca;
        ca.base = ks_args(c, pk, pk, b[0], trace_key(c, 0), c->gal[0], 0, 0, 0);
        ca.buf[0] = b[0]; ca.buf[1] = b[1]; ca.n = n;
        ca.pred = pred; ca.pred_seq = ta.seq; ca.host_count = c->h_tail_fb;
        for (int i = 0; i < n; i++) { ca.key[i] = ta.key[i]; ca.ginv[i] = ta.ginv[i]; }
        with_evk(c, [&](auto sk) {
            constexpr int SK = decltype(sk)::value;
            hipLaunchKernelGGL((k_keyswitch_chain<3, SK, 3>), dim3(1, n0, 1), dim3(T), LDS_BYTES, c->cur, ca);
        });
    }
}

}  // namespace

extern "C" {

int fheram_bank_read_mix(fheram_bank* b, const fheram_mix_reads* r, int64_t* list_out, int64_t* table_out, int64_t* regs_out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (!r) return fail(c, FHERAM_ERR_INVALID_ARG, "null reads");
    const int nl = r->n_list, nt = r->n_table, nr = r->n_regs;
    if (nl < 0 || nt < 0 || nr < 0) return fail(c, FHERAM_ERR_INVALID_ARG, "a group of the mix has a negative count");
    const int n = nl + nt + nr, ws = b->mws, Y = n * ws;
    if (n < 1) return fail(c, FHERAM_ERR_INVALID_ARG, "the mix names no read: all three groups are empty");
    if (n > FHERAM_MIX_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n_list + n_table + n_regs = " + std::to_string(n) + " exceeds FHERAM_MIX_MAX = " + std::to_string(FHERAM_MIX_MAX));
    if (Y > 64)
        return fail(c, FHERAM_ERR_INVALID_ARG, "(n_list + n_table + n_regs) * word_size = " + std::to_string(Y) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    MemberSet s;
    if (nl) {   // the rules of fheram_bank_read_list
        if (!r->members || !r->addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null member list or null address list");
        for (int k = 0; k < nl; k++)
            if (r->members[k] < 0 || r->members[k] >= b->M)
                return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names member " + std::to_string(r->members[k]) + ", outside the bank's " + std::to_string(b->M) + " members");
        s = MemberSet::list(r->members, nl);
        const int rc = members_ready(b, s, r->addrs, 0);
        if (rc != FHERAM_OK) return rc;
    }
    if (nt) {   // ... of fheram_bank_table_read
        if (!r->tables || !r->table_sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null table list or null selector list");
        for (int k = 0; k < nt; k++) {
            const std::string who = "table selector " + std::to_string(k);
            const int rc = table_check_handle(b, r->tables[k], "table " + std::to_string(k));
            if (rc != FHERAM_OK) return rc;
            const fheram_selector* sel = r->table_sels[k];
            if (!sel || sel->bank != b) return fail(c, FHERAM_ERR_INVALID_ARG, who + " is null or belongs to another bank");
            if (sel->empty) return fail(c, FHERAM_ERR_INVALID_ARG, who + " is empty: fheram_bank_table_selector_alloc without fheram_bank_selector_derive");
            if (sel->bits != r->tables[k]->bits) return fail(c, FHERAM_ERR_INVALID_ARG, who + " has " + std::to_string(sel->bits) + " bits, table " + std::to_string(k) + " " + std::to_string(r->tables[k]->bits));
            if (sel->n_digits != r->table_sels[0]->n_digits)
                return fail(c, FHERAM_ERR_INVALID_ARG, who + " has " + std::to_string(sel->n_digits) + " digits, table selector 0 " + std::to_string(r->table_sels[0]->n_digits) + ": all selectors of the group share the digit count");
        }
        for (int k = 0; k < nt; k++)
            if (!r->tables[k]->initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: table " + std::to_string(k) + " has had no fheram_bank_table_upload or fheram_bank_table_load_plain");
    }
    if (nr) {   // ... of fheram_bank_regs_read
        int rc = regs_check_handle(b, r->regs);
        if (rc != FHERAM_OK) return rc;
        if (!r->reg_sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null selector list");
        for (int k = 0; k < nr; k++) {
            rc = regs_check_selector(b, r->regs, r->reg_sels[k], "register selector " + std::to_string(k));
            if (rc != FHERAM_OK) return rc;
            if (r->reg_sels[k]->n_digits != r->reg_sels[0]->n_digits)
                return fail(c, FHERAM_ERR_INVALID_ARG, "register selector " + std::to_string(k) + " has " + std::to_string(r->reg_sels[k]->n_digits) + " digits, register selector 0 " + std::to_string(r->reg_sels[0]->n_digits) + ": all selectors of the group share the digit count");
        }
        rc = regs_check_ready(b, r->regs, 0);
        if (rc != FHERAM_OK) return rc;
    }
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = mix_reserve(b);
    if (rc != FHERAM_OK) return rc;
    if (nl) b->list_n = 0;   // until this mix is enqueued its kinds have no last outputs (as the single calls)
    if (nl > 1) {
        rc = dense_reserve(c, b->list, nl, ws);
        if (rc != FHERAM_OK) return rc;
    }
    // ---- enqueue ----
    MixBufs& M = b->mix;
    // the result buffer no EMPTY kind's last outputs live in (at most two of the three are taken)
    int slot = 0;
    auto taken = [&](int q) {
        return (!nl && b->list_n && b->list_home.mix_slot == q) || (!nt && b->table_n && b->table_home.mix_slot == q) || (!nr && b->regs_n && b->regs_home.mix_slot == q);
    };
    while (taken(slot)) slot++;
    regs_begin(c);
    if (nt) b->table_n = 0;
    if (nr) b->regs_n = 0;
    const long G = (long)fheram_ctx::GLWE;
    const size_t per = (size_t)ws * fheram_ctx::GLWE;
    MixEntry ent[FHERAM_MIX_MAX];
    int ne = 0;
    // 1. the list group goes as far as a read list does before its top: every entry's packed row, in the arena (path.hpp read_local)
    GlweRef pk = ref(nullptr, 0, 0);
    const int d1 = c->n2 == 2 ? (int)c->base2d[1].size() : 0;
    if (nl) {
        double* tab = c->d_prep;
        long stride = 0;
        if (nl == 1) {   // the plain single-member read, on the member's own buffers
            SetPlan p(b, s, r->addrs, false);
            rc = read_local(p.o, p.v, false, &pk, false);
            read_top_done(c, &p.st, false);
            set_assign(b, s, p.st, false, false, true);
        } else {
            RamState st{true, false, false, 0, false};
            const Opnds o = table_opnds(c, &st, r->addrs, nl, ws, b->list.prep, nullptr, s.map(), b->M > 1);
            rc = read_local(o, dense_view(c, b->list), false, &pk, false);
            read_top_done(c, &st, false);
            set_assign(b, s, st, false, false, true);   // every named member: as a read leaves it
            tab = b->list.prep; stride = o.stride;
        }
        if (rc != FHERAM_OK) return rc;
        for (int k = 0; k < nl; k++)
            ent[ne++] = MixEntry{pk.p + (long)k * ws * pk.sy, pk.sy, d1 ? digits_of(c, tab + k * stride, 1) : nullptr, d1};
    }
    // 2. the one-row groups: their selectors' digits, prepared as one_row_reads does; a row is a packed row already
    const int ppd = (int)(fheram_ctx::GGSW / N);
    for (int k = 0; k < nt; k++) {
        const fheram_selector* sel = r->table_sels[k];
        double* prep = b->tabs.prep + (size_t)k * sel->n_digits * fheram_ctx::GGSW;
        launch_prepare(c, sel->d_ggsw, prep, sel->n_digits * ppd);
        ent[ne++] = MixEntry{r->tables[k]->row, G, prep, sel->n_digits};
    }
    for (int k = 0; k < nr; k++) {
        const fheram_selector* sel = r->reg_sels[k];
        double* prep = b->regs.prep + (size_t)k * sel->n_digits * fheram_ctx::GGSW;
        launch_prepare(c, sel->d_ggsw, prep, sel->n_digits * ppd);
        ent[ne++] = MixEntry{r->regs->row, G, prep, sel->n_digits};
    }
    // 3. the top, once for all Y ciphertexts
    const GlweRef ep = ref(M.ep, G, 0), tmp = ref(M.tmp, G, 0), res = ref(M.res[slot], G, 0);
    auto slice = [&](GlweRef g, int e) { g.p += (long)e * ws * g.sy; return g; };
    bool tail = Y <= TAIL_GROUPS && c->cfg.tail_ep && chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail;
    for (int e = 0; e < ne; e++) tail = tail && (ent[e].d == 0 || (ent[e].d >= 2 && ent[e].d <= TAIL_EP_MAX));
    const int n0 = (nl && !d1) ? nl * ws : 0;   // ciphertexts without products: the list group of a one-coordinate bank
    GlweRef tb[2];
    if (tail && chain_bufs(LOGN, ep, res, tmp, tb)) mix_tail_launch(c, ent, ne, ws, pk, n0, ep, tb);
    else {
        if (n0) launch_copy(c, pk, ep, 1, n0);
        for (int e = 0; e < ne; e++)
            if (ent[e].d) ep_chain(c, ref(const_cast<int32_t*>(ent[e].src), ent[e].sy, 0), slice(ep, e), slice(tmp, e), ent[e].prep, ent[e].d, 1, ws);
        trace_steps(c, ep, res, tmp, 0, LOGN, 1, Y);
    }
    // what the three single calls leave: the list's members their result in their slot of d_res, every group its kind's last outputs
    if (nl) {
        for (int m = 0; m < b->M; m++) {
            int last = -1;
            for (int k = 0; k < nl; k++) if (s.m[k] == m) last = k;
            if (last >= 0) launch_copy(c, slice(res, last), member_slot(b, c->d_res, m), 1, ws);
        }
        b->list_n = nl;
        b->list_home = ResHome{M.res[slot], M.h_res, M.d_h_res, slot};
    }
    if (nt) { b->table_n = nt; b->table_home = ResHome{M.res[slot] + (size_t)nl * per, M.h_res, M.d_h_res, slot}; }
    if (nr) { b->regs_n = nr; b->regs_home = ResHome{M.res[slot] + (size_t)(nl + nt) * per, M.h_res, M.d_h_res, slot}; }
    HIPCHK(c, hipGetLastError());
    // 4. ONE export for the groups the caller wants
    ResRun runs[3];
    int64_t* outs[3];
    int n_runs = 0;
    const int cnt[3] = {nl, nt, nr};
    int64_t* const want[3] = {list_out, table_out, regs_out};
    for (int g = 0, first = 0; g < 3; first += cnt[g], g++)
        if (cnt[g] && want[g]) { runs[n_runs] = ResRun{M.res[slot] + (size_t)first * per, (size_t)cnt[g] * per}; outs[n_runs++] = want[g]; }
    if (!n_runs) return FHERAM_OK;
    rc = result_export(c, runs, n_runs, M.h_res, M.d_h_res, nullptr);
    if (rc != FHERAM_OK) return rc;
    size_t at = 0;
    for (int i = 0; i < n_runs; i++) { std::memcpy(outs[i], M.h_res + at, runs[i].n * sizeof(int64_t)); at += runs[i].n; }
    return FHERAM_OK;
}

}  // extern "C"
#endif   // FK_MIX_KERNELS_ONLY

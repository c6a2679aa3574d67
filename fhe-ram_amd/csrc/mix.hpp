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
// where the last operation of a kind left its outputs is the bank's LastOutputs record of that kind (bank.hpp), which select_source and
// the _result downloads follow.  An empty group leaves its kind's last outputs readable: the mix has three result buffers and writes the one
// no empty kind's home is in.  Buffers are allocated whole by the first call; no operation allocates (the list group grows the read
// list's dense set as fheram_bank_read_list does).
//
// fheram_bank_read_prepare_write_mix puts the first halves of a step's writes under the same top: the prepare list goes as
// far as read_prepare_write does before its top (read_local with prepare_write: the products of coordinate 0 in the rows, the packed rows
// left where they are), rd's digits go into the register file's own, and the top runs over [list | table | regs | prepared list |
// prepared regs].  Nothing in the top writes a row or a tree; ONE launch of k_mix_scatter behind it hands over what a read_prepare_write
// keeps (a member's tree top and kept trace, the register file's rotated row and kept trace) and the list reads' results.  Int64-identical
// to read_mix, read_prepare_write_list, regs_read_prepare_write in that order, outputs and bank; it starts no early inverse digits.
// Both operations are ONE function (mix_run): without prepares it enqueues what fheram_bank_read_mix always has.
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

// fheram_bank_read_prepare_write_mix's hand-over (k_mix_scatter): run i copies ws GLWEs, one GLWE apart on both sides, from src[i] to dst[i].
// An entry of the top has at most four runs — its last product and its trace, each to the member's own slot and, under the dense plan, to
// the write lists' set as well (bank.hpp) — so FHERAM_MIX_MAX entries have at most 32.  No two runs of a launch share a destination.
constexpr int MIX_SCATTER_MAX = 32;
constexpr int MIX_SCATTER_SLICES = 8;   // workgroups per ciphertext (blockIdx.z), as the elementwise kernels (launch.hpp EW_SLICES)
struct MixScatterArgs {                 // by value: no table in device memory, nothing to stage
    const int32_t* src[MIX_SCATTER_MAX];
    int32_t* dst[MIX_SCATTER_MAX];
    int n;
};
// grid: (sa.n, ws, MIX_SCATTER_SLICES)
void mix_scatter_launch(int ws, hipStream_t stream, const MixScatterArgs& sa);

}  // namespace fk

#ifndef FK_MIX_KERNELS_ONLY
#include "table.hpp"

#include <optional>

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
    if (e == hipSuccess) e = pinned_result(&nw.h_res, &nw.d_h_res, ct);
    if (e != hipSuccess) { mix_bufs_free(nw); return reserve_failed(c, e, "buffers of the bank's mixed reads"); }
    b->mix = nw;
    return FHERAM_OK;
}

// what fheram_bank_read_prepare_write_mix adds to them (path.hpp MixBufs), whole
int mix_reserve_prepares(fheram_bank* b) {
    fheram_ctx* c = b->c;
    MixBufs& M = b->mix;
    if (M.own) return FHERAM_OK;
    const size_t glwe = fheram_ctx::GLWE * sizeof(int32_t);
    int32_t *own = nullptr, *keep = nullptr;
    double* prep = nullptr;
    hipError_t e = hipMalloc((void**)&own, (size_t)M.cap * glwe);
    if (e == hipSuccess) e = hipMalloc((void**)&keep, (size_t)b->mws * glwe);
    if (e == hipSuccess) e = hipMalloc((void**)&prep, (size_t)c->n_digits * fheram_ctx::GGSW * sizeof(double));
    if (e != hipSuccess) {
        bufs_free({own, keep, prep}, {}, {});
        return reserve_failed(c, e, "buffers of the bank's mixed read_prepare_write");
    }
    M.own = own; M.keep = keep; M.prep = prep;
    return FHERAM_OK;
}

// one entry of the top: its ws ciphertexts sit sy elements apart from src on; d products with the prepared digits at prep (d == 0: none)
struct MixEntry { const int32_t* src; long sy; const double* prep; int d; };
// a run of n ciphertexts of the top, from ciphertext y0 on, WITHOUT products, pk.sy apart from pk.p on: the list group of a one-coordinate
// bank, the prepared list of one
struct MixPlainRun { GlweRef pk; int y0, n; };

// The TAIL form: the products of every entry and trace(0, log N) of all n_ent * ws ciphertexts as ONE launch, and its fallback.
// ep: where a ciphertext's last product lands (the trace chain's source); b: the trace chain's buffers (launch.hpp chain_bufs);
// plain: the runs of ciphertexts without products; store_ep: the caller needs the last products afterwards (a prepared ciphertext's is
// what its read_prepare_write keeps), so the fallback stores them as the tail does.
void mix_tail_launch(fheram_ctx* c, const MixEntry* ent, int n_ent, int ws, const MixPlainRun* plain, int n_plain, GlweRef ep, const GlweRef (&b)[2], bool store_ep) {
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
    // with the same per-ciphertext arguments, those without as the trace chain, run by run
    const GlweRef last = b[(n - 1) & 1];
    const unsigned* pred = c->d_tail_sync + TAIL_GROUPS * 32;
    if (any_ep) {
        RowChainMixArgs ra;
        fill_row_chain(c, ra, nullptr, 0, 0, n);
        ra.ep.src = ep; ra.ep.buf[0] = ra.ep.buf[1] = ep; ra.store_ep = store_ep ? 1 : 0;
        ra.ks.base = ks_args(c, last, last, last, trace_key(c, 0), c->gal[0]);
        ra.ks.buf[0] = ra.ks.buf[1] = last;      // only the last step stores
        ra.hi = ra.trhi = last;
        ra.ks.pred = pred; ra.ks.pred_seq = ta.seq; ra.ks.host_count = c->h_tail_fb;
        ra.x = ta.x;
        c->wide_unsynced = true;                 // (the whole register file, as every k_read_chain_t launch)
        read_chain_x_launch(c->s_evk, Y, c->cur, ra);
    }
    for (int q = 0; q < n_plain; q++) {
        const MixPlainRun& r = plain[q];
        auto from = [&](GlweRef g) { g.p += (long)r.y0 * g.sy; return g; };   // the run's first ciphertext
        KsChainArgs ca;
        ca.base = ks_args(c, r.pk, r.pk, from(b[0]), trace_key(c, 0), c->gal[0], 0, 0, 0);
        ca.buf[0] = from(b[0]); ca.buf[1] = from(b[1]); ca.n = n;
        ca.pred = pred; ca.pred_seq = ta.seq; ca.host_count = c->h_tail_fb;
        for (int i = 0; i < n; i++) { ca.key[i] = ta.key[i]; ca.ginv[i] = ta.ginv[i]; }
        with_evk(c, [&](auto sk) {
            constexpr int SK = decltype(sk)::value;
            hipLaunchKernelGGL((k_keyswitch_chain<3, SK, 3>), dim3(1, r.n, 1), dim3(T), LDS_BYTES, c->cur, ca);
        });
    }
}

// The checks of the three read groups, each with the rules and codes of its single call; s: the list group's members.
int mix_check_reads(fheram_bank* b, const fheram_mix_reads* r, MemberSet* s) {
    fheram_ctx* c = b->c;
    const int nl = r->n_list, nt = r->n_table, nr = r->n_regs;
    if (nl) {   // the rules of fheram_bank_read_list
        if (!r->members || !r->addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null member list or null address list");
        for (int k = 0; k < nl; k++)
            if (r->members[k] < 0 || r->members[k] >= b->M)
                return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names member " + std::to_string(r->members[k]) + ", outside the bank's " + std::to_string(b->M) + " members");
        *s = MemberSet::list(r->members, nl);
        const int rc = members_ready(b, *s, r->addrs, 0);
        if (rc != FHERAM_OK) return rc;
    }
    if (nt) {   // ... of fheram_bank_table_read
        if (!r->tables || !r->table_sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null table list or null selector list");
        const int rc = table_check_reads(b, r->tables, r->table_sels, nt, "table selector ", "all selectors of the group share the digit count");
        if (rc != FHERAM_OK) return rc;
    }
    if (nr) {   // ... of fheram_bank_regs_read
        int rc = regs_check_handle(b, r->regs);
        if (rc != FHERAM_OK) return rc;
        if (!r->reg_sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null selector list");
        rc = regs_check_reads(b, r->regs, r->reg_sels, nr, "register selector ", "all selectors of the group share the digit count");
        if (rc != FHERAM_OK) return rc;
    }
    return FHERAM_OK;
}

// Both operations, behind their checks.  r: the reads (every count 0: none); p: the prepares, nullptr for fheram_bank_read_mix — then this
// enqueues exactly what that operation always has.  s / sp: the members of the read list / of the prepare list.
int mix_run(fheram_bank* b, const fheram_mix_reads* r, const MemberSet& s, const fheram_mix_prepares* p, const MemberSet& sp,
            int64_t* list_out, int64_t* table_out, int64_t* regs_out, int64_t* prep_list_out, int64_t* prep_regs_out) {
    fheram_ctx* c = b->c;
    const int nl = r->n_list, nt = r->n_table, nr = r->n_regs, np = p ? p->n_list : 0, npr = (p && p->regs) ? 1 : 0;
    const int ws = b->mws, Y = (nl + nt + nr + np + npr) * ws;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = mix_reserve(b);
    if (rc == FHERAM_OK && p) rc = mix_reserve_prepares(b);
    if (rc != FHERAM_OK) return rc;
    const bool p_dense = np && !sp.is_range();
    if (p_dense) {   // the dense plan's buffers (bank.hpp bank_read_set)
        rc = dense_reserve(c, b->wl, np, ws, true, &b->wl_fail_alloc);
        if (rc != FHERAM_OK) return rc;
    }
    LastOutputs* const last = b->last;
    if (nl) last[LAST_LIST].n = 0;   // until this mix is enqueued its kinds have no last outputs (as the single calls)
    if (nl > 1) {
        rc = dense_reserve(c, b->list, nl, ws);
        if (rc != FHERAM_OK) return rc;
    }
    // ---- enqueue ----
    MixBufs& M = b->mix;
    // the result buffer no EMPTY kind's last outputs live in (at most two of the three are taken while a read group is not empty; a call
    // without reads has the fourth)
    int slot = 0;
    auto holds = [&](int cnt, LastKind kind, int q) { return !cnt && last[kind].n && last[kind].home.mix_slot == q; };
    auto taken = [&](int q) { return holds(nl, LAST_LIST, q) || holds(nt, LAST_TABLE, q) || holds(nr, LAST_REGS, q); };
    const bool reads = nl + nt + nr > 0;
    while (reads && taken(slot)) slot++;
    int32_t* const resbuf = reads ? M.res[slot] : M.own;
    regs_begin(c);
    if (nt) last[LAST_TABLE].n = 0;
    if (nr) last[LAST_REGS].n = 0;
    const long G = (long)fheram_ctx::GLWE;
    const size_t per = (size_t)ws * fheram_ctx::GLWE;
    MixEntry ent[FHERAM_MIX_MAX];
    MixPlainRun plain[2];
    int ne = 0, n_plain = 0;
    // 1. the list group goes as far as a read list does before its top: every entry's packed row, in the arena (path.hpp read_local)
    GlweRef pk = ref(nullptr, 0, 0);
    const int d1 = c->n2 == 2 ? (int)c->base2d[1].size() : 0;
    if (nl) {
        double* tab = c->d_prep;
        long stride = 0;
        if (nl == 1) {   // the plain single-member read, on the member's own buffers
            SetPlan pl(b, s, r->addrs, false);
            rc = read_local(pl.o, pl.v, false, &pk, false);
            read_top_done(c, &pl.st, false);
            set_assign(b, s, pl.st, false, false, true);
            // a prepare list in place on this member runs on the same arenas before the top has read the packed row: it moves out of the way
            if (rc == FHERAM_OK && np && !p_dense && s.m[0] >= sp.m[0] && s.m[0] < sp.m[0] + np) {
                launch_copy(c, pk, ref(M.keep, G, 0), 1, ws);
                pk = ref(M.keep, G, 0);
            }
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
        if (!d1) plain[n_plain++] = MixPlainRun{pk, 0, nl * ws};
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
    // 3. the prepare list, behind the list group (a member named in both is read first): read_prepare_write as far as its top, on the plan
    // bank_read_set would build.  The products of coordinate 0 land in the rows; the packed rows stay where the last launch left them.
    // One member: its digits in the mix's own slots (the context's may hold the list group's until the top has run), and none of the
    // lone read_prepare_write's machinery is left armed (read_local parks no gate wave here: nothing follows that would release it).
    std::optional<SetPlan> pp;
    const int first_p = ne;
    if (np) {
        if (p_dense) b->kept_alone = 0;   // arena A is this operation's from here on
        pp.emplace(b, sp, p->addrs, false);
        Opnds o = pp->o;
        if (np == 1) o.tab = M.prep;
        const bool opstart = c->opstart_valid;
        GlweRef ppk;
        rc = read_local(o, pp->v, true, &ppk, false);
        c->wide = true; c->opstart_valid = opstart;
        read_top_done(c, &pp->st, true);
        if (rc == FHERAM_OK && p_dense) { b->kept_alone = pp->st.memo_alone; b->kept_n = np; b->kept_map = o.member_map; }
        set_assign(b, sp, pp->st, p_dense, rc == FHERAM_OK, true);   // ram.rs:533
        if (rc != FHERAM_OK) return rc;
        for (int k = 0; k < np; k++)
            ent[ne++] = MixEntry{ppk.p + (long)k * ws * ppk.sy, ppk.sy, d1 ? digits_of(c, o.tab + k * o.stride, 1) : nullptr, d1};
        if (!d1) plain[n_plain++] = MixPlainRun{ppk, first_p * ws, np * ws};
    }
    if (npr) {   // rd: the selector's digits into the register file's own (fheram_bank_regs_read_prepare_write)
        const fheram_selector* sel = p->reg_sel;
        launch_prepare(c, sel->d_ggsw, p->regs->prep, sel->n_digits * ppd);
        ent[ne++] = MixEntry{p->regs->row, G, p->regs->prep, sel->n_digits};
    }
    // 4. the top, once for all Y ciphertexts.  Nothing in it writes a row or a tree: the register file's row is intact for every read of it.
    const GlweRef ep = ref(M.ep, G, 0), tmp = ref(M.tmp, G, 0), res = ref(resbuf, G, 0);
    auto slice = [&](GlweRef g, int e) { g.p += (long)e * ws * g.sy; return g; };
    bool tail = Y <= TAIL_GROUPS && c->cfg.tail_ep && chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail;
    for (int e = 0; e < ne; e++) tail = tail && (ent[e].d == 0 || (ent[e].d >= 2 && ent[e].d <= TAIL_EP_MAX));
    GlweRef tb[2];
    if (tail && chain_bufs(LOGN, ep, res, tmp, tb)) mix_tail_launch(c, ent, ne, ws, plain, n_plain, ep, tb, p != nullptr);
    else {
        for (int q = 0; q < n_plain; q++) launch_copy(c, plain[q].pk, slice(ep, plain[q].y0 / ws), 1, plain[q].n);
        for (int e = 0; e < ne; e++)
            if (ent[e].d) ep_chain(c, ref(const_cast<int32_t*>(ent[e].src), ent[e].sy, 0), slice(ep, e), slice(tmp, e), ent[e].prep, ent[e].d, 1, ws);
        trace_steps(c, ep, res, tmp, 0, LOGN, 1, Y);
    }
    // what the single calls leave: the list's members their result in their slot of d_res, every group its kind's last outputs; a prepared
    // member its tree top and its trace where its read_prepare_write puts them, the register file its rotated row and its kept trace —
    // entry by entry for fheram_bank_read_mix, as ONE launch with the prepares' hand-over otherwise
    MixScatterArgs sa{};
    auto hand = [&](GlweRef from, GlweRef to) {
        if (!p) { launch_copy(c, from, to, 1, ws); return; }
        for (int i = 0; i < sa.n; i++) if (sa.dst[i] == to.p) return;   // (a member read AND prepared with memo = 0: its slot of d_res is the preparation's)
        sa.src[sa.n] = from.p; sa.dst[sa.n++] = to.p;
    };
    for (int k = 0; k < np; k++) {
        const int e = first_p + k, m = sp.m[k];
        const bool in_trtop = pp->st.res_in_trtop;
        if (c->n2 == 2) {   // tree[0] <- the rotated packed row (ram.rs:525-527)
            hand(slice(ep, e), pp->o.slice(ref(pp->v.tree, G, 0), k));
            if (p_dense) hand(slice(ep, e), member_slot(b, c->d_tree, m));
        }
        hand(slice(res, e), pp->o.slice(ref(in_trtop ? pp->v.trtop : pp->v.res, G, 0), k));
        if (p_dense) hand(slice(res, e), member_slot(b, in_trtop ? c->d_trtop : c->d_res, m));
    }
    if (npr) {
        fheram_regs* rf = p->regs;
        hand(slice(ep, ne - 1), ref(rf->row, G, 0));   // the rotated row (ram.rs:502-504, rows == 1)
        hand(slice(res, ne - 1), ref(rf->tr, G, 0));   // ram.rs:540; = what write_first_step computes first
        rf->state = true;                              // ram.rs:533
        rf->memo = c->cfg.memo != 0;
        b->regs_old = rf->tr; b->regs_old_owner = rf;
    }
    if (nl) {
        for (int m = 0; m < b->M; m++) {
            int last = -1;
            for (int k = 0; k < nl; k++) if (s.m[k] == m) last = k;
            if (last >= 0) hand(slice(res, last), member_slot(b, c->d_res, m));
        }
        last[LAST_LIST] = LastOutputs{nl, ResHome{resbuf, M.h_res, M.d_h_res, slot}};
    }
    if (p) {
        ProfScope ps(c, "elementwise", (uint64_t)sa.n * ws);
        mix_scatter_launch(ws, c->cur, sa);
    }
    if (nt) last[LAST_TABLE] = LastOutputs{nt, ResHome{resbuf + (size_t)nl * per, M.h_res, M.d_h_res, slot}};
    if (nr) last[LAST_REGS] = LastOutputs{nr, ResHome{resbuf + (size_t)(nl + nt) * per, M.h_res, M.d_h_res, slot}};
    HIPCHK(c, hipGetLastError());
    // 5. ONE export for the groups the caller wants
    ResRun runs[5];
    int64_t* outs[5];
    int n_runs = 0;
    const int cnt[5] = {nl, nt, nr, np, npr};
    int64_t* const want[5] = {list_out, table_out, regs_out, prep_list_out, prep_regs_out};
    for (int g = 0, first = 0; g < 5; first += cnt[g], g++)
        if (cnt[g] && want[g]) { runs[n_runs] = ResRun{resbuf + (size_t)first * per, (size_t)cnt[g] * per}; outs[n_runs++] = want[g]; }
    if (!n_runs) return FHERAM_OK;
    rc = result_export(c, runs, n_runs, M.h_res, M.d_h_res, nullptr);
    if (rc != FHERAM_OK) return rc;
    size_t at = 0;
    for (int i = 0; i < n_runs; i++) { std::memcpy(outs[i], M.h_res + at, runs[i].n * sizeof(int64_t)); at += runs[i].n; }
    return FHERAM_OK;
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
    const int rc = mix_check_reads(b, r, &s);
    if (rc != FHERAM_OK) return rc;
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    return mix_run(b, r, s, nullptr, MemberSet{}, list_out, table_out, regs_out, nullptr, nullptr);
}

// The reads of a step and the first halves of its writes under one top (header comment of include/fheram.h)
int fheram_bank_read_prepare_write_mix(fheram_bank* b, const fheram_mix_reads* r, const fheram_mix_prepares* p,
                                       int64_t* list_out, int64_t* table_out, int64_t* regs_out, int64_t* prep_list_out, int64_t* prep_regs_out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing.  Reads change no state, so the state as it stands is
    // what the sequence's second and third call would find ----
    if (!p) return fail(c, FHERAM_ERR_INVALID_ARG, "null prepares");
    const fheram_mix_reads none{};
    if (!r) r = &none;
    const int nl = r->n_list, nt = r->n_table, nr = r->n_regs, np = p->n_list, npr = p->regs ? 1 : 0;
    if (nl < 0 || nt < 0 || nr < 0 || np < 0) return fail(c, FHERAM_ERR_INVALID_ARG, "a group of the mix has a negative count");
    if (np + npr < 1) return fail(c, FHERAM_ERR_INVALID_ARG, "the mix names no preparation: the prepare list is empty and there is no register file (that is fheram_bank_read_mix)");
    const long n = (long)nl + nt + nr + np + npr, Y = n * b->mws;
    if (n > FHERAM_MIX_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "the reads, the prepare list and the register file are " + std::to_string(n) + " entries, which exceeds FHERAM_MIX_MAX = " + std::to_string(FHERAM_MIX_MAX));
    if (Y > 64)
        return fail(c, FHERAM_ERR_INVALID_ARG, "entries * word_size = " + std::to_string(Y) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    MemberSet s, sp;
    int rc = mix_check_reads(b, r, &s);
    if (rc != FHERAM_OK) return rc;
    if (np) {   // the rules of fheram_bank_read_prepare_write_list
        if (!p->members || !p->addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null member list or null address list");
        rc = write_list_members(b, p->members, p->addrs, np, 0, &sp);
        if (rc != FHERAM_OK) return rc;
    }
    if (npr) {  // ... of fheram_bank_regs_read_prepare_write
        rc = regs_check_handle(b, p->regs);
        if (rc == FHERAM_OK) rc = regs_check_selector(b, p->regs, p->reg_sel, "the selector");
        if (rc == FHERAM_OK) rc = regs_check_ready(b, p->regs, 0);
        if (rc != FHERAM_OK) return rc;
    }
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    return mix_run(b, r, s, p, sp, list_out, table_out, regs_out, prep_list_out, prep_regs_out);
}

}  // extern "C"
#endif   // FK_MIX_KERNELS_ONLY

// Private to fheram.hip: Ram::read / read_prepare_write / write as launch sequences (reference: src/ram.rs).
// ONE read sequence (read_local + read_top, together read_impl) and ONE write sequence (write_side_begin, write_top, write_rows), over an
// operand set (Opnds: whose digits a product uses, whose RAM state it updates) and a view (RamView: the buffers it runs on).  The plain context, the stages of
// a row-sharded RAM (fheram.hip, group.hpp), fheram_read_batch and fheram_bank_* (bank.hpp; its read list and write lists too) all run these; what is specific to one of them
// is a visible condition in the sequence (n == 1: pre_inv, the gate wave, ev_opstart, ev_wdone, sharding, capture; a bank range or list: Opnds::bank in row_fuse).
// Several addresses are ONE kind of operand set (table_opnds: a digit table and a member map) and several reads ONE buffer set (DenseBufs, read_many).
#pragma once
#include "launch.hpp"

namespace {

// One operation's OPERAND SET: n addresses of ws ciphertexts each (Y = n * ws; ciphertext y = k * ws + w is word w of address k).
// n == 1 is the plain operation: the context's own digit slots, every `for k` loop below runs once and no launch takes a table.
// n > 1: the prepared digits of address k sit k * stride further in a table; every address-independent step is ONE launch over Y, the products
// use the table in the forms that carry one (launch.hpp OpndTable) and run one launch per address on its y-slice with the plain launchers
// everywhere else.  Never sharded, never captured, never with early inverse digits (pre_inv) then.
struct Opnds {
    fheram_ctx* c;
    RamState* st;            // the RAM(s) operated on: read and updated as the operation is enqueued (the context's own; a bank range: the merge of its members')
    const fheram_addr* const* addrs;
    int n, ws;
    double *tab, *tab_inv;   // (inverse) digits of address 0
    long stride;
    // whose rows address k works on: member (member_map >> 4k) & 15 of the view's rows, four bits per address — what the table forms take by value
    // (launch.hpp OpndTable).  n == 1 and fheram_read_batch: 0, every address the view's first ws rows; a bank range: the identity, address k
    // reads and writes member k of the range; a bank's read list: its members, of the whole bank's rows (read-only); a bank's
    // read_prepare_write / write list: its distinct members, of the whole bank's rows, read and written — every other buffer of its view is dense
    unsigned member_map;
    bool bank;               // a range or a list of a bank of several members, n > 1: row_fuse
    int member(int k) const { return (int)((member_map >> (4 * k)) & 15u); }
    // address k's rows are the view's k-th: a launch over all Y ciphertexts may touch the rows directly (else: one launch per address through rows())
    bool rows_dense() const { return map_is_identity(member_map, n); }
    int Y() const { return n * ws; }
    double* prep(int k, int ci) const { return digits_of(c, tab + k * stride, ci); }
    double* inv(int k, int ci) const { return digits_of(c, tab_inv + k * stride, ci); }
    GlweRef slice(GlweRef r, int k) const { r.p += (long)k * ws * r.sy; return r; }   // address k's ws ciphertexts
    GlweRef rows(GlweRef r, int k) const { return slice(r, member(k)); }
    // (store_mapped: a batch's and a read list's maps are not the identity either, but neither ever stores rows; it decides for the write lists)
    OpndTable table() const { return n == 1 ? OpndTable{} : OpndTable{ws, stride, member_map, !rows_dense()}; }
    // The fused row chain (k_read_chain / k_write_chain) for this operation.  A lone context — and a batch like it — splits by column while
    // rows * ws * 2 workgroups still fit the chip (pick_nco), which rules the chain out; for a range of bank members the alternative to the ONE
    // launch with an operand table is not one column-split launch per step but one per MEMBER and step, so the range takes one workgroup
    // per ciphertext from the start, and so does a read list, which is a bank operation.  (The smaller regimes — limb split, fine split, the
    // mid chains — keep their precedence: chain_form.)
    bool row_fuse(int d, int n_tr, int gx) const { return use_row_fuse(c, d, n_tr, gx, Y(), bank); }
};
// the plain operation: one address (a = &addr), the context's d_prep / d_prep_inv, ws ciphertexts (the context's word count and RAM; one member of a bank: its)
Opnds one_addr(fheram_ctx* c, const fheram_addr* const* a, int ws, RamState* st) { return Opnds{c, st, a, 1, ws, c->d_prep, c->d_prep_inv, 0, 0, false}; }
Opnds one_addr(fheram_ctx* c, const fheram_addr* const* a) { return one_addr(c, a, c->ws, &c->ram); }
// n > 1 addresses of ws ciphertexts, their digits in a table ([n][n_digits] prepared GGSW; tab_inv: of a set that is written, else nullptr)
Opnds table_opnds(fheram_ctx* c, RamState* st, const fheram_addr* const* addrs, int n, int ws, double* tab, double* tab_inv, unsigned member_map, bool bank) {
    return Opnds{c, st, addrs, n, ws, tab, tab_inv, (long)c->n_digits * (long)fheram_ctx::GGSW, member_map, bank};
}

// An operation's VIEW: every buffer indexed by ciphertext y, from the operation's first.  The rows, the ping-pong arenas A / B with the third
// and fourth (pack_levels P0 / P1; the write's trace(ct_hi)), the per-ciphertext buffers, and where the result goes.  The context's own
// (ctx_view), those of a read of several addresses (dense_view below: a batch's, a read list's or a write list's), or a range of a bank's members (bank.hpp bank_view).
struct RamView {
    int32_t *rows, *A, *B, *C, *D;   // [Y][rows]
    int32_t *part, *tmp, *tmp2, *res, *tree, *w, *trtop;   // [Y]; part: the packed row where no arena holds it (rows == 1, a shard's partial) / the un-rotated ct_lo
};
RamView ctx_view(const fheram_ctx* c) {
    return RamView{c->d_data, c->d_scrA, c->d_scrB, c->d_scrC, c->d_scrD, c->d_part, c->d_tmp, c->d_tmp2, c->d_res, c->d_tree, c->d_w, c->d_trtop};
}

// What an operation leaves on the host, once it has been enqueued — or replayed (run_op), which does not run the enqueue functions.
// A read has one such function per stage, because the stages of a row-sharded RAM run on different contexts.
void read_local_done(const fheram_ctx* c, RamState* st, bool prepare_write) {   // memo_alone: arena A keeps the rows after their alone levels (two coordinates only)
    if (c->n2 == 2) st->memo_alone = (prepare_write && c->cfg.memo) ? LOGN - ilog2_ceil(c->rows_glob) : 0;
}
void read_top_done(fheram_ctx* c, RamState* st, bool prepare_write) {
    st->memo_top = prepare_write && c->cfg.memo;          // trtop = trace(tree top), kept for the write
    st->res_in_trtop = st->memo_top;
    c->prep1_ready = false;
}
// (inv_id / inv_pending are consumed where the write uses the inverse digits, write_side_begin and write_top; a replay finds them at 0, see run_op)
void write_done(fheram_ctx* c, RamState* st) { st->memo_top = false; st->memo_alone = 0; c->side_begun = false; c->tree_rotate_pending = false; }

// The launch sequence of an op is a function of (context, address, op) and of a few bits of the context's state (what a
// write may resume from): with FHERAM_GRAPH=1 it is captured once per address and state signature into a hipGraph and
// replayed, instead of being re-enqueued kernel by kernel.  (One address only; pre_inv is off under FHERAM_GRAPH=1, so inv_id stays 0.)
template <typename F>
int run_op(fheram_ctx* c, const fheram_addr* addr, int which, F&& enqueue) {
    if (!capturing(c)) return enqueue();
    main_enqueued(c);   // (a replay runs no enqueue function)
    fheram_addr* a = const_cast<fheram_addr*>(addr);
    // what the enqueue function reads of the context's mutable state (a write resumes from what read_prepare_write kept —
    // or not, after a key load or with another address): a capture taken under another signature is not replayed
    const unsigned sig = 1u | (c->ram.memo_top ? 2u : 0u) | ((unsigned)c->ram.memo_alone << 2) | (c->side_begun ? 64u : 0u) |
                         (c->inv_id[0] == addr->id ? 128u : 0u) | (c->inv_id[1] == addr->id ? 256u : 0u);
    if (a->graph[which] && a->graph_sig[which] != sig) { hipGraphExecDestroy(a->graph[which]); a->graph[which] = nullptr; }
    if (!a->graph[which]) {
        hipGraph_t g = nullptr;
        HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue();
        const hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc != FHERAM_OK || e != hipSuccess) {
            if (g) hipGraphDestroy(g);
            return rc != FHERAM_OK ? rc : fail(c, FHERAM_ERR_DEVICE, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        }
        const hipError_t e2 = hipGraphInstantiate(&a->graph[which], g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e2 != hipSuccess) { a->graph[which] = nullptr; return fail(c, FHERAM_ERR_DEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2)); }
        a->graph_sig[which] = sig;
    }
    HIPCHK(c, hipGraphLaunch(a->graph[which], c->stream));
    if (which == 2) write_done(c, &c->ram);
    else { read_local_done(c, &c->ram, which == 1); read_top_done(c, &c->ram, which == 1); }
    return FHERAM_OK;
}

int check_common(fheram_ctx* c, const fheram_addr* addr) {
    if (!c) return FHERAM_ERR_INVALID_ARG;
    mid_rearm(c);
    if (!addr || addr->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "address does not belong to this context (layout mismatch, ram.rs:404)");
    if (addr->empty) return fail(c, FHERAM_ERR_INVALID_ARG, "empty address: fheram_address_alloc without fheram_address_derive");
    if (!c->ram.initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    return FHERAM_OK;
}

// SubRam::read (ram.rs:382-459) / SubRam::read_prepare_write (ram.rs:461-542) for all sub-RAMs of every address of the operand
// set at once, in two stages so that a row-sharded RAM can exchange between them.
// Stage 1 (every shard): coordinate-0 products on the local rows + the packing levels that stay
// inside the shard.  The packed GLWE of every sub-RAM is left where the last launch wrote it (*packed_out,
// indexed by sub-RAM); to_part also copies it into a.part (d_part: the buffer a sharded RAM exchanges).
int read_local(const Opnds& o, const RamView& a, bool prepare_write, GlweRef* packed_out, bool to_part) {
    fheram_ctx* c = o.c;
    const int n = o.n, ws = o.ws, Y = o.Y(), R = (int)c->rows;
    main_enqueued(c);
    c->wide = !prepare_write || n > 1;   // read_prepare_write parks the gate wave beside its launches (read_top): its chain kernels keep a wave slot free; several addresses never park one
    if (n == 1 && prepare_write && c->cfg.pre_inv == 1 && !capturing(c) && (c->wide_unsynced || c->derive_unsynced)) {   // the gate wave may not be parked before this op's own launches start, nor its work read digits a derive launch is still writing (ctx.hpp: ev_opstart)
        hipEventRecord(c->ev_opstart, c->stream);
        c->opstart_valid = true;
    }
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    GlweRef data = ref(a.rows, sy, G), A = ref(a.A, sy, G), B = ref(a.B, sy, G);
    GlweRef part = ref(a.part, G, 0);
    const bool all = (c->n_shards == 1 && c->n2 == 2);   // unsharded: both coordinates now, one launch per address
    for (int k = 0; k < n; k++)                                                           // ram.rs:416-419 / 496-499
        if (all) coordinate_prepare_all(c, o.addrs[k], o.tab + k * o.stride); else coordinate_prepare(c, o.addrs[k], 0, o.tab + k * o.stride);
    c->prep1_ready = all;
    read_local_done(c, o.st, prepare_write);
    const int d0 = (int)c->base2d[0].size();
    if (c->n2 == 1) {
        GlweRef row0 = ref(a.rows, sy, 0);
        for (int k = 0; k < n; k++)
            if (prepare_write) ep_chain(c, o.rows(row0, k), o.rows(row0, k), o.slice(ref(a.A, sy, 0), k), o.prep(k, 0), d0, 1, ws);   // ram.rs:502-504 (rows == 1)
            else ep_chain(c, o.rows(row0, k), o.slice(part, k), o.slice(ref(a.tmp, G, 0), k), o.prep(k, 0), d0, 1, ws);                 // ram.rs:451
        // a list's members are not the view's first rows: the trace (read_top) takes them from a gathered copy in part
        const bool gather = prepare_write && !o.rows_dense();
        if (gather) for (int k = 0; k < n; k++) launch_copy(c, o.rows(row0, k), o.slice(part, k), 1, ws);
        *packed_out = (prepare_write && !gather) ? row0 : part;
        if (prepare_write && to_part && !gather) launch_copy(c, row0, part, 1, Y);
        return FHERAM_OK;
    }
    const int L0 = LOGN - ilog2_ceil(c->rows_glob);
    const bool keep = o.st->memo_alone > 0;   // leaves = the rows then: arena A keeps the rows after their alone levels
    int32_t* packed;
    if (o.row_fuse(d0, L0, R) && !(prepare_write && (d0 & 1))) {
        // the products and the alone packer levels as ONE launch (k_read_chain; with a table: row y takes the digits of address y / ws):
        // rows after the alone levels in arena A (read_prepare_write: the products' result also lands in the rows, ram.rs:502-504)
        launch_read_chain(c, data, prepare_write ? &data : nullptr, A, o.prep(0, 0), d0, L0, R, Y, o.table());   // ram.rs:429-435 / 502-514
        packed = pack_levels(c, a.A, a.A, a.B, sy, G, (size_t)R, Y, 0, L0, keep, a.C, a.D);   // ram.rs:435-448 / 510-521: the pairing levels
    } else {
        for (int k = 0; k < n; k++)
            if (prepare_write) ep_chain(c, o.rows(data, k), o.rows(data, k), o.slice(A, k), o.prep(k, 0), d0, R, ws);   // ram.rs:502-504
            else ep_chain(c, o.rows(data, k), o.slice(A, k), o.slice(B, k), o.prep(k, 0), d0, R, ws);                   // ram.rs:429-434
        int32_t* leaves = prepare_write ? a.rows : a.A;
        if (prepare_write && !o.rows_dense()) {   // a list where the fused chain does not run (forced off, or the default form up to 64 ciphertext rows, 2^14): the members' rows gathered into the fourth arena, which the alone levels only read
            for (int k = 0; k < n; k++) launch_copy(c, o.rows(data, k), o.slice(ref(a.D, sy, G), k), R, ws);
            leaves = a.D;
        }
        packed = pack_levels(c, leaves, a.A, a.B, sy, G, (size_t)R, Y, L0, L0, keep, a.C, a.D);   // ram.rs:435-448 / 510-521
    }
    *packed_out = ref(packed, sy, 0);
    if (to_part) launch_copy(c, *packed_out, part, 1, Y);
    return FHERAM_OK;
}
// Stage 2 (root / unsharded): remaining packing levels over the shards' partials (`gathered`:
// [n_shards][ws] GLWEs, or nullptr when the RAM is not sharded and the packed rows are at `pk`),
// coordinate-1 products and the final trace.  Result left in a.res (d_trtop: below).  Every step is out of place, so
// nothing has to be copied between them.
int read_top(const Opnds& o, const RamView& a, bool prepare_write, int32_t* gathered, GlweRef pk) {
    fheram_ctx* c = o.c;
    const int n = o.n, ws = o.ws, Y = o.Y();
    main_enqueued(c);
    c->wide = !prepare_write || n > 1;
    const long G = (long)fheram_ctx::GLWE;
    GlweRef tmp = ref(a.tmp, G, 0);
    GlweRef last = pk;
    // coordinate 1's products inside the trace chain's launch (k_trace_tail's product steps): from two digits on (the fallback is the fused row chain)
    const int d1 = c->n2 == 2 ? (int)c->base2d[1].size() : 0;
    auto tail_top = [&] { return chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail; };   // the final trace: will it ask for the tail launch (as things stand now)
    const bool fuse_ep = c->n2 == 2 && c->cfg.tail_ep && d1 >= 2 && d1 <= TAIL_EP_MAX && tail_top();
    GlweRef ep_out = ref(prepare_write ? a.tree : a.tmp2, G, 0);                          // read_prepare_write: tree[0] <- rotated packed row, ram.rs:525-527
    auto products1 = [&] { for (int k = 0; k < n; k++) ep_chain(c, o.slice(pk, k), o.slice(ep_out, k), o.slice(tmp, k), o.prep(k, 1), d1, 1, ws); };   // ram.rs:454 (not into res: the trace below runs out of place) / 525-527 + 502-504 (i = 1)
    if (c->n2 == 2) {
        if (gathered) {
            const int kG = ilog2_ceil((size_t)c->n_shards);
            int32_t* a0 = c->d_gat[1];   // gathered partials live in d_gat[0]
            int32_t* a1 = c->d_gat[2];
            int32_t* packed = pack_levels(c, gathered, a0, a1, G, (long)ws * G, (size_t)c->n_shards, ws, 0, LOGN - kG);
            pk = ref(packed, G, 0);
        }
        if (!c->prep1_ready) coordinate_prepare(c, o.addrs[0], 1, o.tab);                 // (a sharded RAM: one address)
        if (!fuse_ep) products1();                                                        // (else enqueued below, with the trace chain)
        last = ep_out;                                                                    // ram.rs:535 (res <- tree[0])
    }                                                                                     // n2 == 1: res <- packed row (ram.rs:452 / 537)
    // read_prepare_write: the result is also what write_first_step computes first (trace of the same ciphertext,
    // ram.rs:571-572): it lands in d_trtop, which no read overwrites, and stays there for the write
    // the write's inverse digits, next to the trace chain below (one launch on half of the XCDs; the side stream has the
    // lowest priority, so that launch is placed first)
    // (only while the write's chains are one workgroup round on the chip: with several rounds — 2^21 on one GPU — the
    // earlier start of the write's main chain interleaves it with the side chain less favourably, write 8.57 -> 8.74 ms)
    const bool pre = n == 1 && prepare_write && c->cfg.pre_inv && (long)c->rows * Y <= c->cus;
    const bool gated = pre && c->cfg.pre_inv == 1 && !capturing(c) && tail_top();   // FHERAM_PRE_INV=2: event fork (A/B switch)
    if (pre && !gated)
        for (int ci = c->n2 - 1; ci >= 0; ci--) precompute_inverse(c, o.addrs[0], ci, ci == c->n2 - 1);   // coordinate 1 first: the write's head needs it first
    read_top_done(c, o.st, prepare_write);
    const GlweRef res = ref(o.st->memo_top ? a.trtop : a.res, G, 0);
    const uint64_t tl0 = c->tail_launches;
    GlweRef tb[2];
    if (fuse_ep && chain_bufs(LOGN, last, res, tmp, tb))                               // ram.rs:454 / 525-527 + 457 / 540 as ONE launch
        launch_trace_tail(c, pk, tb, 0, LOGN, 1, Y, o.prep(0, 1), d1, ep_out, prepare_write, o.table());
    else {
        if (fuse_ep) products1();                                                      // (cannot happen with these buffers; kept for safety)
        trace_steps(c, last, res, tmp, 0, LOGN, 1, Y);                                 // ram.rs:457 / 540
    }
    if (gated && !c->opstart_valid && (c->wide_unsynced || c->derive_unsynced)) {   // (a root's read_finish: no read_local of this op ran on this context)
        hipEventRecord(c->ev_opstart, c->stream);
        c->opstart_valid = true;
    }
    if (gated) {   // behind a gate that opens when the trace chain's launch is placed (no event on the main stream); host order is irrelevant
        const unsigned seq = c->tail_launches != tl0 ? c->tail_seq : 0;                // 0: no such launch after all -> event fork
        for (int ci = c->n2 - 1; ci >= 0; ci--) precompute_inverse(c, o.addrs[0], ci, ci == c->n2 - 1, seq);
    }
    // the tail launch and its fallback are the last launches of this function on the main stream (behind them: at most an event record):
    // a caller that enqueues nothing more arms the host's short cut on that generation (tail_wait.hpp)
    c->tail_wait.note_top(c->tail_launches != tl0 ? c->tail_seq : 0);
    return FHERAM_OK;
}
int read_impl(const Opnds& o, const RamView& a, bool prepare_write) {
    fheram_ctx* c = o.c;
    GlweRef packed;
    int rc = read_local(o, a, prepare_write, &packed, false);
    if (rc != FHERAM_OK) return rc;
    rc = read_top(o, a, prepare_write, nullptr, packed);
    if (o.n == 1 && prepare_write && c->inv_id[0] == o.addrs[0]->id && capturing(c))   // a capture ends with every fork joined
        for (int ci = 0; ci < c->n2; ci++) hipStreamWaitEvent(c->stream, c->ev_inv[ci], 0);
    if (rc == FHERAM_OK && prepare_write) o.st->state = true;                         // ram.rs:533
    return rc;
}

// ---- what every buffer set below shares: the dense sets' and those of the bank's one-row operations (select.hpp, regs.hpp, table.hpp, public_io.hpp, mix.hpp) ----
// HOST BYTES ON THEIR WAY TO THE DEVICE: a device buffer, its pinned twin, the event of the last copy out of the twin and whether one
// is in flight.  The owner allocates the three in the order of its own set (device buffers first, then pinned, then events) and frees
// them with bufs_free; a call waits for the last copy (stage_wait), fills the twin, copies on the main stream and records (stage_record).
struct HostStage {
    unsigned char *d = nullptr, *h = nullptr;
    hipEvent_t ev = nullptr;
    bool busy = false;
    template <typename T> T* dev() const { return reinterpret_cast<T*>(d); }
    template <typename T> T* host() const { return reinterpret_cast<T*>(h); }
    hipError_t pin(size_t bytes) { return hipHostMalloc((void**)&h, bytes, hipHostMallocDefault); }
    hipError_t event() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
};
int stage_wait(fheram_ctx* c, HostStage& s) {   // the last call's copy out of the pinned twin; no other host wait
    if (s.busy) { HIPCHK(c, hipEventSynchronize(s.ev)); s.busy = false; }
    return FHERAM_OK;
}
int stage_record(fheram_ctx* c, HostStage& s) {
    HIPCHK(c, hipEventRecord(s.ev, c->stream));
    s.busy = true;
    return FHERAM_OK;
}
// a set's buffers: the device ones, then the pinned ones, then the events
void bufs_free(std::initializer_list<void*> device, std::initializer_list<void*> pinned, std::initializer_list<hipEvent_t> events) {
    for (void* p : device) if (p) hipFree(p);
    for (void* p : pinned) if (p) hipHostFree(p);
    for (hipEvent_t e : events) if (e) hipEventDestroy(e);
}
// the pinned, device-visible buffer a set's results are exported through: ct bytes of int32 as int64, + the monitor's maximum
hipError_t pinned_result(int64_t** h, int64_t** d_h, size_t ct) {
    const hipError_t e = hipHostMalloc((void**)h, ct * 2 + sizeof(int64_t), hipHostMallocMapped);
    return e == hipSuccess ? hipHostGetDevicePointer((void**)d_h, *h, 0) : e;
}
// a reserve that failed, its new set freed: the next op's error check must not see this allocation's failure
int reserve_failed(fheram_ctx* c, hipError_t e, const std::string& what) {
    (void)hipGetLastError();
    return fail(c, FHERAM_ERR_DEVICE, what + ": " + hipGetErrorString(e));
}

// ---- several Ram::read (ram.rs:172-191) as one launch sequence: fheram_read_batch, fheram_bank_read_list ------------------------------
// A read does not change the RAM (SubRam::read asserts !state and only writes its scratch, ram.rs:393-396): n reads at n addresses share the
// keys and every packing and trace step; only the products with the address digits differ (and, in a bank, whose rows they read).  Such an
// operation runs on a dense buffer set of its own (ctx.hpp DenseBufs), [n * ws][rows] GLWEs with the rows' stride, so that ciphertext y = k * ws + w is
// word w of address k and every address-independent step is ONE launch over gy = n * ws.  A bank's read_prepare_write / write lists run on
// such a set too (bank.hpp), with every buffer of a view in it.
void dense_free(DenseBufs& L) {
    bufs_free({L.A, L.B, L.C, L.D, L.part, L.tmp, L.tmp2, L.res, L.tree, L.w, L.trtop, L.prep}, {L.h_res}, {});
    L = DenseBufs{};
}
// The third arena is only needed where the alone packer levels run as the single-launch tail chain on the operation's rows (at most
// TAIL_GROUPS ciphertexts: 2^13 with n * ws <= 4), whose source must survive the launch (pack_levels P0): allocated only then.
// (The very question pack_levels asks; the fused row chain, which would leave it no alone levels, excludes the Tail form: launch.hpp chain_form.)
// n_ct: the operation's ciphertexts (a batch: K * ws; a bank's read list, whose context has the word count of the whole bank: n * its members' ws)
bool third_arena_needed(const fheram_ctx* c, int n_ct) {
    return c->n2 == 2 && chain_form(c, ChainQuery{false, LOGN - ilog2_ceil(c->rows_glob), (int)c->rows, n_ct}).form == ChainForm::Tail;
}
// Grows the set to n addresses of ws ciphertexts with what the caller's operation needs; on failure the owner holds none of it (and every
// other operation is unaffected).  Regrowing never drops what existed, and keeps the capacity when only buffers are added.
//   reads (a batch, a read list): the result and its pinned copy always.  One address is the plain read on the RAM's own buffers, so the
//     arenas, the temporaries and the digit table wait for the first operation of several addresses, and the third arena for the first that needs it.
//   all (a bank's write lists): the four arenas and the seven per-ciphertext buffers, in the view's order; the side stream may still be
//     working on them; fail_alloc (the self-test's): the *fail_alloc-th of these allocations reports an exhausted device.
int dense_reserve(fheram_ctx* c, DenseBufs& L, int n, int ws, bool all = false, int* fail_alloc = nullptr) {
    const bool work = all || n > 1, third = all || (work && third_arena_needed(c, n * ws));
    if (n <= L.cap && (!work || L.A) && (!third || L.C)) return FHERAM_OK;
    if (n < L.cap) n = L.cap;   // (only the working buffers or the third arena are missing: keep the capacity)
    const bool with_work = work || L.A, with_third = third || L.C;
    if (L.cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (all) HIPCHK(c, hipStreamSynchronize(c->stream2));
        dense_free(L);
    }
    const size_t ct = (size_t)n * ws * fheram_ctx::GLWE * sizeof(int32_t), row = ct * c->rows;
    hipError_t e = hipSuccess;
    auto dev = [&](auto** p, size_t bytes) {
        if (e != hipSuccess) return;
        if (fail_alloc && *fail_alloc > 0 && --*fail_alloc == 0) e = hipErrorOutOfMemory;   // (as the runtime reports an exhausted device)
        else e = hipMalloc((void**)p, bytes);
    };
    if (all) {
        for (int32_t** p : {&L.A, &L.B, &L.C, &L.D}) dev(p, row);
        for (int32_t** p : {&L.part, &L.tmp, &L.tmp2, &L.res, &L.tree, &L.w, &L.trtop}) dev(p, ct);
    } else {
        dev(&L.res, ct);
        if (with_work) {
            for (int32_t** p : {&L.A, &L.B}) dev(p, row);
            if (with_third) dev(&L.C, row);
            for (int32_t** p : {&L.tmp, &L.tmp2}) dev(p, ct);
            dev(&L.prep, (size_t)n * c->n_digits * fheram_ctx::GGSW * sizeof(double));
        }
        if (e == hipSuccess) e = pinned_result(&L.h_res, &L.d_h_res, ct);
    }
    if (e != hipSuccess) {
        dense_free(L);
        return reserve_failed(c, e, all ? "buffers of a write list of " + std::to_string(n) + " members" : "read buffers for " + std::to_string(n) + " addresses");
    }
    L.cap = n;
    return FHERAM_OK;
}
// The view of an operation on such a set: the context's rows (a bank's: the whole bank's, reached through the operand set's map), and
// every launch writes the set's buffers only.  The result of address k is at res + k * ws GLWEs.  A set of reads has no part of its own
// (rows == 1: the products land in tmp2) and no D, tree, w or trtop: a read names none of them.
RamView dense_view(const fheram_ctx* c, const DenseBufs& L) {
    return RamView{c->d_data, L.A, L.B, L.C, L.D, L.part ? L.part : L.tmp2, L.tmp, L.tmp2, L.res, L.tree, L.w, L.trtop};
}

// fheram_bank_select's own buffers (select.hpp): per output ciphertext the packed row, the products' output, two temporaries and the result;
// the selectors' prepared digits; the staged host candidates.  Allocated on first use, grown to the largest call seen, freed with the bank.
struct SelectBufs {
    int cap = 0, prep_cap = 0, host_cap = 0;   // ciphertexts; prepared GGSW digits; ciphertexts of host candidates
    int32_t *packed = nullptr, *ep = nullptr, *tmp = nullptr, *tmp2 = nullptr, *res = nullptr;   // [cap] GLWE
    double* prep = nullptr;                                                                      // [prep_cap] prepared GGSW: select k's digits at k * n_digits
    int64_t *h_res = nullptr, *d_h_res = nullptr;                                                // pinned, device-visible: the results as int64 (+ the monitor's maximum)
    HostStage host;                                                                              // [host_cap] GLWE: host candidates
};
void select_free(SelectBufs& S) {
    bufs_free({S.packed, S.ep, S.tmp, S.tmp2, S.res, S.prep, S.host.d}, {S.h_res, S.host.h}, {S.host.ev});
    S = SelectBufs{};
}
// fheram_bank_select_lanes' pointer table (select_lanes.hpp): [64 output ciphertexts][32 candidates] pointers, 16 KiB — what
// k_select_pack_lanes reads, and the pinned twin the host writes, copied by one hipMemcpyAsync per call.
// Allocated whole on the first lanes call and freed with the bank; NOT among the buffers select_reserve counts and grows.
using SelectLaneTable = HostStage;
void lane_table_free(SelectLaneTable& L) {
    bufs_free({L.d}, {L.h}, {L.ev});
    L = SelectLaneTable{};
}

// What a bank's register files share (regs.hpp), and what its tables share (table.hpp): the buffers of n reads of one-row RAMs as one
// operation — per output ciphertext the fanned-out or gathered row, the products' output, a temporary and the result; the prepared
// digits of its selectors — the pinned result buffer, and one host stage: the host words of a register file's pack or write, the bytes
// of a table's load_plain.  Allocated whole by the bank's first fheram_bank_regs_create / fheram_bank_table_create, freed with the bank.
struct OneRowSet {
    int cap = 0;                                                                  // ciphertexts of a read: min(FHERAM_SELECT_MAX * word_size, 64); 0: not allocated
    int32_t *fan = nullptr, *ep = nullptr, *tmp = nullptr, *res = nullptr;        // [cap] GLWE
    double* prep = nullptr;                                                       // [FHERAM_SELECT_MAX * the kind's digit limit] prepared GGSW: read k's digits at k * n_digits
    int64_t *h_res = nullptr, *d_h_res = nullptr;                                 // pinned, device-visible: the results as int64 (+ the monitor's maximum)
    HostStage stage;                                                              // register files: [2^FHERAM_SELECT_BITS_MAX * word_size] GLWE; tables: [2^FHERAM_TABLE_BITS_MAX * word_size] bytes
};
void one_row_free(OneRowSet& S) {
    bufs_free({S.fan, S.ep, S.tmp, S.res, S.prep, S.stage.d}, {S.h_res, S.stage.h}, {S.stage.ev});
    S = OneRowSet{};
}
// prep_digits: the digits one selector of the kind may have; stage_bytes: its host stage; what: the set, for the failure's message
int one_row_reserve(fheram_ctx* c, OneRowSet& S, int ws, int prep_digits, size_t stage_bytes, const char* what) {
    if (S.cap) return FHERAM_OK;
    OneRowSet nw;
    nw.cap = std::min(FHERAM_SELECT_MAX * ws, 64);
    const size_t ct = (size_t)nw.cap * fheram_ctx::GLWE * sizeof(int32_t);
    hipError_t e = hipSuccess;
    for (int32_t** p : {&nw.fan, &nw.ep, &nw.tmp, &nw.res}) if (e == hipSuccess) e = hipMalloc((void**)p, ct);
    if (e == hipSuccess) e = hipMalloc((void**)&nw.prep, (size_t)FHERAM_SELECT_MAX * prep_digits * fheram_ctx::GGSW * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&nw.stage.d, stage_bytes);
    if (e == hipSuccess) e = pinned_result(&nw.h_res, &nw.d_h_res, ct);
    if (e == hipSuccess) e = nw.stage.pin(stage_bytes);
    if (e == hipSuccess) e = nw.stage.event();
    if (e != hipSuccess) { one_row_free(nw); return reserve_failed(c, e, what); }
    S = nw;
    return FHERAM_OK;
}

// A bank's public side (public_io.hpp): the buffers of fheram_bank_peek / _poke — per ciphertext the gathered, rotated row, a temporary
// and TWO result buffers (an operation writes the one that does not hold the last outputs: res[cur] does) — the pinned result buffer, the
// host words of a poke, and the staged bytes of a fheram_bank_ram_load_plain / _regs_load_plain.  Allocated whole by the bank's first
// such call, freed with the bank.
struct PublicBufs {
    int cap = 0;                                                                  // ciphertexts of a call: min(FHERAM_PEEK_MAX * word_size, 64); 0: not allocated
    int32_t *fan = nullptr, *tmp = nullptr, *res[2] = {nullptr, nullptr};         // [cap] GLWE
    int cur = 0;
    int64_t *h_res = nullptr, *d_h_res = nullptr;                                 // pinned, device-visible: the results as int64 (+ the monitor's maximum)
    HostStage host;                                                               // [FHERAM_PEEK_MAX * word_size] GLWE: host words
    HostStage data;                                                               // [rows * N * word_size] bytes of a load_plain
};
void public_bufs_free(PublicBufs& P) {
    bufs_free({P.fan, P.tmp, P.res[0], P.res[1], P.host.d, P.data.d}, {P.h_res, P.host.h, P.data.h}, {P.host.ev, P.data.ev});
    P = PublicBufs{};
}

// fheram_bank_read_mix's own buffers (mix.hpp): per ciphertext of the shared top the products' output, a temporary and THREE result
// buffers — a mix writes the one that holds no empty group's last outputs — and the pinned result buffer.  The digits of its one-row
// groups are prepared into the tables' and the register files' own (OneRowSet::prep: a group that is not empty has its
// object, so they exist).  Allocated whole by the bank's first fheram_bank_read_mix, freed with the bank.
// fheram_bank_read_prepare_write_mix adds three, allocated whole by the bank's first such call: a fourth result buffer for a call without
// reads (all three others may hold an empty kind's last outputs then), the digits of a prepare list of ONE member (the context's own
// slots may hold those of a read list of one entry until the top has run) and the packed row of such a read list where the prepare
// list works on the same member's arenas.
struct MixBufs {
    int cap = 0;                                                                  // ciphertexts: min(FHERAM_MIX_MAX * word_size, 64); 0: not allocated
    int32_t *ep = nullptr, *tmp = nullptr, *res[3] = {nullptr, nullptr, nullptr}; // [cap] GLWE
    int64_t *h_res = nullptr, *d_h_res = nullptr;                                 // pinned, device-visible: the results as int64 (+ the monitor's maximum)
    int32_t *own = nullptr, *keep = nullptr;                                      // [cap] / [word_size] GLWE (read_prepare_write_mix; nullptr: not allocated)
    double* prep = nullptr;                                                       // [n_digits] prepared GGSW (read_prepare_write_mix)
};
void mix_bufs_free(MixBufs& M) {
    bufs_free({M.ep, M.tmp, M.res[0], M.res[1], M.res[2], M.own, M.keep, M.prep}, {M.h_res}, {});
    M = MixBufs{};
}
// Where the last operation of a kind left its outputs (bank.hpp LastOutputs): the operation's own buffer set, or the mix's when a
// fheram_bank_read_mix ran that kind last.  mix_slot: which of the mix's result buffers (-1: none of them).
struct ResHome {
    const int32_t* res = nullptr;                    // output 0 of the kind
    int64_t *h = nullptr, *d_h = nullptr;            // the pinned buffer a download of it goes through
    int mix_slot = -1;
};

// The one result export: every run (source, int32 count) is widened by the device into the pinned buffer h (device address d_h), back to
// back, with the monitor's maximum as it stood then behind the last (the export kernel copies it there); out != nullptr: copied out.
struct ResRun { const int32_t* src; size_t n; };
int result_export(fheram_ctx* c, const ResRun* runs, int n_runs, int64_t* h, int64_t* d_h, int64_t* out) {
    size_t n = 0;
    for (int i = 0; i < n_runs; i++) {
        const int n4 = (int)(runs[i].n / 4);
        hipLaunchKernelGGL(k_export_i64, dim3((n4 + 255) / 256), dim3(256), 0, c->stream, runs[i].src, reinterpret_cast<long long*>(d_h + n), n4,
                           reinterpret_cast<const long long*>(c->d_tw + N));
        n += runs[i].n;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    main_waited(c);
    double m;
    std::memcpy(&m, h + n, 8);
    if (c->cfg.monitor && m > MON_LIMIT) __atomic_store_n(c->h_ro_flag, 1u, __ATOMIC_RELAXED);
    const int rc = check_precision(c);
    if (rc == FHERAM_OK && out) std::memcpy(out, h, n * sizeof(int64_t));
    return rc;
}

// the results of ciphertexts [first, first + n_ct) of such an operation, widened into its pinned buffer; out: [n_ct][GLWE] int64
int reads_export(fheram_ctx* c, const DenseBufs& L, size_t first, size_t n_ct, int64_t* out) {
    const ResRun run{L.res + first * fheram_ctx::GLWE, n_ct * fheram_ctx::GLWE};
    return result_export(c, &run, 1, L.h_res, L.d_h_res, out);
}
// n >= 2 reads as one operation on `L`: address k reads member (member_map >> 4k) & 15 of the context's rows.  kept(o): what the caller's
// RAM(s) keep of it (where a single read would have left its result), enqueued behind the reads.
// (Never captured: the launch sequence depends on n addresses, and a read's state bookkeeping is done as it is enqueued.)
template <typename F>
int read_many(fheram_ctx* c, DenseBufs& L, RamState* st, const fheram_addr* const* addrs, int n, int ws, unsigned member_map, bool bank, int64_t* out, F&& kept) {
    int rc = dense_reserve(c, L, n, ws);
    if (rc != FHERAM_OK) return rc;
    const Opnds o = table_opnds(c, st, addrs, n, ws, L.prep, nullptr, member_map, bank);
    rc = read_impl(o, dense_view(c, L), false);
    if (rc != FHERAM_OK) return rc;
    kept(o);
    HIPCHK(c, hipGetLastError());
    return out ? reads_export(c, L, 0, (size_t)n * ws, out) : FHERAM_OK;
}

// Ram::write (ram.rs:226-294) of every address of the operand set, in two stages and a side stage.
// Stage 1 (root / unsharded): write_first_step on the top of the tree and, for n2 == 2, the inverse
// coordinate-1 products: leaves the un-rotated ct_lo of every sub-RAM in d_part.
int write_top(const Opnds& o, const RamView& v) {
    fheram_ctx* c = o.c;
    main_enqueued(c);
    c->wide = true;             // (everything a write enqueues runs behind read_prepare_write's trace chain, whose placement releases the gate wave)
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    const int n = o.n, ws = o.ws, Y = o.Y();
    GlweRef wref = ref(v.w, G, 0), tmp = ref(v.tmp, G, 0), tmp2 = ref(v.tmp2, G, 0), tree = ref(v.tree, G, 0);
    // write_first_step (ram.rs:544-577): t <- normalize(t - trace(t) + w)
    GlweRef top = (c->n2 != 1) ? tree : ref(v.rows, sy, 0);
    GlweRef tr = tmp;
    const bool by_member = c->n2 == 1 && !o.rows_dense();   // a list on one-row RAMs: the top is the member's row, one launch per address
    if (o.st->memo_top) tr = ref(v.trtop, G, 0);     // = trace(top), computed by read_prepare_write on this very ciphertext
    else if (by_member) for (int k = 0; k < n; k++) trace_steps(c, o.rows(top, k), o.slice(tmp, k), o.slice(tmp2, k), 0, LOGN, 1, ws);
    else trace_steps(c, top, tmp, tmp2, 0, LOGN, 1, Y);
    if (by_member) {
        ProfScope ps(c, "elementwise", Y);
        for (int k = 0; k < n; k++)
            hipLaunchKernelGGL((k_sub_add_norm<3>), dim3(1, ws, EW_SLICES), dim3(256), 0, c->cur, o.rows(top, k), o.slice(tr, k), o.slice(wref, k), o.rows(top, k));
    } else {
        ProfScope ps(c, "elementwise", Y);
        hipLaunchKernelGGL((k_sub_add_norm<3>), dim3(1, Y, EW_SLICES), dim3(256), 0, c->cur, top, tr, wref, top);
    }
    o.st->memo_top = false;
    if (c->n2 == 2) {
        // the head: per address, the inverse of coordinate 1 (ram.rs:260-271) and its products on the address's tree top (ram.rs:610)
        if (n == 1 && c->inv_id[1] == o.addrs[0]->id) wait_inverse(c, c->stream, 1);    // started by read_prepare_write
        else {
            // another address (or new keys): a precompute that read_prepare_write started for ITS address may still be
            // writing d_prep_inv on the side stream — the main stream must not overtake it
            if (n == 1 && c->inv_pending[1]) wait_inverse(c, c->stream, 1);
            for (int k = 0; k < n; k++) coordinate_prepare_inv(c, o.addrs[k], 1, c->d_ggsw_tmp, o.inv(k, 1));   // ram.rs:260-271
        }
        if (n == 1) { c->inv_pending[1] = false; c->inv_id[1] = 0; }
        for (int k = 0; k < n; k++)                                                        // ram.rs:610: the un-rotated ct_lo, in d_part
            ep_chain(c, o.slice(tree, k), o.slice(ref(v.part, G, 0), k), o.slice(tmp, k), o.inv(k, 1), (int)c->base2d[1].size(), 1, ws);
        // tree[0] <- ct_lo * X^-rows (ram.rs:629, `rows` rotations by X^-1): nothing in this write reads it again, so
        // the rotation is enqueued behind the rows' work (write_rows) instead of in front of it
        c->tree_rotate_pending = true;
    }
    return FHERAM_OK;
}
// Work of a write that does not depend on stage 1: tmp_a = trace(ct_hi) for every local row
// (ram.rs:616) and the inverse of coordinate 0 (ram.rs:278-289).  It is enqueued on the side stream
// so that it fills the CUs the latency-bound stage 1 (a chain of word_size-ciphertext launches)
// leaves idle.
void write_side_begin(const Opnds& o, const RamView& v) {
    fheram_ctx* c = o.c;
    c->wide = true;
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    // behind everything before this write (rows after rpw) — unless the host has waited for the main stream since its last enqueue
    // (ctx.hpp main_idle): then there is nothing to fork from, and what the side stream still holds (the early inverse digits behind
    // ev_wdone, their ev_inv) it orders itself.  A capture needs the fork to pull the side stream in; a shard of a row-sharded RAM keeps it
    // (its main stream also carries the exchange with the other contexts, which this context's host waits do not cover).
    if (!(c->main_idle && !capturing(c) && c->n_shards == 1)) {
        hipEventRecord(c->ev_fork, c->stream);
        hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
    }
    main_enqueued(c);   // (the write this belongs to enqueues on the main stream next; a second side stage forks again)
    c->cur = c->stream2;
    if (c->n2 == 2) {                                 // every row of every address: ONE chain
        const int kept = o.st->memo_alone;   // > 0: arena A = the rows after trace steps 0 .. kept-1 (left there by read_prepare_write)
        c->trhi_in_C = kept > 0 && (LOGN - kept) % 2 == 1;   // ping-pong A <-> C; an odd number of remaining steps ends in C
        if (kept > 0) trace_steps(c, ref(v.A, sy, G), ref(c->trhi_in_C ? v.C : v.A, sy, G), ref(c->trhi_in_C ? v.A : v.C, sy, G), kept, LOGN, (int)c->rows, o.Y());
        else if (!o.rows_dense())   // a list with nothing kept: one chain per address, from the member's rows
            for (int k = 0; k < o.n; k++) trace_steps(c, o.rows(ref(v.rows, sy, G), k), o.slice(ref(v.A, sy, G), k), o.slice(ref(v.C, sy, G), k), 0, LOGN, (int)c->rows, o.ws);
        else trace_steps(c, ref(v.rows, sy, G), ref(v.A, sy, G), ref(v.C, sy, G), 0, LOGN, (int)c->rows, o.Y());
        o.st->memo_alone = 0;
    }
    if (o.n == 1 && c->inv_id[0] == o.addrs[0]->id) wait_inverse(c, c->stream2, 0);   // started by read_prepare_write (on this very stream)
    else for (int k = 0; k < o.n; k++) coordinate_prepare_inv(c, o.addrs[k], 0, c->d_ggsw_tmp2, o.inv(k, 0));   // (a precompute for another address sits on this very stream: ordered)
    if (o.n == 1) { c->inv_id[0] = 0; c->inv_pending[0] = false; }
    hipEventRecord(c->ev_join, c->stream2);
    c->cur = c->stream;
    c->side_begun = true;
}
// Error path of a write whose side-stream work was already enqueued: rejoin the side stream, so that no
// later operation on the main stream can overtake it.
void write_side_abort(fheram_ctx* c) {
    if (!c->side_begun) return;
    hipStreamWaitEvent(c->stream, c->ev_join, 0);
    c->side_begun = false;
}
// Stage 2 (every shard): write_mid_step on the local rows given ct_lo (in d_part), then write_last_step.
int write_rows(const Opnds& o, const RamView& v) {
    fheram_ctx* c = o.c;
    main_enqueued(c);
    c->wide = true;
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    const int n = o.n, ws = o.ws, Y = o.Y(), R = (int)c->rows;
    GlweRef data = ref(v.rows, sy, G), A = ref(v.A, sy, G), B = ref(v.B, sy, G), D = ref(v.D, sy, G);
    GlweRef trhi = ref(c->trhi_in_C ? v.C : v.A, sy, G), part = ref(v.part, G, 0);
    const int d0 = (int)c->base2d[0].size();
    const bool fuse = c->n2 == 2 && o.row_fuse(d0, LOGN, R);
    // unsharded, the fused chain's workgroups of row 0 write the tree's rotated copy of ct_lo themselves (they read ct_lo anyway): a launch less
    // behind the chain, for which the host waits.  A root's rows are every n_shards-th: it keeps the launch.
    const bool rot_in_chain = fuse && c->tree_rotate_pending && c->n_shards == 1;
    const GlweRef tree = ref(v.tree, G, 0);
    if (fuse) {
        // trace(ct_lo * X^-row), normalize(ct_hi - trace(ct_hi) + that) and write_last_step's products as ONE launch (k_write_chain; with a table:
        // row y takes the inverse digits of address y / ws); it needs trace(ct_hi) and the inverse digits of coordinate 0 from the side stream at
        // its start (that stream's chain holds every CU until then anyway)
        hipStreamWaitEvent(c->stream, c->ev_join, 0);
        launch_write_chain(c, part, c->n_shards, c->shard, data, trhi, o.inv(0, 0), d0, LOGN, R, Y, o.table(), rot_in_chain ? &tree : nullptr, -(int)c->rows_glob);   // ram.rs:612-646
    } else if (c->n2 == 2)
        trace_steps(c, part, B, D, 0, LOGN, R, Y, c->n_shards, c->shard);                      // tmp_a = trace(ct_lo * X^-row)   ram.rs:621,629
    if (c->tree_rotate_pending && !rot_in_chain) {   // root / unsharded: the tree's copy of ct_lo, rotated (see write_top)
        ProfScope ps(c, "elementwise", Y);
        hipLaunchKernelGGL((k_rotate<3>), dim3(1, Y, EW_SLICES), dim3(256), 0, c->cur, part, ref(v.tree, G, 0), -(int)c->rows_glob);
    }
    if (!fuse) {
        hipStreamWaitEvent(c->stream, c->ev_join, 0);                                          // side stream: trace(ct_hi), inverse coordinate 0
        if (c->n2 == 2) {
            ProfScope ps(c, "elementwise", (uint64_t)R * Y);
            if (o.rows_dense()) hipLaunchKernelGGL((k_sub_add_norm<3>), dim3(R, Y, EW_SLICES), dim3(256), 0, c->cur, data, trhi, B, data);   // ram.rs:617,625-626
            else for (int k = 0; k < n; k++)   // a list: the rows of member(k), everything else of address k
                hipLaunchKernelGGL((k_sub_add_norm<3>), dim3(R, ws, EW_SLICES), dim3(256), 0, c->cur, o.rows(data, k), o.slice(trhi, k), o.slice(B, k), o.rows(data, k));
        }
        for (int k = 0; k < n; k++) ep_chain(c, o.rows(data, k), o.rows(data, k), o.slice(A, k), o.inv(k, 0), d0, R, ws);   // ram.rs:644-646
    }
    // the next read_prepare_write's side work overwrites d_prep_inv: it is ordered behind this write by an event (the gate
    // launch in front of that work is time-bounded, so it cannot be the only ordering); a table's inverse digits have no such reader
    if (n == 1 && !capturing(c)) { hipEventRecord(c->ev_wdone, c->stream); c->wdone_pending = true; }
    write_done(c, o.st);
    o.st->state = false;                                                                       // ram.rs:648
    return FHERAM_OK;
}

// A whole write that starts here (a bank's range or list; fheram_write keeps its own body: its side stage may have begun with the words
// staged early, and it may be captured).  stage(d_w, ciphertexts) puts the words where the top takes them from, between the side stage —
// which needs no words — and the top; a refusal (a limb out of range) comes before anything of the RAM has been touched.
template <typename S>
int write_all(const Opnds& o, const RamView& v, S&& stage) {
    write_side_begin(o, v);
    int rc = stage(v.w, o.Y());
    if (rc != FHERAM_OK) { write_side_abort(o.c); return rc; }
    rc = write_top(o, v);
    return rc == FHERAM_OK ? write_rows(o, v) : rc;
}

}  // namespace

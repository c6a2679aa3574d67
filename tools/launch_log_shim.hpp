// tools/launch_log.hip: what this tree's csrc/ has no name for, and what it names differently from another tree.
namespace {

// read_top's fuse_ep and gated ask whether the final trace over Y ciphertexts takes the tail launch (path.hpp read_top, tail_top)
bool shim_tail_top(const fheram_ctx* c, int Y) { return chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail; }
// an operand set for the predicates alone; own_rows: a context's (n == 1) or a bank range's, else a batch's
Opnds shim_opnds(fheram_ctx* c, int n, int ws, bool own_rows) { return n == 1 ? one_addr(c, nullptr, ws, &c->ram) : table_opnds(c, &c->ram, nullptr, n, ws, nullptr, nullptr, own_rows ? MEMBER_MAP_IDENTITY : 0, own_rows); }
// the operand table of the row_chains cases: gy ciphertexts as two addresses that read the same rows (store_mapped off: the `_t` kernels,
// which are what a batch and a range launch; the lists' `_m` launchers are recorders of launch_log.hip's own, reached in path mode)
OpndTable shim_table(int gy) { return OpndTable{gy / 2, 1000, 0}; }
bool shim_needs_third(const fheram_ctx* c, int K) { return third_arena_needed(c, K * c->ws); }
// the buffers of a batch and of a bank's read list: field i of launch_log.hip's READS_FIELDS, and the digit table
int32_t*& reads_field(DenseBufs& L, int i) { int32_t** f[] = {&L.A, &L.B, &L.C, &L.res, &L.tmp, &L.tmp2}; return *f[i]; }
int32_t*& shim_batch_field(fheram_ctx* c, int i) { return reads_field(c->batch, i); }
int32_t*& shim_list_field(fheram_bank* b, int i) { return reads_field(b->list, i); }
void shim_batch_prep(fheram_ctx* c, double* prep) { c->batch.prep = prep; c->batch.cap = 4; }
void shim_list_prep(fheram_bank* b, double* prep) { b->list.prep = prep; b->list.cap = 8; }

// ---- path mode: where the per-RAM state lives, and how a context, a batch and a bank range are presented to the sequences ----------------
struct ShimState { bool state, memo_top; int memo_alone; bool res_in_trtop; };
ShimState of(const RamState& r) { return ShimState{r.state, r.memo_top, r.memo_alone, r.res_in_trtop}; }
ShimState shim_state(const fheram_ctx* c) { return of(c->ram); }
ShimState shim_state(const fheram_bank* b, int m) { return of(b->ram[m]); }
char shim_trhi(const fheram_ctx* c) { return c->trhi_in_C ? 'C' : 'A'; }
void shim_loaded(fheram_ctx* c) { c->ram.initialized = true; }
void shim_loaded(fheram_bank* b) { b->c->ram.initialized = true; for (int m = 0; m < b->M; m++) b->ram[m].initialized = true; }
void shim_new_keys(fheram_ctx* c) { c->ram.memo_top = false; c->ram.memo_alone = 0; }   // (fheram_keys_load)

int shim_read(fheram_ctx* c, const fheram_addr* addr, bool prepare_write) { return read_impl(one_addr(c, &addr), ctx_view(c), prepare_write); }
int shim_batch(fheram_ctx* c, const fheram_addr* const* addrs, int K) {   // fheram_read_batch (read_many, the buffers being there)
    const Opnds o = table_opnds(c, &c->ram, addrs, K, c->ws, c->batch.prep, nullptr, 0, false);
    const int rc = read_impl(o, dense_view(c, c->batch), false);
    launch_copy(c, o.slice(ref(c->batch.res, (long)fheram_ctx::GLWE, 0), K - 1), ref(c->d_res, (long)fheram_ctx::GLWE, 0), 1, c->ws);
    return rc;
}
template <typename S>
int shim_write(fheram_ctx* c, const fheram_addr* addr, S&& staged) {   // fheram_write; staged(d_w, ciphertexts): where the words are staged
    const Opnds o = one_addr(c, &addr);
    const RamView v = ctx_view(c);
    if (!c->side_begun) write_side_begin(o, v);
    int rc = staged(c->d_w, c->ws);
    if (rc != FHERAM_OK) { write_side_abort(c); return rc; }
    rc = write_top(o, v);
    return rc == FHERAM_OK ? write_rows(o, v) : rc;
}
// The bank's operations are the bank's own functions, behind their checks: the buffers being there, the reserves allocate nothing, and
// `staged` is the staging step of write_all.
int shim_bank_read(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, bool prepare_write) { return bank_read_set(b, MemberSet::range(first, n), addrs, prepare_write, nullptr); }
template <typename S>
int shim_bank_write(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, S&& staged) { return bank_write_set(b, MemberSet::range(first, n), addrs, staged); }
int shim_bank_rpw_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n) { return bank_read_set(b, MemberSet::list(members, n), addrs, true, nullptr); }
template <typename S>
int shim_bank_write_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, S&& staged) { return bank_write_set(b, MemberSet::list(members, n), addrs, staged); }
int shim_bank_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n) {   // fheram_bank_read_list, n > 1: its call of read_many without the reserve
    const MemberSet s = MemberSet::list(members, n);
    RamState st{true, false, false, 0, false};
    const Opnds o = table_opnds(b->c, &st, addrs, n, b->mws, b->list.prep, nullptr, s.map(), b->M > 1);
    const int rc = read_impl(o, dense_view(b->c, b->list), false);
    set_assign(b, s, st, false, false, true);
    for (int m = 0; m < b->M; m++) {
        int last = -1;
        for (int k = 0; k < n; k++) if (s.m[k] == m) last = k;
        if (last >= 0) launch_copy(b->c, o.slice(ref(b->list.res, (long)fheram_ctx::GLWE, 0), last), member_slot(b, b->c->d_res, m), 1, b->mws);
    }
    return rc;
}

// ---- the write lists: their buffers (field i of launch_log.hip's WL_FIELDS) and what the bank remembers of them --------------------------
int32_t*& shim_wl_field(fheram_bank* b, int i) {
    DenseBufs& L = b->wl;
    int32_t** f[] = {&L.A, &L.B, &L.C, &L.D, &L.part, &L.tmp, &L.tmp2, &L.res, &L.tree, &L.w, &L.trtop};
    return *f[i];
}
void shim_wl_cap(fheram_bank* b, int cap) { b->wl.cap = cap; }
std::string shim_wl_kept(const fheram_bank* b) {
    std::string s = "wl_holds=";
    for (int m = 0; m < b->M; m++) s += b->wl_holds[m] ? '1' : '0';
    char buf[96];
    std::snprintf(buf, sizeof buf, " kept_alone=%d kept_n=%d kept_map=%#x", b->kept_alone, b->kept_n, b->kept_map);
    return s + buf;
}

// ---- the refusals: the checks of the three forms as the entry points run them, and the state they look at -------------------------------
void shim_set_state(fheram_bank* b, int m, bool state) { b->ram[m].state = state; }
void shim_set_initialized(fheram_bank* b, int m, bool on) { b->ram[m].initialized = on; }
int shim_check_range(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, bool null_words, int want) {   // as the entry points call it
    MemberSet s;
    const char* null_args = want == 0 ? (addrs ? nullptr : "null address list") : want == 1 ? ((addrs && !null_words) ? nullptr : "null address list or null words") : nullptr;
    return range_check(b, first, n, want < 0 ? nullptr : addrs, null_args, want, &s);
}
int shim_check_rlist(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n) { MemberSet s; return read_list_check(b, members, addrs, n, &s); }
int shim_check_wlist(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, bool null_words, int want) { MemberSet s; return write_list_check(b, members, addrs, n, null_words, want, &s); }

// ---- the reserves: the two dense buffer sets ------------------------------------------------------------------------------------------
using ShimReadSet = DenseBufs;
int shim_reads_reserve(fheram_ctx* c, ShimReadSet& L, int n, int ws) { return dense_reserve(c, L, n, ws); }
void shim_reads_free(ShimReadSet& L) { dense_free(L); }
// the capacity and the buffers held: first those a set of that kind may hold, in the order of the struct this one replaced, then any other as "+<name>", which no log has
std::string shim_held(const DenseBufs& L, bool all) {
    using F = std::pair<const char*, const void*>;
    const F wl[] = {{"A", L.A}, {"B", L.B}, {"C", L.C}, {"D", L.D}, {"part", L.part}, {"tmp", L.tmp}, {"tmp2", L.tmp2}, {"res", L.res}, {"tree", L.tree}, {"w", L.w}, {"trtop", L.trtop}};
    const F reads[] = {{"A", L.A}, {"B", L.B}, {"C", L.C}, {"res", L.res}, {"tmp", L.tmp}, {"tmp2", L.tmp2}, {"prep", L.prep}, {"h_res", L.h_res}, {"d_h_res", L.d_h_res}};
    const F not_wl[] = {{"prep", L.prep}, {"h_res", L.h_res}, {"d_h_res", L.d_h_res}}, not_reads[] = {{"D", L.D}, {"part", L.part}, {"tree", L.tree}, {"w", L.w}, {"trtop", L.trtop}};
    std::string s = "cap=" + std::to_string(L.cap) + " holds";
    auto add = [&](const F* f, size_t n, const char* sep) { for (size_t i = 0; i < n; i++) if (f[i].second) s += std::string(sep) + f[i].first; };
    if (all) { add(wl, 11, " "); add(not_wl, 3, " +"); } else { add(reads, 9, " "); add(not_reads, 5, " +"); }
    return s;
}
std::string shim_reads_holds(const ShimReadSet& L) { return shim_held(L, false); }
int shim_wl_reserve(fheram_bank* b, int n) { return dense_reserve(b->c, b->wl, n, b->mws, true, &b->wl_fail_alloc); }
void shim_wl_free(fheram_bank* b) { dense_free(b->wl); }
std::string shim_wl_holds(const fheram_bank* b) { return shim_held(b->wl, true) + " fail_alloc=" + std::to_string(b->wl_fail_alloc); }

// ---- onerow mode: where the last operation of a kind left its outputs, the host stages, the one-row buffer sets ----------------------------
// kind: 0 list, 1 select, 2 regs, 3 table, 4 peek.  res / h mean something only while n > 0.
struct ShimLast { int n; const int32_t* res; const int64_t* h; int mix_slot; };
ShimLast shim_last(const fheram_bank* b, int kind) {
    const LastOutputs& L = b->last[kind];   // (LastKind is in this order)
    return ShimLast{L.n, L.home.res, L.home.h, L.home.mix_slot};
}
const int32_t* shim_regs_old(const fheram_bank* b) { return b->regs_old; }
const int32_t* shim_source(const fheram_bank* b, int kind, int index) { return select_source(b, fheram_select_src{kind, index}); }
// the host stages: busy flags, and the pinned side of each (what a refused or accepted call left staged)
std::string shim_busy(const fheram_bank* b) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "busy sel.host=%d lanes=%d regs.host=%d tabs.data=%d pub.host=%d pub.data=%d", b->sel.host.busy, b->lanes.busy, b->regs.stage.busy,
                  b->tabs.stage.busy, b->pub.host.busy, b->pub.data.busy);
    return buf;
}
struct ShimPinned { const char* name; const void* p; size_t bytes; };
int shim_pinned(const fheram_bank* b, ShimPinned* out) {   // up to 6
    const size_t G4 = fheram_ctx::GLWE * sizeof(int32_t);
    int n = 0;
    out[n++] = ShimPinned{"sel.host", b->sel.host.h, (size_t)b->sel.host_cap * G4};
    out[n++] = ShimPinned{"lanes", b->lanes.h, b->lanes.h ? (size_t)SELECT_LANES_CT_MAX * SELECT_CAND_MAX * sizeof(const int32_t*) : 0};
    out[n++] = ShimPinned{"regs.host", b->regs.stage.h, b->regs.cap ? (size_t)(1 << FHERAM_SELECT_BITS_MAX) * b->mws * G4 : 0};
    out[n++] = ShimPinned{"tabs.data", b->tabs.stage.h, b->tabs.cap ? (size_t)(1 << FHERAM_TABLE_BITS_MAX) * b->mws : 0};
    out[n++] = ShimPinned{"pub.host", b->pub.host.h, b->pub.cap ? (size_t)PUB_MAX * b->mws * G4 : 0};
    out[n++] = ShimPinned{"pub.data", b->pub.data.h, b->pub.cap ? (size_t)b->c->rows * N * b->mws : 0};
    return n;
}
// what each buffer set holds: the capacities and the buffers, in one order for every tree
std::string shim_sets(const fheram_bank* b) {
    using F = std::pair<const char*, const void*>;
    std::string s;
    auto add = [&](const char* set, std::initializer_list<int> caps, std::initializer_list<F> f) {
        s += std::string(s.empty() ? "" : " | ") + set + " cap=";
        bool first = true;
        for (int cp : caps) { s += (first ? "" : "/") + std::to_string(cp); first = false; }
        for (const F& x : f) if (x.second) s += std::string(" ") + x.first;
    };
    const SelectBufs& S = b->sel;
    add("sel", {S.cap, S.prep_cap, S.host_cap}, {{"packed", S.packed}, {"ep", S.ep}, {"tmp", S.tmp}, {"tmp2", S.tmp2}, {"res", S.res}, {"prep", S.prep}, {"h_res", S.h_res}, {"d_h_res", S.d_h_res}, {"d_host", S.host.d}, {"h_host", S.host.h}, {"ev", S.host.ev}});
    add("lanes", {}, {{"d_tab", b->lanes.d}, {"h_tab", b->lanes.h}, {"ev", b->lanes.ev}});
    const OneRowSet& R = b->regs;
    add("regs", {R.cap}, {{"fan", R.fan}, {"ep", R.ep}, {"tmp", R.tmp}, {"res", R.res}, {"prep", R.prep}, {"h_res", R.h_res}, {"d_h_res", R.d_h_res}, {"d_stage", R.stage.d}, {"h_stage", R.stage.h}, {"ev", R.stage.ev}});
    const OneRowSet& T = b->tabs;
    add("tabs", {T.cap}, {{"fan", T.fan}, {"ep", T.ep}, {"tmp", T.tmp}, {"res", T.res}, {"prep", T.prep}, {"h_res", T.h_res}, {"d_h_res", T.d_h_res}, {"d_stage", T.stage.d}, {"h_stage", T.stage.h}, {"ev", T.stage.ev}});
    const PublicBufs& P = b->pub;
    add("pub", {P.cap, P.cur}, {{"fan", P.fan}, {"tmp", P.tmp}, {"res0", P.res[0]}, {"res1", P.res[1]}, {"h_res", P.h_res}, {"d_h_res", P.d_h_res}, {"d_host", P.host.d}, {"h_host", P.host.h}, {"ev_host", P.host.ev}, {"d_data", P.data.d}, {"h_data", P.data.h}, {"ev_data", P.data.ev}});
    const MixBufs& M = b->mix;
    add("mix", {M.cap}, {{"ep", M.ep}, {"tmp", M.tmp}, {"res0", M.res[0]}, {"res1", M.res[1]}, {"res2", M.res[2]}, {"h_res", M.h_res}, {"d_h_res", M.d_h_res}, {"own", M.own}, {"keep", M.keep}, {"prep", M.prep}});
    return s + " | fail sel=" + std::to_string(b->sel_fail_alloc) + " pub=" + std::to_string(b->pub_fail_alloc) + " wl=" + std::to_string(b->wl_fail_alloc);
}
// what fheram_bank_destroy frees of the bank's own (the context is this program's)
void shim_release(fheram_bank* b) {
    dense_free(b->list); dense_free(b->wl); select_free(b->sel); lane_table_free(b->lanes);
    regs_bank_release(b); table_bank_release(b); mix_bufs_free(b->mix); public_bufs_free(b->pub);
}

}  // namespace

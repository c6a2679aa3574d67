// tools/launch_log.hip: what this tree's csrc/ has no name for, and what it names differently from another tree.
namespace {

// read_top's fuse_ep and gated ask whether the final trace over Y ciphertexts takes the tail launch (path.hpp read_top, tail_top)
bool shim_tail_top(const fheram_ctx* c, int Y) { return chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail; }
// an operand set for the predicates alone; own_rows: a context's (n == 1) or a bank range's, else a batch's
Opnds shim_opnds(fheram_ctx* c, int n, int ws, bool own_rows) { return n == 1 ? one_addr(c, nullptr, ws, &c->ram) : table_opnds(c, &c->ram, nullptr, n, ws, nullptr, nullptr, own_rows ? MEMBER_MAP_IDENTITY : 0, own_rows); }
// the operand table of the row_chains cases: gy ciphertexts as two addresses that read the same rows (store_mapped off: the `_t` kernels,
// which are what a batch and a range launch; the lists' `_m` kernels live in another translation unit and are not logged)
OpndTable shim_table(int gy) { return OpndTable{gy / 2, 1000, 0}; }
bool shim_needs_third(const fheram_ctx* c, int K) { return third_arena_needed(c, K * c->ws); }
// the buffers of a batch and of a bank's read list: field i of launch_log.hip's READS_FIELDS, and the digit table
int32_t*& reads_field(ReadBufs& L, int i) { int32_t** f[] = {&L.A, &L.B, &L.C, &L.res, &L.tmp, &L.tmp2}; return *f[i]; }
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
    const int rc = read_impl(o, reads_view(c, c->batch), false);
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
int shim_bank_read(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, bool prepare_write) {   // bank_read_op
    RamState st = bank_merge(b, first, n, false);
    const int rc = read_impl(bank_opnds(b, &st, addrs, n), bank_view(b, first), prepare_write);
    bank_assign(b, first, n, st, rc == FHERAM_OK && prepare_write, true);
    return rc;
}
int shim_bank_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n) {   // fheram_bank_read_list, n > 1 (read_many, the buffers being there)
    RamState st{true, false, false, 0, false};
    unsigned map = 0;
    for (int k = 0; k < n; k++) map |= (unsigned)members[k] << (4 * k);
    const Opnds o = table_opnds(b->c, &st, addrs, n, b->mws, b->list.prep, nullptr, map, b->M > 1);
    const int rc = read_impl(o, reads_view(b->c, b->list), false);
    const long G = (long)fheram_ctx::GLWE;
    for (int m = 0; m < b->M; m++) {
        int last = -1;
        for (int k = 0; k < n; k++) if (members[k] == m) last = k;
        if (last < 0) continue;
        RamState& r = b->ram[m];
        r.state = false; r.memo_top = false; r.memo_alone = 0; r.res_in_trtop = false;
        launch_copy(b->c, o.slice(ref(b->list.res, G, 0), last), ref(b->c->d_res + (size_t)m * b->mws * G, G, 0), 1, b->mws);
    }
    return rc;
}
template <typename S>
int shim_bank_write(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, S&& staged) {   // fheram_bank_write
    RamState st = bank_merge(b, first, n, true);
    const Opnds o = bank_opnds(b, &st, addrs, n);
    const RamView v = bank_view(b, first);
    write_side_begin(o, v);
    int rc = staged(v.w, n * b->mws);
    if (rc != FHERAM_OK) { write_side_abort(b->c); bank_assign(b, first, n, st, true, false); return rc; }
    rc = write_top(o, v);
    if (rc == FHERAM_OK) rc = write_rows(o, v);
    bank_assign(b, first, n, st, rc != FHERAM_OK, false);
    return rc;
}

}  // namespace

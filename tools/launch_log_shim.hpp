// tools/launch_log.hip: what this tree's csrc/ has no name for, and what it names differently from another tree.
namespace {

// read_top's fuse_ep and gated ask whether the final trace over Y ciphertexts takes the tail launch (path.hpp read_top, tail_top)
bool shim_tail_top(const fheram_ctx* c, int Y) { return chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail; }
// an operand set for the predicates alone
Opnds shim_opnds(fheram_ctx* c, int n, int ws, bool own_rows) { return Opnds{c, &c->ram, nullptr, n, ws, nullptr, nullptr, 0, own_rows}; }

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
int shim_batch(fheram_ctx* c, const fheram_addr* const* addrs, int K) { return read_impl(batch_opnds(c, addrs, K), batch_view(c), false); }
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

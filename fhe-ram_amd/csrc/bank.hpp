// Included by fheram.hip (same translation unit): fheram_bank — M RAMs of the same shape under ONE prepared key set, and Ram::read /
// read_prepare_write / write (ram.rs:172-294) on a contiguous range of them as ONE operation, one address per member.
// Ram objects are independent units (ram.rs:25-29; `&mut self` serialises per RAM only), so nothing orders operations on different RAMs.
//
// Structure: ONE internal context whose word count is M * ws.  Rows, arenas, tree, results, words and temporaries are laid out
// [M * ws][...], so ciphertext y = m * ws + w is word w of member m, and a member range [first, first + n) is a pointer offset plus
// gy = n * ws: a RamView of its own (bank_view).  On that view the operation is path.hpp's read_impl / write_side_begin / write_top /
// write_rows with the operand set of the range (bank_opnds):
//   - a range of ONE member is the plain operation (one_addr), memo included;
//   - a wider range has its digits in a table: every address-independent step is one launch over n * ws ciphertexts, the address-dependent
//     products take the table where a table form exists (k_read_chain_t, k_trace_tail_t with its k_read_chain_t fallback,
//     k_write_chain_t) and run one launch per member on the member's y-slice everywhere else (prepare, the GGSW inversion, the unfused
//     product chains, n2 == 1).
// Per-member state (the state flag, what read_prepare_write kept for the write, where the last result is) lives here, one RamState per
// member; an operation runs on the merge of its range's (bank_merge) and hands the outcome back to every member of it (bank_assign).  The
// context is never made to look like a range: after fheram_bank_create nothing here writes a field of it (and create itself writes none of its switches).  The write's inverse digits are
// never started early in a bank of more than one member (pre_inv shares d_prep_inv and d_tail_sync between members); a bank of ONE member
// is a plain context in every respect.
// A READ LIST (fheram_bank_read_list) is the general read: entry k reads member members[k], in any order and with repeats.  It is the same
// read_impl on the same kind of operand set (path.hpp table_opnds) with the members as its source map, over the whole bank's rows (one
// member index per entry: Opnds::rows for the per-entry launches, k_read_chain_t for the rows' chain — a range is the identity map, a
// batch the map 0, 0, ...); the digits sit in a table of the list's own, and every launch writes buffers of the list's own (ReadBufs, the
// very set a batch has: path.hpp read_many) — so the arenas, trtop and tree of a member that sits between read_prepare_write and write are not touched.  It runs on a scratch RamState; every named member is then left as a
// read leaves it, with the result of the last entry that named it in its slice of d_res.
// A WRITE LIST (fheram_bank_read_prepare_write_list / fheram_bank_write_list) is the general read_prepare_write / write: entry k works on
// member members[k], distinct members in any order (a RAM has one pending write).  The same read_impl / write_side_begin / write_top /
// write_rows on table_opnds with the members as the map and the bank's d_prep / d_prep_inv (n <= M), over the whole bank's rows: the table
// chains read AND store the rows through the map (k_read_chain_m / k_write_chain_m, mapped_chains.hip), every launch without a table form goes
// member by member through Opnds::rows.  Every other buffer of the view is dense, [n * mws], and the lists' own (WriteListBufs) — not the
// read list's, so that a read list between the two halves destroys nothing.  Per-member hand-over: read_prepare_write copies every entry's
// tree top and result into the member's own slots and sets its RamState, so ranges, single calls and downloads see a prepared member like
// any other; a write list gathers tree and trace(top) from those slots and scatters the tree back.  The rows after the alone levels stay in
// the lists' arena A: they count for a write list of the same members in the same order while every one of them still holds them (wl_holds).
// A list of one member, or of a contiguous ascending run, IS the range operation.
// Bank operations are never captured into a hipGraph: under graph = 1 they are enqueued directly, in the forms that mode selects.
#pragma once
#include "path.hpp"

// The dense buffers of a read_prepare_write / write list: for `cap` entries of mws ciphertexts, allocated on first use, grown to the largest
// list seen, freed with the bank.
struct WriteListBufs {
    int cap = 0;
    int32_t *A = nullptr, *B = nullptr, *C = nullptr, *D = nullptr;   // [cap * mws][rows]
    int32_t *part = nullptr, *tmp = nullptr, *tmp2 = nullptr, *res = nullptr, *tree = nullptr, *w = nullptr, *trtop = nullptr;   // [cap * mws]
    // what the last read_prepare_write list left in A (RamState::memo_alone of a list): for kept_n entries with the map kept_map
    int kept_alone = 0, kept_n = 0;
    unsigned kept_map = 0;
};

struct fheram_bank {
    fheram_ctx* c = nullptr;      // word count M * mws; never row-sharded, never part of a group
    int M = 0, mws = 0;
    RamState ram[FHERAM_BANK_MAX];
    double* d_prep = nullptr;     // [n][n_digits] prepared GGSW: the digits of the k-th address of the range being read   (M > 1)
    double* d_prep_inv = nullptr; // [n][n_digits] the inverse digits of the k-th address of the range being written      (M > 1)
    ReadBufs list;                // fheram_bank_read_list: buffers of its own (path.hpp reads_reserve), sized by mws
    int list_n = 0;               // entries of the last list (their results are in list.res); 0: none has run
    WriteListBufs wl;             // fheram_bank_read_prepare_write_list / fheram_bank_write_list: buffers of their own, sized by mws
    bool wl_holds[FHERAM_BANK_MAX] = {};   // member m is still as the list that filled wl.A left it (cleared by whatever touches the member)
    int wl_fail_alloc = 0;        // fheram_bank_selftest_fail_list_alloc: the wl_fail_alloc-th next device allocation of wl fails (0: none)
};

namespace {

// The buffers as one operation on members [first, first + n) sees them: each starts at the range's first ciphertext (Y = n * mws is the operand set's).
RamView bank_view(const fheram_bank* b, int first) {
    RamView v = ctx_view(b->c);
    const size_t o1 = (size_t)first * b->mws * fheram_ctx::GLWE, oR = o1 * b->c->rows;
    for (int32_t** p : {&v.rows, &v.A, &v.B, &v.C, &v.D}) *p += oR;
    for (int32_t** p : {&v.part, &v.tmp, &v.tmp2, &v.res, &v.tree, &v.w, &v.trtop}) *p += o1;
    return v;
}
// the operand set of an operation on a range: one member is the plain operation on the view; more have their digits in the bank's tables
// and address k works on member k of the view
Opnds bank_opnds(fheram_bank* b, RamState* st, const fheram_addr* const* addrs, int n) {
    if (n == 1) return one_addr(b->c, addrs, b->mws, st);
    return table_opnds(b->c, st, addrs, n, b->mws, b->d_prep, b->d_prep_inv, MEMBER_MAP_IDENTITY, true);
}

// ---- checks: the whole range (or list) before anything is enqueued --------------------------------------------------------------------
int check_addrs(fheram_ctx* c, const fheram_addr* const* addrs, int n) {
    for (int k = 0; k < n; k++) {
        if (!addrs[k] || addrs[k]->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "address " + std::to_string(k) + " is null or does not belong to this bank (layout mismatch, ram.rs:404)");
        if (addrs[k]->empty) return fail(c, FHERAM_ERR_INVALID_ARG, "address " + std::to_string(k) + " is an empty address: fheram_bank_address_alloc without fheram_bank_address_derive");
    }
    return FHERAM_OK;
}
int bank_check(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int want_state) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    if (first < 0 || n < 1 || first > b->M - n)
        return fail(c, FHERAM_ERR_INVALID_ARG, "member range [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") is empty or outside the bank's " + std::to_string(b->M) + " members");
    if (addrs) { const int rc = check_addrs(c, addrs, n); if (rc != FHERAM_OK) return rc; }
    for (int m = first; m < first + n; m++)
        if (!b->ram[m].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (member " + std::to_string(m) + ")");
    if (want_state < 0) return FHERAM_OK;
    if (!addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null address list");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int m = first; m < first + n; m++) {
        if (want_state == 0 && b->ram[m].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.read: internal state is true -> requires calling Memory.write (member " + std::to_string(m) + ")");
        if (want_state == 1 && !b->ram[m].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.write: internal state is false -> requires calling Memory.read_prepare_write (member " + std::to_string(m) + ")");
    }
    return FHERAM_OK;
}
// the RAM state an op on [first, first + n) starts from: what read_prepare_write kept counts only when every member of the range holds it
RamState bank_merge(const fheram_bank* b, int first, int n, bool state) {
    RamState s{true, state, true, b->ram[first].memo_alone, false};
    for (int m = first; m < first + n; m++) {
        s.memo_top = s.memo_top && b->ram[m].memo_top;
        if (b->ram[m].memo_alone != s.memo_alone) s.memo_alone = 0;
    }
    return s;
}
// ... and what the op left of it, for every member of the range; new_result: the op was a read
void bank_assign(fheram_bank* b, int first, int n, const RamState& s, bool state, bool new_result) {
    for (int m = first; m < first + n; m++) {
        RamState& r = b->ram[m];
        r.state = state; r.memo_top = s.memo_top; r.memo_alone = s.memo_alone;
        if (new_result) r.res_in_trtop = s.res_in_trtop;
        b->wl_holds[m] = false;
    }
}
// the results of members [first, first + n), widened into h_res by the device; out: [n][mws][GLWE] int64
int bank_result(fheram_bank* b, int first, int n, int64_t* out) {
    fheram_ctx* c = b->c;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    ResRun runs[FHERAM_BANK_MAX];
    int n_runs = 0;
    for (int k = 0; k < n;) {      // one run per stretch of members whose result sits in the same buffer
        int e = k + 1;
        while (e < n && b->ram[first + e].res_in_trtop == b->ram[first + k].res_in_trtop) e++;
        runs[n_runs++] = ResRun{(b->ram[first + k].res_in_trtop ? c->d_trtop : c->d_res) + (size_t)(first + k) * per, (size_t)(e - k) * per};
        k = e;
    }
    return result_export(c, runs, n_runs, c->h_res, c->d_h_res, out);
}
int bank_read_op(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, bool prepare_write, int64_t* out) {
    if (b && !addrs) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null address list");
    int rc = bank_check(b, first, n, addrs, 0);
    if (rc != FHERAM_OK) return rc;
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    RamState st = bank_merge(b, first, n, false);
    rc = read_impl(bank_opnds(b, &st, addrs, n), bank_view(b, first), prepare_write);
    bank_assign(b, first, n, st, rc == FHERAM_OK && prepare_write, true);                   // ram.rs:533
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipGetLastError());
    return out ? bank_result(b, first, n, out) : FHERAM_OK;
}


// ---- the read list ---------------------------------------------------------------------------------------------------------------
// the whole list before anything is enqueued; codes, order and messages as bank_check
int list_check(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    if (!members || !addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null member list or null address list");
    if (n < 1 || n > FHERAM_READ_LIST_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_READ_LIST_MAX = " + std::to_string(FHERAM_READ_LIST_MAX) + "]");
    if ((long)n * b->mws > 64)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n * word_size = " + std::to_string((long)n * b->mws) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    for (int k = 0; k < n; k++)
        if (members[k] < 0 || members[k] >= b->M)
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names member " + std::to_string(members[k]) + ", outside the bank's " + std::to_string(b->M) + " members");
    const int rc = check_addrs(c, addrs, n);
    if (rc != FHERAM_OK) return rc;
    for (int k = 0; k < n; k++)
        if (!b->ram[members[k]].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (member " + std::to_string(members[k]) + ")");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int k = 0; k < n; k++)
        if (b->ram[members[k]].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.read: internal state is true -> requires calling Memory.write (member " + std::to_string(members[k]) + ")");
    return FHERAM_OK;
}
int list_result(fheram_bank* b, int first, int n, int64_t* out) { return reads_export(b->c, b->list, (size_t)first * b->mws, (size_t)n * b->mws, out); }

// ---- the write lists -------------------------------------------------------------------------------------------------------------
void wlist_free(WriteListBufs& L) {
    void* bufs[] = {L.A, L.B, L.C, L.D, L.part, L.tmp, L.tmp2, L.res, L.tree, L.w, L.trtop};
    for (void* p : bufs) if (p) hipFree(p);
    L = WriteListBufs{};
}
// grows the buffers to n entries of ws ciphertexts; on failure the bank holds none of them (and every other operation is unaffected: what a
// prepared member needs for its write is in its own slots).  Regrowing drops the kept arena, never a member's state.
int wlist_reserve(fheram_ctx* c, WriteListBufs& L, int n, int ws, int* fail_alloc) {
    if (n <= L.cap) return FHERAM_OK;
    if (L.cap) { for (hipStream_t s : {c->stream, c->stream2}) HIPCHK(c, hipStreamSynchronize(s)); wlist_free(L); }
    const size_t G = fheram_ctx::GLWE, nct = (size_t)n * ws, nrow = nct * c->rows;
    hipError_t e = hipSuccess;
    auto dev = [&](int32_t** p, size_t glwes) {
        if (e != hipSuccess) return;
        if (*fail_alloc > 0 && --*fail_alloc == 0) e = hipErrorOutOfMemory;   // (the self-test's: as the runtime reports an exhausted device)
        else e = hipMalloc((void**)p, glwes * G * sizeof(int32_t));
    };
    for (int32_t** p : {&L.A, &L.B, &L.C, &L.D}) dev(p, nrow);
    for (int32_t** p : {&L.part, &L.tmp, &L.tmp2, &L.res, &L.tree, &L.w, &L.trtop}) dev(p, nct);
    if (e != hipSuccess) {
        wlist_free(L);
        (void)hipGetLastError();   // the next op's error check must not see this allocation's failure
        return fail(c, FHERAM_ERR_DEVICE, std::string("buffers of a write list of ") + std::to_string(n) + " members: " + hipGetErrorString(e));
    }
    L.cap = n;
    return FHERAM_OK;
}
RamView wlist_view(const fheram_bank* b) {
    const WriteListBufs& L = b->wl;
    return RamView{b->c->d_data, L.A, L.B, L.C, L.D, L.part, L.tmp, L.tmp2, L.res, L.tree, L.w, L.trtop};
}
unsigned wlist_map(const int* members, int n) {
    unsigned map = 0;
    for (int k = 0; k < n; k++) map |= (unsigned)members[k] << (4 * k);
    return map;
}
// a list of one member or of a contiguous ascending run is the range [members[0], members[0] + n)
bool wlist_is_range(const int* members, int n) {
    for (int k = 1; k < n; k++) if (members[k] != members[0] + k) return false;
    return true;
}
// the whole list before anything is enqueued; codes, order and messages as list_check.  want_state: 0 read_prepare_write, 1 write
int wlist_check(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, bool null_words, int want_state) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    if (!members || !addrs || null_words) return fail(c, FHERAM_ERR_INVALID_ARG, want_state ? "null member list, null address list or null words" : "null member list or null address list");
    if (n < 1 || n > b->M)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, the bank's " + std::to_string(b->M) + " members]");
    unsigned seen = 0;
    for (int k = 0; k < n; k++) {
        if (members[k] < 0 || members[k] >= b->M)
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names member " + std::to_string(members[k]) + ", outside the bank's " + std::to_string(b->M) + " members");
        if (seen & (1u << members[k]))
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names member " + std::to_string(members[k]) + " a second time: a RAM has one pending write (ram.rs:196-294), so the members of a write list are distinct");
        seen |= 1u << members[k];
    }
    const int rc = check_addrs(c, addrs, n);
    if (rc != FHERAM_OK) return rc;
    for (int k = 0; k < n; k++)
        if (!b->ram[members[k]].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (member " + std::to_string(members[k]) + ")");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int k = 0; k < n; k++) {
        if (want_state == 0 && b->ram[members[k]].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.read: internal state is true -> requires calling Memory.write (member " + std::to_string(members[k]) + ")");
        if (want_state == 1 && !b->ram[members[k]].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.write: internal state is false -> requires calling Memory.read_prepare_write (member " + std::to_string(members[k]) + ")");
    }
    return FHERAM_OK;
}
// member m's [mws] slot of a per-ciphertext buffer of the context
GlweRef member_slot(const fheram_bank* b, int32_t* buf, int m) { return ref(buf + (size_t)m * b->mws * fheram_ctx::GLWE, (long)fheram_ctx::GLWE, 0); }

}  // namespace

extern "C" {

int fheram_bank_create(const fheram_params* p, int device, int n_members, const fheram_config* cfg, fheram_bank** out) {
    if (!p || !out) return fail(nullptr, FHERAM_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_members < 1 || n_members > FHERAM_BANK_MAX)
        return fail(nullptr, FHERAM_ERR_INVALID_ARG, "n_members = " + std::to_string(n_members) + " is outside [1, FHERAM_BANK_MAX = " + std::to_string(FHERAM_BANK_MAX) + "]");
    if ((uint64_t)n_members * p->word_size > 64)
        return fail(nullptr, FHERAM_ERR_INVALID_ARG, "n_members * word_size = " + std::to_string((uint64_t)n_members * p->word_size) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    fheram_params wide = *p;
    wide.word_size = (uint32_t)n_members * p->word_size;
    // more than one member: the write's inverse digits are never started early (header comment); 0 survives every rule of config_in_effect
    fheram_config asked;
    if (cfg) asked = *cfg; else fheram_config_default(&asked);
    if (n_members > 1) asked.pre_inv = 0;
    fheram_ctx* c = nullptr;
    const int rc = fheram_ctx_create_cfg(&wide, device, 0, 1, &asked, &c);   // the parameter checks, then "no HIP device"
    if (rc != FHERAM_OK) return rc;
    fheram_bank* b = new fheram_bank();
    b->c = c; b->M = n_members; b->mws = (int)p->word_size;
    c->ram.initialized = true;   // (per member: fheram_bank::ram)
    if (n_members > 1) {   // the operand tables: the context's resources, freed with it
        const size_t bytes = (size_t)n_members * c->n_digits * fheram_ctx::GGSW * sizeof(double);
        hipError_t e = c->res.device(&b->d_prep, bytes);
        if (e == hipSuccess) e = c->res.device(&b->d_prep_inv, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            fheram_bank_destroy(b);
            return fail(nullptr, FHERAM_ERR_DEVICE, std::string("operand tables of the bank: ") + hipGetErrorString(e));
        }
    }
    *out = b;
    return FHERAM_OK;
}
void fheram_bank_destroy(fheram_bank* b) {
    if (!b) return;
    if (b->c) { hipSetDevice(b->c->device); for (hipStream_t s : {b->c->stream, b->c->stream2}) if (s) hipStreamSynchronize(s); }
    reads_free(b->list);
    wlist_free(b->wl);
    fheram_ctx_destroy(b->c);
    delete b;
}
const char* fheram_bank_last_error(const fheram_bank* b) { return fheram_last_error(b ? b->c : nullptr); }
int fheram_bank_size(const fheram_bank* b) { return b ? b->M : 0; }

int fheram_bank_keys_load(fheram_bank* b, const int64_t* gal_els, int n_gal, const int64_t* const* atk_glwe,
                          const int64_t* atk_ggsw_inv, int64_t atk_ggsw_inv_p, const int64_t* tsk) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    const int rc = fheram_keys_load(b->c, gal_els, n_gal, atk_glwe, atk_ggsw_inv, atk_ggsw_inv_p, tsk);
    if (rc != FHERAM_OK) return rc;
    for (int m = 0; m < b->M; m++) { b->ram[m].memo_top = false; b->ram[m].memo_alone = 0; b->wl_holds[m] = false; }   // kept traces are void with new keys
    return FHERAM_OK;
}
int fheram_bank_ram_upload(fheram_bank* b, int member, const int64_t* rows) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (member < 0 || member >= b->M) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member");
    if (!rows) return fail(c, FHERAM_ERR_INVALID_ARG, "null rows");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)b->mws * c->rows * fheram_ctx::GLWE;
    const int rc = upload_i64(c, c->d_data + (size_t)member * n, rows, n);
    if (rc != FHERAM_OK) return rc;
    RamState& r = b->ram[member];
    r.initialized = true; r.state = false; r.memo_top = false; r.memo_alone = 0;
    b->wl_holds[member] = false;
    return FHERAM_OK;
}
int fheram_bank_ram_download(fheram_bank* b, int member, int64_t* rows) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (member < 0 || member >= b->M || !rows) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member, or null rows");
    if (!b->ram[member].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)b->mws * c->rows * fheram_ctx::GLWE;
    const int rc = download_i64(c, rows, c->d_data + (size_t)member * n, n);
    return rc == FHERAM_OK ? check_precision(c) : rc;
}
int fheram_bank_ram_tree_download(fheram_bank* b, int member, int level, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (member < 0 || member >= b->M || !out) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member, or null output");
    if (level != 0 || c->n2 < 2) return fail(c, FHERAM_ERR_INVALID_ARG, "tree level does not exist (ram.rs:315-324)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)b->mws * fheram_ctx::GLWE;
    return download_i64(c, out, c->d_tree + (size_t)member * n, n);
}
int fheram_bank_ram_state(const fheram_bank* b, int member) { return (b && member >= 0 && member < b->M) ? (int)b->ram[member].state : 0; }

int fheram_bank_address_create(fheram_bank* b, const int64_t* const* ggsw, int n_ggsw, fheram_addr** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_address_create(b->c, ggsw, n_ggsw, out);
}

// Addresses derived from encrypted integers (setup.hpp fheram_address_derive): the bank's integers, addresses and the one launch are its
// context's; a derived address is an ordinary bank address and may serve several members.
int fheram_bank_fheuint_create(fheram_bank* b, const int64_t* bits, int n_bits, fheram_fheuint** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_fheuint_create(b->c, bits, n_bits, out);
}
int fheram_bank_address_alloc(fheram_bank* b, fheram_addr** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_address_alloc(b->c, out);
}
int fheram_bank_address_derive(fheram_bank* b, const fheram_fheuint* const* fus, int n, int sign, fheram_addr* const* addrs) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_address_derive(b->c, fus, n, sign, addrs);
}

int fheram_bank_read(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int64_t* out) {
    return bank_read_op(b, first, n, addrs, false, out);
}
int fheram_bank_read_prepare_write(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int64_t* out) {
    return bank_read_op(b, first, n, addrs, true, out);
}
int fheram_bank_write(fheram_bank* b, int first, int n, const int64_t* w, const fheram_addr* const* addrs) {
    if (b && (!addrs || !w)) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null address list or null words");
    int rc = bank_check(b, first, n, addrs, 1);
    if (rc != FHERAM_OK) return rc;
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    RamState st = bank_merge(b, first, n, true);
    const Opnds o = bank_opnds(b, &st, addrs, n);
    const RamView v = bank_view(b, first);
    write_side_begin(o, v);                         // as fheram_write: the part that needs no words is enqueued before the host narrows them
    rc = stage_words(c, v.w, w, n * b->mws);
    if (rc != FHERAM_OK) {                          // (a limb out of range: nothing of the members has been touched)
        write_side_abort(c);
        bank_assign(b, first, n, st, true, false);
        return rc;
    }
    rc = write_top(o, v);
    if (rc == FHERAM_OK) rc = write_rows(o, v);
    bank_assign(b, first, n, st, rc != FHERAM_OK, false);                                   // ram.rs:648
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipGetLastError());
    return FHERAM_OK;
}
int fheram_bank_result_download(fheram_bank* b, int first, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    const int rc = bank_check(b, first, n, nullptr, -1);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(b->c, hipSetDevice(b->c->device));
    return bank_result(b, first, n, out);
}
// K = n independent Ram::read (ram.rs:172-191), entry k on member members[k], as one operation: path.hpp read_many with the members as the
// source map, on the list's own buffers and a scratch RamState.  What the sequence of those K single-member reads leaves: every named member
// in state 0 with nothing kept for a write, the result of the last entry that named it where its own read would have left it (its slice of
// d_res); every other member as it was.  A bank of one member has one source: the list is what fheram_read_batch runs.
int fheram_bank_read_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, int64_t* out) {
    int rc = list_check(b, members, addrs, n);
    if (rc != FHERAM_OK) return rc;
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    const long G = (long)fheram_ctx::GLWE;
    auto res_of = [&](int m) { return ref(c->d_res + (size_t)m * b->mws * G, G, 0); };
    b->list_n = 0;   // until this list is enqueued there is no last list: several entries overwrite res as they run (one entry only with its closing copy, but the rule is one)
    if (n == 1) {   // the plain single-member read; its result is also the list's
        rc = reads_reserve(c, b->list, 1, b->mws);
        if (rc == FHERAM_OK) rc = bank_read_op(b, members[0], 1, addrs, false, nullptr);
        if (rc != FHERAM_OK) return rc;
        launch_copy(c, res_of(members[0]), ref(b->list.res, G, 0), 1, b->mws);
        b->list_n = 1;
        HIPCHK(c, hipGetLastError());
        return out ? list_result(b, 0, 1, out) : FHERAM_OK;
    }
    RamState st{true, false, false, 0, false};
    unsigned map = 0;
    for (int k = 0; k < n; k++) map |= (unsigned)members[k] << (4 * k);
    return read_many(c, b->list, &st, addrs, n, b->mws, map, b->M > 1, out, [&](const Opnds& o) {
        for (int m = 0; m < b->M; m++) {
            int last = -1;
            for (int k = 0; k < n; k++) if (members[k] == m) last = k;
            if (last < 0) continue;
            RamState& r = b->ram[m];
            r.state = false; r.memo_top = false; r.memo_alone = 0; r.res_in_trtop = false;
            launch_copy(c, o.slice(ref(b->list.res, G, 0), last), res_of(m), 1, b->mws);
        }
        b->list_n = n;
    });
}
// n independent Ram::read_prepare_write (ram.rs:196-222), entry k on member members[k], as one operation (header comment: a write list).
int fheram_bank_read_prepare_write_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, int64_t* out) {
    int rc = wlist_check(b, members, addrs, n, false, 0);
    if (rc != FHERAM_OK) return rc;
    if (wlist_is_range(members, n)) return bank_read_op(b, members[0], n, addrs, true, out);
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    rc = wlist_reserve(c, b->wl, n, b->mws, &b->wl_fail_alloc);
    if (rc != FHERAM_OK) return rc;
    WriteListBufs& L = b->wl;
    L.kept_alone = 0;   // arena A is this list's from here on
    RamState st{true, false, false, 0, false};
    const Opnds o = table_opnds(c, &st, addrs, n, b->mws, b->d_prep, b->d_prep_inv, wlist_map(members, n), true);
    rc = read_impl(o, wlist_view(b), true);
    if (rc != FHERAM_OK) return rc;
    // the hand-over: tree top and result into every member's own slots, where a range, a single call or a download looks for them
    const long G = (long)fheram_ctx::GLWE;
    ResRun runs[FHERAM_BANK_MAX];
    for (int k = 0; k < n; k++) {
        const int m = members[k];
        if (c->n2 == 2) launch_copy(c, o.slice(ref(L.tree, G, 0), k), member_slot(b, c->d_tree, m), 1, b->mws);
        int32_t* res_to = st.res_in_trtop ? c->d_trtop : c->d_res;
        launch_copy(c, o.slice(ref(st.res_in_trtop ? L.trtop : L.res, G, 0), k), member_slot(b, res_to, m), 1, b->mws);
        RamState& r = b->ram[m];
        r.state = true; r.memo_top = st.memo_top; r.memo_alone = 0; r.res_in_trtop = st.res_in_trtop;   // (memo_alone is the context's arena: not this list's)
        b->wl_holds[m] = st.memo_alone > 0;
        runs[k] = ResRun{member_slot(b, res_to, m).p, (size_t)b->mws * fheram_ctx::GLWE};
    }
    L.kept_alone = st.memo_alone; L.kept_n = n; L.kept_map = o.member_map;
    HIPCHK(c, hipGetLastError());
    return out ? result_export(c, runs, n, c->h_res, c->d_h_res, out) : FHERAM_OK;
}
// n independent Ram::write (ram.rs:226-294), entry k of w to member members[k], as one operation (header comment: a write list).
int fheram_bank_write_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, const int64_t* w) {
    int rc = wlist_check(b, members, addrs, n, !w, 1);
    if (rc != FHERAM_OK) return rc;
    if (wlist_is_range(members, n)) return fheram_bank_write(b, members[0], n, w, addrs);
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    rc = wlist_reserve(c, b->wl, n, b->mws, &b->wl_fail_alloc);
    if (rc != FHERAM_OK) return rc;
    WriteListBufs& L = b->wl;
    const unsigned map = wlist_map(members, n);
    // what the write resumes from: trace(top) when every member holds its own, the kept arena when it is this very list's
    RamState st{true, true, true, 0, false};
    bool holds = L.kept_alone > 0 && L.kept_n == n && L.kept_map == map;
    for (int k = 0; k < n; k++) {
        st.memo_top = st.memo_top && b->ram[members[k]].memo_top;
        holds = holds && b->wl_holds[members[k]];
    }
    if (holds) st.memo_alone = L.kept_alone;
    L.kept_alone = 0;   // consumed, or overwritten by this write's trace(ct_hi)
    const Opnds o = table_opnds(c, &st, addrs, n, b->mws, b->d_prep, b->d_prep_inv, map, true);
    const RamView v = wlist_view(b);
    const long G = (long)fheram_ctx::GLWE;
    // The gather: every member's tree top and trace(top) into the list's dense buffers — unless this very list prepared the members and
    // all still hold it (holds): then L.tree and L.trtop are what the hand-over copied FROM, nothing has written them since (every list
    // operation ends `holds`), no launch is needed, and write_side_begin may skip its fork event after a host wait as fheram_bank_write's
    // does (main_idle).  With a gather the main stream has work again, so the side stage forks behind it: one event record.
    if (!holds) {
        main_enqueued(c);
        for (int k = 0; k < n; k++) {
            if (c->n2 == 2) launch_copy(c, member_slot(b, c->d_tree, members[k]), o.slice(ref(L.tree, G, 0), k), 1, b->mws);
            if (st.memo_top) launch_copy(c, member_slot(b, c->d_trtop, members[k]), o.slice(ref(L.trtop, G, 0), k), 1, b->mws);
        }
    }
    auto assign = [&](bool state) {
        for (int k = 0; k < n; k++) {
            RamState& r = b->ram[members[k]];
            r.state = state; r.memo_top = st.memo_top; r.memo_alone = 0;
            b->wl_holds[members[k]] = false;
        }
    };
    write_side_begin(o, v);
    rc = stage_words(c, v.w, w, n * b->mws);
    if (rc != FHERAM_OK) {                          // (a limb out of range: nothing of the members has been touched)
        write_side_abort(c);
        assign(true);
        return rc;
    }
    rc = write_top(o, v);
    if (rc == FHERAM_OK) rc = write_rows(o, v);
    if (rc == FHERAM_OK && c->n2 == 2)              // the scatter: the tree's new top (ct_lo, rotated) back into every member's slot
        for (int k = 0; k < n; k++) launch_copy(c, o.slice(ref(L.tree, G, 0), k), member_slot(b, c->d_tree, members[k]), 1, b->mws);
    assign(rc != FHERAM_OK);                                                                // ram.rs:648
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipGetLastError());
    return FHERAM_OK;
}
int fheram_bank_selftest_fail_list_alloc(fheram_bank* b, int nth) {
    if (!b || nth < 0) return FHERAM_ERR_INVALID_ARG;
    b->wl_fail_alloc = nth;
    return FHERAM_OK;
}
int fheram_bank_read_list_result(fheram_bank* b, int first, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!out) return fail(c, FHERAM_ERR_INVALID_ARG, "null output");
    if (!b->list_n) return fail(c, FHERAM_ERR_STATE, "no read list has run on this bank");
    if (first < 0 || n < 1 || first > b->list_n - n)
        return fail(c, FHERAM_ERR_INVALID_ARG, "entries [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") are empty or outside the last list's " + std::to_string(b->list_n) + " entries");
    HIPCHK(c, hipSetDevice(c->device));
    return list_result(b, first, n, out);
}
int fheram_bank_sync(fheram_bank* b) { return b ? fheram_sync(b->c) : FHERAM_ERR_INVALID_ARG; }
int fheram_bank_roundoff_max(fheram_bank* b, double* max_out) { return b ? fheram_roundoff_max(b->c, max_out) : FHERAM_ERR_INVALID_ARG; }
int fheram_bank_roundoff_reset(fheram_bank* b) { return b ? fheram_roundoff_reset(b->c) : FHERAM_ERR_INVALID_ARG; }
int fheram_bank_tail_stats(fheram_bank* b, uint64_t* launches, uint64_t* fallbacks) { return b ? fheram_tail_stats(b->c, launches, fallbacks) : FHERAM_ERR_INVALID_ARG; }
int fheram_bank_mid_stats(fheram_bank* b, uint64_t* launches, uint64_t* fallbacks) { return b ? fheram_mid_stats(b->c, launches, fallbacks) : FHERAM_ERR_INVALID_ARG; }
int fheram_bank_profile_enable(fheram_bank* b, int on) { return b ? fheram_profile_enable(b->c, on) : FHERAM_ERR_INVALID_ARG; }
int fheram_bank_profile_get(fheram_bank* b, const char* cls, uint64_t* launches, uint64_t* blocks, double* total_ms) {
    return b ? fheram_profile_get(b->c, cls, launches, blocks, total_ms) : FHERAM_ERR_INVALID_ARG;
}
int fheram_bank_profile_reset(fheram_bank* b) { return b ? fheram_profile_reset(b->c) : FHERAM_ERR_INVALID_ARG; }

}  // extern "C"

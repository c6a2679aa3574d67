// Included by fheram.hip (same translation unit): fheram_bank — M RAMs of the same shape under ONE prepared key set, and Ram::read /
// read_prepare_write / write (ram.rs:172-294) on a SET of them as ONE operation, one address per member.  Ram objects are independent units
// (ram.rs:25-29; `&mut self` serialises per RAM only), so nothing orders operations on different RAMs.
//
// Storage: ONE internal context whose word count is M * ws.  Rows, arenas, tree, results, words and temporaries are laid out [M * ws][...],
// so ciphertext y = m * ws + w is word w of member m.  Per-member state (the state flag, what read_prepare_write kept for the write, where
// the last result is) lives here, one RamState per member.  After fheram_bank_create nothing here writes a field of the context.
//
// Every read_prepare_write and write — by range or by list — is one function over a MEMBER SET (MemberSet: entry k works on member
// m[k]) and the set's PLAN (SetPlan): path.hpp's read_impl / write_all on the plan's view and operand set, from the plan's RAM state, whose
// outcome set_assign hands back to every member.  There are two plans:
//   - IN PLACE, for a range (one member, or a contiguous ascending run [first, first + n)): the view is the context's buffers from the
//     range's first ciphertext (bank_view), a pointer offset plus gy = n * ws.  One member is the plain operation (one_addr), memo included;
//     more have their digits in the bank's tables with the identity map: every address-independent step is one launch over n * ws
//     ciphertexts, the products take the table where a table form exists and run member by member on the y-slice everywhere else.  The
//     state is the merge of the members': what read_prepare_write kept counts only when every member holds it.
//   - DENSE, for any other set of distinct members: the rows are the whole bank's, reached through the set's map (the table chains read
//     AND store them through it: k_read_chain_m / k_write_chain_m; launches without a table form go member by member, Opnds::rows); every
//     other buffer is the lists' own dense set `wl` (path.hpp dense_reserve) — not the read list's, so a read list between the two halves
//     destroys nothing.  read_prepare_write hands every entry's tree top and result over into the member's own slots, so ranges, single
//     calls and downloads see a prepared member like any other; a write gathers tree and trace(top) from those slots and scatters the tree
//     back.  The rows after the alone levels stay in wl.A: they count (kept_*) for a write of the same members in the same order while
//     every one of them still holds them (wl_holds) — then nothing is gathered either.
// A READ LIST (fheram_bank_read_list) is the general read: members in any order, with repeats, so it is not a plan of the above but
// path.hpp's read_many — the batch's function — with the set's map, on a dense set of its own (`list`) and a scratch state; every named
// member is then left as a read leaves it (set_assign), with the result of the last entry that named it in its slice of d_res.
// The write's inverse digits are never started early in a bank of more than one member (pre_inv shares d_prep_inv and d_tail_sync between
// members); a bank of ONE member is a plain context in every respect.  Bank operations are never captured into a hipGraph: under graph = 1
// they are enqueued directly, in the forms that mode selects.
// The bank's oblivious select (fheram_bank_select, fheram_bank_select_lanes and the write that takes its words from them) is select.hpp: it runs on buffers of its own
// (`sel`) and reads, of what is here, only where a member's result and the last outputs of each kind (LastOutputs) sit.
#pragma once
#include "path.hpp"

struct fheram_regs;   // a register file of the bank (regs.hpp)
struct fheram_table;  // a table of the bank (table.hpp)

// The kinds of operation whose outputs stay readable until the next of the kind: a select candidate may name them (FHERAM_SRC_*_RESULT)
// and a _result entry point downloads them.  One record per kind says how many there are and where they sit.
enum LastKind { LAST_LIST, LAST_SELECT, LAST_REGS, LAST_TABLE, LAST_PEEK, LAST_KINDS };
struct LastOutputs {
    int n = 0;        // outputs of the last operation of the kind; 0: none has run
    ResHome home;     // where they are: the kind's own buffer set, or the mix's (path.hpp)
};

struct fheram_bank {
    fheram_ctx* c = nullptr;      // word count M * mws; never row-sharded, never part of a group
    int M = 0, mws = 0;
    RamState ram[FHERAM_BANK_MAX];
    double* d_prep = nullptr;     // [n][n_digits] prepared GGSW: the digits of the k-th address of the set being read   (M > 1)
    double* d_prep_inv = nullptr; // [n][n_digits] the inverse digits of the k-th address of the set being written      (M > 1)
    DenseBufs list;               // fheram_bank_read_list: buffers of its own, sized by mws
    LastOutputs last[LAST_KINDS]; // the last read list, select, register read, table read and peek / poke (each set by whatever finishes one: the single calls, the mixes)
    DenseBufs wl;                 // the dense plan's buffers (read_prepare_write / write lists), sized by mws
    // what the last dense read_prepare_write left in wl.A (RamState::memo_alone of a list): for kept_n entries with the map kept_map ...
    int kept_alone = 0, kept_n = 0;
    unsigned kept_map = 0;
    bool wl_holds[FHERAM_BANK_MAX] = {};   // ... and member m is still as that operation left it (cleared by whatever touches the member)
    SelectBufs sel;               // fheram_bank_select: buffers of its own (select.hpp)
    SelectLaneTable lanes;        // fheram_bank_select_lanes: the pointer table of its pack (allocated on the first lanes call)
    int sel_fail_alloc = 0;       // the self-test's failing allocation, as wl_fail_alloc
    bool has_res[FHERAM_BANK_MAX] = {};  // member m has the result of a read / read_prepare_write in its slot (a select may take it as a candidate)
    int wl_fail_alloc = 0;        // fheram_bank_selftest_fail_list_alloc: the wl_fail_alloc-th next device allocation of wl fails (0: none)
    // the register files (regs.hpp): what they share, the live ones, and — beside the records above, with ONE result — where the last
    // fheram_bank_regs_read_prepare_write left its (the kept trace of regs_old_owner; nullptr: none has run)
    OneRowSet regs;
    std::vector<fheram_regs*> regfiles;
    const int32_t* regs_old = nullptr;
    const fheram_regs* regs_old_owner = nullptr;
    // the tables (table.hpp): what they share, the live ones
    OneRowSet tabs;
    std::vector<fheram_table*> tables;
    MixBufs mix;                  // fheram_bank_read_mix (mix.hpp)
    PublicBufs pub;               // the public side (public_io.hpp)
    int pub_fail_alloc = 0;       // fheram_bank_selftest_fail_public_alloc: the pub_fail_alloc-th next device allocation of pub fails (0: none)
};

namespace {

// regs.hpp: new keys void what every register file kept; a destroyed bank takes its register files' device buffers with it
void regs_keys_changed(fheram_bank* b);
void regs_bank_release(fheram_bank* b);
// table.hpp: a destroyed bank takes its tables' device buffers with it
void table_bank_release(fheram_bank* b);

static_assert(FHERAM_READ_LIST_MAX >= FHERAM_BANK_MAX && FHERAM_READ_LIST_MAX * 4 <= 32, "a member set has four bits of the map per entry");
// The members an operation works on, entry by entry: a range [first, first + n), or a list (checked by the caller).
struct MemberSet {
    int n = 0;
    int m[FHERAM_READ_LIST_MAX];
    static MemberSet range(int first, int n) { MemberSet s; s.n = n; for (int k = 0; k < n; k++) s.m[k] = first + k; return s; }
    static MemberSet list(const int* members, int n) { MemberSet s; s.n = n; for (int k = 0; k < n; k++) s.m[k] = members[k]; return s; }
    // one member, or a contiguous ascending run: the range [m[0], m[0] + n)
    bool is_range() const { for (int k = 1; k < n; k++) if (m[k] != m[0] + k) return false; return true; }
    unsigned map() const { unsigned v = 0; for (int k = 0; k < n; k++) v |= (unsigned)m[k] << (4 * k); return v; }   // Opnds::member_map
};

// The buffers as one operation on members [first, ...) sees them in place: each starts at the range's first ciphertext.
RamView bank_view(const fheram_bank* b, int first) {
    RamView v = ctx_view(b->c);
    const size_t o1 = (size_t)first * b->mws * fheram_ctx::GLWE, oR = o1 * b->c->rows;
    for (int32_t** p : {&v.rows, &v.A, &v.B, &v.C, &v.D}) *p += oR;
    for (int32_t** p : {&v.part, &v.tmp, &v.tmp2, &v.res, &v.tree, &v.w, &v.trtop}) *p += o1;
    return v;
}
// member m's [mws] slot of a per-ciphertext buffer of the context
GlweRef member_slot(const fheram_bank* b, int32_t* buf, int m) { return ref(buf + (size_t)m * b->mws * fheram_ctx::GLWE, (long)fheram_ctx::GLWE, 0); }

// ---- checks: the whole set before anything is enqueued.  Each form has its own front (null arguments, n, the members); all end here -------
int check_addrs(fheram_ctx* c, const fheram_addr* const* addrs, int n) {
    for (int k = 0; k < n; k++) {
        if (!addrs[k] || addrs[k]->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "address " + std::to_string(k) + " is null or does not belong to this bank (layout mismatch, ram.rs:404)");
        if (addrs[k]->empty) return fail(c, FHERAM_ERR_INVALID_ARG, "address " + std::to_string(k) + " is an empty address: fheram_bank_address_alloc without fheram_bank_address_derive");
    }
    return FHERAM_OK;
}
// the addresses (none: a result download), every member initialised, the keys, every member in the wanted state (0: read / read_prepare_write, 1: write, -1: any, keys or not)
int members_ready(fheram_bank* b, const MemberSet& s, const fheram_addr* const* addrs, int want_state) {
    fheram_ctx* c = b->c;
    if (addrs) { const int rc = check_addrs(c, addrs, s.n); if (rc != FHERAM_OK) return rc; }
    for (int k = 0; k < s.n; k++)
        if (!b->ram[s.m[k]].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (member " + std::to_string(s.m[k]) + ")");
    if (want_state < 0) return FHERAM_OK;
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int k = 0; k < s.n; k++) {
        if (want_state == 0 && b->ram[s.m[k]].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.read: internal state is true -> requires calling Memory.write (member " + std::to_string(s.m[k]) + ")");
        if (want_state == 1 && !b->ram[s.m[k]].state)
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.write: internal state is false -> requires calling Memory.read_prepare_write (member " + std::to_string(s.m[k]) + ")");
    }
    return FHERAM_OK;
}
// a range; null_args: what the entry point found missing (refused before the call counts for the mid re-arm: a range's always was)
int range_check(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, const char* null_args, int want_state, MemberSet* s) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (null_args) return fail(c, FHERAM_ERR_INVALID_ARG, null_args);
    mid_rearm(c);
    if (first < 0 || n < 1 || first > b->M - n)
        return fail(c, FHERAM_ERR_INVALID_ARG, "member range [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") is empty or outside the bank's " + std::to_string(b->M) + " members");
    *s = MemberSet::range(first, n);
    return members_ready(b, *s, addrs, want_state);
}
// a read list: any members, in any order, with repeats
int read_list_check(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, MemberSet* s) {
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
    *s = MemberSet::list(members, n);
    return members_ready(b, *s, addrs, 0);
}
// the members of a read_prepare_write / write list, behind the null arguments: n, each in range and named once, then what every set ends in
// (fheram_bank_read_prepare_write_mix checks its prepare list with this)
int write_list_members(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, int want_state, MemberSet* s) {
    fheram_ctx* c = b->c;
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
    *s = MemberSet::list(members, n);
    return members_ready(b, *s, addrs, want_state);
}
// a read_prepare_write (want_state 0) or write (1, which also has words) list: distinct members, in any order
int write_list_check(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, bool null_words, int want_state, MemberSet* s) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    if (!members || !addrs || null_words) return fail(c, FHERAM_ERR_INVALID_ARG, want_state ? "null member list, null address list or null words" : "null member list or null address list");
    return write_list_members(b, members, addrs, n, want_state, s);
}

// ---- the plan of a read_prepare_write / write on a member set (header comment) ----------------------------------------------------------
// The RAM state the operation starts from.  In place: the merge of the members'.  Dense: trace(top) when every member holds its own, the
// kept arena when it is this very set's and every member still holds it.
RamState set_state(const fheram_bank* b, const MemberSet& s, bool dense, bool write) {
    RamState st{true, write, true, dense ? 0 : b->ram[s.m[0]].memo_alone, false};
    bool holds = dense && write && b->kept_alone > 0 && b->kept_n == s.n && b->kept_map == s.map();
    for (int k = 0; k < s.n; k++) {
        const RamState& r = b->ram[s.m[k]];
        st.memo_top = st.memo_top && r.memo_top;
        if (!dense && r.memo_alone != st.memo_alone) st.memo_alone = 0;
        holds = holds && b->wl_holds[s.m[k]];
    }
    if (holds) st.memo_alone = b->kept_alone;
    return st;
}
struct SetPlan {
    const bool dense;   // (its buffers reserved by the caller)
    RamState st;
    const RamView v;
    const Opnds o;      // o.st points at st: a plan is built where it lives
    SetPlan(fheram_bank* b, const MemberSet& s, const fheram_addr* const* addrs, bool write)
        : dense(!s.is_range()), st(set_state(b, s, dense, write)), v(dense ? dense_view(b->c, b->wl) : bank_view(b, s.m[0])),
          o(s.n == 1 ? one_addr(b->c, addrs, b->mws, &st)
                     : table_opnds(b->c, &st, addrs, s.n, b->mws, b->d_prep, b->d_prep_inv, dense ? s.map() : MEMBER_MAP_IDENTITY, true)) {}
    SetPlan(const SetPlan&) = delete;
};
// what the operation left, for every member of the set; new_result: it was a read.  A member's memo_alone speaks of the context's arena, so
// a dense operation leaves 0 there and says in wl_holds whether the lists' arena holds the member's rows.
void set_assign(fheram_bank* b, const MemberSet& s, const RamState& st, bool dense, bool state, bool new_result) {
    for (int k = 0; k < s.n; k++) {
        RamState& r = b->ram[s.m[k]];
        r.state = state; r.memo_top = st.memo_top; r.memo_alone = dense ? 0 : st.memo_alone;
        if (new_result) { r.res_in_trtop = st.res_in_trtop; b->has_res[s.m[k]] = true; }
        b->wl_holds[s.m[k]] = dense && st.memo_alone > 0;
    }
}
// the results of the set's members, widened into h_res by the device; out: [n][mws][GLWE] int64.  In place: one run per stretch of members
// whose result sits in the same buffer; dense: one per entry.
int set_result(fheram_bank* b, const MemberSet& s, bool dense, int64_t* out) {
    fheram_ctx* c = b->c;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    ResRun runs[FHERAM_BANK_MAX];
    int n_runs = 0;
    for (int k = 0; k < s.n; k++) {
        const int32_t* src = (b->ram[s.m[k]].res_in_trtop ? c->d_trtop : c->d_res) + (size_t)s.m[k] * per;
        if (!dense && n_runs && runs[n_runs - 1].src + runs[n_runs - 1].n == src) runs[n_runs - 1].n += per;
        else runs[n_runs++] = ResRun{src, per};
    }
    return result_export(c, runs, n_runs, c->h_res, c->d_h_res, out);
}
// Ram::read / read_prepare_write on every member of a checked set as one operation
int bank_read_set(fheram_bank* b, const MemberSet& s, const fheram_addr* const* addrs, bool prepare_write, int64_t* out) {
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!s.is_range()) {
        const int rc = dense_reserve(c, b->wl, s.n, b->mws, true, &b->wl_fail_alloc);
        if (rc != FHERAM_OK) return rc;
        b->kept_alone = 0;   // arena A is this operation's from here on
    }
    SetPlan p(b, s, addrs, false);
    const int rc = read_impl(p.o, p.v, prepare_write);
    if (rc == FHERAM_OK && p.dense) {   // the hand-over: tree top and result into every member's own slots, where a range, a single call or a download looks for them
        const long G = (long)fheram_ctx::GLWE;
        for (int k = 0; k < s.n; k++) {
            if (c->n2 == 2) launch_copy(c, p.o.slice(ref(p.v.tree, G, 0), k), member_slot(b, c->d_tree, s.m[k]), 1, b->mws);
            launch_copy(c, p.o.slice(ref(p.st.res_in_trtop ? p.v.trtop : p.v.res, G, 0), k), member_slot(b, p.st.res_in_trtop ? c->d_trtop : c->d_res, s.m[k]), 1, b->mws);
        }
        b->kept_alone = p.st.memo_alone; b->kept_n = s.n; b->kept_map = p.o.member_map;
    }
    set_assign(b, s, p.st, p.dense, rc == FHERAM_OK && prepare_write, true);                // ram.rs:533
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipGetLastError());
    return out ? set_result(b, s, p.dense, out) : FHERAM_OK;
}
// Ram::write on every member of a checked set as one operation; stage(d_w, ciphertexts): path.hpp write_all
template <typename S>
int bank_write_set(fheram_bank* b, const MemberSet& s, const fheram_addr* const* addrs, S&& stage) {
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!s.is_range()) {
        const int rc = dense_reserve(c, b->wl, s.n, b->mws, true, &b->wl_fail_alloc);
        if (rc != FHERAM_OK) return rc;
    }
    SetPlan p(b, s, addrs, true);
    const long G = (long)fheram_ctx::GLWE;
    if (p.dense) {
        // The gather: every member's tree top and trace(top) into the dense buffers — unless this very set prepared the members and all
        // still hold it (the plan's state then resumes from the kept arena): then tree and trtop are what the hand-over copied FROM, nothing
        // has written them since, no launch is needed, and write_side_begin may skip its fork event after a host wait as a range's does
        // (main_idle).  With a gather the main stream has work again, so the side stage forks behind it: one event record.
        const bool holds = p.st.memo_alone > 0;
        b->kept_alone = 0;   // consumed, or overwritten by this write's trace(ct_hi)
        if (!holds) {
            main_enqueued(c);
            for (int k = 0; k < s.n; k++) {
                if (c->n2 == 2) launch_copy(c, member_slot(b, c->d_tree, s.m[k]), p.o.slice(ref(p.v.tree, G, 0), k), 1, b->mws);
                if (p.st.memo_top) launch_copy(c, member_slot(b, c->d_trtop, s.m[k]), p.o.slice(ref(p.v.trtop, G, 0), k), 1, b->mws);
            }
        }
    }
    const int rc = write_all(p.o, p.v, stage);   // (refused words: nothing of the members has been touched)
    if (rc == FHERAM_OK && p.dense && c->n2 == 2)   // the scatter: the tree's new top (ct_lo, rotated) back into every member's slot
        for (int k = 0; k < s.n; k++) launch_copy(c, p.o.slice(ref(p.v.tree, G, 0), k), member_slot(b, c->d_tree, s.m[k]), 1, b->mws);
    set_assign(b, s, p.st, p.dense, rc != FHERAM_OK, false);                                // ram.rs:648
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipGetLastError());
    return FHERAM_OK;
}
// ---- the last outputs of a kind: the words its messages use, and the one download --------------------------------------------------------
struct LastKindText {
    int src;                       // the FHERAM_SRC_* kind that names them
    const char *unit, *units;      // what one of them is called
    const char *last, *of_last;    // the operation: as a source names it, as its _result entry point does
    const char* none;              // "... on this bank": none has run
};
const LastKindText LAST_TEXT[LAST_KINDS] = {
    {FHERAM_SRC_LIST_RESULT, "entry", "entries", "read list", "list", "no read list has run"},
    {FHERAM_SRC_SELECT_RESULT, "output", "outputs", "select", "select", "no select has run"},
    {FHERAM_SRC_REGS_RESULT, "output", "outputs", "register read", "register read", "no fheram_bank_regs_read has run"},
    {FHERAM_SRC_TABLE_RESULT, "output", "outputs", "table read", "table read", "no fheram_bank_table_read has run"},
    {FHERAM_SRC_PEEK_RESULT, "output", "outputs", "peek", "peek", "no fheram_bank_peek or fheram_bank_poke has run"},
};
// outputs [first, first + n) of the last operation of the kind, behind the entry point's null-bank test
int last_result(fheram_bank* b, LastKind kind, int first, int n, int64_t* out) {
    fheram_ctx* c = b->c;
    const LastOutputs& L = b->last[kind];
    const LastKindText& t = LAST_TEXT[kind];
    if (!out) return fail(c, FHERAM_ERR_INVALID_ARG, "null output");
    if (!L.n) return fail(c, FHERAM_ERR_STATE, std::string(t.none) + " on this bank");
    if (first < 0 || n < 1 || first > L.n - n)
        return fail(c, FHERAM_ERR_INVALID_ARG, std::string(t.units) + " [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") are empty or outside the last " + t.of_last + "'s " + std::to_string(L.n) + " " + t.units);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    const ResRun run{L.home.res + (size_t)first * per, (size_t)n * per};
    return result_export(c, &run, 1, L.home.h, L.home.d_h, out);
}
void list_done(fheram_bank* b, int n) { b->last[LAST_LIST] = LastOutputs{n, ResHome{b->list.res, b->list.h_res, b->list.d_h_res, -1}}; }

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
    dense_free(b->list);
    dense_free(b->wl);
    select_free(b->sel);
    lane_table_free(b->lanes);
    regs_bank_release(b);
    table_bank_release(b);
    mix_bufs_free(b->mix);
    public_bufs_free(b->pub);
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
    regs_keys_changed(b);
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
int fheram_bank_address_derive_at(fheram_bank* b, const fheram_fheuint* const* fus, const int* first_bit, int n, int sign, fheram_addr* const* addrs) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_address_derive_at(b->c, fus, first_bit, n, sign, addrs);
}

int fheram_bank_read(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int64_t* out) {
    MemberSet s;
    const int rc = range_check(b, first, n, addrs, addrs ? nullptr : "null address list", 0, &s);
    return rc == FHERAM_OK ? bank_read_set(b, s, addrs, false, out) : rc;
}
int fheram_bank_read_prepare_write(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int64_t* out) {
    MemberSet s;
    const int rc = range_check(b, first, n, addrs, addrs ? nullptr : "null address list", 0, &s);
    return rc == FHERAM_OK ? bank_read_set(b, s, addrs, true, out) : rc;
}
int fheram_bank_write(fheram_bank* b, int first, int n, const int64_t* w, const fheram_addr* const* addrs) {
    MemberSet s;
    const int rc = range_check(b, first, n, addrs, (addrs && w) ? nullptr : "null address list or null words", 1, &s);
    return rc == FHERAM_OK ? bank_write_set(b, s, addrs, [&](int32_t* d_w, int n_ct) { return stage_words(b->c, d_w, w, n_ct); }) : rc;
}
int fheram_bank_result_download(fheram_bank* b, int first, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    MemberSet s;
    const int rc = range_check(b, first, n, nullptr, nullptr, -1, &s);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(b->c, hipSetDevice(b->c->device));
    return set_result(b, s, false, out);
}
// K = n independent Ram::read (ram.rs:172-191), entry k on member members[k], as one operation: path.hpp read_many with the members as the
// source map, on the list's own buffers and a scratch RamState.  What the sequence of those K single-member reads leaves: every named member
// in state 0 with nothing kept for a write, the result of the last entry that named it where its own read would have left it (its slice of
// d_res); every other member as it was.  A bank of one member has one source: the list is what fheram_read_batch runs.
int fheram_bank_read_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, int64_t* out) {
    MemberSet s;
    int rc = read_list_check(b, members, addrs, n, &s);
    if (rc != FHERAM_OK) return rc;
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    const long G = (long)fheram_ctx::GLWE;
    b->last[LAST_LIST].n = 0;   // until this list is enqueued there is no last list: several entries overwrite res as they run (one entry only with its closing copy, but the rule is one)
    if (n == 1) {   // the plain single-member read; its result is also the list's
        rc = dense_reserve(c, b->list, 1, b->mws);
        if (rc == FHERAM_OK) rc = bank_read_set(b, s, addrs, false, nullptr);
        if (rc != FHERAM_OK) return rc;
        launch_copy(c, member_slot(b, c->d_res, s.m[0]), ref(b->list.res, G, 0), 1, b->mws);
        list_done(b, 1);
        HIPCHK(c, hipGetLastError());
        return out ? last_result(b, LAST_LIST, 0, 1, out) : FHERAM_OK;
    }
    RamState st{true, false, false, 0, false};
    return read_many(c, b->list, &st, addrs, n, b->mws, s.map(), b->M > 1, out, [&](const Opnds& o) {
        set_assign(b, s, st, false, false, true);   // every named member: as a read leaves it
        for (int m = 0; m < b->M; m++) {
            int last = -1;
            for (int k = 0; k < n; k++) if (s.m[k] == m) last = k;
            if (last >= 0) launch_copy(c, o.slice(ref(b->list.res, G, 0), last), member_slot(b, c->d_res, m), 1, b->mws);
        }
        list_done(b, n);
    });
}
// n independent Ram::read_prepare_write (ram.rs:196-222), entry k on member members[k], as one operation (header comment)
int fheram_bank_read_prepare_write_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, int64_t* out) {
    MemberSet s;
    const int rc = write_list_check(b, members, addrs, n, false, 0, &s);
    return rc == FHERAM_OK ? bank_read_set(b, s, addrs, true, out) : rc;
}
// n independent Ram::write (ram.rs:226-294), entry k of w to member members[k], as one operation (header comment)
int fheram_bank_write_list(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, const int64_t* w) {
    MemberSet s;
    const int rc = write_list_check(b, members, addrs, n, !w, 1, &s);
    return rc == FHERAM_OK ? bank_write_set(b, s, addrs, [&](int32_t* d_w, int n_ct) { return stage_words(b->c, d_w, w, n_ct); }) : rc;
}
int fheram_bank_selftest_fail_list_alloc(fheram_bank* b, int nth) {
    if (!b || nth < 0) return FHERAM_ERR_INVALID_ARG;
    b->wl_fail_alloc = nth;
    return FHERAM_OK;
}
int fheram_bank_read_list_result(fheram_bank* b, int first, int n, int64_t* out) {
    return b ? last_result(b, LAST_LIST, first, n, out) : FHERAM_ERR_INVALID_ARG;
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

// Included by fheram.hip (same translation unit): the oblivious select of a bank — pick one of m candidate words by an ENCRYPTED index,
// on the device, and a write that takes its words from there.
//
// What is restated is the selection step the reference's select_store (store.rs:40-67) and select_rd (arithmetic.rs:212-231) share: "blind-
// rotate a packed ciphertext by an encrypted index, then trace".  CONTRACT-COMPATIBLE ONLY, as fheram_address_derive is:
// their callers (the BDD circuits, splice_u8 / splice_u16) are un-vendored and stay out of scope.  In this project's own arithmetic that step
// is Ram::read on a ONE-ROW RAM (ram.rs:451,457, the rows == 1 path) of max_addr = 2^bits: the row packs candidate j at coefficient j,
// the address is the index.  So:
//   selector   the Address of such a RAM: the digits get_base_2d(2^bits) gives over the bank's DECOMP_N (one coordinate), each the GGSW of
//              X^-v (Address::encrypt_sk's sign) in the layout of address digits; created from host digits or derived from bits
//              [first_bit, first_bit + bits) of an encrypted integer by k_cmux_chain with that plan (one launch per distinct (first_bit, bits))
//              A FIELD selector (the _fields entry points) takes its plan from the caller's widths instead: digit d from an integer and a bit
//              position of its own, one k_cmux_chain launch per field (the store merge indexes by op + 4 * offset: DESIGN.md 15)
//   pack       k_select_pack (select_pack.hip): one launch per call over n * ws output ciphertexts; fheram_bank_select_lanes: k_select_pack_lanes
//              (select_lanes.hip), every candidate assembled lane by lane through a pointer table in device memory
//   chain      the prepared selector digits (k_prepare), the products and the trace: what read_top enqueues for the second coordinate
//              of a RAM of n * ws ciphertexts with a per-ciphertext operand table — the same launchers, so the same forms under every
//              configuration (chain_form), `safe`, tail = 0 and fuse = 0 included
// Everything runs on the bank's main stream and on buffers of the select's own (path.hpp SelectBufs): no member's rows, state flag, tree,
// result or kept memo is touched, the last read list's results stay readable, and a member between read_prepare_write and write resumes
// its write exactly as before.
#pragma once
#include "bank.hpp"
#include "select_pack.hpp"
#include "select_lanes.hpp"

struct fheram_selector {
    fheram_bank* bank;   // owner (identity check only after creation)
    int device, bits, n_digits;
    int32_t* d_ggsw;     // [n_digits] std-form GGSW, int32 (the layout of address digits)
    unsigned char rsh[FHERAM_SELECT_BITS_MAX], width[FHERAM_SELECT_BITS_MAX], lsh[FHERAM_SELECT_BITS_MAX];   // the digit plan (conversion.rs:45-62)
    bool empty;          // fheram_bank_selector_alloc: no digits yet
    bool fields;         // made by a _fields call: the plan is the caller's widths, digit d derived from an integer and a bit offset of its own
};

namespace {

static_assert(FHERAM_SELECT_MAX == SELECT_K_MAX && (1 << FHERAM_SELECT_BITS_MAX) == SELECT_CAND_MAX, "the argument struct of k_select_pack holds FHERAM_SELECT_MAX selects of 2^FHERAM_SELECT_BITS_MAX candidates");
static_assert(FHERAM_SELECT_MAX <= DERIVE_K_MAX && FHERAM_SELECT_BITS_MAX <= DERIVE_DIGITS_MAX, "a selector derivation is one k_cmux_chain launch");
static_assert(SELECT_LANES_SLICES == EW_SLICES && SELECT_LANES_CT_MAX == 64, "k_select_pack_lanes covers a ciphertext as the elementwise kernels do; a call has at most 64 output ciphertexts");
static_assert(FHERAM_SELECT_FIELDS_MAX == FHERAM_SELECT_BITS_MAX, "a field has at least one bit");

static_assert(FHERAM_SELECTOR_WIDE_DIGITS_MAX == FHERAM_SELECT_BITS_MAX && FHERAM_SELECTOR_WIDE_DIGITS_MAX == FHERAM_SELECT_FIELDS_MAX, "a selector's plan arrays hold FHERAM_SELECTOR_WIDE_DIGITS_MAX digits, a wide selector's too");
static_assert(FHERAM_TABLE_BITS_MAX == LOGN && FHERAM_SELECTOR_WIDE_DIGITS_MAX <= DERIVE_DIGITS_MAX, "a row holds N words; a wide selector's derivation is one k_cmux_chain launch");

// what both forms of a new selector end in: the handle with its plan — digit d has widths[d] bits at bit offset sum(widths[0..d)); one
// coordinate: bit_lsh and bit_rsh advance together — and its device buffer, no digits yet
int selector_alloc(fheram_bank* b, int bits, const int* widths, int n_digits, bool fields, fheram_selector** out) {
    fheram_ctx* c = b->c;
    HIPCHK(c, hipSetDevice(c->device));
    fheram_selector* s = new fheram_selector{b, c->device, bits, n_digits, nullptr, {}, {}, {}, true, fields};
    unsigned at = 0;
    for (int d = 0; d < n_digits; d++) {
        s->rsh[d] = s->lsh[d] = (unsigned char)at; s->width[d] = (unsigned char)widths[d];
        at += (unsigned)widths[d];
    }
    const hipError_t e = hipMalloc(&s->d_ggsw, (size_t)n_digits * fheram_ctx::GGSW * sizeof(int32_t));
    if (e != hipSuccess) { delete s; return reserve_failed(c, e, "hipMalloc"); }
    *out = s;
    return FHERAM_OK;
}
// the selector of `bits` bits, its plan the bank's DECOMP_N's.  bits_max: FHERAM_SELECT_BITS_MAX, or FHERAM_TABLE_BITS_MAX
// for a WIDE selector (table.hpp: the address of a table), whose plan may then be longer than the plan arrays
int selector_new(fheram_bank* b, int bits, fheram_selector** out, int bits_max = FHERAM_SELECT_BITS_MAX, const char* max_name = "FHERAM_SELECT_BITS_MAX") {
    fheram_ctx* c = b->c;
    if (bits < 1 || bits > bits_max)
        return fail(c, FHERAM_ERR_INVALID_ARG, "bits = " + std::to_string(bits) + " is outside [1, " + max_name + " = " + std::to_string(bits_max) + "]");
    const std::vector<std::vector<int>> plan = base_2d((uint64_t)1 << bits, c->p);
    if (plan.size() != 1)
        return fail(c, FHERAM_ERR_UNSUPPORTED, "the bank's DECOMP_N gives a selector of " + std::to_string(bits) + " bits " + std::to_string(plan.size()) + " coordinates; a select is a read of a one-row RAM of one coordinate");
    if ((int)plan[0].size() > FHERAM_SELECTOR_WIDE_DIGITS_MAX)
        return fail(c, FHERAM_ERR_UNSUPPORTED, "the bank's DECOMP_N gives a selector of " + std::to_string(bits) + " bits " + std::to_string(plan[0].size()) + " digits, more than FHERAM_SELECTOR_WIDE_DIGITS_MAX = " + std::to_string(FHERAM_SELECTOR_WIDE_DIGITS_MAX));
    return selector_alloc(b, bits, plan[0].data(), (int)plan[0].size(), false, out);
}

// The selector whose digit d has widths[d] bits at bit offset sum(widths[0..d)): the Address of a one-row RAM of max_addr = 2^bits whose DECOMP_N
// starts with `widths` (get_base_2d then gives [widths]), whatever the bank's own DECOMP_N is.  The plan comes from the caller, not from base_2d.
int selector_new_fields(fheram_bank* b, const int* widths, int n_fields, fheram_selector** out, int bits_max = FHERAM_SELECT_BITS_MAX, const char* max_name = "FHERAM_SELECT_BITS_MAX") {
    fheram_ctx* c = b->c;
    if (!widths) return fail(c, FHERAM_ERR_INVALID_ARG, "null widths");
    if (n_fields < 1 || n_fields > FHERAM_SELECT_FIELDS_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n_fields = " + std::to_string(n_fields) + " is outside [1, FHERAM_SELECT_FIELDS_MAX = " + std::to_string(FHERAM_SELECT_FIELDS_MAX) + "]");
    int bits = 0;
    for (int d = 0; d < n_fields; d++) {
        if (widths[d] < 1) return fail(c, FHERAM_ERR_INVALID_ARG, "field " + std::to_string(d) + " has the width " + std::to_string(widths[d]) + ", below 1");
        bits += widths[d];
        if (bits > bits_max)
            return fail(c, FHERAM_ERR_INVALID_ARG, std::string("the widths sum to more than ") + max_name + " = " + std::to_string(bits_max) + " bits");
    }
    return selector_alloc(b, bits, widths, n_fields, true, out);
}
// The second half of every _create entry point: the output and the digits there at all ...
int selector_create_args(fheram_bank* b, const int64_t* const* ggsw, fheram_selector** out) {
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    if (!ggsw) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null ggsw");
    return FHERAM_OK;
}
// ... and the new selector s filled with them (wrong_count: what to say when there are not as many as its plan has); a failure destroys s
int selector_fill(fheram_bank* b, fheram_selector* s, const int64_t* const* ggsw, int n_ggsw, const std::string& wrong_count, fheram_selector** out) {
    fheram_ctx* c = b->c;
    int rc = n_ggsw != s->n_digits ? fail(c, FHERAM_ERR_INVALID_ARG, wrong_count) : (int)FHERAM_OK;
    for (int i = 0; i < n_ggsw && rc == FHERAM_OK; i++)
        rc = ggsw[i] ? upload_i64(c, s->d_ggsw + (size_t)i * fheram_ctx::GGSW, ggsw[i], fheram_ctx::GGSW) : fail(c, FHERAM_ERR_INVALID_ARG, "null ggsw digit");
    if (rc != FHERAM_OK) { fheram_selector_destroy(s); return rc; }
    s->empty = false;
    *out = s;
    return FHERAM_OK;
}
// a selector an operation takes: the bank's, and with digits (alloc_name: the entry point that made it empty)
int selector_check(fheram_bank* b, const fheram_selector* s, const std::string& who, const char* alloc_name = "fheram_bank_selector_alloc") {
    if (!s || s->bank != b) return fail(b->c, FHERAM_ERR_INVALID_ARG, who + " is null or belongs to another bank");
    if (s->empty) return fail(b->c, FHERAM_ERR_INVALID_ARG, who + " is empty: " + alloc_name + " without fheram_bank_selector_derive");
    return FHERAM_OK;
}

// Grows the select's buffers to n_ct output ciphertexts, n_prep prepared digits and n_host ciphertexts of host candidates.  The new set is
// complete before the old one goes, and the last select's results move over: a failure leaves the bank as it was (FHERAM_ERR_DEVICE, and every
// other operation — a smaller select too — still works).
int select_reserve(fheram_bank* b, int n_ct, int n_prep, int n_host) {
    fheram_ctx* c = b->c;
    SelectBufs& S = b->sel;
    if (n_ct <= S.cap && n_prep <= S.prep_cap && n_host <= S.host_cap) return FHERAM_OK;
    SelectBufs nw;
    nw.cap = std::max(n_ct, S.cap); nw.prep_cap = std::max(n_prep, S.prep_cap); nw.host_cap = std::max(n_host, S.host_cap);
    const size_t ct = (size_t)nw.cap * fheram_ctx::GLWE * sizeof(int32_t);
    hipError_t e = hipSuccess;
    auto dev = [&](auto** p, size_t bytes) {
        if (e != hipSuccess) return;
        if (b->sel_fail_alloc > 0 && --b->sel_fail_alloc == 0) e = hipErrorOutOfMemory;   // (as the runtime reports an exhausted device)
        else e = hipMalloc((void**)p, bytes);
    };
    for (int32_t** p : {&nw.packed, &nw.ep, &nw.tmp, &nw.tmp2, &nw.res}) dev(p, ct);
    dev(&nw.prep, (size_t)nw.prep_cap * fheram_ctx::GGSW * sizeof(double));
    if (nw.host_cap) dev(&nw.host.d, (size_t)nw.host_cap * fheram_ctx::GLWE * sizeof(int32_t));
    if (e == hipSuccess) e = pinned_result(&nw.h_res, &nw.d_h_res, ct);
    if (e == hipSuccess && nw.host_cap) e = nw.host.pin((size_t)nw.host_cap * fheram_ctx::GLWE * sizeof(int32_t));
    if (e == hipSuccess) e = nw.host.event();
    LastOutputs& last = b->last[LAST_SELECT];
    if (e == hipSuccess && last.n) e = hipMemcpyAsync(nw.res, S.res, (size_t)last.n * b->mws * fheram_ctx::GLWE * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && S.cap) e = hipStreamSynchronize(c->stream);   // whatever still reads or writes the old set
    if (e != hipSuccess) { select_free(nw); return reserve_failed(c, e, "buffers of a select of " + std::to_string(n_ct) + " ciphertexts"); }
    select_free(S);
    S = nw;
    last.home = ResHome{S.res, S.h_res, S.d_h_res, -1};   // the last select's outputs have moved
    return FHERAM_OK;
}

// the kind of last outputs a source kind names (-1: none of them)
int last_kind_of(int src_kind) {
    for (int k = 0; k < LAST_KINDS; k++) if (LAST_TEXT[k].src == src_kind) return k;
    return -1;
}
// where candidate (kind, index) sits on the device: ws GLWEs (nullptr: ZERO); d_host: the staged host words (a select's own; a register
// file's pack and write and a poke stage theirs in their own sets)
const int32_t* select_source(const fheram_bank* b, const fheram_select_src& s, const int32_t* d_host) {
    const fheram_ctx* c = b->c;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    const int last = last_kind_of(s.kind);
    if (last >= 0) return b->last[last].home.res + (size_t)s.index * per;   // (the kind's own buffers, or the last mix's: path.hpp ResHome)
    switch (s.kind) {
    case FHERAM_SRC_HOST: return d_host + (size_t)s.index * per;
    case FHERAM_SRC_MEMBER_RESULT: return (b->ram[s.index].res_in_trtop ? c->d_trtop : c->d_res) + (size_t)s.index * per;   // (as set_result)
    case FHERAM_SRC_REGS_OLD: return b->regs_old;
    default: return nullptr;
    }
}
const int32_t* select_source(const fheram_bank* b, const fheram_select_src& s) { return select_source(b, s, b->sel.host.dev<int32_t>()); }

// GLWE `lane` of that word: what one entry of k_select_pack_lanes' table points to
const int32_t* select_source_lane(const fheram_bank* b, const fheram_select_lane& l) {
    const int32_t* p = select_source(b, fheram_select_src{l.kind, l.index});
    return p ? p + (size_t)l.lane * fheram_ctx::GLWE : nullptr;
}

// ---- what fheram_bank_select and fheram_bank_select_lanes share: the checks (every one before anything is enqueued) and everything behind the pack
int select_check_sels(fheram_bank* b, const fheram_selector* const* sels, const int* n_cand, int n, int* total) {
    fheram_ctx* c = b->c;
    if (n < 1 || n > FHERAM_SELECT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_SELECT_MAX = " + std::to_string(FHERAM_SELECT_MAX) + "]");
    const int Y = n * b->mws;
    if (Y > 64)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n * word_size = " + std::to_string(Y) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    *total = 0;
    for (int k = 0; k < n; k++) {
        const int rc = selector_check(b, sels[k], "selector " + std::to_string(k));
        if (rc != FHERAM_OK) return rc;
        if (sels[k]->bits > FHERAM_SELECT_BITS_MAX)   // a wide selector (table.hpp): the pack holds 2^FHERAM_SELECT_BITS_MAX candidates
            return fail(c, FHERAM_ERR_INVALID_ARG, "selector " + std::to_string(k) + " has " + std::to_string(sels[k]->bits) + " bits, more than FHERAM_SELECT_BITS_MAX = " + std::to_string(FHERAM_SELECT_BITS_MAX) + ": a wide selector addresses a table (fheram_bank_table_read)");
        if (sels[k]->bits != sels[0]->bits)
            return fail(c, FHERAM_ERR_INVALID_ARG, "selector " + std::to_string(k) + " has " + std::to_string(sels[k]->bits) + " bits, selector 0 " + std::to_string(sels[0]->bits) + ": the selects of one call share one digit count (the operand table's)");
        if (sels[k]->n_digits != sels[0]->n_digits)   // (field selectors: the same bits in another number of digits)
            return fail(c, FHERAM_ERR_INVALID_ARG, "selector " + std::to_string(k) + " has " + std::to_string(sels[k]->n_digits) + " digits, selector 0 " + std::to_string(sels[0]->n_digits) + ": the operand table of one call has one stride");
        if (n_cand[k] < 1 || n_cand[k] > (1 << sels[k]->bits))
            return fail(c, FHERAM_ERR_INVALID_ARG, "select " + std::to_string(k) + " has " + std::to_string(n_cand[k]) + " candidates, outside [1, 2^bits = " + std::to_string(1 << sels[k]->bits) + "]");
        *total += n_cand[k];
    }
    return FHERAM_OK;
}
// one (kind, index) of a source or a lane; need: bit k for the last outputs of kind k, bit LAST_KINDS for the last register read_prepare_write
constexpr unsigned NEED_REGS_OLD = 1u << LAST_KINDS;
int select_check_source(fheram_bank* b, int kind, int index, const std::string& who, const int64_t* host_words, unsigned& need) {
    fheram_ctx* c = b->c;
    const int last = last_kind_of(kind);
    if (last >= 0) {
        const int n = b->last[last].n;
        const LastKindText& t = LAST_TEXT[last];
        if (index < 0 || (n && index >= n)) return fail(c, FHERAM_ERR_INVALID_ARG, who + " names " + t.unit + " " + std::to_string(index) + ", outside the last " + t.last + "'s " + std::to_string(n) + " " + t.units);
        need |= 1u << last;
        return FHERAM_OK;
    }
    switch (kind) {
    case FHERAM_SRC_ZERO: break;
    case FHERAM_SRC_HOST:
        if (!host_words) return fail(c, FHERAM_ERR_INVALID_ARG, who + " is a host word and host_words is null");
        if (index < 0 || index >= FHERAM_SELECT_MAX * (1 << FHERAM_SELECT_BITS_MAX)) return fail(c, FHERAM_ERR_INVALID_ARG, who + " names host slot " + std::to_string(index) + ", outside [0, " + std::to_string(FHERAM_SELECT_MAX * (1 << FHERAM_SELECT_BITS_MAX)) + ")");
        break;
    case FHERAM_SRC_MEMBER_RESULT:
        if (index < 0 || index >= b->M) return fail(c, FHERAM_ERR_INVALID_ARG, who + " names member " + std::to_string(index) + ", outside the bank's " + std::to_string(b->M) + " members");
        break;
    case FHERAM_SRC_REGS_OLD:
        if (index != 0) return fail(c, FHERAM_ERR_INVALID_ARG, who + " names index " + std::to_string(index) + " of the last register read_prepare_write, which has one result: index 0");
        need |= NEED_REGS_OLD;
        break;
    default: return fail(c, FHERAM_ERR_INVALID_ARG, who + " has the unknown kind " + std::to_string(kind));
    }
    return FHERAM_OK;
}
// the keys, and every kind a source named has run (in the order the kinds were added: list, select, regs, regs-old, table, peek)
int select_check_state(fheram_bank* b, unsigned need, bool keys = true) {
    fheram_ctx* c = b->c;
    if (keys && !c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int k = 0; k < LAST_KINDS; k++) {
        if (k == LAST_TABLE && (need & NEED_REGS_OLD) && !b->regs_old)
            return fail(c, FHERAM_ERR_STATE, "a source names the last register read_prepare_write and none has run on this bank (or its register file is gone)");
        if ((need >> k & 1u) && !b->last[k].n) return fail(c, FHERAM_ERR_STATE, std::string("a source names the last ") + LAST_TEXT[k].last + " and " + LAST_TEXT[k].none + " on this bank");
    }
    return FHERAM_OK;
}
// The sources of a select, a register file's pack or write, a poke: kind and index of each, the caller's own limit on host slots
// (slot_limit; 0: the select's, which select_check_source has applied), what a kind needs to have run, a member's result.
// n_host: slots [0, n_host) cover every slot named.
int sources_check(fheram_bank* b, const fheram_select_src* srcs, int n, const int64_t* host_words, int slot_limit, const char* limit_text, bool keys, int* n_host) {
    fheram_ctx* c = b->c;
    unsigned need = 0;
    *n_host = 0;
    for (int i = 0; i < n; i++) {
        const std::string who = "source " + std::to_string(i);
        const int rc = select_check_source(b, srcs[i].kind, srcs[i].index, who, host_words, need);
        if (rc != FHERAM_OK) return rc;
        if (srcs[i].kind != FHERAM_SRC_HOST) continue;
        if (slot_limit && srcs[i].index >= slot_limit)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " names host slot " + std::to_string(srcs[i].index) + ", outside the [0, " + std::to_string(slot_limit) + ") " + limit_text);
        *n_host = std::max(*n_host, srcs[i].index + 1);
    }
    const int rc = select_check_state(b, need, keys);
    if (rc != FHERAM_OK) return rc;
    for (int i = 0; i < n; i++)
        if (srcs[i].kind == FHERAM_SRC_MEMBER_RESULT && !b->has_res[srcs[i].index])
            return fail(c, FHERAM_ERR_STATE, "source " + std::to_string(i) + " names the result of member " + std::to_string(srcs[i].index) + ", which has none yet");
    return FHERAM_OK;
}
// the host slots the sources name, whole words: range-checked as write words are into the stage's pinned twin (a refusal comes before
// anything is enqueued) ...
int host_words_stage(fheram_bank* b, HostStage& st, const fheram_select_src* srcs, int n, int n_host, const int64_t* host_words) {
    fheram_ctx* c = b->c;
    if (!n_host) return FHERAM_OK;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    const int rc = stage_wait(c, st);
    if (rc != FHERAM_OK) return rc;
    std::vector<char> staged((size_t)n_host, 0);
    for (int i = 0; i < n; i++) {
        if (srcs[i].kind != FHERAM_SRC_HOST || staged[(size_t)srcs[i].index]) continue;
        staged[(size_t)srcs[i].index] = 1;
        if (!narrow(host_words + (size_t)srcs[i].index * per, st.host<int32_t>() + (size_t)srcs[i].index * per, per))
            return fail(c, FHERAM_ERR_RANGE, "limb out of the normalised range [-2^16, 2^16]");
    }
    return FHERAM_OK;
}
// ... and copied to the device on the bank's stream, slot by slot
int host_words_copy(fheram_bank* b, HostStage& st, const fheram_select_src* srcs, int n, int n_host) {
    fheram_ctx* c = b->c;
    if (!n_host) return FHERAM_OK;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    for (int sl = 0; sl < n_host; sl++) {
        bool used = false;
        for (int i = 0; i < n && !used; i++) used = srcs[i].kind == FHERAM_SRC_HOST && srcs[i].index == sl;
        if (used) HIPCHK(c, hipMemcpyAsync(st.dev<int32_t>() + (size_t)sl * per, st.host<int32_t>() + (size_t)sl * per, per * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    return stage_record(c, st);
}
// n independent Ram::read of one-row RAMs as one operation, on the caller's buffers (S.packed holds the n * ws rows): the selectors' digits
// prepared, the products, the trace.  A select's chain (its packed candidates) and a register file's read (the fanned-out row, regs.hpp).
struct OneRowBufs { int32_t *packed, *ep, *tmp, *res; double* prep; };
void one_row_reads(fheram_bank* b, const OneRowBufs& S, const fheram_selector* const* sels, int n) {
    fheram_ctx* c = b->c;
    const int ws = b->mws, Y = n * ws, d = sels[0]->n_digits;
    const long G = (long)fheram_ctx::GLWE;
    // the selectors' digits, prepared: select k's at k * stride (CoordinatePrepared::prepare, coordinate_prepared.rs:104-116)
    const long stride = (long)d * (long)fheram_ctx::GGSW;
    for (int k = 0; k < n; k++) launch_prepare(c, sels[k]->d_ggsw, S.prep + k * stride, d * (int)(fheram_ctx::GGSW / N));
    // Ram::read of the one-row RAM {packed} (ram.rs:451,457): the products with the digits in order, then trace(0, log N) — as read_top runs
    // the second coordinate's products and the final trace of n * ws ciphertexts
    const GlweRef packed = ref(S.packed, G, 0), ep = ref(S.ep, G, 0), tmp = ref(S.tmp, G, 0), res = ref(S.res, G, 0);
    const OpndTable table = n == 1 ? OpndTable{} : OpndTable{ws, stride, MEMBER_MAP_IDENTITY, false};
    auto slice = [&](GlweRef r, int k) { r.p += (long)k * ws * r.sy; return r; };
    auto products = [&] { for (int k = 0; k < n; k++) ep_chain(c, slice(packed, k), slice(ep, k), slice(tmp, k), S.prep + k * stride, d, 1, ws); };
    const bool fuse_ep = c->cfg.tail_ep && d >= 2 && d <= TAIL_EP_MAX && chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail;
    GlweRef tb[2];
    if (fuse_ep && chain_bufs(LOGN, ep, res, tmp, tb))
        launch_trace_tail(c, packed, tb, 0, LOGN, 1, Y, S.prep, d, ep, false, table);
    else {
        products();
        trace_steps(c, ep, res, tmp, 0, LOGN, 1, Y);
    }
}
// Behind the pack (S.packed holds n * ws packed rows): that chain, the export
int select_chain(fheram_bank* b, const fheram_selector* const* sels, int n, int64_t* out) {
    fheram_ctx* c = b->c;
    SelectBufs& S = b->sel;
    const int Y = n * b->mws;
    one_row_reads(b, OneRowBufs{S.packed, S.ep, S.tmp, S.res, S.prep}, sels, n);
    HIPCHK(c, hipGetLastError());
    b->last[LAST_SELECT].n = n;   // (in S.res: select_reserve keeps the record's home)
    if (!out) return FHERAM_OK;
    const ResRun run{S.res, (size_t)Y * fheram_ctx::GLWE};
    return result_export(c, &run, 1, S.h_res, S.d_h_res, out);
}
// the pointer table of the lanes pack: allocated whole on the first lanes call.  The self-test's failing allocation (fheram_bank_selftest_fail_select_alloc)
// reaches the table's device allocation as the one AFTER those select_reserve makes in the same call.
int lane_table_reserve(fheram_bank* b) {
    fheram_ctx* c = b->c;
    SelectLaneTable& L = b->lanes;
    if (L.d) return FHERAM_OK;
    SelectLaneTable nw;
    const size_t bytes = (size_t)SELECT_LANES_CT_MAX * SELECT_CAND_MAX * sizeof(const int32_t*);
    hipError_t e;
    if (b->sel_fail_alloc > 0 && --b->sel_fail_alloc == 0) e = hipErrorOutOfMemory;
    else e = hipMalloc((void**)&nw.d, bytes);
    if (e == hipSuccess) e = nw.pin(bytes);
    if (e == hipSuccess) e = nw.event();
    if (e != hipSuccess) { lane_table_free(nw); return reserve_failed(c, e, "pointer table of a lanes select"); }
    L = nw;
    return FHERAM_OK;
}

}  // namespace

extern "C" {

int fheram_bank_selector_alloc(fheram_bank* b, int bits, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    return selector_new(b, bits, out);
}
int fheram_bank_selector_create(fheram_bank* b, const int64_t* const* ggsw, int n_ggsw, int bits, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_selector* s = nullptr;
    int rc = selector_create_args(b, ggsw, out);
    if (rc == FHERAM_OK) rc = selector_new(b, bits, &s);
    if (rc != FHERAM_OK) return rc;
    return selector_fill(b, s, ggsw, n_ggsw, "a selector of " + std::to_string(bits) + " bits has " + std::to_string(s->n_digits) + " digits, not " + std::to_string(n_ggsw), out);
}
int fheram_bank_selector_alloc_fields(fheram_bank* b, const int* widths, int n_fields, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    return selector_new_fields(b, widths, n_fields, out);
}
int fheram_bank_selector_create_fields(fheram_bank* b, const int64_t* const* ggsw, int n_ggsw, const int* widths, int n_fields, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_selector* s = nullptr;
    int rc = selector_create_args(b, ggsw, out);
    if (rc == FHERAM_OK) rc = selector_new_fields(b, widths, n_fields, &s);
    if (rc != FHERAM_OK) return rc;
    return selector_fill(b, s, ggsw, n_ggsw, "a selector of " + std::to_string(n_fields) + " fields has as many digits, not " + std::to_string(n_ggsw), out);
}
// digit d of sel <- bits [first_bit[d], first_bit[d] + widths[d]) of fus[d], in place: the unchanged k_cmux_chain, ONE LAUNCH PER FIELD of grid
// (6, 1, 1) with `out` advanced to the digit and the plan's entry 0 set to the field's (the argument struct holds one plan for all its integers, and
// fields never share an lsh).  No allocation, no host wait; ordered by the bank's main stream as fheram_bank_selector_derive is.
int fheram_bank_selector_derive_fields(fheram_bank* b, fheram_selector* sel, const fheram_fheuint* const* fus, const int* first_bit) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!sel || !fus || !first_bit) return fail(c, FHERAM_ERR_INVALID_ARG, "null selector, integer list or bit list");
    if (sel->bank != b) return fail(c, FHERAM_ERR_INVALID_ARG, "the selector belongs to another bank");
    if (!sel->fields) return fail(c, FHERAM_ERR_INVALID_ARG, "the selector was not made by fheram_bank_selector_alloc_fields / _create_fields");
    for (int d = 0; d < sel->n_digits; d++) {   // every check before anything is enqueued: a refused call changes no digit
        if (!fus[d] || fus[d]->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "integer " + std::to_string(d) + " is null or belongs to another bank");
        if (first_bit[d] < 0 || first_bit[d] + sel->width[d] > fus[d]->n_bits)
            return fail(c, FHERAM_ERR_INVALID_ARG, "bits [" + std::to_string(first_bit[d]) + ", " + std::to_string(first_bit[d]) + " + " + std::to_string(sel->width[d]) + ") of integer " + std::to_string(d) + " are beyond its " + std::to_string(fus[d]->n_bits) + " bits");
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->cur = c->stream;
    main_enqueued(c);
    const int rows = fheram_ctx::DNUM_CT * 2;
    for (int d = 0; d < sel->n_digits; d++) {
        CmuxChainArgs ca{};
        ca.tw = c->d_tw;
        ca.sign = 0;   // X^-v: what Ram::read accepts (address.rs:102-108)
        ca.fu[0] = fus[d]->d_prep;
        ca.out[0] = sel->d_ggsw + (size_t)d * fheram_ctx::GGSW;
        ca.first[0] = (unsigned char)first_bit[d]; ca.bits[0] = sel->width[d]; ca.lsh[0] = sel->lsh[d];
        ProfScope ps(c, "derive", (uint64_t)rows);
        cmux_chain_launch(dim3(rows, 1, 1), c->cur, ca);
    }
    HIPCHK(c, hipGetLastError());
    sel->empty = false;
    return FHERAM_OK;
}
// sels[i] <- the selector of bits [first_bit[i], first_bit[i] + bits_i) of fus[i]: Address::set_from_fheuint (conversion.rs:41-65) with the
// selector's plan shifted by first_bit, through k_cmux_chain — one launch per distinct (first_bit, bits) pair, no allocation, no host wait,
// in place.  Selector digits are read on the main stream only (fheram_bank_select prepares them there), so the launch is ordered by the stream.
int fheram_bank_selector_derive(fheram_bank* b, const fheram_fheuint* const* fus, const int* first_bit, int n, fheram_selector* const* sels) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!fus || !first_bit || !sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null integer list, bit list or selector list");
    if (n < 1 || n > FHERAM_SELECT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_SELECT_MAX = " + std::to_string(FHERAM_SELECT_MAX) + "]");
    for (int k = 0; k < n; k++) {   // every check for the whole list before anything is enqueued: a refused call changes no selector
        if (!fus[k] || fus[k]->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "integer " + std::to_string(k) + " is null or belongs to another bank");
        if (!sels[k] || sels[k]->bank != b) return fail(c, FHERAM_ERR_INVALID_ARG, "selector " + std::to_string(k) + " is null or belongs to another bank");
        if (sels[k]->fields) return fail(c, FHERAM_ERR_INVALID_ARG, "selector " + std::to_string(k) + " is a field selector: fheram_bank_selector_derive_fields derives it");
        if (first_bit[k] < 0 || first_bit[k] + sels[k]->bits > fus[k]->n_bits)
            return fail(c, FHERAM_ERR_INVALID_ARG, "bits [" + std::to_string(first_bit[k]) + ", " + std::to_string(first_bit[k]) + " + " + std::to_string(sels[k]->bits) + ") of integer " + std::to_string(k) + " are beyond its " + std::to_string(fus[k]->n_bits) + " bits");
        for (int q = 0; q < k; q++)
            if (sels[q] == sels[k]) return fail(c, FHERAM_ERR_INVALID_ARG, "selector " + std::to_string(k) + " appears twice in the list");
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->cur = c->stream;
    main_enqueued(c);
    bool done[FHERAM_SELECT_MAX] = {};
    for (int k = 0; k < n; k++) {
        if (done[k]) continue;
        CmuxChainArgs ca{};
        ca.tw = c->d_tw;
        ca.sign = 0;   // X^-v: what Ram::read accepts (address.rs:102-108)
        const fheram_selector* s0 = sels[k];
        for (int d = 0; d < s0->n_digits; d++) { ca.first[d] = (unsigned char)(first_bit[k] + s0->rsh[d]); ca.bits[d] = s0->width[d]; ca.lsh[d] = s0->lsh[d]; }
        int K = 0;
        for (int q = k; q < n; q++)
            if (first_bit[q] == first_bit[k] && sels[q]->bits == s0->bits) { ca.fu[K] = fus[q]->d_prep; ca.out[K] = sels[q]->d_ggsw; K++; done[q] = true; }
        const int rows = fheram_ctx::DNUM_CT * 2;
        ProfScope ps(c, "derive", (uint64_t)K * s0->n_digits * rows);
        cmux_chain_launch(dim3(rows, s0->n_digits, K), c->cur, ca);
    }
    HIPCHK(c, hipGetLastError());
    for (int k = 0; k < n; k++) sels[k]->empty = false;
    return FHERAM_OK;
}
int fheram_bank_selector_download(fheram_bank* b, const fheram_selector* s, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!out) return fail(c, FHERAM_ERR_INVALID_ARG, "null output");
    if (!s || s->bank != b) return fail(c, FHERAM_ERR_INVALID_ARG, "selector is null or belongs to another bank");
    if (s->empty) return fail(c, FHERAM_ERR_INVALID_ARG, "empty selector: fheram_bank_selector_alloc without fheram_bank_selector_derive");
    HIPCHK(c, hipSetDevice(c->device));
    return download_i64(c, out, s->d_ggsw, (size_t)s->n_digits * fheram_ctx::GGSW);
}
int fheram_selector_n_digits(const fheram_selector* s) { return s ? s->n_digits : 0; }
void fheram_selector_destroy(fheram_selector* s) {
    if (!s) return;
    hipSetDevice(s->device);
    if (s->d_ggsw) hipFree(s->d_ggsw);   // hipFree waits for outstanding work on the buffer
    delete s;
}

int fheram_bank_select(fheram_bank* b, const fheram_selector* const* sels, const int* n_cand, int n, const fheram_select_src* srcs,
                       const int64_t* host_words, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (!sels || !n_cand || !srcs) return fail(c, FHERAM_ERR_INVALID_ARG, "null selector list, candidate counts or sources");
    int total = 0, n_host = 0;
    int rc = select_check_sels(b, sels, n_cand, n, &total);
    if (rc == FHERAM_OK) rc = sources_check(b, srcs, total, host_words, 0, "", true, &n_host);
    if (rc != FHERAM_OK) return rc;
    const int ws = b->mws, Y = n * ws;
    HIPCHK(c, hipSetDevice(c->device));
    const int d = sels[0]->n_digits;
    rc = select_reserve(b, Y, n * d, n_host * ws);
    if (rc != FHERAM_OK) return rc;
    SelectBufs& S = b->sel;
    rc = host_words_stage(b, S.host, srcs, total, n_host, host_words);   // the host candidates: only the slots a source names
    if (rc != FHERAM_OK) return rc;
    // ---- enqueue ----
    main_enqueued(c);
    c->cur = c->stream;
    c->wide = true;   // (as a write: whatever gate wave a read_prepare_write parked is released by that operation's own trace chain, which is ahead of this on the stream)
    rc = host_words_copy(b, S.host, srcs, total, n_host);
    if (rc != FHERAM_OK) return rc;
    b->last[LAST_SELECT].n = 0;   // until this select is enqueued there is no last select
    {   // the pack: ONE launch, whatever n and m are
        SelectPackArgs sa{};
        sa.out = S.packed; sa.ws = ws;
        for (int k = 0, i = 0; k < n; k++) {
            sa.m[k] = n_cand[k];
            for (int j = 0; j < n_cand[k]; j++, i++) sa.cand[k][j] = select_source(b, srcs[i]);
        }
        ProfScope ps(c, "select_pack", (uint64_t)Y);
        select_pack_launch(dim3(1, Y, EW_SLICES), c->cur, sa);
    }
    return select_chain(b, sels, n, out);
}
// As fheram_bank_select with every candidate assembled lane by lane: the pack is k_select_pack_lanes over a pointer table in device memory
// (select_lanes.hip), everything behind it is select_chain.
int fheram_bank_select_lanes(fheram_bank* b, const fheram_selector* const* sels, const int* n_cand, int n, const fheram_select_lane* lanes,
                             const int64_t* host_words, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (!sels || !n_cand || !lanes) return fail(c, FHERAM_ERR_INVALID_ARG, "null selector list, candidate counts or lanes");
    int total = 0, n_host = 0;
    int rc = select_check_sels(b, sels, n_cand, n, &total);
    if (rc != FHERAM_OK) return rc;
    const int ws = b->mws, Y = n * ws, n_lanes = total * ws;
    unsigned need = 0;
    for (int i = 0; i < n_lanes; i++) {
        const fheram_select_lane& l = lanes[i];
        const std::string who = "lane " + std::to_string(i % ws) + " of candidate " + std::to_string(i / ws);
        rc = select_check_source(b, l.kind, l.index, who, host_words, need);
        if (rc != FHERAM_OK) return rc;
        if (l.reserved != 0) return fail(c, FHERAM_ERR_INVALID_ARG, who + " has reserved = " + std::to_string(l.reserved) + ", not 0");
        if (l.kind != FHERAM_SRC_ZERO && (l.lane < 0 || l.lane >= ws))
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " names lane " + std::to_string(l.lane) + ", outside the word's " + std::to_string(ws) + " ciphertexts");
        if (l.kind == FHERAM_SRC_HOST) n_host = std::max(n_host, l.index + 1);
    }
    rc = select_check_state(b, need);
    if (rc != FHERAM_OK) return rc;
    for (int i = 0; i < n_lanes; i++)
        if (lanes[i].kind == FHERAM_SRC_MEMBER_RESULT && !b->has_res[lanes[i].index])
            return fail(c, FHERAM_ERR_STATE, "lane " + std::to_string(i % ws) + " of candidate " + std::to_string(i / ws) + " names the result of member " + std::to_string(lanes[i].index) + ", which has none yet");
    HIPCHK(c, hipSetDevice(c->device));
    const int d = sels[0]->n_digits;
    rc = select_reserve(b, Y, n * d, n_host * ws);
    if (rc != FHERAM_OK) return rc;
    rc = lane_table_reserve(b);
    if (rc != FHERAM_OK) return rc;
    SelectBufs& S = b->sel;
    SelectLaneTable& L = b->lanes;
    const size_t G = fheram_ctx::GLWE;
    std::vector<char> staged((size_t)n_host * ws, 0);   // host ciphertext (slot, lane): named by a lane
    if (n_host) {   // range-checked as write words are: only the ciphertexts a lane names
        rc = stage_wait(c, S.host);
        if (rc != FHERAM_OK) return rc;
        for (int i = 0; i < n_lanes; i++) {
            if (lanes[i].kind != FHERAM_SRC_HOST) continue;
            const size_t at = (size_t)lanes[i].index * ws + lanes[i].lane;
            if (staged[at]) continue;
            staged[at] = 1;
            if (!narrow(host_words + at * G, S.host.host<int32_t>() + at * G, G))
                return fail(c, FHERAM_ERR_RANGE, "limb out of the normalised range [-2^16, 2^16]");
        }
    }
    rc = stage_wait(c, L);   // the last call's copy out of the pinned table
    if (rc != FHERAM_OK) return rc;
    SelectLanesArgs sa{};
    sa.table = L.dev<const int32_t*>(); sa.out = S.packed; sa.ws = ws;
    for (int k = 0, i = 0; k < n; k++) {
        sa.m[k] = n_cand[k];
        for (int j = 0; j < n_cand[k]; j++, i++)
            for (int w = 0; w < ws; w++) L.host<const int32_t*>()[(size_t)(k * ws + w) * SELECT_CAND_MAX + j] = select_source_lane(b, lanes[(size_t)i * ws + w]);
    }
    // ---- enqueue ----
    main_enqueued(c);
    c->cur = c->stream;
    c->wide = true;   // (as fheram_bank_select)
    if (n_host) {
        for (size_t at = 0; at < staged.size(); at++)
            if (staged[at]) HIPCHK(c, hipMemcpyAsync(S.host.dev<int32_t>() + at * G, S.host.host<int32_t>() + at * G, G * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        rc = stage_record(c, S.host);
        if (rc != FHERAM_OK) return rc;
    }
    b->last[LAST_SELECT].n = 0;   // until this select is enqueued there is no last select
    HIPCHK(c, hipMemcpyAsync(L.d, L.h, (size_t)Y * SELECT_CAND_MAX * sizeof(const int32_t*), hipMemcpyHostToDevice, c->stream));
    rc = stage_record(c, L);
    if (rc != FHERAM_OK) return rc;
    {   // the pack: ONE launch, whatever n, m and the lanes are
        ProfScope ps(c, "select_pack", (uint64_t)Y);
        select_lanes_launch(Y, c->cur, sa);
    }
    return select_chain(b, sels, n, out);
}
int fheram_bank_select_result(fheram_bank* b, int first, int n, int64_t* out) {
    return b ? last_result(b, LAST_SELECT, first, n, out) : FHERAM_ERR_INVALID_ARG;
}
// n independent Ram::write, entry k's words = output picks[k] of the last select: bank_write_set with a stage that copies on the device
// (no host wait, no range check: a select's outputs are normalised by construction)
int fheram_bank_write_list_selected(fheram_bank* b, const int* members, const fheram_addr* const* addrs, int n, const int* picks) {
    MemberSet s;
    const int rc = write_list_check(b, members, addrs, n, !picks, 1, &s);
    if (rc != FHERAM_OK) return rc;
    fheram_ctx* c = b->c;
    const int sel_n = b->last[LAST_SELECT].n;
    if (!sel_n) return fail(c, FHERAM_ERR_STATE, "no select has run on this bank");
    for (int k = 0; k < n; k++)
        if (picks[k] < 0 || picks[k] >= sel_n)
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " picks output " + std::to_string(picks[k]) + ", outside the last select's " + std::to_string(sel_n) + " outputs");
    const long G = (long)fheram_ctx::GLWE;
    return bank_write_set(b, s, addrs, [&](int32_t* d_w, int) {
        main_enqueued(c);
        for (int k = 0; k < n; k++) launch_copy(c, ref(b->sel.res + (size_t)picks[k] * b->mws * G, G, 0), ref(d_w + (size_t)k * b->mws * G, G, 0), 1, b->mws);
        return (int)FHERAM_OK;
    });
}
int fheram_bank_selftest_fail_select_alloc(fheram_bank* b, int nth) {
    if (!b || nth < 0) return FHERAM_ERR_INVALID_ARG;
    b->sel_fail_alloc = nth;
    return FHERAM_OK;
}

}  // extern "C"

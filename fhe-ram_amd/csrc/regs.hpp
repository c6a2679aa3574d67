// A bank's REGISTER FILE: a one-row RAM of 2^bits words (1 <= bits <= FHERAM_SELECT_BITS_MAX; a WIDE one, made by
// fheram_bank_regs_create_wide and addressed by wide selectors: <= FHERAM_TABLE_BITS_MAX) that lives beside the bank's members, under
// the bank's keys, stream, configuration and round-off monitor.  Its addresses are the bank's selectors, its results feed the selects,
// and it takes a written word from any source a select candidate may come from.
//
// CONTRACT-COMPATIBLE ONLY, as the select is (select.hpp): the operations are Ram::read / read_prepare_write / write
// (ram.rs:172-294, the rows == 1, one-coordinate path) of a RAM of max_addr = 2^bits whose row w packs byte w of word j at coefficient j.
// select.hpp already states that a select IS Ram::read on such a row; here the row persists and has a write side:
//   read                n reads of the row as ONE operation: the row fanned out to n * ws chain inputs (k_regs_fan, one launch), then exactly
//                       what a select enqueues behind its pack (select.hpp one_row_reads), on the register files' own buffers
//   read_prepare_write  the products with the selector's digits IN PLACE on the row (ram.rs:502-504), then trace(0, log N) of the rotated
//                       row into the register file's kept trace — the result (the OLD word), and what the write starts from (memo_top)
//   write               row <- normalize(row - trace(row) + w) (k_regs_merge: write_first_step, the word through a pointer), the selector's
//                       inverse digits (coordinate_prepare_inv on its digits), the products with them in place (ram.rs:644-646)
// Everything runs on the bank's main stream.  A register file owns its device buffers (the row, the kept trace, two temporaries, its
// prepared digits, its inverse digits), all allocated by fheram_bank_regs_create; what the register files of a bank share (path.hpp
// OneRowSet) is allocated by the bank's first create.  No operation allocates.  No member's rows, state flag, tree, result or kept memo is
// touched, nor the last read list's or the last select's results.
//
// This file has two parts: what regs.hip (the kernels' translation unit) and fheram.hip share — the argument structs and the launchers —
// and, for fheram.hip only, the host logic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int REGS_SLICES = 8;     // workgroups per ciphertext (blockIdx.z), as the elementwise kernels (launch.hpp EW_SLICES)
constexpr int REGS_CT_MAX = 64;    // ciphertexts of one launch: n * ws of a read, ws of a write
struct RegsFanArgs {
    const int32_t* row;            // [ws] GLWE (3 limbs)
    int32_t* out;                  // [n * ws] GLWE: out[k * ws + w] = row[w]
    int ws;
};
struct RegsMergeArgs {             // by value: no table in device memory, nothing to stage
    int32_t* row;                  // [ws] GLWE, in place: row[w] <- normalize(row[w] - tr[w] + src[w])
    const int32_t* tr;             // [ws] GLWE
    const int32_t* src[REGS_CT_MAX];   // ciphertext w of the written word: ONE GLWE; nullptr: the all-zero ciphertext
};
// grid: (1, n_ct, REGS_SLICES) / (1, ws, REGS_SLICES)
void regs_fan_launch(int n_ct, hipStream_t stream, const RegsFanArgs& fa);
void regs_merge_launch(int ws, hipStream_t stream, const RegsMergeArgs& ma);

}  // namespace fk

#ifndef FK_REGS_KERNELS_ONLY
#include "select.hpp"

struct fheram_regs {
    fheram_bank* bank;     // owner; nullptr once the bank has been destroyed (the device buffers went with it)
    int device, bits;
    bool initialized = false, state = false;
    bool memo = false;     // tr = trace(row), left by read_prepare_write on this very row (RamState::memo_top)
    int32_t *row = nullptr, *tr = nullptr, *tmp = nullptr, *tmp2 = nullptr;   // [ws] GLWE
    double* prep = nullptr;       // [REGS_DIGITS_MAX] prepared GGSW: read_prepare_write's digits
    int32_t* inv_std = nullptr;   // [REGS_DIGITS_MAX] std-form GGSW: the write's inverse digits
    double* inv_prep = nullptr;   // [REGS_DIGITS_MAX] prepared GGSW: the same, prepared
};

namespace {

static_assert(REGS_SLICES == EW_SLICES && REGS_CT_MAX == 64, "the register kernels cover a ciphertext as the elementwise kernels do; a call has at most 64 ciphertexts");
// the digits of one selector a register file's own buffers (prep, inv_std, inv_prep) and the shared set's prepared digits hold
constexpr int REGS_DIGITS_MAX = FHERAM_SELECT_BITS_MAX;
static_assert(REGS_DIGITS_MAX == FHERAM_SELECTOR_WIDE_DIGITS_MAX, "a wide register file's selector has up to FHERAM_SELECTOR_WIDE_DIGITS_MAX digits: the per-object and per-bank digit buffers hold them");
static_assert((1 << FHERAM_TABLE_BITS_MAX) == N, "a wide register file's row holds one word per coefficient");

void regs_free_device(fheram_regs* r) {
    void* bufs[] = {r->row, r->tr, r->tmp, r->tmp2, r->prep, r->inv_std, r->inv_prep};
    for (void* p : bufs) if (p) hipFree(p);
    r->row = r->tr = r->tmp = r->tmp2 = r->inv_std = nullptr;
    r->prep = r->inv_prep = nullptr;
}
void regs_keys_changed(fheram_bank* b) {
    for (fheram_regs* r : b->regfiles) r->memo = false;   // a kept trace is void with new keys
}
// fheram_bank_destroy (both streams idle): every live register file loses its device buffers and its bank; its handle stays valid for
// fheram_regs_destroy and for nothing else
void regs_bank_release(fheram_bank* b) {
    for (fheram_regs* r : b->regfiles) { regs_free_device(r); r->bank = nullptr; r->initialized = false; }
    b->regfiles.clear();
    one_row_free(b->regs);
}
// what the register files of a bank share, whole (path.hpp OneRowSet): the stage holds the 2^FHERAM_SELECT_BITS_MAX host words of a pack or a write
int regs_bufs_reserve(fheram_bank* b) {
    return one_row_reserve(b->c, b->regs, b->mws, REGS_DIGITS_MAX, (size_t)(1 << FHERAM_SELECT_BITS_MAX) * b->mws * fheram_ctx::GLWE * sizeof(int32_t), "buffers of the bank's register files");
}
// the handle: null, of another bank (or of a destroyed one)
int regs_check_handle(fheram_bank* b, const fheram_regs* r) {
    if (!r || r->bank != b) return fail(b->c, FHERAM_ERR_INVALID_ARG, "the register file is null or belongs to another bank");
    return FHERAM_OK;
}
// a selector as the address of register file r
int regs_check_selector(fheram_bank* b, const fheram_regs* r, const fheram_selector* s, const std::string& who) {
    const int rc = selector_check(b, s, who);
    if (rc != FHERAM_OK) return rc;
    if (s->bits != r->bits) return fail(b->c, FHERAM_ERR_INVALID_ARG, who + " has " + std::to_string(s->bits) + " bits, the register file " + std::to_string(r->bits));
    return FHERAM_OK;
}
// initialised, the keys, the wanted state (0: read / read_prepare_write, 1: write)
int regs_check_ready(fheram_bank* b, const fheram_regs* r, int want_state) {
    fheram_ctx* c = b->c;
    if (!r->initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: the register file has had no fheram_bank_regs_upload or fheram_bank_regs_pack");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    if (want_state == 0 && r->state)
        return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.read: internal state is true -> requires calling Memory.write (register file)");
    if (want_state == 1 && !r->state)
        return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.write: internal state is false -> requires calling Memory.read_prepare_write (register file)");
    return FHERAM_OK;
}
// The sources of a pack or a write (select.hpp sources_check): a host slot is one of the 2^FHERAM_SELECT_BITS_MAX the register files stage
int regs_check_sources(fheram_bank* b, const fheram_select_src* srcs, int n, const int64_t* host_words, bool keys, int* n_host) {
    return sources_check(b, srcs, n, host_words, 1 << FHERAM_SELECT_BITS_MAX, "a register file takes", keys, n_host);
}
// n reads of register file r as one operation, behind the handle and the list: every selector, then the state.  who: what a selector is
// called ("selector ", the mix's "register selector "); digits_tail: why two selectors may not differ in digits, in the caller's words
int regs_check_reads(fheram_bank* b, const fheram_regs* r, const fheram_selector* const* sels, int n, const std::string& who, const char* digits_tail) {
    for (int k = 0; k < n; k++) {
        const int rc = regs_check_selector(b, r, sels[k], who + std::to_string(k));
        if (rc != FHERAM_OK) return rc;
        if (sels[k]->n_digits != sels[0]->n_digits)   // (field selectors: the same bits in another number of digits)
            return fail(b->c, FHERAM_ERR_INVALID_ARG, who + std::to_string(k) + " has " + std::to_string(sels[k]->n_digits) + " digits, " + who + "0 " + std::to_string(sels[0]->n_digits) + ": " + digits_tail);
    }
    return regs_check_ready(b, r, 0);
}
// one row up or down: a register file's, a table's (table.hpp)
int row_upload(fheram_bank* b, int32_t* dst, const int64_t* row) {
    fheram_ctx* c = b->c;
    if (!row) return fail(c, FHERAM_ERR_INVALID_ARG, "null row");
    HIPCHK(c, hipSetDevice(c->device));
    return upload_i64(c, dst, row, (size_t)b->mws * fheram_ctx::GLWE);
}
int row_download(fheram_bank* b, const int32_t* src, bool initialized, const char* uninitialized, int64_t* row) {
    fheram_ctx* c = b->c;
    if (!row) return fail(c, FHERAM_ERR_INVALID_ARG, "null row");
    if (!initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, uninitialized);
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = download_i64(c, row, src, (size_t)b->mws * fheram_ctx::GLWE);
    return rc == FHERAM_OK ? check_precision(c) : rc;
}
void regs_begin(fheram_ctx* c) {
    main_enqueued(c);
    c->cur = c->stream;
    c->wide = true;   // (as a select: whatever gate wave a member's read_prepare_write parked is released by that operation's own trace chain, ahead of this on the stream)
}
// both creators: the bound on the bits is the caller's (bits_max, by its name), everything else is one register file's
int regs_new(fheram_bank* b, int bits, int bits_max, const char* max_name, fheram_regs** out) {
    fheram_ctx* c = b->c;
    if (!out) return fail(c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    if (bits < 1 || bits > bits_max)
        return fail(c, FHERAM_ERR_INVALID_ARG, "bits = " + std::to_string(bits) + " is outside [1, " + max_name + " = " + std::to_string(bits_max) + "]");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = regs_bufs_reserve(b);
    if (rc != FHERAM_OK) return rc;
    fheram_regs* r = new fheram_regs{b, c->device, bits};
    const size_t ct = (size_t)b->mws * fheram_ctx::GLWE * sizeof(int32_t), digits = (size_t)REGS_DIGITS_MAX * fheram_ctx::GGSW;
    hipError_t e = hipSuccess;
    for (int32_t** p : {&r->row, &r->tr, &r->tmp, &r->tmp2}) if (e == hipSuccess) e = hipMalloc((void**)p, ct);
    if (e == hipSuccess) e = hipMalloc((void**)&r->prep, digits * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&r->inv_std, digits * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&r->inv_prep, digits * sizeof(double));
    if (e != hipSuccess) {
        regs_free_device(r);
        delete r;
        (void)hipGetLastError();
        return fail(c, FHERAM_ERR_DEVICE, std::string("buffers of a register file: ") + hipGetErrorString(e));
    }
    b->regfiles.push_back(r);
    *out = r;
    return FHERAM_OK;
}

}  // namespace

extern "C" {

int fheram_bank_regs_create(fheram_bank* b, int bits, fheram_regs** out) {
    return b ? regs_new(b, bits, FHERAM_SELECT_BITS_MAX, "FHERAM_SELECT_BITS_MAX", out) : FHERAM_ERR_INVALID_ARG;
}
// a WIDE register file: up to one word per coefficient of the row, addressed by wide selectors (table.hpp)
int fheram_bank_regs_create_wide(fheram_bank* b, int bits, fheram_regs** out) {
    return b ? regs_new(b, bits, FHERAM_TABLE_BITS_MAX, "FHERAM_TABLE_BITS_MAX", out) : FHERAM_ERR_INVALID_ARG;
}
// Who frees: a register file frees its own device buffers here while its bank lives; fheram_bank_destroy frees those of every register file
// still alive and detaches them, after which this only releases the handle.  Either order is safe.
void fheram_regs_destroy(fheram_regs* r) {
    if (!r) return;
    if (fheram_bank* b = r->bank) {
        hipSetDevice(r->device);
        regs_free_device(r);   // hipFree waits for outstanding work on the buffer
        b->regfiles.erase(std::remove(b->regfiles.begin(), b->regfiles.end(), r), b->regfiles.end());
        if (b->regs_old_owner == r) { b->regs_old = nullptr; b->regs_old_owner = nullptr; }   // its kept trace WAS the last read_prepare_write's result
    }
    delete r;
}
int fheram_regs_bits(const fheram_regs* r) { return r ? r->bits : 0; }
int fheram_bank_regs_state(const fheram_bank* b, const fheram_regs* r) { return (b && r && r->bank == b) ? (int)r->state : 0; }

int fheram_bank_regs_upload(fheram_bank* b, fheram_regs* r, const int64_t* row) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    int rc = regs_check_handle(b, r);
    if (rc == FHERAM_OK) rc = row_upload(b, r->row, row);
    if (rc != FHERAM_OK) return rc;
    r->initialized = true; r->state = false; r->memo = false;
    return FHERAM_OK;
}
int fheram_bank_regs_download(fheram_bank* b, const fheram_regs* r, int64_t* row) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    const int rc = regs_check_handle(b, r);
    return rc == FHERAM_OK ? row_download(b, r->row, r->initialized, "unitialized memory: the register file has had no fheram_bank_regs_upload or fheram_bank_regs_pack", row) : rc;
}
// row <- glwe_normalize(sum_j X^j * c_j[w]): the pack of fheram_bank_select (k_select_pack, one launch) into the register file
int fheram_bank_regs_pack(fheram_bank* b, fheram_regs* r, int n_cand, const fheram_select_src* srcs, const int64_t* host_words) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc != FHERAM_OK) return rc;
    if (!srcs) return fail(c, FHERAM_ERR_INVALID_ARG, "null sources");
    if (n_cand < 1 || n_cand > (1 << r->bits))
        return fail(c, FHERAM_ERR_INVALID_ARG, "the pack has " + std::to_string(n_cand) + " candidates, outside [1, 2^bits = " + std::to_string(1 << r->bits) + "]");
    if (n_cand > SELECT_CAND_MAX)   // (a wide register file)
        return fail(c, FHERAM_ERR_INVALID_ARG, "the pack has " + std::to_string(n_cand) + " candidates, more than the " + std::to_string(SELECT_CAND_MAX) + " the argument struct of k_select_pack holds (words behind them: fheram_bank_regs_poke)");
    int n_host = 0;
    rc = regs_check_sources(b, srcs, n_cand, host_words, false, &n_host);
    if (rc != FHERAM_OK) return rc;
    if (r->initialized && r->state)
        return fail(c, FHERAM_ERR_STATE, "the register file is between read_prepare_write and write: a pack would drop the pending write (fheram_bank_regs_upload resets)");
    HIPCHK(c, hipSetDevice(c->device));
    rc = host_words_stage(b, b->regs.stage, srcs, n_cand, n_host, host_words);
    if (rc != FHERAM_OK) return rc;
    // ---- enqueue ----
    regs_begin(c);
    rc = host_words_copy(b, b->regs.stage, srcs, n_cand, n_host);
    if (rc != FHERAM_OK) return rc;
    {
        SelectPackArgs sa{};
        sa.out = r->row; sa.ws = b->mws; sa.m[0] = n_cand;
        for (int j = 0; j < n_cand; j++) sa.cand[0][j] = select_source(b, srcs[j], b->regs.stage.dev<int32_t>());
        ProfScope ps(c, "select_pack", (uint64_t)b->mws);
        select_pack_launch(dim3(1, b->mws, EW_SLICES), c->cur, sa);
    }
    HIPCHK(c, hipGetLastError());
    r->initialized = true; r->state = false; r->memo = false;
    return FHERAM_OK;
}
// n independent Ram::read of the row as ONE operation (header comment)
int fheram_bank_regs_read(fheram_bank* b, const fheram_regs* r, const fheram_selector* const* sels, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc != FHERAM_OK) return rc;
    if (!sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null selector list");
    if (n < 1 || n > FHERAM_SELECT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_SELECT_MAX = " + std::to_string(FHERAM_SELECT_MAX) + "]");
    const int ws = b->mws, Y = n * ws;
    if (Y > REGS_CT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n * word_size = " + std::to_string(Y) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    rc = regs_check_reads(b, r, sels, n, "selector ", "the operand table of one call has one stride");
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // ---- enqueue ----
    OneRowSet& R = b->regs;
    regs_begin(c);
    b->last[LAST_REGS].n = 0;   // until this read is enqueued there is no last register read
    {
        RegsFanArgs fa{r->row, R.fan, ws};
        ProfScope ps(c, "elementwise", (uint64_t)Y);
        regs_fan_launch(Y, c->cur, fa);
    }
    one_row_reads(b, OneRowBufs{R.fan, R.ep, R.tmp, R.res, R.prep}, sels, n);
    HIPCHK(c, hipGetLastError());
    b->last[LAST_REGS] = LastOutputs{n, ResHome{R.res, R.h_res, R.d_h_res, -1}};
    if (!out) return FHERAM_OK;
    const ResRun run{R.res, (size_t)Y * fheram_ctx::GLWE};
    return result_export(c, &run, 1, R.h_res, R.d_h_res, out);
}
int fheram_bank_regs_result(fheram_bank* b, int first, int n, int64_t* out) {
    return b ? last_result(b, LAST_REGS, first, n, out) : FHERAM_ERR_INVALID_ARG;
}
// Ram::read_prepare_write (ram.rs:196-222) of the one-row RAM (header comment)
int fheram_bank_regs_read_prepare_write(fheram_bank* b, fheram_regs* r, const fheram_selector* sel, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc == FHERAM_OK) rc = regs_check_selector(b, r, sel, "the selector");
    if (rc == FHERAM_OK) rc = regs_check_ready(b, r, 0);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // ---- enqueue ----
    regs_begin(c);
    const int ws = b->mws, d = sel->n_digits;
    const long G = (long)fheram_ctx::GLWE;
    const GlweRef row = ref(r->row, G, 0), tr = ref(r->tr, G, 0), tmp = ref(r->tmp, G, 0);
    launch_prepare(c, sel->d_ggsw, r->prep, d * (int)(fheram_ctx::GGSW / N));   // CoordinatePrepared::prepare
    ep_chain(c, row, row, tmp, r->prep, d, 1, ws);                              // ram.rs:502-504 (rows == 1): the rotated row stays in place
    trace_steps(c, row, tr, tmp, 0, LOGN, 1, ws);                               // ram.rs:540; = what write_first_step computes first (ram.rs:571-572)
    HIPCHK(c, hipGetLastError());
    r->state = true;                                                            // ram.rs:533
    r->memo = c->cfg.memo != 0;
    b->regs_old = r->tr; b->regs_old_owner = r;
    if (!out) return FHERAM_OK;
    const ResRun run{r->tr, (size_t)ws * fheram_ctx::GLWE};
    return result_export(c, &run, 1, b->regs.h_res, b->regs.d_h_res, out);
}
int fheram_bank_regs_old_result(fheram_bank* b, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!out) return fail(c, FHERAM_ERR_INVALID_ARG, "null output");
    if (!b->regs_old) return fail(c, FHERAM_ERR_STATE, "no fheram_bank_regs_read_prepare_write has run on this bank (or its register file is gone)");
    HIPCHK(c, hipSetDevice(c->device));
    const ResRun run{b->regs_old, (size_t)b->mws * fheram_ctx::GLWE};
    return result_export(c, &run, 1, b->regs.h_res, b->regs.d_h_res, out);
}
// Ram::write (ram.rs:226-294) of ONE word, taken on the device from any source kind (header comment).  No host wait.
int fheram_bank_regs_write(fheram_bank* b, fheram_regs* r, const fheram_selector* sel, fheram_select_src src, const int64_t* host_words) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc == FHERAM_OK) rc = regs_check_selector(b, r, sel, "the selector");
    if (rc != FHERAM_OK) return rc;
    int n_host = 0;
    rc = regs_check_sources(b, &src, 1, host_words, true, &n_host);
    if (rc == FHERAM_OK) rc = regs_check_ready(b, r, 1);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = host_words_stage(b, b->regs.stage, &src, 1, n_host, host_words);   // a refused word: the register file stays prepared and untouched
    if (rc != FHERAM_OK) return rc;
    // ---- enqueue ----
    regs_begin(c);
    rc = host_words_copy(b, b->regs.stage, &src, 1, n_host);
    if (rc != FHERAM_OK) return rc;
    const int ws = b->mws, d = sel->n_digits;
    const long G = (long)fheram_ctx::GLWE;
    const GlweRef row = ref(r->row, G, 0), tmp = ref(r->tmp, G, 0), tmp2 = ref(r->tmp2, G, 0);
    const int32_t* tr = r->tr;                                   // = trace(row), computed by read_prepare_write on this very row
    if (!r->memo) { trace_steps(c, row, tmp, tmp2, 0, LOGN, 1, ws); tr = r->tmp; }   // memo = 0, new keys: recomputed (ram.rs:571-572)
    {   // write_first_step (ram.rs:544-577): row <- normalize(row - trace(row) + w)
        RegsMergeArgs ma{};
        ma.row = r->row; ma.tr = tr;
        const int32_t* w = select_source(b, src, b->regs.stage.dev<int32_t>());
        for (int i = 0; i < ws; i++) ma.src[i] = w ? w + (size_t)i * G : nullptr;
        ProfScope ps(c, "elementwise", (uint64_t)ws);
        regs_merge_launch(ws, c->cur, ma);
    }
    coordinate_prepare_inv(c, sel->d_ggsw, d, r->inv_std, r->inv_prep);   // ram.rs:278-289
    ep_chain(c, row, row, tmp, r->inv_prep, d, 1, ws);                    // ram.rs:644-646
    HIPCHK(c, hipGetLastError());
    r->state = false; r->memo = false;                                    // ram.rs:648
    return FHERAM_OK;
}

}  // extern "C"
#endif   // FK_REGS_KERNELS_ONLY

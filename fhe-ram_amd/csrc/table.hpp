// A bank's TABLES: read-only one-row RAMs of 2^bits words (1 <= bits <= FHERAM_TABLE_BITS_MAX = log N) that live beside the bank's members
// and register files, under the bank's keys, main stream, configuration and round-off monitor: an instruction ROM, or a lookup table
// indexed by an encrypted field.  A row is one GLWE of N coefficients, so a one-row RAM holds up to N words; as a bank member the same
// ROM would have the bank's shape and pay the members' row chains on every fetch.
//
// CONTRACT-COMPATIBLE ONLY, as the select and the register file are (select.hpp, regs.hpp): the read is Ram::read
// (ram.rs:172-191, the rows == 1, one-coordinate path) of a RAM of max_addr = 2^bits whose row w packs byte w of word j at coefficient j.
//   read        n reads of any tables of the bank as ONE operation: row w of tables[k] gathered to chain input k * ws + w (k_table_fan, one
//               launch), then exactly what a select enqueues behind its pack (select.hpp one_row_reads), on the tables' own buffers
//   load_plain  public bytes as the trivial ciphertext Ram::encrypt_sk's encoding gives with all-zero mask and noise (k_table_encode, one
//               launch from a pinned staging buffer): no host encryption, no keys, no secret
//   selectors   WIDE selectors: fheram_selector handles of up to FHERAM_TABLE_BITS_MAX bits and FHERAM_SELECTOR_WIDE_DIGITS_MAX digits,
//               made here; every derivation takes them unchanged, the select and the register file refuse them
// Everything runs on the bank's main stream.  A table owns its row, allocated by fheram_bank_table_create; what the tables of a bank
// share (path.hpp OneRowSet) is allocated by the bank's first create.  No operation allocates.  No member's rows, state flag, tree, result
// or kept memo is touched, no register file's row or state, nor the last read list's, select's or register read's results.
//
// This file has two parts: what table.hip (the kernels' translation unit) and fheram.hip share — the argument structs and the launchers —
// and, for fheram.hip only, the host logic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int TABLE_SLICES = 8;     // workgroups per ciphertext (blockIdx.z), as the elementwise kernels (launch.hpp EW_SLICES)
constexpr int TABLE_CT_MAX = 64;    // ciphertexts of one launch: n * ws of a read
struct TableFanArgs {               // by value: no table in device memory, nothing to stage
    const int32_t* src[TABLE_CT_MAX];   // output ciphertext y = k * ws + w: row w of tables[k], ONE GLWE (3 limbs)
    int32_t* out;                       // [n * ws] GLWE
};
struct TableEncodeArgs {
    const uint8_t* data;            // [n_words * ws] bytes: byte w of word j at data[j * ws + w]
    int32_t* row;                   // [ws] GLWE (3 limbs)
    int ws, n_words;                // n_words <= N
    int k_pt, size_pt;              // the plaintext precision and its limbs (setup.hpp encode_value)
};
// grid: (1, n_ct, TABLE_SLICES) / (1, ws, TABLE_SLICES)
void table_fan_launch(int n_ct, hipStream_t stream, const TableFanArgs& fa);
void table_encode_launch(int ws, hipStream_t stream, const TableEncodeArgs& ea);

}  // namespace fk

#ifndef FK_TABLE_KERNELS_ONLY
#include "regs.hpp"

struct fheram_table {
    fheram_bank* bank;     // owner; nullptr once the bank has been destroyed (the row went with it)
    int device, bits;
    bool initialized = false;
    int32_t* row = nullptr;   // [ws] GLWE
};

namespace {

static_assert(TABLE_SLICES == EW_SLICES && TABLE_CT_MAX == 64, "the table kernels cover a ciphertext as the elementwise kernels do; a call has at most 64 ciphertexts");
static_assert((1 << FHERAM_TABLE_BITS_MAX) == N, "a table's row holds one word per coefficient");

// fheram_bank_destroy (both streams idle): every live table loses its row and its bank; its handle stays valid for fheram_table_destroy
// and for nothing else
void table_bank_release(fheram_bank* b) {
    for (fheram_table* t : b->tables) { if (t->row) hipFree(t->row); t->row = nullptr; t->bank = nullptr; t->initialized = false; }
    b->tables.clear();
    one_row_free(b->tabs);
}
// what the tables of a bank share, whole (path.hpp OneRowSet): the stage holds the bytes of a load_plain
int table_bufs_reserve(fheram_bank* b) {
    return one_row_reserve(b->c, b->tabs, b->mws, FHERAM_SELECTOR_WIDE_DIGITS_MAX, (size_t)(1 << FHERAM_TABLE_BITS_MAX) * b->mws, "buffers of the bank's tables");
}
// the handle: null, of another bank (or of a destroyed one)
int table_check_handle(fheram_bank* b, const fheram_table* t, const std::string& who) {
    if (!t || t->bank != b) return fail(b->c, FHERAM_ERR_INVALID_ARG, who + " is null or belongs to another bank");
    return FHERAM_OK;
}
// n reads of tables as one operation, behind the lists: every table and its selector, then every table initialised.  who: what a selector
// is called ("selector ", the mix's "table selector "); digits_tail: why two selectors may not differ in digits, in the caller's words
int table_check_reads(fheram_bank* b, const fheram_table* const* tables, const fheram_selector* const* sels, int n, const std::string& who, const char* digits_tail) {
    fheram_ctx* c = b->c;
    for (int k = 0; k < n; k++) {
        int rc = table_check_handle(b, tables[k], "table " + std::to_string(k));
        if (rc == FHERAM_OK) rc = selector_check(b, sels[k], who + std::to_string(k), "fheram_bank_table_selector_alloc");
        if (rc != FHERAM_OK) return rc;
        const fheram_selector* s = sels[k];
        if (s->bits != tables[k]->bits) return fail(c, FHERAM_ERR_INVALID_ARG, who + std::to_string(k) + " has " + std::to_string(s->bits) + " bits, table " + std::to_string(k) + " " + std::to_string(tables[k]->bits));
        if (s->n_digits != sels[0]->n_digits)   // (the tables of a call may differ in bits; the operand table has one stride)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + std::to_string(k) + " has " + std::to_string(s->n_digits) + " digits, " + who + "0 " + std::to_string(sels[0]->n_digits) + ": " + digits_tail);
    }
    for (int k = 0; k < n; k++)
        if (!tables[k]->initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: table " + std::to_string(k) + " has had no fheram_bank_table_upload or fheram_bank_table_load_plain");
    return FHERAM_OK;
}

}  // namespace

extern "C" {

int fheram_bank_table_create(fheram_bank* b, int bits, fheram_table** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!out) return fail(c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    if (bits < 1 || bits > FHERAM_TABLE_BITS_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "bits = " + std::to_string(bits) + " is outside [1, FHERAM_TABLE_BITS_MAX = " + std::to_string(FHERAM_TABLE_BITS_MAX) + "]");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = table_bufs_reserve(b);
    if (rc != FHERAM_OK) return rc;
    fheram_table* t = new fheram_table{b, c->device, bits};
    const hipError_t e = hipMalloc((void**)&t->row, (size_t)b->mws * fheram_ctx::GLWE * sizeof(int32_t));
    if (e != hipSuccess) {
        delete t;
        (void)hipGetLastError();
        return fail(c, FHERAM_ERR_DEVICE, std::string("the row of a table: ") + hipGetErrorString(e));
    }
    b->tables.push_back(t);
    *out = t;
    return FHERAM_OK;
}
// Who frees: a table frees its own row here while its bank lives; fheram_bank_destroy frees those of every table still alive and
// detaches them, after which this only releases the handle.  Either order is safe.
void fheram_table_destroy(fheram_table* t) {
    if (!t) return;
    if (fheram_bank* b = t->bank) {
        hipSetDevice(t->device);
        if (t->row) hipFree(t->row);   // hipFree waits for outstanding work on the buffer
        b->tables.erase(std::remove(b->tables.begin(), b->tables.end(), t), b->tables.end());
    }
    delete t;
}
int fheram_table_bits(const fheram_table* t) { return t ? t->bits : 0; }

int fheram_bank_table_upload(fheram_bank* b, fheram_table* t, const int64_t* row) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    int rc = table_check_handle(b, t, "the table");
    if (rc == FHERAM_OK) rc = row_upload(b, t->row, row);
    if (rc != FHERAM_OK) return rc;
    t->initialized = true;
    return FHERAM_OK;
}
int fheram_bank_table_download(fheram_bank* b, const fheram_table* t, int64_t* row) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    const int rc = table_check_handle(b, t, "the table");
    return rc == FHERAM_OK ? row_download(b, t->row, t->initialized, "unitialized memory: the table has had no fheram_bank_table_upload or fheram_bank_table_load_plain", row) : rc;
}
// the row <- the trivial ciphertext of public bytes (header comment): one copy out of the pinned staging buffer, one launch
int fheram_bank_table_load_plain(fheram_bank* b, fheram_table* t, const uint8_t* data, size_t data_len) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = table_check_handle(b, t, "the table");
    if (rc != FHERAM_OK) return rc;
    if (!data) return fail(c, FHERAM_ERR_INVALID_ARG, "null data");
    const size_t want = ((size_t)1 << t->bits) * (size_t)b->mws;
    if (data_len != want)
        return fail(c, FHERAM_ERR_INVALID_ARG, "invalid data: data_len = " + std::to_string(data_len) + ", a table of " + std::to_string(t->bits) + " bits takes 2^bits * word_size = " + std::to_string(want) + " bytes");
    const int k_pt = (int)c->p.k_glwe_pt, size_pt = (k_pt + BASE2K - 1) / BASE2K;
    if (k_pt <= 0 || k_pt > 8 + BASE2K || size_pt > fheram_ctx::S_CT) return fail(c, FHERAM_ERR_UNSUPPORTED, "k_glwe_pt out of range");   // (as fheram_ram_encrypt_sk)
    HIPCHK(c, hipSetDevice(c->device));
    HostStage& st = b->tabs.stage;
    rc = stage_wait(c, st);
    if (rc != FHERAM_OK) return rc;
    std::memcpy(st.h, data, data_len);
    // ---- enqueue ----
    main_enqueued(c);
    c->cur = c->stream;
    HIPCHK(c, hipMemcpyAsync(st.d, st.h, data_len, hipMemcpyHostToDevice, c->stream));
    rc = stage_record(c, st);
    if (rc != FHERAM_OK) return rc;
    {
        const TableEncodeArgs ea{st.d, t->row, b->mws, 1 << t->bits, k_pt, size_pt};
        ProfScope ps(c, "elementwise", (uint64_t)b->mws);
        table_encode_launch(b->mws, c->cur, ea);
    }
    HIPCHK(c, hipGetLastError());
    t->initialized = true;
    return FHERAM_OK;
}
// n independent Ram::read of one-row RAMs as ONE operation (header comment)
int fheram_bank_table_read(fheram_bank* b, const fheram_table* const* tables, const fheram_selector* const* sels, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (!tables || !sels) return fail(c, FHERAM_ERR_INVALID_ARG, "null table list or null selector list");
    if (n < 1 || n > FHERAM_SELECT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_SELECT_MAX = " + std::to_string(FHERAM_SELECT_MAX) + "]");
    const int ws = b->mws, Y = n * ws;
    if (Y > TABLE_CT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n * word_size = " + std::to_string(Y) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    const int rc = table_check_reads(b, tables, sels, n, "selector ", "the operand table of one call has one stride");
    if (rc != FHERAM_OK) return rc;
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    HIPCHK(c, hipSetDevice(c->device));
    // ---- enqueue ----
    OneRowSet& B = b->tabs;
    regs_begin(c);
    b->last[LAST_TABLE].n = 0;   // until this read is enqueued there is no last table read
    {
        TableFanArgs fa{};
        fa.out = B.fan;
        for (int k = 0; k < n; k++)
            for (int w = 0; w < ws; w++) fa.src[k * ws + w] = tables[k]->row + (size_t)w * fheram_ctx::GLWE;
        ProfScope ps(c, "elementwise", (uint64_t)Y);
        table_fan_launch(Y, c->cur, fa);
    }
    one_row_reads(b, OneRowBufs{B.fan, B.ep, B.tmp, B.res, B.prep}, sels, n);
    HIPCHK(c, hipGetLastError());
    b->last[LAST_TABLE] = LastOutputs{n, ResHome{B.res, B.h_res, B.d_h_res, -1}};
    if (!out) return FHERAM_OK;
    const ResRun run{B.res, (size_t)Y * fheram_ctx::GLWE};
    return result_export(c, &run, 1, B.h_res, B.d_h_res, out);
}
int fheram_bank_table_result(fheram_bank* b, int first, int n, int64_t* out) {
    return b ? last_result(b, LAST_TABLE, first, n, out) : FHERAM_ERR_INVALID_ARG;
}

// WIDE selectors: the selectors of select.hpp with the table's bound on the bits (selector_new says what else is refused)
int fheram_bank_table_selector_alloc(fheram_bank* b, int bits, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    return selector_new(b, bits, out, FHERAM_TABLE_BITS_MAX, "FHERAM_TABLE_BITS_MAX");
}
int fheram_bank_table_selector_create(fheram_bank* b, const int64_t* const* ggsw, int n_ggsw, int bits, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_selector* s = nullptr;
    int rc = selector_create_args(b, ggsw, out);
    if (rc == FHERAM_OK) rc = selector_new(b, bits, &s, FHERAM_TABLE_BITS_MAX, "FHERAM_TABLE_BITS_MAX");
    if (rc != FHERAM_OK) return rc;
    return selector_fill(b, s, ggsw, n_ggsw, "a selector of " + std::to_string(bits) + " bits has " + std::to_string(s->n_digits) + " digits, not " + std::to_string(n_ggsw), out);
}
int fheram_bank_table_selector_alloc_fields(fheram_bank* b, const int* widths, int n_fields, fheram_selector** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    *out = nullptr;
    return selector_new_fields(b, widths, n_fields, out, FHERAM_TABLE_BITS_MAX, "FHERAM_TABLE_BITS_MAX");
}

}  // extern "C"
#endif   // FK_TABLE_KERNELS_ONLY

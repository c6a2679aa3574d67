// A bank's PUBLIC side: data put in and taken out at places everybody knows — a program or data image loaded as public bytes, one word
// read (peek) or written (poke) at a PUBLIC address.  The server that hosts a bank has no secret key; with a public address there is
// nothing to hide, so none of this pays an oblivious operation's row chains over every row.
//
// CONTRACT-COMPATIBLE ONLY, as the select, the register file and the tables are (select.hpp, regs.hpp, table.hpp): with a
// public address a = r * N + q the reference's operations collapse to row r.
//   load_plain  public bytes as the trivial ciphertexts Ram::encrypt_sk's encoding gives with all-zero mask and noise, the rule of
//               fheram_bank_table_load_plain, for a member's rows [first_row, first_row + n_rows) or a register file's row: the bytes
//               staged row by row into a pinned buffer, one copy, ONE launch (k_rows_plain).  No int64 image crosses the host boundary.
//   peek        out_k[y] = trace(0, log N)( glwe_rotate(-q_k, rows[member_k][y][r_k]) ): Ram::read (ram.rs:451,457) without the products.
//               ONE gather launch (k_peek_gather) for the n * ws rotated ciphertexts, then ONE trace over all of them through
//               trace_steps, in the form the bank's configuration selects (the tail launch up to 8 ciphertexts).  Changes nothing but
//               the public side's own result buffer.
//   poke        every touched row ciphertext R <- normalize(R - sum_j glwe_rotate(+q_j, t_j) + sum_j glwe_rotate(+q_j, w_j[y])) over the
//               entries j of that row, t_j = the peek of entry j: write_first_step's normalize(a - b + c) (ram.rs:574-576) on that one
//               row.  The peek's gather and trace, then ONE launch (k_poke_merge).  All entries see the rows as they were before the call.
//   regs        fheram_bank_regs_peek / _poke: the same on a register file's one row (narrow or wide, regs.hpp): word i is coefficient i of
//               row 0 of the one-row RAM.  An entry is a PLACE (PubPlace: the row, the stride between its word ciphertexts, the
//               coefficient), and pub_peek / pub_poke run the members' and the register file's entries alike.
// Everything runs on the bank's main stream.  The public side's buffers (path.hpp PublicBufs) are allocated whole by the first call that
// needs them and freed with the bank; no later operation allocates.  The outputs of the last peek or poke are the source kind
// FHERAM_SRC_PEEK_RESULT.  There are TWO result buffers: an operation writes the one that does not hold the last outputs, so a poke
// may take its words from the peek before it.
//
// This file has two parts: what public_io.hip (the kernels' translation unit) and fheram.hip share — the argument structs and the
// launchers — and, for fheram.hip only, the host logic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int PUB_SLICES = 8;      // workgroups per ciphertext (blockIdx.z), as the elementwise kernels (launch.hpp EW_SLICES)
constexpr int PUB_CT_MAX = 64;     // ciphertexts of one peek or poke: n * ws
constexpr int PUB_MAX = 16;        // entries of one peek or poke (FHERAM_PEEK_MAX)
struct RowsPlainArgs {
    const uint8_t* data;           // [n_words * ws] bytes: byte w of word j at data[j * ws + w]; word 0 is coefficient 0 of row 0 of the launch
    int32_t* rows;                 // row x of word ciphertext w at rows + w * w_stride + x * GLWE (3 limbs)
    long w_stride;                 // int32 elements between the word ciphertexts of one row: the member's rows * GLWE
    int ws;
    long n_words;                  // <= gridDim.x * N: coefficients behind it are zero padding (a ragged last row)
    int k_pt, size_pt;             // the plaintext precision and its limbs (setup.hpp encode_value)
};
struct PeekGatherArgs {            // by value: no table in device memory, nothing to stage
    const int32_t* src[PUB_CT_MAX];    // output ciphertext y = k * ws + w: row r_k of word ciphertext w of members[k], ONE GLWE (3 limbs)
    int q[PUB_CT_MAX];                 // out[y] = glwe_rotate(-q[y], *src[y]), 0 <= q < N
    int32_t* out;                      // [n * ws] GLWE
};
struct PokeMergeArgs {             // by value, as k_mix_scatter's
    int32_t* row[PUB_MAX];             // touched row g: its word ciphertext 0; word ciphertext w is w * w_stride further.  In place.
    int first[PUB_MAX + 1];            // its entries: [first[g], first[g + 1])
    const int32_t* t[PUB_MAX];         // entry j: its peek, ws GLWEs one GLWE apart
    const int32_t* w[PUB_MAX];         // entry j: the written word, ws GLWEs one GLWE apart; nullptr: the all-zero ciphertexts
    int q[PUB_MAX];                    // entry j: its coefficient, 0 <= q < N
    long w_stride;
};
// grid: (n_rows, ws, PUB_SLICES) / (1, n_ct, PUB_SLICES) / (n_touched, ws, PUB_SLICES)
void rows_plain_launch(int n_rows, hipStream_t stream, const RowsPlainArgs& ra);
void peek_gather_launch(int n_ct, hipStream_t stream, const PeekGatherArgs& ga);
void poke_merge_launch(int n_touched, int ws, hipStream_t stream, const PokeMergeArgs& ma);

}  // namespace fk

#ifndef FK_PUBLIC_KERNELS_ONLY
#include "table.hpp"

namespace {

static_assert(PUB_SLICES == EW_SLICES && PUB_CT_MAX == 64 && PUB_MAX == FHERAM_PEEK_MAX, "the public kernels cover a ciphertext as the elementwise kernels do; a call has at most 64 ciphertexts");

// the public side's buffers, whole (path.hpp PublicBufs)
int pub_reserve(fheram_bank* b) {
    fheram_ctx* c = b->c;
    if (b->pub.cap) return FHERAM_OK;
    PublicBufs nw;
    nw.cap = std::min(PUB_MAX * b->mws, PUB_CT_MAX);
    const size_t ct = (size_t)nw.cap * fheram_ctx::GLWE * sizeof(int32_t);
    const size_t host = (size_t)PUB_MAX * b->mws * fheram_ctx::GLWE * sizeof(int32_t);
    const size_t data = (size_t)c->rows * N * b->mws;   // one member's bytes, the ragged last row padded (a register file's row is no longer)
    hipError_t e = hipSuccess;
    auto dev = [&](auto** p, size_t bytes) {
        if (e != hipSuccess) return;
        if (b->pub_fail_alloc > 0 && --b->pub_fail_alloc == 0) e = hipErrorOutOfMemory;   // (as the runtime reports an exhausted device)
        else e = hipMalloc((void**)p, bytes);
    };
    for (int32_t** p : {&nw.fan, &nw.tmp, &nw.res[0], &nw.res[1]}) dev(p, ct);
    dev(&nw.host.d, host);
    dev(&nw.data.d, data);
    if (e == hipSuccess) e = pinned_result(&nw.h_res, &nw.d_h_res, ct);
    if (e == hipSuccess) e = nw.host.pin(host);
    if (e == hipSuccess) e = nw.data.pin(data);
    if (e == hipSuccess) e = nw.host.event();
    if (e == hipSuccess) e = nw.data.event();
    if (e != hipSuccess) { public_bufs_free(nw); return reserve_failed(c, e, "buffers of the bank's public side"); }
    b->pub = nw;
    return FHERAM_OK;
}
// a member's rows are as an upload leaves them: whatever an earlier operation kept of them is void
void pub_rows_changed(fheram_bank* b, int member) {
    RamState& r = b->ram[member];
    r.memo_top = false; r.memo_alone = 0;
    b->wl_holds[member] = false;
}
int pub_check_plain(fheram_ctx* c) {
    const int k_pt = (int)c->p.k_glwe_pt, size_pt = (k_pt + BASE2K - 1) / BASE2K;
    if (k_pt <= 0 || k_pt > 8 + BASE2K || size_pt > fheram_ctx::S_CT) return fail(c, FHERAM_ERR_UNSUPPORTED, "k_glwe_pt out of range");   // (as fheram_ram_encrypt_sk)
    return FHERAM_OK;
}
// n_words words of public bytes into n_rows rows from `rows` on: staged row by row (the ragged last row zero-padded), one copy, one launch
int pub_load_rows(fheram_bank* b, int32_t* rows, long w_stride, int n_rows, size_t n_words, const uint8_t* data) {
    fheram_ctx* c = b->c;
    PublicBufs& P = b->pub;
    const size_t row_bytes = (size_t)N * b->mws, have = n_words * (size_t)b->mws, all = (size_t)n_rows * row_bytes;
    int rc = stage_wait(c, P.data);
    if (rc != FHERAM_OK) return rc;
    for (size_t o = 0; o < all; o += row_bytes) {
        const size_t n = o < have ? std::min(row_bytes, have - o) : 0;
        if (n) std::memcpy(P.data.h + o, data + o, n);
        if (n < row_bytes) std::memset(P.data.h + o + n, 0, row_bytes - n);
    }
    // ---- enqueue ----
    main_enqueued(c);
    c->cur = c->stream;
    HIPCHK(c, hipMemcpyAsync(P.data.d, P.data.h, all, hipMemcpyHostToDevice, c->stream));
    rc = stage_record(c, P.data);
    if (rc != FHERAM_OK) return rc;
    {
        const int k_pt = (int)c->p.k_glwe_pt;
        const RowsPlainArgs ra{P.data.d, rows, w_stride, b->mws, (long)n_words, k_pt, (k_pt + BASE2K - 1) / BASE2K};
        ProfScope ps(c, "elementwise", (uint64_t)n_rows * b->mws);
        rows_plain_launch(n_rows, c->cur, ra);
    }
    HIPCHK(c, hipGetLastError());
    return FHERAM_OK;
}
// the entries of a peek or a poke: n, every member and address, then what the members must be (as bank.hpp members_ready, want_state 0)
int pub_check_entries(fheram_bank* b, const int* members, const uint64_t* addrs, int n, const char* who) {
    fheram_ctx* c = b->c;
    if (n < 1 || n > PUB_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_PEEK_MAX = " + std::to_string(PUB_MAX) + "]");
    if ((long)n * b->mws > PUB_CT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n * word_size = " + std::to_string((long)n * b->mws) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    for (int k = 0; k < n; k++) {
        if (members[k] < 0 || members[k] >= b->M)
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names member " + std::to_string(members[k]) + ", outside the bank's " + std::to_string(b->M) + " members");
        if (addrs[k] >= (uint64_t)c->p.max_addr)
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names address " + std::to_string(addrs[k]) + ", outside max_addr = " + std::to_string(c->p.max_addr));
    }
    for (int k = 0; k < n; k++)
        if (!b->ram[members[k]].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (member " + std::to_string(members[k]) + ")");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int k = 0; k < n; k++)
        if (b->ram[members[k]].state)
            return fail(c, FHERAM_ERR_STATE, std::string("invalid call to ") + who + ": the member is between read_prepare_write and write, its rows are rotated (member " + std::to_string(members[k]) + ")");
    return FHERAM_OK;
}
// row r of word ciphertext w of a member
int32_t* pub_row(const fheram_bank* b, int member, size_t r, int w) {
    const fheram_ctx* c = b->c;
    return c->d_data + (((size_t)member * b->mws + (size_t)w) * c->rows + r) * fheram_ctx::GLWE;
}
// where an entry of a peek or a poke sits: word ciphertext 0 of its row (word ciphertext w is w * w_stride further) and its coefficient.
// A member's entry at address a: row a / N, coefficient a % N; a register file's entry at word i: its one row, coefficient i.
struct PubPlace { int32_t* row0; long w_stride; int q; };
void pub_member_places(const fheram_bank* b, const int* members, const uint64_t* addrs, int n, PubPlace* at) {
    for (int k = 0; k < n; k++) at[k] = PubPlace{pub_row(b, members[k], (size_t)(addrs[k] / N), 0), (long)(b->c->rows * fheram_ctx::GLWE), (int)(addrs[k] % N)};
}
void pub_regs_places(const fheram_regs* r, const uint32_t* idx, int n, PubPlace* at) {
    for (int k = 0; k < n; k++) at[k] = PubPlace{r->row, (long)fheram_ctx::GLWE, (int)idx[k]};
}
// the entries of a register file's peek or poke, in the order of pub_check_entries: n, every index, then what the register file must be
int pub_check_regs_entries(fheram_bank* b, const fheram_regs* r, const uint32_t* idx, int n, const char* who) {
    fheram_ctx* c = b->c;
    if (n < 1 || n > PUB_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_PEEK_MAX = " + std::to_string(PUB_MAX) + "]");
    if ((long)n * b->mws > PUB_CT_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n * word_size = " + std::to_string((long)n * b->mws) + " exceeds 64, the ciphertext limit of the single-launch chains (k_chain_mid)");
    for (int k = 0; k < n; k++)
        if (idx[k] >= ((uint32_t)1 << r->bits))
            return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names word " + std::to_string(idx[k]) + ", outside the register file's 2^bits = " + std::to_string(1 << r->bits) + " words");
    if (!r->initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: the register file has had no fheram_bank_regs_upload or fheram_bank_regs_pack");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    if (r->state)
        return fail(c, FHERAM_ERR_STATE, std::string("invalid call to ") + who + ": the register file is between read_prepare_write and write, its row is rotated");
    return FHERAM_OK;
}
// gather + trace of the n entries into the result buffer that does not hold the last outputs; returns it (the caller makes it the last)
int32_t* pub_peek_enqueue(fheram_bank* b, const PubPlace* at, int n) {
    fheram_ctx* c = b->c;
    PublicBufs& P = b->pub;
    const int ws = b->mws, Y = n * ws;
    const long G = (long)fheram_ctx::GLWE;
    int32_t* res = P.res[P.cur ^ 1];
    {
        PeekGatherArgs ga{};
        ga.out = P.fan;
        for (int k = 0; k < n; k++)
            for (int w = 0; w < ws; w++) {
                ga.src[k * ws + w] = at[k].row0 + (long)w * at[k].w_stride;
                ga.q[k * ws + w] = at[k].q;
            }
        ProfScope ps(c, "elementwise", (uint64_t)Y);
        peek_gather_launch(Y, c->cur, ga);
    }
    trace_steps(c, ref(P.fan, G, 0), ref(res, G, 0), ref(P.tmp, G, 0), 0, LOGN, 1, Y);   // ram.rs:457
    return res;
}
void pub_peek_done(fheram_bank* b, int n) {
    PublicBufs& P = b->pub;
    P.cur ^= 1;
    b->last[LAST_PEEK] = LastOutputs{n, ResHome{P.res[P.cur], P.h_res, P.d_h_res, -1}};
}
// behind the checks and pub_reserve: the peek of the n entries, enqueued and exported
int pub_peek(fheram_bank* b, const PubPlace* at, int n, int64_t* out) {
    fheram_ctx* c = b->c;
    // ---- enqueue ----
    regs_begin(c);
    const int32_t* res = pub_peek_enqueue(b, at, n);
    HIPCHK(c, hipGetLastError());
    pub_peek_done(b, n);
    if (!out) return FHERAM_OK;
    const ResRun run{res, (size_t)n * b->mws * fheram_ctx::GLWE};
    return result_export(c, &run, 1, b->pub.h_res, b->pub.d_h_res, out);
}
// behind the checks and pub_reserve: the poke of the n entries (distinct places; n_host: sources_check's).  The caller voids what was kept
// of the touched rows.
int pub_poke(fheram_bank* b, const PubPlace* at, int n, const fheram_select_src* srcs, int n_host, const int64_t* host_words) {
    fheram_ctx* c = b->c;
    PublicBufs& P = b->pub;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    int rc = host_words_stage(b, P.host, srcs, n, n_host, host_words);
    if (rc != FHERAM_OK) return rc;
    // ---- enqueue ----
    regs_begin(c);
    rc = host_words_copy(b, P.host, srcs, n, n_host);
    if (rc != FHERAM_OK) return rc;
    PokeMergeArgs ma{};
    // the words, where they sit NOW: a PEEK_RESULT source names the outputs this call's own peek is about to succeed
    const int32_t* words[PUB_MAX];
    for (int k = 0; k < n; k++) words[k] = select_source(b, srcs[k], P.host.dev<int32_t>());
    const int32_t* t = pub_peek_enqueue(b, at, n);
    // the touched rows, each with its entries side by side
    int n_touched = 0, n_ent = 0;
    bool placed[PUB_MAX] = {};
    for (int k = 0; k < n; k++) {
        if (placed[k]) continue;
        ma.row[n_touched] = at[k].row0;
        ma.first[n_touched++] = n_ent;
        for (int j = k; j < n; j++) {
            if (placed[j] || at[j].row0 != at[k].row0) continue;
            placed[j] = true;
            ma.t[n_ent] = t + (size_t)j * per;
            ma.w[n_ent] = words[j];
            ma.q[n_ent++] = at[j].q;
        }
    }
    ma.first[n_touched] = n_ent;
    ma.w_stride = at[0].w_stride;   // (one call's entries are all members' or all one register file's)
    {
        ProfScope ps(c, "elementwise", (uint64_t)n_touched * b->mws);
        poke_merge_launch(n_touched, b->mws, c->cur, ma);
    }
    HIPCHK(c, hipGetLastError());
    pub_peek_done(b, n);   // the OLD words, as read_prepare_write returns them
    return FHERAM_OK;
}

}  // namespace

extern "C" {

int fheram_bank_ram_load_plain(fheram_bank* b, int member, size_t first_row, size_t n_rows, const uint8_t* data, size_t data_len) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (member < 0 || member >= b->M) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member");
    if (!data) return fail(c, FHERAM_ERR_INVALID_ARG, "null data");
    if (n_rows < 1 || first_row >= c->rows || n_rows > c->rows - first_row)
        return fail(c, FHERAM_ERR_INVALID_ARG, "rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " + std::to_string(n_rows) + ") are empty or outside the member's " + std::to_string(c->rows) + " rows");
    const size_t n_words = std::min((size_t)c->p.max_addr, (first_row + n_rows) * N) - first_row * N, want = n_words * (size_t)b->mws;
    if (data_len != want)
        return fail(c, FHERAM_ERR_INVALID_ARG, "invalid data: data_len = " + std::to_string(data_len) + ", rows [" + std::to_string(first_row) + ", " + std::to_string(first_row + n_rows) + ") hold " + std::to_string(n_words) + " words of word_size bytes = " + std::to_string(want) + " bytes");
    int rc = pub_check_plain(c);
    if (rc != FHERAM_OK) return rc;
    RamState& r = b->ram[member];
    const bool whole = first_row == 0 && n_rows == c->rows;
    if (!whole) {   // a row range: the other rows must be there, and not rotated
        if (!r.initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (a row range is loaded into a member that has rows)");
        if (r.state) return fail(c, FHERAM_ERR_STATE, "the member is between read_prepare_write and write: its rows are rotated (a whole-member load resets)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    rc = pub_reserve(b);
    if (rc != FHERAM_OK) return rc;
    rc = pub_load_rows(b, pub_row(b, member, first_row, 0), (long)(c->rows * fheram_ctx::GLWE), (int)n_rows, n_words, data);
    if (rc != FHERAM_OK) return rc;
    r.initialized = true; r.state = false;   // as fheram_bank_ram_upload
    pub_rows_changed(b, member);
    return FHERAM_OK;
}
int fheram_bank_regs_load_plain(fheram_bank* b, fheram_regs* r, const uint8_t* data, size_t data_len) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc != FHERAM_OK) return rc;
    if (!data) return fail(c, FHERAM_ERR_INVALID_ARG, "null data");
    const size_t n_words = (size_t)1 << r->bits, want = n_words * (size_t)b->mws;
    if (data_len != want)
        return fail(c, FHERAM_ERR_INVALID_ARG, "invalid data: data_len = " + std::to_string(data_len) + ", a register file of " + std::to_string(r->bits) + " bits takes 2^bits * word_size = " + std::to_string(want) + " bytes");
    rc = pub_check_plain(c);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = pub_reserve(b);
    if (rc != FHERAM_OK) return rc;
    rc = pub_load_rows(b, r->row, (long)fheram_ctx::GLWE, 1, n_words, data);
    if (rc != FHERAM_OK) return rc;
    r->initialized = true; r->state = false; r->memo = false;   // as fheram_bank_regs_upload
    return FHERAM_OK;
}

int fheram_bank_peek(fheram_bank* b, const int* members, const uint64_t* addrs, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (!members || !addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null member list or null address list");
    int rc = pub_check_entries(b, members, addrs, n, "fheram_bank_peek");
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = pub_reserve(b);
    if (rc != FHERAM_OK) return rc;
    PubPlace at[PUB_MAX];
    pub_member_places(b, members, addrs, n, at);
    return pub_peek(b, at, n, out);
}
int fheram_bank_selftest_fail_public_alloc(fheram_bank* b, int nth) {
    if (!b || nth < 0) return FHERAM_ERR_INVALID_ARG;
    b->pub_fail_alloc = nth;
    return FHERAM_OK;
}
int fheram_bank_peek_result(fheram_bank* b, int first, int n, int64_t* out) {
    return b ? last_result(b, LAST_PEEK, first, n, out) : FHERAM_ERR_INVALID_ARG;
}
int fheram_bank_poke(fheram_bank* b, const int* members, const uint64_t* addrs, int n, const fheram_select_src* srcs, const int64_t* host_words) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    if (!members || !addrs || !srcs) return fail(c, FHERAM_ERR_INVALID_ARG, "null member list, null address list or null sources");
    int rc = pub_check_entries(b, members, addrs, n, "fheram_bank_poke");
    if (rc != FHERAM_OK) return rc;
    for (int k = 0; k < n; k++)
        for (int j = 0; j < k; j++)
            if (members[j] == members[k] && addrs[j] == addrs[k])
                return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names address " + std::to_string(addrs[k]) + " of member " + std::to_string(members[k]) + " a second time: the targets of a poke are distinct");
    int n_host = 0;
    rc = sources_check(b, srcs, n, host_words, PUB_MAX, "a poke takes", true, &n_host);   // the public side stages PUB_MAX host slots
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = pub_reserve(b);
    if (rc != FHERAM_OK) return rc;
    PubPlace at[PUB_MAX];
    pub_member_places(b, members, addrs, n, at);
    rc = pub_poke(b, at, n, srcs, n_host, host_words);
    if (rc != FHERAM_OK) return rc;
    for (int k = 0; k < n; k++) pub_rows_changed(b, members[k]);
    return FHERAM_OK;
}
// The register file's twins: word idx[k] of the one row is coefficient idx[k] of row 0 of the one-row RAM, so the same gather, trace and
// merge run with the row's pointer — ONE touched row for a poke, whatever n is.
int fheram_bank_regs_peek(fheram_bank* b, const fheram_regs* r, const uint32_t* idx, int n, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc != FHERAM_OK) return rc;
    if (!idx) return fail(c, FHERAM_ERR_INVALID_ARG, "null index list");
    rc = pub_check_regs_entries(b, r, idx, n, "fheram_bank_regs_peek");
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = pub_reserve(b);
    if (rc != FHERAM_OK) return rc;
    PubPlace at[PUB_MAX];
    pub_regs_places(r, idx, n, at);
    return pub_peek(b, at, n, out);
}
int fheram_bank_regs_poke(fheram_bank* b, fheram_regs* r, const uint32_t* idx, int n, const fheram_select_src* srcs, const int64_t* host_words) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    // ---- every check before anything is enqueued: a refused call changes nothing ----
    int rc = regs_check_handle(b, r);
    if (rc != FHERAM_OK) return rc;
    if (!idx || !srcs) return fail(c, FHERAM_ERR_INVALID_ARG, "null index list or null sources");
    rc = pub_check_regs_entries(b, r, idx, n, "fheram_bank_regs_poke");
    if (rc != FHERAM_OK) return rc;
    for (int k = 0; k < n; k++)
        for (int j = 0; j < k; j++)
            if (idx[j] == idx[k])
                return fail(c, FHERAM_ERR_INVALID_ARG, "entry " + std::to_string(k) + " names word " + std::to_string(idx[k]) + " a second time: the targets of a poke are distinct");
    int n_host = 0;
    rc = sources_check(b, srcs, n, host_words, PUB_MAX, "a poke takes", true, &n_host);   // the public side stages PUB_MAX host slots
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = pub_reserve(b);
    if (rc != FHERAM_OK) return rc;
    PubPlace at[PUB_MAX];
    pub_regs_places(r, idx, n, at);
    rc = pub_poke(b, at, n, srcs, n_host, host_words);
    if (rc != FHERAM_OK) return rc;
    r->memo = false;   // the kept trace was of the row before the poke
    return FHERAM_OK;
}

}  // extern "C"
#endif   // FK_PUBLIC_KERNELS_ONLY

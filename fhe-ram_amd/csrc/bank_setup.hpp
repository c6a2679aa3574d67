// Included by fheram.hip (same translation unit): the SETUP SIDE of a bank — what setup.hpp is to a context.  With it a
// bank is usable on its own: its keys, members, register files, tables, addresses, selectors and encrypted integers are encrypted on the
// device from host-drawn randomness (sampling stays on the host, include/fheram.h "Setup side on the device"), and what it leaves on the
// device is decrypted and decoded there.
//   handles     fheram_bank_secret_create, _keys_encrypt_sk, _address_encrypt_sk, _fheuint_encrypt_sk, _glwe_encrypt_sk, _glwe_decrypt:
//               the context's calls on the bank's context (keys: and what fheram_bank_keys_load voids)
//   rows        fheram_bank_ram_encrypt_sk (one member), _regs_encrypt_sk, _table_encrypt_sk (the one-row RAM of max_addr = 2^bits):
//               setup.hpp's ram_encrypt_body, straight into the rows
//   selectors   fheram_bank_selector_encrypt_sk: setup.hpp's digits_encrypt_body over the plan the handle stores, in place
//   decrypt     k_decrypt_decode (decrypt_decode.hip): fheram_bank_source_decrypt (coefficient 0 of n words named as a select's
//               candidates are), fheram_bank_ram_decrypt / _regs_decrypt / _table_decrypt (every data coefficient of every row)
// Every call waits for the device, as the context's setup calls do: both streams are idle before anything is written or read, and again
// when the call returns.  Every check runs before anything is enqueued or staged; a refused call changes nothing.  The decrypting calls
// read the ciphertexts through const pointers: no result buffer, row, state flag or memo changes.
#pragma once
#include "table.hpp"
#include "decrypt_decode.hpp"

namespace {

// both streams idle: whatever still reads or writes the bank's buffers is over
int bank_quiesce(fheram_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    return FHERAM_OK;
}
int bank_check_secret(fheram_ctx* c, const fheram_secret* sk) {
    if (!sk || sk->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "secret belongs to another context");
    return FHERAM_OK;
}
// the one-row RAM of max_addr = 2^bits a register file or a table is (regs.hpp, table.hpp)
int one_row_encrypt(fheram_bank* b, int bits, int32_t* row, const fheram_secret* sk, const uint8_t* data, size_t data_len, const int64_t* mask, const int64_t* noise) {
    fheram_ctx* c = b->c;
    if (!data || !mask || !noise) return fail(c, FHERAM_ERR_INVALID_ARG, "null argument");
    int rc = bank_check_secret(c, sk);
    if (rc == FHERAM_OK) rc = bank_quiesce(c);
    if (rc != FHERAM_OK) return rc;
    return ram_encrypt_body(c, sk, data, data_len, mask, noise, RamShape{(size_t)b->mws, 1, (size_t)1 << bits, 0, 1}, row, true);
}
// what the decrypting calls share: the precisions k_decrypt_decode decodes with
int decrypt_check(fheram_ctx* c, const fheram_secret* sk) {
    const int rc = bank_check_secret(c, sk);
    if (rc != FHERAM_OK) return rc;
    if (c->p.k_glwe_pt > 30) return fail(c, FHERAM_ERR_UNSUPPORTED, "k_glwe_pt above 30: a decoded value does not fit the kernel's int32");
    return FHERAM_OK;
}
double log2_noise_of(int64_t abs_diff, int k) { return std::log2((double)abs_diff) - (double)k; }   // examples/fhe-ram.rs:231 (-inf for 0)

// Every data coefficient of the rows [ws][rows][GLWE] at d_rows of a RAM of max_addr words: values [max_addr][ws] int32 in the interleaved
// order of Ram::encrypt_sk's data, worst (optional): max over the data coefficients of log2|diff| - k against each coefficient's own value.
// One launch per word and up to DECRYPT_ROWS_MAX rows into a device staging buffer, one copy into the context's pinned buffer, the
// interleave on the host.  Device memory: the staging buffer, allocated and freed here.
int rows_decrypt(fheram_ctx* c, const fheram_secret* sk, const int32_t* d_rows, size_t ws, size_t rows, size_t max_addr, int32_t* values, double* worst) {
    int rc = bank_quiesce(c);
    if (rc == FHERAM_OK) rc = pin_init(c);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, decrypt_decode_register());
    const size_t CH = DECRYPT_ROWS_MAX, n_stage = std::min(CH, rows);
    static_assert((size_t)DECRYPT_ROWS_MAX * N + 2 * DECRYPT_ROWS_MAX <= PIN_CHUNK, "a launch's values and maxima fit one pinned staging buffer");
    int32_t* d_val = nullptr;
    HIPCHK(c, hipMalloc((void**)&d_val, n_stage * N * sizeof(int32_t) + n_stage * sizeof(long long)));
    long long* d_max = reinterpret_cast<long long*>(d_val + n_stage * N);
    int64_t top = 0;
    hipError_t e = hipSuccess;
    c->cur = c->stream;
    for (size_t w = 0; w < ws && e == hipSuccess; w++)
        for (size_t x0 = 0; x0 < rows && e == hipSuccess; x0 += CH) {
            const size_t nx = std::min(CH, rows - x0);
            DecryptDecodeArgs da{};
            da.base = d_rows + (w * rows + x0) * fheram_ctx::GLWE;
            da.s_hat = sk->d_hat; da.tw = c->d_tw;
            da.k = (int)c->p.k_glwe_ct; da.k_pt = (int)c->p.k_glwe_pt;
            da.n_coef = N;
            da.n_coef_last = (int)std::min((size_t)N, max_addr - (x0 + nx - 1) * N);   // the ragged last row: its padding is skipped
            da.values = d_val; da.max_diff = d_max;
            {
                ProfScope ps(c, "decrypt_decode", (uint64_t)nx);
                decrypt_decode_launch((int)nx, c->cur, da);
            }
            int32_t* h = c->h_pin[0];
            e = hipMemcpyAsync(h, d_val, n_stage * N * sizeof(int32_t) + n_stage * sizeof(long long), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) break;
            const long long* h_max = reinterpret_cast<const long long*>(h + n_stage * N);
            for (size_t x = 0; x < nx; x++) {
                const size_t a0 = (x0 + x) * N, cnt = std::min((size_t)N, max_addr - a0);
                for (size_t q = 0; q < cnt; q++) values[(a0 + q) * ws + w] = h[x * N + q];
                top = std::max(top, (int64_t)h_max[x]);
            }
        }
    if (e == hipSuccess) e = hipGetLastError();
    hipFree(d_val);
    if (e != hipSuccess) return fail(c, FHERAM_ERR_DEVICE, std::string("k_decrypt_decode: ") + hipGetErrorString(e));
    if (worst) *worst = log2_noise_of(top, (int)c->p.k_glwe_ct);
    return check_precision(c);
}

}  // namespace

extern "C" {

// ---- handles that forward to the bank's context -----------------------------------------------------------------------------------------
int fheram_bank_secret_create(fheram_bank* b, const int64_t* sk, fheram_secret** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_secret_create(b->c, sk, out);
}
int fheram_bank_keys_encrypt_sk(fheram_bank* b, const fheram_secret* sk, const int64_t* mask, const int64_t* noise, int64_t* std_out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    const int rc = fheram_keys_encrypt_sk(b->c, sk, mask, noise, std_out);
    if (rc != FHERAM_OK) return rc;
    for (int m = 0; m < b->M; m++) { b->ram[m].memo_top = false; b->ram[m].memo_alone = 0; b->wl_holds[m] = false; }   // as fheram_bank_keys_load
    regs_keys_changed(b);
    return FHERAM_OK;
}
int fheram_bank_address_encrypt_sk(fheram_bank* b, const fheram_secret* sk, uint32_t value, const int64_t* mask, const int64_t* noise, fheram_addr** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_address_encrypt_sk(b->c, sk, value, mask, noise, out);
}
int fheram_bank_fheuint_encrypt_sk(fheram_bank* b, const fheram_secret* sk, uint32_t value, int n_bits, const int64_t* mask, const int64_t* noise, fheram_fheuint** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_fheuint_encrypt_sk(b->c, sk, value, n_bits, mask, noise, out);
}
int fheram_bank_glwe_encrypt_sk(fheram_bank* b, const fheram_secret* sk, int n_glwe, int size, int k, const int64_t* pt, int pt_size, int pt_col,
                                const int64_t* mask, const int64_t* noise, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_glwe_encrypt_sk(b->c, sk, n_glwe, size, k, pt, pt_size, pt_col, mask, noise, out);
}
int fheram_bank_glwe_decrypt(fheram_bank* b, const fheram_secret* sk, int n_glwe, int size, const int64_t* ct, int64_t* pt) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_glwe_decrypt(b->c, sk, n_glwe, size, ct, pt);
}

// ---- rows encrypted straight into the bank ------------------------------------------------------------------------------------------------
int fheram_bank_ram_encrypt_sk(fheram_bank* b, int member, const fheram_secret* sk, const uint8_t* data, size_t data_len, const int64_t* mask, const int64_t* noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (member < 0 || member >= b->M) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member");
    if (!data || !mask || !noise) return fail(c, FHERAM_ERR_INVALID_ARG, "null argument");
    int rc = bank_check_secret(c, sk);
    if (rc == FHERAM_OK) rc = bank_quiesce(c);
    if (rc != FHERAM_OK) return rc;
    // (the context's word count is M * mws: the member's shape is the bank's fheram_params)
    const size_t per = (size_t)b->mws * c->rows * fheram_ctx::GLWE;
    rc = ram_encrypt_body(c, sk, data, data_len, mask, noise, RamShape{(size_t)b->mws, c->rows, (size_t)c->p.max_addr, 0, 1}, c->d_data + (size_t)member * per, true);
    if (rc != FHERAM_OK) return rc;
    RamState& r = b->ram[member];   // as fheram_bank_ram_upload
    r.initialized = true; r.state = false; r.memo_top = false; r.memo_alone = 0;
    b->wl_holds[member] = false;
    return FHERAM_OK;
}
int fheram_bank_regs_encrypt_sk(fheram_bank* b, fheram_regs* r, const fheram_secret* sk, const uint8_t* data, size_t data_len, const int64_t* mask, const int64_t* noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    int rc = regs_check_handle(b, r);
    if (rc == FHERAM_OK) rc = one_row_encrypt(b, r->bits, r->row, sk, data, data_len, mask, noise);
    if (rc != FHERAM_OK) return rc;
    r->initialized = true; r->state = false; r->memo = false;   // as fheram_bank_regs_upload
    return FHERAM_OK;
}
int fheram_bank_table_encrypt_sk(fheram_bank* b, fheram_table* t, const fheram_secret* sk, const uint8_t* data, size_t data_len, const int64_t* mask, const int64_t* noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    int rc = table_check_handle(b, t, "the table");
    if (rc == FHERAM_OK) rc = one_row_encrypt(b, t->bits, t->row, sk, data, data_len, mask, noise);
    if (rc != FHERAM_OK) return rc;
    t->initialized = true;   // as fheram_bank_table_upload
    return FHERAM_OK;
}

// ---- selectors encrypted in place ---------------------------------------------------------------------------------------------------------
int fheram_bank_selector_encrypt_sk(fheram_bank* b, const fheram_secret* sk, fheram_selector* sel, uint32_t value, const int64_t* mask, const int64_t* noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!sel || sel->bank != b) return fail(c, FHERAM_ERR_INVALID_ARG, "selector is null or belongs to another bank");
    if (!mask || !noise) return fail(c, FHERAM_ERR_INVALID_ARG, "null argument");
    int rc = check_setup_args(c, sk, fheram_ctx::S_ADDR, (int)c->p.k_ggsw_addr);
    if (rc != FHERAM_OK) return rc;
    if (((uint64_t)value >> sel->bits) != 0)   // debug_assert!(self.base2d.max() > value) (address.rs:98)
        return fail(c, FHERAM_ERR_INVALID_ARG, "self.base2d.max() > value (address.rs:98): address does not fit the digit plan");
    {   // every draw, before a digit is overwritten
        int64_t bad = 0;
        const size_t n_noise = (size_t)sel->n_digits * fheram_ctx::DNUM_CT * 2 * N, n_mask = n_noise * fheram_ctx::S_ADDR;
        for (size_t i = 0; i < n_mask; i++) bad |= (mask[i] > 65535) | (mask[i] < -65536);
        for (size_t i = 0; i < n_noise; i++) bad |= (noise[i] >= NOISE_LIM) | (noise[i] <= -NOISE_LIM);
        if (bad) return fail(c, FHERAM_ERR_RANGE, "mask limb outside [-2^16, 2^16) or |noise| >= 2^30");
    }
    rc = bank_quiesce(c);
    if (rc != FHERAM_OK) return rc;
    DigitPlan pl;   // the plan the handle stores: one coordinate of `bits` bits
    pl.n_digits = sel->n_digits;
    for (int d = 0; d < sel->n_digits; d++) {
        pl.rsh[d] = sel->rsh[d]; pl.width[d] = sel->width[d]; pl.lsh[d] = sel->lsh[d];
        pl.coord_rsh[d] = 0; pl.coord_bits[d] = (unsigned char)sel->bits;
    }
    rc = digits_encrypt_body(c, sk, value, pl, mask, noise, sel->d_ggsw);
    if (rc != FHERAM_OK) return rc;
    sel->empty = false;
    return FHERAM_OK;
}

// ---- decrypt and decode on the device -----------------------------------------------------------------------------------------------------
int fheram_bank_source_decrypt(fheram_bank* b, const fheram_secret* sk, const fheram_select_src* srcs, int n, const int64_t* want, int64_t* values, double* log2_noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!srcs || !values) return fail(c, FHERAM_ERR_INVALID_ARG, "null sources or null values");
    const int ws = b->mws;
    if (n < 1 || (long)n * ws > DECRYPT_SRC_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + ": n * word_size is outside [1, 64]");
    int rc = decrypt_check(c, sk);
    if (rc != FHERAM_OK) return rc;
    unsigned need = 0;
    for (int i = 0; i < n; i++) {
        const std::string who = "source " + std::to_string(i);
        if (srcs[i].kind == FHERAM_SRC_HOST || srcs[i].kind == FHERAM_SRC_ZERO)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " is a host word or the zero word: there is nothing on the device to decrypt");
        rc = select_check_source(b, srcs[i].kind, srcs[i].index, who, nullptr, need);
        if (rc != FHERAM_OK) return rc;
    }
    rc = select_check_state(b, need, false);
    if (rc != FHERAM_OK) return rc;
    for (int i = 0; i < n; i++)
        if (srcs[i].kind == FHERAM_SRC_MEMBER_RESULT && !b->has_res[srcs[i].index])
            return fail(c, FHERAM_ERR_STATE, "source " + std::to_string(i) + " names the result of member " + std::to_string(srcs[i].index) + ", which has none yet");
    rc = bank_quiesce(c);
    if (rc == FHERAM_OK) rc = pin_init(c);
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, decrypt_decode_register());
    const int Y = n * ws;
    DecryptDecodeArgs da{};
    for (int i = 0; i < n; i++) {
        const int32_t* p = select_source(b, srcs[i]);
        for (int w = 0; w < ws; w++) da.src[i * ws + w] = p + (size_t)w * fheram_ctx::GLWE;
    }
    if (want) { da.has_want = 1; for (int y = 0; y < Y; y++) da.want[y] = want[y]; }
    da.s_hat = sk->d_hat; da.tw = c->d_tw;
    da.k = (int)c->p.k_glwe_ct; da.k_pt = (int)c->p.k_glwe_pt;
    da.n_coef = da.n_coef_last = 1;
    // device memory: [Y] diff, [Y] max |diff| (int64), [Y] values (int32), allocated and freed here
    long long* d_out = nullptr;
    const size_t bytes = (size_t)Y * (2 * sizeof(long long) + sizeof(int32_t));
    HIPCHK(c, hipMalloc((void**)&d_out, bytes));
    da.diff = d_out; da.max_diff = d_out + Y; da.values = reinterpret_cast<int32_t*>(d_out + 2 * Y);
    c->cur = c->stream;
    {
        ProfScope ps(c, "decrypt_decode", (uint64_t)Y);
        decrypt_decode_launch(Y, c->cur, da);
    }
    long long* h = reinterpret_cast<long long*>(c->h_pin[0]);
    hipError_t e = hipMemcpyAsync(h, d_out, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    hipFree(d_out);
    if (e != hipSuccess) return fail(c, FHERAM_ERR_DEVICE, std::string("k_decrypt_decode: ") + hipGetErrorString(e));
    const int32_t* h_val = reinterpret_cast<const int32_t*>(h + 2 * Y);
    for (int y = 0; y < Y; y++) {
        values[y] = h_val[y];
        if (log2_noise) log2_noise[y] = log2_noise_of(h[y] < 0 ? -(int64_t)h[y] : (int64_t)h[y], da.k);
    }
    return check_precision(c);
}
int fheram_bank_ram_decrypt(fheram_bank* b, int member, const fheram_secret* sk, int32_t* values, double* worst_log2_noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (member < 0 || member >= b->M) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member");
    if (!values) return fail(c, FHERAM_ERR_INVALID_ARG, "null values");
    const int rc = decrypt_check(c, sk);
    if (rc != FHERAM_OK) return rc;
    if (!b->ram[member].initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0");
    if (b->ram[member].state)
        return fail(c, FHERAM_ERR_STATE, "the member is between read_prepare_write and write: its rows are rotated (member " + std::to_string(member) + ")");
    const size_t per = (size_t)b->mws * c->rows * fheram_ctx::GLWE;
    return rows_decrypt(c, sk, c->d_data + (size_t)member * per, (size_t)b->mws, c->rows, (size_t)c->p.max_addr, values, worst_log2_noise);
}
int fheram_bank_regs_decrypt(fheram_bank* b, const fheram_regs* r, const fheram_secret* sk, int32_t* values, double* worst_log2_noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    int rc = regs_check_handle(b, r);
    if (rc != FHERAM_OK) return rc;
    if (!values) return fail(c, FHERAM_ERR_INVALID_ARG, "null values");
    rc = decrypt_check(c, sk);
    if (rc != FHERAM_OK) return rc;
    if (!r->initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: the register file has had no fheram_bank_regs_upload or fheram_bank_regs_pack");
    if (r->state) return fail(c, FHERAM_ERR_STATE, "the register file is between read_prepare_write and write: its row is rotated");
    return rows_decrypt(c, sk, r->row, (size_t)b->mws, 1, (size_t)1 << r->bits, values, worst_log2_noise);
}
int fheram_bank_table_decrypt(fheram_bank* b, const fheram_table* t, const fheram_secret* sk, int32_t* values, double* worst_log2_noise) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    int rc = table_check_handle(b, t, "the table");
    if (rc != FHERAM_OK) return rc;
    if (!values) return fail(c, FHERAM_ERR_INVALID_ARG, "null values");
    rc = decrypt_check(c, sk);
    if (rc != FHERAM_OK) return rc;
    if (!t->initialized) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: the table has had no fheram_bank_table_upload or fheram_bank_table_load_plain");
    return rows_decrypt(c, sk, t->row, (size_t)b->mws, 1, (size_t)1 << t->bits, values, worst_log2_noise);
}

}  // extern "C"

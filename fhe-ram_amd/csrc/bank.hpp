// Included by fheram.hip (same translation unit): fheram_bank — M RAMs of the same shape under ONE prepared key set, and Ram::read /
// read_prepare_write / write (ram.rs:172-294) on a contiguous range of them as ONE operation, one address per member.
// Ram objects are independent units (ram.rs:25-29; `&mut self` serialises per RAM only), so nothing orders operations on different RAMs.
//
// Structure: ONE internal context whose word count is M * ws.  Rows, arenas, tree, results, words and temporaries are laid out
// [M * ws][...], so ciphertext y = m * ws + w is word w of member m, and a member range [first, first + n) is a pointer offset plus
// gy = n * ws (BankView).  On that view the operation is path.hpp's read_impl / write_side_begin / write_top / write_rows with the operand set
// of the range (bank_opnds):
//   - a range of ONE member is the plain operation (one_addr), memo included;
//   - a wider range has its digits in a table: every address-independent step is one launch over n * ws ciphertexts, the address-dependent
//     products take the table where a table form exists (k_read_chain_b / _bw, k_trace_tail_b with its k_read_chain_b fallback,
//     k_write_chain_b) and run one launch per member on the member's y-slice everywhere else (prepare, the GGSW inversion, the unfused
//     product chains, n2 == 1).
// Per-member state (the state flag, what read_prepare_write kept for the write) lives here; the context's own fields are loaded from
// it for the duration of an operation.  The write's inverse digits are never started early in a bank of more than one member (pre_inv
// shares d_prep_inv and d_tail_sync between members); a bank of ONE member is a plain context in every respect.
// Bank operations are never captured into a hipGraph: under graph = 1 they are enqueued directly, in the forms that mode selects.
#pragma once
#include "path.hpp"

struct fheram_bank {
    fheram_ctx* c = nullptr;      // word count M * mws; never row-sharded, never part of a group
    int M = 0, mws = 0;
    bool init[FHERAM_BANK_MAX] = {}, state[FHERAM_BANK_MAX] = {};
    bool memo_top[FHERAM_BANK_MAX] = {};     // per member: fheram_ctx::memo_top / memo_alone / where the last result was left
    bool res_trtop[FHERAM_BANK_MAX] = {};
    int memo_alone[FHERAM_BANK_MAX] = {};
    double* d_prep = nullptr;     // [n][n_digits] prepared GGSW: the digits of the k-th address of the range being read   (M > 1)
    double* d_prep_inv = nullptr; // [n][n_digits] the inverse digits of the k-th address of the range being written      (M > 1)
};

namespace {

// The context as one operation on members [first, first + n) sees it: every buffer indexed by y starts at the range's first
// ciphertext and the word count is n * mws.  Restored when the operation has been enqueued.
struct BankView {
    fheram_ctx* c;
    int ws;
    int32_t *data, *A, *B, *C, *D, *tree, *res, *tmp, *tmp2, *w, *part, *trtop;
    BankView(fheram_bank* b, int first, int n) : c(b->c) {
        ws = c->ws; data = c->d_data; A = c->d_scrA; B = c->d_scrB; C = c->d_scrC; D = c->d_scrD;
        tree = c->d_tree; res = c->d_res; tmp = c->d_tmp; tmp2 = c->d_tmp2; w = c->d_w; part = c->d_part; trtop = c->d_trtop;
        const size_t o1 = (size_t)first * b->mws * fheram_ctx::GLWE, oR = o1 * c->rows;
        c->ws = n * b->mws;
        c->d_data += oR; c->d_scrA += oR; c->d_scrB += oR; c->d_scrC += oR; c->d_scrD += oR;
        c->d_tree += o1; c->d_res += o1; c->d_tmp += o1; c->d_tmp2 += o1; c->d_w += o1; c->d_part += o1; c->d_trtop += o1;
    }
    ~BankView() {
        c->ws = ws; c->d_data = data; c->d_scrA = A; c->d_scrB = B; c->d_scrC = C; c->d_scrD = D;
        c->d_tree = tree; c->d_res = res; c->d_tmp = tmp; c->d_tmp2 = tmp2; c->d_w = w; c->d_part = part; c->d_trtop = trtop;
        c->d_trhi = nullptr; c->d_last_res = nullptr;
    }
};

// the operand set of an operation on a range: one member is the plain operation on the view; more have their digits in the bank's tables
Opnds bank_opnds(fheram_bank* b, const fheram_addr* const* addrs, int n) {
    if (n == 1) return one_addr(b->c, addrs);
    return Opnds{b->c, addrs, n, b->mws, b->d_prep, b->d_prep_inv, (long)b->c->n_digits * (long)fheram_ctx::GGSW, true};
}

// ---- checks: the whole range before anything is enqueued -----------------------------------------------------------------------------
int bank_check(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int want_state) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    mid_rearm(c);
    if (first < 0 || n < 1 || first > b->M - n)
        return fail(c, FHERAM_ERR_INVALID_ARG, "member range [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") is empty or outside the bank's " + std::to_string(b->M) + " members");
    if (addrs) for (int k = 0; k < n; k++)
        if (!addrs[k] || addrs[k]->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "address " + std::to_string(k) + " is null or does not belong to this bank (layout mismatch, ram.rs:404)");
    for (int m = first; m < first + n; m++)
        if (!b->init[m]) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0 (member " + std::to_string(m) + ")");
    if (want_state < 0) return FHERAM_OK;
    if (!addrs) return fail(c, FHERAM_ERR_INVALID_ARG, "null address list");
    if (!c->keys_loaded) return fail(c, FHERAM_ERR_KEYS, "evaluation keys not loaded");
    for (int m = first; m < first + n; m++) {
        if (want_state == 0 && b->state[m])
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.read: internal state is true -> requires calling Memory.write (member " + std::to_string(m) + ")");
        if (want_state == 1 && !b->state[m])
            return fail(c, FHERAM_ERR_STATE, "invalid call to Memory.write: internal state is false -> requires calling Memory.read_prepare_write (member " + std::to_string(m) + ")");
    }
    return FHERAM_OK;
}
// the context's per-RAM fields for the duration of an op on [first, first + n): what read_prepare_write kept counts only when every
// member of the range holds it
void bank_load_state(fheram_bank* b, int first, int n, bool state) {
    fheram_ctx* c = b->c;
    c->initialized = true; c->state = state;
    c->memo_top = true; c->memo_alone = b->memo_alone[first];
    for (int m = first; m < first + n; m++) {
        c->memo_top = c->memo_top && b->memo_top[m];
        if (b->memo_alone[m] != c->memo_alone) c->memo_alone = 0;
    }
}
void bank_store_state(fheram_bank* b, int first, int n, bool state, bool new_result) {
    fheram_ctx* c = b->c;
    for (int m = first; m < first + n; m++) {
        b->state[m] = state; b->memo_top[m] = c->memo_top; b->memo_alone[m] = c->memo_alone;
        if (new_result) b->res_trtop[m] = c->d_last_res == c->d_trtop;
    }
    c->state = false; c->memo_top = false; c->memo_alone = 0;
}
// the results of members [first, first + n), widened into h_res by the device; out: [n][mws][GLWE] int64
int bank_result(fheram_bank* b, int first, int n, int64_t* out) {
    fheram_ctx* c = b->c;
    const size_t per = (size_t)b->mws * fheram_ctx::GLWE;
    ResRun runs[FHERAM_BANK_MAX];
    int n_runs = 0;
    for (int k = 0; k < n;) {      // one run per stretch of members whose result sits in the same buffer
        int e = k + 1;
        while (e < n && b->res_trtop[first + e] == b->res_trtop[first + k]) e++;
        runs[n_runs++] = ResRun{(b->res_trtop[first + k] ? c->d_trtop : c->d_res) + (size_t)(first + k) * per, (size_t)(e - k) * per};
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
    {
        BankView v(b, first, n);
        bank_load_state(b, first, n, false);
        rc = read_impl(bank_opnds(b, addrs, n), ctx_arenas(c), prepare_write);
        bank_store_state(b, first, n, rc == FHERAM_OK && prepare_write, true);              // ram.rs:533
    }
    if (rc != FHERAM_OK) return rc;
    HIPCHK(c, hipGetLastError());
    return out ? bank_result(b, first, n, out) : FHERAM_OK;
}

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
    fheram_ctx* c = nullptr;
    const int rc = fheram_ctx_create_cfg(&wide, device, 0, 1, cfg, &c);   // the parameter checks, then "no HIP device"
    if (rc != FHERAM_OK) return rc;
    fheram_bank* b = new fheram_bank();
    b->c = c; b->M = n_members; b->mws = (int)p->word_size;
    c->initialized = true;   // (per member: fheram_bank::init)
    if (n_members > 1) {
        c->pre_inv = 0;
        const size_t bytes = (size_t)n_members * c->n_digits * fheram_ctx::GGSW * sizeof(double);
        hipError_t e = hipMalloc((void**)&b->d_prep, bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_prep_inv, bytes);
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
    if (b->c) {
        hipSetDevice(b->c->device);
        if (b->c->stream) hipStreamSynchronize(b->c->stream);
        if (b->c->stream2) hipStreamSynchronize(b->c->stream2);
    }
    if (b->d_prep) hipFree(b->d_prep);
    if (b->d_prep_inv) hipFree(b->d_prep_inv);
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
    for (int m = 0; m < b->M; m++) { b->memo_top[m] = false; b->memo_alone[m] = 0; }   // kept traces are void with new keys
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
    b->init[member] = true; b->state[member] = false; b->memo_top[member] = false; b->memo_alone[member] = 0;
    return FHERAM_OK;
}
int fheram_bank_ram_download(fheram_bank* b, int member, int64_t* rows) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (member < 0 || member >= b->M || !rows) return fail(c, FHERAM_ERR_INVALID_ARG, "no such member, or null rows");
    if (!b->init[member]) return fail(c, FHERAM_ERR_UNINITIALIZED, "unitialized memory: self.data.len()=0");
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
int fheram_bank_ram_state(const fheram_bank* b, int member) { return (b && member >= 0 && member < b->M) ? (int)b->state[member] : 0; }

int fheram_bank_address_create(fheram_bank* b, const int64_t* const* ggsw, int n_ggsw, fheram_addr** out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    return fheram_address_create(b->c, ggsw, n_ggsw, out);
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
    {
        BankView v(b, first, n);
        bank_load_state(b, first, n, true);
        const Opnds o = bank_opnds(b, addrs, n);
        write_side_begin(o);                        // as fheram_write: the part that needs no words is enqueued before the host narrows them
        rc = fheram_word_stage(c, w, c->ws);
        if (rc != FHERAM_OK) {                      // (a limb out of range: nothing of the members has been touched)
            write_side_abort(c);
            bank_store_state(b, first, n, true, false);
            return rc;
        }
        rc = write_top(o);
        if (rc == FHERAM_OK) rc = write_rows(o);
        c->words_staged = false;
        bank_store_state(b, first, n, rc != FHERAM_OK, false);                              // ram.rs:648
    }
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

// Included by fheram.hip (same translation unit): fheram_bank — M RAMs of the same shape under ONE prepared key set, and Ram::read /
// read_prepare_write / write (ram.rs:172-294) on a contiguous range of them as ONE operation, one address per member.
// Ram objects are independent units (ram.rs:25-29; `&mut self` serialises per RAM only), so nothing orders operations on different RAMs.
//
// Structure: ONE internal context whose word count is M * ws.  Rows, arenas, tree, results, words and temporaries are laid out
// [M * ws][...], so ciphertext y = m * ws + w is word w of member m, and a member range [first, first + n) is a pointer offset plus
// gy = n * ws (BankView).  On that view
//   - a range of ONE member is the plain operation (path.hpp read_impl / write_top / write_rows), memo included;
//   - a wider range runs bank_read_impl / bank_write_*: the launch sequences of path.hpp with every address-independent step as one
//     launch over n * ws ciphertexts, the address-dependent products with an operand table (y / ws -> member) where a table form exists
//     (k_read_chain_b / _bw, k_trace_tail_b with its k_read_chain_b fallback, k_write_chain_b), and one launch per member on the
//     member's y-slice everywhere else (prepare, the GGSW inversion, the unfused product chains, n2 == 1) — as read_batch_impl does.
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

// what the path functions below share: the operand tables and a member's y-slice of a buffer
struct BankOp {
    fheram_bank* b;
    const fheram_addr* const* addrs;
    int n;
    long ostride() const { return (long)b->c->n_digits * (long)fheram_ctx::GGSW; }
    double* prep(int k, int ci) const { return b->d_prep + k * ostride() + (long)coord_first_digit(b->c, ci) * (long)fheram_ctx::GGSW; }
    double* inv(int k, int ci) const { return b->d_prep_inv + k * ostride() + (long)coord_first_digit(b->c, ci) * (long)fheram_ctx::GGSW; }
    GlweRef slice(GlweRef r, int k) const { r.p += (long)k * b->mws * r.sy; return r; }   // the k-th member's mws ciphertexts
};

// use_row_fuse for a range of members.  A lone context splits by column while rows * ws * 2 workgroups still fit the chip (pick_nco),
// which rules the fused row chain out; for a range the alternative to the ONE launch with an operand table is not one column-split
// launch per step but one per MEMBER and step, so the range takes one workgroup per ciphertext from the start.  (The smaller regimes —
// limb split, fine split, the mid chains — keep their precedence inside use_row_fuse.)
bool bank_row_fuse(fheram_ctx* c, int d, int n_tr, int gx, int gy) {
    const int nco = c->nco;
    if (nco == 0) c->nco = 2;
    const bool fuse = use_row_fuse(c, d, n_tr, gx, gy);
    c->nco = nco;
    return fuse;
}

// SubRam::read / read_prepare_write (ram.rs:382-542) of n members (path.hpp read_local + read_top, unsharded); the context is the view
int bank_read_impl(const BankOp& o, bool prepare_write) {
    fheram_ctx* c = o.b->c;
    c->wide = true;   // (a bank of more than one member never parks a gate wave)
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    const int ws = o.b->mws, Y = c->ws, R = (int)c->rows, n = o.n;
    for (int k = 0; k < n; k++)                                                       // ram.rs:416-419 / 496-499, every member's address
        launch_prepare(c, o.addrs[k]->d_ggsw, o.b->d_prep + k * o.ostride(), c->n_digits * (int)(fheram_ctx::GGSW / N));
    GlweRef data = ref(c->d_data, sy, G), A = ref(c->d_scrA, sy, G), B = ref(c->d_scrB, sy, G);
    GlweRef tmp = ref(c->d_tmp, G, 0), tree = ref(c->d_tree, G, 0);
    const int d0 = (int)c->base2d[0].size();
    GlweRef pk;
    c->memo_alone = 0;
    if (c->n2 == 1) {
        GlweRef row0 = ref(c->d_data, sy, 0);
        if (prepare_write) {
            for (int k = 0; k < n; k++) ep_chain(c, o.slice(row0, k), o.slice(row0, k), o.slice(ref(c->d_scrA, sy, 0), k), o.prep(k, 0), d0, 1, ws);   // ram.rs:502-504 (rows == 1)
            pk = row0;
        } else {
            GlweRef part = ref(c->d_part, G, 0);
            for (int k = 0; k < n; k++) ep_chain(c, o.slice(row0, k), o.slice(part, k), o.slice(tmp, k), o.prep(k, 0), d0, 1, ws);                     // ram.rs:451
            pk = part;
        }
    } else {
        const int L0 = LOGN - ilog2_ceil(c->rows_glob);
        const bool keep = prepare_write && c->memo && L0 > 0;
        int32_t* packed;
        if (bank_row_fuse(c, d0, L0, R, Y) && !(prepare_write && (d0 & 1))) {
            // every member's products and alone packer levels as ONE launch: row y reads its own rows and the digits of member y / ws
            launch_read_chain(c, data, prepare_write ? &data : nullptr, A, o.prep(0, 0), d0, L0, R, Y, ws, o.ostride(), Y);   // ram.rs:429-435 / 502-514
            packed = pack_levels(c, c->d_scrA, c->d_scrA, c->d_scrB, sy, G, (size_t)R, Y, 0, L0, keep, c->d_scrC, c->d_scrD);
        } else {
            int32_t* leaves;
            if (prepare_write) {
                for (int k = 0; k < n; k++) ep_chain(c, o.slice(data, k), o.slice(data, k), o.slice(A, k), o.prep(k, 0), d0, R, ws);   // ram.rs:502-504
                leaves = c->d_data;
            } else {
                for (int k = 0; k < n; k++) ep_chain(c, o.slice(data, k), o.slice(A, k), o.slice(B, k), o.prep(k, 0), d0, R, ws);      // ram.rs:429-434
                leaves = c->d_scrA;
            }
            packed = pack_levels(c, leaves, c->d_scrA, c->d_scrB, sy, G, (size_t)R, Y, L0, L0, keep, c->d_scrC, c->d_scrD);   // ram.rs:435-448 / 510-521
        }
        c->memo_alone = keep ? L0 : 0;
        pk = ref(packed, sy, 0);
    }
    GlweRef last = pk;
    const int d1 = c->n2 == 2 ? (int)c->base2d[1].size() : 0;
    const bool fuse_ep = c->n2 == 2 && c->tail_ep && d1 >= 2 && d1 <= TAIL_EP_MAX && use_tail(c, LOGN, 1, Y);
    GlweRef ep_out = prepare_write ? tree : ref(c->d_tmp2, G, 0);
    auto products1 = [&] { for (int k = 0; k < n; k++) ep_chain(c, o.slice(pk, k), o.slice(ep_out, k), o.slice(tmp, k), o.prep(k, 1), d1, 1, ws); };   // ram.rs:454 / 525-527
    if (c->n2 == 2) {
        if (!fuse_ep) products1();
        last = ep_out;                                                                // ram.rs:535 (res <- tree[0])
    }
    c->memo_top = prepare_write && c->memo;
    c->d_last_res = c->memo_top ? c->d_trtop : c->d_res;
    GlweRef tb[2];
    if (fuse_ep && chain_bufs(LOGN, last, ref(c->d_last_res, G, 0), tmp, tb))          // ram.rs:454 / 525-527 + 457 / 540 of every member as ONE launch
        launch_trace_tail(c, pk, tb, 0, LOGN, 1, Y, o.prep(0, 1), d1, ep_out, prepare_write, ws, o.ostride());
    else {
        if (fuse_ep) products1();
        trace_steps(c, last, ref(c->d_last_res, G, 0), tmp, 0, LOGN, 1, Y);           // ram.rs:457 / 540
    }
    c->prep1_ready = false;
    return FHERAM_OK;
}

// Ram::write (ram.rs:226-294) of n members: path.hpp write_side_begin, write_top, write_rows (unsharded)
void bank_write_side_begin(const BankOp& o) {
    fheram_ctx* c = o.b->c;
    c->wide = true;
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    hipEventRecord(c->ev_fork, c->stream);
    hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
    c->cur = c->stream2;
    if (c->n2 == 2) {                                                                 // trace(ct_hi) of every row of every member: ONE chain
        c->d_trhi = c->d_scrA;
        if (c->memo_alone > 0) {
            if ((LOGN - c->memo_alone) % 2 == 1) c->d_trhi = c->d_scrC;
            int32_t* tmp = c->d_trhi == c->d_scrA ? c->d_scrC : c->d_scrA;
            trace_steps(c, ref(c->d_scrA, sy, G), ref(c->d_trhi, sy, G), ref(tmp, sy, G), c->memo_alone, LOGN, (int)c->rows, c->ws);
        } else {
            trace_steps(c, ref(c->d_data, sy, G), ref(c->d_scrA, sy, G), ref(c->d_scrC, sy, G), 0, LOGN, (int)c->rows, c->ws);
        }
        c->memo_alone = 0;
    }
    for (int k = 0; k < o.n; k++) coordinate_prepare_inv(c, o.addrs[k], 0, c->d_ggsw_tmp2, o.inv(k, 0));   // ram.rs:278-289
    hipEventRecord(c->ev_join, c->stream2);
    c->cur = c->stream;
    c->side_begun = true;
}
int bank_write_top(const BankOp& o) {
    fheram_ctx* c = o.b->c;
    c->wide = true;
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    const int ws = o.b->mws, Y = c->ws;
    GlweRef wref = ref(c->d_w, G, 0), tmp = ref(c->d_tmp, G, 0), tmp2 = ref(c->d_tmp2, G, 0), tree = ref(c->d_tree, G, 0);
    // write_first_step (ram.rs:544-577) of every member: t <- normalize(t - trace(t) + w)
    GlweRef top = (c->n2 != 1) ? tree : ref(c->d_data, sy, 0);
    GlweRef tr = tmp;
    if (c->memo_top) tr = ref(c->d_trtop, G, 0);
    else trace_steps(c, top, tmp, tmp2, 0, LOGN, 1, Y);
    {
        ProfScope ps(c, "elementwise", Y);
        hipLaunchKernelGGL((k_sub_add_norm<3>), dim3(1, Y, EW_SLICES), dim3(256), 0, c->cur, top, tr, wref, top);
    }
    c->memo_top = false;
    if (c->n2 == 2) {
        // the head: per member, the inverse of coordinate 1 (ram.rs:260-271) and its products on the member's tree top (ram.rs:610)
        const int d1 = (int)c->base2d[1].size();
        for (int k = 0; k < o.n; k++) coordinate_prepare_inv(c, o.addrs[k], 1, c->d_ggsw_tmp, o.inv(k, 1));
        for (int k = 0; k < o.n; k++) ep_chain(c, o.slice(tree, k), o.slice(ref(c->d_part, G, 0), k), o.slice(tmp, k), o.inv(k, 1), d1, 1, ws);
        c->tree_rotate_pending = true;
    }
    return FHERAM_OK;
}
int bank_write_rows(const BankOp& o) {
    fheram_ctx* c = o.b->c;
    c->wide = true;
    const long G = (long)fheram_ctx::GLWE;
    const long sy = (long)c->rows * G;
    const int ws = o.b->mws, Y = c->ws, R = (int)c->rows;
    GlweRef data = ref(c->d_data, sy, G), A = ref(c->d_scrA, sy, G), B = ref(c->d_scrB, sy, G), D = ref(c->d_scrD, sy, G);
    GlweRef trhi = ref(c->d_trhi ? c->d_trhi : c->d_scrA, sy, G);
    const int d0 = (int)c->base2d[0].size();
    auto rotate_tree = [&] {                                                           // tree[0] <- ct_lo * X^-rows (ram.rs:629), every member
        if (!c->tree_rotate_pending) return;
        ProfScope ps(c, "elementwise", Y);
        hipLaunchKernelGGL((k_rotate<3>), dim3(1, Y, EW_SLICES), dim3(256), 0, c->cur, ref(c->d_part, G, 0), ref(c->d_tree, G, 0), -(int)c->rows_glob);
        c->tree_rotate_pending = false;
    };
    if (c->n2 == 2 && bank_row_fuse(c, d0, LOGN, R, Y)) {
        // ram.rs:612-646 of every row of every member as ONE launch (k_write_chain_b): row y takes the inverse digits of member y / ws
        hipStreamWaitEvent(c->stream, c->ev_join, 0);
        launch_write_chain(c, ref(c->d_part, G, 0), 1, 0, data, trhi, o.inv(0, 0), d0, LOGN, R, Y, ws, o.ostride());
        rotate_tree();
    } else {
        if (c->n2 == 2) trace_steps(c, ref(c->d_part, G, 0), B, D, 0, LOGN, R, Y, 1, 0);   // tmp_a = trace(ct_lo * X^-row)   ram.rs:621,629
        rotate_tree();
        hipStreamWaitEvent(c->stream, c->ev_join, 0);
        if (c->n2 == 2) {
            ProfScope ps(c, "elementwise", (uint64_t)R * Y);
            hipLaunchKernelGGL((k_sub_add_norm<3>), dim3(R, Y, EW_SLICES), dim3(256), 0, c->cur, data, trhi, B, data);   // ram.rs:617,625-626
        }
        for (int k = 0; k < o.n; k++) ep_chain(c, o.slice(data, k), o.slice(data, k), o.slice(A, k), o.inv(k, 0), d0, R, ws);   // ram.rs:644-646
    }
    c->side_begun = false;
    return FHERAM_OK;
}

// ---- checks: the whole range before anything is enqueued -----------------------------------------------------------------------------
int bank_check(fheram_bank* b, int first, int n, const fheram_addr* const* addrs, int want_state) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!c->mid && c->mid_saved && ++c->mid_off_ops >= 256) { c->mid = c->mid_saved; c->mid_saved = 0; c->mid_bad_windows = 0; c->mid_off_ops = 0; }   // (path.hpp check_common)
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
    const long long* mon = reinterpret_cast<const long long*>(c->d_tw + N);
    for (int k = 0; k < n;) {      // one launch per run of members whose result sits in the same buffer (the monitor's maximum lands behind the last)
        int e = k + 1;
        while (e < n && b->res_trtop[first + e] == b->res_trtop[first + k]) e++;
        const int32_t* src = (b->res_trtop[first + k] ? c->d_trtop : c->d_res) + (size_t)(first + k) * per;
        const int n4 = (int)((size_t)(e - k) * per / 4);
        hipLaunchKernelGGL(k_export_i64, dim3((n4 + 255) / 256), dim3(256), 0, c->stream, src, reinterpret_cast<long long*>(c->d_h_res + (size_t)k * per), n4, mon);
        k = e;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    c->wide_unsynced = false;
    double m;
    std::memcpy(&m, c->h_res + (size_t)n * per, 8);
    if (c->monitor && m > MON_LIMIT) __atomic_store_n(c->h_ro_flag, 1u, __ATOMIC_RELAXED);
    const int rc = check_precision(c);
    if (rc != FHERAM_OK) return rc;
    std::memcpy(out, c->h_res, (size_t)n * per * sizeof(int64_t));
    return FHERAM_OK;
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
        if (n == 1) rc = read_impl(c, addrs[0], prepare_write);      // the plain operation on that member
        else rc = bank_read_impl(BankOp{b, addrs, n}, prepare_write);
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
        const BankOp o{b, addrs, n};
        // as fheram_write: the part that needs no words is enqueued before the host narrows them
        if (n == 1) write_side_begin(c, addrs[0]); else bank_write_side_begin(o);
        rc = fheram_word_stage(c, w, c->ws);
        if (rc != FHERAM_OK) {                      // (a limb out of range: nothing of the members has been touched)
            write_side_abort(c);
            bank_store_state(b, first, n, true, false);
            return rc;
        }
        if (n == 1) { rc = write_top(c, addrs[0]); if (rc == FHERAM_OK) rc = write_rows(c, addrs[0]); }
        else { rc = bank_write_top(o); if (rc == FHERAM_OK) rc = bank_write_rows(o); }
        c->words_staged = false;
        c->memo_top = false; c->memo_alone = 0;
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

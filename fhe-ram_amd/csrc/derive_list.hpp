// Included by fheram.hip (same translation unit): fheram_bank_derive_list — the addresses, selectors and selector fields of a whole VM step
// derived from encrypted integers in ONE launch (k_cmux_jobs, cmux_jobs.hip), and fheram_bank_address_download.
//
// CONTRACT-COMPATIBLE ONLY, as fheram_address_derive and the select are.  The three existing derivations are the
// specification: address_derive_body (setup.hpp) and fheram_bank_selector_derive / _derive_fields (select.hpp) each hand k_cmux_chain ONE digit plan
// per launch, so a step's derivations are a launch per distinct first bit, per (first bit, width) pair and per field.  Here every output digit is
// a job with a plan entry of its own: the same chains, the same cmux_step, the same integers in the digits, one launch.
// Ordering and bookkeeping are the union of the three bodies': the waits of derive_wait_readers for the named addresses, fresh ids and
// derive_unsynced through derive_addresses_written, empty = false on the named selectors, class "derive".
#pragma once
#include "select.hpp"
#include "cmux_jobs.hpp"

namespace {
static_assert(FHERAM_DERIVE_LIST_DIGITS_MAX == CMUX_JOBS_MAX, "the argument struct of k_cmux_jobs holds FHERAM_DERIVE_LIST_DIGITS_MAX digit jobs");
static_assert(sizeof(fheram_derive_item) == 32, "fheram_derive_item is 32 bytes (api.py mirrors it)");
}  // namespace

extern "C" {

int fheram_bank_derive_list(fheram_bank* b, const fheram_derive_item* items, int n) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    fheram_ctx* c = b->c;
    if (!items) return fail(c, FHERAM_ERR_INVALID_ARG, "null item list");
    if (n < 1 || n > FHERAM_DERIVE_LIST_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "n = " + std::to_string(n) + " is outside [1, FHERAM_DERIVE_LIST_MAX = " + std::to_string(FHERAM_DERIVE_LIST_MAX) + "]");
    unsigned plan_bits = 0;
    for (auto& b1 : c->base2d) for (int w : b1) plan_bits += (unsigned)w;
    // ---- every check for the whole list before anything is enqueued: a refused call changes no target ----
    std::vector<CmuxJob> jobs;
    fheram_addr* addrs[FHERAM_DERIVE_LIST_MAX];
    fheram_selector* sels[FHERAM_DERIVE_LIST_MAX];   // every selector the call names, once
    unsigned seen[FHERAM_DERIVE_LIST_MAX];           // ... and the digits of a field selector named so far
    int n_addr = 0, n_sel = 0, digits = 0;
    bool plan_too_long = false;
    unsigned char a_rsh[DERIVE_DIGITS_MAX] = {}, a_bits[DERIVE_DIGITS_MAX] = {}, a_lsh[DERIVE_DIGITS_MAX] = {};
    if (c->n_digits <= DERIVE_DIGITS_MAX) address_plan(c, a_rsh, a_bits, a_lsh);
    auto beyond = [&](int k, int first, int width, const fheram_fheuint* fu) {
        return fail(c, FHERAM_ERR_INVALID_ARG, "bits [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(width) + ") of the integer of item " + std::to_string(k) + " are beyond its " + std::to_string(fu->n_bits) + " bits");
    };
    for (int k = 0; k < n; k++) {
        const fheram_derive_item& it = items[k];
        const std::string who = "item " + std::to_string(k);
        if (it.kind != FHERAM_DERIVE_ADDRESS && it.kind != FHERAM_DERIVE_SELECTOR && it.kind != FHERAM_DERIVE_FIELD)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " has the unknown kind " + std::to_string(it.kind));
        if (!it.fu || it.fu->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "the integer of " + who + " is null or belongs to another bank");
        if (!it.target) return fail(c, FHERAM_ERR_INVALID_ARG, "the target of " + who + " is null");
        if (it.kind != FHERAM_DERIVE_ADDRESS && it.sign != 0)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " is a selector item with sign = " + std::to_string(it.sign) + ", not 0 (selectors are X^-v)");
        if (it.kind != FHERAM_DERIVE_FIELD && it.field != 0)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " is no field item and has field = " + std::to_string(it.field) + ", not 0");
        if (it.first_bit < 0) return fail(c, FHERAM_ERR_INVALID_ARG, who + " has first_bit = " + std::to_string(it.first_bit) + ", below 0");
        if (it.kind == FHERAM_DERIVE_ADDRESS) {
            fheram_addr* a = static_cast<fheram_addr*>(it.target);
            if (a->ctx != c) return fail(c, FHERAM_ERR_INVALID_ARG, "the address of " + who + " belongs to another bank");
            if (it.first_bit > it.fu->n_bits - (int)plan_bits) return beyond(k, it.first_bit, (int)plan_bits, it.fu);
            for (int q = 0; q < n_addr; q++)
                if (addrs[q] == a) return fail(c, FHERAM_ERR_INVALID_ARG, "the address of " + who + " appears twice in the list");
            addrs[n_addr++] = a;
            if (c->n_digits > DERIVE_DIGITS_MAX) { plan_too_long = true; continue; }
            digits += c->n_digits;
            for (int d = 0; d < c->n_digits; d++)
                jobs.push_back(CmuxJob{it.fu->d_prep, a->d_ggsw + (size_t)d * fheram_ctx::GGSW, (unsigned char)(a_rsh[d] + it.first_bit), a_bits[d], a_lsh[d], (unsigned char)(it.sign ? 1 : 0)});
            continue;
        }
        fheram_selector* s = static_cast<fheram_selector*>(it.target);
        if (s->bank != b) return fail(c, FHERAM_ERR_INVALID_ARG, "the selector of " + who + " belongs to another bank");
        int at = 0;
        while (at < n_sel && sels[at] != s) at++;
        if (it.kind == FHERAM_DERIVE_SELECTOR) {
            if (s->fields) return fail(c, FHERAM_ERR_INVALID_ARG, "the selector of " + who + " is a field selector: FHERAM_DERIVE_FIELD items derive it");
            if (it.first_bit > it.fu->n_bits - s->bits) return beyond(k, it.first_bit, s->bits, it.fu);
            if (at < n_sel) return fail(c, FHERAM_ERR_INVALID_ARG, "the selector of " + who + " appears twice in the list");
            sels[n_sel] = s; seen[n_sel++] = 0;
            digits += s->n_digits;
            for (int d = 0; d < s->n_digits; d++)
                jobs.push_back(CmuxJob{it.fu->d_prep, s->d_ggsw + (size_t)d * fheram_ctx::GGSW, (unsigned char)(it.first_bit + s->rsh[d]), s->width[d], s->lsh[d], 0});
            continue;
        }
        if (!s->fields) return fail(c, FHERAM_ERR_INVALID_ARG, "the selector of " + who + " was not made by fheram_bank_selector_alloc_fields / _create_fields");
        if (it.field < 0 || it.field >= s->n_digits)
            return fail(c, FHERAM_ERR_INVALID_ARG, who + " names field " + std::to_string(it.field) + ", outside the selector's " + std::to_string(s->n_digits) + " digits");
        const int d = it.field;
        if (it.first_bit > it.fu->n_bits - (int)s->width[d]) return beyond(k, it.first_bit, (int)s->width[d], it.fu);
        if (at == n_sel) { sels[n_sel] = s; seen[n_sel++] = 0; }
        if (seen[at] & (1u << d)) return fail(c, FHERAM_ERR_INVALID_ARG, who + " names field " + std::to_string(d) + " of its selector a second time");
        seen[at] |= 1u << d;
        digits += 1;
        jobs.push_back(CmuxJob{it.fu->d_prep, s->d_ggsw + (size_t)d * fheram_ctx::GGSW, (unsigned char)it.first_bit, s->width[d], s->lsh[d], 0});
    }
    for (int q = 0; q < n_sel; q++)   // a field selector is derived whole, as fheram_bank_selector_derive_fields derives it: empty = false is set once
        if (sels[q]->fields && seen[q] != (1u << sels[q]->n_digits) - 1u)
            return fail(c, FHERAM_ERR_INVALID_ARG, "the call names some of the " + std::to_string(sels[q]->n_digits) + " fields of a field selector and not all of them");
    if (plan_too_long)
        return fail(c, FHERAM_ERR_UNSUPPORTED, "fheram_bank_derive_list takes address plans of at most " + std::to_string(DERIVE_DIGITS_MAX) + " digits, as fheram_address_derive");
    if (digits > FHERAM_DERIVE_LIST_DIGITS_MAX)
        return fail(c, FHERAM_ERR_INVALID_ARG, "the items have " + std::to_string(digits) + " digits in total, more than FHERAM_DERIVE_LIST_DIGITS_MAX = " + std::to_string(FHERAM_DERIVE_LIST_DIGITS_MAX));
    HIPCHK(c, hipSetDevice(c->device));
    // The longest chains first: a call of more than one workgroup per CU (256 at 144 KiB of LDS each) starts them in its first round.
    std::stable_sort(jobs.begin(), jobs.end(), [](const CmuxJob& x, const CmuxJob& y) { return x.bits > y.bits; });
    CmuxJobsArgs ja{};
    ja.tw = c->d_tw;
    for (size_t j = 0; j < jobs.size(); j++) ja.job[j] = jobs[j];
    // ---- enqueue ----
    const int rc = derive_wait_readers(c, addrs, n_addr);
    if (rc != FHERAM_OK) return rc;
    c->cur = c->stream;
    main_enqueued(c);   // (as the selector derivations; derive_addresses_written says it again for a call that names an address: idempotent)
    {
        const int rows = fheram_ctx::DNUM_CT * 2;
        ProfScope ps(c, "derive", (uint64_t)jobs.size() * rows);
        cmux_jobs_launch(rows, (int)jobs.size(), c->cur, ja);
    }
    HIPCHK(c, hipGetLastError());
    if (n_addr) derive_addresses_written(c, addrs, n_addr);
    for (int q = 0; q < n_sel; q++) sels[q]->empty = false;
    return FHERAM_OK;
}

int fheram_bank_address_download(fheram_bank* b, const fheram_addr* addr, int64_t* out) {
    if (!b) return FHERAM_ERR_INVALID_ARG;
    if (!out) return fail(b->c, FHERAM_ERR_INVALID_ARG, "null output");
    return fheram_address_download(b->c, addr, out);
}

}  // extern "C"

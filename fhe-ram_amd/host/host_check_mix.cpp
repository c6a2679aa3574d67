// Build + link + run check of Bank::read_mix, the C++ mirror of fheram_bank_read_mix (tests/test_mix_abi.py builds and runs it).  Without a
// GPU the first Bank throws the C ABI's FHERAM_ERR_DEVICE, which ends the check loudly with exit status 0; with one, a mix is compared with
// the three single calls on the same bank.  Synthetic normalised limbs throughout: the path is deterministic.
#include "fheram.hpp"
#include <cstdio>

int main() {
    using B = fheram::Bank;
    const fheram::Parameters bp(2, {3, 3, 3, 3}, 1 << 12);
    const size_t n = bp.n();
    uint64_t lcg = 88172645463325252ull;
    auto synth = [&](size_t count) {
        std::vector<int64_t> v(count);
        for (auto& x : v) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; x = (int64_t)((lcg >> 40) & 0x1ffff) - (1 << 16); }
        return v;
    };
    auto digits = [&](int d) { std::vector<std::vector<int64_t>> v; for (int i = 0; i < d; i++) v.push_back(synth(3 * 2 * 4 * 2 * n)); return v; };
    try {
        fheram::EvaluationKeysPrepared bk;
        bk.gal_els.push_back(-1);
        for (uint32_t i = 1; i < bp.p.log_n; i++) {
            uint64_t g = 5;
            for (uint32_t s = 1; s < i; s++) g = g * g % (2 * n);
            bk.gal_els.push_back((int64_t)g);
        }
        for (size_t i = 0; i < bk.gal_els.size(); i++) bk.atk_glwe.push_back(synth(3 * 4 * 2 * n));
        bk.atk_ggsw_inv = synth(4 * 5 * 2 * n);
        bk.tsk_ggsw_inv = synth(4 * 5 * 2 * n);
        B bank(bp, 2);
        for (int m = 0; m < 2; m++) bank.load_encrypted(m, synth(2 * bank.glwe_len()));
        fheram::Address a0(digits(4)), a1(digits(4));
        B::Table rom(bank, 12), lut(bank, 12);
        B::RegFile rf(bank, 5);
        rom.load(synth(2 * bank.glwe_len()));
        lut.load(synth(2 * bank.glwe_len()));
        rf.load(synth(2 * bank.glwe_len()));
        B::Selector fetch(bank, B::Selector::Wide{}, 12, digits(4)), look(bank, B::Selector::Wide{}, 12, digits(4));
        B::Selector rs1(bank, 5, digits(2)), rs2(bank, 5, digits(2));
        if (fetch.n_digits() != 4 || rs1.n_digits() != 2) return 2;
        // one entry of each kind: six ciphertexts with 0 / 4 / 2 products in front of one trace
        std::vector<fheram::Address*> one_a = {&a1}, two_a = {&a0, &a1};
        const auto l1 = bank.read_list({1}, one_a, bk);
        const auto t1 = bank.table_read({&rom}, {&fetch});
        const auto r1 = rf.read({&rs1});
        const B::MixResult m1 = bank.read_mix({1}, one_a, {&rom}, {&fetch}, &rf, {&rs1}, bk);
        if (m1.list != l1 || m1.table != t1 || m1.regs != r1) { std::printf("read_mix: one entry of each kind differs from the three single calls\n"); return 3; }
        if (bank.list_result(0, 1) != l1 || bank.table_result(0, 1) != t1 || rf.result(0, 1) != r1) { std::printf("read_mix: the _result downloads differ\n"); return 3; }
        // two entries of each kind (twelve ciphertexts: the products entry by entry, one trace), without a host wait
        const auto l2 = bank.read_list({0, 1}, two_a, bk);
        const auto t2 = bank.table_read({&rom, &lut}, {&fetch, &look});
        const auto r2 = rf.read({&rs1, &rs2});
        const B::MixResult m2 = bank.read_mix({0, 1}, two_a, {&rom, &lut}, {&fetch, &look}, &rf, {&rs1, &rs2}, bk, false);
        if (!m2.list.empty() || !m2.table.empty() || !m2.regs.empty()) return 4;
        if (bank.list_result(0, 2) != l2 || bank.table_result(0, 2) != t2 || rf.result(0, 2) != r2) { std::printf("read_mix: two entries of each kind differ\n"); return 4; }
        // an empty group keeps its kind's last outputs
        std::vector<fheram::Address*> none;
        const B::MixResult m3 = bank.read_mix({}, none, {&lut}, {&look}, nullptr, {}, bk);
        if (m3.table.size() != 1 || m3.table[0] != t2[1] || !m3.list.empty() || !m3.regs.empty()) { std::printf("read_mix: the table group alone differs\n"); return 5; }
        if (bank.list_result(0, 2) != l2 || rf.result(0, 2) != r2) { std::printf("read_mix: an empty group lost its last outputs\n"); return 5; }
        if (bank.select({&rs1}, {{B::src_list(1), B::src_table(0), B::src_regs(1)}}).size() != 1) return 5;
        // refusals: the mirror's own, and the library's
        try { bank.read_mix({}, none, {}, {}, nullptr, {}, bk); return 6; }
        catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 6; }
        try { bank.read_mix({0}, two_a, {}, {}, nullptr, {}, bk); return 6; }
        catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 6; }
        try { bank.read_mix({}, none, {&rom}, {&rs1}, nullptr, {}, bk); return 6; }   // a 5-bit selector at a table of 12
        catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 6; }
        try { bank.read_mix({}, none, {}, {}, &rf, {&fetch}, bk); return 6; }          // a wide selector at the register file
        catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 6; }
        if (bank.table_result(0, 1) != m3.table) { std::printf("read_mix: a refused call changed the last table read\n"); return 6; }
        std::printf("bank read_mix == read_list, table_read, RegFile::read: ok\n");
    } catch (const fheram::Error& e) {
        if (e.code != FHERAM_ERR_DEVICE) { std::printf("unexpected error %d: %s\n", e.code, e.what()); return 1; }
        std::printf("no GPU: %s\n", e.what());
    }
    return 0;
}

// Build + link check of the C++ host mirror (no GPU needed: without a device Ram::Ram throws the
// C ABI's FHERAM_ERR_DEVICE, which is the behaviour the check asserts on a CPU-only box).
#include "fheram.hpp"
#include <cstdio>

// a sampler with the interface the encrypt_sk methods take (a real host plugs in its own CSPRNG)
struct ZeroSource : fheram::Source {
    void uniform_limbs(int64_t* out, size_t count) override { for (size_t i = 0; i < count; i++) out[i] = 0; }
    void gaussian(int64_t* out, size_t count, double) override { for (size_t i = 0; i < count; i++) out[i] = 0; }
};

int main() {
    fheram::Parameters p;
    if (p.max_addr() != (1u << 14) || p.word_size() != 4 || p.basek() != 17) return 2;   // parameters.rs:11-21
    fheram::Parameters rd = fheram::Parameters::readme();                                    // README.md:20-33
    if (rd.max_addr() != (1u << 18) || rd.k_glwe_pt() != 9 || rd.p.k_evk_trace != 5 * 17) return 2;
    {   // execution switches: library defaults (pure host code: runs without a GPU)
        const fheram_config c = fheram::Ram::default_config();
        if (!c.fuse || !c.tail || c.chain_y != 3 || c.reserved != 0) return 6;
    }
    try {
        fheram::Ram ram = fheram::Ram::new_from_ram_params(4, {3, 3, 3, 3}, 1 << 12);
        if (ram.config().fuse != fheram::Ram::default_config().fuse) return 6;
        fheram::EvaluationKeysPrepared keys;
        fheram::Address addr;
        try { ram.read(addr, keys); return 3; }                      // no keys, empty RAM: must throw
        catch (const fheram::Error& e) { std::printf("refused as the reference would: %s\n", e.what()); }
        // setup side on the device: secret, keys, RAM and address, then one read and its decryption
        ZeroSource xa, xe;
        std::vector<int64_t> sk(p.n(), 0);
        sk[1] = 1; sk[5] = -1;
        fheram::Ram::Secret dsk(ram, sk);
        ram.encrypt_keys(keys, dsk, xa, xe);
        std::vector<uint8_t> data((size_t)(1 << 12) * 4);
        for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)(i * 7 + 3);
        ram.encrypt_sk(data, dsk, xa, xe);
        const uint32_t idx = 1234;
        ram.encrypt_address(addr, idx, dsk, xa, xe);
        std::vector<int64_t> pt = ram.decrypt(ram.read(addr, keys), dsk);
        for (size_t i = 0; i < 4; i++) {                             // noiseless: limb 0 of coefficient 0 is the byte's low 3 bits << 14
            const int64_t want = (int64_t)((int8_t)(uint8_t)(data[idx * 4 + i] << 5) >> 5) * (1 << 14);
            const int64_t got = pt[i * 3 * p.n()];
            if (((got - want) & ((1 << 17) - 1)) != 0) { std::printf("word %zu: got %lld want %lld\n", i, (long long)got, (long long)want); return 5; }
        }
        std::printf("device-side setup + read + decrypt: ok\n");
        {   // the result in place (pinned host buffer the device wrote): the same limbs as the copy returned by read
            std::vector<fheram::Glwe> r = ram.read(addr, keys);
            const int64_t* v = ram.result_view();
            for (size_t i = 0; i < r.size(); i++)
                for (size_t k = 0; k < r[i].size(); k++)
                    if (v[i * r[i].size() + k] != r[i][k]) { std::printf("result_view differs\n"); return 7; }
            std::printf("result in place == result copied: ok\n");
            const auto ts = ram.tail_stats();
            if (ts.launches == 0 || ts.redone != 0) { std::printf("tail stats: %llu launches, %llu redone\n", (unsigned long long)ts.launches, (unsigned long long)ts.redone); return 10; }
        }
        // Address::set_from_fheuint (conversion.rs:68-82): the same word through an address derived from an encrypted integer
        fheram::Ram::FheUintPrepared fu(ram, idx, dsk, xa, xe, 12);
        fheram::Address derived;
        ram.set_from_fheuint(derived, fu);
        std::vector<int64_t> pt2 = ram.decrypt(ram.read(derived, keys), dsk);
        for (size_t i = 0; i < 4; i++)
            if (((pt2[i * 3 * p.n()] - pt[i * 3 * p.n()]) & ((1 << 17) - 1)) != 0) { std::printf("derived address: word %zu differs\n", i); return 6; }
        std::printf("address derived from an encrypted integer reads the same word: ok\n");
        {   // the same word again through a BYTE address: the word address sits above two lane-offset bits (fheram_address_derive_at, first_bit = 2)
            fheram::Ram::FheUintPrepared byte_addr(ram, (idx << 2) | 3, dsk, xa, xe, 14);
            fheram::Address at2;
            ram.derive({&byte_addr}, {&at2}, false, {2});
            std::vector<int64_t> pt3 = ram.decrypt(ram.read(at2, keys), dsk);
            for (size_t i = 0; i < 4; i++)
                if (((pt3[i * 3 * p.n()] - pt[i * 3 * p.n()]) & ((1 << 17) - 1)) != 0) { std::printf("address derived at bit 2: word %zu differs\n", i); return 6; }
            try { ram.derive({&byte_addr}, {&at2}, false, {3}); return 6; }   // 3 + 12 bits are beyond the integer's 14
            catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 6; }
            std::printf("address derived from bit 2 of a byte address reads the same word: ok\n");
        }
        // one handle over "two GPUs" (the same device twice: rehearsal): a group must refuse an operation before its keys
        // and RAM are loaded exactly as the single context does
        fheram::GroupRam grp(fheram::Parameters(4, {3, 3, 3, 3}, 1 << 13), {0, 0});   // two rows per sub-RAM: one per shard
        if (grp.size() != 2) return 8;
        try { fheram::Address a2; grp.read(a2, fheram::EvaluationKeysPrepared()); return 9; }
        catch (const fheram::Error& e) { std::printf("group refused as the reference would: %s\n", e.what()); }
        {   // the setup side of a bank, every call once with the noiseless sampler: the bank needs no twin context and no host encryption, and
            // what it leaves on the device is decrypted and decoded there
            using B = fheram::Bank;
            const fheram::Parameters sp(2, {3, 3, 3, 3}, 1 << 12);
            B sb(sp, 2);
            B::Secret bsk(sb, sk);
            fheram::EvaluationKeysPrepared bkeys;
            sb.encrypt_keys(bkeys, bsk, xa, xe);
            std::vector<uint8_t> d0((size_t)(1 << 12) * 2), rd(32 * 2), td(128 * 2);
            for (size_t i = 0; i < d0.size(); i++) d0[i] = (uint8_t)(i * 5 + 1);
            for (size_t i = 0; i < rd.size(); i++) rd[i] = (uint8_t)(i * 3 + 2);
            for (size_t i = 0; i < td.size(); i++) td[i] = (uint8_t)(i * 11 + 7);
            auto plain = [](uint8_t b) { return (int)((int8_t)(uint8_t)(b << 5) >> 5); };   // the byte's low 3 bits, centred
            for (int m = 0; m < 2; m++) sb.encrypt_sk(m, d0, bsk, xa, xe);
            B::RegFile rf(sb, 5);
            B::Table tb(sb, 7);
            rf.encrypt_sk(rd, bsk, xa, xe);
            tb.encrypt_sk(td, bsk, xa, xe);
            double worst = 0.0;
            const std::vector<int32_t> mv = sb.decrypt(1, bsk, &worst), rv = rf.decrypt(bsk), tv = tb.decrypt(bsk);
            if (mv.size() != d0.size() || rv.size() != rd.size() || tv.size() != td.size()) return 24;
            for (size_t i = 0; i < d0.size(); i++) if (mv[i] != plain(d0[i])) { std::printf("Bank::decrypt: byte %zu decodes to %d\n", i, mv[i]); return 24; }
            for (size_t i = 0; i < rd.size(); i++) if (rv[i] != plain(rd[i])) { std::printf("RegFile::decrypt: byte %zu decodes to %d\n", i, rv[i]); return 24; }
            for (size_t i = 0; i < td.size(); i++) if (tv[i] != plain(td[i])) { std::printf("Table::decrypt: byte %zu decodes to %d\n", i, tv[i]); return 24; }
            if (worst > -40.0) { std::printf("Bank::decrypt: worst log2 noise %.2f of a noiseless member\n", worst); return 24; }
            fheram::Address ba, bd;
            sb.encrypt_address(ba, 777, bsk, xa, xe);
            B::FheUintPrepared bfu(sb, 778u, bsk, xa, xe, 12);
            sb.derive({&bfu}, {&bd});
            B::Selector s5(sb, 5), s7(sb, B::Selector::Wide{}, 7);
            s5.encrypt_sk(sb, 19, bsk, xa, xe);
            s7.encrypt_sk(sb, 100, bsk, xa, xe);
            std::vector<fheram::Address*> at_ba = {&ba}, at_bd = {&bd};
            sb.read(at_ba, bkeys, 0);
            sb.read_list({1}, at_bd, bkeys);
            rf.read({&s5}, false);
            sb.table_read({&tb}, {&s7}, false);
            std::vector<double> nz;
            const std::vector<int64_t> got = sb.decrypt_sources(bsk, {B::src_member(0), B::src_list(0), B::src_regs(0), B::src_table(0)}, {}, &nz);
            const uint8_t want[8] = {d0[777 * 2], d0[777 * 2 + 1], d0[778 * 2], d0[778 * 2 + 1], rd[19 * 2], rd[19 * 2 + 1], td[100 * 2], td[100 * 2 + 1]};
            for (size_t i = 0; i < 8; i++)
                if (got[i] != plain(want[i]) || nz[i] > -4.0) { std::printf("Bank::decrypt_sources: value %zu is %lld (log2 noise %.2f), want %d\n", i, (long long)got[i], nz[i], plain(want[i])); return 24; }
            const std::vector<int64_t> wpt = sb.decrypt(sb.encrypt_word({5, 200}, bsk, xa, xe), bsk);
            if (((wpt[0] - (int64_t)plain(5) * (1 << 14)) & ((1 << 17) - 1)) != 0 || ((wpt[3 * sp.n()] - (int64_t)plain(200) * (1 << 14)) & ((1 << 17) - 1)) != 0) return 24;
            std::printf("bank setup side: keys, members, register file, table, address, integer, selectors, words, decrypt on the device: ok\n");
        }
        {   // Bank::read_list on a bank of two members: slice k is what the single-member read of members[k] returns, in any order and
            // with repeats; afterwards the bank is where those reads leave it.  Synthetic normalised limbs (the path is deterministic).
            const fheram::Parameters bp(4, {3, 3, 3, 3}, 1 << 12);
            const size_t n = bp.n();
            uint64_t lcg = 88172645463325252ull;
            auto synth = [&](size_t count) {
                std::vector<int64_t> v(count);
                for (auto& x : v) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; x = (int64_t)((lcg >> 40) & 0x1ffff) - (1 << 16); }
                return v;
            };
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
            fheram::Bank bank(bp, 2);
            for (int m = 0; m < 2; m++) bank.load_encrypted(m, synth(4 * bank.glwe_len()));
            auto address = [&] { std::vector<std::vector<int64_t>> d; for (int i = 0; i < 4; i++) d.push_back(synth(3 * 2 * 4 * 2 * n)); return d; };
            fheram::Address a0(address()), a1(address());
            std::vector<fheram::Address*> la = {&a0, &a1, &a1}, one(1);
            const std::vector<int> members = {1, 0, 1};
            const auto got = bank.read_list(members, la, bk);
            if (got.size() != 3 || bank.list_result(1, 2) != std::vector<std::vector<fheram::Glwe>>(got.begin() + 1, got.end())) return 11;
            for (size_t k = 0; k < members.size(); k++) {
                one[0] = la[k];
                if (bank.read(one, bk, members[k])[0] != got[k]) { std::printf("read_list: entry %zu differs from the single-member read\n", k); return 11; }
            }
            if (bank.state(0) || bank.state(1)) return 11;
            try { std::vector<fheram::Address*> bad = {&a0}; bank.read_list({2}, bad, bk); return 12; }
            catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 12; }
            std::printf("bank read list == single-member reads: ok\n");
            // Bank::read_prepare_write_list / write_list on members {2, 0} of a bank of three against a twin driven member by member
            fheram::Bank lists(bp, 3), twin(bp, 3);
            for (int m = 0; m < 3; m++) { const auto r = synth(4 * lists.glwe_len()); lists.load_encrypted(m, r); twin.load_encrypted(m, r); }
            std::vector<fheram::Address*> wa = {&a1, &a0};
            const std::vector<int> wm = {2, 0};
            std::vector<std::vector<fheram::Glwe>> words(2);
            for (auto& word : words) for (int i = 0; i < 4; i++) word.push_back(synth(lists.glwe_len()));
            const auto prepared = lists.read_prepare_write_list(wm, wa, bk);
            if (prepared.size() != 2 || !lists.state(2) || !lists.state(0) || lists.state(1)) return 13;
            for (size_t k = 0; k < wm.size(); k++) {
                one[0] = wa[k];
                if (twin.read_prepare_write(one, bk, wm[k])[0] != prepared[k]) { std::printf("read_prepare_write_list: entry %zu differs\n", k); return 13; }
            }
            lists.write_list(wm, words, wa, bk);
            for (size_t k = 0; k < wm.size(); k++) {
                one[0] = wa[k];
                twin.write({words[k]}, one, bk, wm[k]);
            }
            for (int m = 0; m < 3; m++)
                if (lists.state(m) || lists.store_encrypted(m) != twin.store_encrypted(m)) { std::printf("write_list: member %d differs\n", m); return 13; }
            try { std::vector<fheram::Address*> dup = {&a0, &a1}; lists.read_prepare_write_list({1, 1}, dup, bk); return 14; }
            catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 14; }
            std::printf("bank write lists == single-member operations: ok\n");
            // Bank::select / write_selected: the conditional write of members {2, 0} with the picked words kept on the device, against the twin
            // that downloads its select outputs and writes them with write_list (synthetic selector digits: the path is deterministic)
            std::vector<std::vector<int64_t>> sd = {synth(3 * 2 * 4 * 2 * n)};
            fheram::Bank::Selector ls0(lists, 1, sd), ls1(lists, 1, sd), ts0(twin, 1, sd), ts1(twin, 1, sd);
            if (ls0.n_digits() != 1) return 15;
            const std::vector<std::vector<fheram_select_src>> cand = {{fheram::Bank::src_member(2), fheram::Bank::src_host(0)}, {fheram::Bank::src_member(0), fheram::Bank::src_host(1)}};
            lists.read_prepare_write_list(wm, wa, bk);
            twin.read_prepare_write_list(wm, wa, bk);
            if (!lists.select({&ls0, &ls1}, cand, words, false).empty()) return 15;
            const auto picked = twin.select({&ts0, &ts1}, cand, words);
            if (picked.size() != 2 || lists.select_result(0, 2) != picked) { std::printf("select: the two banks differ\n"); return 15; }
            lists.write_selected(wm, {0, 1}, wa, bk);
            twin.write_list(wm, picked, wa, bk);
            for (int m = 0; m < 3; m++)
                if (lists.state(m) || lists.store_encrypted(m) != twin.store_encrypted(m)) { std::printf("write_selected: member %d differs\n", m); return 15; }
            try { lists.select({&ts0}, {{fheram::Bank::src_zero()}}); return 16; }   // a selector of another bank
            catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 16; }
            std::printf("bank select + write_selected == select, download, write_list: ok\n");
            {   // Bank::select_lanes: identity lanes are select; swapped lanes are select on the host-assembled word; field selectors; derive at an offset
                using B = fheram::Bank;
                std::vector<std::vector<std::vector<fheram_select_lane>>> ident(2), swapped(1);
                for (size_t k = 0; k < 2; k++)
                    for (auto& src : cand[k]) { ident[k].emplace_back(); for (int w = 0; w < 4; w++) ident[k].back().push_back(B::lane_of(src, w)); }
                if (lists.select_lanes({&ls0, &ls1}, ident, words) != twin.select({&ts0, &ts1}, cand, words)) { std::printf("select_lanes: identity lanes differ from select\n"); return 17; }
                const int perm[4] = {1, 0, 3, 2};
                swapped[0].emplace_back(); swapped[0].emplace_back();
                for (int w = 0; w < 4; w++) { swapped[0][0].push_back(B::lane_of(B::src_host(0), perm[w])); swapped[0][1].push_back(B::lane_of(B::src_host(1), w)); }
                std::vector<std::vector<fheram::Glwe>> shuffled = words;
                for (int w = 0; w < 4; w++) shuffled[0][w] = words[0][perm[w]];
                if (lists.select_lanes({&ls0}, swapped, words) != twin.select({&ts0}, {{B::src_host(0), B::src_host(1)}}, shuffled)) { std::printf("select_lanes: permuted lanes differ\n"); return 17; }
                // a selector of two one-bit fields: from host digits, and derived field by field from two synthetic integers
                const std::vector<std::vector<int64_t>> fd = {sd[0], synth(3 * 2 * 4 * 2 * n)};
                B::Selector lf(lists, std::vector<int>{1, 1}, fd), tf(twin, std::vector<int>{1, 1}, fd), ld(lists, std::vector<int>{1, 1}), td(twin, std::vector<int>{1, 1});
                if (lf.n_digits() != 2 || ld.n_digits() != 2) return 18;
                const std::vector<std::vector<fheram_select_src>> four = {{B::src_host(0), B::src_host(1), B::src_zero(), B::src_member(0)}};
                if (lists.select({&lf}, four, words) != twin.select({&tf}, four, words)) return 18;
                const std::vector<int64_t> ia = synth(3 * 4 * 2 * 5 * 2 * n), ib = synth(2 * 4 * 2 * 5 * 2 * n);
                B::FheUintPrepared la3(lists, ia, 3), lb2(lists, ib, 2), ta3(twin, ia, 3), tb2(twin, ib, 2);
                lists.derive_selector_fields(ld, {&la3, &lb2}, {2, 0});
                twin.derive_selector_fields(td, {&ta3, &tb2}, {2, 0});
                if (lists.select({&ld}, four, words) != twin.select({&td}, four, words)) return 18;
                try { lists.select({&ld, &ls0}, {four[0], four[0]}, words); return 18; }   // two bits in two digits beside one bit
                catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 18; }
                try { lists.derive_selector_fields(ld, {&la3, &lb2}, {2, 2}); return 18; }   // bit [2, 3) is beyond the second integer's 2 bits
                catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 18; }
                std::printf("bank select_lanes, field selectors: ok\n");
                {   // Bank::derive_list: an address at bit 2, a plain selector and the two fields in ONE launch, against the twin's three calls
                    const std::vector<int64_t> ic = synth(14 * 4 * 2 * 5 * 2 * n);
                    B::FheUintPrepared lc14(lists, ic, 14), tc14(twin, ic, 14);
                    fheram::Address da, ta;
                    B::Selector lp(lists, 1), tp(twin, 1);
                    lists.derive_list({B::derive_address(lc14, da, 2), B::derive_selector(la3, lp, 1), B::derive_field(la3, ld, 0, 2), B::derive_field(lb2, ld, 1, 0)});
                    twin.derive({&tc14}, {&ta}, false, {2});
                    twin.derive_selectors({&ta3}, {1}, {&tp});
                    twin.derive_selector_fields(td, {&ta3, &tb2}, {2, 0});
                    if (lists.address_digits(da) != twin.address_digits(ta) || lists.address_digits(da).size() != 4) { std::printf("derive_list: the address differs\n"); return 19; }
                    if (lists.select({&ld}, four, words) != twin.select({&td}, four, words)) return 19;
                    if (lists.select({&lp}, {{B::src_host(0), B::src_host(1)}}, words) != twin.select({&tp}, {{B::src_host(0), B::src_host(1)}}, words)) return 19;
                    try { lists.derive_list({B::derive_field(la3, ld, 0, 2)}); return 19; }   // a field selector is derived whole
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 19; }
                    std::printf("bank derive_list == derive, derive_selectors, derive_selector_fields: ok\n");
                }
                {   // Bank::RegFile: a register file of 2 words, every call once; a packed one reads as the select on the same sources does
                    B::RegFile lr(lists, 1), tr(twin, 1);
                    if (lr.bits() != 1 || lr.state()) return 20;
                    const auto row = synth(4 * lists.glwe_len());
                    lr.load(row);
                    tr.load(row);
                    if (lr.store() != row) { std::printf("RegFile: the row differs from what was loaded\n"); return 20; }
                    if (!lr.read({&ls0, &ls1}, false).empty()) return 20;
                    if (lr.result(0, 2) != tr.read({&ts0, &ts1})) { std::printf("RegFile::read: the two banks differ\n"); return 20; }
                    lr.read_prepare_write(ls0, false);
                    if (!lr.state() || lr.old_result() != tr.read_prepare_write(ts0)) { std::printf("RegFile::read_prepare_write: the two banks differ\n"); return 20; }
                    lr.write(ls0, B::src_host(1), words);
                    tr.write(ts0, B::src_host(1), words);
                    if (lr.state() || lr.store() != tr.store()) { std::printf("RegFile::write: the two banks differ\n"); return 20; }
                    lr.read_prepare_write(ls0, false);
                    lr.write(ls0, B::src_regs_old());   // the old word put back, on the device
                    lr.pack({B::src_host(0), B::src_regs(1)}, words);
                    const auto want = lists.select({&ls0}, {{B::src_host(0), B::src_regs(1)}}, words);   // (before the read below replaces the last register read)
                    if (lr.read({&ls0}) != want) { std::printf("RegFile::pack + read differs from select\n"); return 20; }
                    try { lr.read({&ts0}); return 21; }   // a selector of another bank
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 21; }
                    try { lr.write(ls0, B::src_zero()); return 21; }   // no read_prepare_write before
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_STATE) return 21; }
                    std::printf("bank register file: read, read_prepare_write, write, pack: ok\n");
                }
                {   // Bank::read_prepare_write_mix: a read of member 1 and of the register file, the preparation of member 0 and of that
                    // register file under ONE top, against the twin's three calls; then both halves' writes
                    B::RegFile lr(lists, 1), tr(twin, 1);
                    const auto row = synth(4 * lists.glwe_len());
                    lr.load(row);
                    tr.load(row);
                    std::vector<fheram::Address*> ra = {&a1}, pa = {&a0};
                    const auto mixed = lists.read_prepare_write_mix({1}, ra, {}, {}, &lr, {&ls1}, {0}, pa, &lr, &ls0, bk);
                    const auto t_reads = twin.read_mix({1}, ra, {}, {}, &tr, {&ts1}, bk);
                    const auto t_list = twin.read_prepare_write_list({0}, pa, bk);
                    const auto t_old = tr.read_prepare_write(ts0);
                    if (mixed.reads.list != t_reads.list || mixed.reads.regs != t_reads.regs) { std::printf("read_prepare_write_mix: the reads differ\n"); return 25; }
                    if (mixed.prep_list != t_list || mixed.prep_regs != t_old) { std::printf("read_prepare_write_mix: the old words differ\n"); return 25; }
                    if (!lists.state(0) || lists.state(1) || !lr.state() || lr.old_result() != t_old) return 25;
                    lists.write_list({0}, {words[0]}, pa, bk);
                    twin.write_list({0}, {words[0]}, pa, bk);
                    lr.write(ls0, B::src_regs_old());
                    tr.write(ts0, B::src_regs_old());
                    for (int m = 0; m < 3; m++)
                        if (lists.state(m) || lists.store_encrypted(m) != twin.store_encrypted(m)) { std::printf("read_prepare_write_mix + write_list: member %d differs\n", m); return 25; }
                    if (lr.state() || lr.store() != tr.store()) { std::printf("read_prepare_write_mix + RegFile::write: the two banks differ\n"); return 25; }
                    try { std::vector<fheram::Address*> none; lists.read_prepare_write_mix({1}, ra, {}, {}, nullptr, {}, {}, none, nullptr, nullptr, bk); return 26; }   // no preparation: that is read_mix
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 26; }
                    std::printf("bank read_prepare_write_mix == read_mix, read_prepare_write_list, RegFile::read_prepare_write: ok\n");
                }
                {   // Bank::Table: a table of 2 words reads as a register file holding the same row does; a ROM of 4096 public words at a wide selector
                    B::Table lt(lists, 1), rom(lists, 12);
                    B::RegFile lr(lists, 1);
                    if (lt.bits() != 1 || rom.bits() != 12) return 22;
                    const auto row = synth(4 * lists.glwe_len());
                    lt.load(row);
                    lr.load(row);
                    if (lt.download() != row) { std::printf("Table: the row differs from what was loaded\n"); return 22; }
                    if (!lists.table_read({&lt, &lt}, {&ls0, &ls1}, false).empty()) return 22;
                    if (lists.table_result(0, 2) != lr.read({&ls0, &ls1})) { std::printf("table_read differs from RegFile::read of the same row\n"); return 22; }
                    const std::vector<std::vector<fheram::Glwe>> hw = {lists.table_result(1, 1)[0], words[0]};
                    if (lists.select({&ls0}, {{B::src_table(1), B::src_host(1)}}, hw) != lists.select({&ls0}, {{B::src_host(0), B::src_host(1)}}, hw)) { std::printf("src_table differs from the downloaded output\n"); return 22; }
                    std::vector<uint8_t> bytes(4096 * 4);
                    for (size_t i = 0; i < bytes.size(); i++) bytes[i] = (uint8_t)(i * 37 + 11);
                    rom.load_plain(bytes);
                    const auto plain = rom.download();
                    for (size_t i = 0; i < n; i++) if (plain[n + i] != 0) { std::printf("Table::load_plain: a mask limb is not zero\n"); return 22; }
                    const std::vector<int64_t> ipc = synth(14 * 4 * 2 * 5 * 2 * n);
                    B::FheUintPrepared pc(lists, ipc, 14);
                    B::Selector fetch(lists, B::Selector::Wide{}, 12), f66(lists, B::Selector::Wide{}, std::vector<int>{6, 6});
                    if (fetch.n_digits() != 4 || f66.n_digits() != 2) return 22;
                    lists.derive_list({B::derive_selector(pc, fetch, 2), B::derive_field(pc, f66, 0, 2), B::derive_field(pc, f66, 1, 8)});
                    if (lists.table_read({&rom, &rom}, {&fetch, &fetch}).size() != 2 || lists.table_read({&rom}, {&f66}).size() != 1) return 22;
                    try { lists.select({&fetch}, {{B::src_zero()}}); return 23; }   // a wide selector: the pack holds 32 candidates
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 23; }
                    try { lists.table_read({&lt}, {&fetch}); return 23; }   // 12 bits at a table of 1
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 23; }
                    try { B::Selector narrow(lists, 6); return 23; }   // fheram_bank_selector_alloc keeps its bound
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 23; }
                    std::printf("bank table: load, load_plain, table_read, table_result, wide selectors: ok\n");
                }
                {   // the public side: a public image into member 1 of both banks, a peek, a poke of a host word and of the old word back
                    std::vector<uint8_t> image(4096 * 4);
                    for (size_t i = 0; i < image.size(); i++) image[i] = (uint8_t)(i * 29 + 5);
                    lists.load_plain(1, image);
                    twin.load_plain(1, image);
                    const auto rows = lists.store_encrypted(1);
                    for (size_t i = 0; i < n; i++) if (rows[n + i] != 0) { std::printf("load_plain: a mask limb is not zero\n"); return 27; }
                    if (!lists.peek({1, 1}, {7, 4095}, false).empty()) return 27;
                    if (lists.peek_result(0, 2) != twin.peek({1, 1}, {7, 4095})) { std::printf("peek: the two banks differ\n"); return 27; }
                    if (lists.store_encrypted(1) != rows) { std::printf("peek changed the rows\n"); return 27; }
                    lists.poke({1}, {7}, {B::src_host(1)}, words);
                    twin.poke({1}, {7}, {B::src_host(1)}, words);
                    if (lists.store_encrypted(1) != twin.store_encrypted(1) || lists.store_encrypted(1) == rows) { std::printf("poke: the two banks differ\n"); return 27; }
                    lists.poke({1}, {7}, {B::src_peek(0)});   // the old word put back, on the device
                    B::RegFile lr(lists, 1);
                    lists.load_plain(lr, std::vector<uint8_t>(image.begin(), image.begin() + 8));
                    if (lr.state() || lr.store().size() != 4 * lists.glwe_len()) return 27;
                    try { lists.poke({1, 1}, {7, 7}, {B::src_zero(), B::src_zero()}); return 28; }   // one target twice
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 28; }
                    try { lists.peek({1}, {4096}); return 28; }   // an address outside the member
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 28; }
                    std::printf("bank public side: load_plain, peek, peek_result, poke: ok\n");
                }
                {   // Bank::scratch: a WIDE register file of 4096 words holds a public image; a peek, a poke and a write cycle at a wide selector
                    B::RegFile ls = lists.scratch(12), ts = twin.scratch(12);
                    if (ls.bits() != 12) return 29;
                    std::vector<uint8_t> image(4096 * 4);
                    for (size_t i = 0; i < image.size(); i++) image[i] = (uint8_t)(i * 41 + 3);
                    lists.load_plain(ls, image);
                    twin.load_plain(ts, image);
                    const auto row = ls.store();
                    if (!ls.peek({7, 4095}, false).empty()) return 29;
                    if (lists.peek_result(0, 2) != ts.peek({7, 4095})) { std::printf("RegFile::peek: the two banks differ\n"); return 29; }
                    if (ls.store() != row) { std::printf("RegFile::peek changed the row\n"); return 29; }
                    ls.poke({7, 2048}, {B::src_host(1), B::src_zero()}, words);
                    ts.poke({7, 2048}, {B::src_host(1), B::src_zero()}, words);
                    if (ls.store() != ts.store() || ls.store() == row) { std::printf("RegFile::poke: the two banks differ\n"); return 29; }
                    const std::vector<int64_t> ipc = synth(14 * 4 * 2 * 5 * 2 * n);
                    B::FheUintPrepared lpc(lists, ipc, 14), tpc(twin, ipc, 14);
                    B::Selector lw(lists, B::Selector::Wide{}, 12), tw(twin, B::Selector::Wide{}, 12);
                    lists.derive_list({B::derive_selector(lpc, lw, 2)});
                    twin.derive_list({B::derive_selector(tpc, tw, 2)});
                    if (ls.read({&lw}) != ts.read({&tw})) { std::printf("wide RegFile::read: the two banks differ\n"); return 29; }
                    if (ls.read_prepare_write(lw) != ts.read_prepare_write(tw) || !ls.state()) { std::printf("wide RegFile::read_prepare_write: the two banks differ\n"); return 29; }
                    ls.write(lw, B::src_host(0), words);
                    ts.write(tw, B::src_host(0), words);
                    if (ls.state() || ls.store() != ts.store()) { std::printf("wide RegFile::write: the two banks differ\n"); return 29; }
                    try { B::RegFile six(lists, 6); return 30; }   // fheram_bank_regs_create keeps its bound
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 30; }
                    try { ls.poke({7, 7}, {B::src_zero(), B::src_zero()}); return 30; }   // one target twice
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 30; }
                    try { ls.peek({4096}); return 30; }   // an index outside the register file
                    catch (const fheram::Error& e) { if (e.code != FHERAM_ERR_INVALID_ARG) return 30; }
                    std::printf("bank scratch: wide RegFile peek, poke, read, read_prepare_write, write: ok\n");
                }
            }
        }
    } catch (const fheram::Error& e) {
        if (e.code != FHERAM_ERR_DEVICE) { std::printf("unexpected error %d: %s\n", e.code, e.what()); return 4; }
        std::printf("no GPU: %s\n", e.what());
    }
    return 0;
}

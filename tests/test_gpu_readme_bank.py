"""The bank operations on the parameter block of the reference's README (README.md:17-34): K_PT = 9 and 5-limb trace / packing keys
(K_EVK_TRACE = 85).  tests/test_gpu_readme_params.py covers the context's own operations on that block; here every bank operation that
dispatches on the limb count of the trace keys, or encodes / decodes at k_glwe_pt, runs on it.

The 5-limb instantiations are kernels of their own (other limb loops, LDS and register footprints, a grid of TAIL_GROUPS * 2 * 5 * 3 = 240
workgroups for the tail), and at K_PT = 9 a byte read as signed (Ram::encrypt_sk, ram.rs:364: -128..127) and as unsigned (the example's
written words: 0..255) are DIFFERENT torus elements, which they are not up to K_PT = 8.  The contracts are those of the files the helpers
come from (test_gpu_mix.py, test_gpu_rpw_mix.py, test_gpu_select.py, test_gpu_lanes.py, test_gpu_regs.py, test_gpu_table.py,
test_gpu_public_io.py, test_gpu_bank_setup.py): every comparison is np.array_equal on int64 against the oracle under the same block.

Which launch ran is asserted through the profile classes: `keyswitch_tail_launch` is launch_trace_tail and the mix's top (k_trace_tail<3,5,3>,
k_trace_tail_t<3,5,3>, k_trace_tail_x<3,5,3> under these keys), and fheram_bank_tail_stats' fallbacks under tail_test = 1 are the predicated
launches behind them (k_keyswitch_chain<3,5,3>, k_read_chain<5,4>, k_read_chain_x<5,4>)."""
import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import sha
from test_gpu_bank_setup import NOISE_ABS
from test_gpu_lanes import VALUE_B, LaneWorld, identity
from test_gpu_mix import assert_oracle, assert_same, groups, keyed_bank, kit, results, singles, tail_launches
from test_gpu_public_io import N, RAGGED, _Zeros, check_poke, decrypts, enc_addr, opeek, rows_of
from test_gpu_regs import decrypts_to, oaddr, oram_of, orow, regs_rows, word_of
from test_gpu_regs import selector as narrow_selector
from test_gpu_rpw_mix import (RD, assert_member_is_oracle, assert_outputs, assert_snapshots, mix, oracle_member, rd_of, sequence, snapshot, twins,
                              write_both_halves)
from test_gpu_select import VALUE, host_srcs
from test_gpu_table import loaded_table, oracle_reads, wide

pytestmark = pytest.mark.gpu
README = {"k_glwe_pt": 9, "k_evk_trace": 85}
_BANKS = {}


@pytest.fixture(scope="module")
def r12(po):
    return LaneWorld(po, 1 << 12, 2, 2, seed=900, **README)


@pytest.fixture(scope="module")
def r13(po):
    return LaneWorld(po, 1 << 13, 2, 2, seed=910, **README)


@pytest.fixture(scope="module")
def r16(po):
    return LaneWorld(po, 1 << 16, 2, 2, seed=920, **README)


@pytest.fixture(scope="module")
def r12x4(po):
    return LaneWorld(po, 1 << 12, 2, 4, seed=930, **README)


@pytest.fixture(scope="module")
def r12x1(po):
    return LaneWorld(po, 1 << 12, 2, 1, seed=940, **README)


def world(request, shape):
    return request.getfixturevalue({12: "r12", 13: "r13", 16: "r16"}[shape])


def shared_bank(w):
    """one default bank per world for the tests that change no row"""
    if id(w) not in _BANKS:
        _BANKS[id(w)] = keyed_bank(w)
    return _BANKS[id(w)]


def test_the_worlds_are_on_the_readme_block(r12, r13):
    for w in (r12, r13):
        p = w.params
        assert (p.k_glwe_pt(), p.k_evk_trace(), p.k_evk_ggsw_inv()) == (9, 85, 85)
        assert all(k.size == 3 * 5 * 2 * N for k in w.keys.atk_glwe)
        ob = w.small(5)[0]   # the small oracles carry the block: 5-limb keys are prepared by a 5-limb oracle
        assert (ob.p.k_glwe_pt, ob.p.k_evk_trace, ob.p.atk_trace_len) == (9, 85, 3 * 5 * 2 * N)
        fo = w.field_oracle((2, 2))[0]
        assert (fo.p.k_glwe_pt, fo.p.k_evk_trace) == (9, 85)


# ---- 1. read_mix ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12, 16])
def test_read_mix_one_entry_of_each_kind(request, shape):
    """test_gpu_mix.py's test_one_entry_of_each_kind under 5-limb keys: product counts 1 / 4 / 2, 0 / 4 / 2 and 2 / 4 / 2.  One
    keyswitch_tail_launch for the top of the mix is k_trace_tail_x<3,5,3> at 2^12 and 2^16 (at 2^16 with a list entry's products inside it)."""
    w = world(request, shape)
    k = kit(w, shared_bank(w))
    assert w.po.get_base_2d(w.max_addr, [3, 3, 3, 3])[1:] == {12: [], 13: [[1]], 16: [[3, 1]]}[shape]
    assert (k.tsel[0].n_digits(), k.rsel[0].n_digits()) == (4, 2)
    lst, tabs, regs = groups(k, 1, 1, 1)
    n_list, _ = tail_launches(k.bank, lambda: k.bank.read_list(lst[0], lst[1], w.keys))
    n_seq, want = tail_launches(k.bank, lambda: singles(k, lst, tabs, regs))
    f0 = k.bank.tail_stats()["fallbacks"]
    n_mix, got = tail_launches(k.bank, lambda: k.bank.read_mix(lst, tabs, regs))
    assert k.bank.tail_stats()["fallbacks"] == f0, "the top of the mix gave up on an idle device"
    assert_same(got, want, shape)
    assert_same(results(k, lst, tabs, regs), want, (shape, "the _result downloads"))
    assert_oracle(k, got, 1, 1, 1)
    local = n_list - 1   # the list group's own stage
    print(f"readme 2^{shape}: keyswitch_tail_launch {n_mix} for the mix, {n_seq} for the three single calls, {n_list} for the read list alone")
    assert local == (1 if shape == 13 else 0), (shape, n_list)
    assert (n_mix, n_seq) == (1 + local, 3 + local), (shape, n_mix, n_seq, n_list)
    assert sha(k.t.download()) == sha(k.trow) and sha(k.rf.store()) == sha(k.rrow) and not k.rf.state() and not k.bank.state(1)
    assert np.array_equal(k.bank.result(1, 1)[0], got[0][0])


@pytest.mark.parametrize("shape", [13, 12, 16])
def test_read_mix_tail_gives_up_and_the_fallback_redoes_it(request, shape):
    """tail_test = 1 (the designed give-up): the same int64, and the launch and fallback deltas of test_gpu_mix.py — the fallback of the top
    is k_read_chain_x<5,4> where ciphertexts have products in the tail (2^12, 2^16)"""
    w = world(request, shape)
    kd = kit(w, shared_bank(w))
    default = kd.bank.read_mix(*groups(kd, 1, 1, 1))
    k = kit(w, keyed_bank(w, {"tail_test": 1}))
    lst, tabs, regs = groups(k, 1, 1, 1)

    def delta(run):
        a = k.bank.tail_stats()
        out = run()
        b = k.bank.tail_stats()
        return b["launches"] - a["launches"], b["fallbacks"] - a["fallbacks"], out

    l_list, f_list, _ = delta(lambda: k.bank.read_list(lst[0], lst[1], w.keys))
    l_mix, f_mix, got = delta(lambda: k.bank.read_mix(lst, tabs, regs))
    assert_same(got, default, (shape, "tail_test"))
    print(f"readme 2^{shape} tail_test: the mix {l_mix} tail launches, {f_mix} fallbacks; a read list alone {l_list}, {f_list}")
    local = 1 if shape == 13 else 0
    assert (l_list, f_list) == (1 + local, 1 + local), (shape, l_list, f_list)
    assert l_mix == 1 + local, (shape, l_mix)
    assert f_mix - local == (2 if shape == 12 else 1), (shape, f_mix)


def test_read_mix_at_word_size_4(r12x4):
    """list + regs = 8 ciphertexts, the bound of the one-launch top (one keyswitch_tail_launch against two); table + regs + list = 12, the
    unfused form"""
    w = r12x4
    k = kit(w, shared_bank(w))
    lst, tabs, regs = groups(k, 1, 0, 1)
    n_seq, want = tail_launches(k.bank, lambda: singles(k, lst, tabs, regs))
    n_mix, got = tail_launches(k.bank, lambda: k.bank.read_mix(lst, tabs, regs))
    assert_same(got, want, "Y = 8")
    assert_oracle(k, got, 1, 0, 1)
    assert (n_mix, n_seq) == (1, 2), (n_mix, n_seq)
    lst, tabs, regs = groups(k, 1, 1, 1)
    want = singles(k, lst, tabs, regs)
    got = k.bank.read_mix(lst, tabs, regs)
    assert_same(got, want, "Y = 12")
    assert_oracle(k, got, 1, 1, 1)


def test_read_mix_at_word_size_1(r12x1):
    """Y = 3: the groups sit at consecutive ciphertext indices, so per-group pointers, digits and counts change at every index"""
    w = r12x1
    k = kit(w, shared_bank(w))
    lst, tabs, regs = groups(k, 1, 1, 1)
    n_seq, want = tail_launches(k.bank, lambda: singles(k, lst, tabs, regs))
    n_mix, got = tail_launches(k.bank, lambda: k.bank.read_mix(lst, tabs, regs))
    assert_same(got, want, "Y = 3")
    assert_oracle(k, got, 1, 1, 1)
    assert (n_mix, n_seq) == (1, 3), (n_mix, n_seq)


@pytest.mark.parametrize("shape", [13, 12])
@pytest.mark.parametrize("config", [{"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}], ids=["safe_monitor2", "tail0_fuse0"])
def test_read_mix_under_other_configurations(request, shape, config):
    w = world(request, shape)
    kd = kit(w, shared_bank(w))
    default = kd.bank.read_mix(*groups(kd, 1, 1, 1))
    k = kit(w, keyed_bank(w, config))
    lst, tabs, regs = groups(k, 1, 1, 1)
    got = k.bank.read_mix(lst, tabs, regs)
    assert_same(got, default, (shape, config))
    assert_same(got, singles(k, lst, tabs, regs), (shape, config, "the single calls under the same configuration"))
    print(f"readme mix 2^{shape} {config}: round-off maximum {k.bank.roundoff_max():.4f}")   # (raises FHERAM_ERR_PRECISION above 3/8)


# ---- 2. read_prepare_write_mix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,config", [(13, None), (16, None), (13, {"memo": 0})], ids=["2p13", "2p16", "2p13-memo0"])
def test_rpw_mix_a_full_step(request, shape, config):
    """list, table, regs, a prepared list of both members and the prepared register file: the five outputs and everything left on the bank
    equal the sequence on a twin; then write_list and RegFile.write on both, and every member's rows and the register file's row are the
    oracle's (k_mix_scatter behind a 5-limb top)"""
    w = world(request, shape)
    S, a = w.pkg.Src, w.addrs
    km, kt = twins(w, config)
    plist = ([1, 0], [a[1], a[2]])
    reads = groups(km, 1, 1, 1)
    got = mix(km, reads, plist, rd_of(km))
    want = sequence(kt, groups(kt, 1, 1, 1), plist, rd_of(kt))
    assert_outputs(got, want, (shape, config))
    assert_snapshots(snapshot(km, results=(0, 1), old=True), snapshot(kt, results=(0, 1), old=True), (shape, config))
    assert km.bank.state(0) and km.bank.state(1) and km.rf.state()
    assert_oracle(km, got[:3], 1, 1, 1)
    oms = {}
    for e, (m, j) in enumerate(zip(plist[0], (1, 2))):
        oms[m], old = oracle_member(w, m, j)
        assert np.array_equal(got[3][e], old), ("the old word is not the oracle's", m)
        assert_member_is_oracle(km, m, oms[m], (shape, config, m))
    oram, okeys = oram_of(w, km.rb, km.rrow), w.small(km.rb)[1]
    assert np.array_equal(got[4], oram.read_prepare_write(oaddr(w, RD, km.rb), okeys))
    assert np.array_equal(km.rf.store(), orow(w, oram))
    vals, cts = w.candidates(3, seed=52)
    write_both_halves((km, kt), cts, plist, True, S)
    assert_snapshots(snapshot(km), snapshot(kt), (shape, config, "after the writes"))
    for e, (m, j) in enumerate(zip(plist[0], (1, 2))):
        oms[m].write(cts[e], w.o.address_new(w.addr_g[j]), w.okeys)
        assert np.array_equal(km.bank.store_encrypted(m), oms[m].store()), (shape, config, "rows after the write", m)
        assert not km.bank.state(m)
    oram.write(cts[2], oaddr(w, RD, km.rb), okeys)
    assert np.array_equal(km.rf.store(), orow(w, oram)) and not km.rf.state()
    back = km.bank.read([a[2]], w.keys, first=0)
    assert np.array_equal(back[0], oms[0].read(w.o.address_new(w.addr_g[2]), w.okeys))
    w.check_value(back[0], vals[1], "the word written to member 0")


# ---- 3. select, select_lanes, the register file, table_read ---------------------------------------------------------------------------------------
def profiled_tail(bank, run):
    """(keyswitch_tail_launch launches, fallbacks the run took, its output)"""
    f0 = bank.tail_stats()["fallbacks"]
    n, out = tail_launches(bank, run)
    return n, bank.tail_stats()["fallbacks"] - f0, out


def test_select_and_select_lanes(r12):
    """b = 5 (two digits), m = 20 against SelWorld.oselect; lanes swapped on host candidates; a (2, 2) field selector against the field
    oracle under the block.  Each is one keyswitch_tail_launch (launch_trace_tail under with_evk: sk = 5) and no fallback."""
    w, pkg, L = r12, r12.pkg, r12.pkg.Lane
    bank = shared_bank(w)
    b, m, idx = 5, 20, 19
    vals, cts = w.candidates(m)
    n, fb, got = profiled_tail(bank, lambda: bank.select([w.selector(bank, idx, b)], [host_srcs(pkg, m)], host_words=cts))
    want = w.oselect(b, cts, w.index_digits(idx, b))
    assert np.array_equal(got[0], want), np.count_nonzero(got[0] != want)
    assert (n, fb) == (1, 0), (n, fb)
    print(f"readme select b={b} m={m}: log2 noise {w.check_value(got[0], vals[idx]):.2f}")
    # lanes: candidate 0 with its two bytes swapped, candidate 1 as it is
    lanes = [[[L.host(0, 1), L.host(0, 0)], [L.host(1, 0), L.host(1, 1)]]]
    for i in (0, 1):
        n, fb, got = profiled_tail(bank, lambda: bank.select_lanes([w.selector(bank, i, 1)], lanes, host_words=cts))
        want = w.oselect(1, np.stack([cts[0][::-1], cts[1]]), w.index_digits(i, 1))
        assert np.array_equal(got[0], want), (i, np.count_nonzero(got[0] != want))
        assert (n, fb) == (1, 0), (i, n, fb)
    w.check_value(got[0], vals[1], "lanes, candidate 1")
    # a field selector: digit 0 from bits [3, 5) of one integer, digit 1 from bits [11, 13) of another
    widths, index = (2, 2), ((VALUE >> 3) & 3) | (((VALUE_B >> 11) & 3) << 2)
    digits = w.field_digits(widths, [VALUE, VALUE_B], [3, 11])
    sel = pkg.Selector.from_digits_fields(bank, list(widths), list(digits))
    got = bank.select_lanes([sel], [identity(pkg, host_srcs(pkg, 16), w.ws)], host_words=cts)
    want = w.oselect_fields(widths, cts[:16], digits)
    assert np.array_equal(got[0], want), np.count_nonzero(got[0] != want)
    w.check_value(got[0], vals[index], ("field selector", index))


def test_regfile_cycle(r12):
    """test_gpu_regs.py's write cycle at b = 5, with the read's and the write's launch classes"""
    w, S = r12, r12.pkg.Src
    b, idx = 5, 19
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=43)
    bank = keyed_bank(w)
    rf = bank.regfile(b)
    rf.load(row)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    sel = narrow_selector(w, bank, idx, b)
    n, fb, got = profiled_tail(bank, lambda: rf.read([sel]))
    assert np.array_equal(got[0], oram.read(oaddr(w, idx, b), okeys))
    assert (n, fb) == (1, 0), (n, fb)
    decrypts_to(w, got[0], word_of(w, data, idx), False, "the word read")
    old = rf.read_prepare_write(sel)
    assert np.array_equal(old, oram.read_prepare_write(oaddr(w, idx, b), okeys))
    assert np.array_equal(rf.store(), orow(w, oram)), "the rotated row"
    rf.write(sel, S.host(0), host_words=cts)
    oram.write(cts[0], oaddr(w, idx, b), okeys)
    assert np.array_equal(rf.store(), orow(w, oram)), "the row after the write"
    assert not rf.state()
    others = [0, 31]
    got = rf.read([sel] + [narrow_selector(w, bank, i, b) for i in others])
    for k, i in enumerate([idx] + others):
        want = oram.read(oaddr(w, i, b), okeys)
        assert np.array_equal(got[k], want), (i, np.count_nonzero(got[k] != want))
    noise = decrypts_to(w, got[0], vals[0], True, "the written word")
    print(f"readme regs write cycle: log2 noise of the written word {noise:.2f}, round-off maximum {bank.roundoff_max():.4f}")


@pytest.mark.parametrize("b", [6, 12])
def test_table_read(r12, b):
    """2 and 4 digits; three entries in one call (6 ciphertexts: the table form of the tail launch, k_trace_tail_t<3,5,3>)"""
    w = r12
    bank = shared_bank(w)
    t, data, row = loaded_table(w, bank, b)
    idxs = [0, (1 << b) - 1, (1 << b) // 2 + 5]
    sels = [wide(w, bank, i, b) for i in idxs]
    assert sels[0].n_digits() == b // 3
    n, fb, got = profiled_tail(bank, lambda: bank.table_read([t] * 3, sels))
    for k, (idx, want) in enumerate(zip(idxs, oracle_reads(w, b, row, idxs))):
        assert np.array_equal(got[k], want), (b, idx, np.count_nonzero(got[k] != want))
    assert (n, fb) == (1, 0), (n, fb)
    print(f"readme table read b={b}: log2 noise {decrypts_to(w, got[2], word_of(w, data, idxs[2]), False):.2f}")
    assert sha(t.download()) == sha(row)


# ---- 4. the public side at k_pt = 9 ----------------------------------------------------------------------------------------------------------------
def every_byte(count, seed):
    """`count` bytes in which every value 0..255 appears (count >= 256): all of them in order first — the signed and the unsigned reading of
    128..255 differ by 1/2 at k_pt = 9 — then the generator's"""
    assert count >= 256
    data = np.concatenate([np.arange(256), np.random.default_rng(seed).integers(0, 256, size=count - 256)]).astype(np.uint8)
    assert set(data[:256].tolist()) == set(range(256))
    return data


def plain(o, values, written):
    return np.array([o.expected_plain(int(x), 9, written) for x in np.ravel(values)], dtype=np.int64)


@pytest.mark.parametrize("max_addr", [1 << 13, RAGGED], ids=["2p13", "ragged"])
def test_load_plain_of_every_byte_at_k_pt_9(po, max_addr):
    """load_plain of a member, of a 5-bit register file and of a table: the same object's encrypt_sk fed a zero mask and zero noise, and the
    bank's own decrypt gives expected_plain(byte, 9, written=False): -128..127"""
    pkg = load_package()
    ws = 2
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=ws, **README))
    assert o.expected_plain(255, 9, False) == -1 and o.expected_plain(255, 9, True) == 255 and o.expected_plain(128, 9, False) == -128
    sk = o.secret_gen(9300)
    p = pkg.Parameters(max_addr=max_addr, word_size=ws, **README)
    bank = pkg.RamBank(p, 2)
    bsk = pkg.GLWESecret(bank, sk)
    data = every_byte(max_addr * ws, 9301 + max_addr)
    bank.load_plain(0, data)
    rows = bank.store_encrypted(0)
    bank.encrypt_sk(1, data, bsk, _Zeros(), _Zeros())
    want = bank.store_encrypted(1)
    assert np.array_equal(rows, want), np.count_nonzero(rows != want)
    for a in (0, 64, 127, max_addr - 1):   # the oracle's own decryption of single coefficients: bytes 0, 1, 128, 129, 254, 255 among them
        for i in range(ws):
            want_v = o.expected_plain(int(data[i + ws * a]), 9, False)
            v, noise = o.glwe_decrypt(rows[i][a // N], want_v, sk, a % N)
            assert v == want_v and noise < -o.p.k_glwe_ct, (a, i, v, want_v, noise)
    vals, worst = bank.decrypt(0, bsk)
    assert np.array_equal(vals, plain(o, data, False).reshape(max_addr, ws))
    assert vals.min() == -128 and vals.max() == 127
    rf, twin = bank.regfile(5), bank.regfile(5)
    d5 = np.arange(3, 256, 4, dtype=np.uint8)   # 32 words of 2 bytes: 3, 7, .., 255
    assert d5.size == 32 * ws
    rf.load_plain(d5)
    twin.encrypt_sk(d5, bsk, _Zeros(), _Zeros())
    assert np.array_equal(rf.store(), twin.store())
    assert np.array_equal(rf.decrypt(bsk)[0], plain(o, d5, False).reshape(32, ws))
    tdata = every_byte(128 * ws, 9302)
    t, ttwin = bank.table(7), bank.table(7)
    t.load_plain(tdata)
    ttwin.encrypt_sk(tdata, bsk, _Zeros(), _Zeros())
    assert np.array_equal(t.download(), ttwin.download())
    tv = t.decrypt(bsk)[0]
    assert np.array_equal(tv, plain(o, tdata, False).reshape(128, ws)) and tv.min() == -128 and tv.max() == 127


def test_poke_peek_and_read_of_bytes_128_to_255(r13):
    """host words encrypted from bytes 128..255 are poked, peeked and read at encrypted addresses: opoke / opeek / the oracle, and they decrypt
    to expected_plain(byte, 9, written=True) = +128..+255, while a LOADED 255 beside them decrypts to -1.  decrypt_sources on Src.peek, a
    member result and a table result gives the same values and the oracle's noise."""
    w, pkg, S = r13, r13.pkg, r13.pkg.Src
    o = w.o
    bank = keyed_bank(w)
    dsk = pkg.GLWESecret(bank, w.sk)
    rows = rows_of(w)
    bytes_ = np.array([[128, 255], [200, 129], [254, 191]], dtype=np.uint8)
    cts = np.stack([np.stack([o.glwe_encrypt_coeff0(int(v), w.sk, 9400 + 2 * k + i, 9450 + 2 * k + i) for i, v in enumerate(bytes_[k])]) for k in range(3)])
    members, addrs = [0, 1, 1], [7, N - 1, N + 3]
    want = check_poke(w, bank, rows, members, addrs, cts)
    got = bank.peek(members, addrs)
    for k, (m, a) in enumerate(zip(members, addrs)):
        assert np.array_equal(got[k], opeek(w, want, m, a)), (k, m, a)
        noise = decrypts(w, got[k], bytes_[k], True, ("peek", k))
        assert noise < -(9 + 1), noise
    values, noise = bank.decrypt_sources(dsk, [S.peek(0), S.peek(2)])
    assert np.array_equal(values, np.array([[128, 255], [254, 191]]))
    # an oblivious read of a poked word: a member result
    addr, oad = enc_addr(w, addrs[2], seed=3)
    read = bank.read([addr], w.keys, first=1)[0]
    oram = o.ram_new()
    oram.load(want[1])
    assert np.array_equal(read, oram.read(oad, w.okeys))
    assert decrypts(w, read, bytes_[2], True, "the oblivious read") < -(9 + 1)
    # a table loaded with 255s reads -1: the loaded reading of the same byte
    t = bank.table(6)
    tdata = np.full(64 * w.ws, 255, dtype=np.uint8)
    t.load_plain(tdata)
    tres = bank.table_read([t], [wide(w, bank, 33, 6)])[0]
    srcs = [S.peek(1), S.member(1), S.table(0)]
    ctl = [got[1], read, tres]
    values, noise = bank.decrypt_sources(dsk, srcs)
    assert np.array_equal(values, np.array([[200, 129], [254, 191], [-1, -1]])), values
    for k, ct in enumerate(ctl):
        for i in range(w.ws):
            ov, onoise = o.glwe_decrypt(ct[i], int(values[k, i]), w.sk)
            assert ov == int(values[k, i]) and noise[k, i] == pytest.approx(onoise, abs=NOISE_ABS), (k, i, noise[k, i], onoise)


# ---- 5. setup on the device --------------------------------------------------------------------------------------------------------------------------
def test_setup_on_the_device_equals_the_oracle(r13):
    """keys (5-limb automorphism keys), a member, an address, a narrow and a 12-bit table selector and words, each from the oracle's seeded
    sources replayed"""
    w, pkg, o = r13, r13.pkg, r13.o
    bank = w.new_bank(2)
    dsk = pkg.GLWESecret(bank, w.sk)
    keys = pkg.EvaluationKeysPrepared.encrypt_sk(bank, dsk, o.source(9501), o.source(9502), keep_std=True)
    evk2 = o.evk_gen(w.sk, 9501, 9502)
    assert keys.atk_glwe[0].size == 3 * 5 * 2 * N
    for i in range(12):
        assert np.array_equal(keys.atk_glwe[i], evk2["atk_glwe"][i].ravel()), i
    assert np.array_equal(keys.tsk_ggsw_inv, evk2["tsk"].ravel()) and np.array_equal(keys.atk_ggsw_inv, evk2["atk_ggsw_inv"].ravel())
    data = every_byte(w.max_addr * w.ws, 9503)
    bank.encrypt_sk(1, data, dsk, o.source(9504), o.source(9505))
    assert np.array_equal(bank.store_encrypted(1), o.ram_encrypt(data, w.sk, 9504, 9505))
    vals, worst = bank.decrypt(1, dsk)
    assert np.array_equal(vals, plain(o, data, False).reshape(w.max_addr, w.ws)) and worst < -(9 + 1)
    for value in (0, 4097, (1 << 13) - 1):
        addr = pkg.Address.encrypt_sk(bank, value, dsk, o.source(9510), o.source(9511))
        assert np.array_equal(bank.address_digits(addr), o.address_encrypt(value, w.sk, 9510, 9511)), value
    for b, mk, value in ((5, lambda: bank.selector(5), 19), (12, lambda: bank.table_selector(12), 3001)):
        ob = w.small(b)[0]
        sel = mk()
        sel.encrypt_sk(value, dsk, ob.source(9520 + b), ob.source(9540 + b))
        assert np.array_equal(sel.download(), ob.address_encrypt(value, w.sk, 9520 + b, 9540 + b)), b
    bytes_ = [0, 127, 128, 255]
    words = bank.encrypt_word(dsk, bytes_, o.source(9530), o.source(9531))
    assert np.array_equal(words[0], o.glwe_encrypt_coeff0(bytes_[0], w.sk, 9530, 9531))
    wants = [o.expected_plain(v, 9, True) for v in bytes_]
    assert wants == [0, 127, 128, 255]
    for (v, noise), want, ct in zip(bank.decrypt_coeff(dsk, words, wants), wants, words):
        ov, onoise = o.glwe_decrypt(ct, want, w.sk)
        assert v == want == ov and noise == pytest.approx(onoise, abs=NOISE_ABS)
    # the keys made on the device read the member encrypted on the device
    got = bank.read([w.addrs[0]], keys, first=1)[0]
    oram = o.ram_new()
    oram.load(bank.store_encrypted(1))
    assert np.array_equal(got, oram.read(o.address_new(w.addr_g[0]), o.keys_prepare(evk2)))

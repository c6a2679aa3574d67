"""The setup side of a bank (include/fheram.h "Setup side of a bank"): keys, members, register files, tables, addresses,
selectors, encrypted integers and words encrypted on the bank's device from host-drawn randomness, and what a bank leaves on the device
decrypted and decoded there (k_decrypt_decode).

The contract, in the oracle's own operations: with the oracle's seeded `Source` replayed on the host (as tests/test_gpu_setup.py does),
every device encryption is np.array_equal on int64 to the oracle's — a member's rows to Oracle.ram_encrypt, a register file's or a table's
row to the ram_encrypt of the small oracle of max_addr = 2^bits, a selector's digits to that oracle's address_encrypt (a field selector:
the oracle whose DECOMP_N is the widths, padded).  A decoded value is exactly Oracle.glwe_decrypt's; a noise figure equals it to
abs = 1e-9, the tolerance tests/test_gpu_setup.py uses for the same quantity (both sides take log2 of the same exact integer).
Banks are at max_addr = 2^13 (two rows per word), word_size 2, two members unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import World, lib, member_snapshot, sha
from test_gpu_regs import oram_of
from test_gpu_select import N_BITS, VALUE, SelWorld

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED = 1, 2, 3
I64P = C.POINTER(C.c_int64)
NOISE_ABS = 1e-9


def decode(o, pt):
    """decode_coeff_i64 + the example's rounding (examples/fhe-ram.rs:224-237) of normalised phase limbs pt [3][N], vectorised in int64:
    (res, value), as Oracle.glwe_decrypt forms them (oracle/setup.hpp decrypt_glwe)"""
    k, k_pt, b2k = o.p.k_glwe_ct, o.p.k_glwe_pt, o.p.base2k
    rem = b2k - (k % b2k)
    hi = (pt[0] << b2k) + pt[1]
    res = (hi << (b2k - rem)) + (pt[2] >> rem) if rem != b2k else (hi << b2k) + pt[2]
    ls = k - k_pt
    mag = (np.abs(res) + (1 << (ls - 1))) >> ls if ls > 0 else np.abs(res)
    return res, np.where(res < 0, -mag, mag)


def host_rows_decode(o, sk, rows, max_addr):
    """rows [ws][rows][GLWE] -> (values [max_addr][ws], worst log2 noise against each coefficient's own decoded value)"""
    ws, n_rows = rows.shape[0], rows.shape[1]
    n, k, ls = o.p.n, o.p.k_glwe_ct, o.p.k_glwe_ct - o.p.k_glwe_pt
    values = np.zeros((max_addr, ws), dtype=np.int64)
    top = 0
    for w in range(ws):
        for r in range(n_rows):
            res, val = decode(o, o.glwe_phase(rows[w, r], sk))
            cnt = min(n, max_addr - r * n)
            values[r * n:r * n + cnt, w] = val[:cnt]
            top = max(top, int(np.abs(res - (val << ls))[:cnt].max()))
    return values, (float(np.log2(top)) - k if top else float("-inf"))


def check_decode_helper(o, sk, ct, coeffs):
    """the helper above IS the oracle's decrypt: value and noise at a few coefficients"""
    res, val = decode(o, o.glwe_phase(ct, sk))
    ls = o.p.k_glwe_ct - o.p.k_glwe_pt
    for i in coeffs:
        v, noise = o.glwe_decrypt(ct, int(val[i]), sk, coeff=i)
        d = abs(int(res[i]) - (int(val[i]) << ls))
        assert v == int(val[i]) and noise == pytest.approx(float(np.log2(d)) - o.p.k_glwe_ct if d else float("-inf"), abs=NOISE_ABS)


@pytest.fixture(scope="module")
def w13(po):
    return SelWorld(po, 1 << 13, 2, 2, seed=500)


@pytest.fixture(scope="module")
def shared(w13):
    """one bank of two loaded members under the world's keys, with the world's secret on it: for the tests that change no member's rows"""
    bank = w13.new_bank(2)
    bank._use_keys(w13.keys)
    return bank, w13.pkg.GLWESecret(bank, w13.sk)


def field_oracle(w, max_addr, decomp):
    ob = w.po.Oracle(w.oparams(max_addr, decomp_n=decomp))
    return ob, ob.keys_prepare(w.evk)


def c_data(data):
    return data.ctypes.data_as(C.POINTER(C.c_uint8))


# ---- 1. members ---------------------------------------------------------------------------------------------------------------------------
def test_member_encrypted_on_the_device_equals_the_oracle(w13):
    w, pkg, o = w13, w13.pkg, w13.o
    bank = w.new_bank(2)
    dsk = pkg.GLWESecret(bank, w.sk)
    before = member_snapshot(bank, 0)
    bank.read_prepare_write([w.addrs[0]], w.keys, first=1)      # member 1 is between its two halves: the encryption resets it
    data = np.random.default_rng(81).integers(0, 256, size=w.max_addr * w.ws, dtype=np.uint8)
    bank.encrypt_sk(1, data, dsk, o.source(8101), o.source(8102))
    assert np.array_equal(bank.store_encrypted(1), o.ram_encrypt(data, w.sk, 8101, 8102))
    assert not bank.state(1)
    after = member_snapshot(bank, 0)
    assert sha(after[0]) == sha(before[0]) and sha(after[1]) == sha(before[1]) and after[2] == before[2], "member 0 changed"
    # the member reads like any other
    got = bank.read([w.addrs[1]], w.keys, first=1)[0]
    oram = o.ram_new()
    oram.load(bank.store_encrypted(1))
    assert np.array_equal(got, oram.read(o.address_new(w.addr_g[1]), w.okeys))
    # refusals: the reference's messages, and nothing changes
    rows = sha(bank.store_encrypted(1))
    for bad in (data[:-2], data[:-1]):
        with pytest.raises(pkg.FheRamError, match="invalid data"):
            bank.encrypt_sk(1, bad, dsk, o.source(1), o.source(2))
    mask = o.source(1).uniform_limbs(w.ws * 2 * 3 * 4096)
    noise = np.zeros(w.ws * 2 * 4096, dtype=np.int64)
    L = lib()
    assert L.fheram_bank_ram_encrypt_sk(bank._h, 2, dsk._h, c_data(data), data.size, mask.ctypes.data_as(I64P), noise.ctypes.data_as(I64P)) == ST_INVALID_ARG
    assert b"no such member" in L.fheram_bank_last_error(bank._h)
    with pytest.raises(pkg.FheRamError, match="mask limb"):   # a bad draw is found before a row is written
        class Bad:
            def uniform_limbs(self, count):
                a = np.zeros(count, dtype=np.int64)
                a[-1] = 1 << 16
                return a

            def gaussian(self, count, scale):
                return np.zeros(count, dtype=np.int64)
        bank.encrypt_sk(1, data, dsk, Bad(), Bad())
    assert sha(bank.store_encrypted(1)) == rows and not bank.state(1)


def test_ragged_member_and_its_decrypt(po):
    """max_addr = 5000, word_size 3: the last row holds 904 words and zero padding behind them"""
    w = World(po, 5000, 1, word_size=3, seed=510, n_addr=1)
    pkg, o = w.pkg, w.o
    bank = w.new_bank(1, load=False)
    dsk = pkg.GLWESecret(bank, w.sk)
    with pytest.raises(pkg.FheRamError) as e:
        bank.decrypt(0, dsk)
    assert e.value.code == ST_UNINITIALIZED
    bank.encrypt_sk(0, w.data[0], dsk, o.source(8201), o.source(8202))
    rows = o.ram_encrypt(w.data[0], w.sk, 8201, 8202)
    assert np.array_equal(bank.store_encrypted(0), rows)
    values, worst = bank.decrypt(0, dsk)
    want, want_worst = host_rows_decode(o, w.sk, rows, 5000)
    check_decode_helper(o, w.sk, rows[2, 1], [0, 903])
    assert values.dtype == np.int32 and values.shape == (5000, 3) and np.array_equal(values, want)
    assert worst == pytest.approx(want_worst, abs=NOISE_ABS)
    model = np.array([o.expected_plain(int(b), o.p.k_glwe_pt) for b in w.data[0]]).reshape(5000, 3)
    assert np.array_equal(values, model)
    assert sha(bank.store_encrypted(0)) == sha(rows) and not bank.state(0)


# ---- 2. register files and tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,b", [("regs", 1), ("regs", 5), ("table", 7), ("table", 12)])
def test_one_row_objects_encrypted_on_the_device(w13, shared, kind, b):
    w, pkg, (bank, dsk) = w13, w13.pkg, shared
    ob, okeys = w.small(b)
    data = np.random.default_rng(8300 + b).integers(0, 256, size=(1 << b) * w.ws, dtype=np.uint8)
    obj = bank.regfile(b) if kind == "regs" else bank.table(b)
    with pytest.raises(pkg.FheRamError) as e:
        obj.decrypt(dsk)
    assert e.value.code == ST_UNINITIALIZED
    with pytest.raises(pkg.FheRamError, match="invalid data"):
        obj.encrypt_sk(data[:-1], dsk, ob.source(1), ob.source(2))
    obj.encrypt_sk(data, dsk, ob.source(8310 + b), ob.source(8320 + b))
    row = ob.ram_encrypt(data, w.sk, 8310 + b, 8320 + b).reshape(w.ws, -1)
    got_row = obj.store() if kind == "regs" else obj.download()
    assert np.array_equal(got_row, row)
    # a read at a selector encrypted on the device equals the oracle's read
    idx = (1 << b) - 1 if b > 1 else 1
    sel = bank.selector(b) if kind == "regs" else bank.table_selector(b)
    sel.encrypt_sk(idx, dsk, ob.source(8330 + b), ob.source(8340 + b))
    digits = sel.download()
    assert np.array_equal(digits, ob.address_encrypt(idx, w.sk, 8330 + b, 8340 + b))
    got = obj.read([sel])[0] if kind == "regs" else bank.table_read([obj], [sel])[0]
    assert np.array_equal(got, oram_of(w, b, row).read(ob.address_new(digits), okeys))
    # the whole object, decrypted and decoded on the device
    values, worst = obj.decrypt(dsk)
    want, want_worst = host_rows_decode(ob, w.sk, row.reshape(w.ws, 1, -1), 1 << b)
    assert values.shape == (1 << b, w.ws) and np.array_equal(values, want)
    assert worst == pytest.approx(want_worst, abs=NOISE_ABS)
    assert np.array_equal(values, np.array([ob.expected_plain(int(x), ob.p.k_glwe_pt) for x in data]).reshape(-1, w.ws))
    after = obj.store() if kind == "regs" else obj.download()
    assert sha(after) == sha(row), "the decrypt changed the row"
    if kind == "regs":
        obj.read_prepare_write(sel, download=False)
        with pytest.raises(pkg.FheRamError) as e:
            obj.decrypt(dsk)
        assert e.value.code == ST_STATE and obj.state()


# ---- 3. selectors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["b1", "b3", "b5", "f22", "f66", "t12"])
def test_selectors_encrypted_in_place(w13, shared, form):
    w, pkg, (bank, dsk) = w13, w13.pkg, shared
    if form[0] == "b":
        bits = int(form[1])
        ob, mk = w.small(bits)[0], lambda: bank.selector(bits)
    elif form == "t12":
        bits = 12
        ob, mk = w.small(12)[0], lambda: bank.table_selector(12)
    elif form == "f22":
        bits = 4
        ob, mk = field_oracle(w, 16, [2, 2, 2, 2, 2, 2])[0], lambda: bank.selector_fields([2, 2])
        assert w.po.get_base_2d(16, [2, 2, 2, 2, 2, 2]) == [[2, 2]]
    else:
        bits = 12
        ob, mk = field_oracle(w, 1 << 12, [6, 6])[0], lambda: bank.table_selector_fields([6, 6])
        assert w.po.get_base_2d(1 << 12, [6, 6]) == [[6, 6]]
    sel = mk()
    assert sel.n_digits() == ob.n_digits
    mid = (0b101101101101 & ((1 << bits) - 1)) | (1 << (bits - 1)) if bits > 1 else 1
    for j, value in enumerate([0, mid, (1 << bits) - 1]):
        sel.encrypt_sk(value, dsk, ob.source(8400 + j), ob.source(8450 + j))     # (the second and third: over digits it already holds)
        assert np.array_equal(sel.download(), ob.address_encrypt(value, w.sk, 8400 + j, 8450 + j)), (form, value)
    held = sha(sel.download())
    with pytest.raises(pkg.FheRamError, match=r"base2d.max\(\) > value") as e:      # address.rs:98
        sel.encrypt_sk(1 << bits, dsk, ob.source(1), ob.source(2))
    assert e.value.code == ST_INVALID_ARG and sha(sel.download()) == held
    if form == "b3":   # in place over a derivation, and the refusals of foreign handles
        fu = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))
        bank.derive_selectors([fu], [4], [sel])
        assert np.array_equal(sel.download(), w.digits(VALUE, 4, 3))
        sel.encrypt_sk(5, dsk, ob.source(8460), ob.source(8461))
        assert np.array_equal(sel.download(), ob.address_encrypt(5, w.sk, 8460, 8461))
        other = w.new_bank(1, load=False)
        osk, osel = pkg.GLWESecret(other, w.sk), other.selector(3)
        L = lib()
        n = sel.n_digits() * 3 * 2 * 4096
        mask, noise = np.zeros(n * 4, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for b_, s_, k_ in ((bank, osel, dsk), (bank, sel, osk), (bank, None, dsk), (bank, sel, None)):
            rc = L.fheram_bank_selector_encrypt_sk(b_._h, k_._h if k_ else None, s_._h if s_ else None, 1, mask.ctypes.data_as(I64P), noise.ctypes.data_as(I64P))
            assert rc == ST_INVALID_ARG
        assert np.array_equal(sel.download(), ob.address_encrypt(5, w.sk, 8460, 8461))


# ---- 4. keys, address, integer, words -----------------------------------------------------------------------------------------------------
def test_keys_address_integer_and_words_equal_the_oracle(w13):
    w, pkg, o = w13, w13.pkg, w13.o
    bank = w.new_bank(2)
    dsk = pkg.GLWESecret(bank, w.sk)
    # a member between its two halves under the world's keys ...
    oram = w.new_oram(0)
    oaddr = o.address_new(w.addr_g[0])
    assert np.array_equal(bank.read_prepare_write([w.addrs[0]], w.keys, first=0)[0], oram.read_prepare_write(oaddr, w.okeys))
    # ... then new keys, made on the device: the oracle's from the same draws
    keys = pkg.EvaluationKeysPrepared.encrypt_sk(bank, dsk, o.source(8501), o.source(8502), keep_std=True)
    evk2 = o.evk_gen(w.sk, 8501, 8502)
    assert list(keys.gal_els) == list(evk2["gal_els"])
    for i in range(12):
        assert np.array_equal(keys.atk_glwe[i], evk2["atk_glwe"][i].ravel()), i
    assert np.array_equal(keys.tsk_ggsw_inv, evk2["tsk"].ravel()) and np.array_equal(keys.atk_ggsw_inv, evk2["atk_ggsw_inv"].ravel())
    # what the member kept for its write is void: the write under the new keys gives the oracle's rows
    vals, cts = w.words(1, seed=85)
    bank.write(cts, [w.addrs[0]], keys, first=0)
    oram.write(cts[0], oaddr, o.keys_prepare(evk2))
    assert np.array_equal(bank.store_encrypted(0), oram.store()) and not bank.state(0)
    # device-only keys are accepted by the bank they were made on
    keys_dev = pkg.EvaluationKeysPrepared.encrypt_sk(bank, dsk, o.source(8501), o.source(8502))
    assert keys_dev.atk_glwe is None
    assert np.array_equal(bank.read([w.addrs[0]], keys_dev, first=0)[0], oram.read(oaddr, o.keys_prepare(evk2)))
    # an address
    for value in (0, 4097, (1 << 13) - 1):
        addr = pkg.Address.encrypt_sk(bank, value, dsk, o.source(8510), o.source(8511))
        assert np.array_equal(bank.address_digits(addr), o.address_encrypt(value, w.sk, 8510, 8511)), value
    with pytest.raises(pkg.FheRamError, match=r"base2d.max\(\) > value"):
        pkg.Address.encrypt_sk(bank, 1 << 13, dsk, o.source(1), o.source(2))
    # an encrypted integer: an integer stays on the bank's device, so it is compared through the address derived from it
    fu = pkg.FheUintPrepared.encrypt_sk(bank, VALUE, dsk, o.source(8520), o.source(8521), n_bits=N_BITS)
    derived = bank.derive_addresses([fu])[0]
    bank.sync()
    assert np.array_equal(bank.address_digits(derived), o.address_from_fheuint(o.fheuint_encrypt(VALUE, N_BITS, w.sk, 8520, 8521), sign=False))
    # words, and the decryption of downloaded ciphertexts
    bytes_ = [0, 5, 200, 255]
    words = bank.encrypt_word(dsk, bytes_, o.source(8530), o.source(8531))
    assert np.array_equal(words[0], o.glwe_encrypt_coeff0(bytes_[0], w.sk, 8530, 8531))
    wants = [o.expected_plain(v, o.p.k_glwe_pt, True) for v in bytes_]
    for (v, noise), want, ct in zip(bank.decrypt_coeff(dsk, words, wants), wants, words):
        ov, onoise = o.glwe_decrypt(ct, want, w.sk)
        assert v == want == ov and noise == pytest.approx(onoise, abs=NOISE_ABS)
    assert np.array_equal(bank.glwe_decrypt(dsk, words[1])[0], o.glwe_phase(words[1], w.sk))


# ---- 5. source_decrypt --------------------------------------------------------------------------------------------------------------------
def test_source_decrypt_equals_the_oracle_and_changes_nothing(w13, shared):
    w, pkg, o, (bank, dsk) = w13, w13.pkg, w13.o, shared
    S = pkg.Src
    ob5, ob3, ob7 = w.small(5)[0], w.small(3)[0], w.small(7)[0]
    rng = np.random.default_rng(86)
    rf5, rf3, tab = bank.regfile(5), bank.regfile(3), bank.table(7)
    for obj, ob, b in ((rf5, ob5, 5), (rf3, ob3, 3), (tab, ob7, 7)):
        obj.encrypt_sk(rng.integers(0, 256, size=(1 << b) * w.ws, dtype=np.uint8), dsk, ob.source(8600 + b), ob.source(8650 + b))
    s5, s3, s7 = bank.selector(5), bank.selector(3), bank.table_selector(7)
    s5.encrypt_sk(19, dsk, ob5.source(8601), ob5.source(8602))
    s3.encrypt_sk(6, dsk, ob3.source(8603), ob3.source(8604))
    s7.encrypt_sk(100, dsk, ob7.source(8605), ob7.source(8606))
    # before its operation has run, a source kind is refused
    fresh = w.new_bank(2)
    fsk = pkg.GLWESecret(fresh, w.sk)
    for src, code in ((S.list(0), ST_STATE), (S.select(0), ST_STATE), (S.regs(0), ST_STATE), (S.regs_old(), ST_STATE), (S.table(0), ST_STATE),
                      (S.member(0), ST_STATE), (S.host(0), ST_INVALID_ARG), (S.zero(), ST_INVALID_ARG), (S.member(2), ST_INVALID_ARG)):
        with pytest.raises(pkg.FheRamError) as e:
            fresh.decrypt_sources(fsk, [src])
        assert e.value.code == code, (src.kind, e.value.code, e.value.msg)
    # one of every kind
    bank.read_list([1, 0], [w.addrs[1], w.addrs[2]], w.keys, download=False)
    bank.read([w.addrs[0]], w.keys, first=0, download=False)
    bank.select([s3], [[S.member(0), S.list(0), S.zero(), S.list(1), S.member(1), S.zero(), S.list(0)]], download=False)   # index 6: list entry 0
    rf5.read([s5], download=False)
    rf3.read_prepare_write(s3, download=False)
    bank.table_read([tab], [s7], download=False)
    srcs = [S.member(0), S.list(1), S.select(0), S.regs(0), S.regs_old(), S.table(0)]

    def device_state():
        return [sha(bank.result(0, 2)), sha(bank.list_result(0, 2)), sha(bank.select_result(0, 1)), sha(rf5.result(0, 1)), sha(rf3.old_result()),
                sha(bank.table_result(0, 1)), sha(bank.store_encrypted(0)), sha(bank.store_encrypted(1)), sha(rf5.store()), sha(rf3.store()),
                sha(tab.download()), bank.state(0), bank.state(1), rf5.state(), rf3.state()]
    before = device_state()
    cts = [bank.result(0, 1)[0], bank.list_result(1, 1)[0], bank.select_result(0, 1)[0], rf5.result(0, 1)[0], rf3.old_result(), bank.table_result(0, 1)[0]]
    # with wants: the plaintext model's where it is at hand (the member's and the list's words), else the oracle's decoded value
    wants = np.array([[o.glwe_decrypt(ct[i], 0, w.sk)[0] for i in range(w.ws)] for ct in cts], dtype=np.int64)
    assert list(wants[0]) == [o.expected_plain(int(w.data[0][i + w.ws * w.idx[0]]), o.p.k_glwe_pt) for i in range(w.ws)]
    assert list(wants[1]) == [o.expected_plain(int(w.data[0][i + w.ws * w.idx[2]]), o.p.k_glwe_pt) for i in range(w.ws)]
    assert list(wants[2]) == list(wants[1] * 0 + [o.expected_plain(int(w.data[1][i + w.ws * w.idx[1]]), o.p.k_glwe_pt) for i in range(w.ws)])
    wants[3, 0] += 1   # a wrong expectation: the value is still the decoded one, the noise is the oracle's for that want
    for given in (wants, None):
        values, noise = bank.decrypt_sources(dsk, srcs, wants=given)
        assert values.shape == noise.shape == (6, w.ws) and values.dtype == np.int64
        for k, ct in enumerate(cts):
            for i in range(w.ws):
                want = int(values[k, i]) if given is None else int(given[k, i])
                ov, onoise = o.glwe_decrypt(ct[i], want, w.sk)
                assert int(values[k, i]) == ov, (k, i)
                assert noise[k, i] == pytest.approx(onoise, abs=NOISE_ABS), (k, i, noise[k, i], onoise)
    assert device_state() == before, "decrypt_sources changed something on the device"
    with pytest.raises(pkg.FheRamError) as e:   # a secret of another bank
        bank.decrypt_sources(fsk, srcs)
    assert e.value.code == ST_INVALID_ARG
    with pytest.raises(pkg.FheRamError) as e:   # n * word_size <= 64
        bank.decrypt_sources(dsk, [S.member(0)] * 33)
    assert e.value.code == ST_INVALID_ARG
    assert device_state() == before


# ---- 6. whole-object decrypt --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [None, {"safe": 1, "monitor": 2}])
def test_member_decrypt_equals_the_host_decode(w13, config):
    w, pkg, o = w13, w13.pkg, w13.o
    bank = w.new_bank(2, config=config)
    dsk = pkg.GLWESecret(bank, w.sk)
    want, want_worst = host_rows_decode(o, w.sk, w.rows[1], w.max_addr)
    check_decode_helper(o, w.sk, w.rows[1][1, 1], [0, 1, 4095])
    values, worst = bank.decrypt(1, dsk)
    assert values.shape == (w.max_addr, w.ws) and np.array_equal(values, want)
    assert worst == pytest.approx(want_worst, abs=NOISE_ABS) and worst < -(o.p.k_glwe_pt + 1)
    assert np.array_equal(values, np.array([o.expected_plain(int(x), o.p.k_glwe_pt) for x in w.data[1]]).reshape(-1, w.ws))
    assert sha(bank.store_encrypted(1)) == sha(w.rows[1]) and not bank.state(1)
    assert bank.roundoff_max() < 0.375
    bank.read_prepare_write([w.addrs[0]], w.keys, first=1)
    rotated = sha(bank.store_encrypted(1))
    with pytest.raises(pkg.FheRamError) as e:
        bank.decrypt(1, dsk)
    assert e.value.code == ST_STATE and sha(bank.store_encrypted(1)) == rotated and bank.state(1)
    assert np.array_equal(bank.decrypt(0, dsk)[0], host_rows_decode(o, w.sk, w.rows[0], w.max_addr)[0])   # member 0 is not between halves


# ---- 7. end to end: the oracle is the sampler and nothing else ----------------------------------------------------------------------------
def test_end_to_end_on_the_device(po):
    from _pkg import load_package
    pkg = load_package()
    S, D = pkg.Src, pkg.Derive
    max_addr, ws = 1 << 13, 2
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=ws))
    k_pt = o.p.k_glwe_pt
    plain = lambda data: np.array([o.expected_plain(int(x), k_pt) for x in data]).reshape(-1, ws)
    src = lambda i: o.source(8800 + i)
    sk = o.secret_gen(88)
    bank = pkg.RamBank(pkg.Parameters(max_addr=max_addr, word_size=ws), 2)
    dsk = pkg.GLWESecret(bank, sk)
    keys = pkg.EvaluationKeysPrepared.encrypt_sk(bank, dsk, src(1), src(2))
    rng = np.random.default_rng(88)
    data = [rng.integers(0, 256, size=max_addr * ws, dtype=np.uint8) for _ in range(2)]
    for m in range(2):
        bank.encrypt_sk(m, data[m], dsk, src(3 + 2 * m), src(4 + 2 * m))
    rdata, tdata = rng.integers(0, 256, size=32 * ws, dtype=np.uint8), rng.integers(0, 256, size=128 * ws, dtype=np.uint8)
    rf, tab = bank.regfile(5), bank.table(7)
    rf.encrypt_sk(rdata, dsk, src(7), src(8))
    tab.encrypt_sk(tdata, dsk, src(9), src(10))
    mem, regs, table = [plain(d) for d in data], plain(rdata), plain(tdata)
    value = 0xB5E3A6D9
    fu = pkg.FheUintPrepared.encrypt_sk(bank, value, dsk, src(11), src(12), n_bits=32)
    field = lambda first, bits: (value >> first) & ((1 << bits) - 1)
    i0, i1, i7, i5, i1b = field(0, 13), field(13, 13), field(3, 7), field(8, 5), field(20, 1)
    a0, a1 = pkg.Address.alloc(bank), pkg.Address.alloc(bank)
    s7, s5, s1 = bank.table_selector(7), bank.selector(5), bank.selector(1)
    bank.derive_list([D.address(fu, a0, 0), D.address(fu, a1, 13), D.selector(fu, s7, 3), D.selector(fu, s5, 8), D.selector(fu, s1, 20)])
    bank.table_read([tab], [s7], download=False, keys=keys)
    rf.read([s5], download=False)
    bank.read_list([0, 1], [a0, a1], keys, download=False)
    want_list = np.stack([mem[0][i0], mem[1][i1]])
    bank.read_prepare_write_list([1, 0], [a0, a1], keys, download=False)
    want_old = np.stack([mem[0][i1], mem[1][i0]])                   # member results, by member
    bank.select([s1], [[S.table(0), S.regs(0)]], download=False)
    picked = (regs[i5] if i1b else table[i7]).copy()
    # (the members' results are decrypted before the write, which starts from the buffers they sit in)
    srcs = [S.table(0), S.regs(0), S.list(0), S.list(1), S.member(0), S.member(1), S.select(0)]
    wants = np.stack([table[i7], regs[i5], want_list[0], want_list[1], want_old[0], want_old[1], picked])
    values, noise = bank.decrypt_sources(dsk, srcs, wants=wants)
    bank.write_list_selected([1, 0], [0, 0], [a0, a1], keys)
    mem[1][i0], mem[0][i1] = picked, picked
    rf.read_prepare_write(s5, download=False)
    old_value, old_noise = bank.decrypt_sources(dsk, [S.regs_old()], wants=regs[i5][None])
    rf.write(s5, S.select(0))
    values, noise, wants = np.concatenate([values, old_value]), np.concatenate([noise, old_noise]), np.concatenate([wants, regs[i5][None]])
    regs[i5] = picked
    assert np.array_equal(values, wants), (values, wants)
    print("end to end, log2 noise of the decrypted sources:", np.array2string(noise, precision=2))
    assert np.all(noise < -(k_pt + 1)), noise                      # the reference example's own bound (examples/fhe-ram.rs)
    got_regs, worst_regs = rf.decrypt(dsk)
    assert np.array_equal(got_regs, regs)
    for m in range(2):
        got, worst = bank.decrypt(m, dsk)
        assert np.array_equal(got, mem[m]), m
        print(f"end to end, member {m}: worst log2 noise against the decoded values {worst:.2f}; register file {worst_regs:.2f}")
        assert worst < -(k_pt + 1) and worst_regs < -(k_pt + 1)
    assert bank.roundoff_max() < 0.375


def test_null_secret_and_null_objects_are_refused(w13, shared):
    """every call on a null secret or a null object is FHERAM_ERR_INVALID_ARG before a draw is read (the null bank: tests/test_bank_setup_abi.py)"""
    bank, dsk = shared
    L = lib()
    z = np.zeros(8, dtype=np.int64)
    zp = z.ctypes.data_as(I64P)
    b8 = c_data(np.zeros(8, dtype=np.uint8))
    i32 = np.zeros(8, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    src = (w13.pkg.api._CSelectSrc * 1)(w13.pkg.api._CSelectSrc(2, 0))
    out, d = C.c_void_p(), C.c_double()
    rf, tab, sel = bank.regfile(1), bank.table(1), bank.selector(1)
    for what, rc in (("secret_create", L.fheram_bank_secret_create(bank._h, None, C.byref(out))),
                     ("keys", L.fheram_bank_keys_encrypt_sk(bank._h, None, zp, zp, None)),
                     ("address", L.fheram_bank_address_encrypt_sk(bank._h, None, 0, zp, zp, C.byref(out))),
                     ("fheuint", L.fheram_bank_fheuint_encrypt_sk(bank._h, None, 0, 8, zp, zp, C.byref(out))),
                     ("glwe_encrypt", L.fheram_bank_glwe_encrypt_sk(bank._h, None, 1, 3, 51, None, 0, 0, zp, zp, zp)),
                     ("glwe_decrypt", L.fheram_bank_glwe_decrypt(bank._h, None, 1, 3, zp, zp)),
                     ("ram_encrypt", L.fheram_bank_ram_encrypt_sk(bank._h, 0, None, b8, 8, zp, zp)),
                     ("regs_encrypt sk", L.fheram_bank_regs_encrypt_sk(bank._h, rf._h, None, b8, 8, zp, zp)),
                     ("regs_encrypt regs", L.fheram_bank_regs_encrypt_sk(bank._h, None, dsk._h, b8, 8, zp, zp)),
                     ("table_encrypt sk", L.fheram_bank_table_encrypt_sk(bank._h, tab._h, None, b8, 8, zp, zp)),
                     ("table_encrypt table", L.fheram_bank_table_encrypt_sk(bank._h, None, dsk._h, b8, 8, zp, zp)),
                     ("selector sk", L.fheram_bank_selector_encrypt_sk(bank._h, None, sel._h, 0, zp, zp)),
                     ("source_decrypt sk", L.fheram_bank_source_decrypt(bank._h, None, src, 1, None, zp, None)),
                     ("source_decrypt srcs", L.fheram_bank_source_decrypt(bank._h, dsk._h, None, 1, None, zp, None)),
                     ("ram_decrypt", L.fheram_bank_ram_decrypt(bank._h, 0, None, i32, C.byref(d))),
                     ("regs_decrypt sk", L.fheram_bank_regs_decrypt(bank._h, rf._h, None, i32, C.byref(d))),
                     ("regs_decrypt regs", L.fheram_bank_regs_decrypt(bank._h, None, dsk._h, i32, C.byref(d))),
                     ("table_decrypt sk", L.fheram_bank_table_decrypt(bank._h, tab._h, None, i32, C.byref(d))),
                     ("table_decrypt table", L.fheram_bank_table_decrypt(bank._h, None, dsk._h, i32, C.byref(d)))):
        assert rc == ST_INVALID_ARG, (what, rc)
    assert not out.value


# ---- 8. lifetimes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank_first", [True, False])
def test_bank_and_secret_destroyed_in_either_order(w13, bank_first):
    w, pkg = w13, w13.pkg
    L = lib()
    bank = w.new_bank(1, load=False)
    out = C.c_void_p()
    assert L.fheram_bank_secret_create(bank._h, w.sk.ctypes.data_as(I64P), C.byref(out)) == 0 and out.value
    h, bank._h = bank._h, None
    if bank_first:
        L.fheram_bank_destroy(h)
        L.fheram_secret_destroy(out.value)
    else:
        L.fheram_secret_destroy(out.value)
        L.fheram_bank_destroy(h)
    again = w.new_bank(1, load=False)   # the device is still usable
    assert pkg.GLWESecret(again, w.sk)._h

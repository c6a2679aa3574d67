"""Precisions inside the limb counts.  fheram_ctx_create_cfg accepts any precision whose limb count the kernels are built for — k_glwe_ct
35..51, k_ggsw_addr 52..68, k_evk_trace 52..68 or 69..85, k_evk_ggsw_inv 69..85 — and any k_glwe_pt in [1, k_glwe_ct] (the encoders take
1..25, the decoder up to 30).  Every other file creates its contexts at multiples of 17 and k_glwe_pt 3 or 9; here the blocks below run one
world each at max_addr = 2^13, word_size 1:
  - the device's encryption of the keys, the member and an address equals the oracle's from the same seeded draws (noise_limb(k) placement
    with a scaled draw, the two-limb encodings of k_glwe_pt 18..25);
  - read, read_prepare_write + write and the read back equal the oracle's, the words decrypt, and the noise stays below the project's bound
    -(k_glwe_pt + 1).  The oracle alone gives, log2, read / read after write: defaults -47.1 / -34.1; k_pt 9 + k_evk_trace 85 -40.9 / -33.2;
    k_ct 40 -37.2 / -31.7; k_ct 35 + k_pt 1 -32.2 / -32.7; k_ct 50 + k_pt 9 -41.5 / -33.5; k_pt 17 -43.0 / -36.9; k_pt 18 -42.1 / -34.5;
    k_pt 25 -42.3 / -33.3; k_addr 52 -26.3 / -28.1; k_addr 60 + k_evk 69 / 69 -37.7 / -16.3; k_evk_trace 52 -27.5 / -25.7 — which is why no
    block combines a reduced key precision with k_pt >= 15;
  - the bank's decrypt and decrypt_sources equal Oracle.glwe_decrypt and a plain-Python big-integer model of decode_coeff_i64 and the
    example's rounding (model() below), the k % 17 != 0 branch of k_decrypt_decode included;
  - load_plain equals the zero-randomness encrypt_sk for every byte value.
The decoder's edges (ties of both signs, 0, +-1, the ends of the digit range) are fed as rows that are no ciphertexts: a zero mask and
chosen body digits.  Every comparison is exact (np.array_equal on int64, or equality of Python integers); a noise figure is compared to the
NOISE_ABS of tests/test_gpu_bank_setup.py (both sides take log2 of the same exact integer)."""
import math

import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import World, sha
from test_gpu_bank_setup import NOISE_ABS
from test_gpu_public_io import _Zeros

pytestmark = pytest.mark.gpu

ST_UNSUPPORTED = 5
N = 4096
LO, HI = -(1 << 16), (1 << 16) - 1
BLOCKS = [
    {},
    {"k_glwe_pt": 9, "k_evk_trace": 85},
    {"k_glwe_ct": 40},
    {"k_glwe_ct": 35, "k_glwe_pt": 1},
    {"k_glwe_ct": 50, "k_glwe_pt": 9},
    {"k_glwe_pt": 17},
    {"k_glwe_pt": 18},
    {"k_glwe_pt": 25},
    {"k_ggsw_addr": 52},
    {"k_ggsw_addr": 60, "k_evk_trace": 69, "k_evk_ggsw_inv": 69},
    {"k_evk_trace": 52},
]


def block_id(crypto):
    return "-".join(f"{k[2:]}{v}" for k, v in crypto.items()) or "defaults"


@pytest.fixture(scope="module", params=BLOCKS, ids=block_id)
def pw(po, request):
    return World(po, 1 << 13, 1, word_size=1, n_addr=2, **request.param)


# ---- the big-integer model ------------------------------------------------------------------------------------------------------------------------
def model(d0, d1, d2, k, k_pt):
    """(res, value) of the phase digits d0, d1, d2 (most significant first), Python integers: decode_coeff_i64(k) and the example's rounding,
    half away from zero (examples/fhe-ram.rs:224-237)"""
    x = (int(d0) << 34) + (int(d1) << 17) + int(d2)
    res = x >> (51 - k)   # (floor)
    ls = k - k_pt
    mag = (abs(res) + (1 << (ls - 1))) >> ls if ls > 0 else abs(res)
    return res, (-mag if res < 0 else mag)


def model_noise(res, want, k, k_pt):
    d = abs(res - (want << (k - k_pt)))
    return math.log2(d) - k if d else float("-inf")


def model_rows(o, sk, rows, max_addr):
    """rows [1][rows][GLWE] of a word_size-1 RAM -> (values [max_addr], the worst log2 noise against each coefficient's own value)"""
    k, k_pt = o.p.k_glwe_ct, o.p.k_glwe_pt
    values, top = [], 0
    for r in range(rows.shape[1]):
        pt = np.asarray(o.glwe_phase(rows[0, r], sk)).reshape(3, N)
        for i in range(min(N, max_addr - r * N)):
            res, val = model(pt[0, i], pt[1, i], pt[2, i], k, k_pt)
            values.append(val)
            top = max(top, abs(res - (val << (k - k_pt))))
    return np.array(values, dtype=np.int64), (math.log2(top) - k if top else float("-inf"))


def same_noise(got, want):
    return got == want if math.isinf(want) else got == pytest.approx(want, abs=NOISE_ABS)


def every_byte(count, seed):
    data = np.concatenate([np.arange(256), np.random.default_rng(seed).integers(0, 256, size=count - 256)]).astype(np.uint8)
    assert set(data[:256].tolist()) == set(range(256))
    return data


# ---- 1. one world per block -------------------------------------------------------------------------------------------------------------------------
def test_device_encryption_equals_the_oracle(pw):
    """the world's keys, member and first address were made by the oracle from seeds: the device makes the same from the same draws"""
    w, pkg, o = pw, pw.pkg, pw.o
    bank = w.new_bank(1, load=False)
    dsk = pkg.GLWESecret(bank, w.sk)
    keys = pkg.EvaluationKeysPrepared.encrypt_sk(bank, dsk, o.source(1901), o.source(1902), keep_std=True)
    assert keys.atk_glwe[0].size == o.p.atk_trace_len
    for i in range(12):
        assert np.array_equal(keys.atk_glwe[i], w.evk["atk_glwe"][i].ravel()), i
    assert np.array_equal(keys.tsk_ggsw_inv, w.evk["tsk"].ravel()) and np.array_equal(keys.atk_ggsw_inv, w.evk["atk_ggsw_inv"].ravel())
    bank.encrypt_sk(0, w.data[0], dsk, o.source(1904), o.source(1905))
    got = bank.store_encrypted(0)
    assert np.array_equal(got, w.rows[0]), np.count_nonzero(got != w.rows[0])
    addr = pkg.Address.encrypt_sk(bank, w.idx[0], dsk, o.source(2000), o.source(2001))
    assert np.array_equal(bank.address_digits(addr), w.addr_g[0])
    word = bank.encrypt_word(dsk, [200], o.source(3100), o.source(3500))
    assert np.array_equal(word[0], o.glwe_encrypt_coeff0(200, w.sk, 3100, 3500))


def test_read_write_cycle_equals_the_oracle_and_decrypts(pw):
    w, o = pw, pw.o
    bank, oram = w.new_bank(1), w.new_oram(0)
    a, oa = w.addrs, [o.address_new(g) for g in w.addr_g]
    got = bank.read([a[0]], w.keys)[0]
    assert np.array_equal(got, oram.read(oa[0], w.okeys)), np.count_nonzero(got != oram.read(oa[0], w.okeys))
    w.check_word(got, w.data[0], 0)   # the value, and noise < -(k_pt + 1)
    got = bank.read_prepare_write([a[1]], w.keys)[0]
    assert np.array_equal(got, oram.read_prepare_write(oa[1], w.okeys))
    w.check_word(got, w.data[0], 1)
    word = np.stack([o.glwe_encrypt_coeff0(200, w.sk, 3100, 3500)])[None]
    bank.write(word, [a[1]], w.keys)
    oram.write(word[0], oa[1], w.okeys)
    assert np.array_equal(bank.store_encrypted(0), oram.store()) and not bank.state(0)
    back = bank.read([a[1]], w.keys)[0]
    assert np.array_equal(back, oram.read(oa[1], w.okeys))
    data2 = w.data[0].copy()
    data2[w.idx[1]] = 200
    w.check_word(back, data2, 1, written=True)
    _, n_read = o.glwe_decrypt(bank.read([a[0]], w.keys)[0][0], o.expected_plain(int(data2[w.idx[0]]), o.p.k_glwe_pt, w.idx[0] == w.idx[1]), w.sk)
    _, n_back = o.glwe_decrypt(back[0], o.expected_plain(200, o.p.k_glwe_pt, True), w.sk)
    print(f"precisions {block_id(w.crypto)}: log2 noise of a read after the write {n_read:.1f}, of the written word read back {n_back:.1f}; bound {-(o.p.k_glwe_pt + 1)}")
    assert bank.roundoff_max() < 0.375


def test_decrypt_equals_the_oracle_and_the_model(pw):
    w, pkg, o = pw, pw.pkg, pw.o
    k, k_pt = o.p.k_glwe_ct, o.p.k_glwe_pt
    bank = w.new_bank(1)
    dsk = pkg.GLWESecret(bank, w.sk)
    values, worst = bank.decrypt(0, dsk)
    want, want_worst = model_rows(o, w.sk, w.rows[0], w.max_addr)
    assert values.shape == (w.max_addr, 1) and np.array_equal(values[:, 0], want)
    assert same_noise(worst, want_worst), (worst, want_worst)
    assert np.array_equal(want, [o.expected_plain(int(x), k_pt) for x in w.data[0]])
    for addr in (0, 1, N - 1, N, w.max_addr - 1):   # Oracle.glwe_decrypt at single coefficients, value and noise
        pt = np.asarray(o.glwe_phase(w.rows[0][0, addr // N], w.sk)).reshape(3, N)[:, addr % N]
        res, val = model(pt[0], pt[1], pt[2], k, k_pt)
        ov, onoise = o.glwe_decrypt(w.rows[0][0, addr // N], val, w.sk, addr % N)
        assert ov == val == int(values[addr, 0]) and same_noise(onoise, model_noise(res, val, k, k_pt)), (addr, ov, val, onoise)
    # a member result, through decrypt_sources: with the decoded value as the expectation, and with a wrong one
    ct = bank.read([w.addrs[0]], w.keys)[0]
    pt = np.asarray(o.glwe_phase(ct[0], w.sk)).reshape(3, N)[:, 0]
    res, val = model(pt[0], pt[1], pt[2], k, k_pt)
    assert val == o.expected_plain(int(w.data[0][w.idx[0]]), k_pt)
    for want_v in (val, val + 1):
        got_v, got_n = bank.decrypt_sources(dsk, [pkg.Src.member(0)], wants=np.array([[want_v]]))
        ov, onoise = o.glwe_decrypt(ct[0], want_v, w.sk)
        assert int(got_v[0, 0]) == ov == val
        assert same_noise(float(got_n[0, 0]), model_noise(res, want_v, k, k_pt)) and same_noise(onoise, model_noise(res, want_v, k, k_pt)), (want_v, got_n, onoise)
    assert sha(bank.store_encrypted(0)) == sha(w.rows[0])


def test_load_plain_is_the_trivial_encryption_of_every_byte(pw):
    w, pkg, o = pw, pw.pkg, pw.o
    bank = pkg.RamBank(w.params, 2)
    dsk = pkg.GLWESecret(bank, w.sk)
    data = every_byte(w.max_addr, 4100)
    bank.load_plain(0, data)
    bank.encrypt_sk(1, data, dsk, _Zeros(), _Zeros())
    got, want = bank.store_encrypted(0), bank.store_encrypted(1)
    assert np.array_equal(got, want), np.count_nonzero(got != want)
    assert not np.any(got.reshape(1, 2, 3, 2, N)[:, :, :, 1, :]), "a mask limb is not zero"
    values, worst = bank.decrypt(0, dsk)
    assert np.array_equal(values[:, 0], [o.expected_plain(int(x), o.p.k_glwe_pt) for x in data])
    want_v, want_worst = model_rows(o, w.sk, got, w.max_addr)
    assert np.array_equal(values[:, 0], want_v) and same_noise(worst, want_worst), (worst, want_worst)
    for a in (0, 127, 128, 255):
        plain = o.expected_plain(int(data[a]), o.p.k_glwe_pt)
        v, noise = o.glwe_decrypt(got[0][0], plain, w.sk, a)
        assert v == plain and noise < -o.p.k_glwe_ct, (a, v, plain, noise)


# ---- 2. the decoder's edges -------------------------------------------------------------------------------------------------------------------------
def digits_of(x):
    """the balanced base-2^17 digits (d0, d1, d2) of x, or None where d0 leaves the normalised range"""
    out = []
    for _ in range(2):
        d = ((x + (1 << 16)) % (1 << 17)) - (1 << 16)
        out.append(d)
        x = (x - d) >> 17
    return (x, out[1], out[0]) if LO <= x <= HI else None


def edge_digits(k, k_pt):
    """phase digits whose res is a tie of both signs, next to a tie, 0, +-1, and the ends of the digit range"""
    ls, sh = k - k_pt, 51 - k
    half = 1 << (ls - 1)
    targets = [0, 1, -1]
    for t in (0, 1, 2, 5, 1000):
        for r in (t * (1 << ls) + half, t * (1 << ls) + half - 1, t * (1 << ls) + half + 1):
            targets += [r, -r]
    cases = [(HI, HI, HI), (LO, LO, LO), (HI, LO, HI), (LO, HI, LO)]
    for res in targets:
        for low in sorted({0, (1 << sh) - 1, (1 << sh) // 3}):   # the bits the floor drops (k = 51: none)
            d = digits_of((res << sh) + low)
            if d is not None:
                assert model(*d, k, k_pt)[0] == res
                cases.append(d)
    return cases


@pytest.mark.parametrize("k", [51, 40])
@pytest.mark.parametrize("k_pt", [1, 3, 9, 25])
def test_decoder_edges_equal_the_model(po, k, k_pt):
    """rows with a zero mask and chosen body digits (no ciphertexts: nothing is encrypted, everything compares): the phase digits are the body
    digits themselves, one case per coefficient"""
    pkg = load_package()
    crypto = {"k_glwe_ct": k, "k_glwe_pt": k_pt}
    o = po.Oracle(po.OParams(max_addr=N, word_size=1, **crypto))
    sk = o.secret_gen(77)
    bank = pkg.RamBank(pkg.Parameters(max_addr=N, word_size=1, **crypto), 1)
    dsk = pkg.GLWESecret(bank, sk)
    cases = edge_digits(k, k_pt)
    ls = k - k_pt
    ties = [d for d in cases if abs(model(*d, k, k_pt)[0]) % (1 << ls) == 1 << (ls - 1)]
    assert any(model(*d, k, k_pt)[0] > 0 for d in ties) and any(model(*d, k, k_pt)[0] < 0 for d in ties) and len(cases) < N
    row = np.zeros((3, 2, N), dtype=np.int64)
    for i, d in enumerate(cases):
        row[:, 0, i] = d
    rows = row.reshape(1, 1, -1)
    bank.load_encrypted(0, rows)
    assert np.array_equal(np.asarray(o.glwe_phase(rows[0, 0], sk)).reshape(3, N), row[:, 0, :]), "the digits are not their own phase"
    values, worst = bank.decrypt(0, dsk)
    top = 0
    for i, d in enumerate(cases):
        res, val = model(*d, k, k_pt)
        assert -(1 << 31) <= val < (1 << 31)
        assert int(values[i, 0]) == val, (i, d, res, val, int(values[i, 0]))
        ov, onoise = o.glwe_decrypt(rows[0, 0], val, sk, i)
        assert ov == val and same_noise(onoise, model_noise(res, val, k, k_pt)), (i, d, ov, val)
        top = max(top, abs(res - (val << ls)))
    assert not np.any(values[len(cases):])
    assert top == 1 << (ls - 1), "a tie is the largest distance a decoded value can have"
    assert same_noise(worst, math.log2(top) - k), (worst, top)
    for d in ties:   # half rounds away from zero
        res, val = model(*d, k, k_pt)
        assert abs(val) == (abs(res) >> ls) + 1 and (val < 0) == (res < 0)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_ct", [34, 52])
def test_k_glwe_ct_outside_three_limbs_is_refused_at_creation(k_ct):
    pkg = load_package()
    with pytest.raises(pkg.FheRamError) as e:
        pkg.RamBank(pkg.Parameters(max_addr=N, word_size=1, k_glwe_ct=k_ct), 1)
    assert e.value.code == ST_UNSUPPORTED and "limb counts" in e.value.msg, e.value


def test_k_pt_26_is_refused_by_the_encoders_and_still_decrypts(po):
    pkg = load_package()
    crypto = {"k_glwe_pt": 26}
    o = po.Oracle(po.OParams(max_addr=N, word_size=1, **crypto))
    sk = o.secret_gen(78)
    bank = pkg.RamBank(pkg.Parameters(max_addr=N, word_size=1, **crypto), 1)
    dsk = pkg.GLWESecret(bank, sk)
    cases = edge_digits(51, 26)
    row = np.zeros((3, 2, N), dtype=np.int64)
    for i, d in enumerate(cases):
        row[:, 0, i] = d
    bank.load_encrypted(0, row.reshape(1, 1, -1))
    before = sha(bank.store_encrypted(0))
    data = every_byte(N, 4200)
    t = bank.table(7)
    for what, call in (("load_plain", lambda: bank.load_plain(0, data)), ("Table.load_plain", lambda: t.load_plain(data[:128])),
                       ("encrypt_sk", lambda: bank.encrypt_sk(0, data, dsk, o.source(1), o.source(2)))):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_UNSUPPORTED and "k_glwe_pt out of range" in e.value.msg, (what, e.value)
        assert sha(bank.store_encrypted(0)) == before and not bank.state(0), what
    values, worst = bank.decrypt(0, dsk)
    assert [int(v) for v in values[:len(cases), 0]] == [model(*d, 51, 26)[1] for d in cases]
    assert sha(bank.store_encrypted(0)) == before


def test_k_pt_31_is_refused_by_the_decoder(po):
    pkg = load_package()
    bank = pkg.RamBank(pkg.Parameters(max_addr=N, word_size=1, k_glwe_pt=31), 1)
    o = po.Oracle(po.OParams(max_addr=N, word_size=1))
    dsk = pkg.GLWESecret(bank, o.secret_gen(79))
    rows = np.zeros((1, 1, 3 * 2 * N), dtype=np.int64)
    bank.load_encrypted(0, rows)
    with pytest.raises(pkg.FheRamError) as e:
        bank.decrypt(0, dsk)
    assert e.value.code == ST_UNSUPPORTED and "k_glwe_pt above 30" in e.value.msg, e.value
    assert not np.any(bank.store_encrypted(0)) and not bank.state(0)

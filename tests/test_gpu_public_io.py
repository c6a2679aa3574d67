"""The public side of a bank (include/fheram.h "THE PUBLIC SIDE of a bank"): fheram_bank_ram_load_plain / _regs_load_plain,
fheram_bank_peek / _peek_result and fheram_bank_poke (RamBank.load_plain / peek / peek_result / poke, RegFile.load_plain, Src.peek).

The contract, in the oracle's own operations, with a public address a = r * N + q:
  load   the rows are Ram::encrypt_sk's with an all-zero mask and zero noise (the bank's own encrypt_sk fed zeros), and every coefficient
         decrypts under the oracle to the oracle's encoding with a difference of exactly 0
  peek   out[y] = glwe_trace(0, log N)(glwe_rotate(-q, row r of word ciphertext y))
  poke   R' = big_normalize(R - sum_j glwe_rotate(+q_j, t_j) + sum_j glwe_rotate(+q_j, w_j[y])) over the entries j of a touched row, t_j
         the peek of entry j
Every comparison is np.array_equal on int64.  Banks have 2 members at max_addr = 2^12 (one row), 2^13 (two rows) and 2^12 + 512 (a ragged
second row)."""
import ctypes as C

import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import World, lib, sha
from test_gpu_regs import regs_rows
from test_gpu_regs import selector as reg_selector
from test_gpu_select import SelWorld

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS, ST_RANGE, ST_DEVICE = 1, 2, 3, 4, 6, 7
N, LOGN = 4096, 12
LO, HI = -(1 << 16), (1 << 16) - 1   # the ends of the normalised range (tests/test_gpu_extremes.py)
I64P, U8P = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
RAGGED = (1 << 12) + 512


class _Zeros:
    """mask and noise sources that draw zeros: Ram::encrypt_sk then gives the trivial ciphertext"""

    def uniform_limbs(self, count):
        return np.zeros(count, dtype=np.int64)

    def gaussian(self, count, scale):
        return np.zeros(count, dtype=np.int64)


@pytest.fixture(scope="module")
def w12(po):
    return SelWorld(po, 1 << 12, 2, 2, seed=600)


@pytest.fixture(scope="module")
def w13(po):
    return SelWorld(po, 1 << 13, 2, 2, seed=610)


@pytest.fixture(scope="module")
def wrag(po):
    return World(po, RAGGED, 2, word_size=4, seed=620)


def world_of(request, log):
    return request.getfixturevalue({12: "w12", 13: "w13", "ragged": "wrag"}[log])


def keyed_bank(w, config=None):
    bank = w.new_bank(2, config=config)
    bank._use_keys(w.keys)
    return bank


def rows_of(w):
    """every member's rows as [ws][rows][GLWE], copies"""
    return [np.array(r, dtype=np.int64).reshape(w.ws, -1, w.params.glwe_len()).copy() for r in w.rows]


def digest(bank, w):
    M, two = w.M, w.params.rows() > 1
    return ([sha(bank.store_encrypted(m)) for m in range(M)], [bank.state(m) for m in range(M)], sha(bank.result(0, M)),
            [sha(bank.tree(m, 0)) for m in range(M)] if two else None)


_PEEKS = {}


def opeek(w, rows, m, a):
    """the contract of one peek entry on `rows`: [ws][GLWE]"""
    r, q = divmod(a, N)
    key = (id(w), sha(rows[m][:, r]), q)
    if key not in _PEEKS:
        _PEEKS[key] = np.stack([w.o.glwe_trace(w.okeys, 0, LOGN, w.o.glwe_rotate(-q, rows[m][y][r])) for y in range(w.ws)])
    return _PEEKS[key]


def opoke(w, rows, members, addrs, words):
    """the contract of a poke on `rows` (a list of [ws][rows][GLWE]): (the new rows, the old words [n][ws][GLWE])"""
    o = w.o
    t = [opeek(w, rows, m, a) for m, a in zip(members, addrs)]
    new = [r.copy() for r in rows]
    for m, r in sorted({(m, a // N) for m, a in zip(members, addrs)}):
        for y in range(w.ws):
            acc = rows[m][y][r].astype(np.int64).reshape(3, 2, N).copy()
            for j, (mj, aj) in enumerate(zip(members, addrs)):
                if (mj, aj // N) != (m, r):
                    continue
                acc -= o.glwe_rotate(aj % N, t[j][y]).reshape(3, 2, N)
                acc += o.glwe_rotate(aj % N, np.asarray(words[j][y], dtype=np.int64)).reshape(3, 2, N)
            new[m][y][r] = np.stack([o.big_normalize(np.ascontiguousarray(acc[:, col, :]), 3) for col in (0, 1)], axis=1).ravel()
    return new, np.stack(t)


def enc_addr(w, a, seed=0):
    g = w.o.address_encrypt(a, w.sk, 8800 + seed, 8900 + seed)
    return w.pkg.Address(w.params, list(g)), w.o.address_new(g)


def decrypts(w, cts, values, written, what=""):
    """cts [ws][GLWE] decrypt to the bytes `values` with noise below the example's bound; returns the largest log2 noise"""
    worst = -1e9
    for i in range(w.ws):
        want = w.o.expected_plain(int(values[i]), w.o.p.k_glwe_pt, written)
        v, noise = w.o.glwe_decrypt(cts[i], want, w.sk)
        assert v == want, (what, i, v, want, noise)
        worst = max(worst, noise)
    return worst


# ---- 1. plain loads ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [2, 4])
@pytest.mark.parametrize("max_addr", [1 << 12, 1 << 13, RAGGED], ids=["2p12", "2p13", "ragged"])
def test_load_plain_is_the_trivial_encryption(po, max_addr, ws):
    pkg = load_package()
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=ws))
    sk = o.secret_gen(6300 + ws)
    p = pkg.Parameters(max_addr=max_addr, word_size=ws)
    R, G = p.rows(), p.glwe_len()
    assert R == -(-max_addr // N)
    bank = pkg.RamBank(p, 2)
    bsk = pkg.GLWESecret(bank, sk)
    rng = np.random.default_rng(6400 + max_addr + ws)
    data = rng.integers(0, 256, size=max_addr * ws, dtype=np.uint8)
    bank.load_plain(0, data)
    assert not bank.state(0)
    rows = bank.store_encrypted(0)
    assert rows.shape == (ws, R, G)
    assert not np.any(rows.reshape(ws, R, 3, 2, N)[:, :, :, 1, :]), "a mask limb is not zero"
    bank.encrypt_sk(1, data, bsk, _Zeros(), _Zeros())
    want = bank.store_encrypted(1)
    assert np.array_equal(rows, want), np.count_nonzero(rows != want)
    # the oracle's encoding: its decryption of a data coefficient differs from its own encoding of the byte by exactly 0 (log2 of 0)
    for a in sorted({0, 1, N - 1, min(N, max_addr - 1), max_addr - 1}):
        for i in range(ws):
            plain = o.expected_plain(int(data[i + ws * a]), o.p.k_glwe_pt, False)
            v, noise = o.glwe_decrypt(rows[i][a // N], plain, sk, a % N)
            assert v == plain and noise < -o.p.k_glwe_ct, (a, i, v, plain, noise)
    if max_addr % N:   # the ragged last row's padding is the encoding of 0
        v, noise = o.glwe_decrypt(rows[0][R - 1], 0, sk, N - 1)
        assert v == 0 and noise < -o.p.k_glwe_ct
    vals, worst = bank.decrypt(0, bsk)
    assert np.array_equal(vals, np.array([o.expected_plain(int(x), o.p.k_glwe_pt, False) for x in data]).reshape(max_addr, ws))
    print(f"load_plain 2^{np.log2(max_addr):.2f} x {ws}: worst log2 noise of the bank's own decrypt {worst}")
    if R > 1:   # a row range: the last row alone; the other row's digest does not change
        first = sha(rows[:, 0])
        tail = rng.integers(0, 256, size=(max_addr - N) * ws, dtype=np.uint8)
        bank.load_plain(0, tail, first_row=1)
        again = bank.store_encrypted(0)
        assert sha(again[:, 0]) == first, "a row range load changed another row"
        bank.encrypt_sk(1, np.concatenate([data[:N * ws], tail]), bsk, _Zeros(), _Zeros())
        assert np.array_equal(again, bank.store_encrypted(1))
    # a second load straight behind the first (the staging buffer's one wait), then the first contents again
    bank.load_plain(0, data[::-1].copy())
    bank.load_plain(0, data)
    assert sha(bank.store_encrypted(0)) == sha(rows)
    # a 5-bit register file
    rf, twin = bank.regfile(5), bank.regfile(5)
    d5 = rng.integers(0, 256, size=32 * ws, dtype=np.uint8)
    rf.load_plain(d5)
    twin.encrypt_sk(d5, bsk, _Zeros(), _Zeros())
    assert not rf.state() and np.array_equal(rf.store(), twin.store())
    v5, _ = rf.decrypt(bsk)
    assert np.array_equal(v5, np.array([o.expected_plain(int(x), o.p.k_glwe_pt, False) for x in d5]).reshape(32, ws))


# ---- 2. peek ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [12, 13, "ragged"])
def test_peek_equals_rotate_and_trace(request, log):
    """addresses 0, N - 1, N (where the member has a second row), max_addr - 1 and a repeat, in two members, as ONE call (10 or 20
    ciphertexts: beyond the tail launch) and the first two alone (4 or 8: the tail launch)"""
    w = world_of(request, log)
    pkg, S = w.pkg, w.pkg.Src
    bank = keyed_bank(w)
    rows = rows_of(w)
    addrs = [0, N - 1, min(N, w.max_addr - 2), w.max_addr - 1, N - 1]
    members = [0, 1, 0, 1, 1]
    before = digest(bank, w)
    got = bank.peek(members, addrs)
    assert got.shape == (5, w.ws, w.params.glwe_len())
    for k, (m, a) in enumerate(zip(members, addrs)):
        want = opeek(w, rows, m, a)
        assert np.array_equal(got[k], want), (log, k, m, a, np.count_nonzero(got[k] != want))
        noise = decrypts(w, got[k], [w.data[m][i + w.ws * a] for i in range(w.ws)], False, (log, m, a))
        assert noise < -(w.o.p.k_glwe_pt + 1), noise
        print(f"peek {log} member {m} address {a}: log2 noise {noise:.2f}")
    assert digest(bank, w) == before, "a peek changed the bank"
    assert np.array_equal(bank.peek_result(0, 5), got) and np.array_equal(bank.peek_result(3, 1)[0], got[3])
    assert bank.peek(members[:2], addrs[:2], download=False) is None
    assert np.array_equal(bank.peek_result(0, 2), got[:2])
    assert digest(bank, w) == before
    if log == "ragged":
        return
    # the outputs as a select's candidates, against the same select on HOST copies of them
    bank.peek(members, addrs, download=False)
    sel = w.selector(bank, 1, 1)
    via_kind = bank.select([sel], [[S.peek(0), S.peek(3)]])
    via_host = bank.select([sel], [[S.host(0), S.host(1)]], host_words=np.stack([got[0], got[3]]))
    assert np.array_equal(via_kind, via_host)
    L = pkg.Lane
    via_lane = bank.select_lanes([sel], [[[L.peek(2, 1), L.peek(2, 0)], [L.peek(4, 0), L.peek(4, 1)]]])
    host_lane = bank.select([sel], [[S.host(0), S.host(1)]], host_words=np.stack([got[2][::-1], got[4]]))
    assert np.array_equal(via_lane, host_lane)
    vals, _ = bank.decrypt_sources(pkg.GLWESecret(bank, w.sk), [S.peek(1)])
    assert [int(v) for v in vals[0]] == [w.o.expected_plain(int(w.data[1][i + w.ws * (N - 1)]), w.o.p.k_glwe_pt, False) for i in range(w.ws)]
    assert digest(bank, w) == before


# ---- 3. poke ----------------------------------------------------------------------------------------------------------------------------------------
POKES = {
    "one": (12, [0], [100]),
    "two_in_one_row_its_ends": (12, [0, 0], [0, N - 1]),
    "two_members_two_rows": (13, [0, 0, 1, 1], [5, N + 7, N - 1, N]),
}


def check_poke(w, bank, rows, members, addrs, words, srcs=None, host_words=None):
    """pokes, compares rows and old words with the contract, returns the contract's rows"""
    want, old = opoke(w, rows, members, addrs, words)
    if srcs is None:
        bank.poke(members, addrs, words=words)
    else:
        bank.poke(members, addrs, words=host_words, srcs=srcs)
    for m in range(w.M):
        got = bank.store_encrypted(m)
        assert np.array_equal(got, want[m]), (m, np.count_nonzero(got != want[m]))
        assert not bank.state(m)
    assert np.array_equal(bank.peek_result(0, len(members)), old), "the old words are not the last peek"
    return want


@pytest.mark.parametrize("case", list(POKES))
def test_poke_equals_the_formula(request, case):
    log, members, addrs = POKES[case]
    w = world_of(request, log)
    bank = keyed_bank(w)
    rows = rows_of(w)
    n = len(members)
    vals, cts = w.words(n, seed=len(case))
    # what an earlier write pair and read leave on the members must not reach the operations behind the poke
    a0, oa0 = w.addrs[0], w.o.address_new(w.addr_g[0])
    bank.read_prepare_write_list([1, 0], [a0, a0], w.keys)
    pre = np.stack([cts[0], cts[0]])
    bank.write_list([1, 0], pre, [a0, a0], w.keys)
    for m in range(2):
        oram = w.o.ram_new()
        oram.load(rows[m])
        oram.read_prepare_write(oa0, w.okeys)
        oram.write(cts[0], oa0, w.okeys)
        rows[m] = oram.store().reshape(rows[m].shape).copy()
        assert np.array_equal(bank.store_encrypted(m), rows[m])
    untouched = {(m, r): sha(rows[m][:, r]) for m in range(2) for r in range(w.params.rows()) if (m, r) not in {(mm, a // N) for mm, a in zip(members, addrs)}}
    want = check_poke(w, bank, rows, members, addrs, cts)
    for (m, r), h in untouched.items():
        assert sha(bank.store_encrypted(m)[:, r]) == h, ("an untouched row changed", m, r)
    # an oblivious read at the ENCRYPTED address returns the poked word
    for k, (m, a) in enumerate(zip(members, addrs)):
        addr, oaddr = enc_addr(w, a, seed=k)
        got = bank.read([addr], w.keys, first=m)[0]
        oram = w.o.ram_new()
        oram.load(want[m])
        assert np.array_equal(got, oram.read(oaddr, w.okeys)), (case, k)
        noise = decrypts(w, got, vals[k], True, (case, k))
        print(f"poke {case} entry {k}: oblivious read back, log2 noise {noise:.2f}")
    # the write pair of the poked member equals the oracle's on the oracle-poked rows: nothing kept from before the poke is used
    m = members[-1]
    wv, wct = w.words(1, seed=77)
    bank.read_prepare_write([w.addrs[1]], w.keys, first=m)
    bank.write(wct, [w.addrs[1]], w.keys, first=m)
    oram, oa1 = w.o.ram_new(), w.o.address_new(w.addr_g[1])
    oram.load(want[m])
    oram.read_prepare_write(oa1, w.okeys)
    oram.write(wct[0], oa1, w.okeys)
    assert np.array_equal(bank.store_encrypted(m), oram.store().reshape(want[m].shape)), case
    # ... and as a dense list over both members, straight behind another poke
    bank.read_prepare_write_list([1, 0], [w.addrs[2], w.addrs[1]], w.keys)
    bank.write_list([1, 0], np.stack([wct[0], wct[0]]), [w.addrs[2], w.addrs[1]], w.keys)
    rows3 = [bank.store_encrypted(i) for i in range(2)]
    want2 = check_poke(w, bank, rows3, members[:1], addrs[:1], cts[:1])
    bank.read_prepare_write_list([1, 0], [w.addrs[2], w.addrs[1]], w.keys)
    bank.write_list([1, 0], np.stack([wct[0], wct[0]]), [w.addrs[2], w.addrs[1]], w.keys)
    for i, j in ((1, 2), (0, 1)):
        oram, oa = w.o.ram_new(), w.o.address_new(w.addr_g[j])
        oram.load(want2[i])
        oram.read_prepare_write(oa, w.okeys)
        oram.write(wct[0], oa, w.okeys)
        assert np.array_equal(bank.store_encrypted(i), oram.store().reshape(want2[i].shape)), (case, "dense list behind a poke", i)


def test_poke_takes_its_words_from_the_device(w12):
    """a select's output, a register read's, a member's result, the zero word and the last peek (the old word put back) as sources"""
    w, S = w12, w12.pkg.Src
    bank = keyed_bank(w)
    rows = rows_of(w)
    vals, cts = w.words(2, seed=31)
    sel = w.selector(bank, 1, 1)
    picked = bank.select([sel], [[S.host(0), S.host(1)]], host_words=cts)
    _, row = regs_rows(w, 1)
    rf = bank.regfile(1)
    rf.load(row)
    reg = rf.read([reg_selector(w, bank, 1, 1)])
    res = bank.read([w.addrs[0]], w.keys, first=1)[0]
    members, addrs = [0, 1, 0, 1], [9, 4000, 10, 9]
    srcs = [S.select(0), S.regs(0), S.member(1), S.zero()]
    words = [picked[0], reg[0], res, np.zeros_like(res)]
    rows = check_poke(w, bank, rows, members, addrs, words, srcs=srcs)
    addr, _ = enc_addr(w, 9, seed=40)
    decrypts(w, bank.read([addr], w.keys, first=0)[0], vals[1], True, "the selected word")
    old = bank.peek_result(0, 4)
    # the old words back where they were, from the last peek: the call's own peek must not overwrite its sources
    rows = check_poke(w, bank, rows, [0, 1], [9, 4000], [old[0], old[1]], srcs=[S.peek(0), S.peek(1)])
    decrypts(w, bank.read([addr], w.keys, first=0)[0], [w.data[0][i + w.ws * 9] for i in range(w.ws)], False, "the old word put back")
    # a host slot beside a device source
    old2 = bank.peek_result(0, 2)
    check_poke(w, bank, rows, [1, 0], [1, 2], [cts[1], old2[0]], srcs=[S.host(1), S.peek(0)], host_words=cts)


@pytest.mark.parametrize("pat", [("hi", "hi"), ("alternating", "lo"), ("lo", "hi")], ids=lambda p: "-".join(p))
def test_poke_on_extreme_limbs(w12, pat):
    """rows and written words at the ends of the normalised range (not valid ciphertexts: nothing decrypts, everything compares): the sums
    R - t + w reach 3 * 2^16 and every carry of the merge's walk is taken"""
    w = w12
    bank = keyed_bank(w)
    G = w.params.glwe_len()

    def fill(kind, shape):
        n = int(np.prod(shape))
        a = {"lo": np.full(n, LO), "hi": np.full(n, HI), "alternating": np.where(np.arange(n) % 2 == 0, LO, HI)}[kind]
        return a.astype(np.int64).reshape(shape)

    rows = [fill(pat[0], (w.ws, 1, G)), rows_of(w)[1]]
    bank.load_encrypted(0, rows[0])
    words = fill(pat[1], (3, w.ws, G))
    check_poke(w, bank, rows, [0, 0, 0], [0, 1, N - 1], words)


_CONFIG_WANT = {}


@pytest.mark.parametrize("log", [12, 13])
@pytest.mark.parametrize("config", [{"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}, {"memo": 0}], ids=["safe_monitor2", "tail0_fuse0", "memo0"])
def test_other_configurations(request, config, log):
    w = world_of(request, log)
    bank = keyed_bank(w, config=config)
    members, addrs = [0, 1, 1], [3, w.max_addr - 1, N - 2]
    vals, cts = w.words(3, seed=55)
    if log not in _CONFIG_WANT:
        rows = rows_of(w)
        _CONFIG_WANT[log] = (np.stack([opeek(w, rows, m, a) for m, a in zip(members, addrs)]), opoke(w, rows, members, addrs, cts)[0])
    peeked, poked = _CONFIG_WANT[log]
    assert np.array_equal(bank.peek(members, addrs), peeked), config
    assert np.array_equal(bank.peek(members[:1], addrs[:1])[0], peeked[0]), config
    check_poke(w, bank, rows_of(w), members, addrs, cts)
    assert all(np.array_equal(bank.store_encrypted(m), poked[m]) for m in range(2))
    bank.read_prepare_write([w.addrs[0]], w.keys, first=1)
    wv, wct = w.words(1, seed=56)
    bank.write(wct, [w.addrs[0]], w.keys, first=1)
    oram, oa = w.o.ram_new(), w.o.address_new(w.addr_g[0])
    oram.load(poked[1])
    oram.read_prepare_write(oa, w.okeys)
    oram.write(wct[0], oa, w.okeys)
    assert np.array_equal(bank.store_encrypted(1), oram.store().reshape(poked[1].shape)), config
    print(f"public side {config} 2^{log}: round-off maximum {bank.roundoff_max():.4f}")   # (raises FHERAM_ERR_PRECISION above 3/8)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(w13):
    w, pkg, S, L = w13, w13.pkg, w13.pkg.Src, lib()
    bank = keyed_bank(w)
    vals, cts = w.words(2, seed=90)
    G = w.params.glwe_len()
    sel = w.selector(bank, 1, 1)

    def refused(code, call, what):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code and e.value.msg, (what, e.value)

    def raw(fn, *args):
        return getattr(L, fn)(bank._h, *args)

    mem, adr = (C.c_int * 2)(0, 1), (C.c_uint64 * 2)(5, 6)
    zero = (pkg.api._CSelectSrc * 2)(pkg.api._CSelectSrc(0, 0), pkg.api._CSelectSrc(0, 0))
    out = np.zeros((2, w.ws, G), dtype=np.int64)
    data = np.zeros(w.max_addr * w.ws, dtype=np.uint8)
    dp = data.ctypes.data_as(U8P)
    # -- before any peek: the kind and the download have nothing to name
    refused(ST_STATE, lambda: bank.peek_result(0, 1), "peek_result before any peek")
    refused(ST_STATE, lambda: bank.select([sel], [[S.peek(0)]]), "PEEK_RESULT in a select before any peek")
    refused(ST_STATE, lambda: bank.poke([0], [5], srcs=[S.peek(0)]), "PEEK_RESULT in a poke before any peek")
    refused(ST_STATE, lambda: bank.poke([0], [5], srcs=[S.select(0)]), "SELECT_RESULT before any select")
    refused(ST_STATE, lambda: bank.poke([0], [5], srcs=[S.member(1)]), "a member without a result")
    first = bank.peek([0, 1], [5, 6])
    before = (digest(bank, w), sha(bank.peek_result(0, 2)))

    def same(what):
        assert (digest(bank, w), sha(bank.peek_result(0, 2))) == before, what

    # -- FHERAM_ERR_INVALID_ARG
    assert raw("fheram_bank_peek", None, adr, 2, None) == ST_INVALID_ARG and raw("fheram_bank_peek", mem, None, 2, None) == ST_INVALID_ARG
    assert raw("fheram_bank_poke", None, adr, 2, zero, None) == ST_INVALID_ARG and raw("fheram_bank_poke", mem, None, 2, zero, None) == ST_INVALID_ARG
    assert raw("fheram_bank_poke", mem, adr, 2, None, None) == ST_INVALID_ARG
    assert raw("fheram_bank_peek_result", 0, 1, None) == ST_INVALID_ARG
    assert raw("fheram_bank_ram_load_plain", 0, 0, 2, None, data.size) == ST_INVALID_ARG
    for n in (0, -1, 17):
        assert raw("fheram_bank_peek", mem, adr, n, None) == ST_INVALID_ARG and raw("fheram_bank_poke", mem, adr, n, zero, None) == ST_INVALID_ARG, n
    for m_bad in (-1, 2):
        assert raw("fheram_bank_peek", (C.c_int * 2)(0, m_bad), adr, 2, None) == ST_INVALID_ARG
        assert raw("fheram_bank_poke", (C.c_int * 2)(0, m_bad), adr, 2, zero, None) == ST_INVALID_ARG
        assert raw("fheram_bank_ram_load_plain", m_bad, 0, 2, dp, data.size) == ST_INVALID_ARG
    for a_bad in (w.max_addr, 1 << 40):
        assert raw("fheram_bank_peek", mem, (C.c_uint64 * 2)(5, a_bad), 2, None) == ST_INVALID_ARG
        assert raw("fheram_bank_poke", mem, (C.c_uint64 * 2)(5, a_bad), 2, zero, None) == ST_INVALID_ARG
    assert raw("fheram_bank_poke", (C.c_int * 2)(1, 1), (C.c_uint64 * 2)(6, 6), 2, zero, None) == ST_INVALID_ARG   # one target twice
    refused(ST_INVALID_ARG, lambda: bank.peek_result(1, 2), "outputs outside the last peek")
    refused(ST_INVALID_ARG, lambda: bank.peek_result(0, 0), "an empty slice")
    for bad in (S(7, 0), S(9, 0), S(11, 0), S.peek(2), S.peek(-1), S.member(2), S.list(-1)):
        refused(ST_INVALID_ARG, lambda: bank.poke([0], [5], srcs=[bad]), f"source {bad.kind}, {bad.index}")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.peek(2)]]), "an output outside the last peek in a select")
    src_host = (pkg.api._CSelectSrc * 2)(pkg.api._CSelectSrc(1, 0), pkg.api._CSelectSrc(1, 16))
    assert raw("fheram_bank_poke", mem, adr, 1, src_host, None) == ST_INVALID_ARG                                  # HOST without host_words
    big = np.zeros((17, w.ws, G), dtype=np.int64)
    assert raw("fheram_bank_poke", mem, adr, 2, src_host, big.ctypes.data_as(I64P)) == ST_INVALID_ARG              # host slot 16
    for first_row, n_rows in ((0, 0), (0, 3), (2, 1), (1, 2), (1 << 62, 1 << 62)):
        assert raw("fheram_bank_ram_load_plain", 0, first_row, n_rows, dp, data.size) == ST_INVALID_ARG, (first_row, n_rows)
    assert raw("fheram_bank_ram_load_plain", 0, 0, 2, dp, data.size - 1) == ST_INVALID_ARG
    assert raw("fheram_bank_ram_load_plain", 0, 1, 1, dp, data.size) == ST_INVALID_ARG
    rf = bank.regfile(3)
    assert raw("fheram_bank_regs_load_plain", rf._h, dp, 8 * w.ws + 1) == ST_INVALID_ARG and raw("fheram_bank_regs_load_plain", rf._h, None, 8 * w.ws) == ST_INVALID_ARG
    assert raw("fheram_bank_regs_load_plain", None, dp, 8 * w.ws) == ST_INVALID_ARG
    same("after the FHERAM_ERR_INVALID_ARG refusals")
    # n * word_size > 64 (a bank of word size 8, refused before its missing rows and keys are looked at)
    wide = pkg.RamBank(pkg.Parameters(max_addr=1 << 12, word_size=8), 1)
    assert L.fheram_bank_peek(wide._h, (C.c_int * 9)(), (C.c_uint64 * 9)(), 9, None) == ST_INVALID_ARG
    assert L.fheram_bank_poke(wide._h, (C.c_int * 9)(), (C.c_uint64 * 9)(*range(9)), 9, (pkg.api._CSelectSrc * 9)(), None) == ST_INVALID_ARG
    # -- FHERAM_ERR_RANGE
    bad_w = cts.copy()
    bad_w[1, 0, 5] = (1 << 16) + 1
    refused(ST_RANGE, lambda: bank.poke([0, 1], [5, 6], words=bad_w), "a host limb out of range")
    same("after FHERAM_ERR_RANGE")
    # -- FHERAM_ERR_STATE: a member between read_prepare_write and write
    bank.read_prepare_write([w.addrs[0]], w.keys, first=1)
    before = (digest(bank, w), sha(bank.peek_result(0, 2)))
    refused(ST_STATE, lambda: bank.peek([0, 1], [5, 6]), "peek of a prepared member")
    refused(ST_STATE, lambda: bank.poke([1], [6], words=cts[:1]), "poke of a prepared member")
    refused(ST_STATE, lambda: bank.load_plain(1, data[:N * w.ws], first_row=0), "a row range into a prepared member")
    same("after FHERAM_ERR_STATE")
    assert np.array_equal(bank.peek([0], [5])[0], first[0]), "member 0 is not prepared: its peek runs"
    bank.write(cts[:1], [w.addrs[0]], w.keys, first=1)
    # -- FHERAM_ERR_UNINITIALIZED and FHERAM_ERR_KEYS
    empty = w.new_bank(2, load=False)
    empty._use_keys(w.keys)
    refused(ST_UNINITIALIZED, lambda: empty.peek([0], [5]), "peek of a member without rows")
    refused(ST_UNINITIALIZED, lambda: empty.poke([0], [5], words=cts[:1]), "poke of a member without rows")
    refused(ST_UNINITIALIZED, lambda: empty.load_plain(0, data[:N * w.ws], first_row=1), "a row range into a member without rows")
    empty.load_plain(0, data)   # (a whole-member load needs nothing)
    assert empty.peek([0], [5]).shape == (1, w.ws, G)
    # -- FHERAM_ERR_DEVICE: every one of the six device allocations in turn; the bank works on, and the next call allocates the whole set
    fresh = keyed_bank(w)
    want = fresh.read([w.addrs[0]], w.keys, first=0)
    before_fresh = digest(fresh, w)
    assert L.fheram_bank_selftest_fail_public_alloc(fresh._h, -1) == ST_INVALID_ARG
    for nth, call in enumerate([lambda: fresh.peek([0], [5]), lambda: fresh.poke([0], [5], words=cts[:1]), lambda: fresh.load_plain(1, data),
                                lambda: fresh.regfile(3).load_plain(data[:8 * w.ws]), lambda: fresh.peek([0], [5]), lambda: fresh.peek([1], [6])], start=1):
        fresh.selftest_fail_public_alloc(nth)
        refused(ST_DEVICE, call, f"device allocation {nth} of the public side fails")
        assert digest(fresh, w) == before_fresh, nth
        refused(ST_STATE, lambda: fresh.peek_result(0, 1), "no peek has run")
    assert np.array_equal(fresh.read([w.addrs[0]], w.keys, first=0), want), "a read after the refused allocations"
    assert np.array_equal(fresh.peek([0, 1], [5, 6]), first)
    fresh.selftest_fail_public_alloc(1)   # the buffers exist: nothing allocates any more, the request stays unused
    assert np.array_equal(fresh.peek([0, 1], [5, 6]), first)
    nokeys = w.new_bank(2)
    refused(ST_KEYS, lambda: nokeys.peek([0], [5]), "peek without keys")
    refused(ST_KEYS, lambda: nokeys.poke([0], [5], srcs=[S.zero()]), "poke without keys")
    assert sha(nokeys.store_encrypted(0)) == sha(w.rows[0])

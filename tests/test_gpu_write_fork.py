"""write_side_begin forks the side stream from the main stream with an event — unless the host has waited for the main stream since the last
enqueue on it (ctx.hpp main_idle), when there is nothing to fork from.  A fork skipped wrongly would let the side stage of a write (the
inverse digits of coordinate 0, read from the address's digits and the keys) run ahead of what the main stream still holds: a wrong result,
not a slow one.  Three calling patterns of the pair read_prepare_write + write, each three times in a row on one context at MAX_ADDR = 2^12
with 2-byte words; after every write the rows must equal the oracle's (and the result of every read_prepare_write too).
  synchronous   a host wait between the two ops (the flag is set: the fork is skipped)
  back to back  NULL result pointers and no wait in between (never set: the fork is taken)
  interleaved   a fheram_address_derive launch that writes the address's digits in front of the pair, with and without a wait before the
                write (the launch clears the flag and sets derive_unsynced)
All three use the same addresses (derived from the same encrypted integers) and words, so the oracle's sequence is computed once."""
import numpy as np
import pytest

from _pkg import load_package

pytestmark = pytest.mark.gpu
MAX_ADDR, WS, REPS = 1 << 12, 2, 3
KS = (0x5A3, 0, MAX_ADDR - 1)   # the addresses of the three repeats


@pytest.fixture(scope="module")
def seq(po):
    """keys, rows, per repeat (encrypted integer, its digits, words), and the oracle's results and rows after every pair"""
    pkg = load_package()
    o = po.Oracle(po.OParams(max_addr=MAX_ADDR, word_size=WS))
    sk = o.secret_gen(6100)
    evk = o.evk_gen(sk, 6101, 6102)
    okeys = o.keys_prepare(evk)
    rng = np.random.default_rng(6103)
    rows = o.ram_encrypt(rng.integers(0, 256, size=MAX_ADDR * WS, dtype=np.uint8), sk, 6104, 6105)
    bits = [o.fheuint_encrypt(k, 12, sk, 6200 + 2 * i, 6201 + 2 * i) for i, k in enumerate(KS)]
    digits = [o.address_from_fheuint(b, sign=False) for b in bits]
    words = [np.stack([o.glwe_encrypt_coeff0(int(v), sk, 6300 + 10 * i + j, 6350 + 10 * i + j) for j, v in enumerate(rng.integers(0, 256, size=WS))])
             for i in range(REPS)]
    oram = o.ram_new()
    oram.load(rows)
    want = []
    for i in range(REPS):
        oa = o.address_new(digits[i])
        res = np.array(oram.read_prepare_write(oa, okeys))
        oram.write(words[i], oa, okeys)
        want.append((res, np.array(oram.store())))
    assert not np.array_equal(want[0][1], want[1][1]) and not np.array_equal(want[1][1], want[2][1])   # every write changes the rows
    return dict(pkg=pkg, params=pkg.Parameters(max_addr=MAX_ADDR, word_size=WS), keys=pkg.EvaluationKeysPrepared.from_dict(evk), rows=rows,
                bits=bits, digits=digits, words=words, want=want)


def new_ram(seq):
    ram = seq["pkg"].Ram(seq["params"])
    ram.load_encrypted(seq["rows"])
    ram._use_keys(seq["keys"])
    return ram


def check(ram, seq, i, what):
    res, rows = seq["want"][i]
    assert np.array_equal(ram.result(), res), f"{what}: result of read_prepare_write {i} differs"
    assert np.array_equal(ram.store_encrypted(), rows), f"{what}: rows after write {i} differ"


def test_synchronous_pair(seq):
    ram = new_ram(seq)
    for i in range(REPS):
        a = seq["pkg"].Address(seq["params"], list(seq["digits"][i]))
        ram.read_prepare_write(a, seq["keys"], download=False)
        ram.sync()
        ram.write(seq["words"][i], a, seq["keys"])
        check(ram, seq, i, "synchronous")


def test_back_to_back_pair(seq):
    ram = new_ram(seq)
    for i in range(REPS):
        a = seq["pkg"].Address(seq["params"], list(seq["digits"][i]))
        ram.read_prepare_write(a, seq["keys"], download=False)
        ram.write(seq["words"][i], a, seq["keys"])
        check(ram, seq, i, "back to back")


def test_pair_behind_a_derive_launch(seq):
    pkg = seq["pkg"]
    ram = new_ram(seq)
    a = pkg.Address.alloc(ram)
    for i in range(REPS):
        fu = pkg.FheUintPrepared.from_host(ram, seq["bits"][i])
        ram.sync()
        ram.derive_addresses([fu], [a])            # one launch on the main stream, no host wait: a's digits are being written
        ram.read_prepare_write(a, seq["keys"], download=False)
        if i != 1:
            ram.sync()
        ram.write(seq["words"][i], a, seq["keys"])
        check(ram, seq, i, "behind a derive launch")

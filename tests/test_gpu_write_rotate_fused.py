"""The write's fused row chain (k_write_chain / k_write_chain_t) also writes the tree's rotated copy of ct_lo (ram.rs:629), from the workgroup
of row 0 of every word, so that no k_rotate launch follows it.  By the default decision the fused chain is reached from 129 ciphertexts on;
here it is forced on small RAMs (limb_split = 0, fine_split = 0, chain = 1; nco = 2 because a lone context otherwise splits so few rows by
column, which rules the Chain form out) and the example flow read_prepare_write -> write -> read_prepare_write -> write -> read is compared
with the oracle after every op: the result, the rows, and the tree (after a write: rot(ct_lo, -rows), computed from the oracle's ct_lo).
The second pair starts from what the first write left, so a wrong tree copy also shows in its rows.

Shapes: MAX_ADDR = 2^13 with 2-byte words (two rows per word: row 0 and a non-zero row both exist, two words: "row 0 of EACH word";
rot by -2 crosses the sign boundary at coefficients 0 and 1), and 2^14 with 1-byte words on the README block (5-limb keys)."""
import numpy as np
import pytest

from _oracle_engine import OracleShardEngine
from _pkg import load_package
from test_gpu_parity import World

pytestmark = pytest.mark.gpu
CHAIN = {"limb_split": 0, "fine_split": 0, "chain": 1, "nco": 2}
README = {"k_glwe_pt": 9, "k_evk_trace": 85}


def words(w, ws, seed):
    vals = w.rng.integers(0, 256, size=ws, dtype=np.uint8)
    return np.stack([w.o.glwe_encrypt_coeff0(int(v), w.sk, seed + i, seed + 50 + i) for i, v in enumerate(vals)])


def eng_read(eng, w, prepare_write):
    part = eng.read_partial(w.addr_g, w.okeys, prepare_write)
    return eng.read_finish(w.addr_g, w.okeys, part[None], prepare_write)


def eng_write(eng, w, wct):
    """-> the tree after the write: ct_lo * X^-rows per word (ram.rs:629)"""
    ct_lo = eng.write_root(wct, w.addr_g, w.okeys)
    eng.write_shard(w.addr_g, w.okeys, ct_lo)
    return np.stack([w.o.glwe_rotate(-eng.R, ct_lo[s]) for s in range(eng.ws)])


@pytest.mark.parametrize("log_max_addr,ws,crypto", [(13, 2, {}), (14, 1, README)], ids=["2_13x2", "2_14x1_readme"])
def test_flow_through_the_forced_write_chain(po, log_max_addr, ws, crypto):
    pkg = load_package()
    w = World(po, 1 << log_max_addr, word_size=ws, seed=70 + log_max_addr, **crypto)
    ram = pkg.Ram(w.ram.params, config=CHAIN)
    ram.load_encrypted(w.rows)
    eng = OracleShardEngine(w.o, ram.params, w.rows, 0, 1)
    assert eng.R == 1 << (log_max_addr - 12) and eng.R >= 2
    ram.profile_enable(True)
    for rnd in range(2):
        got = ram.read_prepare_write(w.addr, w.keys)
        assert np.array_equal(got, eng_read(eng, w, True)), f"read_prepare_write {rnd} differs"
        assert np.array_equal(ram.store_encrypted(), eng.data), f"rows after read_prepare_write {rnd} differ"
        assert np.array_equal(ram.tree(0), eng.tree), f"tree after read_prepare_write {rnd} differs"
        wct = words(w, ws, 900 + 10 * rnd)
        ram.write(wct, w.addr, w.keys)
        tree = eng_write(eng, w, wct)
        assert np.array_equal(ram.store_encrypted(), eng.data), f"rows after write {rnd} differ"
        assert np.array_equal(ram.tree(0), tree), f"the tree's rotated copy of ct_lo after write {rnd} differs"
    got = ram.read(w.addr, w.keys)
    assert np.array_equal(got, eng_read(eng, w, False)), "read-back differs"
    ram.profile_enable(False)
    # the forced form was the one that ran: one fused chain launch per write over every row of every word
    prof = ram.profile_get("write_chain_launch")
    assert prof["launches"] == 2 and prof["blocks"] == 2 * eng.R * ws, prof


def test_bank_write_of_two_members_through_the_table_form(po):
    """k_write_chain_t: the same flow on a bank of two members (a range of a bank takes one workgroup per ciphertext), every member against
    its own oracle flow; members differ in rows, address and words"""
    pkg = load_package()
    ws = 2
    ws_worlds = [World(po, 1 << 13, word_size=ws, seed=90), None]
    w0 = ws_worlds[0]
    # the second member: the same keys (a bank shares them), other rows, another address
    rng = np.random.default_rng(91)
    data1 = rng.integers(0, 256, size=(1 << 13) * ws, dtype=np.uint8)
    rows1 = w0.o.ram_encrypt(data1, w0.sk, 591, 691)
    idx1 = (w0.idx + 4097 + 13) % (1 << 13)
    addr1_g = w0.o.address_encrypt(idx1, w0.sk, 791, 891)
    bank = pkg.RamBank(w0.ram.params, 2, 0, config=dict(CHAIN, nco=0))
    bank.load_encrypted(0, w0.rows)
    bank.load_encrypted(1, rows1)
    A = [w0.addr, pkg.Address(w0.ram.params, list(addr1_g))]

    class Member:   # what eng_read / eng_write take of a World
        def __init__(self, addr_g):
            self.addr_g, self.okeys, self.o = addr_g, w0.okeys, w0.o

    mem = [Member(w0.addr_g), Member(addr1_g)]
    engs = [OracleShardEngine(w0.o, w0.ram.params, r, 0, 1) for r in (w0.rows, rows1)]
    bank.profile_enable(True)
    for rnd in range(2):
        got = bank.read_prepare_write(A, w0.keys)
        for m in range(2):
            assert np.array_equal(got[m], eng_read(engs[m], mem[m], True)), (rnd, m, "read_prepare_write differs")
        W = np.stack([words(w0, ws, 1000 + 100 * rnd + 10 * m) for m in range(2)])
        bank.write(W, A, w0.keys)
        for m in range(2):
            tree = eng_write(engs[m], mem[m], W[m])
            assert np.array_equal(bank.store_encrypted(m), engs[m].data), (rnd, m, "rows after write differ")
            assert np.array_equal(bank.tree(m), tree), (rnd, m, "the tree's rotated copy of ct_lo differs")
    got = bank.read(A, w0.keys)
    for m in range(2):
        assert np.array_equal(got[m], eng_read(engs[m], mem[m], False)), (m, "read-back differs")
    bank.profile_enable(False)
    prof = bank.profile_get("write_chain_launch")
    assert prof["launches"] == 2 and prof["blocks"] == 2 * 2 * engs[0].R * ws, prof

"""fheram_read_batch / Ram.read_batch: K independent Ram::read (ram.rs:172-191) of the same RAM as one operation.

Every slice of a batch must be int64-identical to Ram.read of its address on the same state (and to the oracle's read), in
every launch form the batch can take; afterwards the context must be in the state the K reads leave (result, write path)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _pkg import load_package

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS = 1, 2, 3, 4


class World:
    """Keys, one encrypted RAM and n_addr encrypted addresses from the oracle's setup side."""

    def __init__(self, po, max_addr, word_size=4, seed=0, n_addr=8, **crypto):
        pkg = load_package()
        self.pkg, self.po, self.crypto = pkg, po, crypto
        self.max_addr, self.ws = max_addr, word_size
        self.o = po.Oracle(po.OParams(max_addr=max_addr, word_size=word_size, **crypto))
        o = self.o
        self.sk = o.secret_gen(900 + seed)
        self.evk = o.evk_gen(self.sk, 901 + seed, 902 + seed)
        self.keys = pkg.EvaluationKeysPrepared.from_dict(self.evk)
        rng = np.random.default_rng(903 + seed)
        self.data = rng.integers(0, 256, size=max_addr * word_size, dtype=np.uint8)
        self.rows = o.ram_encrypt(self.data, self.sk, 904 + seed, 905 + seed)
        self.idx = [int(v) for v in rng.integers(0, max_addr, size=n_addr)]
        self.addr_g = [o.address_encrypt(i, self.sk, 1000 + seed + 2 * j, 1001 + seed + 2 * j) for j, i in enumerate(self.idx)]
        self.ram = self.new_ram()
        self.addrs = [pkg.Address(self.ram.params, list(g)) for g in self.addr_g]
        self._okeys = None
        self._oread = {}
        self._gread = {}

    def new_ram(self, config=None, load=True):
        pkg = self.pkg
        params = pkg.Parameters(max_addr=self.max_addr, word_size=self.ws, **self.crypto)
        ram = pkg.Ram(params, 0, config=config)
        if load:
            ram.load_encrypted(self.rows)
        return ram

    def oracle_read(self, j):
        if j not in self._oread:
            if self._okeys is None:
                self._okeys = self.o.keys_prepare(self.evk)
            oram = self.o.ram_new()
            oram.load(self.rows)
            self._oread[j] = oram.read(self.o.address_new(self.addr_g[j]), self._okeys)
        return self._oread[j]

    def gpu_read(self, j):
        """Ram.read of address j on the default context (the RAM is never written there)"""
        if j not in self._gread:
            self._gread[j] = self.ram.read(self.addrs[j], self.keys).copy()
        return self._gread[j]

    def check_word(self, cts, j, data=None, written=False):
        """examples/fhe-ram.rs:104-115"""
        data = self.data if data is None else data
        for i in range(self.ws):
            want = self.o.expected_plain(int(data[i + self.ws * self.idx[j]]), self.o.p.k_glwe_pt, written)
            v, noise = self.o.glwe_decrypt(cts[i], want, self.sk)
            assert v == want, (j, i, v, want, noise)
            assert noise < -(self.o.p.k_glwe_pt + 1), noise


@pytest.fixture(scope="module")
def w14(po):
    return World(po, 1 << 14)


def lib():
    return load_package().library()


def tail_stats(ram):
    t = ram.tail_stats()
    return t["launches"], t["fallbacks"]


def c_batch(ram, handles, out=None):
    arr = (C.c_void_p * max(1, len(handles)))(*handles)
    return lib().fheram_read_batch(ram._h, arr, len(handles), out.ctypes.data_as(C.POINTER(C.c_int64)) if out is not None else None)


@pytest.mark.parametrize("sel", [[0], [1, 2], [3, 4, 5], [6, 7, 0, 1], list(range(8)), [2, 5, 2]],
                         ids=["K1", "K2", "K3", "K4", "K8", "K3-duplicate"])
def test_batch_equals_reads_oracle_and_decrypts_2_14(w14, sel):
    w = w14
    got = w.ram.read_batch([w.addrs[j] for j in sel], w.keys)
    assert got.shape == (len(sel), w.ws, w.ram.params.glwe_len())
    for k, j in enumerate(sel):
        assert np.array_equal(got[k], w.gpu_read(j)), (k, j, np.count_nonzero(got[k] != w.gpu_read(j)))
        assert np.array_equal(got[k], w.oracle_read(j)), (k, j)
        w.check_word(got[k], j)


@pytest.mark.parametrize("config", [{"tail": 0}, {"tail_ep": 0}, {"mid": 0}, {"fuse": 0}, {"safe": 1}, {"graph": 1},
                                    {"tail_test": 1}, {"mid_test": 1}],
                         ids=["tail0", "tail_ep0", "mid0", "fuse0", "safe", "graph", "tail-gives-up", "mid-gives-up"])
def test_forced_forms_equal_sequential_reads_2_14(w14, config):
    """K = 3 (12 ciphertexts: the mid chains and per-address product launches) and K = 2 (8 ciphertexts: the trace-only tail over the
    batch).  At 2^14 coordinate 1 has ONE digit (base2d [[3,3,3,3],[2]]), so its products are per-address launches and the tail
    carries none: the tail with per-address products and its fallback are tested at 2^16 below."""
    w = w14
    ram = w.new_ram(config)
    addrs = [w.pkg.Address(ram.params, list(g)) for g in w.addr_g]
    for sel in ([0, 3, 6], [5, 1]):
        seq = [ram.read(addrs[j], w.keys).copy() for j in sel]
        l0, f0 = tail_stats(ram) if config.get("tail_test") else (0, 0)
        got = ram.read_batch([addrs[j] for j in sel], w.keys)
        for k, j in enumerate(sel):
            assert np.array_equal(got[k], seq[k]), (config, sel, k)
            assert np.array_equal(got[k], w.gpu_read(j)), (config, sel, k)
        if config.get("tail_test") and len(sel) == 2:   # the batch's own tail launch gave up and its fallback produced the results
            l1, f1 = tail_stats(ram)
            assert l1 > l0 and f1 > f0, (l0, l1, f0, f1)


@pytest.mark.parametrize("case", ["2_12", "readme_2_14"])
def test_one_row_and_readme_block(po, case):
    w = World(po, 1 << 12, seed=50, n_addr=4) if case == "2_12" else World(po, 1 << 14, seed=60, n_addr=4, k_glwe_pt=9, k_evk_trace=85)
    for sel in ([0, 1], [0, 1, 2, 3]):
        got = w.ram.read_batch([w.addrs[j] for j in sel], w.keys)
        for k, j in enumerate(sel):
            assert np.array_equal(got[k], w.gpu_read(j)), (case, sel, k)
            w.check_word(got[k], j)
    assert np.array_equal(got[0], w.oracle_read(0))


@pytest.fixture(scope="module", params=["source", "readme"])
def w16(po, request):
    """2^16: coordinate 1 has two digits (base2d [[3,3,3,3],[3,1]]), so at K = 2 (8 ciphertexts) the batch's tail carries the
    per-address products (k_trace_tail_t), and at K = 4 (16 rows x 16 ciphertexts) the row chains of all addresses are the one
    fused launch (k_read_chain_t).  "readme": the 5-limb trace keys (the <5, ...> instantiations)."""
    crypto = {} if request.param == "source" else {"k_glwe_pt": 9, "k_evk_trace": 85}
    return World(po, 1 << 16, seed=80, n_addr=4, **crypto)


def test_batched_kernels_2_16(w16):
    w = w16
    ram = w.new_ram()
    addrs = [w.pkg.Address(ram.params, list(g)) for g in w.addr_g]
    rows = ram.params.rows()
    for sel, form in (([0, 1], "keyswitch_tail_launch"), ([0, 1, 2, 3], "read_chain_launch")):
        seq = [ram.read(addrs[j], w.keys).copy() for j in sel]
        ram.profile_enable(True)
        ram.profile_reset()
        got = ram.read_batch([addrs[j] for j in sel], w.keys)
        prof = ram.profile_get(form)
        ram.profile_enable(False)
        if form == "read_chain_launch":
            assert prof["launches"] == 1 and prof["blocks"] == rows * len(sel) * w.ws, prof    # ONE launch for every address's rows
        else:
            assert prof["launches"] == 1 and prof["blocks"] == len(sel) * w.ws * 12, prof     # ONE tail over the batch, 12 trace steps
        for k, j in enumerate(sel):
            assert np.array_equal(got[k], seq[k]), (sel, k)
            w.check_word(got[k], j)
    assert np.array_equal(got[3], w.oracle_read(3))


def test_tail_fallback_with_per_address_operands_2_16(w16):
    """tail_test: the batch's k_trace_tail_t gives up late and the predicated k_read_chain_t behind it redoes coordinate 1's products
    (operands of address y / ws) and the trace from the batch's packed rows"""
    w = w16
    ram = w.new_ram({"tail_test": 1})
    addrs = [w.pkg.Address(ram.params, list(g)) for g in w.addr_g]
    for sel in ([2, 0], [1, 1]):
        seq = [ram.read(addrs[j], w.keys).copy() for j in sel]
        l0, f0 = tail_stats(ram)
        got = ram.read_batch([addrs[j] for j in sel], w.keys)
        l1, f1 = tail_stats(ram)
        assert l1 == l0 + 1 and f1 == f0 + 1, (l0, l1, f0, f1)   # the batch's one tail launch, and its fallback taken
        for k, j in enumerate(sel):
            assert np.array_equal(got[k], seq[k]), (sel, k)
            w.check_word(got[k], j)


def test_eight_addresses_one_row_chain_2_16(po):
    """K = 8 at word size 1: the all-zero source map over all eight entries of k_read_chain_t (every entry reads the same 16 rows).
    16 x 8 = 128 ciphertext rows are 256 workgroups when split by column, which a chip of 256 CUs still holds (launch.hpp pick_nco), so a
    batch of this shape runs its products per address by default; with one workgroup per ciphertext (nco = 2) they are the ONE fused
    launch of rows * 8 blocks.  Both against eight sequential reads, exactly."""
    w = World(po, 1 << 16, word_size=1, seed=140, n_addr=8)
    rows = w.ram.params.rows()
    seq = [w.gpu_read(j) for j in range(8)]
    for config in (None, {"nco": 2}):
        ram = w.new_ram(config)
        addrs = [w.pkg.Address(ram.params, list(g)) for g in w.addr_g]
        own = [ram.read(a, w.keys).copy() for a in addrs]
        ram.profile_enable(True)
        ram.profile_reset()
        got = ram.read_batch(addrs, w.keys)
        prof = ram.profile_get("read_chain_launch")
        ram.profile_enable(False)
        print("read_batch K=8 2^16 ws=1", config, "read_chain_launch", prof)
        for k in range(8):
            assert np.array_equal(got[k], own[k]), (config, k)
            assert np.array_equal(got[k], seq[k]), (config, k)
        if config:
            assert prof["launches"] == 1 and prof["blocks"] == rows * 8, prof
    w.check_word(got[5], 5)
    assert np.array_equal(got[7], w.oracle_read(7))


def unsynced_flow(w, ram, sync):
    """read_batch of two addresses left on the device, read_prepare_write, write and a read-back; sync: the host waits after every call"""
    addrs = [w.pkg.Address(ram.params, list(g)) for g in w.addr_g[:3]]
    for a in addrs:
        a._device(ram)   # (the upload is a host wait of its own: before the flow)
    wct = np.stack([w.o.glwe_encrypt_coeff0(17 + 5 * i, w.sk, 5200 + i, 5300 + i) for i in range(w.ws)])
    wait = ram.sync if sync else (lambda: None)
    ram.read_batch(addrs[:2], w.keys, download=False)
    wait()
    ram.read_prepare_write(addrs[2], w.keys, download=False)
    wait()
    ram.write(wct, addrs[2], w.keys)
    wait()
    return ram.read(addrs[2], w.keys).copy(), ram.store_encrypted(), ram.tree(0)


def assert_unsynced_flow_equals_synced(w):
    ram, ref = w.new_ram(), w.new_ram()
    t0 = tail_stats(ram)
    got = unsynced_flow(w, ram, False)
    want = unsynced_flow(w, ref, True)
    for g, x, what in zip(got, want, ("result", "rows", "tree")):
        assert np.array_equal(g, x), (what, np.count_nonzero(g != x))
    t1 = tail_stats(ram)
    assert t1[0] > t0[0] and t1[1] == t0[1], (t0, t1)   # tail launches, and no fallback


def test_batch_then_read_prepare_write_without_a_host_wait_2_14(w14):
    """A batch of two (8 ciphertexts: its end is the tail launch), then — the host not waiting — read_prepare_write, which parks the gate
    wave beside its launches, write and a read-back: result, rows and tree as with a host wait after every call, and the tail's
    fallback never runs.  At 2^14 coordinate 1 has one digit, so the batch's tail is the trace alone (k_trace_tail)."""
    assert_unsynced_flow_equals_synced(w14)


def test_batch_then_read_prepare_write_without_a_host_wait_2_16(w16):
    """The same where the batch's tail carries the per-address products (k_trace_tail_t, two digits: from 2^16 on) while its rows'
    chains are not the fused launch: the fallback enqueued behind that tail is the whole-register-file k_read_chain_t, so the context
    counts a wide launch as under way and the read_prepare_write behind it records ev_opstart for its gate wave."""
    assert_unsynced_flow_equals_synced(w16)


def test_2_18_against_committed_digests(po):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_golden import golden_inputs, sha
    pkg = load_package()
    d, inp = golden_inputs(po, 1 << 18)
    ws, max_addr = d["word_size"], d["max_addr"]
    ram = pkg.Ram.new_from_ram_params(ws, [3, 3, 3, 3], max_addr)
    keys = pkg.EvaluationKeysPrepared(inp["gal_els"], list(inp["atk_glwe"]), inp["atk_ggsw_inv"], inp["tsk"])
    a = pkg.Address(ram.params, list(inp["addr"]))
    ram.load_encrypted(inp["rows"])
    l0, f0 = C.c_uint64(), C.c_uint64()
    lib().fheram_tail_stats(ram._h, C.byref(l0), C.byref(f0))
    got = ram.read_batch([a, a], keys)
    assert sha(got[0]) == d["outputs"]["read"] and sha(got[1]) == d["outputs"]["read"]
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=ws))
    rng = np.random.default_rng(77)
    idx = [int(v) for v in rng.integers(0, max_addr, size=3)]
    extra = [pkg.Address(ram.params, list(o.address_encrypt(i, inp["sk"], 7000 + 2 * j, 7001 + 2 * j))) for j, i in enumerate(idx)]
    for sel in ([extra[0], a], [extra[1], a, extra[2], extra[0]]):
        seq = [ram.read(x, keys).copy() for x in sel]
        got = ram.read_batch(sel, keys)
        for k in range(len(sel)):
            assert np.array_equal(got[k], seq[k]), (len(sel), k)
    for k, i in enumerate(idx[:1]):   # decrypts to the word (examples/fhe-ram.rs:104-115)
        for wi in range(ws):
            want = o.expected_plain(int(inp["data"][wi + ws * i]), o.p.k_glwe_pt, False)
            v, noise = o.glwe_decrypt(got[3][wi], want, inp["sk"])
            assert v == want and noise < -(o.p.k_glwe_pt + 1)
    l1, f1 = C.c_uint64(), C.c_uint64()
    assert lib().fheram_tail_stats(ram._h, C.byref(l1), C.byref(f1)) == 0
    assert l1.value > l0.value and f1.value == f0.value, (l0.value, l1.value, f0.value, f1.value)   # no fallback in the default run


def test_state_machine(po):
    w = World(po, 1 << 14, seed=20, n_addr=3)
    ram, keys, a, b = w.ram, w.keys, w.addrs[0], w.addrs[1]
    oram = w.o.ram_new()
    oram.load(w.rows)
    okeys = w.o.keys_prepare(w.evk)
    oa, ob = w.o.address_new(w.addr_g[0]), w.o.address_new(w.addr_g[1])

    ram.read_prepare_write(a, keys)
    oram.read_prepare_write(oa, okeys)
    with pytest.raises(load_package().FheRamError) as e:
        ram.read_batch([a, b], keys)
    assert e.value.code == ST_STATE
    val = np.array([11, 22, 33, 44], dtype=np.uint8)
    wct = np.stack([w.o.glwe_encrypt_coeff0(int(v), w.sk, 3000 + i, 3100 + i) for i, v in enumerate(val)])
    ram.write(wct, a, keys)
    oram.write(wct, oa, okeys)
    data2 = w.data.copy()
    data2[w.ws * w.idx[0]: w.ws * (w.idx[0] + 1)] = val
    got = ram.read_batch([a, b], keys)
    w.check_word(got[0], 0, data2, written=True)
    if w.idx[1] != w.idx[0]:
        w.check_word(got[1], 1, data2)
    # the last address's result is what fheram_result_download returns after the batch
    res = np.zeros((w.ws, ram.params.glwe_len()), dtype=np.int64)
    assert lib().fheram_result_download(ram._h, res.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert np.array_equal(res, got[1])
    # a read_prepare_write / write after the batch behaves as after two reads (memo on: the write resumes from it)
    ram.read_prepare_write(b, keys)
    oram.read_prepare_write(ob, okeys)
    wct2 = np.stack([w.o.glwe_encrypt_coeff0(int(v), w.sk, 3200 + i, 3300 + i) for i, v in enumerate(val[::-1])])
    ram.write(wct2, b, keys)
    oram.write(wct2, ob, okeys)
    assert np.array_equal(ram.store_encrypted(), oram.store())


def test_errors(po, w14):
    w = w14
    pkg = load_package()
    h = [x._device(w.ram) for x in w.addrs[:2]]
    assert c_batch(w.ram, []) == ST_INVALID_ARG
    assert c_batch(w.ram, h * 4 + h[:1]) == ST_INVALID_ARG                 # 9 > FHERAM_READ_BATCH_MAX
    assert b"n_addr" in lib().fheram_last_error(w.ram._h)
    assert c_batch(w.ram, [h[0], None]) == ST_INVALID_ARG
    other = w.new_ram()
    assert c_batch(w.ram, [h[0], w.addrs[2]._device(other)]) == ST_INVALID_ARG
    assert b"does not belong" in lib().fheram_last_error(w.ram._h)
    with pytest.raises(pkg.FheRamError):
        w.ram.read_batch([], w.keys)
    with pytest.raises(pkg.FheRamError):
        w.ram.read_batch(w.addrs + w.addrs[:1], w.keys)
    empty = w.new_ram(load=False)
    with pytest.raises(pkg.FheRamError) as e:
        empty.read_batch(w.addrs[:2], w.keys)
    assert e.value.code == ST_UNINITIALIZED
    nokeys = w.new_ram()
    assert c_batch(nokeys, [x._device(nokeys) for x in w.addrs[:2]]) == ST_KEYS
    params = pkg.Parameters(max_addr=w.max_addr, word_size=w.ws)
    shard = pkg.Ram(params, 0, shard=0, n_shards=2)
    shard.load_encrypted(w.rows[:, 0::2])
    with pytest.raises(pkg.FheRamError) as e:
        shard.read_batch(w.addrs[:2], w.keys)
    assert e.value.code == ST_INVALID_ARG
    # the context that refused all of these still reads
    assert np.array_equal(w.ram.read_batch(w.addrs[:2], w.keys)[1], w.gpu_read(1))

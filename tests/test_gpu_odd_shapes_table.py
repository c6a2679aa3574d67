"""The operations on several addresses — fheram_bank ranges, fheram_read_batch, fheram_bank_read_list, fheram_address_derive — at the
shapes the single-context test_odd_shapes_flow_and_oracle_agreement covers for one address: row counts that are no power of two, a ragged
last row, word sizes 1 to 3, digit plans of 2 to 8 digits, one coordinate.  The table forms index their operands by y / ws with a stride of
n_digits * GGSW, read rows through the member map and choose their form from rows, d0, L0 and the parity of d0 (path.hpp read_local,
launch.hpp chain_form / use_row_fuse): all of that changes with the shape, and none of it had run with n > 1 outside 2^12 .. 2^18 and the
[3,3,3,3] plan.

Valid ciphertexts throughout; every result, row and tree level is compared with the oracle per member or entry by np.array_equal — no
tolerance anywhere — and one word per shape is decrypted and its noise checked.  The launch profile of the row chains is printed per op,
and asserted where chain_form leaves no choice (see row_chain_expected)."""
import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import CLASSES, World, profiled
from test_gpu_extremes import _threads

pytestmark = pytest.mark.gpu

ST_UNSUPPORTED = 5
N, LOGN = 4096, 12
DEFAULT = (3, 3, 3, 3)
# (max_addr, word size, digit plan)
SHAPES = [
    (11 * 4096, 3, DEFAULT),           # 11 rows: a ragged packer tree with lone accumulators; L0 = 8; y / ws with ws = 3
    (5000, 2, DEFAULT),                # 2 rows, the last one partly filled; a 1-bit second coordinate
    (3 * 4096, 1, (2, 2, 2, 2, 2, 2)),  # 7 digits: the operand stride is neither 5 nor 6 digits; d0 = 6
    (1 << 14, 2, (4, 4, 4)),           # 4 digits
    (5000, 2, (5, 4, 3)),              # d0 = 3, odd
    (1 << 13, 1, (12,)),               # one digit per coordinate
    (1000, 1, DEFAULT),                # below N: n2 == 1, the per-entry ep_chain branch
    # beside the seven above: d0 = 3 at a size where a bank's rows DO take the table launch (99 ciphertext rows), so that read runs
    # k_read_chain_t with three digits and read_prepare_write takes the `prepare_write && (d0 & 1)` branch of read_local beside it
    (11 * 4096, 3, (5, 4, 3)),
]
CONFIGS = [{"monitor": 2}, {"monitor": 2, "fuse": 0}]
M = 3
# address index per member: the whole range reads at RD, prepares and writes at WR; the sub-range [1, 3) at RD2 / WR2
RD, WR = [0, 1, 2], [1, 2, 3]
RD2, WR2 = [3, 0], [0, 1]
BATCH = [0, 1, 2]                              # on member 0's rows
LIST_MEMBERS, LIST_ADDRS = [2, 0, 0, 1], [2, 0, 1, 3]
_WORLDS = {}


def _shape_id(s):
    return f"{s[0]}x{s[1]}-" + "_".join(map(str, s[2]))


class ShapeWorld(World):
    """test_gpu_bank.World with a digit plan; addresses 0, max_addr - 1 and two in between; the oracle's side of every test, computed once"""

    def __init__(self, po, max_addr, ws, plan, seed):
        super().__init__(po, max_addr, M, word_size=ws, seed=seed, n_addr=0, decomp_n=list(plan))
        self.o.set_threads(_threads())
        self.idx = [0, max_addr - 1, max_addr // 2 + 1, max_addr // 3]
        assert len(set(self.idx)) == 4
        self.addr_g = [self.o.address_encrypt(i, self.sk, 2000 + seed + 2 * j, 2001 + seed + 2 * j) for j, i in enumerate(self.idx)]
        self.addrs = [self.pkg.Address(self.params, list(g)) for g in self.addr_g]
        self.n2 = len(self.params.base2d().v)
        self.d0 = len(self.params.base2d().v[0].d)
        self.n_digits = self.params.base2d().as_1d().size()
        self.n_bits = sum(sum(b.d) for b in self.params.base2d().v)
        self._oaddr, self._oread, self._oflow, self._derived = {}, {}, None, None
        self.wordsA, self.wordsB = self.words(M, seed=1), self.words(2, seed=2)

    def oaddr(self, j):
        if j not in self._oaddr:
            self._oaddr[j] = self.o.address_new(self.addr_g[j])
        return self._oaddr[j]

    def oread(self, m, j):
        """the oracle's read of member m's rows as loaded at address j"""
        if (m, j) not in self._oread:
            self._oread[(m, j)] = self.new_oram(m).read(self.oaddr(j), self.okeys)
        return self._oread[(m, j)]

    def oflow(self):
        """the oracle's flow per member: the whole range [0, 3), then the sub-range [1, 3) on the state that leaves"""
        if self._oflow is None:
            orams = [self.new_oram(m) for m in range(M)]

            def run(members, rd, wr, wct):
                out = {k: [] for k in ("read", "rpw", "tree_after_rpw", "rows_after_write", "tree_after_write", "read_back")}
                for k, m in enumerate(members):
                    o = orams[m]
                    out["read"].append(o.read(self.oaddr(rd[k]), self.okeys))
                    out["rpw"].append(o.read_prepare_write(self.oaddr(wr[k]), self.okeys))
                    out["tree_after_rpw"].append(o.tree(0))
                    o.write(wct[k], self.oaddr(wr[k]), self.okeys)
                    out["rows_after_write"].append(o.store())
                    out["tree_after_write"].append(o.tree(0))
                    out["read_back"].append(o.read(self.oaddr(wr[k]), self.okeys))
                return out

            self._oflow = (run([0, 1, 2], RD, WR, self.wordsA[1]), run([1, 2], RD2, WR2, self.wordsB[1]))
        return self._oflow

    def derived(self):
        """three encrypted integers (0, max_addr - 1, one in between), the digits the oracle derives from them (the convention of
        Address::encrypt_sk: sign = False) and the oracle's read of member m through the m-th of them"""
        if self._derived is None:
            values = [0, self.max_addr - 1, self.max_addr // 2 + 1]
            bits = [self.o.fheuint_encrypt(v, self.n_bits, self.sk, 5200 + 2 * k, 5201 + 2 * k) for k, v in enumerate(values)]
            digits = [self.o.address_from_fheuint(b, sign=False) for b in bits]
            reads = [self.new_oram(m).read(self.o.address_new(digits[m]), self.okeys) for m in range(M)]
            self._derived = (values, bits, digits, reads)
        return self._derived


@pytest.fixture(scope="module", params=SHAPES, ids=_shape_id)
def w(po, request):
    _WORLDS.clear()   # (one shape's world at a time)
    _WORLDS[request.param] = ShapeWorld(po, *request.param, seed=300 + 20 * SHAPES.index(request.param))
    return _WORLDS[request.param]


def row_chain_expected(w, cfg, n, prepare_write=False):
    """Whether the rows of an operation on n members run as the ONE launch with an operand table (k_read_chain_t / k_write_chain_t), as far
    as launch.hpp decides it whatever the other switches are: True, False, or None where chain_form's answer depends on them.
    use_row_fuse needs the `fuse` switch, two coordinates and both chains of a row in the Chain form.  A bank range or list takes one
    workgroup per ciphertext (one_wg), so with B = rows * n * ws ciphertext rows: B > 64 rules out the limb split, the fine split (B * 24
    workgroups on 256 CUs) and every Mid split (at most 64), and a chain of 2 .. CHAIN_MAX = 12 steps is then in the Chain form: the
    products need d0 >= 2, and the trace chains have L0 = 12 - ceil(log2 rows) >= 2 (read) or 12 (write) steps.  B <= 32 admits the limb
    split for the products (B * 8 workgroups fit 256 CUs), or the Mid form, or the products are too few: never the Chain form.
    read_prepare_write leaves the fused launch to read when d0 is odd (read_local)."""
    rows = w.params.rows()
    B = rows * n * w.ws
    if not cfg.get("fuse", 1) or w.n2 == 1 or w.d0 < 2 or B <= 32:
        return False
    if B <= 64:
        return None
    L0 = LOGN - (rows - 1).bit_length()
    assert 2 <= L0 <= 12 and w.d0 <= 12
    return not (prepare_write and w.d0 % 2 == 1)


def show(w, what, prof):
    print(f"{_shape_id((w.max_addr, w.ws, tuple(w.params.decomp_n())))} {what}: " +
          (", ".join(f"{c} {v['launches']}x/{v['blocks']}" for c, v in prof.items() if v["launches"]) or "none of the chain launches"))


def check_rows_profile(w, cfg, n, op, prof):
    cls = "write_chain_launch" if op == "write" else "read_chain_launch"
    want = row_chain_expected(w, cfg, n, prepare_write=(op == "rpw"))
    if want is True:
        assert prof[cls]["launches"] == 1 and prof[cls]["blocks"] == w.params.rows() * n * w.ws, (op, prof)
    elif want is False:
        assert prof[cls]["launches"] == 0, (op, prof)


def snapshot(w, bank, m):
    return bank.store_encrypted(m), (bank.tree(m, 0) if w.n2 == 2 else None), bank.state(m)


def assert_untouched(w, bank, m, snap, what):
    rows, tree, state = snap
    assert bank.state(m) == state, (what, m)
    assert np.array_equal(bank.store_encrypted(m), rows), (what, m)
    if tree is not None:
        assert np.array_equal(bank.tree(m, 0), tree), (what, m)


def same(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, (what, f"{len(bad)} limbs differ, the first at {tuple(int(x) for x in bad[0])}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
def test_bank_range_and_sub_range(w, cfg):
    """read, read_prepare_write, write and the read-back on [0, 3), then on [1, 3) (first = 1) of the state that leaves; member 0 is
    untouched by the second round"""
    wantA, wantB = w.oflow()
    bank = w.new_bank(M, config=cfg)
    sid = (w.max_addr, w.ws, cfg)

    def round_(first, n, rd, wr, wct, want, outside):
        ar, aw = [w.addrs[j] for j in rd], [w.addrs[j] for j in wr]
        snaps = {m: snapshot(w, bank, m) for m in outside}

        def untouched(what):
            for m, s in snaps.items():
                assert_untouched(w, bank, m, s, (sid, what))

        got, prof = profiled(bank, lambda: bank.read(ar, w.keys, first=first), CLASSES)
        show(w, f"{cfg} read [{first},{first + n})", prof)
        for k in range(n):
            same(got[k], want["read"][k], (sid, "read", "member", first + k))
        check_rows_profile(w, cfg, n, "read", prof)
        untouched("read")
        got, prof = profiled(bank, lambda: bank.read_prepare_write(aw, w.keys, first=first), CLASSES)
        show(w, f"{cfg} read_prepare_write [{first},{first + n})", prof)
        for k in range(n):
            same(got[k], want["rpw"][k], (sid, "read_prepare_write", "member", first + k))
            assert bank.state(first + k) is True
            if w.n2 == 2:
                same(bank.tree(first + k, 0), want["tree_after_rpw"][k], (sid, "tree after read_prepare_write", "member", first + k))
        check_rows_profile(w, cfg, n, "rpw", prof)
        untouched("read_prepare_write")
        _, prof = profiled(bank, lambda: bank.write(wct, aw, w.keys, first=first), CLASSES)
        show(w, f"{cfg} write [{first},{first + n})", prof)
        for k in range(n):
            same(bank.store_encrypted(first + k), want["rows_after_write"][k], (sid, "rows after write", "member", first + k))
            assert bank.state(first + k) is False
            if w.n2 == 2:
                same(bank.tree(first + k, 0), want["tree_after_write"][k], (sid, "tree after write", "member", first + k))
        check_rows_profile(w, cfg, n, "write", prof)
        untouched("write")
        got, prof = profiled(bank, lambda: bank.read(aw, w.keys, first=first), CLASSES)
        for k in range(n):
            same(got[k], want["read_back"][k], (sid, "read-back", "member", first + k))
        check_rows_profile(w, cfg, n, "read", prof)
        untouched("read-back")
        return got

    for m in range(M):   # (the whole range's reads are reads of the rows as loaded)
        same(wantA["read"][m], w.oread(m, RD[m]), "oracle")
    back = round_(0, M, RD, WR, w.wordsA[1], wantA, [])
    data = [d.copy() for d in w.data]
    for m in range(M):
        data[m][w.ws * w.idx[WR[m]]: w.ws * (w.idx[WR[m]] + 1)] = w.wordsA[0][m]
    w.check_word(back[0], data[0], WR[0], written=True)          # the value, and the noise bound: once per shape and configuration
    back = round_(1, 2, RD2, WR2, w.wordsB[1], wantB, [0])
    data[2][w.ws * w.idx[WR2[1]]: w.ws * (w.idx[WR2[1]] + 1)] = w.wordsB[0][1]
    w.check_word(back[1], data[2], WR2[1], written=True)
    ro = bank.roundoff_max()
    print(f"{sid}: round-off {ro:.6g}")
    assert ro < 3 / 8


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
def test_read_batch(w, cfg):
    """three addresses, the first and the last of the RAM among them, on member 0's rows"""
    ram = w.new_ram(0, config=cfg)
    ram.profile_enable(True)
    ram.profile_reset()
    got = ram.read_batch([w.addrs[j] for j in BATCH], w.keys)
    prof = {c: ram.profile_get(c) for c in CLASSES}
    ram.profile_enable(False)
    show(w, f"{cfg} read_batch", prof)
    assert w.idx[BATCH[0]] == 0 and w.idx[BATCH[1]] == w.max_addr - 1
    for k, j in enumerate(BATCH):
        same(got[k], w.oread(0, j), ((w.max_addr, w.ws, cfg), "read_batch", "address", k))
    w.check_word(got[1], w.data[0], BATCH[1])
    assert np.array_equal(ram.store_encrypted(), w.rows[0]) and not ram.state
    assert ram.roundoff_max() < 3 / 8


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
def test_read_list(w, cfg):
    """[2, 0, 0, 1] at four different addresses: every entry against the oracle's read of that member at that address"""
    bank = w.new_bank(M, config=cfg)
    snaps = [snapshot(w, bank, m) for m in range(M)]
    got, prof = profiled(bank, lambda: bank.read_list(LIST_MEMBERS, [w.addrs[j] for j in LIST_ADDRS], w.keys), CLASSES)
    show(w, f"{cfg} read_list {LIST_MEMBERS}", prof)
    for k, (m, j) in enumerate(zip(LIST_MEMBERS, LIST_ADDRS)):
        same(got[k], w.oread(m, j), ((w.max_addr, w.ws, cfg), "read_list", "entry", k, "member", m))
    check_rows_profile(w, cfg, len(LIST_MEMBERS), "read", prof)
    w.check_word(got[0], w.data[2], LIST_ADDRS[0])
    for m in range(M):
        assert_untouched(w, bank, m, snaps[m], "after the list")
    assert bank.roundoff_max() < 3 / 8


def got_digits(addr):
    addr._digits = None   # (always from the device)
    return np.stack(addr.digits)


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
def test_derive_and_read_through_the_derived_addresses(w, cfg):
    """K = 3 integers in one k_cmux_chain launch under this shape's plan (at most 8 digits in every shape here), against the oracle's
    address_from_fheuint; then the same derivation on a bank, and a range read through the three derived addresses"""
    pkg = w.pkg
    values, bits, digits, reads = w.derived()
    assert w.n_digits <= 8
    ram = pkg.Ram(w.params, 0, config=cfg)
    ram.profile_enable(True)
    ram.profile_reset()
    addrs = ram.derive_addresses([pkg.FheUintPrepared.from_host(ram, b) for b in bits])
    prof = ram.profile_get("derive")
    ram.profile_enable(False)
    assert prof["launches"] == 1 and prof["blocks"] == 3 * w.n_digits * 6, prof
    for k, a in enumerate(addrs):
        same(got_digits(a), digits[k], ((w.max_addr, w.ws, cfg), "derived digits of", values[k]))
    assert ram.roundoff_max() < 3 / 8
    bank = w.new_bank(M, config=cfg)
    baddrs = bank.derive_addresses([pkg.FheUintPrepared.from_host(bank, b) for b in bits])
    got = bank.read(baddrs, w.keys)
    for m in range(M):
        same(got[m], reads[m], ((w.max_addr, w.ws, cfg), "read through the address derived from", values[m], "member", m))
    for i in range(w.ws):   # the value (a derived address is noisier than an encrypted one: the comparison above is the check)
        want = w.o.expected_plain(int(w.data[1][i + w.ws * values[1]]), w.o.p.k_glwe_pt)
        assert w.o.glwe_decrypt(got[1][i], want, w.sk)[0] == want, i
    assert bank.roundoff_max() < 3 / 8


def test_a_nine_digit_plan_is_refused_and_the_address_keeps_its_digits(po):
    """fheram_address_derive takes plans of at most 8 digits (the argument struct of k_cmux_chain): FHERAM_ERR_UNSUPPORTED, and the address
    named in the call keeps the digits it had.  (test_gpu_derive.py::test_refusals_change_nothing has no plan of more than 8 digits.)"""
    pkg = load_package()
    plan, max_addr = [2, 2, 2, 1, 1, 1, 1, 1, 1], 1 << 12
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=1, decomp_n=plan))
    sk = o.secret_gen(41)
    params = pkg.Parameters(max_addr=max_addr, word_size=1, decomp_n=plan)
    assert params.base2d().as_1d().size() == 9
    ram = pkg.Ram(params, 0)
    before = o.address_encrypt(777, sk, 42, 43)
    a = pkg.Address(params, list(before))
    a._device(ram)
    fu = pkg.FheUintPrepared.from_host(ram, o.fheuint_encrypt(1234, 12, sk, 44, 45))
    with pytest.raises(pkg.FheRamError) as e:
        ram.derive_addresses([fu], [a])
    assert e.value.code == ST_UNSUPPORTED and "8 digits" in e.value.msg, (e.value.code, e.value.msg)
    assert np.array_equal(got_digits(a), before)
    blank = pkg.Address.alloc(ram)
    with pytest.raises(pkg.FheRamError) as e:
        ram.derive_addresses([fu], [blank])
    assert e.value.code == ST_UNSUPPORTED
    with pytest.raises(pkg.FheRamError):   # still empty
        blank.digits
    assert np.array_equal(got_digits(pkg.Address.set_from_fheuint(ram, fu, sign=False)), o.address_from_fheuint(fu.download(), sign=False))

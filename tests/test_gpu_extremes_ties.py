"""Rounding ties THROUGH the chain kernels.  tests/test_gpu_limb_forms.py drives the scalar limb forms (csrc/limb_forms.hpp) over
directed inputs one coefficient at a time; here the same sharp inputs reach them inside k_read_chain, k_write_chain, the mid
chain and the tail.  Kind `tie_mono`: every key, address-digit and trace-key polynomial is -2^16 * X^0, rows and written words
are pseudo-random normalised limbs.  Then every un-normalised limb of every product is a multiple of 2^16 (at most 6 * 2^32 in
magnitude), and about half of all coefficients sit on a rounding tie of carry = floor(v / 2^17 + 1/2) in the lowest limb and
in the extra carry e of the closed-form normalisation — where round-half-even in place of round-half-up, a dropped inner
carry or a wrong window constant shows.  On pseudo-random operands one carry lands on a tie with probability 2^-17.
Read, read_prepare_write, write, store and read-back against the oracle (exact integers); flow and oracle helpers:
tests/test_gpu_extremes.py.  The inputs are not valid ciphertexts: nothing decrypts, everything compares."""
import numpy as np
import pytest

from _pkg import load_package
from test_gpu_extremes import LO, HI, N, _oracle_flow, _threads

pytestmark = pytest.mark.gpu

FUSED = {"limb_split": 0, "fine_split": 0, "chain": 1, "nco": 2}      # one workgroup per ciphertext: the fused row chains
LAUNCHES = ("read_chain_launch", "write_chain_launch", "keyswitch_chain_launch", "keyswitch_mid_launch", "ext_product_mid_launch", "keyswitch_tail_launch")


def _fill(kind, shape, rng):
    n = int(np.prod(shape))
    if kind == "tie_mono":
        a = np.zeros(n, dtype=np.int64)
        a[::N] = LO                          # -2^16 * X^0, every polynomial
    elif kind == "random":
        a = rng.integers(LO, HI + 1, n, dtype=np.int64)
    else:
        raise ValueError(kind)
    return a.reshape(shape)


def tie_share(rows, addr_digit, sg=4):
    """the share of coefficients of the flow's first product (the rows with the GGSW of the first address digit) whose lowest
    big limb is an odd multiple of 2^16.  The GGSW's polynomials are constants c * X^0, so the product is coefficient-wise."""
    g = np.asarray(addr_digit, dtype=np.int64).reshape(6, sg, 2, N)           # [digit r, column cin][limb][column][N]
    assert not g[..., 1:].any()
    x = np.asarray(rows, dtype=np.int64).reshape(-1, 6, N)                      # [ciphertext][limb r, column cin][N]
    big = np.einsum("ckn,ko->con", x, g[:, sg - 1, :, 0])                       # lowest limb, both columns
    assert np.abs(big).max() <= 6 << 32 and not (big % (1 << 16)).any()
    return float(np.mean((big >> 16) & 1))


@pytest.mark.parametrize("log_max_addr", [14, 16])
def test_rounding_ties_through_the_chain_kernels(po, log_max_addr):
    """2^14 x 2 B (8 ciphertexts a round: the tail) and 2^16 x 2 B (32: the mid chain, and the tail behind it), the smallest shapes at
    which those launches run; the default form, the limb-form chains (chain_y = 0) and — so few ciphertexts are split over the chip by
    default — the one-workgroup-per-ciphertext form forced (as tests/test_gpu_write_rotate_fused.py does), in which k_read_chain and
    k_write_chain take both chains of every row."""
    pkg = load_package()
    max_addr, ws = 1 << log_max_addr, 2
    rng = np.random.default_rng(4200 + log_max_addr)
    p = pkg.Parameters(max_addr=max_addr, decomp_n=[3, 3, 3, 3], word_size=ws)
    n_digits = p.base2d().as_1d().size()
    inp = {"atk": _fill("tie_mono", (12, 3 * 4 * 2 * N), rng), "atk_inv": _fill("tie_mono", 4 * 5 * 2 * N, rng), "tsk": _fill("tie_mono", 4 * 5 * 2 * N, rng),
           "addr": _fill("tie_mono", (n_digits, p.ggsw_len()), rng), "rows": _fill("random", (ws, max_addr // N, p.glwe_len()), rng),
           "words": _fill("random", (ws, p.glwe_len()), rng)}
    share = tie_share(inp["rows"], inp["addr"][0])
    print(f"ties 2^{log_max_addr}: share of coefficients on a tie in the lowest limb of the first product {share:.4f}")
    assert share >= 0.25                      # random rows give 1/2: the pattern has not degenerated
    want = _oracle_flow(po, max_addr, ws, inp, _threads())      # asserts max_big < 2^47 (here <= 6 * 2^32 by construction)
    for cfg in ({"monitor": 2}, {"monitor": 2, "chain_y": 0}, dict(FUSED, monitor=2)):
        ram = pkg.Ram(p, config=cfg)
        keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(inp["atk"]), inp["atk_inv"], inp["tsk"])
        addr = pkg.Address(p, list(inp["addr"]))
        ram.load_encrypted(inp["rows"])
        ram.profile_enable(True)
        ram.profile_reset()
        got = {"read": ram.read(addr, keys), "rpw": ram.read_prepare_write(addr, keys)}
        ram.write(inp["words"], addr, keys)
        got["rows_after_write"] = ram.store_encrypted()
        got["read_back"] = ram.read(addr, keys)
        ram.profile_enable(False)
        for k in ("read", "rpw", "rows_after_write", "read_back"):
            bad = np.count_nonzero(np.asarray(got[k]) != np.asarray(want[k]))
            assert bad == 0, (cfg, k, bad)
        ro = ram.roundoff_max()               # raises PRECISION above the monitor's limit
        assert ro <= 0.25, (cfg, ro)
        ran = {k: ram.profile_get(k)["launches"] for k in LAUNCHES}
        t, m = ram.tail_stats(), ram.mid_stats()
        print(f"ties 2^{log_max_addr} {cfg}: round-off {ro:.4g} launches {ran} tail {t} mid {m}")
        assert t["fallbacks"] == 0 and m["fallbacks"] == 0
        _assert_kernels_ran(cfg, log_max_addr, ran, t, m)
        del ram


def _assert_kernels_ran(cfg, log_max_addr, ran, t, m):
    """which launches the flow took (csrc/launch.hpp chain_form): 3 reads (read, read_prepare_write, read-back) and 1 write"""
    assert t["launches"] == ran["keyswitch_tail_launch"] and m["launches"] == ran["keyswitch_mid_launch"] + ran["ext_product_mid_launch"], (ran, t, m)
    if cfg.get("limb_split") == 0:
        assert ran["read_chain_launch"] >= 3 and ran["write_chain_launch"] >= 1, ran     # k_read_chain / k_write_chain: both chains of every row
        assert t["launches"] == 0 and m["launches"] == 0, (t, m)
    else:                                                                                # (chain_y = 0 changes the steps' form, not which chains hand over in one launch)
        assert ran["read_chain_launch"] == 0 and ran["write_chain_launch"] == 0, ran
        assert t["launches"] >= 3, t                                                     # k_trace_tail ends every read
        assert (m["launches"] >= 3) if log_max_addr == 16 else (m["launches"] == 0), m   # 32 ciphertexts: k_chain_mid; 8: none

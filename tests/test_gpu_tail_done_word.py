"""The host's wait at the end of a read-type operation ends on the done word of k_trace_tail (csrc/tail_wait.hpp, fheram_sync) instead of
on the end of that kernel and of the predicated fallback launch behind it.  Whatever the wait ends on, what the host then downloads is the
oracle's result, bit for bit: on the first call of a context, after a hundred more (the words hold the launch's generation: the comparison
must not be fooled by an older one), when the tail gives up (the host must fall through to the stream wait: the fallback does the work),
and whatever the bound of the poll (FHERAM_TAIL_POLL_US: 0 = one look, -1 = never look).
Shapes: 2^12 x 4 B (one row: the final trace is the only tail launch) and 2^13 x 4 B (two rows: the alone packer levels are a tail launch
too, so the armed generation is not the operation's first), the sizes test_gpu_parity.py uses for the tail."""
import numpy as np
import pytest

from test_gpu_parity import World

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[12, 13], ids=lambda k: f"2^{k}")
def world(po, request):
    """one RAM per shape and the oracle's results, computed once: read, read_prepare_write, rows after the write, read-back"""
    w = World(po, 1 << request.param, word_size=4, seed=70 + request.param)
    o = w.o
    oram = o.ram_new()
    oram.load(w.rows)
    w.wct = np.stack([o.glwe_encrypt_coeff0(17 + i, w.sk, 900 + i, 950 + i) for i in range(4)])
    w.want = {"read": oram.read(w.oaddr, w.okeys), "rpw": oram.read_prepare_write(w.oaddr, w.okeys)}
    oram.write(w.wct, w.oaddr, w.okeys)
    w.want["rows"] = oram.store()
    w.want["back"] = oram.read(w.oaddr, w.okeys)
    return w


def _ram(w, config=None):
    ram = w.pkg.Ram(w.ram.params, config=config) if config else w.pkg.Ram(w.ram.params)
    ram.load_encrypted(w.rows)
    return ram, w.pkg.Address(ram.params, list(w.addr_g))


def _step(w, ram, addr):
    """read / read_prepare_write / write / read, the host waiting with sync() after each call and fetching the result afterwards"""
    ram.read(addr, w.keys, download=False)
    ram.sync()
    assert np.array_equal(ram.result(), w.want["read"]), "read"
    ram.read_prepare_write(addr, w.keys, download=False)
    ram.sync()
    assert np.array_equal(ram.result(), w.want["rpw"]), "read_prepare_write"
    ram.write(w.wct, addr, w.keys)
    ram.sync()
    assert np.array_equal(ram.store_encrypted(), w.want["rows"]), "rows after the write"
    ram.read(addr, w.keys, download=False)
    ram.sync()
    assert np.array_equal(ram.result(), w.want["back"]), "read-back"


def test_first_call_and_after_a_hundred(world):
    w = world
    ram, addr = _ram(w)
    ram.read(addr, w.keys, download=False)          # the context's first launch of the tail: the words still hold 0
    ram.sync()
    assert np.array_equal(ram.result(), w.want["read"])
    for _ in range(100):
        ram.read(addr, w.keys, download=False)
        ram.sync()
    assert np.array_equal(ram.result(), w.want["read"])
    ram.sync()                                      # nothing armed any more: the plain stream wait
    _step(w, ram, addr)
    t = ram.tail_stats()
    assert t["launches"] >= 104 and t["fallbacks"] == 0, t


def test_forced_give_up_falls_through_to_the_stream_wait(world):
    w = world
    ram, addr = _ram(w, {"tail_test": 1})           # every tail launch gives up two steps before its end
    _step(w, ram, addr)
    t = ram.tail_stats()
    assert t["launches"] > 0 and t["fallbacks"] == t["launches"], t
    # and a context that gave up does not poison the next one's words
    ram2, addr2 = _ram(w)
    _step(w, ram2, addr2)


@pytest.mark.parametrize("bound", ["0", "-1", "5"])
def test_any_poll_bound_gives_the_same_answers(world, monkeypatch, bound):
    """0: one look and then the stream wait; -1: never look; 5 us: the bound runs out long before the operation ends"""
    w = world
    monkeypatch.setenv("FHERAM_TAIL_POLL_US", bound)
    ram, addr = _ram(w)
    _step(w, ram, addr)
    assert ram.tail_stats()["fallbacks"] == 0

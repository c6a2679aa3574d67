"""Every transform form the kernels call (csrc/fft_dev.hpp), on the device, under its call sites' own buffer discipline:
fheram_selftest_forms (csrc/selftest_forms.hip) runs ntt_fwd<1 | 2 | 3> and then, in ONE workgroup, K batches of two accumulated
products through one inverse form — the barrier-fenced pair and single that tests/test_gpu_fft.py already pins, the unfenced
single on alternating buffers and behind a forward transform, the singles and pairs fenced by the free counter in LDS, the two
hooked forms with the next batch's multiply-accumulates and operand loads between their phases, and the five-limb unit sequence
that mixes both hooked forms.  Raw doubles come back, so the round-off itself is visible, not only rint(x).

All forms run the same three passes on a polynomial and the library is built with -ffp-contract=off: for the same operands every
form must return the SAME doubles.  The form pinned against exact integers is therefore an exact reference for the others;
a difference is a bug in that form or a race in its buffers, never a tolerance question.  The bounds against exact integers are
the ones tests/test_gpu_fft.py pins for the same patterns (2^-8 uniform, 0.2 constant, [0.2, 0.3] searched worst pattern).

Largest raw round-off per pattern, measured on an MI355X, the same for every form and every ntt_fwd<B> by the bit-identity test:
uniform 0.00042724609375, every coefficient -2^16 0.125, searched worst pattern 0.25, uniform with two terms 0.000244140625,
three different batches 0.00042724609375."""
import os

import numpy as np
import pytest

from _pkg import load_package

pytestmark = pytest.mark.gpu
N = 4096
LO, HI = -(1 << 16), (1 << 16) - 1

# inverse forms (include/fheram.h, csrc/selftest_forms.hpp: SelftestForm)
FORMS = ["skew<1,1>", "skew<2,1>", "skew<1,0> alternating", "skew<1,0> behind fwd", "skew<1,2>", "skew<2,2>", "inv1_hooked<2>", "inv2_hooked<2>",
         "five-limb units"]
FORM_IDS = ["skew11", "skew21", "skew10_alt", "skew10_fwd", "skew12", "skew22", "hooked1", "hooked2", "units5"]
REF_FORM = 0
# The coefficient class (j // 512) that the default monitor (mode 1) samples at each rounding site: the compile-time SEL of
# fft_dev.hpp — fft_inv_skew's first and second polynomial, fft_inv1_hooked's MSEL, fft_inv2_hooked's MSEL and (MSEL + 3) % 8.
# Classes 2 and 7 are sampled nowhere.  include/fheram.h (FHERAM_ERR_PRECISION) and DESIGN.md §2 give the same table: a change of the
# sampling changes all three together.
SITE_SEL = {"skew": (0, 3), "hooked1": (5,), "hooked2": (1, 4)}


def sampled_class(form, batch, which):
    """class sampled for output `which` (0 | 1) of `batch` by form `form`"""
    if form in (0, 2, 3, 4):                      # one polynomial per call: always the site's first
        return SITE_SEL["skew"][0]
    if form in (1, 5):
        return SITE_SEL["skew"][which]
    if form == 6 or (form == 8 and batch % 3 == 2):
        return SITE_SEL["hooked1"][0]
    return SITE_SEL["hooked2"][which]


def exact_sums(a, g):
    """[2][N] int64: sum_r a_r * g_r and sum_r a_r * g_{r ^ 1} mod X^N + 1; np.convolve on int64 is direct and exact (|sum| < 2^47)"""
    a, g = a.astype(np.int64), g.astype(np.int64)
    out = np.zeros((2, N), dtype=np.int64)
    for b in range(2):
        for r in range(a.shape[0]):
            full = np.convolve(a[r], g[r ^ b])
            out[b, :N] += full[:N]
            out[b, :N - 1] -= full[N:]
    return out


def _worst():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft_worst_pattern.bin")
    bits = np.unpackbits(np.fromfile(path, dtype=np.uint8), bitorder="little")
    assert bits.size == 12 * N
    v = np.where(bits.reshape(12, N) == 1, HI, LO).astype(np.int64)
    return v[:6], v[6:]


@pytest.fixture(scope="module")
def sets():
    """name -> (a [K][R][N], g, exact [K][2][N], lower bound, upper bound of max |raw - exact|): computed once, never changed"""
    rng = np.random.default_rng(20)
    ua, ug = rng.integers(LO, HI + 1, (6, N)), rng.integers(LO, HI + 1, (6, N))
    const = np.full((6, N), LO, dtype=np.int64)
    wa, wg = _worst()
    rot = np.roll(np.arange(6), 1)
    s = {
        "uniform": ([ua], [ug], 0.0, 2.0 ** -8),
        "constant": ([const], [const], 0.0, 0.2),
        "worst": ([wa], [wg], 0.2, 0.3),
        "uniform R=2": ([ua[:2]], [ug[:2]], 0.0, 2.0 ** -8),
        # three different batches: the term order rotated (another pairing of out[1], another order of accumulation), one negated
        "three batches": ([ua, ua[rot], -ua[rot[rot]]], [ug, ug[rot], ug[rot[rot]]], 0.0, 2.0 ** -8),
    }
    out = {}
    for name, (a, g, lo, hi) in s.items():
        a, g = np.stack(a).astype(np.int32), np.stack(g).astype(np.int32)
        want = np.stack([exact_sums(a[i], g[i]) for i in range(a.shape[0])])
        for v in (a, g, want):
            v.setflags(write=False)
        out[name] = (a, g, want, lo, hi)
    return out


SET_NAMES = ["uniform", "constant", "worst", "uniform R=2", "three batches"]


@pytest.fixture(scope="module")
def ram():
    pkg = load_package()
    return pkg.Ram.new_from_ram_params(4, [3, 3, 3, 3], 4096)        # monitor = 1, the default


@pytest.fixture(scope="module")
def ram_all():
    pkg = load_package()
    r = pkg.Ram(pkg.Parameters(max_addr=4096, decomp_n=[3, 3, 3, 3], word_size=4), config={"monitor": 2})
    assert r.forms()["monitor"] == 2
    return r


@pytest.fixture(scope="module")
def ref_raw(ram, sets):
    """raw output of the pinned form (fft_inv_skew<1, 1> behind ntt_fwd<1>) and the forward launch's spectra, per operand set"""
    return {name: ram.selftest_forms(a, g, REF_FORM, fwd_polys=1, spectra=True) for name, (a, g, _, _, _) in sets.items()}


def test_reference_is_the_suites_exact_convolution(sets):
    from test_gpu_fft import exact_negacyclic
    a, g, want, _, _ = sets["uniform R=2"]
    assert np.array_equal(want[0][0], exact_negacyclic(a[0], g[0]))
    assert np.array_equal(want[0][1], exact_negacyclic(a[0], g[0][::-1]))


# ---- 1. raw sums against exact integers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
def test_raw_sums_are_within_the_pinned_bounds_of_the_exact_integers(ram, sets, form, name):
    a, g, want, lo, hi = sets[name]
    for fwd in (1, 2, 3):
        raw = ram.selftest_forms(a, g, form, fwd_polys=fwd)
        err = np.abs(raw - want).max()
        print(f"{FORMS[form]} ntt_fwd<{fwd}> {name}: max |raw - exact| = {err!r}")
        assert lo <= err <= hi, (FORMS[form], fwd, name, err)
        assert np.array_equal(np.rint(raw).astype(np.int64), want), (FORMS[form], fwd, name)


# ---- 2. bit-identity across forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
def test_every_form_returns_the_doubles_of_the_pinned_form(ram, sets, ref_raw, form, name):
    a, g = sets[name][:2]
    for fwd in (1, 2, 3):
        raw = ram.selftest_forms(a, g, form, fwd_polys=fwd)
        assert np.array_equal(raw, ref_raw[name][0]), (FORMS[form], fwd, name, np.abs(raw - ref_raw[name][0]).max())


@pytest.mark.parametrize("name", SET_NAMES)
def test_forward_spectra_do_not_depend_on_how_many_run_together(ram, sets, ref_raw, name):
    a, g = sets[name][:2]
    for fwd in (2, 3):
        sp = ram.selftest_forms(a, g, REF_FORM, fwd_polys=fwd, spectra=True)[1]
        assert np.array_equal(sp, ref_raw[name][1]), (fwd, name)
    assert np.abs(ref_raw[name][1]).max() > 0.0


@pytest.mark.parametrize("name", ["uniform", "worst", "uniform R=2"])
def test_one_batch_is_the_convolve_selftest_bit_for_bit(ram, sets, name):
    a, g = sets[name][:2]
    assert np.array_equal(ram.selftest_forms(a, g, 1)[0], ram.selftest_convolve(a[0], g[0]))
    assert np.array_equal(ram.selftest_forms(a, g, 0, fwd_polys=1)[0], ram.selftest_convolve(a[0], g[0], singles=True))


# ---- 3. buffer reuse ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fwd", [2, 3])
@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
def test_batches_in_the_same_buffers_do_not_disturb_each_other(ram, sets, ref_raw, form, fwd):
    a, g = sets["worst"][:2]
    same = ram.selftest_forms(np.repeat(a, 4, axis=0), np.repeat(g, 4, axis=0), form, fwd_polys=fwd)
    for i in range(4):
        assert np.array_equal(same[i], ref_raw["worst"][0][0]), (FORMS[form], i)
    # four different batches: each is what the same form returns for it alone
    names = ["uniform", "constant", "worst"]
    a4 = np.concatenate([sets[n][0] for n in names] + [sets["three batches"][0][2:3]])
    g4 = np.concatenate([sets[n][1] for n in names] + [sets["three batches"][1][2:3]])
    mixed = ram.selftest_forms(a4, g4, form, fwd_polys=fwd)
    for i in range(4):
        alone = ram.selftest_forms(a4[i:i + 1], g4[i:i + 1], form, fwd_polys=fwd)
        assert np.array_equal(mixed[i], alone[0]), (FORMS[form], i)
        assert np.array_equal(np.rint(mixed[i]), np.rint(ref_raw[names[i]][0][0] if i < 3 else ref_raw["three batches"][0][2])), (FORMS[form], i)


# ---- 4. and 5. the round-off monitor at every rounding site ----------------------------------------------------------------------------
def _plant(batch, which, j):
    """operands whose sum `which` of batch `batch` is 1 at coefficient j and 0 elsewhere: 1/2 under operand_scale = 0.5"""
    a = np.zeros((batch + 1, 2, N), dtype=np.int32)
    g = np.zeros((batch + 1, 2, N), dtype=np.int32)
    a[batch, 0, 0] = 1
    g[batch, which, j] = 1
    return a, g


def _plants():
    for batch in (0, 2):                 # (batch 2 of the five-limb units is the pair of single transforms)
        for which in (0, 1):
            for k in range(8):
                yield batch, which, k, 512 * k + 64 * k + 5      # one coefficient per class, on different waves


@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
def test_full_monitor_reports_the_raw_roundoff_of_every_form(ram_all, sets, form):
    a, g, want, _, _ = sets["constant"]
    ram_all.roundoff_reset()
    raw = ram_all.selftest_forms(a, g, form)
    assert ram_all.roundoff_max() == 0.0                          # raw runs report nothing
    rounded = ram_all.selftest_forms(a, g, form, rounded=True)
    assert np.array_equal(rounded.astype(np.int64), want)
    ro = ram_all.roundoff_max()
    assert ro == np.abs(raw - np.rint(raw)).max(), (FORMS[form], ro)
    assert 0.05 < ro <= 0.2
    ram_all.roundoff_reset()


@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
def test_full_monitor_sees_a_half_integer_in_every_class_of_both_outputs(ram_all, form):
    pkg = load_package()
    for batch, which, k, j in _plants():
        a, g = _plant(batch, which, j)
        ram_all.roundoff_reset()
        with pytest.raises(pkg.FheRamError) as e:
            ram_all.selftest_forms(a, g, form, rounded=True, operand_scale=0.5)
        assert e.value.code == 8, (FORMS[form], batch, which, k)
        assert 0.49 < ram_all.roundoff_max(check=False) <= 0.5, (FORMS[form], batch, which, k)
    ram_all.roundoff_reset()
    ram_all.sync()


@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
def test_default_monitor_sees_exactly_the_class_its_site_samples(ram, form):
    """mode 1 observes ONE class per rounding site (SITE_SEL).  Every other coefficient of the planted sums is 0 up to the round-off of
    transforms of unit operands (a few 2^-52), so a plant outside the sampled class leaves the maximum below 2^-30."""
    pkg = load_package()
    assert ram.forms()["monitor"] == 1
    for batch, which, k, j in _plants():
        a, g = _plant(batch, which, j)
        ram.roundoff_reset()
        if k == sampled_class(form, batch, which):
            with pytest.raises(pkg.FheRamError) as e:
                ram.selftest_forms(a, g, form, rounded=True, operand_scale=0.5)
            assert e.value.code == 8, (FORMS[form], batch, which, k)
            assert 0.49 < ram.roundoff_max(check=False) <= 0.5, (FORMS[form], batch, which, k)
        else:
            out = ram.selftest_forms(a, g, form, rounded=True, operand_scale=0.5)
            assert np.abs(out).max() <= 1.0
            assert ram.roundoff_max() < 2.0 ** -30, (FORMS[form], batch, which, k)
    ram.roundoff_reset()
    ram.sync()

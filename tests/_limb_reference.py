"""Exact-integer reference of the limb forms (fhe-ram_amd/csrc/limb_forms.hpp, limb_forms_eval.hpp) and the inputs the limb
tests run: pure Python and numpy int64, no float arithmetic, no oracle, none of the float restatements of test_oracle.py.

  limb walk        vec_znx_big_normalize on one coefficient: from the least significant limb, c = (v + 2^16) // 2^17,
                   d = v - c * 2^17, the carry out of limb 0 dropped
  balanced digits  of an integer modulo 2^51: the three digits in [-2^16, 2^16)
  rsh(1)           as oracle/znx.hpp rsh_inplace defines it (shift by one limb, then a normalisation shifted by 16 bits)

`cases(form)` returns (inputs [n][LF_IN] float64, expected [n][LF_OUT] int64, number of outputs the form produces): 2^16
random coefficients, a directed grid (a Cartesian product over the limbs of per-limb edge sets, at most 9^5 coefficients
each) and solved cases that put V on the window's edges, on the largest |V| the documented bounds allow, on a second
quotient of +-2^16 and on coincident ties.  The preconditions of the contract are asserted for every generated input:
|big limb| < 2^47, |V| < 2^53 (and |V| + C < 2^53, which is what makes window51's fma exact), every cmux carry below 2^31,
every integer that travels as a double below 2^53.  No case is dropped."""
import functools
import itertools

import numpy as np

LF_IN, LF_OUT = 10, 6
(NORM3, NORM4, RSH1_3, Y_OF, DIGITS3, DIGITS3_WRAPPED, CLOSED4, CLOSED5, WRITE_POST, PAIR_SUM, PAIR_DIFF, PAIR_OUT,
 CMUX_4_4, CMUX_5_4) = range(14)
FORMS = {"NORM3": NORM3, "NORM4": NORM4, "RSH1_3": RSH1_3, "Y_OF": Y_OF, "DIGITS3": DIGITS3, "DIGITS3_WRAPPED": DIGITS3_WRAPPED,
         "CLOSED4": CLOSED4, "CLOSED5": CLOSED5, "WRITE_POST": WRITE_POST, "PAIR_SUM": PAIR_SUM, "PAIR_DIFF": PAIR_DIFF,
         "PAIR_OUT": PAIR_OUT, "CMUX_4_4": CMUX_4_4, "CMUX_5_4": CMUX_5_4}

B = 17
HALF = 1 << 16
C = (1 << 16) + (1 << 33) + (1 << 50)      # the digit window of three balanced digits is [-C, 2^51 - C)
P51 = 1 << 51
BIG_BOUND = 1 << 47                        # |un-normalised limb| < 2^47 (6 * 4096 * 2^32: SURVEY.md A.9)
Y_BOUND = (1 << 50) + (1 << 33)            # |Y| < 2^50 + 2^33
N_RANDOM = 1 << 16
GRID_MAX = 9 ** 5


def i64(x):
    return np.asarray(x, dtype=np.int64)


# ---- the reference operations (exact integers; >> and // floor on int64) -------------------------------------------------
def carry(v):
    return (i64(v) + HALF) >> B


def cmod(v, bits):
    v = i64(v)
    return v - (((v + (1 << (bits - 1))) >> bits) << bits)


def walk(v, n_out=None):
    """v [n][S] limbs, most significant first -> the n_out most significant digits of the walk [n][n_out]"""
    v = i64(v)
    s = v.shape[1]
    n_out = s if n_out is None else n_out
    out = np.zeros((v.shape[0], n_out), dtype=np.int64)
    c = np.zeros(v.shape[0], dtype=np.int64)
    for j in range(s - 1, -1, -1):
        t = v[:, j] + c
        c = carry(t)
        if j < n_out:
            out[:, j] = t - (c << B)
    return out


def whole(d):
    """[n][3] limbs -> the integer they stand for"""
    d = i64(d)
    return (d[:, 0] << (2 * B)) + (d[:, 1] << B) + d[:, 2]


def digits_quotient(a):
    """the two low balanced digits of a and the second quotient as the top one [n][3]"""
    a = i64(a)
    d2 = cmod(a, B)
    q = (a - d2) >> B
    d1 = cmod(q, B)
    return np.stack([(q - d1) >> B, d1, d2], axis=1)


def digits51(a):
    """the balanced digits of a modulo 2^51 [n][3]"""
    d = digits_quotient(a)
    d[:, 0] = cmod(d[:, 0], B)
    return d


def ceil_half(a):
    return (i64(a) + 1) >> 1


def rsh1(x):
    """oracle/znx.hpp rsh_inplace(base2k = 17, k = 1) on [n][S] limbs: lsh = 16, digits of one bit"""
    x = i64(x)
    s = x.shape[1]
    y = np.zeros_like(x)
    d = -(x[:, s - 1] & 1)                     # get_digit(1, x): 0 or -1
    c = (x[:, s - 1] - d) >> 1
    for j in range(s - 1, 0, -1):
        src = x[:, j - 1]
        d = -(src & 1)
        cr = (src - d) >> 1
        dpc = (d << 16) + c
        y[:, j] = cmod(dpc, B)
        c = cr + ((dpc - y[:, j]) >> B)
    y[:, 0] = cmod(c, B)
    return y


# ---- preconditions ----------------------------------------------------------------------------------------------------
def _require(cond, what):
    assert bool(np.all(cond)), "precondition of the limb contract violated by a generated input: " + what


def closed_v(start, acc):
    """V of the closed form: start + e + acc_2 + cmod34(acc_1) 2^17 + cmod17(acc_0) 2^34; acc [n][SK]"""
    acc = i64(acc)
    e = np.zeros(acc.shape[0], dtype=np.int64)
    for j in range(acc.shape[1] - 1, 2, -1):
        e = carry(acc[:, j] + e)
    return i64(start) + e + acc[:, 2] + (cmod(acc[:, 1], 2 * B) << B) + (cmod(acc[:, 0], B) << (2 * B))


# ---- edge sets ------------------------------------------------------------------------------------------------------------
BIG_A = [0, 1, -1, HALF, -HALF, HALF - 1, -(HALF - 1), BIG_BOUND - 1, -(BIG_BOUND - 1)]
# odd and even multiples of 2^16 up to 2^46, and values = 2^16 - 1 (mod 2^17) that turn a carry-in of 1 into a ripple
BIG_B = [0, HALF, -HALF, 3 * HALF, 2 * HALF, (1 << 46) - HALF, -(1 << 46), 5 * (1 << B) + HALF - 1, -HALF - 1]
BIG_C = [HALF, HALF - 1, -HALF, -3 * HALF, (1 << 46) + HALF, -(1 << 46) + HALF - 1, (1 << 40) + HALF - 1, -(1 << 33), (1 << 33) - 1]
STORED = [-HALF, HALF - 1, HALF, 0, 1, -1]            # +2^16 is what a rotation's negation leaves
RSH_LIMBS = STORED + [2 * HALF, -2 * HALF, 2 * HALF - 1, -2 * HALF + 1, HALF + 1, -HALF - 1, 2]   # sums and differences reaching +-2^17
# one-double values: the window's edges, a second quotient of exactly +-2^16, ties in every digit
_Y_CORE = [0, HALF, -HALF, (1 << 33), -(1 << 33), (1 << 33) + HALF, (1 << 50), -(1 << 50), (1 << 50) + (1 << 33) - 1, -(1 << 50) - (1 << 33) + 1,
           (1 << 50) - (1 << 33) - HALF, -C, P51 - C, (1 << 50) - (1 << 33), (HALF - 1) << 34, -(HALF << 34) + (1 << 33), 3 * HALF + (3 << 33)]
Y_EDGES = sorted({v + d for v in _Y_CORE for d in (-2, -1, 0, 1, 2) if abs(v + d) < Y_BOUND})
WINDOW_EDGES = sorted({v + d for v in _Y_CORE + [P51 - C - 1] for d in (-2, -1, 0, 1, 2) if -C <= v + d < P51 - C})


def product(*sets):
    g = np.array(list(itertools.product(*sets)), dtype=np.int64)
    assert len(g) <= GRID_MAX
    return g


def cycle(values, n, stride=1):
    v = i64(values)
    return v[(np.arange(n) * stride) % len(v)]


def _rng(form):
    return np.random.default_rng(1000 + form)


def _big_random(rng, n, k):
    """random big limbs: full range, and a quarter of them multiples of 2^16 (ties)"""
    v = rng.integers(-BIG_BOUND + 1, BIG_BOUND, (n, k))
    t = rng.integers(-(1 << 30), 1 << 30, (n, k)) * HALF
    return np.where(rng.random((n, k)) < 0.25, t, v)


def _stored_random(rng, n, k):
    v = rng.integers(-HALF, HALF, (n, k))
    return np.where(rng.random((n, k)) < 0.1, HALF, v)


def _y_random(rng, n):
    return rng.integers(-Y_BOUND + 1, Y_BOUND, n)


def _window_random(rng, n):
    return rng.integers(-C, P51 - C, n)


# ---- solved cases of the closed form ---------------------------------------------------------------------------------------
def _closed_solved(sk):
    """rows (start, acc_0 .. acc_{sk-1}) whose V lands within +-2 of the window's edges and of the largest |V| allowed, starts whose
    second quotient is +-2^16, and coincident ties in every limb"""
    rows = []
    extras = [[0] * (sk - 3), [HALF] * (sk - 3), [HALF - 1] * (sk - 4) + [HALF], [-HALF - 1] * (sk - 3), [3 * HALF] + [0] * (sk - 4)]
    menus = [(-(1 << 50), 0, 0), (0, -HALF, 0), (0, 0, -(1 << 33)), ((1 << 50) - (1 << 34), 0, 0), (Y_BOUND - 1, HALF - 1, (1 << 33) - 1),
             (-(Y_BOUND - 1), -HALF, -(1 << 33)), (-(1 << 50), -HALF, 0), ((1 << 50), 0, (1 << 33) - 1), (0, HALF - 1, -(1 << 33)),
             (-(1 << 50), -HALF + (1 << 17), -(1 << 33) + (1 << 34))]      # the last one: acc_0, acc_1 outside the centred range (only the remainder counts)
    targets = [-C, P51 - C, -C - P51]
    for (y, a0, a1), ex, t, d in itertools.product(menus, extras, targets, (-2, -1, 0, 1, 2)):
        e = int(closed_v([0], [[0, 0, 0] + ex])[0])
        a2 = t + d - y - e - (int(cmod(a1, 2 * B)) << B) - (int(cmod(a0, B)) << (2 * B))
        if abs(a2) < BIG_BOUND:
            rows.append([y, a0, a1, a2] + ex)
    assert {t for t in targets} and len(rows) > 100
    # the largest |V| the documented bounds allow, both signs, with and without an extra carry
    for sg in (1, -1):
        for ex in ([sg * (BIG_BOUND - 1)] * (sk - 3), [0] * (sk - 3)):
            for d in (0, 1, 2):
                a0 = HALF - 1 if sg > 0 else -HALF
                a1 = (1 << 33) - 1 if sg > 0 else -(1 << 33)
                rows.append([sg * (Y_BOUND - 1 - d), a0, a1, sg * (BIG_BOUND - 1 - d)] + ex)
    # coincident ties: every limb's sum lands on 2^16 (mod 2^17) once the carry from below has come in
    for m in itertools.product((0, 1, -1, 2), repeat=sk):
        for y in (0, HALF - 1, (1 << 50) + 5):
            yd = [int(v) for v in digits51([y])[0]]
            acc, c = [0] * sk, 0
            for j in range(sk - 1, -1, -1):
                x = yd[j] if j < 3 else 0
                acc[j] = (m[j] << B) + HALF - c - x
                c = (acc[j] + x + c + HALF) >> B
            rows.append([y] + acc)
    rows = i64(rows)
    hit = closed_v(rows[:, 0], rows[:, 1:])
    for t in targets:                                  # the solved rows do land where they were aimed
        for d in (-2, -1, 0, 1, 2):
            assert np.any(hit == t + d), (t, d)
    return rows


# ---- the forms -----------------------------------------------------------------------------------------------------------
def _pack(cols, expected, n_out):
    cols = i64(cols)
    expected = i64(expected)
    _require(np.abs(cols) < (1 << 53), "an input is not an exact double")
    _require(np.abs(expected) < (1 << 53), "an output is not an exact double")
    inp = np.zeros((cols.shape[0], LF_IN), dtype=np.float64)
    inp[:, :cols.shape[1]] = cols.astype(np.float64)
    assert np.array_equal(inp[:, :cols.shape[1]].astype(np.int64), cols)
    exp = np.zeros((cols.shape[0], LF_OUT), dtype=np.int64)
    exp[:, :n_out] = expected.reshape(cols.shape[0], n_out)
    assert cols.shape[0] <= (1 << 20)
    return inp, exp, n_out


def _closed_expected(start, acc):
    """the limb walk of v_j = acc_j + x_j, x the (wrapped) digits of the start value"""
    acc = i64(acc)
    _require(np.abs(acc) < BIG_BOUND, "|acc_j| < 2^47")
    v = closed_v(start, acc)
    _require(np.abs(v) < (1 << 53), "|V| < 2^53")
    _require(np.abs(v) + C < (1 << 53), "|V| + C < 2^53")
    lim = acc.copy()
    lim[:, :3] += digits51(start)
    d = walk(lim, 3)
    a = whole(d)
    return np.column_stack([a, d, ceil_half(a)])


@functools.lru_cache(maxsize=None)
def cases(form, n_random=N_RANDOM):
    rng = _rng(form)
    n = n_random
    if form in (NORM3, NORM4):
        s = 3 if form == NORM3 else 4
        grids = [product(*([sorted(set(BIG_A + BIG_B + BIG_C))] * 3))] if s == 3 else [product(*([g] * 4)) for g in (BIG_A, BIG_B, BIG_C)] + [product(BIG_A, BIG_B, BIG_C, BIG_B)]
        x = np.concatenate([_big_random(rng, n, s), _stored_random(rng, n // 4, s) * 3] + grids)
        _require(np.abs(x) < BIG_BOUND, "|limb| < 2^47")
        return _pack(x, walk(x), s)
    if form in (RSH1_3, Y_OF):
        x = np.concatenate([_stored_random(rng, n, 3), rng.integers(-2 * HALF, 2 * HALF + 1, (n // 4, 3)), product(*([RSH_LIMBS] * 3))])
        if form == RSH1_3:
            return _pack(x, rsh1(x), 3)
        x = np.concatenate([np.column_stack([x, np.full(len(x), sg)]) for sg in (0, 1)])
        a = whole(x[:, :3]) * (1 - 2 * x[:, 3])
        return _pack(x, ceil_half(a), 1)
    if form in (DIGITS3, DIGITS3_WRAPPED):
        a = np.concatenate([_y_random(rng, n), _window_random(rng, n // 4), i64(Y_EDGES), i64(WINDOW_EDGES),
                            i64([(q << 34) + (d1 << B) + d2 for q in (HALF, -HALF, HALF - 1, 0, -1) for d1 in (-HALF, HALF - 1, 0) for d2 in (-HALF, HALF - 1, 0, 1)
                                 if abs((q << 34) + (d1 << B) + d2) < Y_BOUND])])
        if form == DIGITS3:
            d = digits_quotient(a)
            return _pack(a[:, None], np.column_stack([d, d]), 6)
        return _pack(a[:, None], digits51(a), 3)
    if form in (CLOSED4, CLOSED5):
        sk = 4 if form == CLOSED4 else 5
        sets = [(BIG_A,) * 4, (BIG_B,) * 4, (BIG_C, BIG_A, BIG_B, BIG_C)] if sk == 4 else [(BIG_A,) * 5, (BIG_B,) * 5, (BIG_C, BIG_B, BIG_A, BIG_B, BIG_C)]
        parts = [np.column_stack([_y_random(rng, n), _big_random(rng, n, sk)])]
        # the body column's start: Y +- Y_body
        parts.append(np.column_stack([_y_random(rng, n // 4) + _y_random(rng, n // 4), _big_random(rng, n // 4, sk)]))
        for k, st in enumerate(sets):
            g = product(*st)
            parts.append(np.column_stack([cycle(Y_EDGES, len(g), 7 + 4 * k), g]))     # (strides coprime to the sets' 9 and to len(Y_EDGES))
        parts.append(_closed_solved(sk))
        x = np.concatenate(parts)
        return _pack(x, _closed_expected(x[:, 0], x[:, 1:]), 5)
    if form == WRITE_POST:
        g = product(*([STORED] * 6))
        x = np.concatenate([np.column_stack([_stored_random(rng, n, 6), _window_random(rng, n)]),
                            np.column_stack([g, cycle(WINDOW_EDGES, len(g), 5)]),
                            np.column_stack([cycle(STORED, 6 * len(WINDOW_EDGES), 1).reshape(-1, 1).repeat(6, 1) * np.array([1, -1, 1, -1, 1, -1]).clip(-1, 1),
                                             np.repeat(i64(WINDOW_EDGES), 6)])])
        _require((x[:, 6] >= -C) & (x[:, 6] < P51 - C), "a is a window51 value")
        _require(np.abs(x[:, :6]) <= HALF, "stored limbs")
        v = whole(x[:, 0:3]) - whole(x[:, 3:6]) + x[:, 6]
        _require(np.abs(v) + C < (1 << 53), "|V| + C < 2^53")
        return _pack(x, whole(walk(x[:, 0:3] - x[:, 3:6] + digits51(x[:, 6]))), 1)
    if form in (PAIR_SUM, PAIR_DIFF):
        g = product(*([STORED] * 6))
        ab = np.concatenate([_stored_random(rng, n, 6), g])
        x = np.concatenate([np.column_stack([ab[:, :3], np.full(len(ab), sg), ab[:, 3:]]) for sg in (0, 1)])
        _require(np.abs(np.delete(x, 3, axis=1)) <= HALF, "stored limbs")
        a = x[:, 0:3] * (1 - 2 * x[:, 3:4])                       # the rotation's negation, limb by limb
        b = x[:, 4:7]
        if form == PAIR_SUM:
            return _pack(x, whole(rsh1(a + b)), 1)                # rsh(1) of un-normalised limbs reaching +-2^17, top digit wrapped
        return _pack(x, np.column_stack([whole(rsh1(a - b)), ceil_half(whole(a) - whole(b))]), 2)
    if form == PAIR_OUT:
        w_edges = sorted({t + d for t in (-C, P51 - C, -C - P51, 0, 3 * (1 << 50) + BIG_BOUND, -3 * (1 << 50) - BIG_BOUND, (1 << 50), HALF, (1 << 33) + HALF)
                          for d in (-2, -1, 0, 1, 2)})
        g = product(WINDOW_EDGES, w_edges)
        x = np.concatenate([np.column_stack([_window_random(rng, n), rng.integers(-(13 << 48), 13 << 48, n)]), g])
        _require((x[:, 0] >= -C) & (x[:, 0] < P51 - C), "u is a window51 value")
        _require(np.abs(x[:, 1]) + C < (1 << 53), "|W| + C < 2^53")
        d = walk(digits51(x[:, 0]) - digits51(x[:, 1]))
        return _pack(x, np.column_stack([whole(d), d]), 4)
    if form in (CMUX_4_4, CMUX_5_4):
        sg = 4 if form == CMUX_4_4 else 5
        prods = [product(*([s] * sg)) for s in (BIG_A, BIG_B)] if sg == 5 else [product(*([s] * 4)) for s in (BIG_A, BIG_B, BIG_C)]
        p = np.concatenate([_big_random(rng, n, sg)] + prods)
        rows = np.concatenate([_stored_random(rng, n, 4).clip(-HALF, HALF - 1)] + [np.column_stack([cycle(STORED[:2] + STORED[3:], len(g), st) for st in (1, 2, 3, 4)]) for g in prods])
        _require(np.abs(p) < BIG_BOUND, "|product limb| < 2^47")
        c = np.zeros(len(p), dtype=np.int64)
        for j in range(sg - 1, -1, -1):
            c = carry(p[:, j] + c)
            _require(np.abs(c) < (1 << 31), "every cmux carry below 2^31")
        _require((rows >= -HALF) & (rows < HALF), "the row is normalised")
        return _pack(np.column_stack([p, rows]), walk(rows + walk(p, 4)), 4)
    raise ValueError(form)


def digest(outputs, start=0):
    """the digest tests/limb_forms_host.cpp's main prints: sum over the outputs' bit patterns times (2 * index + 1), modulo 2^64"""
    bits = np.ascontiguousarray(outputs, dtype=np.float64).reshape(-1).view(np.uint64)
    w = (np.arange(start, start + len(bits), dtype=np.uint64) << np.uint64(1)) + np.uint64(1)
    return int((bits * w).sum(dtype=np.uint64)), start + len(bits)


def grid_file_bytes(n_random=256):
    """every form's whole edge grid (and a few random coefficients) with the expected outputs, in the layout
    tests/limb_forms_host.cpp's main reads: per form int32 form, n, n_in, n_out, then the n * n_in doubles the form reads,
    then its n * n_out outputs as int64"""
    out = []
    for form in range(len(FORMS)):
        inp, exp, n_out = cases(form, n_random)
        n_in = int(np.max(np.nonzero(inp.any(axis=0))[0])) + 1
        out.append(np.array([form, len(inp), n_in, n_out], dtype=np.int32).tobytes())
        out.append(np.ascontiguousarray(inp[:, :n_in]).tobytes())
        out.append(np.ascontiguousarray(exp[:, :n_out]).tobytes())
    return b"".join(out)

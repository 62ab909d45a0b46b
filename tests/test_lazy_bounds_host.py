"""CPU: the crafted operands of tests/lazy_inputs.py reach the edges they were made for, the reduction policy of csrc/ntt_core.cuh is
sound by interval reasoning alone, and the whole-transform model never wraps on the tightest modulus of every class.

Nothing here touches a GPU: `lazy_probe policy` / `consts` are host-only modes of tests/cpp/lazy_probe.hip."""
import numpy as np
import pytest

from fractions import Fraction

import lazy_inputs as li
import lazy_model as lm
import lazy_stress as ls

M64 = lm.M64
MODULI = li.moduli()


def test_probe_builds_and_its_policy_is_the_one_restated_here():
    """build-only test of lazy_probe (no GPU): its `policy` mode prints fwd_reduce_mask, InvPolicy and TQ as the headers compute them"""
    pol, classes, raw = lm.probe_policy()
    assert raw["hl_lit"] == lm.HL_LIT and raw["hl_lit_exact"] == 2 and raw["block"] == lm.BLOCK
    assert sorted(pol) == [(logn, hl) for logn in range(11, 16) for hl in range(2, 7)]
    for (logn, hl), e in pol.items():
        assert e == lm.policy_py(logn, hl), (logn, hl)
    assert sorted(classes) == sorted([(6, True), (5, True), (4, True), (3, True), (2, True), (6, False), (4, False), (3, False), (2, False),
                                      (lm.HL_LIT, False)])


def test_moduli_cover_every_bit_length_and_both_sides_of_near():
    names = dict(MODULI)
    for k in li.BITS:
        top, gen, low = names["top-%d" % k], names["general-top-%d" % k], names["low-%d" % k]
        for q in (top, gen, low):
            assert q.bit_length() == k and q % li.STEP == 1 and li.fz.is_prime(q)
        assert lm.consts(top)["near_ok"] and not lm.consts(gen)["near_ok"]
        assert not any(li.fz.is_prime(m) for m in range(top + li.STEP, 1 << k, li.STEP))          # the largest one
        assert low < (1 << (k - 1)) + (1 << (k - 1)) // 10
    qs = set(names.values())
    assert all(q in qs for nm, q in li.fz.threshold_primes() if nm.startswith("near-"))       # (some ARE a general-top prime)
    assert sum(nm.startswith("barrett-inexact") for nm in names) == 2
    assert all(not li.barrett_exact(q) for nm, q in MODULI if nm.startswith("barrett-inexact"))
    # every instantiated class is run by some modulus
    assert {c for _, q in MODULI for c in li.classes_for(q)} == set(lm.probe_policy()[1])


def test_constants_restated_here_are_the_librarys():
    """lazy_probe consts = prime_reduction_constants, the function fast_tables_create calls"""
    for nm, q in MODULI:
        c, p = lm.consts(q), lm.probe_consts(q)
        for key in ("nq", "red_sh1", "red_sh2", "red_c", "delta", "near_sh", "near_mask", "near_ok"):
            assert c[key] == p[key], (nm, key)


def test_red_c_is_the_floor_and_the_estimate_is_exact_or_one_less_on_the_whole_domain():
    """the library's own constants (`lazy_probe consts`), by their defining property and not by a copy of the formula: red_c =
    floor(2^(31 + k) / q) in 32 bits, sh1 + sh2 = k - 1, the top bits of every x < B q fit 32 bits, and the real number the estimate
    floors, t red_c / 2^(32 + sh2) with t = floor(x / 2^sh1), lies below x / q by less than the slack
        x / 2^(k + 31)  [red_c rounded down]  +  2^sh1 / q  [x's low bits dropped]  +  2^-(k + 31)  [both at once]
    which is below 1 at x = B q: e is floor(x / q) or one less on all of [0, B q)"""
    for nm, q in MODULI:
        k, p = q.bit_length(), lm.probe_consts(q)
        c, sh1, sh2 = p["red_c"], p["red_sh1"], p["red_sh2"]
        assert c * q <= (1 << (31 + k)) < (c + 1) * q and c < (1 << 32), nm
        assert sh1 + sh2 == k - 1, nm
        B = li.reduce_domain(q)
        assert B * q <= min(1 << (32 + sh1), 1 << 64), nm
        slack = Fraction(B * q, 1 << (k + 31)) + Fraction(1 << sh1, q) + Fraction(1, 1 << (k + 31))
        assert slack < 1, (nm, float(slack))
        # the bound is the one the words obey: at the x just below each multiple of q, where the estimate is weakest
        xs = lm.arr([m * q - 1 for m in range(1, B + 1)])
        t = xs >> np.uint64(sh1)
        real = [Fraction(int(ti) * c, 1 << (32 + sh2)) for ti in t]
        assert all(0 <= Fraction(int(x), q) - r < slack for x, r in zip(xs, real)), nm


def _restated(op, c, tup, hl, near):
    """the word-exact restatement on one record's tuples (classification code: checked against the contracts below, never expected)"""
    q = c["q"]
    a = [lm.arr([t[i] for t in tup]) for i in range(len(tup[0]))]
    if op == "mul_hi":
        return [int(x) for x in lm.w_mul_hi(a[0], a[1])]
    if op == "mul_wide":
        with np.errstate(over="ignore"):
            return list(zip((int(x) for x in a[0] * a[1]), (int(x) for x in lm.w_mul_hi(a[0], a[1]))))
    if op in ("shoup_mul_lazy", "mul_shoup2"):
        return [int(x) for x in lm.w_mul_shoup2(a[0], a[1], a[2], q)]
    if op.startswith("mul_shoup4m"):
        return [int(x) for x in lm.w_mul_shoup4m(a[0], a[1], a[2], q, a[3])]
    if op == "reduce_2q":
        return [int(x) for x in lm.w_reduce_2q(a[0], c)[1]]
    if op == "reduce_2q_near":
        return [int(x) for x in lm.w_reduce_2q_near(a[0], c)[1]]
    if op == "mul_fold_near":
        return lm.w_mul_fold_near(a[0], a[1], c)[2]
    return None


def test_crafted_operands_reach_every_band_error_and_corner():
    """per modulus: quotient error 0, 1, 2 and result bands 0 .. 3 of mul_shoup4m, both bands of mul_shoup2, both outcomes of the
    reduce_2q estimate, the largest e of reduce_2q_near, the largest F and t of mul_fold_near -- and the restated algorithms keep the
    contracts on every crafted tuple (so the claims hold on the CPU before a GPU is asked)"""
    exceptions = []
    for nm, q in MODULI:
        c = lm.consts(q)
        k = c["k"]
        recs, tuples = li.records_for(q)
        by = {}
        for (op, hl, near, _, arrays), tup in zip(recs, tuples):
            by.setdefault(op, tup)
            for a in arrays:
                assert all(0 <= x <= M64 for x in a), (nm, op)
            got = _restated(op, c, tup, hl, near)
            if got is not None:
                for t, g in zip(tup, got):
                    assert lm.contract(op, c, t, g, hl, near) is None, (nm, op, t, g, lm.contract(op, c, t, g, hl, near))
        # mul_shoup4m
        T = by["mul_shoup4m"]
        y, w = lm.arr([t[0] for t in T]), lm.arr([t[1] for t in T])
        err, band, _ = lm.classify_shoup4m(y, w, q)
        assert int(err.max()) <= 2 and int(band.max()) <= 3, nm
        assert set(err.tolist()) == {0, 1, 2}, (nm, set(err.tolist()))
        assert set(band.tolist()) == {0, 1, 2, 3}, (nm, set(band.tolist()))
        for op in ("mul_shoup4m_tws", "mul_shoup4m_acc", "mul_shoup4m_acc_tws"):       # the regrouped sets lose nothing
            e2, b2, _ = lm.classify_shoup4m(lm.arr([t[0] for t in by[op]]), lm.arr([t[1] for t in by[op]]), q)
            assert set(e2.tolist()) == {0, 1, 2} and set(b2.tolist()) == {0, 1, 2, 3}, (nm, op)
        # the corners of the domain
        ys, ws = {t[0] for t in T}, {t[1] for t in T}
        assert {0, 1, q - 1, q, 2 * q - 1, 2 * q, 4 * q - 1, M64} <= ys and set(li.w_corners(q)) <= ws, nm
        assert {t[3] for t in by["mul_shoup4m_acc"]} >= {0, 2 * q - 1}, nm
        # mul_shoup2
        r2 = lm.w_mul_shoup2(y, w, lm.arr([t[2] for t in T]), q) // np.uint64(q)
        assert set(r2.tolist()) == {0, 1}, nm
        # reduce_2q: e exact, and one less with the result in [q, 2q)
        xs = lm.arr([t[0] for t in by["reduce_2q"]])
        e, r = lm.w_reduce_2q(xs, c)
        d = (xs // np.uint64(q)) - e
        assert set(d.tolist()) <= {0, 1}, nm
        if set(d.tolist()) != {0, 1}:
            # Argument: e = floor(floor(x / 2^sh1) * red_c / 2^(32 + sh2)) with red_c = floor(2^(31 + k) / q), sh1 + sh2 = k - 1: the
            # estimate loses (x mod 2^sh1) / q < 2^(k - 17) / q <= 2^-16 and t * (2^(31 + k) / q - red_c) / 2^(32 + sh2) < t / 2^48;
            # the exhaustive scan of both neighbours of every multiple m q, m <= B, below shows no x of the domain where that costs
            # a unit -- such a modulus has no one-less outcome to reach.
            B = li.reduce_domain(q)
            scan = lm.arr(sorted({m * q + j for m in range(1, B + 1) for j in range(0, 4096) if m * q + j < min(B * q, M64 + 1)}))
            es, _ = lm.w_reduce_2q(scan, c)
            assert bool((es == scan // np.uint64(q)).all()), nm
            exceptions.append((nm, "reduce_2q one-less"))
        else:
            assert bool(((r >= np.uint64(q)) == (d == 1)).all()), nm
        assert int(r.max()) < 2 * q
        if c["near_ok"]:
            # reduce_2q_near: the largest e = 2^(64 - k) - 1, with x mod 2^k = 2^k - 1
            xs = lm.arr([t[0] for t in by["reduce_2q_near"]])
            e, r = lm.w_reduce_2q_near(xs, c)
            assert int(e.max()) == (1 << (64 - k)) - 1 and M64 in set(xs.tolist()), nm
            assert int(r.max()) < 2 * q, nm
            # mul_fold_near: F = Phi delta + Plo with Phi = P >> k <= Phimax = ((2q - 1)(2^k - 1)) >> k: the set holds an operand whose
            # Phi IS Phimax, so its F lies within 2^k of any F the domain can produce
            T = by["mul_fold_near"]
            assert (2 * q - 1, (1 << k) - 1) in T and (2 * q - 1, q - 1) in T, nm
            F, t, R = lm.w_mul_fold_near([x for x, _ in T], [b for _, b in T], c)
            phimax = ((2 * q - 1) * ((1 << k) - 1)) >> k
            fbound = phimax * c["delta"] + (1 << k) - 1
            assert max(F) >= phimax * c["delta"] and max(F) <= fbound < (1 << 96) and (fbound >> k) < (1 << 32), nm    # (F: three words)
            # (t = F >> k: Plo < 2^k adds at most one to (Phimax delta) >> k, so the set's largest t is the domain's or one less)
            tlow = (phimax * c["delta"]) >> k
            assert tlow <= max(t) <= fbound >> k <= tlow + 1, (nm, max(t), fbound >> k)
            assert max(R) < 2 * q, nm
    # DESIGN.md ("Lazy-range sweep") lists these
    assert len(exceptions) == EXPECTED_EXCEPTIONS, exceptions


EXPECTED_EXCEPTIONS = 0


def test_lit_inputs_reach_the_non_canonical_words_of_single_barrett(oracle):
    """the Python statement of singleBarrett is the oracle's, and on the Barrett-inexact moduli the crafted pairs reach q + r"""
    L = oracle.lib()
    for nm, q in MODULI:
        c = lm.consts(q)
        T = li.lit_inputs(q)
        words = [lm.single_barrett(a, b, q, c["mu"], c["k"]) for a, b in T]
        for (a, b), wd in list(zip(T, words))[::7]:
            assert wd == L.orc_barrett(a, b, q, c["mu"], c["k"]), (nm, a, b)
        canonical_pairs = [(a, b, wd) for (a, b), wd in zip(T, words) if a < q and b < q]
        if li.barrett_exact(q):
            assert all(wd == a * b % q for a, b, wd in canonical_pairs), nm
        else:
            assert any(wd >= q for a, b, wd in canonical_pairs), nm


# ---- policy soundness ----------------------------------------------------------------------------------------------------
def _largest_q(hl):
    """the largest modulus a class serves: below 2^(64 - hl) (class 6: up to 58 bits)"""
    return (1 << (64 - hl)) - 1


def _check_all(policy_of, qmax_of=_largest_q):
    bad = []
    for hl, near in lm.probe_policy()[1]:
        if hl == lm.HL_LIT:
            continue
        for logn in range(11, 16):
            for fused in (False, True):
                for split16 in ((False, True) if logn == 15 else (False,)):
                    b, _, _ = lm.check_policy(policy_of(logn, hl), hl, near, qmax_of(hl), split16=split16, fused=fused)
                    bad += [((logn, hl, near, fused, split16), m) for m in b]
    return bad


def test_policy_is_sound_by_interval_reasoning():
    """forward, fused hand-over and inverse of every instantiated (LOGN, HL, NEAR), with the n = 2^16 coupling stage around the 2^15
    halves: sums below 2^64 for the largest q of the class, every cq at least what is subtracted, every operand inside its domain"""
    pol = lm.probe_policy()[0]
    assert _check_all(lambda logn, hl: pol[(logn, hl)]) == []


def test_the_checker_rejects_unsound_policies():
    """H doubled, and one cmul lowered by one, with and without the fused hand-over and the n = 2^16 coupling stage: the checker
    must bite.  (Behind the fused product of the folding classes the first stage subtracts with 2q, IN2Q, whatever cmul[0] says: there
    cmul[0] is not read and only s >= 1 can be lowered.)"""
    for hl, near in lm.probe_policy()[1]:
        if hl == lm.HL_LIT:
            continue
        for logn in range(11, 16):
            good = lm.probe_policy()[0][(logn, hl)]
            for fused in (False, True):
                for split16 in ((False, True) if logn == 15 else (False,)):
                    kw = dict(fused=fused, split16=split16)
                    bad, _, _ = lm.check_policy(lm.policy_py(logn, hl, h_scale=2), hl, near, _largest_q(hl), **kw)
                    assert bad, ("H doubled passes", logn, hl, near, kw)
                    first = 1 if fused and lm.fused_is_lazy(hl, near) else 0
                    for s in range(first, logn):
                        low = dict(good, cmul=[c - (i == s) for i, c in enumerate(good["cmul"])])
                        bad, _, _ = lm.check_policy(low, hl, near, _largest_q(hl), **kw)
                        assert any("cq" in m for m in bad), ("cmul[%d] - 1 passes" % s, logn, hl, near, kw)


# ---- whole-transform model ----------------------------------------------------------------------------------------------
TIGHT = [e for e in ls.entries() if e[0].startswith("tight-")]


@pytest.mark.parametrize("n", ls.MODEL_SIZES)
def test_transform_model_never_wraps_and_stays_below_the_policy_bound(n):
    """the lazy rounds of every class on the tightest modulus of the class, on EVERY seed of the search -- all q - 1, alternating
    0 / q - 1, a single q - 1 at 0, 1, n/2, n - 1, the stage-state back-solves, the random polynomials of the family: no operation
    wraps 2^64 or goes negative (run_model raises), no value passes the bound the interval checker allows, every margin is positive;
    on the model-free seeds, the whole-transform back-solves and one random polynomial the canonical result is the exact transform's"""
    logn = n.bit_length() - 1
    for name, q, hl, near in TIGHT:
        tb = ls.tables(q, n)
        _, pf, pi = lm.check_policy(lm.probe_policy()[0][(logn, hl)], hl, near, q, fused=True)
        allowed = {"fwd": pf, "inv": pi, "mul": max(pf, pi)}
        b = ls.bhat(q, n)
        for op in ls.OPS:
            for nm, thunk in ls.seeds(q, n, hl, near, op).items():
                a = lm.arr(thunk())
                assert int(a.max()) < q, (name, op, nm)
                got, tr = lm.run_model(op, a, b if op == "mul" else None, tb, hl, near)
                assert tr.peak_word <= M64 and tr.peak_q <= allowed[op] and tr.margin > 0, (name, op, nm, tr.peak_q, allowed[op], tr.margin)
                if nm in ("fwd-state@%d" % logn, "inv-state@%d" % logn):         # the back-solve did what its name says
                    want = [q - 1] * n if op == "fwd" else [(q - 1) * tb.ninv % q] * n
                    if op != "mul":
                        assert got.tolist() == want, (name, op, nm)
                if "@" in nm and "state" not in nm or nm in ("allmax", "alt", "random0"):
                    if op == "fwd":
                        want = lm.exact_forward(a, tb)
                    elif op == "inv":
                        want = lm.exact_inverse(a, tb)
                    else:
                        want = lm.exact_inverse([x * int(y) % q for x, y in zip(lm.exact_forward(a, tb), b)], tb)
                    assert got.tolist() == want, (name, op, nm)


def test_replicated_back_solve_is_the_stage_state_back_solve():
    """the forward stage-state back-solve the GPU test builds above n = 4096 from a size-2^s table (lazy_stress.replicated_forward_state)
    is, where both exist, the one undone stage by stage on the full table"""
    n, (name, q, hl, near) = 4096, TIGHT[0]
    tb = ls.tables(q, n)
    for s in (1, 5, 12):
        assert ls.replicated_forward_state(q, fz_psi(q, n), n, s).tolist() == lm.undo_forward_stages([q - 1] * n, tb, s), s


def fz_psi(q, n):
    return li.fz.psi_for(q, n)


@pytest.mark.parametrize("idx", range(len(ls.entries())), ids=[e[0] for e in ls.entries()])
def test_committed_stress_polynomials_reach_at_least_what_random_data_reach(idx):
    """tests/golden/lazy_stress_*.npz, re-run through the model: canonical words, at most MAX_CHANGED searched coefficients, nothing
    wraps or goes negative (run_model raises), no value passes the checker's bound, the model shows again what the generator recorded,
    and per (n, op) the winner for the peak is not below the peak of the 16 random polynomials of the seed family, the winner for the
    margin not above their smallest margin"""
    entry = ls.entries()[idx]
    name, q, hl, near = entry
    for n in ls.MODEL_SIZES:
        _, pf, pi = lm.check_policy(lm.probe_policy()[0][(n.bit_length() - 1, hl)], hl, near, q, fused=True)
        allowed = {"fwd": pf, "inv": pi, "mul": max(pf, pi)}
        for op in ls.OPS:
            rnd = [ls.evaluate(q, n, hl, near, op, r) for r in ls.randoms(q, n, op)]
            res = {}
            for goal in ls.GOALS:
                key = "%d_%s_%s_" % (n, op, goal)
                a = ls.crafted(entry, n, op, goal)
                assert int(a.max()) < q and len(ls._fixture(name)[key + "pos"]) <= ls.MAX_CHANGED, (name, key)
                res[goal] = ls.evaluate(q, n, hl, near, op, a)
                assert list(res[goal]) == ls._fixture(name)[key + "result"].tolist(), (name, key)
                assert res[goal][1] <= 1.0 and res[goal][0] <= allowed[op] and res[goal][2] > 0, (name, key, res[goal], allowed[op])
            print("%s n=%d %s allowed %d random %.2f crafted %.2f (%.4f of 2^64) margin random %.3g crafted %.3g"
                  % (name, n, op, allowed[op], max(r[0] for r in rnd), res["peak"][0], res["peak"][1], min(r[2] for r in rnd),
                     res["margin"][2]))
            assert res["peak"][0] >= max(r[0] for r in rnd), (name, n, op, res["peak"][0], max(r[0] for r in rnd))
            assert res["margin"][2] <= min(r[2] for r in rnd), (name, n, op, res["margin"][2], min(r[2] for r in rnd))

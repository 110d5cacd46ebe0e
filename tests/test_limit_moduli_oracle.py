"""The oracle anchored at the limit moduli of tests/limit_moduli.py (no GPU).

The GPU tests compare the kernels with the oracle at moduli and residues the oracle itself had never seen: the largest NTT prime below
2^61, both sides of 2^60, 2^57, 2^46, 2^33, 2^32 and the extension moduli on either side of each admission bound.  Here the oracle is
compared, at those moduli and on the stress polynomials, with arithmetic that shares nothing with it: direct evaluation of the transform
in Python integers, and exact rational arithmetic on the CRT-reconstructed value for the basis extension, ModDown and the divisions by
the last modulus.  The helper itself (prime search, predicate mirrors, the Python restatement of the butterfly networks, the stage-pinned
polynomials) is checked first."""
from fractions import Fraction

import numpy as np
import pytest

import limit_moduli as lm
from conftest import crt_reconstruct

SMALL_LOGN = (4, 6)


def _all_moduli(logn):
    seen = []
    for s in lm.admission_sets(logn).values():
        for q in s.moduli + s.P:
            if q not in seen:
                seen.append(q)
    return seen


# ------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [4, 6, 12, 16])
def test_below_and_above_are_the_neighbours_of_the_power_of_two(logn):
    step = 2 << logn
    for bits in (32, 33, 46, 57, 60, 61):
        lo, hi = lm.below(bits, logn), lm.above(bits, logn)
        assert lo < (1 << bits) < hi and lo % step == 1 and hi % step == 1
        assert lm.params.is_prime(lo) and lm.params.is_prime(hi)
        assert not any(lm.params.is_prime(p) for p in range(lo + step, hi, step))      # nothing in between
        assert lm.at_most(lo, logn) == lo and lm.more_than(lo, logn) == hi and lm.at_most(hi - 1, logn) == lo
    assert lm.below(61, logn, 3) == sorted(lm.below(61, logn, 3), reverse=True)
    # the moduli the issue's emulator run was made with
    if logn == 12:
        assert lm.below(61, 12) == 0x1ffffffffffde001 and lm.below(57, 12) == 0x1ffffffffff6001
        assert lm.above(57, 12) == 0x200000000032001 and lm.above(33, 12) == 0x200026001


@pytest.mark.parametrize("logn", [4, 6, 12, 15])
def test_each_admission_set_sits_on_the_side_it_names(logn):
    sets = lm.admission_sets(logn)
    top = 1 << 61
    for s in sets.values():
        assert lm.supported(s.moduli + s.P), s.name
    m = {k: lm.ntt_mode(v.moduli) for k, v in sets.items() if v.kind == "ntt"}
    a = {k: lm.asm_variants(v.moduli) for k, v in sets.items() if v.kind == "ntt"}
    assert (m["ntt_below61"], a["ntt_below61"]) == (0 | 256, (0, 0)) and max(sets["ntt_below61"].moduli) < top
    assert not lm.supported([lm.above(61, logn)])
    assert (m["ntt_below60"], a["ntt_below60"]) == (1 | 256, (1, 1))
    assert (m["ntt_above60"], a["ntt_above60"]) == (0 | 256, (0, 0))
    assert (m["ntt_below57"], a["ntt_below57"]) == (2 | 256, (2, 1))
    assert (m["ntt_above57"], a["ntt_above57"]) == (1 | 256, (1, 1))
    assert (m["ntt_below46"], a["ntt_below46"]) == (2 | 256, (3, 3))
    assert (m["ntt_above46"], a["ntt_above46"]) == (2 | 256, (2, 1))
    assert lm.asm_variants(sets["ntt_below46"].moduli, no_fp=True) == (2, 1)
    assert (m["ntt_above33"], a["ntt_above33"]) == (2 | 256, (3, 3))         # the FP64 body takes them; the integer bodies would too
    assert lm.asm_variants(sets["ntt_above33"].moduli, no_fp=True) == (2, 1)
    assert lm.asm_variants(sets["ntt_above33"].moduli, asm_variant=0) == (0, 0)
    assert (m["ntt_straddle33"], a["ntt_straddle33"]) == (2 | 256, (3, 3))   # below 2^46: the dual kernels' FP64 body ...
    assert lm.asm_variants(sets["ntt_straddle33"].moduli, no_fp=True) == (-1, -1)   # ... and without it no assembly kernel at all
    assert m["ntt_above32"] == 2 | 256 and m["ntt_below32"] == 2
    # the forced modes of the testing aid: 0 only where 1 is chosen, 3 anywhere
    assert lm.ntt_mode(sets["ntt_below60"].moduli, 0) == 0 | 256 and lm.ntt_mode(sets["ntt_below57"].moduli, 0) == 2 | 256
    assert lm.ntt_mode(sets["ntt_below61"].moduli, 3) == 3 | 256
    for k, s in sets.items():
        if s.kind != "ext":
            continue
        n, inside = s.terms, s.admitted
        if k.startswith("ext_lazy"):
            assert lm.lazy_terms(s.P) == (n if inside else n - 1), k
            assert lm.ext_kernel(s.moduli, s.P, n, 1 << logn) == ("ext_sum" if inside else "ext_wide<%d>" % n), k
        elif k.startswith("ext_exact"):
            assert lm.exact_terms(s.P) == (8 if inside else 7), k
            assert lm.ext_kernel(s.moduli, s.P, n, 1 << logn, ext_narrow=True) == ("ext_shoup<7>" if inside else "ext_shoup<3>"), k
            assert lm.ext_kernel(s.moduli, s.P, n, 1 << logn) == "ext_wide<8>", k
        elif k.startswith("ext_wide"):
            assert (lm.wide_ok(s.moduli) >= n) == inside and lm.lazy_terms(s.P) < n, k
            assert lm.ext_kernel(s.moduli, s.P, n, 1 << logn) == ("ext_wide<%d>" % n if inside else "ext_wide<8>"), k
        elif k.startswith("ext_word"):
            assert lm.word_barrett(s.P) == int(inside), k
            assert lm.ext_kernel(s.moduli, s.P, n, 1 << logn) == ("ext_sum" if inside else "ext_shoup<0>"), k
    assert lm.wide_ok(sets["ext_wide8_in"].moduli) == 8                     # exactly the group size
    for k, s in sets.items():
        if s.kind == "keymac":
            assert lm.keymac_wide_ok(s.moduli + s.P, s.terms) == s.admitted, k
            assert lm.keymac_wide_ok(s.moduli + s.P, s.terms - 1) and not lm.keymac_wide_ok(s.moduli + s.P, s.terms + 1), k
            assert not lm.keymac_wide_ok(s.moduli + s.P, s.terms, keymac_narrow=True)


@pytest.mark.parametrize("logn", [4, 6, 10])
def test_python_networks_restate_the_oracle(oracle, logn):
    """the stage loops of limit_moduli (ring/ntt.go in Python integers, with tables built from the root the oracle chose) against
    oracle.ntt / oracle.intt on a random poly, and their inverses against themselves"""
    N = 1 << logn
    moduli = [lm.below(61, logn), lm.above(57, logn), lm.below(46, logn), lm.below(32, logn)]
    oc = oracle.Context(N, moduli)
    rng = np.random.default_rng(logn)
    x = np.array([[int(v) % q for v in rng.integers(0, 1 << 63, N, dtype=np.uint64)] for q in moduli], dtype=np.uint64)
    X, Xi = oc.ntt(x), oc.intt(x)
    for i, q in enumerate(moduli):
        fwd, inv = lm.psi_tables(q, N, lm.oracle_psi(oc, i))
        mont = (1 << 64) % q
        assert [w * mont % q for w in fwd[1:]] == [int(w) for w in oc.ntt_psi[i][1:]]
        assert [w * mont % q for w in inv[1:]] == [int(w) for w in oc.ntt_psi_inv[i][1:]]
        assert [int(v) for v in lm.fwd_stages(x[i], q, fwd)] == [int(v) for v in X[i]]
        assert [int(v) for v in lm.inv_stages(x[i], q, inv)] == [int(v) for v in Xi[i]]
        for s in (1, logn // 2, logn):
            assert list(lm.fwd_unstages(lm.fwd_stages(x[i], q, fwd, 0, s), q, fwd, s)) == [int(v) for v in x[i]]
            assert list(lm.inv_unstages(lm.inv_stages(x[i], q, inv, 0, s, scale=False), q, inv, s)) == [int(v) for v in x[i]]


@pytest.mark.parametrize("logn", [4, 6])
def test_stage_pinned_polys_pin_their_stage(logn):
    """entering stage s every upper slot is q - 1 and every product is q - 1: the butterfly's sum is 2q - 2, its difference 0"""
    N = 1 << logn
    for q in (lm.below(61, logn), lm.above(33, logn)):
        psi = next(g for g in (pow(b, (q - 1) // (2 * N), q) for b in range(2, 100)) if pow(g, N, q) == q - 1)
        fwd, inv = lm.psi_tables(q, N, psi)
        for s in range(logn):
            st = lm.fwd_stages(lm.stage_pinned(q, N, fwd, s), q, fwd, 0, s).reshape(1 << s, 2, N >> (s + 1))
            w = np.array(fwd[1 << s:2 << s], dtype=object).reshape(-1, 1)
            assert (st[:, 0, :] == q - 1).all() and (st[:, 1, :] * w % q == q - 1).all()
            st = lm.inv_stages(lm.stage_pinned(q, N, inv, s, inverse=True), q, inv, 0, s, scale=False).reshape(N >> (s + 1), 2, 1 << s)
            w = np.array(inv[N >> (s + 1):N >> s], dtype=object).reshape(-1, 1)
            assert (st[:, 0, :] == q - 1).all() and ((st[:, 0, :] - st[:, 1, :]) * w % q == q - 1).all()


def test_stress_polys_carry_every_family(oracle):
    N, logn = 64, 6
    moduli = lm.admission_sets(logn)["ntt_below61"].moduli
    oc = oracle.Context(N, moduli)
    names, x = lm.stress_polys(moduli, N, "ntt", oc)
    assert names == ["zero", "qm1", "alt", "first", "last", "spectrum_qm1", "uniform", "top"] + ["stage%d" % s for s in range(logn)]
    assert x.shape == (len(names), 2, N) and x.dtype == np.uint64
    assert set(lm.harshest(logn)) <= set(names)
    assert (x[names.index("top")] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert np.array_equal(oc.ntt(x[names.index("spectrum_qm1")]), x[names.index("qm1")])
    ni, xi = lm.stress_polys(moduli, N, "intt", oc)
    assert ni == names and all((xi[ni.index("top"), i] == np.uint64(4 * q - 1)).all() for i, q in enumerate(moduli))
    assert np.array_equal(oc.intt(xi[ni.index("spectrum_qm1")]), xi[ni.index("qm1")])
    nl, xl = lm.stress_polys(moduli, N, "lazy2q")
    assert nl == ["zero", "qm1", "alt", "first", "last", "uniform", "top"]
    assert lm.stress_polys(moduli, N, "ntt", oc, families=lm.harshest(logn))[0] == ["qm1", "top", "stage5"]
    assert lm.stress_polys(moduli, N, "canonical")[0] == nl[:-1]


# ------------------------------------------------------------------------------------------
# the oracle's transforms against direct evaluation
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", SMALL_LOGN)
def test_oracle_ntt_is_the_evaluation_at_the_odd_powers_of_psi(oracle, logn):
    """every modulus of every admission set, every stress poly: NTT(x)[i] = x(psi^(2 bitrev(i) + 1)), InvNTT its inverse, in Python integers"""
    N = 1 << logn
    for q in _all_moduli(logn):
        oc = oracle.Context(N, [q])
        psi = lm.oracle_psi(oc, 0)
        assert pow(psi, N, q) == q - 1
        roots = [pow(psi, 2 * lm.bitrev(i, logn) + 1, q) for i in range(N)]
        V = np.array([[pow(r, j, q) for j in range(N)] for r in roots], dtype=object)
        Vi = np.array([[pow(r, -j, q) for r in roots] for j in range(N)], dtype=object)
        n_inv = pow(N, -1, q)
        for domain, f in (("ntt", oc.ntt), ("intt", oc.intt)):
            names, x = lm.stress_polys([q], N, domain, oc)
            red = lm.canon(x, [q])
            for k, name in enumerate(names):
                got = [int(v) for v in f(red[k])[0]]
                xs = np.array([int(v) for v in red[k, 0]], dtype=object)
                want = list(V.dot(xs) % q) if domain == "ntt" else list(Vi.dot(xs) * n_inv % q)
                assert got == want, (hex(q), domain, name)


# ------------------------------------------------------------------------------------------
# basis extension, ModDown, division by the last modulus against exact rational arithmetic
# ------------------------------------------------------------------------------------------
def _prod(ms):
    r = 1
    for m in ms:
        r *= m
    return r


def _canonical_families(moduli, N, oc):
    names, x = lm.stress_polys(moduli, N, "ntt", oc)
    return names, lm.canon(x, moduli)


def _reference_v(ys, qs):
    """ring_basis_extension.go:372-376: the float64 sum of y_i / q_i, truncated"""
    v = 0.0
    for y, q in zip(ys, qs):
        v += float(y) / float(q)
    return int(v)


def _ext_sets(logn):
    return [s for s in lm.admission_sets(logn).values() if s.kind in ("ext", "keymac")]


@pytest.mark.parametrize("logn", SMALL_LOGN)
def test_oracle_modup_is_the_crt_value_up_to_the_documented_multiple_of_q(oracle, logn):
    """ModUpSplitQP (ring_basis_extension.go:147, modUpExact :352-393): with y_i = x_i (Q/q_i)^-1 mod q_i the value is
    X = sum y_i Q/q_i - k Q, k = floor(sum y_i / q_i) exactly.  The reference takes k from a float64 sum, v, so its output is
    X + (k - v) Q mod p_j: equal to X unless the fractional part of the sum is within float64 rounding of an integer (all q_i - 1:
    X = Q - 1, the fraction is 1 - 1/Q, v = k + 1 and the output is -1 mod p_j).  Asserted: the documented form with v computed as the
    reference does, and v = k wherever the fraction leaves float64 room."""
    N = 1 << logn
    off_by_one = 0
    for s in _ext_sets(logn):
        Q, P = s.moduli, s.P
        ocQ, ocP = oracle.Context(N, Q), oracle.Context(N, P)
        bx = oracle.BasisExtender(ocQ, ocP)
        names, x = _canonical_families(Q, N, ocQ)
        # (the full level only: below it the reference keeps the constants of the full Q -- :147-149 pass paramsQP whatever the level --
        # so its output is not the CRT value of the limbs it reads; the GPU tests compare those levels with the oracle as it is)
        for level in [len(Q) - 1]:
            qs = Q[:level + 1]
            Ql = _prod(qs)
            hat = [Ql // q for q in qs]
            hat_inv = [pow(h, -1, q) for h, q in zip(hat, qs)]
            for k, name in enumerate(names):
                got = bx.modup_split_qp(level, x[k][:level + 1])
                X = crt_reconstruct(x[k][:level + 1], qs)
                for c in range(N):
                    ys = [int(x[k, i, c]) * hat_inv[i] % qs[i] for i in range(level + 1)]
                    total = sum(y * h for y, h in zip(ys, hat))
                    kk = total // Ql
                    assert total - kk * Ql == X[c]
                    v = _reference_v(ys, qs)
                    frac = Fraction(total, Ql) - kk
                    if Fraction(level + 2, 1 << 52) < frac < 1 - Fraction(level + 2, 1 << 52):
                        assert v == kk, (s.name, name, c)
                    assert abs(v - kk) <= 1
                    off_by_one += v != kk
                    for j, p in enumerate(P):
                        assert int(got[j, c]) == (total - v * Ql) % p, (s.name, level, name, c, j)
    assert off_by_one > 0            # the all-(q - 1) family is such a case: the test would otherwise not have met the documented form


@pytest.mark.parametrize("logn", SMALL_LOGN)
def test_oracle_moddown_is_the_exact_quotient_by_p(oracle, logn):
    """ModDownPQ (ring_basis_extension.go:248) and ModDownNTTPQ (:163) on x over Q u P: (x - [x]_P) / P mod q_i, where [x]_P is the
    extension of x's P residues to Q -- x mod P, or that plus or minus P where the float64 sum behind the correction lands on the other
    side of an integer (see the ModUp test; x mod P = 2^64 - 1 against P of 120 bits is such a case, the sum sits 2^-56 above an integer) --
    so the result is floor(x / P), or one more or one less in that documented case, never anything else"""
    N = 1 << logn
    for s in _ext_sets(logn):
        Q, P = s.moduli[:4], s.P
        ocQ, ocP = oracle.Context(N, Q), oracle.Context(N, P)
        bx = oracle.BasisExtender(ocQ, ocP)
        names, xq = _canonical_families(Q, N, ocQ)
        _, xp = _canonical_families(P, N, ocP)
        level = len(Q) - 1
        Pp = _prod(P)
        hat = [Pp // p for p in P]
        hat_inv = [pow(h, -1, p) for h, p in zip(hat, P)]
        for k, name in enumerate(names):
            kp = (k + 1) % len(names)                  # another family on the P side: x is not a constant polynomial's lift
            got = bx.moddown_pq(level, np.concatenate([xq[k], xp[kp]]))
            got_ntt = ocQ.intt(bx.moddown_ntt_pq(level, np.concatenate([ocQ.ntt(xq[k]), ocP.ntt(xp[kp])])))
            X = crt_reconstruct(np.concatenate([xq[k], xp[kp]]), Q + P)
            for c in range(N):
                ys = [int(xp[kp, j, c]) * hat_inv[j] % P[j] for j in range(len(P))]
                total = sum(y * h for y, h in zip(ys, hat))
                v = _reference_v(ys, P)
                xP = total - v * Pp                     # X mod P, or that plus or minus P
                assert xP in (X[c] % Pp, X[c] % Pp - Pp, X[c] % Pp + Pp)
                for i, q in enumerate(Q):
                    want = (X[c] - xP) // Pp % q
                    assert (X[c] - xP) % Pp == 0
                    assert int(got[i, c]) == want, (s.name, name, c, i)
                    assert int(got_ntt[i, c]) == want, (s.name, name, c, i)


@pytest.mark.parametrize("logn", SMALL_LOGN)
def test_oracle_divisions_by_the_last_modulus_are_floor_and_round(oracle, logn):
    """DivFloorByLastModulus (ring_scaling.go:37) = floor(x / q_last), DivRoundByLastModulus (:117) = floor((x + (q_last - 1) / 2) / q_last)
    = round(x / q_last) (q_last is odd: no ties), limb by limb, with the last limb's residue on either side of the rounding point added to
    the stress polys; the NTT forms (:9, :72) agree after the transforms"""
    N = 1 << logn
    sets = lm.admission_sets(logn)
    for moduli in ([lm.below(61, logn, 3), lm.above(60, logn, 3), sets["ntt_above57"].moduli + sets["ntt_below57"].moduli,
                    sets["ntt_below32"].moduli + sets["ntt_above33"].moduli + [lm.below(61, logn)]]):
        oc = oracle.Context(N, moduli)
        names, x = _canonical_families(moduli, N, oc)
        ql = moduli[-1]
        tie = x[names.index("uniform")].copy()
        tie[-1, 0::2], tie[-1, 1::2] = (ql - 1) // 2, (ql + 1) // 2
        x = np.concatenate([x, tie[None]])
        names = names + ["tie"]
        Qrest = moduli[:-1]
        for k, name in enumerate(names):
            X = crt_reconstruct(x[k], moduli)
            fl = oc.rescale_op("oc_div_floor_by_last_modulus", x[k])
            rd = oc.rescale_op("oc_div_round_by_last_modulus", x[k])
            fl_ntt = oc.intt(oc.rescale_op("oc_div_floor_by_last_modulus_ntt", oc.ntt(x[k])))
            rd_ntt = oc.intt(oc.rescale_op("oc_div_round_by_last_modulus_ntt", oc.ntt(x[k])))
            for c in range(N):
                want_f = X[c] // ql
                want_r = int(Fraction(2 * X[c] + ql, 2 * ql).__floor__())
                assert want_r == (X[c] + (ql - 1) // 2) // ql
                for i, q in enumerate(Qrest):
                    assert int(fl[i, c]) == want_f % q == int(fl_ntt[i, c]), (name, c, i)
                    assert int(rd[i, c]) == want_r % q == int(rd_ntt[i, c]), (name, c, i)


# ------------------------------------------------------------------------------------------
# the host side of lr_arith.hpp at the same moduli
# ------------------------------------------------------------------------------------------
def test_host_shoup_and_reduction_primitives_at_the_limit_moduli(tmp_path):
    """tests/cpp/shoup_products.cpp: mul_shoup_lazy, mul_shoup_lazy_lowreg, mul_shoup_exact, bred*, mred*, mform*, inv_mform of
    lr_arith.hpp compiled for the host (with the sanitizers) against unsigned __int128 on the operand corners: congruence, the 4q and 2q
    ranges, and the quotient estimate's deficit of at most 2"""
    import os
    import subprocess

    from conftest import ROOT
    csrc = os.path.join(ROOT, "lattigo-fhe-by-go_amd", "csrc")
    exe = str(tmp_path / "shoup_products")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "shoup_products.cpp"), "-o", exe])
    moduli = [lm.below(61, 12), lm.above(60, 12), lm.below(60, 12), lm.above(57, 12), lm.below(57, 12), lm.above(46, 12), lm.below(46, 12),
              lm.above(33, 12), lm.below(33, 12), lm.above(32, 12), lm.below(32, 12), 12289]
    out = subprocess.run([exe] + [str(q) for q in moduli], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "moduli %d," % len(moduli) in out.stdout and "failures 0" in out.stdout, out.stdout


# ------------------------------------------------------------------------------------------
# the oracle's coefficient-wise family on the operand corners
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [6, 12])
def test_oracle_canonical_ewise_forms_are_the_integer_formulas(oracle, logn):
    """every canonical op of the coefficient-wise family, at one modulus per size class, on operands in which every pair of corner values
    occurs at every lane position: the oracle against the integer formula"""
    N = 1 << logn
    moduli = lm.ewise_moduli(logn)
    assert [q.bit_length() for q in moduli] == [61, 61, 58, 57, 32, 14 if logn <= 11 else 16]
    oc = oracle.Context(N, moduli)
    for wide in (False, True):
        a, b, c = lm.corner_operands(moduli, N, wide)
        for i, q in enumerate(moduli):
            assert lm.pairs_at_every_lane(a[:, i], b[:, i], q, wide)
        for op, f in lm.EWISE_FORMULAS.items():
            if wide and op not in lm.EWISE_WIDE:
                continue
            for k in range(0, a.shape[0], max(1, a.shape[0] // 2)):        # (a sample of the batch: the GPU tests run all of it)
                got = oc.ewise(op, a[k], b[k], out=c[k])
                for i, q in enumerate(moduli):
                    want = [f(int(x), int(y), int(z), q) for x, y, z in zip(a[k, i], b[k, i], c[k, i])]
                    assert [int(v) for v in got[i]] == want, (op, wide, hex(q))


# ------------------------------------------------------------------------------------------
# the host's admission predicates themselves
# ------------------------------------------------------------------------------------------
def test_host_admission_predicates_are_the_restated_ones(tmp_path):
    """tests/cpp/admission_driver.cpp: the product's host code computes lazy_terms, exact_terms, word_barrett, wide_ok (lr_host.hpp) and
    keymac_wide_ok (lr_abi_ckks.cpp) for every extension and key-switch admission set, and the recording launch stubs hand back what the
    launch structs carried; limit_moduli's Python restatement must say the same, on both sides of every bound.  (This is where a changed
    bound shows without a device: the sets are chosen so that one term more or less flips the value.)"""
    from host_stub_build import ASAN_UBSAN, run_host_driver
    logn = 12
    sets = [s for s in lm.admission_sets(logn).values() if s.kind in ("ext", "keymac")]
    args = []
    for s in sets:
        args += [s.kind, s.name, logn, len(s.moduli), len(s.P)] + ([s.terms] if s.kind == "ext" else []) + s.moduli + s.P
    stdout, _, _ = run_host_driver(tmp_path, "admission_driver", *ASAN_UBSAN, args=args, timeout=300, summary=False)      # (it prints no summary line)
    got = {}
    for ln in stdout.splitlines():
        f = ln.split()
        got[(f[1], f[2])] = [int(v) for v in f[3:]]
    for s in sets:
        if s.kind == "ext":
            for opt, narrow in (("default", False), ("ext_narrow", True)):
                want = [lm.lazy_terms(s.P), lm.exact_terms(s.P), lm.word_barrett(s.P), lm.wide_ok(s.moduli, narrow), s.terms]
                assert got[(s.name, opt)] == want, (s.name, opt)
        else:
            beta = -(-len(s.moduli) // len(s.P))
            assert beta == s.terms
            for opt, narrow in (("default", False), ("keymac_narrow", True)):
                want = [beta, int(lm.keymac_wide_ok(s.moduli, beta, narrow)), int(lm.keymac_wide_ok(s.P, beta, narrow))]
                assert got[(s.name, opt)] == want, (s.name, opt)
    assert len(got) == 2 * len(sets)

"""lr_setup on the device against the restatement over the CPU oracle (tests/setup_ref.py), bit for bit: CKG, the three rounds and the
finalize of RKG, the two rounds and the finalize of the naive RKG in both schemes' lines, the RTG share and its finalize, and the fold;
host and device-pointer randomness, the default shape and lr_options::no_epilogue (the reference's call-by-call shape), 1 and 3 parties
per call, keys shared by the call or one per party, on
  n16        N = 2^4, 2 + 1 limbs of Qi60 / Pi60, beta 2: less than one workgroup, the 60-bit transform route
  PN12QP109  N = 2^12, 2 + 1 limbs, beta 2: CKKS moduli, the FP64-butterfly route
  ragged     N = 2^11, the first 5 Q and both P of PN14QP438, beta 3: the last digit owns one row (the reference's break)
  PN14QP438  its moduli at N = 2^11, 10 + 2 limbs, beta 5, alpha 2
  n65536     N = 2^16, 2 + 1 limbs of PN16QP1761: one RTG share (the sub-block transform route and a 2^16 Galois gather); one party's CKG
             share, RKG rounds 1-3 and naive rounds 1-2 with their keys: the one degree at which a lane of the streaming kernels makes a
             second trip of its loop
The randomness carries every edge decision at fixed positions (setup_ref.inputs): the four ternary (coeff, sign) pairs, a bit plane of
all ones, the noise bytes (0, sign 0), (0, sign 1), (19, +-), (127, +-), with (0, sign 0) also on a last coefficient; crs and crp have
coefficients 0 and q_j - 1.  Outputs are pre-filled with a pattern; every input is compared unchanged afterwards.  33 shares in one fold
run its second pass; 70 parties in one call at n16 run the passes beyond the first 32; both in-place cases run; one chain runs on
device-made objects only; every refusal of the header that a context can be made for is exercised (N > 2^30 has none); one _device call replays from a HIP graph."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ckks_encoder_ref as encoder_ref
import setup_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = ref.PARTIES
SHAPES = ["n16", "PN12QP109", "ragged", "PN14QP438"]
_CACHE = {}


def _moduli(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    if name == "n65536":
        N, Q, P = pkg.params.ckks_moduli("PN16QP1761")
        return N, list(Q[:2]), list(P[:1])
    if name == "ragged":
        _, Q, P = pkg.params.ckks_moduli("PN14QP438")
        return 1 << 11, list(Q[:5]), list(P)
    N, Q, P = pkg.params.ckks_moduli(name)
    return (1 << 11 if name == "PN14QP438" else N), list(Q), list(P)


def _case(oracle, pkg, name):
    """the inputs of one shape, the secret and ephemeral keys, and a memo of the restatement's shares: want(kind, k, key) is party k's
    share computed with the keys of party `key` (the call's shared key, or k's own)"""
    if name in _CACHE:
        return _CACHE[name]
    N, Q, P = _moduli(pkg, name)
    st, ck = ref.Setup(oracle, N, Q, P, "bfv"), ref.Setup(oracle, N, Q, P, "ckks")
    gens = [5, pow(5, -1, 2 * N), 2 * N - 1]
    d = ref.inputs(N, Q, P, len(name), n_gens=len(gens))
    c = dict(d, N=N, Q=Q, P=P, beta=st.beta, rows=len(Q) + len(P), ref=st, gens=gens)
    c["sk"] = np.stack([st.ternary_ntt(d["sk_bits"][0][k], d["sk_bits"][1][k]) for k in range(K)])
    c["u"] = np.stack([st.ternary_ntt(d["u_bits"][0][k], d["u_bits"][1][k]) for k in range(K)])
    rng = np.random.default_rng(N + len(name))
    QP, beta = Q + P, st.beta
    # the aggregates a later round reads are inputs of that round: uniform polys serve, with the edge residues
    for k, members in (("pk0", None), ("r1_sum", beta), ("r2_sum", 2 * beta), ("r3_sum", beta), ("n1_sum", 2 * beta), ("n2_sum", 2 * beta)):
        c[k] = ref.edge_uniform(ref.uniform(rng, QP, N, members), QP)
    memo = {}

    def want(kind, k=0, key=0):
        m = (kind, k, key)
        if m in memo:
            return memo[m]
        sk, u, crp = c["sk"][key], c["u"][key], c["crp"]
        if kind == "ckg":
            r = st.ckg_share(sk, c["crs"], c["ckg_e"][k])
        elif kind == "r1":
            r = st.rkg_round1(u, sk, crp, c["r1_e"][k])
        elif kind == "r2":
            r = st.rkg_round2(c["r1_sum"], sk, crp, c["r2_e"][k])
        elif kind == "r3":
            r = st.rkg_round3(c["r2_sum"], u, sk, c["r3_e"][k])
        elif kind in ("n1_bfv", "n1_ckks"):
            r = (st if kind == "n1_bfv" else ck).naive_round1(sk, c["pk0"], c["crs"], c["n1_e"][k], c["n1_bits"][0][k], c["n1_bits"][1][k])
        elif kind == "n2":
            r = st.naive_round2(c["n1_sum"], sk, c["pk0"], c["crs"], c["n2_bits"][0][k], c["n2_bits"][1][k], c["n2_e"][k])
        elif kind == "rtg":                      # k = the index of the Galois element; party 0's bytes of that element
            r = st.rtg_share(c["sk"][0], gens[k], crp, c["rtg_e"][k][0])
        elif kind == "rlk":
            r = st.rkg_key(c["r2_sum"], c["r3_sum"])
        elif kind == "rlk_naive":
            r = st.naive_key(c["n2_sum"])
        else:                                    # "rot": Finalize of r1_sum standing as an aggregate RTG share
            r = st.rtg_key(c["r1_sum"], crp)
        memo[m] = r
        return r
    c["want"] = want
    _CACHE[name] = c
    return c


def _bytes_on_device(ring, cQ, arrays):
    """byte arrays one behind the other in device memory (a one-limb poly used as a plain buffer); returns the poly and the pointers"""
    N = cQ.N
    flat = np.concatenate([np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in arrays])
    words = -(-flat.size // (8 * N)) * N
    buf = np.zeros(words * 8, dtype=np.uint8)
    buf[:flat.size] = flat
    poly = ring.Poly(cQ, 1, words // N).set(buf.view(np.uint64).reshape(words // N, 1, N))
    ptrs, off = [], 0
    for a in arrays:
        ptrs.append(poly.device_ptr + off)
        off += np.asarray(a).size
    return poly, ptrs


def _rings(ring, c, no_epilogue):
    opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
    return opt, ring.NewContextWithParams(c["N"], c["Q"], options=opt), ring.NewContextWithParams(c["N"], c["P"], options=opt)


def _pattern(batch, limbs, N):
    return (np.arange(batch * limbs * N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).reshape(batch, limbs, N)


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("n", [1, K])
@pytest.mark.parametrize("name", SHAPES)
def test_shares_against_the_restatement(gpu_pkg, oracle, name, n, shared):
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, name)
    N, rows, beta, want = c["N"], c["rows"], c["beta"], c["want"]
    kb = 1 if shared else n
    key = (lambda k: 0) if shared else (lambda k: k)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        st = ring.Setup(cQ, cP, n, options=opt)
        assert st.beta == beta and st.rows == rows
        qp = lambda x: ring.Poly(cQ, rows, x.shape[0]).set(x) if x.ndim == 3 else ring.Poly(cQ, rows, 1).set(x[None])
        rand = {"ckg": c["ckg_e"][:n], "r1": c["r1_e"][:n], "r2": c["r2_e"][:n], "r3": c["r3_e"][:n], "n1": c["n1_e"][:n],
                "n1c": c["n1_bits"][0][:n], "n1s": c["n1_bits"][1][:n], "n2": c["n2_e"][:n], "n2c": c["n2_bits"][0][:n],
                "n2s": c["n2_bits"][1][:n], "rtg": c["rtg_e"][:n, 0]}
        names = list(rand)
        keep, ptr_list = _bytes_on_device(ring, cQ, [rand[k] for k in names])
        ptr = dict(zip(names, ptr_list))
        inputs = {k: qp(c[k]) for k in ("crs", "crp", "pk0", "r1_sum", "r2_sum", "r3_sum", "n1_sum", "n2_sum")}
        sk, u, sk0 = qp(c["sk"][:kb]), qp(c["u"][:kb]), qp(c["sk"][:1])
        pk = (inputs["pk0"], inputs["crs"])
        for on_device in (False, True):
            where = (name, n, shared, no_epilogue, on_device)
            r = (lambda k: ptr[k]) if on_device else (lambda k: rand[k])
            dev = "Device" if on_device else ""
            call = lambda fn, *args: getattr(st, fn + dev)(*args)
            new = lambda members: [ring.Poly(cQ, rows, members).set(_pattern(members, rows, N)) for _ in range(n)]

            def check(shares, kind, what):
                for k, s in enumerate(shares):
                    assert np.array_equal(s.get(), want(kind, k, key(k))), where + (what, k)
            # CKG
            share = ring.Poly(cQ, rows, n).set(_pattern(n, rows, N))
            call("CkgShare", sk, inputs["crs"], r("ckg"), share)
            got = share.get().reshape(n, rows, N)
            for k in range(n):
                assert np.array_equal(got[k], want("ckg", k, key(k))), where + ("ckg", k)
            # RKG, three rounds
            check(call("RkgRound1", u, sk, inputs["crp"], r("r1"), new(beta)), "r1", "round 1")
            check(call("RkgRound2", inputs["r1_sum"], sk, inputs["crp"], r("r2"), new(2 * beta)), "r2", "round 2")
            check(call("RkgRound3", inputs["r2_sum"], u, sk, r("r3"), new(beta)), "r3", "round 3")
            # RKG, naive, both schemes' round one
            bits1, bits2 = (r("n1c"), r("n1s")), (r("n2c"), r("n2s"))
            check(call("RkgNaiveRound1", st.BFV, sk, pk, r("n1"), bits1, new(2 * beta)), "n1_bfv", "naive round 1, dbfv")
            check(call("RkgNaiveRound1", st.CKKS, sk, pk, r("n1"), bits1, new(2 * beta)), "n1_ckks", "naive round 1, dckks")
            check(call("RkgNaiveRound2", inputs["n1_sum"], sk, pk, bits2, r("n2"), new(2 * beta)), "n2", "naive round 2")
            # RTG: n Galois elements in one call, one secret key
            if not shared:
                shares = call("RtgShare", sk0, c["gens"][:n], inputs["crp"], r("rtg"), new(beta))
                for j, s in enumerate(shares):
                    assert np.array_equal(s.get(), want("rtg", j)), where + ("rtg", c["gens"][j])
        # the finalize steps and the fold have no randomness
        where = (name, n, shared, no_epilogue)
        if n == K and not shared:
            evk = st.RkgKey(inputs["r2_sum"], inputs["r3_sum"], st.NewPairShare().set(_pattern(2 * beta, rows, N)))
            assert np.array_equal(evk.get(), want("rlk")), where + ("rlk",)
            evk = st.RkgNaiveKey(inputs["n2_sum"], st.NewPairShare().set(_pattern(2 * beta, rows, N)))
            assert np.array_equal(evk.get(), want("rlk_naive")), where + ("naive rlk",)
            rot = st.RtgKey(inputs["r1_sum"], inputs["crp"], st.NewPairShare().set(_pattern(2 * beta, rows, N)))
            assert np.array_equal(rot.get(), want("rot")), where + ("rot",)
            for a in (c["r2_sum"], c["n2_sum"]):       # in place: evk_out == round2
                r2 = qp(a)
                if a is c["r2_sum"]:
                    st.RkgKey(r2, inputs["r3_sum"], r2)
                    assert np.array_equal(r2.get(), want("rlk")), where + ("rlk in place",)
                else:
                    st.RkgNaiveKey(r2, r2)
                    assert np.array_equal(r2.get(), want("rlk_naive")), where + ("naive rlk in place",)
            # the fold over polys of batch 1, beta and 2 beta; out a fresh poly, and out == a share
            for k_in, members in (("pk0", 1), ("r1_sum", beta), ("r2_sum", 2 * beta)):
                terms = [c[k_in], c["crs"] if members == 1 else c[{beta: "r3_sum", 2 * beta: "n1_sum"}[members]],
                         c["sk"][1] if members == 1 else c[{beta: "crp", 2 * beta: "n2_sum"}[members]]]
                sum_want = c["ref"].aggregate(terms)
                polys = [qp(t) for t in terms]
                out = st.Aggregate(polys, ring.Poly(cQ, rows, members).set(_pattern(members, rows, N)))
                assert np.array_equal(out.get().reshape(sum_want.shape), sum_want), where + ("fold", members)
                for p, t in zip(polys, terms):
                    assert np.array_equal(p.get().reshape(t.shape), t), where + ("a share changed", members)
                st.Aggregate(polys, polys[1])
                assert np.array_equal(polys[1].get().reshape(sum_want.shape), sum_want), where + ("fold in place", members)
        for k, p in inputs.items():
            assert np.array_equal(p.get().reshape(c[k].shape), c[k]), where + (k, "changed")
        assert np.array_equal(sk.get().reshape(kb, rows, N), c["sk"][:kb]) and np.array_equal(u.get().reshape(kb, rows, N), c["u"][:kb])
        del keep


def test_one_rtg_share_at_n65536(gpu_pkg, oracle):
    """the sub-block transform route and a 2^16 Galois gather, in both shapes"""
    ring = gpu_pkg.ring
    N, Q, P = _moduli(gpu_pkg, "n65536")
    r = ref.Setup(oracle, N, Q, P, "bfv")
    rng = np.random.default_rng(65536)
    QP, rows, beta = Q + P, len(Q) + len(P), r.beta
    sk = r.ternary_ntt(ref.draw(rng, (N >> 3,)), ref.draw(rng, (N >> 3,)))
    crp, e = ref.edge_uniform(ref.uniform(rng, QP, N, beta), QP), ref.edge_noise(ref.draw(rng, shape_noise=(1, beta, N)))
    want = r.rtg_share(sk, 5, crp, e[0])
    for no_epilogue in (False, True):
        opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
        cQ, cP = ring.NewContextWithParams(N, Q, options=opt), ring.NewContextWithParams(N, P, options=opt)
        st = ring.Setup(cQ, cP, 1, options=opt)
        share = st.RtgShare(st.NewPoly().set(sk[None]), [5], st.NewShare().set(crp), e, [st.NewShare().set(_pattern(beta, rows, N))])[0]
        assert np.array_equal(share.get(), want), no_epilogue


def test_one_party_through_every_round_at_n65536(gpu_pkg, oracle):
    """two trips of the streaming loops in the CKG pass, the five share kinds beside RTG and the key pass, in both shapes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n65536")
    N, rows, beta, want = c["N"], c["rows"], c["beta"], c["want"]
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        st = ring.Setup(cQ, cP, 1, options=opt)
        qp = lambda x: ring.Poly(cQ, rows, x.shape[0]).set(x) if x.ndim == 3 else ring.Poly(cQ, rows, 1).set(x[None])
        new = lambda members: [ring.Poly(cQ, rows, members).set(_pattern(members, rows, N))]
        inputs = {k: qp(c[k]) for k in ("crs", "crp", "pk0", "r1_sum", "r2_sum", "r3_sum", "n1_sum", "n2_sum")}
        sk, u, pk = qp(c["sk"][:1]), qp(c["u"][:1]), (inputs["pk0"], inputs["crs"])
        share = st.CkgShare(sk, inputs["crs"], c["ckg_e"][:1], ring.Poly(cQ, rows, 1).set(_pattern(1, rows, N)))
        assert np.array_equal(share.get().reshape(rows, N), want("ckg")), no_epilogue
        got = {"r1": st.RkgRound1(u, sk, inputs["crp"], c["r1_e"][:1], new(beta)),
               "r2": st.RkgRound2(inputs["r1_sum"], sk, inputs["crp"], c["r2_e"][:1], new(2 * beta)),
               "r3": st.RkgRound3(inputs["r2_sum"], u, sk, c["r3_e"][:1], new(beta)),
               "n1_bfv": st.RkgNaiveRound1(st.BFV, sk, pk, c["n1_e"][:1], (c["n1_bits"][0][:1], c["n1_bits"][1][:1]), new(2 * beta)),
               "n2": st.RkgNaiveRound2(inputs["n1_sum"], sk, pk, (c["n2_bits"][0][:1], c["n2_bits"][1][:1]), c["n2_e"][:1], new(2 * beta))}
        for kind, shares in got.items():
            assert np.array_equal(shares[0].get(), want(kind)), (kind, no_epilogue)
        evk = st.RkgKey(inputs["r2_sum"], inputs["r3_sum"], st.NewPairShare().set(_pattern(2 * beta, rows, N)))
        assert np.array_equal(evk.get(), want("rlk")), no_epilogue
        evk = st.RkgNaiveKey(inputs["n2_sum"], st.NewPairShare().set(_pattern(2 * beta, rows, N)))
        assert np.array_equal(evk.get(), want("rlk_naive")), no_epilogue


def test_thirty_three_shares_in_one_fold(gpu_pkg, oracle):
    """more than the 32 shares of one pass: the running sum goes through the pool; out fresh and out == the last share"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P, rows, beta = c["N"], c["Q"], c["P"], c["rows"], c["beta"]
    terms = ref.uniform(np.random.default_rng(33), Q + P, N, 33 * 2 * beta).reshape(33, 2 * beta, rows, N)
    terms[5, 1, :, 3] = np.array(Q + P, dtype=np.uint64)       # a share may hold the residue q_j itself
    want = c["ref"].aggregate(list(terms))
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        st = ring.Setup(cQ, cP, 1, options=opt)
        polys = [st.NewPairShare().set(t) for t in terms]
        out = st.Aggregate(polys, st.NewPairShare().set(_pattern(2 * beta, rows, N)))
        assert np.array_equal(out.get(), want), no_epilogue
        st.Aggregate(polys, polys[32])
        assert np.array_equal(polys[32].get(), want), (no_epilogue, "in place")
        assert np.array_equal(polys[0].get(), terms[0])


MANY = 70      # more than the 32 parties of one pass: passes of 32, 32 and 6


def test_more_parties_than_one_pass(gpu_pkg, oracle):
    """n16 with max_batch = n = 70: every offset a later pass adds -- into the noise bytes, the bit planes, the per-party keys, the Galois
    elements, the share array -- and the pool's reuse across passes, in both shapes, host and device-pointer bytes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P, beta, rows, r = c["N"], c["Q"], c["P"], c["beta"], c["rows"], c["ref"]
    rng = np.random.default_rng(4343)
    sk = np.stack([r.ternary_ntt(ref.draw(rng, (N >> 3,)), ref.draw(rng, (N >> 3,))) for _ in range(MANY)])
    u = np.roll(sk, 1, axis=0)
    e1, e2 = ref.draw(rng, shape_noise=(MANY, beta, N)), ref.draw(rng, shape_noise=(MANY, beta, 2, N))
    bits = (ref.draw(rng, (MANY, beta, N >> 3)), ref.draw(rng, (MANY, beta, N >> 3)))
    cycle = [5, pow(5, -1, 2 * N), 2 * N - 1, 1, 25, 13, 7]
    gens = [cycle[k % len(cycle)] for k in range(MANY)]
    want = {"r1": [r.rkg_round1(u[k], sk[k], c["crp"], e1[k]) for k in range(MANY)],
            "n2": [r.naive_round2(c["n1_sum"], sk[k], c["pk0"], c["crs"], bits[0][k], bits[1][k], e2[k]) for k in range(MANY)],
            "rtg": [r.rtg_share(sk[0], gens[k], c["crp"], e1[k]) for k in range(MANY)]}
    assert not np.array_equal(want["r1"][32], want["r1"][64]) and not np.array_equal(want["n2"][33], want["n2"][34])
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        st = ring.Setup(cQ, cP, MANY, options=opt)
        qp = lambda x: ring.Poly(cQ, rows, x.shape[0]).set(x)
        keep, ptrs = _bytes_on_device(ring, cQ, [e1, e2, bits[0], bits[1]])
        dsk, du, dsk0, crp, crs, pk0, n1 = qp(sk), qp(u), qp(sk[:1]), qp(c["crp"]), qp(c["crs"][None]), qp(c["pk0"][None]), qp(c["n1_sum"])
        for on_device in (False, True):
            new = lambda members: [ring.Poly(cQ, rows, members).set(_pattern(members, rows, N)) for _ in range(MANY)]
            if on_device:
                got = {"r1": st.RkgRound1Device(du, dsk, crp, ptrs[0], new(beta)),
                       "n2": st.RkgNaiveRound2Device(n1, dsk, (pk0, crs), (ptrs[2], ptrs[3]), ptrs[1], new(2 * beta)),
                       "rtg": st.RtgShareDevice(dsk0, gens, crp, ptrs[0], new(beta))}
            else:
                got = {"r1": st.RkgRound1(du, dsk, crp, e1, new(beta)), "n2": st.RkgNaiveRound2(n1, dsk, (pk0, crs), bits, e2, new(2 * beta)),
                       "rtg": st.RtgShare(dsk0, gens, crp, e1, new(beta))}
            for kind, shares in got.items():
                for k in range(MANY):
                    assert np.array_equal(shares[k].get(), want[kind][k]), (no_epilogue, on_device, kind, k)
        assert np.array_equal(dsk.get(), sk)
        del keep


def test_ckg_without_p(gpu_pkg, oracle):
    """ctxP == NULL is the reference's "P is empty": CKG and its fold over Q, everything else refused"""
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "n16")
    N, Q = c["N"], c["Q"]
    r = ref.Setup(oracle, N, Q, [], "bfv")
    cQ = ring.NewContextWithParams(N, Q)
    st = ring.Setup(cQ, None, K)
    sk = np.stack([r.ternary_ntt(c["sk_bits"][0][k], c["sk_bits"][1][k]) for k in range(K)])
    crs = c["crs"][:len(Q)]
    share = st.CkgShare(st.NewPoly(K).set(sk), st.NewPoly().set(crs[None]), c["ckg_e"], st.NewPoly(K))
    want = np.stack([r.ckg_share(sk[k], crs, c["ckg_e"][k]) for k in range(K)])
    assert np.array_equal(share.get().reshape(want.shape), want)
    parts = [st.NewPoly().set(w[None]) for w in want]
    assert np.array_equal(st.Aggregate(parts, st.NewPoly()).get(), r.aggregate(list(want)))
    one = st.NewPoly()
    # st.NewShare and st.RkgRound1 are refused by the Python mirror (Setup.beta) in the same words, before any C call ...
    for call in (st.NewShare, lambda: st.RkgKey(one, one, one), lambda: st.RkgNaiveKey(one, one), lambda: st.RtgKey(one, one, one),
                 lambda: st.RkgRound1(one, one, one, c["ckg_e"][:1], [one])):
        with pytest.raises(nat.LatticeRingError, match="modulus P is empty") as e:
            call()
        assert e.value.code == 4
    # ... so the C refusal of every share call is reached through the library itself, in both forms
    L, check = nat.lib(), nat.check
    b, h, arr, g = np.zeros(64, dtype=np.uint8).ctypes.data_as(C.c_void_p), one.h, (C.c_void_p * 1)(one.h.value), (C.c_uint64 * 1)(5)
    raw = {"rkg_round1": (h, h, h, b, 1, arr), "rkg_round2": (h, h, h, b, 1, arr), "rkg_round3": (h, h, h, b, 1, arr),
           "rkg_naive_round1": (0, h, h, h, b, b, b, 1, arr), "rkg_naive_round2": (h, h, h, h, b, b, b, 1, arr), "rtg_share": (h, g, 1, h, b, arr)}
    for name, args in raw.items():
        for form in ("", "_device"):
            with pytest.raises(nat.LatticeRingError, match="modulus P is empty") as e:
                check(getattr(L, "lr_setup_" + name + form)(st.h, *args))
            assert e.value.code == 4, name + form


def test_staging_is_reused_across_consecutive_host_calls(gpu_pkg, oracle):
    """two host-form calls one behind the other with different bytes, no synchronisation between them: the second waits for the first
    one's copy out of the pinned buffer before it refills it"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "PN12QP109")
    rows = c["rows"]
    _, cQ, cP = _rings(ring, c, False)
    st = ring.Setup(cQ, cP, 1)
    sk, u = (ring.Poly(cQ, rows, 1).set(c[k][:1]) for k in ("sk", "u"))
    crp = st.NewShare().set(c["crp"])
    shares = [st.NewShare(), st.NewShare()]
    for k in range(2):
        st.RkgRound1(u, sk, crp, c["r1_e"][k:k + 1], [shares[k]])
    for k in range(2):
        assert np.array_equal(shares[k].get(), c["want"]("r1", k, 0)), k


def test_chain_on_device_made_objects_only(gpu_pkg, oracle):
    """three parties: secret and ephemeral keys (lr_keygen) -> CKG, three-round RKG, one RTG key (lr_setup) -> Encode -> Encrypt under the
    collective pk -> MulRelin -> Rotate -> Decrypt under the sum of the secret keys, all on the device from setup_ref's bytes: every
    collective key and the decrypted plaintext poly equal the restatement's bit for bit"""
    ring = gpu_pkg.ring
    N, Q, P = gpu_pkg.params.ckks_moduli(ref.CHAIN_PARAMS)
    Q, P = list(Q), list(P)
    level, roots = len(Q) - 1, encoder_ref.roots_table(N)
    w = ref.oracle_chain(oracle, N, Q, P, 0, roots)
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    kg, st, plan = ring.KeyGenerator(cQ, cP, K), ring.Setup(cQ, cP, K), ring.CkksPlan(cQ, cP, 1)
    enc, coder = ring.CkksEncryptor(cQ, cP, 1), ring.CkksEncoder(cQ, 1, roots)
    sk, u = kg.GenSecretKey(w["sk_bits"], kg.NewKey(K)), kg.GenSecretKey(w["u_bits"], kg.NewKey(K))
    assert np.array_equal(sk.get(), w["sk"]) and np.array_equal(u.get(), w["u"])
    member = lambda p, k: ring.Poly.wrap(cQ, p.device_ptr + k * p.limbs * N * 8, p.limbs, 1)
    crs, crp, crp_rot = st.NewPoly().set(w["crs"][None]), st.NewShare().set(w["crp"]), st.NewShare().set(w["crp_rot"][0])
    ckg = st.CkgShare(sk, crs, w["ckg_e"], st.NewPoly(K))
    pk0 = st.Aggregate([member(ckg, k) for k in range(K)], st.NewPoly())
    assert np.array_equal(pk0.get(), w["pk0"])
    shares = lambda make: [make() for _ in range(K)]
    r1 = st.Aggregate(st.RkgRound1(u, sk, crp, w["r1_e"], shares(st.NewShare)), st.NewShare())
    r2 = st.Aggregate(st.RkgRound2(r1, sk, crp, w["r2_e"], shares(st.NewPairShare)), st.NewPairShare())
    r3 = st.Aggregate(st.RkgRound3(r2, u, sk, w["r3_e"], shares(st.NewShare)), st.NewShare())
    rlk = st.RkgKey(r2, r3, r2)
    assert np.array_equal(rlk.get(), w["rlk"])
    rtg = [st.RtgShare(member(sk, k), [ref.CHAIN_GEN], crp_rot, w["rtg_e"][0][k:k + 1], [st.NewShare()])[0] for k in range(K)]
    rot = st.RtgKey(st.Aggregate(rtg, st.NewShare()), crp_rot, plan.NewSwitchingKey())
    assert np.array_equal(rot.get(), w["rot"][0])
    one = lambda x: np.asarray(x)[None]
    cts = []
    for k in ("x", "y"):
        pt = coder.Encode(cQ.NewPoly(), one(w[k]), level, ref.CHAIN_SCALE)
        cts.append(enc.EncryptPk((pk0, crs), (one(w[k + "_u"][0]), one(w[k + "_u"][1])), (one(w[k + "_e"][0]), one(w[k + "_e"][1])), pt,
                                 (cQ.NewPoly(), cQ.NewPoly()), level, fast=False))
    for ct, want in zip(cts, w["cts"]):
        assert np.array_equal(ct[0].get(), want[0]) and np.array_equal(ct[1].get(), want[1])
    ct, out = (cQ.NewPoly(), cQ.NewPoly()), (cQ.NewPoly(), cQ.NewPoly())
    plan.MulRelin(level, cts[0], cts[1], rlk, ct)
    plan.PermuteNTT(level, ct, ref.CHAIN_GEN, rot, out)
    sk_sum = st.Aggregate([member(sk, k) for k in range(K)], st.NewPoly())
    assert np.array_equal(sk_sum.get(), w["sk_sum"])
    pt = cQ.NewPoly()
    plan.Decrypt(level, out, sk_sum, pt)
    assert np.array_equal(pt.get()[:level + 1], w["pt"])


def test_refusals(gpu_pkg, oracle):
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P, beta, rows = c["N"], c["Q"], c["P"], c["beta"], c["rows"]
    cQ, cP, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, Q)

    def code(f, *args, **kw):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args, **kw)
        return e.value.code
    ARG, SHAPE = 4, 3
    # creation: as lr_keygen_create
    assert code(ring.Setup, cQ, cP, 0) == ARG and code(ring.Setup, cQ, cP, 65536) == ARG                    # max_batch outside 1 .. 65535
    assert code(ring.Setup, ring.NewContextWithParams(4, Q), None, 1) == ARG                                # N < 8
    assert code(ring.Setup, cQ, ring.NewContextWithParams(2 * N, P), 1) == ARG                              # ctxP with another N
    if nat.device_count() > 1:
        assert code(ring.Setup, cQ, ring.NewContextWithParams(N, P, device=1), 1) == ARG                    # ctxP on another device
    # more than 64 limbs in Q||P: 64 limbs of Q and one of P; the handle pointer stays NULL; without the ctxP the same ring makes a handle.
    # (The header's other LR_ERR_UNSUPPORTED, N > 2^30, has no context to be tried with: see the header.)
    UNSUPPORTED = 6
    wide = ring.NewContextWithParams(N, list(gpu_pkg.params.Qi60()[:64]))
    assert code(ring.Setup, wide, cP, 1) == UNSUPPORTED
    out = C.c_void_p(0x1234)
    assert nat.lib().lr_setup_create(wide.h, cP.h, 1, C.byref(out)) == UNSUPPORTED and not out.value
    assert ring.Setup(wide, None, 1).rows == 64
    L = nat.lib()
    assert L.lr_setup_create(None, cP.h, 1, C.byref(C.c_void_p())) == ARG and L.lr_setup_create(cQ.h, cP.h, 1, None) == ARG
    assert L.lr_setup_destroy(None) == 0
    st = ring.Setup(cQ, cP, 2)
    P1 = lambda ctx=cQ, batch=1, limbs=rows: ring.Poly(ctx, limbs, batch)
    sk, u, crs, crp, pk = P1(batch=2), P1(batch=2), P1(), st.NewShare(), (P1(), P1())
    r1, r2, r3 = st.NewShare(), st.NewPairShare(), st.NewShare()
    s1, s2 = [st.NewShare(), st.NewShare()], [st.NewPairShare(), st.NewPairShare()]
    e1, e2 = c["r1_e"][:2], c["r2_e"][:2]
    bits = (c["n1_bits"][0][:2], c["n1_bits"][1][:2])
    inside = lambda p, m=0: ring.Poly.wrap(cQ, p.device_ptr + m * rows * N * 8, rows, 1)
    # CKG
    assert code(st.CkgShare, P1(other, 2), crs, c["ckg_e"][:2], P1(batch=2)) == ARG and code(st.CkgShare, sk, P1(other), c["ckg_e"][:2], P1(batch=2)) == ARG
    assert code(st.CkgShare, sk, crs, c["ckg_e"][:2], P1(other, 2)) == ARG                                  # a poly of another context
    assert code(st.CkgShare, sk, crs, c["ckg_e"][:2], sk) == ARG and code(st.CkgShare, sk, inside(sk), c["ckg_e"][:2], sk) == ARG   # the output is an input
    assert code(st.CkgShare, P1(batch=2, limbs=rows - 1), crs, c["ckg_e"][:2], P1(batch=2)) == SHAPE        # too few limbs
    assert code(st.CkgShare, P1(batch=3), crs, c["ckg_e"], P1(batch=3)) == SHAPE                            # batch > max_batch
    assert code(st.CkgShare, P1(batch=3), crs, c["ckg_e"][:2], P1(batch=2)) == SHAPE                        # a key whose batch is neither 1 nor n
    # the rounds: contexts, limbs, batches, overlaps
    for fn, args, out in ((st.RkgRound1, lambda **k: (k.get("u", u), k.get("sk", sk), k.get("crp", crp), e1), s1),
                          (st.RkgRound2, lambda **k: (k.get("in", r1), k.get("sk", sk), k.get("crp", crp), e2), s2),
                          (st.RkgRound3, lambda **k: (k.get("in", r2), k.get("u", u), k.get("sk", sk), e1), s1)):
        members = out[0].batch
        assert code(fn, *args(sk=P1(other, 2)), out) == ARG, fn.__name__
        assert code(fn, *args(sk=P1(batch=2, limbs=rows - 1)), out) == SHAPE
        assert code(fn, *args(sk=P1(batch=3)), out) == SHAPE                                                # neither 1 nor n
        assert code(fn, *args(), [out[0], out[0]]) == ARG                                                   # two outputs share memory
        assert code(fn, *args(), [out[0], ring.Poly(other, rows, members)]) == ARG
        assert code(fn, *args(), [out[0], P1(batch=members + 1)]) == SHAPE                                  # a share whose batch is not beta / 2 beta
        assert code(fn, *args(), [out[0], P1(batch=members, limbs=rows - 1)]) == SHAPE
        one_party = args(sk=inside(out[0]), u=P1())                                                         # one party: keys of batch 1
        assert code(fn, *one_party[:3], one_party[3][:1], [out[0]]) == ARG                                  # an output is an input
        if fn.__name__ != "RkgRound3":
            assert code(fn, *args(crp=P1(batch=beta + 1)), out) == SHAPE and code(fn, *args(crp=ring.Poly(other, rows, beta)), out) == ARG
        if fn.__name__ != "RkgRound1":
            assert code(fn, *args(**{"in": P1(batch=3 * beta)}), out) == SHAPE                              # the aggregate's batch
    three = [st.NewShare() for _ in range(3)]
    assert code(st.RkgRound1, u, sk, crp, c["r1_e"], three) == SHAPE                                        # n > max_batch
    # the naive rounds
    assert code(st.RkgNaiveRound1, 2, sk, pk, e2, bits, s2) == ARG                                          # an unknown scheme
    assert code(st.RkgNaiveRound1, st.BFV, sk, (pk[0], P1(batch=2)), e2, bits, s2) == SHAPE                 # pk has batch 1
    assert code(st.RkgNaiveRound1, st.BFV, sk, (P1(other), pk[1]), e2, bits, s2) == ARG
    assert code(st.RkgNaiveRound1, st.CKKS, sk, pk, e2, bits, [s2[0], s2[0]]) == ARG
    assert code(st.RkgNaiveRound1, st.BFV, sk, pk, e2, bits, s1) == SHAPE                                   # shares of beta polys where pairs are due
    assert code(st.RkgNaiveRound2, r1, sk, pk, bits, e2, s2) == SHAPE                                       # round1 is not a share of pairs
    assert code(st.RkgNaiveRound2, r2, sk, (inside(s2[0]), pk[1]), bits, e2, s2) == ARG                     # an output is an input
    # the finalize steps
    assert code(st.RkgKey, r2, r3, st.NewShare()) == SHAPE and code(st.RkgKey, r1, r3, st.NewPairShare()) == SHAPE
    assert code(st.RkgKey, r2, r3, ring.Poly(other, rows, 2 * beta)) == ARG
    assert code(st.RkgKey, r2, r3, ring.Poly.wrap(cQ, r2.device_ptr, rows, 2 * beta - 1)) == SHAPE
    shifted = ring.Poly(cQ, rows, 2 * beta + 1)
    a, b = ring.Poly.wrap(cQ, shifted.device_ptr, rows, 2 * beta), ring.Poly.wrap(cQ, shifted.device_ptr + rows * N * 8, rows, 2 * beta)
    assert code(st.RkgKey, a, r3, b) == ARG and code(st.RkgNaiveKey, a, b) == ARG                           # a partial overlap
    assert code(st.RkgKey, r2, inside(r2, 1), r2) == SHAPE and code(st.RkgKey, r2, r3, ring.Poly.wrap(cQ, r3.device_ptr, rows, beta)) == SHAPE
    big = ring.Poly(cQ, rows, 3 * beta)
    assert code(st.RkgKey, r2, ring.Poly.wrap(cQ, big.device_ptr, rows, beta), ring.Poly.wrap(cQ, big.device_ptr, rows, 2 * beta)) == ARG   # evk is round3
    assert code(st.RtgKey, ring.Poly.wrap(cQ, big.device_ptr, rows, beta), crp, ring.Poly.wrap(cQ, big.device_ptr, rows, 2 * beta)) == ARG
    assert code(st.RtgKey, r2, crp, st.NewPairShare()) == SHAPE
    # RTG
    sk1 = P1()
    assert code(st.RtgShare, sk1, [5, 6], crp, e1, s1) == ARG and code(st.RtgShare, sk1, [0, 5], crp, e1, s1) == ARG   # an even Galois element
    assert code(st.RtgShare, sk, [5, 25], crp, e1, s1) == SHAPE                                             # one secret key
    assert code(st.RtgShare, sk1, [5, 25, 125], crp, c["r1_e"], three) == SHAPE                             # n_keys > max_batch
    # the fold
    assert code(st.Aggregate, [r1, r2], st.NewShare()) == SHAPE and code(st.Aggregate, [r1, ring.Poly(other, rows, beta)], st.NewShare()) == ARG
    assert code(st.Aggregate, [P1(batch=3 * beta)], P1(batch=3 * beta)) == SHAPE                            # neither 1, beta nor 2 beta
    assert code(st.Aggregate, [a], b) == ARG                                                                # a partial overlap
    assert L.lr_setup_aggregate(st.h, (C.c_void_p * 1)(r1.h.value), 0, r1.h) == SHAPE
    assert L.lr_setup_aggregate(st.h, (C.c_void_p * 1)(None), 1, r1.h) == ARG and L.lr_setup_aggregate(st.h, None, 1, r1.h) == ARG
    # ctxQ and ctxP on different streams: every entry point refuses
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0                                            # hipStreamNonBlocking
    cQ.SetStream(stream.value)
    try:
        with pytest.raises(nat.LatticeRingError, match="different streams"):
            st.RkgRound1(u, sk, crp, e1, s1)
        assert code(st.CkgShare, sk, crs, c["ckg_e"][:2], P1(batch=2)) == ARG and code(st.RkgRound2, r1, sk, crp, e2, s2) == ARG
        assert code(st.RkgRound3, r2, u, sk, e1, s1) == ARG and code(st.RkgKey, r2, r3, r2) == ARG and code(st.RkgNaiveKey, r2, r2) == ARG
        assert code(st.RkgNaiveRound1, st.BFV, sk, pk, e2, bits, s2) == ARG and code(st.RkgNaiveRound2, r2, sk, pk, bits, e2, s2) == ARG
        assert code(st.RtgShare, sk1, [5, 25], crp, e1, s1) == ARG and code(st.RtgKey, r1, crp, st.NewPairShare()) == ARG
        assert code(st.Aggregate, [r1, r3], st.NewShare()) == ARG and code(st.RkgRound1Device, u, sk, crp, 0x1000, s1) == ARG
    finally:
        cQ.Sync()
        cQ.SetStream(None)
        assert hip.hipStreamDestroy(stream) == 0
    # raw calls: NULL arguments and counts < 1
    bb = np.zeros(1024, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    arr1, arr2 = (C.c_void_p * 2)(s1[0].h.value, s1[1].h.value), (C.c_void_p * 2)(s2[0].h.value, s2[1].h.value)
    g2 = (C.c_uint64 * 2)(5, 25)
    h = lambda p: p.h
    calls = [("ckg_share", [st.h, h(sk), h(crs), bb, 2, h(P1(batch=2))], 4), ("rkg_round1", [st.h, h(u), h(sk), h(crp), bb, 2, arr1], 5),
             ("rkg_round2", [st.h, h(r1), h(sk), h(crp), bb, 2, arr2], 5), ("rkg_round3", [st.h, h(r2), h(u), h(sk), bb, 2, arr1], 5),
             ("rkg_naive_round1", [st.h, 0, h(sk), h(pk[0]), h(pk[1]), bb, bb, bb, 2, arr2], 8),
             ("rkg_naive_round2", [st.h, h(r2), h(sk), h(pk[0]), h(pk[1]), bb, bb, bb, 2, arr2], 8),
             ("rtg_share", [st.h, h(sk1), g2, 2, h(crp), bb, arr1], 3)]
    for name, args, count in calls:
        for fn in (getattr(L, "lr_setup_" + name), getattr(L, "lr_setup_" + name + "_device")):
            for i in range(len(args)):
                if i != count and not isinstance(args[i], int):
                    assert fn(*[None if j == i else x for j, x in enumerate(args)]) == ARG, (fn.__name__, i)
            for bad in (0, -1):
                assert fn(*[bad if j == count else x for j, x in enumerate(args)]) == SHAPE, (fn.__name__, bad)
    assert L.lr_setup_rkg_round1(st.h, h(u), h(sk), h(crp), bb, 2, (C.c_void_p * 2)(s1[0].h.value, None)) == ARG
    for fn, args in ((L.lr_setup_rkg_key, [st.h, h(r2), h(r3), h(r2)]), (L.lr_setup_rkg_naive_key, [st.h, h(r2), h(r2)]),
                     (L.lr_setup_rtg_key, [st.h, h(r1), h(crp), h(st.NewPairShare())])):
        for i in range(len(args)):
            assert fn(*[None if j == i else x for j, x in enumerate(args)]) == ARG, (fn.__name__, i)
    # the handle stays usable after its refusals
    dsk, du, dcrp = P1(batch=2).set(c["sk"][:2]), P1(batch=2).set(c["u"][:2]), st.NewShare().set(c["crp"])
    got = st.RkgRound1(du, dsk, dcrp, e1, s1)
    for k in range(2):
        assert np.array_equal(got[k].get(), c["want"]("r1", k, k)), ("after the refusals", k)


def test_device_form_replays_from_a_hip_graph(gpu_pkg):
    """tests/_setup_graph_worker.py, in its own process because torch's HIP runtime has to come up before the library's"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_setup_graph_worker.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "graph replay ok" in res.stdout

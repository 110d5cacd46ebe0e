"""lr_refresh on the device against the restatement over the CPU oracle (tests/refresh_ref.py), bit for bit: GenShares, Recode, Finalize of
dckks and dbfv and the fold, host and device-pointer randomness, the default shape and lr_options::no_epilogue (the reference's
call-by-call shape), batch 1 and 3, keys shared by the batch or one per ciphertext, on the shapes of test_gpu_collective.py:
  n16                  N = 2^4, 2 + 1 limbs of Qi60 / Pi60, both schemes; levelStart 0, 1 (1 and 2 mask words)
  ckks PN12QP109       N = 2^12, 2 limbs; levelStart 0, 1
  ckks PN13QP218       N = 2^13, 6 limbs; levelStart 0, 3, 5 = L: 1, 2 and 3 mask words
  ckks PN14QP438       its moduli at N = 2^11, 10 limbs; levelStart 0 and 9 (6 words)
  bfv PN12QP109, PN13QP218, PN14QP438 (N = 2^11, |P| = 2)
  n65536               N = 2^16, 2 limbs of CKKS PN16QP1761: one shares + finalize, batch 1; with its P limb, one dbfv shares + finalize:
                       the one degree at which a lane of the streaming kernels makes a second trip of its loop
and beyond them 20 limbs of Qi60 at N = 2^4 (Recode with more than 16 digits per coefficient) and handles of max_batch 5 at batches 1, 3.
The noise carries the edge decisions (0, +) (0, -) (19, +-) (127, +-) at fixed positions, with (0, sign 0) also on the last coefficient of
another batch member; the CKKS masks 0, +-1, +-(2^64 - 1), +-2^64, the largest and smallest W-word values and a multiple of q_i; the
integers Recode lifts 0, 1, (Q_ls - 1) / 2 - 1, (Q_ls - 1) / 2, (Q_ls + 1) / 2, Q_ls - 1; the BFV mask 0 and t - 1; c1 coefficients 0 and
q_j - 1.  Outputs are pre-filled with a pattern (limbs above levelStart keep it); every input is compared unchanged afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import keygen_ref
import refresh_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 3
T = ref.BFV_T
CKKS_SHAPES = {"n16": [0, 1], "PN12QP109": [0, 1], "PN13QP218": [0, 3, 5], "PN14QP438": [0, 9]}
CKKS_WORDS = {"n16": [1, 2], "PN12QP109": [1, 2], "PN13QP218": [1, 2, 3], "PN14QP438": [1, 6]}
BFV_SHAPES = ["n16", "PN12QP109", "PN13QP218", "PN14QP438"]
_CACHE = {}


def _moduli(pkg, scheme, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    if name == "n65536":
        N, Q, P = pkg.params.ckks_moduli("PN16QP1761")
        return N, list(Q[:2]), list(P[:1])
    if scheme == "ckks":
        N, Q, P = pkg.params.ckks_moduli(name)
    else:
        N, Q, P, _ = pkg.params.bfv_moduli(name)
    return (1 << 11 if name == "PN14QP438" else N), list(Q), list(P)


def _edge_masks(rng, Q, ls, N):
    W = ref.mask_words(Q, ls)
    top = 1 << (64 * W - 1)
    edges = [v for v in (0, 1, -1, (1 << 64) - 1, -((1 << 64) - 1), 1 << 64, -(1 << 64), top - 1, -top, 3 * Q[0], -5 * Q[-1]) if -top <= v < top]
    bound = ref.product(Q[:ls + 1]) // 6
    return (edges + ref.draw_mask(rng, bound, N))[:N]


def _edge_integers(rng, Q, ls, N):
    Qls = ref.product(Q[:ls + 1])
    hand = [0, 1, (Qls - 1) // 2 - 1, (Qls - 1) // 2, (Qls + 1) // 2, Qls - 1]
    return (hand + [int.from_bytes(rng.bytes(8 * len(Q) + 8), "little") % Qls for _ in range(N)])[:N]


def _case(oracle, pkg, scheme, name):
    """inputs of one shape and a cache of the restatement's results, each computed once; key = the index of the batch member whose secret
    key is used (0 when the batch shares it)"""
    if (scheme, name) in _CACHE:
        return _CACHE[(scheme, name)]
    N, Q, P = _moduli(pkg, scheme, name)
    QP, nQ = Q + P, len(Q)
    rng = np.random.default_rng(len(name) * 1000 + N + (9 if scheme == "bfv" else 4))
    kg = keygen_ref.KeyGenerator(oracle, N, Q, P, scheme)
    r = ref.Refresh(oracle, N, Q, P, T if scheme == "bfv" else 0)
    bits = lambda: (keygen_ref.draw(rng, (N >> 3,)), keygen_ref.draw(rng, (N >> 3,)))
    k = 1 if name == "n65536" else K
    c = {"N": N, "Q": Q, "P": P, "ref": r, "k": k}
    c["sk"] = np.stack([kg.gen_secret_key(*bits()) for _ in range(k)])
    c1 = keygen_ref.uniform(rng, Q, N, k)
    c1[0][:, 1] = 0
    c1[0][:, 2] = np.array(Q, dtype=np.uint64) - np.uint64(1)
    c["c1"] = c1
    c["crs"] = keygen_ref.uniform(rng, QP if scheme == "bfv" else Q, N, k)
    c["c0"] = keygen_ref.uniform(rng, Q, N, k)
    c["dec"], c["rec"] = keygen_ref.uniform(rng, Q, N, k), keygen_ref.uniform(rng, Q, N, k)     # what a fold of shares may hold
    e = ref.regular_bytes(rng, (2, k, N))
    for x in e:
        x[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
        x[k - 1, N - 1] = 0                                              # (0, sign 0) on the last coefficient of another batch member
    c["e"] = e
    if scheme == "ckks":
        levels = [nQ - 1] if name == "n65536" else CKKS_SHAPES[name]
        c["mask"] = {ls: [_edge_masks(rng, Q, ls, N) for _ in range(k)] for ls in levels}
        # the sums c0 + dec that Recode lifts: the hand-set integers at the first coefficients; c0 is chosen to produce them
        c["sum"], c["c0_at"] = {}, {}
        for ls in levels:
            s = np.stack([r.cQ.ntt(r.set_coefficients_bigint(_edge_integers(rng, Q, ls, N), ls + 1)) for _ in range(k)])
            c["sum"][ls] = s
            c["c0_at"][ls] = np.stack([r.cQ.ewise("SUB", s[b], c["dec"][b][:ls + 1]) for b in range(k)])
    else:
        mask = rng.integers(0, T, (k, N)).astype(np.uint64)
        mask[0, :2] = [0, T - 1]
        c["mask"] = mask
    memo = {}

    def want(kind, ls, b, key=0):
        m = (kind, ls, b, key)
        if m not in memo:
            if kind == "shares" and scheme == "ckks":
                memo[m] = r.ckks_gen_shares(ls, c["sk"][key], c1[b], c["crs"][b], c["mask"][ls][b], e[0, b], e[1, b])
            elif kind == "shares":
                memo[m] = r.bfv_gen_shares(c["sk"][key], c1[b], c["crs"][b], c["mask"][b], e[0, b], e[1, b])
            elif kind == "recode":
                memo[m] = r.ckks_recode(c["sum"][ls][b])
            elif scheme == "ckks":
                memo[m] = r.ckks_finalize(ls, c["c0_at"][ls][b], c["dec"][b], c["rec"][b])
            else:
                memo[m] = r.bfv_finalize(c["c0"][b], c["crs"][b], c["dec"][b], c["rec"][b])
        return memo[m]
    c["want"] = want
    _CACHE[(scheme, name)] = c
    return c


def _on_device(ring, cQ, arrays):
    """arrays one behind the other in device memory, each from a 16-byte boundary (a one-limb poly used as a plain buffer)"""
    N = cQ.N
    chunks = []
    for a in arrays:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        chunks.append(np.concatenate([raw, np.zeros(-raw.size % 16, dtype=np.uint8)]))
    flat = np.concatenate(chunks)
    words = -(-flat.size // (8 * N)) * N
    buf = np.zeros(words * 8, dtype=np.uint8)
    buf[:flat.size] = flat
    poly = ring.Poly(cQ, 1, words // N).set(buf.view(np.uint64).reshape(words // N, 1, N))
    ptrs, off = [], 0
    for ch in chunks:
        ptrs.append(poly.device_ptr + off)
        off += ch.size
    return poly, ptrs


def _rings(ring, c, no_epilogue, with_p):
    opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
    cQ = ring.NewContextWithParams(c["N"], c["Q"], options=opt)
    return opt, cQ, ring.NewContextWithParams(c["N"], c["P"], options=opt) if with_p else None


def _pattern(batch, limbs, N):
    return (np.arange(batch * limbs * N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).reshape(batch, limbs, N)


def _get(p):
    return p.get().reshape(p.batch, -1, p.N)


def _run_ckks(ring, oracle, pkg, name, n, shared):
    c = _case(oracle, pkg, "ckks", name)
    N, Q, nQ, want = c["N"], c["Q"], len(c["Q"]), c["want"]
    kb = 1 if shared else n
    pat = _pattern(n, nQ, N)
    for no_epilogue in (False, True):
        opt, cQ, _ = _rings(ring, c, no_epilogue, False)
        r = ring.Refresh(cQ, None, 0, n, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        sk, c1, crs = qp(c["sk"][:kb, :nQ]), qp(c["c1"][:n]), qp(c["crs"][:n])
        dec_in, rec_in = qp(c["dec"][:n]), qp(c["rec"][:n])
        for ls, words in zip(CKKS_SHAPES[name], CKKS_WORDS[name]):
            assert r.MaskWords(ls) == words == ref.mask_words(Q, ls)
            planes = pkg.sampling.mask_word_planes(c["mask"][ls][:n], words)
            rand = [planes, c["e"][0, :n], c["e"][1, :n]]
            keep, ptrs = _on_device(ring, cQ, rand)
            for on_device in (False, True):
                where = (name, n, shared, no_epilogue, on_device, ls)
                dec, rec = qp(pat), qp(pat)
                if on_device:
                    r.CkksGenSharesDevice(sk, ls, c1, crs, ptrs[0], ptrs[1:], (dec, rec))
                else:
                    r.CkksGenShares(sk, ls, c1, crs, planes, rand[1:], (dec, rec))
                gd, gr = _get(dec), _get(rec)
                for b in range(n):
                    w = want("shares", ls, b, 0 if shared else b)
                    assert np.array_equal(gd[b, :ls + 1], w[0]), where + ("share_decrypt", b)
                    assert np.array_equal(gr[b], w[1]), where + ("share_recrypt", b)
                assert np.array_equal(gd[:, ls + 1:], pat[:, ls + 1:]), where + ("limbs above levelStart were written",)
            del keep
            where = (name, n, shared, no_epilogue, ls)
            summed, c0 = qp(c["sum"][ls][:n]), qp(c["c0_at"][ls][:n])
            out, fin = r.CkksRecode(ls, summed, qp(pat)), r.CkksFinalize(ls, c0, (dec_in, rec_in), qp(pat))
            go, gf = _get(out), _get(fin)
            for b in range(n):
                assert np.array_equal(go[b], want("recode", ls, b)), where + ("recode", b)
                assert np.array_equal(gf[b], want("finalize", ls, b)), where + ("finalize", b)
            assert np.array_equal(_get(summed), c["sum"][ls][:n]) and np.array_equal(_get(c0), c["c0_at"][ls][:n]), "an input changed"
            if ls == nQ - 1:                                             # in place: out = in, out0 = c0
                assert np.array_equal(_get(r.CkksRecode(ls, summed, summed)), go), where + ("recode in place",)
                assert np.array_equal(_get(r.CkksFinalize(ls, c0, (dec_in, rec_in), c0)), gf), where + ("finalize in place",)
        assert np.array_equal(_get(sk), c["sk"][:kb, :nQ]) and np.array_equal(_get(c1), c["c1"][:n]), "sk or c1 changed"
        assert np.array_equal(_get(crs), c["crs"][:n]), "crs changed"
        assert np.array_equal(_get(dec_in), c["dec"][:n]) and np.array_equal(_get(rec_in), c["rec"][:n]), "a share changed"


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("n", [1, K])
@pytest.mark.parametrize("name", list(CKKS_SHAPES))
def test_ckks_against_the_restatement(gpu_pkg, oracle, name, n, shared):
    _run_ckks(gpu_pkg.ring, oracle, gpu_pkg, name, n, shared)


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("n", [1, K])
@pytest.mark.parametrize("name", BFV_SHAPES)
def test_bfv_against_the_restatement(gpu_pkg, oracle, name, n, shared):
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "bfv", name)
    N, nQ, rows, want = c["N"], len(c["Q"]), len(c["Q"]) + len(c["P"]), c["want"]
    kb = 1 if shared else n
    pat = _pattern(n, nQ, N)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue, True)
        r = ring.Refresh(cQ, cP, T, n, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        sk, c1, crs, c0 = qp(c["sk"][:kb]), qp(c["c1"][:n]), qp(c["crs"][:n]), qp(c["c0"][:n])
        dec_in, rec_in = qp(c["dec"][:n]), qp(c["rec"][:n])
        rand = [c["mask"][:n], c["e"][0, :n], c["e"][1, :n]]
        keep, ptrs = _on_device(ring, cQ, rand)
        for on_device in (False, True):
            where = (name, n, shared, no_epilogue, on_device)
            dec, rec = qp(pat), qp(pat)
            if on_device:
                r.BfvGenSharesDevice(sk, c1, crs, ptrs[0], ptrs[1:], (dec, rec))
            else:
                r.BfvGenShares(sk, c1, crs, rand[0], rand[1:], (dec, rec))
            gd, gr = _get(dec), _get(rec)
            for b in range(n):
                w = want("shares", None, b, 0 if shared else b)
                assert np.array_equal(gd[b], w[0]), where + ("share_decrypt", b)
                assert np.array_equal(gr[b], w[1]), where + ("share_recrypt", b)
        del keep
        out = r.BfvFinalize(c0, crs, (dec_in, rec_in), (qp(pat), qp(pat)))
        g0, g1 = _get(out[0]), _get(out[1])
        for b in range(n):
            w = want("finalize", None, b)
            assert np.array_equal(g0[b], w[0]) and np.array_equal(g1[b], w[1]), (name, n, no_epilogue, "finalize", b)
        assert np.array_equal(_get(sk), c["sk"][:kb]) and np.array_equal(_get(c1), c["c1"][:n]) and np.array_equal(_get(crs), c["crs"][:n])
        assert np.array_equal(_get(c0), c["c0"][:n]) and np.array_equal(_get(dec_in), c["dec"][:n]) and np.array_equal(_get(rec_in), c["rec"][:n])
        assert np.array_equal(_get(r.BfvFinalize(c0, crs, (dec_in, rec_in), (c0, qp(pat)))[0]), g0), "finalize with out0 = c0"


def test_one_ckks_refresh_at_n65536(gpu_pkg, oracle):
    """the sub-block transform route, in both shapes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", "n65536")
    N, Q, nQ = c["N"], c["Q"], len(c["Q"])
    ls = nQ - 1
    w, wf = c["want"]("shares", ls, 0, 0), c["want"]("finalize", ls, 0)
    planes = gpu_pkg.sampling.mask_word_planes(c["mask"][ls], ref.mask_words(Q, ls))
    for no_epilogue in (False, True):
        opt, cQ, _ = _rings(ring, c, no_epilogue, False)
        r = ring.Refresh(cQ, None, 0, 1, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        dec, rec = r.CkksGenShares(qp(c["sk"][:, :nQ]), ls, qp(c["c1"]), qp(c["crs"]), planes, (c["e"][0], c["e"][1]),
                                   (qp(_pattern(1, nQ, N)), qp(_pattern(1, nQ, N))))
        assert np.array_equal(dec.get(), w[0]) and np.array_equal(rec.get(), w[1]), no_epilogue
        fin = r.CkksFinalize(ls, qp(c["c0_at"][ls]), (qp(c["dec"]), qp(c["rec"])), qp(_pattern(1, nQ, N)))
        assert np.array_equal(fin.get(), wf), no_epilogue


def test_one_bfv_refresh_at_n65536(gpu_pkg, oracle):
    """two trips of the streaming loops in the products in front of the inverse transforms and in both modes of the lift, in both shapes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "bfv", "n65536")
    N, nQ = c["N"], len(c["Q"])
    w, wf = c["want"]("shares", None, 0, 0), c["want"]("finalize", None, 0)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue, True)
        r = ring.Refresh(cQ, cP, T, 1, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        dec, rec = r.BfvGenShares(qp(c["sk"]), qp(c["c1"]), qp(c["crs"]), c["mask"], (c["e"][0], c["e"][1]),
                                  (qp(_pattern(1, nQ, N)), qp(_pattern(1, nQ, N))))
        assert np.array_equal(_get(dec)[0], w[0]) and np.array_equal(_get(rec)[0], w[1]), no_epilogue
        out = r.BfvFinalize(qp(c["c0"]), qp(c["crs"]), (qp(c["dec"]), qp(c["rec"])), (qp(_pattern(1, nQ, N)), qp(_pattern(1, nQ, N))))
        assert np.array_equal(_get(out[0])[0], wf[0]) and np.array_equal(_get(out[1])[0], wf[1]), no_epilogue


def test_recode_beyond_sixteen_digits(gpu_pkg, oracle):
    """levelStart 16 and 19 = L on 20 limbs of Qi60 at N = 2^4 (16 and 19 mask words): more than 16 digits per coefficient take the
    kernel's 64-lane instantiation; Recode and Finalize in both shapes against the restatement"""
    ring = gpu_pkg.ring
    N, Q = 1 << 4, list(gpu_pkg.params.Qi60()[:20])
    nQ, rng = len(Q), np.random.default_rng(61)
    r = ref.Refresh(oracle, N, Q)
    dec, rec = keygen_ref.uniform(rng, Q, N, 2), keygen_ref.uniform(rng, Q, N, 2)
    for ls, words in ((16, 16), (19, 19)):
        summed = np.stack([r.cQ.ntt(r.set_coefficients_bigint(_edge_integers(rng, Q, ls, N), ls + 1)) for _ in range(2)])
        c0 = np.stack([r.cQ.ewise("SUB", summed[b], dec[b][:ls + 1]) for b in range(2)])
        want = [r.ckks_recode(summed[b]) for b in range(2)]
        want_fin = [r.ckks_finalize(ls, c0[b], dec[b], rec[b]) for b in range(2)]
        for no_epilogue in (False, True):
            opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
            cQ = ring.NewContextWithParams(N, Q, options=opt)
            h = ring.Refresh(cQ, None, 0, 2, options=opt)
            assert h.MaskWords(ls) == words == ref.mask_words(Q, ls)
            qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
            got = _get(h.CkksRecode(ls, qp(summed), qp(_pattern(2, nQ, N))))
            fin = _get(h.CkksFinalize(ls, qp(c0), (qp(dec), qp(rec)), qp(_pattern(2, nQ, N))))
            for b in range(2):
                assert np.array_equal(got[b], want[b]), (ls, no_epilogue, "recode", b)
                assert np.array_equal(fin[b], want_fin[b]), (ls, no_epilogue, "finalize", b)


@pytest.mark.parametrize("n", [1, K])
def test_a_batch_below_max_batch(gpu_pkg, oracle, n):
    """handles made for max_batch 5 run batches of 1 and 3: the three pools lie back to back at the CALL's batch, which the transforms
    over 2 and 3 times the batch rely on.  CKKS PN12QP109 at levelStart 0 and 1 and BFV PN12QP109, shares and Finalize, both shapes"""
    ring = gpu_pkg.ring
    for scheme in ("ckks", "bfv"):
        c = _case(oracle, gpu_pkg, scheme, "PN12QP109")
        N, Q, nQ, want = c["N"], c["Q"], len(c["Q"]), c["want"]
        pat = _pattern(n, nQ, N)
        for no_epilogue in (False, True):
            opt, cQ, cP = _rings(ring, c, no_epilogue, scheme == "bfv")
            h = ring.Refresh(cQ, cP, T if scheme == "bfv" else 0, 5, options=opt)
            qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
            sk, c1, crs = qp(c["sk"][:n] if scheme == "bfv" else c["sk"][:n, :nQ]), qp(c["c1"][:n]), qp(c["crs"][:n])
            e = (c["e"][0, :n], c["e"][1, :n])
            for ls in (CKKS_SHAPES["PN12QP109"] if scheme == "ckks" else [None]):
                where = (scheme, n, no_epilogue, ls)
                dec, rec = qp(pat), qp(pat)
                if scheme == "ckks":
                    planes = gpu_pkg.sampling.mask_word_planes(c["mask"][ls][:n], h.MaskWords(ls))
                    h.CkksGenShares(sk, ls, c1, crs, planes, e, (dec, rec))
                    fin = _get(h.CkksFinalize(ls, qp(c["c0_at"][ls][:n]), (qp(c["dec"][:n]), qp(c["rec"][:n])), qp(pat)))
                else:
                    h.BfvGenShares(sk, c1, crs, c["mask"][:n], e, (dec, rec))
                    out = h.BfvFinalize(qp(c["c0"][:n]), crs, (qp(c["dec"][:n]), qp(c["rec"][:n])), (qp(pat), qp(pat)))
                    fin = np.stack([_get(out[0]), _get(out[1])], axis=1)
                gd, gr = _get(dec), _get(rec)
                rows = nQ if ls is None else ls + 1
                for b in range(n):
                    w = want("shares", ls, b, b)
                    assert np.array_equal(gd[b, :rows], w[0]) and np.array_equal(gr[b], w[1]), where + ("shares", b)
                    assert np.array_equal(fin[b], want("finalize", ls, b)), where + ("finalize", b)


@pytest.mark.parametrize("name,counts,batch", [("n16", [1, 2, 3, 33], 2), ("PN13QP218", [3], 1)])
def test_the_fold(gpu_pkg, oracle, name, counts, batch):
    """Aggregate over n parties in one call: n - 1 Context.Add calls on the oracle, in the same order.  Two shares hold the residue q_j
    itself (what Neg leaves).  At the top level and at level 0, out fresh and out = shares[0]"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", name)
    N, Q, nQ, r = c["N"], c["Q"], len(c["Q"]), c["ref"]
    rng = np.random.default_rng(78)
    most = max(counts)
    shares = [keygen_ref.uniform(rng, Q, N, batch) for _ in range(most)]
    shares[0][:, :, 0] = np.array(Q, dtype=np.uint64)
    shares[-1][:, :, 1] = np.array(Q, dtype=np.uint64)
    pat = _pattern(batch, nQ, N)
    for no_epilogue in (False, True):
        opt, cQ, _ = _rings(ring, c, no_epilogue, False)
        h = ring.Refresh(cQ, None, 0, batch, options=opt)
        qp = lambda x: ring.Poly(cQ, nQ, batch).set(x)
        for n in counts:
            for level in sorted({nQ - 1, 0}):
                want = np.stack([r.aggregate([s[b, :level + 1] for s in shares[:n]]) for b in range(batch)])
                for alias in ("fresh", "share0"):
                    where = (name, no_epilogue, n, level, alias)
                    dev = [qp(s) for s in shares[:n]]
                    out = qp(pat) if alias == "fresh" else dev[0]
                    before = _get(out)
                    h.Aggregate(dev, out, level)
                    got = _get(out)
                    assert np.array_equal(got[:, :level + 1], want), where
                    assert np.array_equal(got[:, level + 1:], before[:, level + 1:]), where + ("limbs above the level were written",)
                    for k in range(1 if alias == "share0" else 0, n):
                        assert np.array_equal(_get(dev[k]), shares[k]), where + ("a share changed", k)


def _add_qp(ring, cQ, cP, a, b, out):
    nQ, nP, N = len(cQ.Modulus), len(cP.Modulus), cQ.N
    cQ.AddLvl(nQ - 1, a, b, out)
    wp = lambda p: ring.Poly.wrap(cP, p.device_ptr + 8 * nQ * N, nP, 1)
    cP.Add(wp(a), wp(b), wp(out))
    return out


@pytest.mark.parametrize("scheme,level_start", [("ckks", 0), ("ckks", 1), ("bfv", None)])
def test_chain_on_the_device_only(gpu_pkg, oracle, scheme, level_start):
    """three parties: secrets from lr_keygen summed on the device, the collective public key, a ciphertext from the device encryptor,
    three pairs of shares, the fold, Finalize, Decrypt, Decode -- the bytes of refresh_ref.refresh_inputs.  The refreshed ciphertext equals
    the oracle's bit for bit; BFV decodes to the product's plaintext exactly, CKKS within refresh_ref.REFRESH_TOLERANCE at level L"""
    import ckks_encoder_ref
    ring = gpu_pkg.ring
    if scheme == "ckks":
        N, Q, P = gpu_pkg.params.ckks_moduli(ref.REFRESH_PARAMS)
    else:
        N, Q, P, _ = gpu_pkg.params.bfv_moduli(ref.REFRESH_PARAMS)
    Q, P = list(Q), list(P)
    top, roots = len(Q) - 1, ckks_encoder_ref.roots_table(N) if scheme == "ckks" else None
    w = ref.oracle_refresh(oracle, scheme, N, Q, P, 0, level_start, roots)
    ls = w["level_start"]
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    kg, h = ring.KeyGenerator(cQ, cP, 1), ring.Refresh(cQ, cP, T if scheme == "bfv" else 0, 1)
    one = lambda x: np.asarray(x)[None]
    sks = [kg.GenSecretKey((one(b[0]), one(b[1])), kg.NewKey()) for b in w["sk_bits"]]
    sk = sks[0]
    for k in sks[1:]:
        sk = _add_qp(ring, cQ, cP, sk, k, kg.NewKey())
    pk = kg.GenPublicKey(sk, one(w["pk_e"]), (kg.NewKey(), kg.NewKey().set(w["pk1"])))
    assert np.array_equal(sk.get(), w["sk"]) and np.array_equal(pk[0].get(), w["pk0"])
    ct = (cQ.NewPoly(), cQ.NewPoly())
    u, e = (one(w["enc_u"][0]), one(w["enc_u"][1])), (one(w["enc_e"][0]), one(w["enc_e"][1]))
    out = (cQ.NewPoly(), cQ.NewPoly())
    if scheme == "ckks":
        coder = ring.CkksEncoder(cQ, 1, roots)
        ring.CkksEncryptor(cQ, cP, 1).EncryptPk(pk, u, e, coder.Encode(cQ.NewPoly(), one(w["values"]), top, ref.REFRESH_SCALE), ct, top, fast=False)
        assert np.array_equal(ct[1].get()[:ls + 1], w["ct"][1])
        crs = cQ.NewPoly().set(w["crs"])
        W = h.MaskWords(ls)
        shares = []
        for i in range(len(sks)):
            planes = gpu_pkg.sampling.mask_word_planes(w["mask"][i], W)
            shares.append(h.CkksGenShares(sks[i], ls, ct[1], crs, planes, (one(w["e"][i][0]), one(w["e"][i][1])), (cQ.NewPoly(), cQ.NewPoly())))
            assert np.array_equal(shares[i][0].get()[:ls + 1], w["shares"][i][0]) and np.array_equal(shares[i][1].get(), w["shares"][i][1]), i
        dec = h.Aggregate([s[0] for s in shares], cQ.NewPoly(), ls)
        rec = h.Aggregate([s[1] for s in shares], cQ.NewPoly(), top)
        h.CkksFinalize(ls, ct[0], (dec, rec), out[0])
        cQ.Copy(crs, out[1])                                             # ct[1] = crs.CopyNew()
        assert np.array_equal(out[0].get(), w["out"][0])
        pt = cQ.NewPoly()
        ring.CkksPlan(cQ, cP, 1).Decrypt(top, out, sk, pt)
        got = coder.Decode(pt, N >> 1, top, ref.REFRESH_SCALE).reshape(N >> 1)
        err = float(np.max(np.abs(got - w["values"])))
        print("device refresh levelStart %d: largest slot error %.6e (allowed %.6e)" % (ls, err, ref.REFRESH_TOLERANCE))
        assert err <= ref.REFRESH_TOLERANCE
    else:
        import bfv_encoder_ref
        coder = ring.BfvEncoder(cQ, T, 1)
        ring.BfvEncryptor(cQ, cP, 1).EncryptPk(pk, u, e, coder.EncodeUint(one(w["ints"]), cQ.NewPoly()), ct, fast=False)
        assert np.array_equal(ct[0].get(), w["fresh"][0]) and np.array_equal(ct[1].get(), w["fresh"][1])
        host = bfv_encoder_ref.Encoder(oracle, N, Q, T)
        row = host.cT.intt(host._scatter(w["factor"])[None])[0]
        f = cQ.NewPoly().set(np.broadcast_to(row, (len(Q), N)).copy())
        cQ.NTT(f, f)
        cQ.MForm(f, f)
        for p in ct:                                                     # the product that is refreshed
            cQ.NTT(p, p)
            cQ.MulCoeffsMontgomery(p, f, p)
            cQ.InvNTT(p, p)
        assert np.array_equal(ct[0].get(), w["ct"][0]) and np.array_equal(ct[1].get(), w["ct"][1])
        crs = kg.NewKey().set(w["crs"])
        shares = []
        for i in range(len(sks)):
            shares.append(h.BfvGenShares(sks[i], ct[1], crs, one(w["mask"][i]), (one(w["e"][i][0]), one(w["e"][i][1])), (cQ.NewPoly(), cQ.NewPoly())))
            assert np.array_equal(shares[i][0].get(), w["shares"][i][0]) and np.array_equal(shares[i][1].get(), w["shares"][i][1]), i
        dec = h.Aggregate([s[0] for s in shares], cQ.NewPoly(), top)
        rec = h.Aggregate([s[1] for s in shares], cQ.NewPoly(), top)
        h.BfvFinalize(ct[0], crs, (dec, rec), out)
        assert np.array_equal(out[0].get(), w["out"][0]) and np.array_equal(out[1].get(), w["out"][1])
        pt = cQ.NewPoly()
        ring.BfvDecryptor(cQ, 1).Decrypt(out, sk, pt)
        assert np.array_equal(coder.DecodeUint(pt).reshape(N), w["expected"])


def test_refusals(gpu_pkg, oracle):
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "bfv", "n16")
    N, Q, P = c["N"], c["Q"], c["P"]
    nQ, rows = len(Q), len(Q) + len(P)
    cQ, cP, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, Q)

    def code(f, *args, **kw):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args, **kw)
        return e.value.code
    ARG, SHAPE, UNSUPPORTED = 4, 3, 6
    # creation
    assert code(ring.Refresh, cQ, cP, T, 0) == ARG and code(ring.Refresh, cQ, cP, T, 65536) == ARG                     # max_batch outside 1 .. 65535
    assert code(ring.Refresh, ring.NewContextWithParams(4, Q), None, 0, 1) == ARG                                      # N < 8
    assert code(ring.Refresh, cQ, ring.NewContextWithParams(2 * N, P), T, 1) == ARG                                    # ctxP with another N
    if nat.device_count() > 1:
        assert code(ring.Refresh, cQ, ring.NewContextWithParams(N, P, device=1), T, 1) == ARG
    L = nat.lib()
    assert L.lr_refresh_create(None, cP.h, T, 1, C.byref(C.c_void_p())) == ARG and L.lr_refresh_create(cQ.h, cP.h, T, 1, None) == ARG
    assert L.lr_refresh_destroy(None) == 0
    h = ring.Refresh(cQ, cP, T, 2)
    key = lambda ctx, batch: ring.Poly(ctx, rows, batch)
    q = lambda ctx, batch: ring.Poly(ctx, nQ, batch)
    sk, c1, crs, crsq, dec, rec, out0 = key(cQ, 1), q(cQ, 2), key(cQ, 2), q(cQ, 2), q(cQ, 2), q(cQ, 2), q(cQ, 2)
    e, e3 = (c["e"][0, :2], c["e"][1, :2]), (c["e"][0], c["e"][1])
    bm, bm3 = c["mask"][:2], c["mask"]
    W = h.MaskWords(1)
    cm, cm3 = np.zeros((2, W, N), dtype=np.uint64), np.zeros((3, W, N), dtype=np.uint64)
    ck = lambda *a: h.CkksGenShares(a[0], 1, *a[1:])
    for f, m, m3, r_ in ((ck, cm, cm3, crsq), (h.BfvGenShares, bm, bm3, crs)):
        assert code(f, key(other, 1), c1, r_, m, e, (dec, rec)) == ARG and code(f, sk, q(other, 2), r_, m, e, (dec, rec)) == ARG   # another context
        assert code(f, sk, c1, key(other, 2), m, e, (dec, rec)) == ARG and code(f, sk, c1, r_, m, e, (dec, q(other, 2))) == ARG
        assert code(f, sk, c1, r_, m, e, (c1, rec)) == ARG and code(f, sk, c1, r_, m, e, (dec, r_)) == ARG                # an output is an input
        assert code(f, sk, c1, r_, m, e, (dec, dec)) == ARG                                                              # the two outputs share memory
        assert code(f, sk, c1, r_, m, e, (dec, ring.Poly(cQ, nQ - 1, 2))) == SHAPE                                        # too few limbs
        assert code(f, sk, q(cQ, 1), r_, m, e, (dec, rec)) == SHAPE                                                      # c1 must have the batch
        assert code(f, sk, c1, ring.Poly(cQ, rows, 1), m, e, (dec, rec)) == SHAPE                                         # crs must have the batch
        assert code(f, key(cQ, 3), q(cQ, 3), key(cQ, 3), m3, e3, (q(cQ, 3), q(cQ, 3))) == SHAPE                           # batch > max_batch
    assert code(h.BfvGenShares, q(cQ, 1), c1, crs, bm, e, (dec, rec)) == SHAPE                                            # sk without the rows of P
    assert code(h.BfvGenShares, sk, c1, crsq, bm, e, (dec, rec)) == SHAPE                                                 # crs without the rows of P
    assert code(h.CkksGenShares, sk, 2, c1, crsq, cm, e, (dec, rec)) == SHAPE and code(h.CkksGenShares, sk, -1, c1, crsq, cm, e, (dec, rec)) == SHAPE
    assert code(h.MaskWords, 2) == SHAPE and code(h.MaskWords, -1) == SHAPE
    # Recode and Finalize
    assert code(h.CkksRecode, 1, q(other, 2), out0) == ARG and code(h.CkksRecode, 1, c1, q(other, 2)) == ARG
    assert code(h.CkksRecode, 2, c1, out0) == SHAPE and code(h.CkksRecode, 0, c1, ring.Poly(cQ, 1, 2)) == SHAPE and code(h.CkksRecode, 1, q(cQ, 1), out0) == SHAPE
    inside = ring.Poly.wrap(cQ, out0.device_ptr + 8 * N, 1, 1)                                                            # limb 1 of out0
    assert code(h.CkksRecode, 0, inside, ring.Poly.wrap(cQ, out0.device_ptr, nQ, 1)) == ARG                               # a partial overlap
    assert code(h.CkksFinalize, 1, q(other, 2), (dec, rec), out0) == ARG and code(h.CkksFinalize, 1, c1, (dec, rec), q(other, 2)) == ARG
    assert code(h.CkksFinalize, 1, c1, (dec, rec), dec) == ARG and code(h.CkksFinalize, 1, c1, (dec, rec), rec) == ARG      # out0 is a share
    assert code(h.CkksFinalize, 2, c1, (dec, rec), out0) == SHAPE and code(h.CkksFinalize, 1, c1, (dec, q(cQ, 1)), out0) == SHAPE
    assert code(h.CkksFinalize, 0, c1, (dec, ring.Poly(cQ, 1, 2)), out0) == SHAPE                                         # share_recrypt below all of Q
    out1 = q(cQ, 2)
    assert code(h.BfvFinalize, q(other, 2), crs, (dec, rec), (out0, out1)) == ARG and code(h.BfvFinalize, c1, crs, (dec, rec), (out0, q(other, 2))) == ARG
    assert code(h.BfvFinalize, c1, crs, (dec, rec), (out0, out0)) == ARG and code(h.BfvFinalize, c1, crs, (dec, rec), (out0, c1)) == ARG
    assert code(h.BfvFinalize, c1, crs, (dec, rec), (dec, out1)) == ARG
    assert code(h.BfvFinalize, c1, crsq, (dec, rec), (out0, out1)) == SHAPE and code(h.BfvFinalize, c1, crs, (dec, rec), (out0, q(cQ, 1))) == SHAPE
    # the fold
    s2 = [q(cQ, 2), q(cQ, 2)]
    assert code(h.Aggregate, s2, q(other, 2), 1) == ARG and code(h.Aggregate, [s2[0], q(other, 2)], dec, 1) == ARG
    assert code(h.Aggregate, [ring.Poly.wrap(cQ, out0.device_ptr + 8 * N, nQ, 1)], ring.Poly.wrap(cQ, out0.device_ptr, nQ, 1), 1) == ARG
    assert code(h.Aggregate, s2, dec, 2) == SHAPE and code(h.Aggregate, [s2[0], q(cQ, 1)], dec, 1) == SHAPE
    assert code(h.Aggregate, s2, ring.Poly(cQ, nQ - 1, 2), 1) == SHAPE and code(h.Aggregate, [q(cQ, 3)], q(cQ, 3), 1) == SHAPE
    arr = (C.c_void_p * 2)(s2[0].h.value, s2[1].h.value)
    assert L.lr_refresh_aggregate(h.h, 1, arr, 0, dec.h) == SHAPE and L.lr_refresh_aggregate(h.h, 1, None, 2, dec.h) == ARG
    assert L.lr_refresh_aggregate(h.h, 1, (C.c_void_p * 2)(s2[0].h.value, None), 2, dec.h) == ARG
    assert L.lr_refresh_aggregate(None, 1, arr, 2, dec.h) == ARG and L.lr_refresh_aggregate(h.h, 1, arr, 2, None) == ARG
    # a handle without P or without t: the CKKS entry points only
    for hc in (ring.Refresh(cQ, None, 0, 2), ring.Refresh(cQ, cP, 0, 2), ring.Refresh(cQ, None, T, 2)):
        with pytest.raises(nat.LatticeRingError, match="CKKS entry points only"):
            hc.BfvGenShares(sk, c1, crs, bm, e, (dec, rec))
        assert code(hc.BfvFinalize, c1, crs, (dec, rec), (out0, out1)) == ARG
        hc.CkksGenShares(sk, 1, c1, crsq, cm, e, (dec, rec))
    # more than 64 limbs in Q||P: 64 limbs of Q and one of P
    assert code(ring.Refresh, ring.NewContextWithParams(N, list(gpu_pkg.params.Qi60()[:64])), cP, T, 1) == UNSUPPORTED
    # a Q_levelStart beyond 32 words: 40 limbs of 60 bits reach it from levelStart 34 on
    big = ring.NewContextWithParams(N, list(gpu_pkg.params.Qi60()[:40]))
    hb = ring.Refresh(big, None, 0, 1)
    assert hb.MaskWords(33) == 32 and code(hb.MaskWords, 34) == UNSUPPORTED
    p40 = lambda: ring.Poly(big, 40, 1)
    assert code(hb.CkksRecode, 34, p40(), p40()) == UNSUPPORTED and code(hb.CkksFinalize, 39, p40(), (p40(), p40()), p40()) == UNSUPPORTED
    m33 = np.zeros(33 * N, dtype=np.uint64).ctypes.data_as(C.c_void_p)
    b40 = np.zeros(N, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    assert L.lr_refresh_ckks_shares(hb.h, 34, p40().h, p40().h, p40().h, m33, b40, b40, 1, p40().h, p40().h) == UNSUPPORTED
    # misaligned _device masks
    buf = q(cQ, 2)
    assert code(h.CkksGenSharesDevice, sk, 1, c1, crsq, buf.device_ptr + 4, (buf.device_ptr, buf.device_ptr), (dec, rec)) == ARG
    assert code(h.BfvGenSharesDevice, sk, c1, crs, buf.device_ptr + 8, (buf.device_ptr, buf.device_ptr), (dec, rec)) == ARG
    # ctxQ and ctxP on different streams: every entry point refuses
    hip = C.CDLL("libamdhip64.so")
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0                                                              # hipStreamNonBlocking
    cQ.SetStream(st.value)
    try:
        with pytest.raises(nat.LatticeRingError, match="different streams"):
            h.BfvGenShares(sk, c1, crs, bm, e, (dec, rec))
        assert code(h.CkksGenShares, sk, 1, c1, crsq, cm, e, (dec, rec)) == ARG and code(h.CkksRecode, 1, c1, out0) == ARG
        assert code(h.CkksFinalize, 1, c1, (dec, rec), out0) == ARG and code(h.BfvFinalize, c1, crs, (dec, rec), (out0, out1)) == ARG
        assert code(h.Aggregate, s2, dec, 1) == ARG and code(ring.Refresh, cQ, cP, T, 1) == ARG
    finally:
        cQ.Sync()
        cQ.SetStream(None)
        assert hip.hipStreamDestroy(st) == 0
    # raw calls: NULL arguments and batches < 1
    b = np.zeros(512, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    p = lambda x: x.h
    calls = [("ckks_shares", [h.h, 1, p(sk), p(c1), p(crsq), b, b, b, 2, p(dec), p(rec)], 8, 1),
             ("bfv_shares", [h.h, p(sk), p(c1), p(crs), b, b, b, 2, p(dec), p(rec)], 7, None)]
    for name, args, count, lv in calls:
        for fn in (getattr(L, "lr_refresh_" + name), getattr(L, "lr_refresh_" + name + "_device")):
            for i in range(len(args)):
                if i not in (count, lv):
                    assert fn(*[None if j == i else x for j, x in enumerate(args)]) == ARG, (fn.__name__, i)
            for bad in (0, -1):
                assert fn(*[bad if j == count else x for j, x in enumerate(args)]) == SHAPE, (fn.__name__, bad)
    for fn, args, lv in ((L.lr_refresh_ckks_recode, [h.h, 1, p(c1), p(out0)], 1), (L.lr_refresh_ckks_finalize, [h.h, 1, p(c1), p(dec), p(rec), p(out0)], 1),
                         (L.lr_refresh_bfv_finalize, [h.h, p(c1), p(crs), p(dec), p(rec), p(out0), p(out1)], None)):
        for i in range(len(args)):
            if i != lv:
                assert fn(*[None if j == i else x for j, x in enumerate(args)]) == ARG, (fn.__name__, i)
    assert L.lr_refresh_mask_words(None, 0, C.byref(C.c_int())) == ARG and L.lr_refresh_mask_words(h.h, 0, None) == ARG
    # the handle stays usable after its refusals
    sk1, c1 = key(cQ, 1).set(c["sk"][:1]), c1.set(c["c1"][:2])
    crs.set(c["crs"][:2])
    h.BfvGenShares(sk1, c1, crs, bm, e, (dec, rec))
    for i in range(2):
        w = c["want"]("shares", None, i, 0)
        assert np.array_equal(dec.get()[i], w[0]) and np.array_equal(rec.get()[i], w[1]), i


def test_staging_is_reused_across_consecutive_host_calls(gpu_pkg, oracle):
    """two host-form calls one behind the other with different bytes, no synchronisation between them: the second waits for the first
    one's copy out of the pinned buffer before it refills it"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", "PN12QP109")
    Q, nQ = c["Q"], len(c["Q"])
    ls = nQ - 1
    _, cQ, _ = _rings(ring, c, False, False)
    h = ring.Refresh(cQ, None, 0, 1)
    qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
    sk = qp(c["sk"][:1, :nQ])
    c1, crs = [qp(c["c1"][b:b + 1]) for b in range(2)], [qp(c["crs"][b:b + 1]) for b in range(2)]
    shares = [(cQ.NewPoly(), cQ.NewPoly()) for _ in range(2)]
    W = ref.mask_words(Q, ls)
    for b in range(2):
        h.CkksGenShares(sk, ls, c1[b], crs[b], gpu_pkg.sampling.mask_word_planes(c["mask"][ls][b:b + 1], W),
                        (c["e"][0, b:b + 1], c["e"][1, b:b + 1]), shares[b])
    for b in range(2):
        w = c["want"]("shares", ls, b, 0)
        assert np.array_equal(shares[b][0].get(), w[0]) and np.array_equal(shares[b][1].get(), w[1]), b


def test_device_form_replays_from_a_hip_graph(gpu_pkg):
    """tests/_refresh_graph_worker.py, in its own process because torch's HIP runtime has to come up before the library's"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_refresh_graph_worker.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "graph replay ok" in res.stdout

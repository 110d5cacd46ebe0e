"""lr_collective on the device against the restatement over the CPU oracle (tests/collective_ref.py), bit for bit: CKS and PCKS shares of
dckks and dbfv and the n-ary fold, host and device-pointer randomness, the default shape and lr_options::no_epilogue (the reference's
call-by-call shape), batch 1 and 3, keys shared by the batch or one per ciphertext, on
  n16                  N = 2^4, 2 + 1 limbs of Qi60 / Pi60, both schemes: less than one workgroup, the 60-bit transform route
  ckks PN12QP109       N = 2^12, 2 + 1 limbs: the FP64-butterfly route; levels 0, 1
  ckks PN13QP218       N = 2^13, 6 + 1 limbs; levels 0, 3, 5
  ckks PN14QP438       its moduli at N = 2^11, 10 + 2 limbs, |P| = 2; levels 0, 9
  bfv PN12QP109, PN13QP218   2 + 1 and 3 + 1 limbs: 39- and 54-bit limbs
  bfv PN14QP438        its moduli at N = 2^11, 6 + 2 limbs, |P| = 2
  n65536               N = 2^16, 2 + 1 limbs of CKKS PN16QP1761: one CKS share, one PCKS share and a fold of 3 shares with a base, batch 1:
                       the sub-block transform route, and the one degree at which a lane of the streaming kernels makes a second trip
The noise carries the edge decisions (0, +) (0, -) (19, +-) (127, +-) at fixed positions, with (0, sign 0) also on the last coefficient of
another batch member; sk_in == sk_out on one NTT coefficient; c1 has coefficients 0 and q_j - 1.  Outputs are pre-filled with a pattern
(limbs above the level keep it); every input is compared unchanged afterwards.  The fold runs with 1, 2, 3 and 33 shares (a second pass),
with a base, with out aliasing shares[0] and with out aliasing the base.  One chain per scheme runs on the device only: keys from
lr_keygen, the ciphertext from the device encryptor, three shares, the fold, Decrypt, Decode.  Every refusal of the header is exercised;
one _device call replays from a HIP graph."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import collective_ref as ref
import keygen_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 3
CKKS_SHAPES = {"n16": [0, 1], "PN12QP109": [0, 1], "PN13QP218": [0, 3, 5], "PN14QP438": [0, 9]}
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


def _case(oracle, pkg, scheme, name):
    """inputs of one shape and a cache of the restatement's shares: want(kind, level, b, key) computes each once; key = the index of the
    batch member whose keys are used (0 when the batch shares them)"""
    if (scheme, name) in _CACHE:
        return _CACHE[(scheme, name)]
    N, Q, P = _moduli(pkg, scheme, name)
    QP, nQ = Q + P, len(Q)
    rng = np.random.default_rng(len(name) * 1000 + N + (7 if scheme == "bfv" else 3))
    kg, col = keygen_ref.KeyGenerator(oracle, N, Q, P, scheme), ref.Collective(oracle, N, Q, P)
    bits = lambda: (keygen_ref.draw(rng, (N >> 3,)), keygen_ref.draw(rng, (N >> 3,)))
    k = 1 if name == "n65536" else K
    c = {"N": N, "Q": Q, "P": P, "ref": col}
    c["sk_in"] = np.stack([kg.gen_secret_key(*bits()) for _ in range(k)])
    c["sk_out"] = np.stack([kg.gen_secret_key(*bits()) for _ in range(k)])
    c["sk_out"][0][:, 3] = c["sk_in"][0][:, 3]                            # Delta = CRed(q) = 0 on that coefficient
    c["pk1"] = keygen_ref.uniform(rng, QP, N, k)
    c["pk0"] = np.stack([kg.gen_public_key(kg.gen_secret_key(*bits()), keygen_ref.draw(rng, shape_noise=(N,)), c["pk1"][b]) for b in range(k)])
    c1 = keygen_ref.uniform(rng, Q, N, k)
    c1[0][:, 1] = 0
    c1[0][:, 2] = np.array(Q, dtype=np.uint64) - np.uint64(1)
    c["c1"] = c1
    c["uc"], c["us"] = keygen_ref.draw(rng, (k, N >> 3)), keygen_ref.draw(rng, (k, N >> 3))
    c["uc"][0, 0], c["us"][0, 0] = 0b10101010, 0b11001100
    e = ref.smudging_bytes(rng, (3, k, N))
    for x in e:
        x[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
        x[k - 1, N - 1] = 0                                              # (0, sign 0) on the last coefficient of another batch member
    c["e"] = e
    memo = {}

    def want(kind, level, b, key):
        m = (kind, level, b, key)
        if m not in memo:
            if kind == "cks" and scheme == "ckks":
                memo[m] = col.ckks_cks_share(level, c["sk_in"][key], c["sk_out"][key], c1[b], e[0, b])
            elif kind == "cks":
                memo[m] = col.bfv_cks_share(c["sk_in"][key], c["sk_out"][key], c1[b], e[0, b])
            elif scheme == "ckks":
                memo[m] = col.ckks_pcks_share(level, c["sk_in"][key], c["pk0"][key], c["pk1"][key], c1[b], c["uc"][b], c["us"][b], e[1, b], e[2, b])
            else:
                memo[m] = col.bfv_pcks_share(c["sk_in"][key], c["pk0"][key], c["pk1"][key], c1[b], c["uc"][b], c["us"][b], e[1, b], e[2, b])
        return memo[m]
    c["want"] = want
    _CACHE[(scheme, name)] = c
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


def _get(p):
    return p.get().reshape(p.batch, -1, p.N)


def _run_shares(ring, oracle, pkg, scheme, name, n, shared, levels):
    c = _case(oracle, pkg, scheme, name)
    N, nQ, rows, want = c["N"], len(c["Q"]), len(c["Q"]) + len(c["P"]), c["want"]
    kb = 1 if shared else n
    pat = _pattern(n, nQ, N)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        col = ring.Collective(cQ, cP, n, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        sk_in, sk_out, pk = qp(c["sk_in"][:kb]), qp(c["sk_out"][:kb]), (qp(c["pk0"][:kb]), qp(c["pk1"][:kb]))
        c1 = qp(c["c1"][:n])
        rand = [c["e"][0, :n], c["uc"][:n], c["us"][:n], c["e"][1, :n], c["e"][2, :n]]
        keep, ptrs = _bytes_on_device(ring, cQ, rand)
        for on_device in (False, True):
            for level in levels:
                where = (scheme, name, n, shared, no_epilogue, on_device, level)
                share, o0, o1 = qp(pat), qp(pat), qp(pat)
                if scheme == "ckks" and on_device:
                    col.CkksCksShareDevice(sk_in, sk_out, c1, ptrs[0], share, level)
                    col.CkksPcksShareDevice(sk_in, pk, c1, ptrs[1:3], ptrs[3:5], (o0, o1), level)
                elif scheme == "ckks":
                    col.CkksCksShare(sk_in, sk_out, c1, rand[0], share, level)
                    col.CkksPcksShare(sk_in, pk, c1, rand[1:3], rand[3:5], (o0, o1), level)
                elif on_device:
                    col.BfvCksShareDevice(sk_in, sk_out, c1, ptrs[0], share)
                    col.BfvPcksShareDevice(sk_in, pk, c1, ptrs[1:3], ptrs[3:5], (o0, o1))
                else:
                    col.BfvCksShare(sk_in, sk_out, c1, rand[0], share)
                    col.BfvPcksShare(sk_in, pk, c1, rand[1:3], rand[3:5], (o0, o1))
                got, g0, g1 = _get(share), _get(o0), _get(o1)
                for b in range(n):
                    key = 0 if shared else b
                    assert np.array_equal(got[b, :level + 1], want("cks", level, b, key)), where + ("cks", b)
                    w = want("pcks", level, b, key)
                    assert np.array_equal(g0[b, :level + 1], w[0]), where + ("pcks out0", b)
                    assert np.array_equal(g1[b, :level + 1], w[1]), where + ("pcks out1", b)
                for g in (got, g0, g1):
                    assert np.array_equal(g[:, level + 1:], pat[:, level + 1:]), where + ("limbs above the level were written",)
        assert np.array_equal(_get(sk_in), c["sk_in"][:kb]) and np.array_equal(_get(sk_out), c["sk_out"][:kb]), "a secret key changed"
        assert np.array_equal(_get(pk[0]), c["pk0"][:kb]) and np.array_equal(_get(pk[1]), c["pk1"][:kb]), "the public key changed"
        assert np.array_equal(_get(c1), c["c1"][:n]), "c1 changed"
        del keep


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("n", [1, K])
@pytest.mark.parametrize("name", list(CKKS_SHAPES))
def test_ckks_shares_against_the_restatement(gpu_pkg, oracle, name, n, shared):
    _run_shares(gpu_pkg.ring, oracle, gpu_pkg, "ckks", name, n, shared, CKKS_SHAPES[name])


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("n", [1, K])
@pytest.mark.parametrize("name", BFV_SHAPES)
def test_bfv_shares_against_the_restatement(gpu_pkg, oracle, name, n, shared):
    c = _case(oracle, gpu_pkg, "bfv", name)
    _run_shares(gpu_pkg.ring, oracle, gpu_pkg, "bfv", name, n, shared, [len(c["Q"]) - 1])


def test_one_cks_share_at_n65536(gpu_pkg, oracle):
    """the sub-block transform route, in both shapes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", "n65536")
    N, nQ, level = c["N"], len(c["Q"]), len(c["Q"]) - 1
    want = c["want"]("cks", level, 0, 0)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        col = ring.Collective(cQ, cP, 1, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        share = col.CkksCksShare(qp(c["sk_in"]), qp(c["sk_out"]), qp(c["c1"]), c["e"][0], qp(_pattern(1, nQ, N)), level)
        assert np.array_equal(share.get(), want), no_epilogue


def test_one_pcks_share_and_a_fold_at_n65536(gpu_pkg, oracle):
    """two trips of the streaming loops in the PCKS addend and the fold (3 shares and a base, the residue q_j on the last coefficient)"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", "n65536")
    N, Q, nQ, level = c["N"], c["Q"], len(c["Q"]), len(c["Q"]) - 1
    want = c["want"]("pcks", level, 0, 0)
    rng = np.random.default_rng(65536)
    shares, base = [keygen_ref.uniform(rng, Q, N, 1) for _ in range(3)], keygen_ref.uniform(rng, Q, N, 1)
    shares[1][:, :, N - 1] = np.array(Q, dtype=np.uint64)
    folded = c["ref"].aggregate([s[0] for s in shares], base[0])
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        col = ring.Collective(cQ, cP, 1, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        out = (qp(_pattern(1, nQ, N)), qp(_pattern(1, nQ, N)))
        col.CkksPcksShare(qp(c["sk_in"]), (qp(c["pk0"]), qp(c["pk1"])), qp(c["c1"]), (c["uc"], c["us"]), (c["e"][1], c["e"][2]), out, level)
        assert np.array_equal(out[0].get(), want[0]) and np.array_equal(out[1].get(), want[1]), no_epilogue
        got = col.Aggregate([qp(s) for s in shares], qp(_pattern(1, nQ, N)), level, base=qp(base))
        assert np.array_equal(_get(got)[0], folded), no_epilogue


@pytest.mark.parametrize("name,counts,batch", [("n16", [1, 2, 3, 33], 2), ("PN13QP218", [3], 1)])
def test_the_fold(gpu_pkg, oracle, name, counts, batch):
    """AggregateShares over n parties and KeySwitch's Add in one call: n - 1 Context.Add calls on the oracle, in the same order.  Two
    shares hold the residue q_j itself.  With and without a base, at the top level and at level 0, out fresh, out = shares[0], out = base"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", name)
    N, Q, nQ, r = c["N"], c["Q"], len(c["Q"]), c["ref"]
    rng = np.random.default_rng(77)
    most = max(counts)
    shares = [keygen_ref.uniform(rng, Q, N, batch) for _ in range(most)]
    shares[0][:, :, 0] = np.array(Q, dtype=np.uint64)
    shares[-1][:, :, 1] = np.array(Q, dtype=np.uint64)
    shares[min(1, most - 1)][:, :, 1] = np.array(Q, dtype=np.uint64)
    base = keygen_ref.uniform(rng, Q, N, batch)
    pat = _pattern(batch, nQ, N)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        col = ring.Collective(cQ, cP, batch, options=opt)
        qp = lambda x: ring.Poly(cQ, nQ, batch).set(x)
        for n in counts:
            for level in sorted({nQ - 1, 0}):
                for with_base in (False, True):
                    want = np.stack([r.aggregate([s[b, :level + 1] for s in shares[:n]], base[b] if with_base else None) for b in range(batch)])
                    for alias in ("fresh", "share0", "base"):
                        if alias == "base" and not with_base:
                            continue
                        where = (name, no_epilogue, n, level, with_base, alias)
                        dev = [qp(s) for s in shares[:n]]
                        dbase = qp(base) if with_base else None
                        out = {"fresh": qp(pat), "share0": dev[0], "base": dbase}[alias]
                        before = _get(out)
                        col.Aggregate(dev, out, level, base=dbase)
                        got = _get(out)
                        assert np.array_equal(got[:, :level + 1], want), where
                        assert np.array_equal(got[:, level + 1:], before[:, level + 1:]), where + ("limbs above the level were written",)
                        for k in range(1 if alias == "share0" else 0, n):
                            assert np.array_equal(_get(dev[k]), shares[k]), where + ("a share changed", k)
                        if with_base and alias != "base":
                            assert np.array_equal(_get(dbase), base), where + ("the base changed",)


def _add_qp(ring, cQ, cP, a, b, out):
    """out = a + b over all rows of Q||P: the rows of Q under contextQ, the rows of P under contextP"""
    nQ, nP, N = len(cQ.Modulus), len(cP.Modulus), cQ.N
    cQ.AddLvl(nQ - 1, a, b, out)
    wp = lambda p: ring.Poly.wrap(cP, p.device_ptr + 8 * nQ * N, nP, 1)
    cP.Add(wp(a), wp(b), wp(out))
    return out


@pytest.mark.parametrize("protocol", ["cks", "pcks"])
@pytest.mark.parametrize("scheme,level", [("ckks", None), ("ckks", 0), ("bfv", None)])
def test_chain_on_the_device_only(gpu_pkg, oracle, scheme, level, protocol):
    """three parties: secrets from lr_keygen summed on the device, the collective public key, a ciphertext from the device encryptor,
    three shares, the fold, KeySwitch, Decrypt, Decode -- the bytes of collective_ref.switch_inputs.  The switched ciphertext equals the
    oracle's bit for bit; BFV decodes to the plaintext exactly, CKKS within collective_ref.SWITCH_TOLERANCE"""
    import ckks_encoder_ref
    ring = gpu_pkg.ring
    if scheme == "ckks":
        N, Q, P = gpu_pkg.params.ckks_moduli(ref.SWITCH_PARAMS)
    else:
        N, Q, P, _ = gpu_pkg.params.bfv_moduli(ref.SWITCH_PARAMS)
    Q, P = list(Q), list(P)
    top, rows, roots = len(Q) - 1, len(Q) + len(P), ckks_encoder_ref.roots_table(N) if scheme == "ckks" else None
    w = ref.oracle_switch(oracle, scheme, protocol, N, Q, P, 0, level, roots)
    level = w["level"]
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    kg, col = ring.KeyGenerator(cQ, cP, 1), ring.Collective(cQ, cP, 1)
    one = lambda x: np.asarray(x)[None]
    secret = lambda b: kg.GenSecretKey((one(b[0]), one(b[1])), kg.NewKey())

    def total(keys):
        acc = keys[0]
        for k in keys[1:]:
            acc = _add_qp(ring, cQ, cP, acc, k, kg.NewKey())
        return acc
    sks = [secret(b) for b in w["sk_bits"]]
    sk = total(sks)
    pk = kg.GenPublicKey(sk, one(w["pk_e"]), (kg.NewKey(), kg.NewKey().set(w["pk1"])))
    assert np.array_equal(sk.get(), w["sk"]) and np.array_equal(pk[0].get(), w["pk0"])
    ct = (cQ.NewPoly(), cQ.NewPoly())
    u, e = (one(w["enc_u"][0]), one(w["enc_u"][1])), (one(w["enc_e"][0]), one(w["enc_e"][1]))
    if scheme == "ckks":
        coder = ring.CkksEncoder(cQ, 1, roots)
        ring.CkksEncryptor(cQ, cP, 1).EncryptPk(pk, u, e, coder.Encode(cQ.NewPoly(), one(w["values"]), top, ref.SWITCH_SCALE), ct, top, fast=False)
    else:
        coder = ring.BfvEncoder(cQ, ref.BFV_T, 1)
        ring.BfvEncryptor(cQ, cP, 1).EncryptPk(pk, u, e, coder.EncodeUint(one(w["ints"]), cQ.NewPoly()), ct, fast=False)
    assert np.array_equal(ct[1].get()[:level + 1], w["ct"][1])
    out = (cQ.NewPoly(), cQ.NewPoly())
    if protocol == "cks":
        sk_outs = [secret(b) for b in w["sk_out_bits"]]
        key = total(sk_outs)
        shares = []
        for i in range(len(sks)):
            if scheme == "ckks":
                shares.append(col.CkksCksShare(sks[i], sk_outs[i], ct[1], one(w["cks_e"][i]), cQ.NewPoly(), level))
            else:
                shares.append(col.BfvCksShare(sks[i], sk_outs[i], ct[1], one(w["cks_e"][i]), cQ.NewPoly()))
            assert np.array_equal(shares[i].get()[:level + 1], w["shares"][i]), i
        col.Aggregate(shares, out[0], level, base=ct[0])                 # AggregateShares twice and KeySwitch's Add in one call
        col.Aggregate([ct[1]], out[1], level)                            # KeySwitch's Copy
    else:
        key = secret(w["tgt_bits"])
        tgt = kg.GenPublicKey(key, one(w["tgt_e"]), (kg.NewKey(), kg.NewKey().set(w["tgt_pk1"])))
        shares = []
        for i in range(len(sks)):
            rand = ((one(w["pcks_u"][i][0]), one(w["pcks_u"][i][1])), (one(w["pcks_e"][i][0]), one(w["pcks_e"][i][1])))
            if scheme == "ckks":
                shares.append(col.CkksPcksShare(sks[i], tgt, ct[1], rand[0], rand[1], (cQ.NewPoly(), cQ.NewPoly()), level))
            else:
                shares.append(col.BfvPcksShare(sks[i], tgt, ct[1], rand[0], rand[1], (cQ.NewPoly(), cQ.NewPoly())))
            for k in range(2):
                assert np.array_equal(shares[i][k].get()[:level + 1], w["shares"][i][k]), (i, k)
        col.Aggregate([s[0] for s in shares], out[0], level, base=ct[0])
        col.Aggregate([s[1] for s in shares], out[1], level)
    assert np.array_equal(out[0].get()[:level + 1], w["out"][0]) and np.array_equal(out[1].get()[:level + 1], w["out"][1])
    pt = cQ.NewPoly()
    if scheme == "ckks":
        ring.CkksPlan(cQ, cP, 1).Decrypt(level, out, key, pt)
        got = coder.Decode(pt, N >> 1, level, ref.SWITCH_SCALE).reshape(N >> 1)
        err = float(np.max(np.abs(got - w["values"])))
        print("device switch %s level %d: largest slot error %.6e (allowed %.6e)" % (protocol, level, err, ref.SWITCH_TOLERANCE))
        assert err <= ref.SWITCH_TOLERANCE
    else:
        ring.BfvDecryptor(cQ, 1).Decrypt(out, key, pt)
        assert np.array_equal(coder.DecodeUint(pt).reshape(N), w["ints"])


def test_refusals(gpu_pkg, oracle):
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "ckks", "n16")
    N, Q, P = c["N"], c["Q"], c["P"]
    nQ, rows = len(Q), len(Q) + len(P)
    cQ, cP, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, Q)

    def code(f, *args, **kw):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args, **kw)
        return e.value.code
    ARG, SHAPE = 4, 3
    # creation: as lr_keygen_create, and ctxP is required
    assert code(ring.Collective, cQ, None, 1) == ARG
    assert code(ring.Collective, cQ, cP, 0) == ARG and code(ring.Collective, cQ, cP, 65536) == ARG                      # max_batch outside 1 .. 65535
    assert code(ring.Collective, ring.NewContextWithParams(4, Q), ring.NewContextWithParams(4, P), 1) == ARG           # N < 8
    assert code(ring.Collective, cQ, ring.NewContextWithParams(2 * N, P), 1) == ARG                                     # ctxP with another N
    if nat.device_count() > 1:
        assert code(ring.Collective, cQ, ring.NewContextWithParams(N, P, device=1), 1) == ARG                           # ctxP on another device
    L = nat.lib()
    assert L.lr_collective_create(None, cP.h, 1, C.byref(C.c_void_p())) == ARG and L.lr_collective_create(cQ.h, cP.h, 1, None) == ARG
    assert L.lr_collective_destroy(None) == 0
    col = ring.Collective(cQ, cP, 2)
    key = lambda ctx, batch: ring.Poly(ctx, rows, batch)
    q = lambda ctx, batch: ring.Poly(ctx, nQ, batch)
    sk, pk, c1, share, o1 = key(cQ, 1), (key(cQ, 1), key(cQ, 1)), q(cQ, 2), q(cQ, 2), q(cQ, 2)
    e, e3 = c["e"][0, :2], c["e"][0]
    u, ee = (c["uc"][:2], c["us"][:2]), (c["e"][1, :2], c["e"][2, :2])
    # CKS
    for f, lv in ((col.CkksCksShare, (1,)), (col.BfvCksShare, ())):
        assert code(f, key(other, 1), sk, c1, e, share, *lv) == ARG and code(f, sk, key(other, 1), c1, e, share, *lv) == ARG    # another context
        assert code(f, sk, sk, q(other, 2), e, share, *lv) == ARG and code(f, sk, sk, c1, e, q(other, 2), *lv) == ARG
        assert code(f, sk, sk, c1, e, c1, *lv) == ARG                                                                         # the output is an input
        assert code(f, share, sk, c1, e, share, *lv) == ARG
        assert code(f, ring.Poly(cQ, nQ - 1, 1), sk, c1, e, share, *lv) == SHAPE                                              # too few limbs
        assert code(f, sk, sk, c1, e, ring.Poly(cQ, nQ - 1, 2), *lv) == SHAPE
        assert code(f, sk, sk, q(cQ, 1), e, share, *lv) == SHAPE                                                              # c1 must have the batch
        assert code(f, key(cQ, 3), sk, q(cQ, 3), e3, q(cQ, 3), *lv) == SHAPE                                                  # batch > max_batch
    assert code(col.CkksCksShare, sk, sk, c1, e, share, 2) == SHAPE and code(col.CkksCksShare, sk, sk, c1, e, share, -1) == SHAPE   # level
    # PCKS
    for f, lv in ((col.CkksPcksShare, (1,)), (col.BfvPcksShare, ())):
        assert code(f, key(other, 1), pk, c1, u, ee, (share, o1), *lv) == ARG and code(f, sk, (key(other, 1), pk[1]), c1, u, ee, (share, o1), *lv) == ARG
        assert code(f, sk, pk, c1, u, ee, (share, q(other, 2)), *lv) == ARG
        assert code(f, sk, pk, c1, u, ee, (share, share), *lv) == ARG                                                         # the two outputs share memory
        assert code(f, sk, pk, c1, u, ee, (c1, o1), *lv) == ARG and code(f, sk, pk, c1, u, ee, (share, c1), *lv) == ARG         # an output is an input
        assert code(f, sk, (q(cQ, 1), pk[1]), c1, u, ee, (share, o1), *lv) == SHAPE                                           # the public key over Q only
        assert code(f, sk, pk, c1, u, ee, (share, ring.Poly(cQ, nQ - 1, 2)), *lv) == SHAPE
        assert code(f, sk, pk, q(cQ, 1), u, ee, (share, o1), *lv) == SHAPE
    assert code(col.CkksPcksShare, sk, pk, c1, u, ee, (share, o1), 2) == SHAPE
    # the fold
    s2 = [q(cQ, 2), q(cQ, 2)]
    assert code(col.Aggregate, s2, q(other, 2), 1) == ARG and code(col.Aggregate, [s2[0], q(other, 2)], share, 1) == ARG
    assert code(col.Aggregate, s2, share, 1, base=q(other, 2)) == ARG
    inside = ring.Poly.wrap(cQ, share.device_ptr + 8 * N, nQ, 1)                                                              # limb 1 of share on
    assert code(col.Aggregate, [inside], ring.Poly.wrap(cQ, share.device_ptr, nQ, 1), 1) == ARG                               # a partial overlap
    assert code(col.Aggregate, [q(cQ, 1)], ring.Poly.wrap(cQ, share.device_ptr, nQ, 1), 1, base=inside) == ARG
    assert code(col.Aggregate, s2, share, 2) == SHAPE and code(col.Aggregate, [s2[0], q(cQ, 1)], share, 1) == SHAPE
    assert code(col.Aggregate, s2, ring.Poly(cQ, nQ - 1, 2), 1) == SHAPE and code(col.Aggregate, [q(cQ, 3)], q(cQ, 3), 1) == SHAPE
    arr = (C.c_void_p * 2)(s2[0].h.value, s2[1].h.value)
    assert L.lr_collective_aggregate(col.h, 1, None, arr, 0, share.h) == SHAPE and L.lr_collective_aggregate(col.h, 1, None, None, 2, share.h) == ARG
    assert L.lr_collective_aggregate(col.h, 1, None, (C.c_void_p * 2)(s2[0].h.value, None), 2, share.h) == ARG
    assert L.lr_collective_aggregate(None, 1, None, arr, 2, share.h) == ARG and L.lr_collective_aggregate(col.h, 1, None, arr, 2, None) == ARG
    # ctxQ and ctxP on different streams: every entry point refuses
    hip = C.CDLL("libamdhip64.so")
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0                                                                  # hipStreamNonBlocking
    cQ.SetStream(st.value)
    try:
        with pytest.raises(nat.LatticeRingError, match="different streams"):
            col.CkksCksShare(sk, sk, c1, e, share, 1)
        assert code(col.BfvCksShare, sk, sk, c1, e, share) == ARG and code(col.CkksPcksShare, sk, pk, c1, u, ee, (share, o1), 1) == ARG
        assert code(col.BfvPcksShare, sk, pk, c1, u, ee, (share, o1)) == ARG and code(col.Aggregate, s2, share, 1) == ARG
        assert code(ring.Collective, cQ, cP, 1) == ARG
    finally:
        cQ.Sync()
        cQ.SetStream(None)
        assert hip.hipStreamDestroy(st) == 0
    # raw calls: NULL arguments and batches < 1
    b = np.zeros(256, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    h = lambda p: p.h
    calls = [("ckks_cks_share", [col.h, 1, h(sk), h(sk), h(c1), b, 2, h(share)], 6, 1),
             ("bfv_cks_share", [col.h, h(sk), h(sk), h(c1), b, 2, h(share)], 5, None),
             ("ckks_pcks_share", [col.h, 1, h(sk), h(pk[0]), h(pk[1]), h(c1), b, b, b, b, 2, h(share), h(o1)], 10, 1),
             ("bfv_pcks_share", [col.h, h(sk), h(pk[0]), h(pk[1]), h(c1), b, b, b, b, 2, h(share), h(o1)], 9, None)]
    for name, args, count, lv in calls:
        for fn in (getattr(L, "lr_collective_" + name), getattr(L, "lr_collective_" + name + "_device")):
            for i in range(len(args)):
                if i not in (count, lv):
                    assert fn(*[None if j == i else x for j, x in enumerate(args)]) == ARG, (fn.__name__, i)
            for bad in (0, -1):
                assert fn(*[bad if j == count else x for j, x in enumerate(args)]) == SHAPE, (fn.__name__, bad)
    # the handle stays usable after its refusals
    sk_in, sk_out = key(cQ, 1).set(c["sk_in"][:1]), key(cQ, 1).set(c["sk_out"][:1])
    c1.set(c["c1"][:2])
    col.CkksCksShare(sk_in, sk_out, c1, e, share, 1)
    for i in range(2):
        assert np.array_equal(share.get()[i], c["want"]("cks", 1, i, 0)), i


def test_staging_is_reused_across_consecutive_host_calls(gpu_pkg, oracle):
    """two host-form calls one behind the other with different bytes, no synchronisation between them: the second waits for the first
    one's copy out of the pinned buffer before it refills it"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "ckks", "PN12QP109")
    nQ, level = len(c["Q"]), len(c["Q"]) - 1
    _, cQ, cP = _rings(ring, c, False)
    col = ring.Collective(cQ, cP, 1)
    qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
    sk_in, sk_out = qp(c["sk_in"][:1]), qp(c["sk_out"][:1])
    c1 = [qp(c["c1"][b:b + 1]) for b in range(2)]
    shares = [cQ.NewPoly(), cQ.NewPoly()]
    for b in range(2):
        col.CkksCksShare(sk_in, sk_out, c1[b], c["e"][0, b:b + 1], shares[b], level)
    for b in range(2):
        assert np.array_equal(shares[b].get(), c["want"]("cks", level, b, 0)), b


def test_device_form_replays_from_a_hip_graph(gpu_pkg):
    """tests/_collective_graph_worker.py, in its own process because torch's HIP runtime has to come up before the library's"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_collective_graph_worker.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "graph replay ok" in res.stdout

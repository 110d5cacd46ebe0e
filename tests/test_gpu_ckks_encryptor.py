"""lr_ckks_encryptor on the device against the restatement over the CPU oracle (tests/ckks_encryptor_ref.py), bit for bit: pk and sk, fast
and through P, host and device-pointer randomness, the default shape and lr_options::no_epilogue (the reference's call-by-call shape),
batches 1 and 3, keys and plaintext shared by the batch or one per ciphertext, the fast forms with keys over Q alone, on
  n16        N = 2^4, 2 + 1 limbs of Qi60 / Pi60: less than one workgroup, two bytes per bit plane, the 60-bit transform route
  PN12QP109  N = 2^12, 2 + 1 limbs: CKKS moduli, the FP64-butterfly route
  PN13QP218  N = 2^13, 6 + 1 limbs: levels top, 0 and 3
  PN14QP438  its moduli at N = 2^11, 10 + 2 limbs: the one shape with |P| = 2; levels top, 0 and 5
  n65536     N = 2^16, 2 + 1 limbs of PN16QP1761, batch 2 with shared keys: pk and sk, fast and through P, in both shapes -- the one degree
             at which a lane of the streaming kernels makes a second trip of its loop
The randomness carries every edge decision at fixed positions: the four ternary (coeff, sign) pairs, a bit plane of all ones, the noise
bytes (0, sign 0) -- the residue q -- (0, sign 1), (19, +-), (127, +-); the uniform poly of the sk forms has zero coefficients, so that Neg
yields q.  The outputs are pre-filled with a pattern: limbs above the level keep it.  pk through P equals lr_ckks_encrypt_pk fed the
expanded polys at every tested level.  One chain Encode -> Encrypt -> Decrypt -> Decode stays on the device; every refusal of the header is
exercised; one _device call replays from a HIP graph."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ckks_encoder_ref as encoder_ref
import ckks_encryptor_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH = 3
SHAPES = ["n16", "PN12QP109", "PN13QP218", "PN14QP438"]
FORMS = [("pk", True), ("pk", False), ("sk", True), ("sk", False)]
_CACHE = {}


def _moduli(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    N, Q, P = pkg.params.ckks_moduli(name)
    return (1 << 11 if name == "PN14QP438" else N), list(Q), list(P)


def _levels(name, nQ):
    return [nQ - 1, 0, nQ // 2] if name in ("PN13QP218", "PN14QP438") else [nQ - 1]


def _case(oracle, pkg, name):
    """operands and the restatement's ciphertexts of one shape, computed once: want[(form, fast, level, shared)][b]"""
    if name in _CACHE:
        return _CACHE[name]
    N, Q, P = _moduli(pkg, name)
    QP = Q + P
    rng = np.random.default_rng(len(name) * 1000 + N + 1)
    c = {"N": N, "Q": Q, "P": P, "levels": _levels(name, len(Q))}
    keys = [ref.keygen(oracle, N, QP, rng)[:3] for _ in range(BATCH)]
    c["sk"], c["pk0"], c["pk1"] = (np.stack([k[i] for k in keys]) for i in range(3))
    uni = lambda moduli: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(BATCH)])
    c["crp"], c["pt"] = uni(QP), uni(Q)
    c["crp"][0, :, 3] = 0                                  # zero products: Neg yields q
    c["crp"][2, :, N - 1] = 0
    bits = lambda: rng.integers(0, 256, (BATCH, N >> 3)).astype(np.uint8)
    noise = lambda: (rng.integers(0, 20, (BATCH, N)) | (rng.integers(0, 2, (BATCH, N)) << 7)).astype(np.uint8)
    uc, us, e0, e1, e = bits(), bits(), noise(), noise(), noise()
    uc[0, 0], us[0, 0] = 0b10101010, 0b11001100          # coefficient i of byte 0: (coeff, sign) = (i & 1, (i >> 1) & 1)
    us[0, 1:] = 0xFF
    uc[1, :] = 0xFF                                        # a plane of all ones
    us[2, :] = 0xFF
    for a in (e0, e1, e):
        a[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
        a[1, N - 1] = 0                                    # (0, sign 0) on the last coefficient of another batch element
    c.update(uc=uc, us=us, e0=e0, e1=e1, e=e)
    enc = c["ref"] = ref.Encryptor(oracle, N, Q, P)
    want = {}
    for form, fast in FORMS:
        for level in c["levels"]:
            for shared in (True, False):
                rows = []
                for b in range(BATCH):
                    k = 0 if shared else b
                    if b == 0 and not shared:
                        rows.append(want[(form, fast, level, True)][0])
                    elif form == "pk":
                        rows.append(enc.encrypt_pk(fast, level, c["pk0"][k], c["pk1"][k], uc[b], us[b], e0[b], e1[b], c["pt"][k]))
                    else:
                        rows.append(enc.encrypt_sk(fast, level, c["sk"][k], c["crp"][b], e[b], c["pt"][k]))
                want[(form, fast, level, shared)] = rows
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
    cQ = ring.NewContextWithParams(c["N"], c["Q"], options=opt)
    cP = ring.NewContextWithParams(c["N"], c["P"], options=opt)
    return opt, cQ, cP


def _pattern(batch, limbs, N):
    return (np.arange(batch * limbs * N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).reshape(batch, limbs, N)


def test_pk_and_sk_encryption_at_n65536(gpu_pkg, oracle):
    """two trips of the streaming loops: the expansion and the two fast passes, and through P the products with the keys and the noise of
    the BFV encryptor's kernels; the keys and the plaintext shared by a batch of 2"""
    ring = gpu_pkg.ring
    N, Q, P = gpu_pkg.params.ckks_moduli("PN16QP1761")
    Q, P, batch = list(Q[:2]), list(P[:1]), 2
    nQ, level, rng = len(Q), len(Q) - 1, np.random.default_rng(65536)
    sk, pk0, pk1 = (k[None] for k in ref.keygen(oracle, N, Q + P, rng)[:3])
    uni = lambda moduli, n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(n)])
    crp, pt = uni(Q + P, batch), uni(Q, 1)
    crp[1, :, N - 1] = 0                                   # a zero product on the last coefficient, in the second trip: Neg yields q
    bits = lambda: rng.integers(0, 256, (batch, N >> 3)).astype(np.uint8)
    noise = lambda: (rng.integers(0, 20, (batch, N)) | (rng.integers(0, 2, (batch, N)) << 7)).astype(np.uint8)
    uc, us, e0, e1, e = bits(), bits(), noise(), noise(), noise()
    for a in (e0, e1, e):
        a[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
        a[1, N - 1] = 0                                    # (0, sign 0) on the last coefficient
    r = ref.Encryptor(oracle, N, Q, P)
    want = {}
    for fast in (True, False):
        want[("pk", fast)] = [r.encrypt_pk(fast, level, pk0[0], pk1[0], uc[b], us[b], e0[b], e1[b], pt[0]) for b in range(batch)]
        want[("sk", fast)] = [r.encrypt_sk(fast, level, sk[0], crp[b], e[b], pt[0]) for b in range(batch)]
    for no_epilogue in (False, True):
        opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
        cQ, cP = ring.NewContextWithParams(N, Q, options=opt), ring.NewContextWithParams(N, P, options=opt)
        enc = ring.CkksEncryptor(cQ, cP, batch, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        dpt = cQ.NewPoly(1).set(pt)
        for form, fast in FORMS:
            ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
            if form == "pk":
                enc.EncryptPk((qp(pk0), qp(pk1)), (uc, us), (e0, e1), dpt, ct, level, fast=fast)
            else:
                enc.EncryptSk(qp(sk), qp(crp), e, dpt, ct, level, fast=fast)
            got = [p.get().reshape(batch, nQ, N) for p in ct]
            for b in range(batch):
                w = want[(form, fast)][b]
                assert np.array_equal(got[0][b], w[0]) and np.array_equal(got[1][b], w[1]), (form, fast, no_epilogue, b)


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("batch", [1, BATCH])
@pytest.mark.parametrize("name", SHAPES)
def test_encrypt_against_the_restatement(gpu_pkg, oracle, name, batch, shared):
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, name)
    N, nQ, nP = c["N"], len(c["Q"]), len(c["P"])
    kb = 1 if shared else batch
    mark = _pattern(batch, nQ, N)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        enc = ring.CkksEncryptor(cQ, cP, batch, options=opt)
        plan = ring.CkksPlan(cQ, cP, batch)
        qp = lambda x: ring.Poly(cQ, nQ + nP, x.shape[0]).set(x)
        over_q = lambda x: ring.Poly(cQ, nQ, x.shape[0]).set(np.ascontiguousarray(x[:, :nQ]))
        sk, pk = qp(c["sk"][:kb]), (qp(c["pk0"][:kb]), qp(c["pk1"][:kb]))
        sk_q, pk_q = over_q(c["sk"][:kb]), (over_q(c["pk0"][:kb]), over_q(c["pk1"][:kb]))
        crp, crp_q = qp(c["crp"][:batch]), over_q(c["crp"][:batch])
        pt = cQ.NewPoly(kb).set(c["pt"][:kb])
        rand = [c[k][:batch] for k in ("uc", "us", "e0", "e1", "e")]
        keep, ptrs = _bytes_on_device(ring, cQ, rand)
        for level in c["levels"]:
            # what lr_ckks_encrypt_pk takes for the same decisions (its plaintext and keys may be shared, u and e not)
            ops = [ref.expand_pk_operands(oracle, c["ref"], rand[0][b], rand[1][b], rand[2][b], rand[3][b]) for b in range(batch)]
            old = (cQ.NewPoly(batch).set(mark), cQ.NewPoly(batch).set(mark))
            plan.EncryptPk(level, qp(np.stack([o[0] for o in ops])), pk, (qp(np.stack([o[1] for o in ops])), qp(np.stack([o[2] for o in ops]))),
                           pt, old)
            old = [p.get().reshape(batch, nQ, N) for p in old]
            for form, fast in FORMS:
                for on_device in (False, True):
                    ct = (cQ.NewPoly(batch).set(mark), cQ.NewPoly(batch).set(mark))
                    if form == "pk":
                        keys = pk_q if fast and on_device else pk               # the fast form reads |Q| limbs: a key over Q alone serves too
                        if on_device:
                            enc.EncryptPkDevice(keys, ptrs[0:2], ptrs[2:4], pt, ct, level, fast=fast)
                        else:
                            enc.EncryptPk(keys, rand[0:2], rand[2:4], pt, ct, level, fast=fast)
                    else:
                        key, a = (sk_q, crp_q) if fast and on_device else (sk, crp)
                        if on_device:
                            enc.EncryptSkDevice(key, a, ptrs[4], pt, ct, level, fast=fast)
                        else:
                            enc.EncryptSk(key, a, rand[4], pt, ct, level, fast=fast)
                    got = [p.get().reshape(batch, nQ, N) for p in ct]
                    where = (name, form, fast, level, on_device, no_epilogue)
                    for b in range(batch):
                        want = c["want"][(form, fast, level, shared)][b]
                        assert np.array_equal(got[0][b, :level + 1], want[0]), where + (b, 0)
                        assert np.array_equal(got[1][b, :level + 1], want[1]), where + (b, 1)
                    for k in range(2):
                        assert np.array_equal(got[k][:, level + 1:], mark[:, level + 1:]), where + ("limbs above the level", k)
                        if form == "pk" and not fast:
                            assert np.array_equal(got[k][:, :level + 1], old[k][:, :level + 1]), where + ("lr_ckks_encrypt_pk", k)
                    # the uniform poly is never modified
                    assert np.array_equal(crp.get().reshape(batch, nQ + nP, N), c["crp"][:batch]), where
                    assert np.array_equal(crp_q.get().reshape(batch, nQ, N), c["crp"][:batch, :nQ]), where
        del keep


def test_staging_is_reused_across_consecutive_host_calls(gpu_pkg, oracle):
    """two host-form calls one behind the other with different bytes, no synchronisation between them: the second waits for the first
    one's copy out of the pinned buffer before it refills it"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "PN12QP109")
    N, nQ, nP, level = c["N"], len(c["Q"]), len(c["P"]), len(c["Q"]) - 1
    _, cQ, cP = _rings(ring, c, False)
    enc = ring.CkksEncryptor(cQ, cP, 1)
    pk = (ring.Poly(cQ, nQ + nP, 1).set(c["pk0"][:1]), ring.Poly(cQ, nQ + nP, 1).set(c["pk1"][:1]))
    pt = cQ.NewPoly(1).set(c["pt"][:1])
    cts = [(cQ.NewPoly(1), cQ.NewPoly(1)) for _ in range(2)]
    for b in range(2):
        enc.EncryptPk(pk, (c["uc"][b:b + 1], c["us"][b:b + 1]), (c["e0"][b:b + 1], c["e1"][b:b + 1]), pt, cts[b], level, fast=True)
    for b in range(2):
        want = c["want"][("pk", True, level, True)][b]
        assert np.array_equal(cts[b][0].get(), want[0]) and np.array_equal(cts[b][1].get(), want[1]), b


def test_fast_forms_without_p(gpu_pkg, oracle):
    """ctxP == NULL is the reference's "modulus P is empty": the fast forms give the same bits, fast = 0 is refused"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n16")
    N, nQ, level = c["N"], len(c["Q"]), len(c["Q"]) - 1
    cQ = ring.NewContextWithParams(N, c["Q"])
    enc = ring.CkksEncryptor(cQ, None, 1)
    pk = (ring.Poly(cQ, nQ, 1).set(c["pk0"][:1, :nQ]), ring.Poly(cQ, nQ, 1).set(c["pk1"][:1, :nQ]))
    sk, crp = ring.Poly(cQ, nQ, 1).set(c["sk"][:1, :nQ]), ring.Poly(cQ, nQ, 1).set(c["crp"][:1, :nQ])
    pt, ct = cQ.NewPoly().set(c["pt"][:1]), (cQ.NewPoly(), cQ.NewPoly())
    enc.EncryptPk(pk, (c["uc"][:1], c["us"][:1]), (c["e0"][:1], c["e1"][:1]), pt, ct, level, fast=True)
    want = c["want"][("pk", True, level, True)][0]
    assert np.array_equal(ct[0].get(), want[0]) and np.array_equal(ct[1].get(), want[1])
    enc.EncryptSk(sk, crp, c["e"][:1], pt, ct, level, fast=True)
    want = c["want"][("sk", True, level, True)][0]
    assert np.array_equal(ct[0].get(), want[0]) and np.array_equal(ct[1].get(), want[1])
    for call in (lambda: enc.EncryptPk(pk, (c["uc"][:1], c["us"][:1]), (c["e0"][:1], c["e1"][:1]), pt, ct, level, fast=False),
                 lambda: enc.EncryptSk(sk, crp, c["e"][:1], pt, ct, level, fast=False)):
        with pytest.raises(gpu_pkg._native.LatticeRingError, match="fast form") as e:
            call()
        assert e.value.code == 4


def test_encode_encrypt_decrypt_decode_on_the_device(gpu_pkg, oracle):
    """PN12QP109, all slots, scale 2^32: CkksEncoder.Encode -> Encrypt (pk through P, then pk fast) -> CkksPlan.Decrypt ->
    CkksEncoder.Decode.  The decrypted plaintext poly is the restatement's bit for bit; the decoded slots are within the tolerance that
    tests/test_oracle_ckks_encryptor.py measured for the restatement's round trip (ckks_encryptor_ref.ROUND_TRIP_TOLERANCE)."""
    ring = gpu_pkg.ring
    N, Q, P = gpu_pkg.params.ckks_moduli("PN12QP109")
    Q, P = list(Q), list(P)
    nQ, nP, level, scale, slots, batch = len(Q), len(P), len(Q) - 1, 2.0 ** 32, N >> 1, 2
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    roots = encoder_ref.roots_table(N)
    coder, plan, enc = ring.CkksEncoder(cQ, batch, roots), ring.CkksPlan(cQ, cP, batch), ring.CkksEncryptor(cQ, cP, batch)
    r_enc, r_coder = ref.Encryptor(oracle, N, Q, P), encoder_ref.Encoder(oracle, N, Q, roots)
    rng = np.random.default_rng(77)
    sk_h, pk0_h, pk1_h, _ = ref.keygen(oracle, N, Q + P, rng)
    qp = lambda x: ring.Poly(cQ, nQ + nP, 1).set(x[None])
    sk, pk = qp(sk_h), (qp(pk0_h), qp(pk1_h))
    vals = rng.uniform(0, 1, (batch, slots)) * np.exp(2j * np.pi * rng.uniform(0, 1, (batch, slots)))
    bits = lambda: rng.integers(0, 256, (batch, N >> 3)).astype(np.uint8)
    noise = lambda: (rng.integers(0, 20, (batch, N)) | (rng.integers(0, 2, (batch, N)) << 7)).astype(np.uint8)
    pt = coder.Encode(cQ.NewPoly(batch), vals, level, scale)
    for fast in (False, True):
        uc, us, e0, e1 = bits(), bits(), noise(), noise()
        ct = enc.EncryptPk(pk, (uc, us), (e0, e1), pt, (cQ.NewPoly(batch), cQ.NewPoly(batch)), level, fast=fast)
        out = cQ.NewPoly(batch)
        plan.Decrypt(level, ct, sk, out)
        got_pt, got = out.get().reshape(batch, nQ, N), coder.Decode(out, slots, level, scale)
        for b in range(batch):
            want_ct = r_enc.encrypt_pk(fast, level, pk0_h, pk1_h, uc[b], us[b], e0[b], e1[b], r_coder.encode(vals[b], level, scale))
            assert np.array_equal(got_pt[b], ref.decrypt(oracle, r_enc, level, want_ct, sk_h)), (fast, b)
            assert np.max(np.abs(got[b] - vals[b])) <= ref.ROUND_TRIP_TOLERANCE, (fast, b)


def test_refusals(gpu_pkg, oracle):
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P = c["N"], c["Q"], c["P"]
    nQ, nP, top = len(Q), len(P), len(Q) - 1
    cQ, cP, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, Q)

    def code(f, *args, **kw):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args, **kw)
        return e.value.code
    ARG, SHAPE = 4, 3
    # creation
    assert code(ring.CkksEncryptor, cQ, cP, 0) == ARG and code(ring.CkksEncryptor, cQ, cP, 65536) == ARG                # max_batch outside 1 .. 65535
    assert code(ring.CkksEncryptor, ring.NewContextWithParams(4, Q), None, 1) == ARG                                    # N < 8
    assert code(ring.CkksEncryptor, cQ, ring.NewContextWithParams(2 * N, P), 1) == ARG                                  # ctxP with another N
    if nat.device_count() > 1:
        assert code(ring.CkksEncryptor, cQ, ring.NewContextWithParams(N, P, device=1), 1) == ARG                        # ctxP on another device
    L = nat.lib()
    assert L.lr_ckks_encryptor_create(None, cP.h, 1, C.byref(C.c_void_p())) == ARG and L.lr_ckks_encryptor_create(cQ.h, cP.h, 1, None) == ARG
    assert L.lr_ckks_encryptor_destroy(None) == 0
    enc = ring.CkksEncryptor(cQ, cP, 2)
    qp = lambda ctx, batch: ring.Poly(ctx, nQ + nP, batch)
    pk, sk, crp, pt = (qp(cQ, 1), qp(cQ, 1)), qp(cQ, 1), qp(cQ, 2), cQ.NewPoly(2)
    ct = (cQ.NewPoly(2), cQ.NewPoly(2))
    u, e = (c["uc"][:2], c["us"][:2]), (c["e0"][:2], c["e1"][:2])
    # pk
    assert code(enc.EncryptPk, pk, u, e, pt, (ct[0], ct[0]), top) == ARG                                                 # out_c0 == out_c1
    assert code(enc.EncryptPk, (qp(other, 1), pk[1]), u, e, pt, ct, top) == ARG                                          # a poly of another context
    assert code(enc.EncryptPk, pk, u, e, other.NewPoly(2), ct, top) == ARG
    assert code(enc.EncryptPk, pk, u, e, pt, (ct[0], other.NewPoly(2)), top) == ARG
    assert code(enc.EncryptPk, (ring.Poly(cQ, nQ, 1), pk[1]), u, e, pt, ct, top) == SHAPE                                # too few limbs for the form through P
    assert code(enc.EncryptPk, (ring.Poly(cQ, nQ - 1, 1), pk[1]), u, e, pt, ct, top, fast=True) == SHAPE                 # ... and for the fast form
    assert code(enc.EncryptPk, pk, u, e, pt, (ct[0], ring.Poly(cQ, nQ - 1, 2)), top) == SHAPE                            # fewer than level + 1 limbs
    assert code(enc.EncryptPk, pk, u, e, ring.Poly(cQ, nQ - 1, 2), ct, top) == SHAPE
    assert code(enc.EncryptPk, pk, u, e, pt, ct, -1) == SHAPE and code(enc.EncryptPk, pk, u, e, pt, ct, nQ) == SHAPE     # a level outside 0 .. |Q| - 1
    assert code(enc.EncryptPk, pk, u, e, cQ.NewPoly(3), ct, top) == SHAPE                                                # batch differs from a poly's
    assert code(enc.EncryptPk, (qp(cQ, 3), pk[1]), u, e, pt, ct, top) == SHAPE
    three = (cQ.NewPoly(3), cQ.NewPoly(3))
    assert code(enc.EncryptPk, pk, (c["uc"], c["us"]), (c["e0"], c["e1"]), cQ.NewPoly(3), three, top) == SHAPE           # batch > max_batch
    assert code(enc.EncryptSk, sk, qp(cQ, 3), c["e"], cQ.NewPoly(3), three, top) == SHAPE
    # sk
    assert code(enc.EncryptSk, sk, crp, c["e"][:2], pt, (ct[1], ct[1]), top) == ARG
    assert code(enc.EncryptSk, qp(other, 1), crp, c["e"][:2], pt, ct, top) == ARG
    assert code(enc.EncryptSk, sk, qp(other, 2), c["e"][:2], pt, ct, top) == ARG
    assert code(enc.EncryptSk, sk, ring.Poly(cQ, nQ, 2), c["e"][:2], pt, ct, top) == SHAPE                               # crp over Q alone, form through P
    assert code(enc.EncryptSk, sk, qp(cQ, 1), c["e"][:2], pt, ct, top) == SHAPE                                          # crp must have the batch
    assert code(enc.EncryptSk, sk, crp, c["e"][:2], pt, ct, nQ) == SHAPE and code(enc.EncryptSk, sk, crp, c["e"][:2], pt, ct, -1) == SHAPE
    # raw calls: NULL arguments and batch < 1
    b = np.zeros(64, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    h = lambda p: p.h
    pk_args = [enc.h, 0, top, h(pk[0]), h(pk[1]), b, b, b, b, h(pt), 2, h(ct[0]), h(ct[1])]
    sk_args = [enc.h, 0, top, h(sk), h(crp), b, h(pt), 2, h(ct[0]), h(ct[1])]
    for fn, args, skip in ((L.lr_ckks_encryptor_encrypt_pk, pk_args, (1, 2, 10)), (L.lr_ckks_encryptor_encrypt_pk_device, pk_args, (1, 2, 10)),
                           (L.lr_ckks_encryptor_encrypt_sk, sk_args, (1, 2, 7)), (L.lr_ckks_encryptor_encrypt_sk_device, sk_args, (1, 2, 7))):
        for i in range(len(args)):
            if i not in skip:
                assert fn(*[None if j == i else a for j, a in enumerate(args)]) == ARG, (fn.__name__, i)
        for bad in (0, -1):
            assert fn(*[bad if j == skip[2] else a for j, a in enumerate(args)]) == SHAPE, (fn.__name__, bad)
    # the handle stays usable after its refusals
    pk[0].set(c["pk0"][:1])
    pk[1].set(c["pk1"][:1])
    pt1 = cQ.NewPoly(1).set(c["pt"][:1])
    enc.EncryptPk(pk, u, e, pt1, ct, top)
    want = c["want"][("pk", False, top, True)]
    got = [p.get() for p in ct]
    for bi in range(2):
        assert np.array_equal(got[0][bi], want[bi][0]) and np.array_equal(got[1][bi], want[bi][1])


def test_device_form_replays_from_a_hip_graph(gpu_pkg):
    """tests/_ckks_encryptor_graph_worker.py, in its own process because torch's HIP runtime has to come up before the library's"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ckks_encryptor_graph_worker.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "graph replay ok" in res.stdout

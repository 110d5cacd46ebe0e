"""lr_bfv_encryptor / lr_bfv_decryptor on the device against the restatement over the CPU oracle (tests/bfv_encryptor_ref.py), bit for bit:
pk and sk, fast and through P, host and device-pointer randomness, the default shape and lr_options::no_epilogue (the reference's
call-by-call shape), batches 1 and 3, keys and plaintext shared by the batch or one per ciphertext, on
  n16        N = 2^4, 2 + 1 limbs of Qi60 / Pi60: less than one workgroup, two bytes per bit plane
  PN12QP109  N = 2^12, 2 + 1 limbs
  PN13QP218  N = 2^13, 3 + 1 limbs
  PN14QP438  its moduli at N = 2^11, 6 + 2 limbs: the one shape with |P| = 2
  n65536     N = 2^16, 2 + 1 limbs of CKKS PN16QP1761, batch 2 with shared keys: one pk and one sk encryption, fast, in both shapes -- the
             one degree at which a lane of the streaming kernels makes a second trip of its loop
The randomness carries every edge decision at fixed positions: the four ternary (coeff, sign) pairs, a bit plane of all ones, the noise
bytes (0, sign 0) -- the residue q -- (0, sign 1), (19, +-), (127, +-).  Decrypt: degrees 0, 1, 2, 7, 8 (the reduction cadence) and 9
(above the one-pass kernel's limit), pt_out aliasing the top component, a key over Q||P, components back to back in memory.  One chain
Encode -> Encrypt -> Mul -> Decrypt -> Decode returns the slot-wise products.  Every refusal of the header is exercised."""
import ctypes as C

import numpy as np
import pytest

import bfv_encryptor_ref as ref

pytestmark = pytest.mark.gpu

BATCH = 3
SHAPES = ["n16", "PN12QP109", "PN13QP218", "PN14QP438"]
FORMS = [("pk", True), ("pk", False), ("sk", True), ("sk", False)]
_CACHE = {}


def _moduli(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    N, Q, P, _ = pkg.params.bfv_moduli(name)
    return (1 << 11 if name == "PN14QP438" else N), list(Q), list(P)


def _case(oracle, pkg, name):
    """operands and the restatement's ciphertexts of one shape, computed once: want[(form, fast, shared)][b]"""
    if name in _CACHE:
        return _CACHE[name]
    N, Q, P = _moduli(pkg, name)
    QP = Q + P
    rng = np.random.default_rng(len(name) * 1000 + N)
    c = {"N": N, "Q": Q, "P": P}
    keys = [ref.keygen(oracle, N, QP, rng)[:3] for _ in range(BATCH)]
    c["sk"], c["pk0"], c["pk1"] = (np.stack([k[i] for k in keys]) for i in range(3))
    uni = lambda moduli: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(BATCH)])
    c["crp"], c["pt"] = uni(QP), uni(Q)
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
    enc = ref.Encryptor(oracle, N, Q, P)
    c["ocQ"] = enc.cQ
    want = {}
    for form, fast in FORMS:
        for shared in (True, False):
            rows = []
            for b in range(BATCH):
                k = 0 if shared else b
                if b == 0 and not shared:
                    rows.append(want[(form, fast, True)][0])
                elif form == "pk":
                    rows.append(enc.encrypt_pk(fast, c["pk0"][k], c["pk1"][k], uc[b], us[b], e0[b], e1[b], c["pt"][k]))
                else:
                    rows.append(enc.encrypt_sk(fast, c["sk"][k], c["crp"][b], e[b], c["pt"][k]))
            want[(form, fast, shared)] = rows
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


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("batch", [1, BATCH])
@pytest.mark.parametrize("name", SHAPES)
def test_encrypt_against_the_restatement(gpu_pkg, oracle, name, batch, shared):
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, name)
    N, nQ, nP = c["N"], len(c["Q"]), len(c["P"])
    kb = 1 if shared else batch
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        enc = ring.BfvEncryptor(cQ, cP, batch, options=opt)
        qp = lambda x: ring.Poly(cQ, nQ + nP, x.shape[0]).set(x)
        sk, pk = qp(c["sk"][:kb]), (qp(c["pk0"][:kb]), qp(c["pk1"][:kb]))
        sk_q, pk_q = ring.Poly(cQ, nQ, kb).set(c["sk"][:kb, :nQ]), (ring.Poly(cQ, nQ, kb).set(c["pk0"][:kb, :nQ]), ring.Poly(cQ, nQ, kb).set(c["pk1"][:kb, :nQ]))
        crp, crp_q = qp(c["crp"][:batch]), ring.Poly(cQ, nQ, batch).set(c["crp"][:batch, :nQ])
        pt = cQ.NewPoly(kb).set(c["pt"][:kb])
        rand = [c[k][:batch] for k in ("uc", "us", "e0", "e1", "e")]
        keep, ptrs = _bytes_on_device(ring, cQ, rand)
        for form, fast in FORMS:
            for on_device in (False, True):
                ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
                if form == "pk":
                    keys = pk_q if fast and on_device else pk               # the fast form reads |Q| limbs: a key over Q alone serves too
                    if on_device:
                        enc.EncryptPkDevice(keys, ptrs[0:2], ptrs[2:4], pt, ct, fast=fast)
                    else:
                        enc.EncryptPk(keys, rand[0:2], rand[2:4], pt, ct, fast=fast)
                else:
                    key, a = (sk_q, crp_q) if fast and on_device else (sk, crp)
                    if on_device:
                        enc.EncryptSkDevice(key, a, ptrs[4], pt, ct, fast=fast)
                    else:
                        enc.EncryptSk(key, a, rand[4], pt, ct, fast=fast)
                got = [p.get().reshape(batch, nQ, N) for p in ct]
                for b in range(batch):
                    want = c["want"][(form, fast, shared)][b]
                    where = (name, form, fast, on_device, no_epilogue, b)
                    assert np.array_equal(got[0][b], want[0]), where
                    assert np.array_equal(got[1][b], want[1]), where
        assert np.array_equal(crp.get().reshape(batch, nQ + nP, N), c["crp"][:batch])      # the uniform poly is never modified
        del keep


def test_one_pk_and_one_sk_encryption_at_n65536(gpu_pkg, oracle):
    """two trips of the streaming loops: the ternary expansion, the two products with the public key, the noise added with the plaintext
    (one pass) and expanded alone (call by call), and the negated product with the secret key; the keys and the plaintext shared by a batch of 2"""
    ring = gpu_pkg.ring
    N, Q, P = gpu_pkg.params.ckks_moduli("PN16QP1761")
    Q, P, batch = list(Q[:2]), list(P[:1]), 2
    nQ, rng = len(Q), np.random.default_rng(65536)
    sk, pk0, pk1 = (k[None] for k in ref.keygen(oracle, N, Q + P, rng)[:3])
    uni = lambda moduli, n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(n)])
    crp, pt = uni(Q + P, batch), uni(Q, 1)
    bits = lambda: rng.integers(0, 256, (batch, N >> 3)).astype(np.uint8)
    noise = lambda: (rng.integers(0, 20, (batch, N)) | (rng.integers(0, 2, (batch, N)) << 7)).astype(np.uint8)
    uc, us, e0, e1, e = bits(), bits(), noise(), noise(), noise()
    for a in (e0, e1, e):
        a[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
        a[1, N - 1] = 0                                    # (0, sign 0) on the last coefficient, in the second trip
    r = ref.Encryptor(oracle, N, Q, P)
    want_pk = [r.encrypt_pk(True, pk0[0], pk1[0], uc[b], us[b], e0[b], e1[b], pt[0]) for b in range(batch)]
    want_sk = [r.encrypt_sk(True, sk[0], crp[b], e[b], pt[0]) for b in range(batch)]
    for no_epilogue in (False, True):
        opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
        cQ, cP = ring.NewContextWithParams(N, Q, options=opt), ring.NewContextWithParams(N, P, options=opt)
        enc = ring.BfvEncryptor(cQ, cP, batch, options=opt)
        qp = lambda x: ring.Poly(cQ, x.shape[1], x.shape[0]).set(x)
        dpt = cQ.NewPoly(1).set(pt)
        for form, want in (("pk", want_pk), ("sk", want_sk)):
            ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
            if form == "pk":
                enc.EncryptPk((qp(pk0), qp(pk1)), (uc, us), (e0, e1), dpt, ct, fast=True)
            else:
                enc.EncryptSk(qp(sk), qp(crp), e, dpt, ct, fast=True)
            got = [p.get().reshape(batch, nQ, N) for p in ct]
            for b in range(batch):
                assert np.array_equal(got[0][b], want[b][0]) and np.array_equal(got[1][b], want[b][1]), (form, no_epilogue, b)


def test_fast_forms_without_p(gpu_pkg, oracle):
    """ctxP == NULL is the reference's "modulus P is empty": the fast forms give the same bits, fast = 0 is refused"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n16")
    N, nQ = c["N"], len(c["Q"])
    cQ = ring.NewContextWithParams(N, c["Q"])
    enc = ring.BfvEncryptor(cQ, None, 1)
    pk = (ring.Poly(cQ, nQ, 1).set(c["pk0"][:1, :nQ]), ring.Poly(cQ, nQ, 1).set(c["pk1"][:1, :nQ]))
    pt, ct = cQ.NewPoly().set(c["pt"][:1]), (cQ.NewPoly(), cQ.NewPoly())
    enc.EncryptPk(pk, (c["uc"][:1], c["us"][:1]), (c["e0"][:1], c["e1"][:1]), pt, ct, fast=True)
    want = c["want"][("pk", True, True)][0]
    assert np.array_equal(ct[0].get(), want[0]) and np.array_equal(ct[1].get(), want[1])
    with pytest.raises(gpu_pkg._native.LatticeRingError, match="fast form") as e:
        enc.EncryptPk(pk, (c["uc"][:1], c["us"][:1]), (c["e0"][:1], c["e1"][:1]), pt, ct, fast=False)
    assert e.value.code == 4


@pytest.mark.parametrize("no_epilogue", [False, True], ids=["one_pass", "call_by_call"])
@pytest.mark.parametrize("name", ["n16", "PN12QP109"])
def test_decrypt_against_the_restatement(gpu_pkg, oracle, name, no_epilogue):
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, name)
    N, nQ, nP, batch = c["N"], len(c["Q"]), len(c["P"]), 2
    opt, cQ, _ = _rings(ring, c, no_epilogue)
    dec = ring.BfvDecryptor(cQ, batch)
    rng = np.random.default_rng(5)
    top = 9
    comps = np.stack([np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in c["Q"]], dtype=np.uint64) for _ in range(batch)])
                      for _ in range(top + 1)])                                        # [component][batch][|Q|][N]
    sk_shared = ring.Poly(cQ, nQ + nP, 1).set(c["sk"][:1])                             # a key over Q||P, one for the batch
    sk_own = ring.Poly(cQ, nQ, batch).set(c["sk"][:batch, :nQ])
    for degree in (0, 1, 2, 7, 8, top):
        for sk, own in ((sk_shared, False), (sk_own, True)):
            polys = [cQ.NewPoly(batch).set(comps[i]) for i in range(degree + 1)]
            out = dec.Decrypt(polys, sk, cQ.NewPoly(batch)).get().reshape(batch, nQ, N)
            want = [ref.decrypt(c["ocQ"], comps[:degree + 1, b], c["sk"][b if own else 0]) for b in range(batch)]
            for b in range(batch):
                assert np.array_equal(out[b], want[b]), (degree, own, b)
            for i in range(degree + 1):
                assert np.array_equal(polys[i].get().reshape(batch, nQ, N), comps[i]), (degree, i, "an input was modified")
            if own:
                dec.Decrypt(polys, sk, polys[degree])                                  # pt_out is the top component
                aliased = polys[degree].get().reshape(batch, nQ, N)
                assert all(np.array_equal(aliased[b], want[b]) for b in range(batch)), degree
    # components back to back in one allocation: their transforms share a launch
    degree = 2
    big = ring.Poly(cQ, nQ, (degree + 1) * batch).set(comps[:degree + 1].reshape((degree + 1) * batch, nQ, N))
    views = [ring.Poly.wrap(cQ, big.device_ptr + i * batch * nQ * N * 8, nQ, batch) for i in range(degree + 1)]
    out = dec.Decrypt(views, sk_shared, cQ.NewPoly(batch)).get().reshape(batch, nQ, N)
    for b in range(batch):
        assert np.array_equal(out[b], ref.decrypt(c["ocQ"], comps[:degree + 1, b], c["sk"][0])), b


@pytest.mark.parametrize("form", ["pk", "sk"])
def test_encode_encrypt_mul_decrypt_decode(gpu_pkg, oracle, form):
    """PN12QP109, t = 65537: two slot vectors, one operand encrypted fast and one through P, BfvPlan.Mul, Decrypt of the degree-2 result,
    DecodeUint: the slot-wise product modulo t.  Between encode and decode only the slot values cross the host boundary."""
    ring = gpu_pkg.ring
    t, batch = 65537, 2
    N, Q, P, QMul = gpu_pkg.params.bfv_moduli("PN12QP109")
    Q, P, QMul = list(Q), list(P), list(QMul)
    cQ, cP, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, QMul)
    encoder, plan = ring.BfvEncoder(cQ, t, batch), ring.BfvPlan(cQ, cM, t, batch)
    encryptor, decryptor = ring.BfvEncryptor(cQ, cP, batch), ring.BfvDecryptor(cQ, batch)
    rng = np.random.default_rng(17)
    sk_h, pk0_h, pk1_h, _ = ref.keygen(oracle, N, Q + P, rng)
    qp = lambda x: ring.Poly(cQ, len(Q) + len(P), 1).set(x[None])
    sk, pk = qp(sk_h), (qp(pk0_h), qp(pk1_h))
    slots = [rng.integers(0, t, size=(batch, N), dtype=np.uint64) for _ in range(2)]
    bits = lambda: rng.integers(0, 256, (batch, N >> 3)).astype(np.uint8)
    noise = lambda: (rng.integers(0, 20, (batch, N)) | (rng.integers(0, 2, (batch, N)) << 7)).astype(np.uint8)
    cts = []
    for k, fast in enumerate((True, False)):
        pt = encoder.EncodeUint(slots[k], cQ.NewPoly(batch))
        ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        if form == "pk":
            encryptor.EncryptPk(pk, (bits(), bits()), (noise(), noise()), pt, ct, fast=fast)
        else:
            crp = np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q + P], dtype=np.uint64) for _ in range(batch)])
            encryptor.EncryptSk(sk, ring.Poly(cQ, len(Q) + len(P), batch).set(crp), noise(), pt, ct, fast=fast)
        cts.append(ct)
    for k in range(2):                                   # each operand decrypts to its own slots
        assert np.array_equal(encoder.DecodeUint(decryptor.Decrypt(cts[k], sk, cQ.NewPoly(batch))), slots[k]), k
    prod = [cQ.NewPoly(batch) for _ in range(3)]
    plan.Mul(cts[0], cts[1], prod)
    got = encoder.DecodeUint(decryptor.Decrypt(prod, sk, cQ.NewPoly(batch)))
    assert np.array_equal(got, (slots[0] * slots[1]) % np.uint64(t))


def test_refusals(gpu_pkg, oracle):
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P = c["N"], c["Q"], c["P"]
    nQ, nP = len(Q), len(P)
    cQ, cP, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, Q)

    def code(f, *args, **kw):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args, **kw)
        return e.value.code
    ARG, SHAPE = 4, 3
    # creation
    assert code(ring.BfvEncryptor, cQ, cP, 0) == ARG and code(ring.BfvEncryptor, cQ, cP, 65536) == ARG                  # max_batch outside 1 .. 65535
    assert code(ring.BfvDecryptor, cQ, 0) == ARG and code(ring.BfvDecryptor, cQ, 65536) == ARG
    assert code(ring.BfvEncryptor, ring.NewContextWithParams(4, Q), None, 1) == ARG                                     # N < 8
    assert code(ring.BfvEncryptor, cQ, ring.NewContextWithParams(2 * N, P), 1) == ARG                                   # ctxP with another N
    if nat.device_count() > 1:
        assert code(ring.BfvEncryptor, cQ, ring.NewContextWithParams(N, P, device=1), 1) == ARG                         # ctxP on another device
    L = nat.lib()
    assert L.lr_bfv_encryptor_create(None, cP.h, 1, C.byref(C.c_void_p())) == ARG and L.lr_bfv_encryptor_create(cQ.h, cP.h, 1, None) == ARG
    assert L.lr_bfv_decryptor_create(None, 1, C.byref(C.c_void_p())) == ARG and L.lr_bfv_decryptor_create(cQ.h, 1, None) == ARG
    enc, dec = ring.BfvEncryptor(cQ, cP, 2), ring.BfvDecryptor(cQ, 2)
    qp = lambda ctx, batch: ring.Poly(ctx, nQ + nP, batch)
    pk, sk, crp, pt = (qp(cQ, 1), qp(cQ, 1)), qp(cQ, 1), qp(cQ, 2), cQ.NewPoly(2)
    ct = (cQ.NewPoly(2), cQ.NewPoly(2))
    u, e = (c["uc"][:2], c["us"][:2]), (c["e0"][:2], c["e1"][:2])
    # pk
    assert code(enc.EncryptPk, pk, u, e, pt, (ct[0], ct[0])) == ARG                                                      # out_c0 == out_c1
    assert code(enc.EncryptPk, (qp(other, 1), pk[1]), u, e, pt, ct) == ARG                                               # a poly of another context
    assert code(enc.EncryptPk, pk, u, e, other.NewPoly(2), ct) == ARG
    assert code(enc.EncryptPk, pk, u, e, pt, (ct[0], other.NewPoly(2))) == ARG
    assert code(enc.EncryptPk, (ring.Poly(cQ, nQ, 1), pk[1]), u, e, pt, ct) == SHAPE                                     # too few limbs for the form through P
    assert code(enc.EncryptPk, pk, u, e, pt, (ct[0], ring.Poly(cQ, nQ - 1, 2))) == SHAPE
    assert code(enc.EncryptPk, pk, u, e, cQ.NewPoly(3), ct) == SHAPE                                                     # batch differs from a poly's
    assert code(enc.EncryptPk, (qp(cQ, 3), pk[1]), u, e, pt, ct) == SHAPE
    three = (cQ.NewPoly(3), cQ.NewPoly(3))
    assert code(enc.EncryptPk, pk, (c["uc"], c["us"]), (c["e0"], c["e1"]), cQ.NewPoly(3), three) == SHAPE                # batch > max_batch
    assert code(enc.EncryptSk, sk, qp(cQ, 3), c["e"], cQ.NewPoly(3), three) == SHAPE
    # sk
    assert code(enc.EncryptSk, sk, crp, c["e"][:2], pt, (ct[1], ct[1])) == ARG
    assert code(enc.EncryptSk, qp(other, 1), crp, c["e"][:2], pt, ct) == ARG
    assert code(enc.EncryptSk, sk, ring.Poly(cQ, nQ, 2), c["e"][:2], pt, ct) == SHAPE                                    # crp over Q alone, form through P
    assert code(enc.EncryptSk, sk, qp(cQ, 1), c["e"][:2], pt, ct) == SHAPE                                               # crp must have the batch
    # raw calls: NULL arguments and batch < 1
    b = np.zeros(64, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    h = lambda p: p.h
    pk_args = [enc.h, 0, h(pk[0]), h(pk[1]), b, b, b, b, h(pt), 2, h(ct[0]), h(ct[1])]
    sk_args = [enc.h, 0, h(sk), h(crp), b, h(pt), 2, h(ct[0]), h(ct[1])]
    for fn, args, skip in ((L.lr_bfv_encrypt_pk, pk_args, (1, 9)), (L.lr_bfv_encrypt_pk_device, pk_args, (1, 9)),
                           (L.lr_bfv_encrypt_sk, sk_args, (1, 6)), (L.lr_bfv_encrypt_sk_device, sk_args, (1, 6))):
        for i in range(len(args)):
            if i not in skip:
                assert fn(*[None if j == i else a for j, a in enumerate(args)]) == ARG, (fn.__name__, i)
        for bad in (0, -1):
            assert fn(*[bad if j == skip[1] else a for j, a in enumerate(args)]) == SHAPE, (fn.__name__, bad)
    # decrypt
    cts = [cQ.NewPoly(2), cQ.NewPoly(2)]
    arr = (C.c_void_p * 2)(cts[0].h.value, cts[1].h.value)
    assert L.lr_bfv_decrypt(dec.h, arr, -1, sk.h, pt.h, 2) == ARG                                                        # a negative degree
    assert L.lr_bfv_decrypt(None, arr, 1, sk.h, pt.h, 2) == ARG and L.lr_bfv_decrypt(dec.h, None, 1, sk.h, pt.h, 2) == ARG
    assert L.lr_bfv_decrypt(dec.h, arr, 1, None, pt.h, 2) == ARG and L.lr_bfv_decrypt(dec.h, arr, 1, sk.h, None, 2) == ARG
    assert L.lr_bfv_decrypt(dec.h, (C.c_void_p * 2)(cts[0].h.value, None), 1, sk.h, pt.h, 2) == ARG
    assert L.lr_bfv_decrypt(dec.h, arr, 1, sk.h, pt.h, 0) == SHAPE and L.lr_bfv_decrypt(dec.h, arr, 1, sk.h, pt.h, 3) == SHAPE
    assert code(dec.Decrypt, [cts[0], other.NewPoly(2)], sk, pt) == ARG
    assert code(dec.Decrypt, cts, qp(other, 1), pt) == ARG
    assert code(dec.Decrypt, cts, sk, other.NewPoly(2)) == ARG
    assert code(dec.Decrypt, [cts[0], cQ.NewPoly(1)], sk, pt) == SHAPE                                                   # batch differs
    assert code(dec.Decrypt, [cts[0], ring.Poly(cQ, nQ - 1, 2)], sk, pt) == SHAPE                                        # too few limbs
    assert code(dec.Decrypt, cts, ring.Poly(cQ, nQ - 1, 1), pt) == SHAPE
    # the handles stay usable after their refusals
    sk.set(c["sk"][:1])
    pk[0].set(c["pk0"][:1])
    pk[1].set(c["pk1"][:1])
    pt1 = cQ.NewPoly(1).set(c["pt"][:1])
    enc.EncryptPk(pk, u, e, pt1, ct)
    want = c["want"][("pk", False, True)]
    got = [p.get() for p in ct]
    for bi in range(2):
        assert np.array_equal(got[0][bi], want[bi][0]) and np.array_equal(got[1][bi], want[bi][1])

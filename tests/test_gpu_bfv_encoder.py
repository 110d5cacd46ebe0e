"""bfv.Encoder on the device (lr_bfv_encoder, ring.BfvEncoder) against its line-by-line restatement (tests/bfv_encoder_ref.py), bit for bit:
EncodeUint / EncodeInt / DecodeUint / DecodeInt for batches of plaintexts on the fused route (N = 2^12, 2^13, 2^15 with t < 2^31) and on the
composed one (N = 2^16, N = 2^4, a 40-bit t), for 1, 2 and 6 limbs of Q, partially filled slot vectors, values outside [0, t) and the
centring boundary; both routes through the option field and the environment override; the tables; the device-pointer entry points; the
round trip; Mul of two encodings; every refusal."""
import ctypes as C

import numpy as np
import pytest

import bfv_encoder_ref as ref

pytestmark = pytest.mark.gpu

T40 = 1099512938497          # GenerateNTTPrimes(40, 16, 1)[0]


def _Q(pkg, spec):
    """'qi60:k' = the first k primes of Qi60 (1 mod 2^18: every N here); a BFV parameter set's name = its Q (1 mod 2 N of the set)"""
    if spec.startswith("qi60:"):
        return list(pkg.params.Qi60()[:int(spec[5:])])
    return list(pkg.params.bfv_moduli(spec)[1])


# (logN, Q, t, fused): |Q| in {1, 2, 6}; 2^15 is the LDS limit of the fused kernels, 2^11 their lower bound.  Every pair keeps t^2 far below
# Q: decode rounds t / Q * floor(Q / t) m = m - m (Q mod t) / Q, which is m only while m t < Q / 2 (a one-limb Q takes t up to 2^20 or so)
CASES = [
    (12, "PN12QP109", 65537, True), (12, "qi60:1", 40961, True), (12, "PN14QP438", 786433, True), (12, "PN12QP109", 0x3ee0001, True),
    (12, "qi60:2", 2013265921, True), (13, "PN14QP438", 65537, True), (13, "qi60:2", 2013265921, True), (13, "qi60:1", 786433, True),
    (15, "qi60:6", 65537, True), (15, "qi60:2", 2013265921, True), (15, "qi60:1", 786433, True), (15, "qi60:2", 0x3ee0001, True),
    (16, "qi60:2", 786433, False), (4, "qi60:2", 65537, False), (12, "qi60:2", T40, False),
]
IDS = ["N%d-%s-t%d" % (c[0], c[1].replace(":", ""), c[2]) for c in CASES]

_refs, _pts = {}, {}


def _ref(oracle, pkg, logn, qspec, t):
    key = (logn, qspec, t)
    if key not in _refs:
        _refs[key] = ref.Encoder(oracle, 1 << logn, _Q(pkg, qspec), t)
    return _refs[key]


def _uints(t, N, n, b):
    """slot values of batch element b: random below t; element 1 all t - 1; element 2 at and above t, up to 2^64 - 1"""
    rng = np.random.default_rng(1000 * n + b)
    v = rng.integers(0, t, size=n, dtype=np.uint64)
    if b == 1:
        v[:] = t - 1
    if b == 2:
        v = v + np.uint64(t) * rng.integers(1, 1 << 20, size=n, dtype=np.uint64)
        v[:3] = np.array([t, 2**64 - 1, 2 * t - 1], dtype=np.uint64)[:n]
    return v


def _ints(t, N, n, b):
    """centred values; the first slots are -1, -(t - 1) / 2, t >> 1 and (t >> 1) + 1 -- the last two the centring boundary of DecodeInt"""
    rng = np.random.default_rng(2000 * n + b)
    v = rng.integers(-(t // 2), t // 2 + 1, size=n, dtype=np.int64)
    edge = np.array([-1, -(t - 1) // 2, t >> 1, (t >> 1) + 1, -t, 1 - t], dtype=np.int64)
    v[:len(edge)] = edge[:n]
    return v


def _want(oracle, pkg, case, kind, n, b):
    """(plaintext, decoded slots) of the restatement, computed once per (case, kind, n_values, batch element)"""
    logn, qspec, t, _ = case
    key = (logn, qspec, t, kind, n, b)
    if key not in _pts:
        r = _ref(oracle, pkg, logn, qspec, t)
        if kind == "uint":
            pt = r.encode_uint(_uints(t, 1 << logn, n, b))
            _pts[key] = (pt, r.decode_uint(pt))
        else:
            pt = r.encode_int(_ints(t, 1 << logn, n, b))
            _pts[key] = (pt, r.decode_int(pt))
    return _pts[key]


def _elem(p, b):
    return np.stack(p.get_limb_slices(b))


def _n_values(N):
    return sorted({0, 1, N // 2 + 1, N})


def _check(oracle, pkg, case, enc, cQ, batch, n_list):
    logn, qspec, t, _ = case
    N = 1 << logn
    for n in n_list:
        for kind, gen, encode, decode in (("uint", _uints, enc.EncodeUint, enc.DecodeUint), ("int", _ints, enc.EncodeInt, enc.DecodeInt)):
            vals = np.stack([gen(t, N, n, b) for b in range(batch)]) if n else np.zeros((batch, 0), dtype=np.uint64 if kind == "uint" else np.int64)
            pt = encode(vals, cQ.NewPoly(batch))
            got = decode(pt)
            assert got.shape == (batch, N)
            for b in range(batch):
                want_pt, want_slots = _want(oracle, pkg, case, kind, n, b)
                assert np.array_equal(_elem(pt, b), want_pt), (kind, n, b)
                assert np.array_equal(got[b], want_slots), (kind, n, b)
                # the round trip: the residues of the values (centred for Int), a zero tail
                if kind == "uint":
                    back = vals[b] % np.uint64(t)
                else:
                    back = np.array([((int(x) + t // 2) % t) - t // 2 for x in vals[b]], dtype=np.int64)
                if t <= (1 << 40):
                    assert np.array_equal(got[b][:n], back) and not got[b][n:].any(), (kind, n, b)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_encode_and_decode_match_the_restatement(gpu_pkg, oracle, monkeypatch, case, batch):
    monkeypatch.delenv("LR_BFV_ENCODER_UNFUSED", raising=False)
    logn, qspec, t, fused = case
    N = 1 << logn
    ring = gpu_pkg.ring
    cQ = ring.NewContextWithParams(N, _Q(gpu_pkg, qspec))
    enc = ring.BfvEncoder(cQ, t, max_batch=3)
    assert enc.fused() == fused
    # every n_values at batch 3 (its elements 1 and 2 carry the special values); batch 1 checks the single-plaintext launch
    _check(oracle, gpu_pkg, case, enc, cQ, batch, _n_values(N) if batch == 3 or logn < 15 else [N // 2 + 1, N])


def test_centring_boundary_and_residues(gpu_pkg):
    """the explicit expectations, without the restatement: t >> 1 stays, (t >> 1) + 1 becomes negative, values at and above t wrap"""
    t, N = 65537, 1 << 12
    ring = gpu_pkg.ring
    cQ = ring.NewContextWithParams(N, _Q(gpu_pkg, "PN12QP109"))
    enc = ring.BfvEncoder(cQ, t)
    s = np.array([-1, -(t - 1) // 2, t >> 1, (t >> 1) + 1, -t, -2**63, 2**63 - 1], dtype=np.int64)
    got = enc.DecodeInt(enc.EncodeInt(s, cQ.NewPoly()))[0]
    centre = lambda x: ((x + t // 2) % t) - t // 2
    assert [int(x) for x in got[:7]] == [-1, -(t - 1) // 2, t >> 1, (t >> 1) + 1 - t, 0, centre(-2**63), centre(2**63 - 1)]
    u = np.array([t, t + 5, 2**64 - 1, t - 1], dtype=np.uint64)
    got = enc.DecodeUint(enc.EncodeUint(u, cQ.NewPoly()))[0]
    assert [int(x) for x in got[:4]] == [0, 5, (2**64 - 1) % t, t - 1] and not got[4:].any()


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[5], CASES[8]], ids=[IDS[0], IDS[4], IDS[5], IDS[8]])
def test_both_routes_give_the_same_bits(gpu_pkg, oracle, monkeypatch, case):
    """fused against composed, the latter through lr_options::bfv_encoder_unfused and through LR_BFV_ENCODER_UNFUSED"""
    monkeypatch.delenv("LR_BFV_ENCODER_UNFUSED", raising=False)
    logn, qspec, t, _ = case
    N, batch = 1 << logn, 3
    ring = gpu_pkg.ring
    cQ = ring.NewContextWithParams(N, _Q(gpu_pkg, qspec))
    fused = ring.BfvEncoder(cQ, t, batch)
    by_field = ring.BfvEncoder(cQ, t, batch, options=ring.Options(bfv_encoder_unfused=1))
    monkeypatch.setenv("LR_BFV_ENCODER_UNFUSED", "1")
    by_env = ring.BfvEncoder(cQ, t, batch)
    monkeypatch.delenv("LR_BFV_ENCODER_UNFUSED")
    assert fused.fused() and not by_field.fused() and not by_env.fused()
    n = N // 2 + 1
    u = np.stack([_uints(t, N, n, b) for b in range(batch)])
    s = np.stack([_ints(t, N, n, b) for b in range(batch)])
    pu, ps = fused.EncodeUint(u, cQ.NewPoly(batch)), fused.EncodeInt(s, cQ.NewPoly(batch))
    assert np.array_equal(_elem(pu, 0), _want(oracle, gpu_pkg, case, "uint", n, 0)[0])
    for other in (by_field, by_env):
        assert np.array_equal(other.EncodeUint(u, cQ.NewPoly(batch)).get(), pu.get())
        assert np.array_equal(other.EncodeInt(s, cQ.NewPoly(batch)).get(), ps.get())
        assert np.array_equal(other.DecodeUint(pu), fused.DecodeUint(pu))
        assert np.array_equal(other.DecodeInt(ps), fused.DecodeInt(ps))
    # decode of an arbitrary poly over Q (not an encoding): the routes still agree, and with the restatement
    x = gpu_pkg.sampling.uniform_poly(_Q(gpu_pkg, qspec), N, batch, seed=77).reshape(batch, -1, N)
    px = cQ.NewPoly(batch).set(x)
    want = _ref(oracle, gpu_pkg, logn, qspec, t).decode_int(x[2])
    assert np.array_equal(fused.DecodeInt(px)[2], want) and np.array_equal(by_field.DecodeInt(px)[2], want)


@pytest.mark.parametrize("case", [CASES[2], CASES[8], CASES[13], CASES[14]], ids=[IDS[2], IDS[8], IDS[13], IDS[14]])
def test_tables(gpu_pkg, oracle, case):
    logn, qspec, t, _ = case
    Q = _Q(gpu_pkg, qspec)
    cQ = gpu_pkg.ring.NewContextWithParams(1 << logn, Q)
    index, delta = gpu_pkg.ring.BfvEncoder(cQ, t).tables()
    assert np.array_equal(index, ref.index_matrix(1 << logn))
    assert np.array_equal(delta, ref.delta_mont(oracle, Q, t))


@pytest.mark.parametrize("case", [CASES[0], CASES[14]], ids=[IDS[0], IDS[14]])
def test_device_pointer_entry_points(gpu_pkg, case):
    """slots in device memory (here: one-limb polys used as plain buffers of [batch][N] words) against the host-value calls"""
    logn, qspec, t, _ = case
    N, batch = 1 << logn, 3
    ring = gpu_pkg.ring
    cQ = ring.NewContextWithParams(N, _Q(gpu_pkg, qspec))
    enc = ring.BfvEncoder(cQ, t, batch)
    for signed, vals in ((False, np.stack([_uints(t, N, N, b) for b in range(batch)])), (True, np.stack([_ints(t, N, N, b) for b in range(batch)]))):
        src, dst = ring.Poly(cQ, 1, batch), ring.Poly(cQ, 1, batch)
        src.set(vals.view(np.uint64).reshape(batch, 1, N))
        pt_host = (enc.EncodeInt if signed else enc.EncodeUint)(vals, cQ.NewPoly(batch))
        pt_dev = enc.EncodeDevice(src.device_ptr, N, batch, signed, cQ.NewPoly(batch))
        assert np.array_equal(pt_dev.get(), pt_host.get())
        enc.DecodeDevice(pt_dev, signed, dst.device_ptr)
        cQ.Sync()
        got = dst.get().reshape(batch, N)
        want = (enc.DecodeInt if signed else enc.DecodeUint)(pt_host)
        assert np.array_equal(got.view(want.dtype), want)
    # a partially filled vector: [batch][n_values] is dense
    n = 5
    vals = np.stack([_uints(t, N, n, b) for b in range(batch)])
    src = ring.Poly(cQ, 1, 1)
    flat = np.zeros(N, dtype=np.uint64)
    flat[:batch * n] = vals.reshape(-1)
    src.set(flat.reshape(1, 1, N))
    assert np.array_equal(enc.EncodeDevice(src.device_ptr, n, batch, False, cQ.NewPoly(batch)).get(), enc.EncodeUint(vals, cQ.NewPoly(batch)).get())


def test_product_of_two_encodings_at_pn12qp109(gpu_pkg):
    """encode a and b, the degree-1 ciphertexts (pt, 0), BfvPlan.Mul, decode component 0: a o b modulo t; components 1 and 2 are zero"""
    t = 65537
    N, Q, _, QMul = gpu_pkg.params.bfv_moduli("PN12QP109")
    ring = gpu_pkg.ring
    cQ, cM = ring.NewContextWithParams(N, list(Q)), ring.NewContextWithParams(N, list(QMul))
    batch = 2
    enc, plan = ring.BfvEncoder(cQ, t, batch), ring.BfvPlan(cQ, cM, t, batch)
    rng = np.random.default_rng(91)
    a = rng.integers(0, t, size=(batch, N), dtype=np.uint64)
    b = rng.integers(0, t, size=(batch, N), dtype=np.uint64)
    zero = lambda: cQ.NewPoly(batch)
    ct0 = [enc.EncodeUint(a, cQ.NewPoly(batch)), zero()]
    ct1 = [enc.EncodeUint(b, cQ.NewPoly(batch)), zero()]
    out = [cQ.NewPoly(batch) for _ in range(3)]
    plan.Mul(ct0, ct1, out)
    assert np.array_equal(enc.DecodeUint(out[0]), (a * b) % np.uint64(t))
    assert not out[1].get().any() and not out[2].get().any()


def test_refusals(gpu_pkg):
    t, N = 65537, 1 << 12
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    Q = _Q(gpu_pkg, "PN12QP109")
    cQ, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, Q)

    def err(f, *args):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args)
        return e.value
    # a t that does not allow an NTT at N: lr_context_create's code and message
    want = err(ring.NewContextWithParams, N, [17])
    got = err(ring.BfvEncoder, cQ, 17)
    assert got.code == want.code == 2 and str(got) == str(want)
    assert err(ring.BfvEncoder, cQ, 0).code == 4
    assert err(ring.BfvEncoder, cQ, t, 0).code == 4
    enc = ring.BfvEncoder(cQ, t, max_batch=2)
    one = np.zeros((1, 4), dtype=np.uint64)
    assert err(enc.EncodeUint, np.zeros((1, N + 1), dtype=np.uint64), cQ.NewPoly()).code == 3      # n_values > N
    assert err(enc.EncodeInt, np.zeros((1, N + 1), dtype=np.int64), cQ.NewPoly()).code == 3
    assert err(enc.EncodeUint, one, cQ.NewPoly(2)).code == 3                                        # batch != the poly's
    assert err(enc.EncodeUint, np.zeros((3, 4), dtype=np.uint64), cQ.NewPoly(3)).code == 3          # batch > max_batch
    assert err(enc.DecodeUint, cQ.NewPoly(3)).code == 3
    assert err(enc.EncodeUint, one, other.NewPoly()).code == 4                                      # a poly of another context
    assert err(enc.DecodeInt, other.NewPoly()).code == 4
    assert err(enc.EncodeUint, one, ring.Poly(cQ, len(Q) - 1, 1)).code == 3                         # fewer than |Q| limbs
    assert err(enc.DecodeUint, ring.Poly(cQ, len(Q) - 1, 1)).code == 3
    L, pt = nat.lib(), cQ.NewPoly()
    buf = np.zeros(N, dtype=np.uint64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.lr_bfv_encode_uint(None, ptr, 4, 1, pt.h), L.lr_bfv_encode_uint(enc.h, None, 4, 1, pt.h), L.lr_bfv_encode_int(enc.h, ptr, 4, 1, None),
               L.lr_bfv_decode_uint(enc.h, None, 1, ptr), L.lr_bfv_decode_int(enc.h, pt.h, 1, None), L.lr_bfv_encode_device(enc.h, None, 4, 1, 0, pt.h),
               L.lr_bfv_decode_device(enc.h, pt.h, 1, 0, None), L.lr_bfv_encoder_tables(enc.h, None, None),
               L.lr_bfv_encoder_create(None, t, 1, C.byref(C.c_void_p())), L.lr_bfv_encoder_create(cQ.h, t, 1, None)):
        assert rc == 4
    # the handle stays usable after its refusals
    v = np.arange(8, dtype=np.uint64)
    assert np.array_equal(enc.DecodeUint(enc.EncodeUint(v, pt))[0][:8], v)
